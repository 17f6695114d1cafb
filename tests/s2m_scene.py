"""The small room the scan-to-map hook and host-state tests step through, and scans drawn from it."""
import numpy as np


def scene(seed):
    """a room: floor, two walls and four poles, one point per 0.8 m leaf at most after the filter"""
    rng = np.random.default_rng(seed)
    g = np.arange(-8.0, 8.01, 0.25)
    floor = np.array([[x, y, -1.5] for x in g for y in g])
    wall1 = np.array([[8.0, y, z] for y in g for z in np.arange(-1.5, 2.01, 0.25)])
    wall2 = np.array([[x, -8.0, z] for x in g for z in np.arange(-1.5, 2.01, 0.25)])
    surf = np.vstack([floor, wall1, wall2])
    poles = np.vstack([np.array([[px, py, z] for z in np.arange(-1.5, 2.5, 0.05)]) for px, py in ((3.0, 2.0), (-4.0, 5.0), (5.0, -5.0), (-3.0, -4.0))])
    f4 = lambda p: np.column_stack([p + rng.normal(0, 0.004, p.shape), np.ones(len(p))]).astype(np.float32)
    return f4(poles), f4(surf)


def scans(me, ms, count, seed=5, n_edge=150, n_surf=400):
    """`count` scans of n_edge edge and n_surf surf points drawn from the scene (me, ms), each shifted by a few centimetres"""
    rng = np.random.default_rng(seed)
    return [(np.ascontiguousarray(me[rng.choice(len(me), n_edge, replace=False)] + np.append(rng.normal(0, 0.02, 3), 0).astype(np.float32)),
             np.ascontiguousarray(ms[rng.choice(len(ms), n_surf, replace=False)] + np.append(rng.normal(0, 0.02, 3), 0).astype(np.float32))) for _ in range(count)]
