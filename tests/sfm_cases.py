"""Scenes for the tests of GlobalSFM's frame chain (test_startup_sfm.py): windows built from 3-D points and a camera path, with their ground truth in the
frame of l at the scale relative_T fixes (|relative_T| = 1, the first stage's convention)."""
import numpy as np

FOCAL = 460.0
RT_AXIS, T_DIR = np.array([0.2, 1.0, 0.1]), np.array([1.0, 0.1, 0.2]) / np.linalg.norm([1.0, 0.1, 0.2])


def rot(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    th = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def points3d(rng, n, planar=False):
    """n points in front of camera 0, depth 5 - 50 m"""
    z = rng.uniform(5.0, 50.0, n)
    x, y = rng.uniform(-0.6, 0.6, n), rng.uniform(-0.4, 0.4, n)
    if planar:
        z = 12.0 + 3.0 * x + 2.0 * y
    return np.stack([x * z, y * z, z], axis=1)


def make_window(X, poses, start=None, end=None, rng=None, noise_px=0.0):
    """the feature table of the points X seen from the cameras poses[k] = (R, c) (orientation and position in the frame of camera 0), feature f visible in the
    frames start[f] .. end[f]; end[f] < start[f]: no observation at all"""
    n, nf = len(X), len(poses)
    start = np.zeros(n, dtype=np.int32) if start is None else np.asarray(start, dtype=np.int32)
    end = np.full(n, nf - 1, dtype=np.int32) if end is None else np.asarray(end, dtype=np.int32)
    first, pts = [0], []
    for f in range(n):
        for k in range(start[f], end[f] + 1):
            R, c = poses[k]
            pc = R.T @ (X[f] - c)
            assert pc[2] > 0.5, ("a point behind or at a camera that sees it", f, k, pc)
            p = pc[:2] / pc[2]
            if noise_px > 0:
                p = p + rng.normal(0, noise_px / FOCAL, 2)
            pts.append(p)
        first.append(len(pts))
    return dict(n_frames=nf, start_frame=start, first_obs=np.array(first, dtype=np.int32), pts=np.array(pts, dtype=np.float64).reshape(-1, 2))


def path(rng, n_frames, deg=(1.0, 2.0), step=(0.3, 0.5)):
    """a camera that turns deg[0] .. deg[1] degrees and moves step[0] .. step[1] metres per frame"""
    poses, R, c = [(np.eye(3), np.zeros(3))], np.eye(3), np.zeros(3)
    for _ in range(n_frames - 1):
        R = R @ rot(RT_AXIS + rng.normal(0, 0.1, 3), rng.uniform(*deg))
        c = c + rng.uniform(*step) * (T_DIR + rng.normal(0, 0.05, 3))
        poses.append((R, c.copy()))
    return poses


def truth(X, poses, l):
    """-> (relative_R, relative_T, Q [nf][3][3], T [nf][3], points [n][3]) in the frame of l, the baseline (l, newest) the unit of length"""
    Rl, cl = poses[l]
    Rn, cn = poses[-1]
    s = 1.0 / np.linalg.norm(cn - cl)
    Q = np.array([Rl.T @ R for R, _ in poses])
    T = np.array([s * (Rl.T @ (c - cl)) for _, c in poses])
    return Rl.T @ Rn, s * (Rl.T @ (cn - cl)), Q, T, s * ((X - cl) @ Rl)


def tracks(rng, n, n_full, n_frames):
    """start / end per feature: n_full full-length tracks, the rest with a random start and end (at least two frames), interleaved"""
    start, end = np.zeros(n, dtype=np.int32), np.full(n, n_frames - 1, dtype=np.int32)
    for f in range(n_full, n):
        a, b = sorted(rng.integers(0, n_frames, 2))
        if a == b:
            a, b = (a - 1, b) if a > 0 else (a, b + 1)
        start[f], end[f] = a, b
    order = rng.permutation(n)
    return start[order], end[order]


def chain_scene(seed, n_frames=11, n=150, n_full=60, noise_px=0.0, l=None, deg=(1.0, 2.0), step=(0.3, 0.5), planar=False):
    """-> dict(win, l, rel_R, rel_T, Q, T, X, start, end, poses, X0): a window with mixed tracks and its ground truth; X0 = the points in the frame of camera 0"""
    rng = np.random.default_rng(seed)
    X = points3d(rng, n, planar)
    poses = path(rng, n_frames, deg, step)
    start, end = tracks(rng, n, min(n_full, n), n_frames)
    win = make_window(X, poses, start, end, rng, noise_px)
    l = (n_frames - 1) // 2 if l is None else l
    rel_R, rel_T, Q, T, Xl = truth(X, poses, l)
    return dict(win=win, l=l, rel_R=rel_R, rel_T=rel_T, Q=Q, T=T, X=Xl, start=start, end=end, poses=poses, X0=X)


def rot_err_deg(R, Rt):
    """the angle of R^T Rt from its skew part and its trace (atan2: exact for small angles, where arccos of the trace alone resolves 1e-6 degrees at best)"""
    D = R.T @ Rt
    v = 0.5 * np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.rad2deg(np.arctan2(np.linalg.norm(v), (np.trace(D) - 1) / 2)))
