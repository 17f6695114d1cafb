"""Synthetic cases of the camera-IMU rotation calibration: a ground-truth ric (about 30 degrees about a skew axis), IMU rotations of 5-20 degrees per frame about
axes that change from frame to frame, the camera rotation ric^T R_imu ric with a small translation, 40 points at 3-10 m, no noise."""
import numpy as np

RIC_AXIS, RIC_DEG = np.array([0.4, -0.7, 0.59]), 30.0


def rot(axis, deg):
    """Rodrigues"""
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.linalg.norm(k)
    th = np.deg2rad(deg)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def quat_xyzw(axis, deg):
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.linalg.norm(k)
    h = np.deg2rad(deg) / 2
    return np.array([k[0] * np.sin(h), k[1] * np.sin(h), k[2] * np.sin(h), np.cos(h)])


def ric_true():
    return rot(RIC_AXIS, RIC_DEG)


def angle_between(Ra, Rb):
    """the angle of Ra^T Rb in degrees"""
    c = (np.trace(Ra.T @ Rb) - 1.0) / 2.0
    return float(np.rad2deg(np.arccos(np.clip(c, -1.0, 1.0))))


def imu_rotation(rng, deg=None, axis=None):
    """(axis, degrees) of one frame-to-frame IMU rotation"""
    if axis is None:
        axis = rng.normal(size=3)
    if deg is None:
        deg = rng.uniform(5.0, 20.0)
    return np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis), float(deg)


def points_pair(rng, Rc, m, trans=0.05):
    """m points at 3-10 m in the older camera and their images in both: Rc = the newer camera's rotation in the older one's frame, p its position.
    -> (a [m][2], b [m][2])"""
    z = rng.uniform(3.0, 10.0, size=m)
    X = np.stack([rng.uniform(-0.4, 0.4, size=m) * z, rng.uniform(-0.4, 0.4, size=m) * z, z], axis=1)
    p = rng.normal(size=3)
    p = trans * p / np.linalg.norm(p)
    Xb = (X - p) @ Rc            # rows: Rc^T (X - p)
    assert (Xb[:, 2] > 0.5).all()
    return X[:, :2] / X[:, 2:3], Xb[:, :2] / Xb[:, 2:3]


def make_pushes(seed, n_pushes, m=40, one_axis=False, deg=None, ric=None):
    """-> list of dict(a, b, dq, Rimu, Rc): the pairs of n_pushes consecutive frames. m may be a list (per push). one_axis: every IMU rotation about the same axis"""
    rng = np.random.default_rng(seed)
    ric = ric_true() if ric is None else ric
    fixed = rng.normal(size=3)
    ms = list(m) if np.ndim(m) else [int(m)] * n_pushes
    out = []
    for i in range(n_pushes):
        axis, d = imu_rotation(rng, deg=deg, axis=fixed if one_axis else None)
        Rimu = rot(axis, d)
        Rc = ric.T @ Rimu @ ric
        a, b = points_pair(rng, Rc, ms[i])
        out.append(dict(a=a, b=b, dq=quat_xyzw(axis, d), Rimu=Rimu, Rc=Rc, axis=axis, deg=d))
    return out


def make_images(seed, n_frames, m=40, samples=20, dt=0.005):
    """hand-built inputs of a SlidingWindowEstimator: per frame k the image dict (feature id -> the 8 numbers of a feature point) and the IMU samples since the
    frame before. The features of the pair (k - 1, k) live for exactly these two frames, so getCorresponding(k - 1, k) returns them and nothing else.
    -> dict(images, stamps, imu: per frame a list of (dt, acc, gyr), pushes)"""
    pushes = make_pushes(seed, n_frames - 1, m)
    images = [dict() for _ in range(n_frames)]
    for k, pr in enumerate(pushes):                      # the pair (k, k + 1); ids ascending in k, so the feature order is the pair's order
        for j in range(m):
            fid = k * m + j
            images[k][fid] = np.array([pr["a"][j, 0], pr["a"][j, 1], 1.0, 0.0, 0.0, 0.0, 0.0, -1.0])
            images[k + 1][fid] = np.array([pr["b"][j, 0], pr["b"][j, 1], 1.0, 0.0, 0.0, 0.0, 0.0, -1.0])
    # a constant rate about the pair's axis that integrates to its angle. The mid-point rule averages a sample with the one before it, so every frame ends with a
    # sample of no duration that carries the next frame's rate: no step mixes two rates
    acc = np.array([0.0, 0.0, 9.81])
    rates = [pr["axis"] * np.deg2rad(pr["deg"]) / (samples * dt) for pr in pushes]
    imu = [[(dt, acc.copy(), rates[0].copy())]]
    for k, w in enumerate(rates):
        imu.append([(dt, acc.copy(), w.copy()) for _ in range(samples)] + ([(0.0, acc.copy(), rates[k + 1].copy())] if k + 1 < len(rates) else []))
    return dict(images=images, stamps=[0.1 * k for k in range(n_frames)], imu=imu, pushes=pushes)
