"""Starts and scenes for the tests of GlobalSFM's full bundle adjustment (test_startup_ba.py): the windows of sfm_cases with a start for the BA that does not come
from the chain (ground truth, perturbed), so that every size and edge can be driven directly, and the scenes of the verdict's cases."""
import numpy as np
import sfm_cases as sc


def truth_start(s, state=None):
    """the ground truth of a chain_scene in the BA's convention: c_R[k] = Q[k]^T, c_t[k] = -Q[k]^T T[k]; members = the features with two observations or more"""
    Q, T = np.asarray(s["Q"]), np.asarray(s["T"])
    R = np.array([q.T for q in Q])
    t = np.array([-(q.T @ p) for q, p in zip(Q, T)])
    R[s["l"]], t[s["l"]] = np.eye(3), np.zeros(3)
    nobs = np.diff(np.asarray(s["win"]["first_obs"]))
    st = (nobs >= 2).astype(np.uint8) if state is None else (np.asarray(state, dtype=np.uint8) & (nobs >= 2))
    return dict(l=int(s["l"]), R=R, t=t, state=st, positions=np.where(st[:, None] != 0, np.asarray(s["X"], dtype=np.float64), 0.0), chain_ok=True)


def perturbed(start, seed, rot_deg=0.0, pos=0.0, pt_rel=0.0):
    """the free poses turned by up to rot_deg about a random axis and moved by up to pos (baselines), the members moved by up to pt_rel of their distance; what the
    BA holds constant stays as it is"""
    rng = np.random.default_rng(seed)
    out = dict(start, R=start["R"].copy(), t=start["t"].copy(), positions=start["positions"].copy())
    nf, l = len(out["R"]), start["l"]
    for k in range(nf):
        if k == l:
            continue
        if rot_deg > 0:
            out["R"][k] = sc.rot(rng.normal(0, 1, 3), rng.uniform(0.5, 1.0) * rot_deg) @ out["R"][k]
        if pos > 0 and k != nf - 1:
            out["t"][k] = out["t"][k] + rng.uniform(-1, 1, 3) * pos
    if pt_rel > 0:
        X = out["positions"]
        out["positions"] = X + rng.uniform(-1, 1, X.shape) * pt_rel * np.linalg.norm(X, axis=1, keepdims=True)
    return out


def scene(seed, n_frames=11, n=150, l=None, noise_px=0.1, n_full=None, **kw):
    return sc.chain_scene(seed, n_frames=n_frames, n=n, n_full=min(n, max(1, (2 * n) // 5)) if n_full is None else n_full, l=l, noise_px=noise_px, **kw)


def near(s, seed=7, state=None):
    """the start every size test uses: 0.3 deg, 0.01 baselines, 1 % off the truth"""
    return perturbed(truth_start(s, state), seed, rot_deg=0.3, pos=0.01, pt_rel=0.01)


def far(s, seed=9):
    """far enough that the first steps are rejected and lambda rises: 8 deg, 0.3 baselines, 30 %"""
    return perturbed(truth_start(s), seed, rot_deg=8.0, pos=0.3, pt_rel=0.3)


def interleaved_state(n):
    """every third feature is no member"""
    st = np.ones(n, dtype=np.uint8)
    st[1::3] = 0
    return st


def two_frame_tracks(seed, n_frames=11, n=120, l=5):
    """every second feature is seen in exactly two neighbouring frames"""
    s = scene(seed, n_frames=n_frames, n=n, l=l)
    rng = np.random.default_rng(seed + 1)
    start, end = s["start"].copy(), s["end"].copy()
    a = rng.integers(0, n_frames - 1, n)
    start[::2], end[::2] = a[::2], a[::2] + 1
    s["win"] = sc.make_window(s["X0"], s["poses"], start, end, np.random.default_rng(seed + 2), 0.1)
    s["start"], s["end"] = start, end
    return s


def lonely_frame(seed, n_frames=6, n=80, l=3):
    """frame 0 is seen by two features only; all others start at frame 1 or later"""
    s = scene(seed, n_frames=n_frames, n=n, l=l)
    start, end = np.maximum(s["start"], 1), np.maximum(s["end"], 2)
    start[[3, 40]], end[[3, 40]] = 0, n_frames - 1
    s["win"] = sc.make_window(s["X0"], s["poses"], start, end, np.random.default_rng(seed + 2), 0.1)
    s["start"], s["end"] = start, end
    return s


def behind_the_camera(seed=6100):
    """a member that lies in the plane z = 0 of the camera of l: p_2 = 0 there, the residual is not a number"""
    s = scene(seed, n_frames=4, n=40, l=1, n_full=40)
    st = truth_start(s)
    st["positions"][5, 2] = 0.0
    return s, st


def same_centre(seed=6200, on_axis=False):
    """frames 0 and 1 share their centre (on_axis: their whole pose), and feature 0 is seen in these two only: two identical rays, no parallax, its V has rank 2.
    Off the axis the damping keeps V solvable. on_axis puts the point on the optical axis of both: the third pivot of its V is 0 at any lambda, every step is
    rejected by the pivot rule."""
    rng = np.random.default_rng(seed)
    n, nf = 60, 5
    poses = sc.path(rng, nf)
    poses[1] = (poses[0][0] if on_axis else poses[0][0] @ sc.rot([0.1, 1.0, 0.0], 1.5), poses[0][1].copy())
    X = sc.points3d(rng, n)
    if on_axis:
        X[0] = [0.0, 0.0, 20.0]
    start, end = np.zeros(n, dtype=np.int32), np.full(n, nf - 1, dtype=np.int32)
    end[0] = 1
    win = sc.make_window(X, poses, start, end, rng, 0.0)
    rel_R, rel_T, Q, T, Xl = sc.truth(X, poses, 0)
    s = dict(win=win, l=0, rel_R=rel_R, rel_T=rel_T, Q=Q, T=T, X=Xl, start=start, end=end, poses=poses, X0=X)
    return s, truth_start(s)
