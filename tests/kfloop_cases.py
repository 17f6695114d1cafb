"""Seeded scenes for the second stage of the visual loop closure, shared by tests/test_keyframe_loop_reference.py and tests/test_keyframe_loop.py. No images: the key
frames go in through add_loaded with hand-made descriptors, so the match set of every old key frame is chosen exactly (a matched window point's descriptor is
repeated among the old key points; every other descriptor is random, and random 256-bit words lie about 128 bits apart, far above the acceptance distance of 80:
`load` checks the match set it meant against the first stage's restatement)."""
import numpy as np

QIC = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])         # camera z forward along body x
TIC = np.array([0.05, -0.02, 0.1])
FOCAL = 460.0


def rot(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    th = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def camera_of(vio_R, vio_T, qic, tic):
    """world -> camera (R, t) of a body pose"""
    Rwc, Twc = vio_R @ qic, vio_T + vio_R @ tic
    return Rwc.T, -Rwc.T @ Twc


def descriptors(rng, n):
    return rng.integers(0, 1 << 63, (n, 4), dtype=np.int64).astype(np.uint64) * np.uint64(2) + rng.integers(0, 2, (n, 4)).astype(np.uint64)


def scene(seed, n_window, olds, identity=False, same_point=False, zero_depth=0, n_extra=7):
    """cur with n_window window points and one old key frame per entry of `olds`: dict(m, outliers (share or count), deg, trans, noise (pixels at f = 460; 0: none),
    yaw_only (the offset is a rotation about the world's z)). identity: cur's body pose, qic and tic are I and 0, so the guess is (I, 0) exactly. same_point: every
    world point is the same. zero_depth: that many members of the first old key frame get X_z = 0 (with identity: p_2 = 0 under the guess); they count as outliers.
    -> dict(cur, olds, qic, tic, point_id); an old entry names its members (window indices, ascending = S order), which of them are true, and its true camera pose."""
    rng = np.random.default_rng(seed)
    qic, tic = (np.eye(3), np.zeros(3)) if identity else (QIC, TIC)
    vio_R = np.eye(3) if identity else rot([0, 0, 1], rng.uniform(-170, 170)) @ rot(rng.normal(size=3), 4.0)
    vio_T = np.zeros(3) if identity else rng.uniform(-30, 30, 3)
    Rc, tc = camera_of(vio_R, vio_T, qic, tic)
    z = rng.uniform(10.0, 25.0, n_window)
    pc = np.stack([z * rng.uniform(-0.45, 0.45, n_window), z * rng.uniform(-0.35, 0.35, n_window), z], axis=1)
    if same_point:
        pc[:] = pc[0]
    X = ((pc - tc) @ Rc).astype(np.float32)                                       # R^T (p - t)
    win_desc = descriptors(rng, n_window)
    cur = dict(keypoints=np.zeros((0, 2), dtype=np.float32), keypoints_norm=np.zeros((0, 2), dtype=np.float32), descriptors=np.zeros((0, 4), dtype=np.uint64),
               window_uv=(FOCAL * pc[:, :2] / pc[:, 2:3] + [320.0, 240.0]).astype(np.float32), window_descriptors=win_desc, point_3d=X, vio_R=vio_R, vio_T=vio_T)
    out = []
    for k, spec in enumerate(olds):
        m = int(spec["m"])
        members = np.sort(rng.choice(n_window, m, replace=False))
        axis = [0, 0, 1] if spec.get("yaw_only") else rng.normal(size=3)
        d = rng.normal(size=3)
        old_R = rot(axis, spec.get("deg", 0.0)) @ vio_R
        old_T = vio_T + spec.get("trans", 0.0) * d / np.linalg.norm(d)
        Ro, to = camera_of(old_R, old_T, qic, tic)
        Xm = X[members].astype(np.float64)
        if zero_depth and k == 0:
            assert identity
            Xm[:zero_depth, 2] = 0.0
            X[members[:zero_depth], 2] = 0.0
        p = Xm @ Ro.T + to
        true = p[:, 2] > 0.5
        with np.errstate(all="ignore"):
            u = p[:, :2] / p[:, 2:3] + rng.normal(size=(m, 2)) * (spec.get("noise", 1.0) / FOCAL)
        n_out = spec.get("outliers", 0)
        n_out = int(round(n_out * m)) if isinstance(n_out, float) else int(n_out)
        bad = rng.choice(m, n_out, replace=False)
        true[bad] = False
        if zero_depth and k == 0:
            true[:zero_depth] = False
        gross = ~true
        ang = rng.uniform(0, 2 * np.pi, m)
        u[gross] = np.nan_to_num(u[gross], nan=0.0, posinf=0.0, neginf=0.0).clip(-2, 2) + (rng.uniform(0.15, 0.6, m)[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1))[gross]
        u = u.astype(np.float32)
        extra = rng.uniform(-0.5, 0.5, (n_extra, 2)).astype(np.float32)
        order = rng.permutation(m + n_extra)                                      # the old key points in no particular order
        kn = np.concatenate([u, extra])[order]
        kd = np.concatenate([win_desc[members], descriptors(rng, n_extra)])[order]
        out.append(dict(keypoints=(FOCAL * kn + np.float32([320.0, 240.0])).astype(np.float32), keypoints_norm=kn, descriptors=kd, window_uv=np.zeros((0, 2), dtype=np.float32),
                        window_descriptors=np.zeros((0, 4), dtype=np.uint64), members=members, u=u, true=true, R_true=Ro, t_true=to, vio_R=old_R, vio_T=old_T))
    cur["point_3d"] = X
    return dict(cur=cur, olds=out, qic=qic, tic=tic, point_id=(np.arange(n_window) * 3 + 11).astype(np.int32))


def load(store, sc, check=None):
    """the scene's key frames into a store (the device's or the restatement's): the old ones first, then cur with its geometry -> (cur, [old indices]). With `check`
    (the restatement's store) the match sets are compared with the ones the scene meant."""
    first = len(store)
    olds = [store.add_loaded(o["keypoints"], o["keypoints_norm"], o["descriptors"], o["window_uv"], o["window_descriptors"]) for o in sc["olds"]]
    c = sc["cur"]
    cur = store.add_loaded(c["keypoints"], c["keypoints_norm"], c["descriptors"], c["window_uv"], c["window_descriptors"])
    store.set_geometry(cur, c["point_3d"], c["vio_R"], c["vio_T"])
    assert olds == list(range(first, first + len(olds))) and cur == first + len(olds)
    if check is not None:
        res = check.searchByBRIEFDes(cur, olds)
        for i, o in enumerate(sc["olds"]):
            assert np.array_equal(np.flatnonzero(res["status"][i]), o["members"]), "the scene's match set"
            assert np.array_equal(res["pt_old_norm"][i][o["members"]].view(np.uint32), o["u"].view(np.uint32))
    return cur, olds
