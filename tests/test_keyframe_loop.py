"""The second stage of the visual loop closure on the device (vilf_kf_set_geometry, vilf_kf_find_connection, estimator.KeyFrameStore.findConnection) against
tests/kfloop_reference.py, the numpy restatement of the contract in include/vilfusion.h. Counts, flags, masks and everything up to the pose out compare on integers
and float bits; the host's decision (libm against numpy) to 1e-12. The restatement itself is measured in tests/test_keyframe_loop_reference.py."""
import ctypes as C
import numpy as np
import pytest
import kf_reference as kr
import kfloop_reference as kl
import kfloop_cases as kc
from vil_fusion_amd import abi

pytestmark = pytest.mark.gpu
CAM = (460.0, 460.0, 320.0, 240.0, 0.0, 0.0, 0.0, 0.0)
PATTERN = kr.read_pattern()
EXACT = ("n_matched", "n_inliers", "best_k", "flags", "has_loop", "accepted")
BITS = ("R", "t", "PnP_R_old", "PnP_T_old", "cost0", "cost1")
CLOSE = ("relative_t", "relative_q", "relative_yaw")
INV = abi.VILF_ERR_INVALID_ARGUMENT


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


@pytest.fixture(scope="module")
def solver():
    from vil_fusion_amd.estimator import BackendSolver
    s = BackendSolver()
    yield s
    s.close()


def make(solver, cap_keyframes=8, cap_keypoints=8192):
    from vil_fusion_amd.estimator import KeyFrameStore
    return KeyFrameStore(solver, 64, 48, CAM, PATTERN, cap_keyframes=cap_keyframes, cap_keypoints=cap_keypoints), \
        kl.KeyFrameStore(64, 48, CAM, PATTERN, cap_keyframes=cap_keyframes, cap_keypoints=cap_keypoints)


def compare_row(got, want, what, exact=False):
    for k in EXACT:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in BITS:
        assert np.array_equal(bits(got[k]), bits(want[k])), (what, k, got[k], want[k])
    for k in CLOSE:
        if exact:
            assert np.array_equal(bits(got[k]), bits(want[k])), (what, k)
        else:
            assert np.abs(np.asarray(got[k]) - np.asarray(want[k])).max() <= 1e-12, (what, k, got[k], want[k])
    assert np.array_equal(got["status"], want["status"]) and got["status"].dtype == np.uint8, (what, np.flatnonzero(got["status"] != want["status"]))
    assert (got["loop_info"] is None) == (want["loop_info"] is None) == (not want["has_loop"]), what
    if want["loop_info"] is not None:
        assert got["loop_info"].shape == (8,) and np.abs(got["loop_info"] - want["loop_info"]).max() <= 1e-12, what
    if "match_points" in want:
        assert got["match_points"].dtype == np.float32 and got["match_points"].shape == want["match_points"].shape, what
        assert np.array_equal(got["match_points"].view(np.uint32), want["match_points"].view(np.uint32)), what


def both(solver, sc, olds=None, **params):
    """the scene through the device and the restatement -> (device rows, restatement rows)"""
    t, ref = make(solver)
    cur, idx = kc.load(t, sc)
    assert (cur, idx) == kc.load(ref, sc, check=ref)
    sel = idx if olds is None else [idx[i] for i in olds]
    got = t.findConnection(cur, sel, sc["qic"], sc["tic"], point_id=sc["point_id"], **params)
    want = ref.findConnection(cur, sel, sc["qic"], sc["tic"], point_id=sc["point_id"], **params)
    assert len(got) == len(want) == len(sel)
    for i, (g, w) in enumerate(zip(got, want)):
        compare_row(g, w, f"candidate {i}")
    return got, want


# ---- sizes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [25, 26, 63, 64, 65, 255, 256, 257, 1000])
def test_member_counts(solver, m):
    """the gate, a wave of the gather, the stride of the refit's partial sums and the score's chunk, VILF_MAX_FEATURES"""
    sc = kc.scene(100 + m, min(m + 13, abi.VILF_MAX_FEATURES), [dict(m=m, outliers=0.0 if m <= 26 else 0.3, deg=10.0, trans=2.0)])      # at the gate every member is true: 26 inliers close a loop
    got, want = both(solver, sc)
    w = want[0]
    print(m, {k: w[k] for k in EXACT}, w["relative_yaw"])
    assert w["n_matched"] == m
    if m == 25:
        assert w["flags"] == kl.GATE and not w["status"].any()
    else:
        assert w["flags"] == kl.REFIT | kl.LOOP and w["n_inliers"] == int(sc["olds"][0]["true"].sum()) and w["accepted"] > 0


@pytest.mark.parametrize("n_in", [255, 256, 257])
def test_inlier_counts(solver, n_in):
    """the inliers that the refit compacts into LDS: a full stride of 256, one below, one above"""
    sc = kc.scene(200 + n_in, 320, [dict(m=300, outliers=300 - n_in, deg=8.0, trans=1.5)])
    _, want = both(solver, sc)
    assert want[0]["n_inliers"] == n_in and want[0]["status"].sum() == n_in and want[0]["has_loop"]


@pytest.mark.parametrize("K", [1, 64, 65, 256])
def test_hypothesis_counts(solver, K):
    sc = kc.scene(300, 90, [dict(m=70, outliers=0.25, deg=12.0, trans=2.0)])
    _, want = both(solver, sc, n_hypotheses=K, seed=12345)
    assert 0 <= want[0]["best_k"] < K
    if K >= 64:
        assert want[0]["has_loop"]


def test_parameters_reach_the_kernels(solver):
    sc = kc.scene(301, 90, [dict(m=70, outliers=0.25, deg=12.0, trans=2.0)])
    a = both(solver, sc, n_hypotheses=64)[1][0]
    for over in (dict(seed=0xffffffff), dict(hyp_iterations=2), dict(refine_iterations=1), dict(lambda0=10.0), dict(reproj_threshold=1.0 / 460.0), dict(min_loop_num=69)):
        b = both(solver, sc, n_hypotheses=64, **over)[1][0]
        assert any(not np.array_equal(bits(a[k]), bits(b[k])) for k in BITS) or a["best_k"] != b["best_k"] or a["n_inliers"] != b["n_inliers"] or a["has_loop"] != b["has_loop"], over
    assert both(solver, sc, n_hypotheses=64, min_loop_num=70)[1][0]["flags"] == kl.GATE


# ---- several candidates ------------------------------------------------------------------------------------------------------------
def test_candidates_are_independent(solver):
    """three old key frames, the middle one below the gate; an index repeated; every row equals the row of a call with that candidate alone, to the bit"""
    sc = kc.scene(400, 120, [dict(m=70, outliers=0.3, deg=6.0, trans=1.0), dict(m=10, outliers=0, deg=6.0, trans=1.0), dict(m=90, outliers=0.2, deg=15.0, trans=3.0)])
    t, ref = make(solver)
    cur, idx = kc.load(t, sc)
    assert (cur, idx) == kc.load(ref, sc, check=ref)
    alone = {i: t.findConnection(cur, [i], sc["qic"], sc["tic"], point_id=sc["point_id"])[0] for i in idx}
    for i in idx:
        compare_row(alone[i], ref.findConnection(cur, [i], sc["qic"], sc["tic"], point_id=sc["point_id"])[0], f"alone {i}")
    assert alone[idx[0]]["has_loop"] and alone[idx[1]]["flags"] == kl.GATE and alone[idx[1]]["n_matched"] == 10 and alone[idx[2]]["has_loop"]
    assert alone[idx[0]]["best_k"] != alone[idx[2]]["best_k"] or not np.array_equal(alone[idx[0]]["R"], alone[idx[2]]["R"])
    for sel in ([idx[0], idx[1], idx[0]], [idx[2], idx[1], idx[0]]):
        rows = t.findConnection(cur, sel, sc["qic"], sc["tic"], point_id=sc["point_id"])
        for k, (i, r) in enumerate(zip(sel, rows)):
            compare_row(r, alone[i], f"call {sel}, row {k}", exact=True)


def test_ties_go_to_the_lowest_k(solver):
    sc = kc.scene(500, 60, [dict(m=50, outliers=0, noise=0.0, deg=3.0, trans=0.5)])
    _, want = both(solver, sc, n_hypotheses=64)
    o, c = sc["olds"][0], sc["cur"]
    X, u = c["point_3d"][o["members"]].astype(np.float64), o["u"].astype(np.float64)
    R, t = kl.hypotheses(X, u, kl.samples(50, 64, 0 + 0), *kl.guess(c["vio_R"], c["vio_T"], sc["qic"], sc["tic"]), 5, 1e-3)      # the old key frame is number 0: seed + 0
    score = kl.inliers(R, t, X, u, np.float64(10.0 / 460.0) ** 2).sum(axis=1)
    full = np.flatnonzero(score == 50)
    print("hypotheses with every member an inlier:", len(full))
    assert len(full) > 1 and want[0]["best_k"] == full[0] and want[0]["n_inliers"] == 50


# ---- degenerate input ---------------------------------------------------------------------------------------------------------------------
def test_equal_world_points(solver):
    """every X_j the same: H has rank 2 and only the damping keeps the pivots positive. Whatever the steps do, the hypotheses stay valid and the device follows the
    restatement bit for bit"""
    sc = kc.scene(600, 40, [dict(m=40, outliers=0, deg=2.0, trans=0.2)], same_point=True)
    _, want = both(solver, sc, n_hypotheses=64)
    w = want[0]
    assert w["best_k"] == 0 and w["flags"] & (kl.REFIT | kl.REFIT_DROPPED)
    print("equal points:", w["n_inliers"], w["accepted"], w["flags"])


def test_member_on_the_camera_plane_is_an_outlier(solver):
    sc = kc.scene(601, 70, [dict(m=60, outliers=0.2, deg=4.0, trans=0.5)], identity=True, zero_depth=3)
    _, want = both(solver, sc, n_hypotheses=128)
    o = sc["olds"][0]
    assert (sc["cur"]["point_3d"][o["members"][:3], 2] == 0).all()
    R0, t0 = kl.guess(sc["cur"]["vio_R"], sc["cur"]["vio_T"], sc["qic"], sc["tic"])
    assert np.array_equal(R0, np.eye(3)) and not t0.any()                        # p_2 = X_z = 0 under the guess
    assert not want[0]["status"][o["members"][:3]].any() and want[0]["has_loop"]
    S = kl.samples(60, 128, 0)
    assert (S < 3).any(), "some hypothesis draws a member with p_2 = 0"


def test_no_hypothesis_reaches_the_gate(solver):
    sc = kc.scene(602, 70, [dict(m=60, outliers=1.0, deg=4.0, trans=0.5)])
    _, want = both(solver, sc, n_hypotheses=64)
    w = want[0]
    print("all outliers:", w["n_inliers"], w["best_k"], w["flags"])
    assert w["best_k"] >= 0 and w["n_inliers"] <= 25 and not w["has_loop"] and w["flags"] in (kl.REFIT, kl.REFIT_DROPPED) and w["R"].any() and not w["relative_q"].any()


# ---- the decision --------------------------------------------------------------------------------------------------------------------------
def test_loop_refused_by_yaw_or_by_distance_alone(solver):
    sc = kc.scene(700, 80, [dict(m=60, outliers=0.2, deg=5.0, trans=1.0, yaw_only=True)])
    w = both(solver, sc, n_hypotheses=64)[1][0]
    assert w["has_loop"] and 4.0 < abs(w["relative_yaw"]) < 6.0 and 0.8 < np.linalg.norm(w["relative_t"]) < 1.2
    y = both(solver, sc, n_hypotheses=64, max_yaw=3.0)[1][0]
    assert not y["has_loop"] and y["flags"] == kl.REFIT and y["loop_info"] is None and y["n_inliers"] == w["n_inliers"] and y["relative_q"].any()
    d = both(solver, sc, n_hypotheses=64, max_dist=0.5)[1][0]
    assert not d["has_loop"] and d["flags"] == kl.REFIT and abs(d["relative_yaw"]) < 30.0


def test_python_outputs(solver):
    sc = kc.scene(701, 80, [dict(m=60, outliers=0.2, deg=5.0, trans=1.0)])
    got, want = both(solver, sc, n_hypotheses=64)
    g, o = got[0], sc["olds"][0]
    assert g["loop_info"].shape == (8,) and np.array_equal(g["loop_info"][:3], g["relative_t"]) and np.array_equal(g["loop_info"][3:7], g["relative_q"]) and g["loop_info"][7] == g["relative_yaw"]
    on = np.flatnonzero(g["status"])
    assert g["match_points"].shape == (len(on), 3) and np.array_equal(g["match_points"][:, 2], sc["point_id"][on].astype(np.float32))
    member = {int(w): k for k, w in enumerate(o["members"])}
    assert np.array_equal(g["match_points"][:, :2], o["u"][[member[int(w)] for w in on]])
    t, _ = make(solver)
    cur, idx = kc.load(t, sc)
    assert "match_points" not in t.findConnection(cur, idx, sc["qic"], sc["tic"], n_hypotheses=64)[0]
    assert list(t.loop_profile()) == ["gather", "hypotheses", "score", "refine", "download"]


def test_resetting_the_geometry(solver):
    sc = kc.scene(800, 80, [dict(m=60, outliers=0.2, deg=5.0, trans=1.0)])
    t, ref = make(solver)
    cur, idx = kc.load(t, sc)
    kc.load(ref, sc, check=ref)
    first = t.findConnection(cur, idx, sc["qic"], sc["tic"], n_hypotheses=64)[0]
    compare_row(first, ref.findConnection(cur, idx, sc["qic"], sc["tic"], n_hypotheses=64)[0], "first geometry")
    # the whole world moved and turned: other numbers, the same relative geometry
    A, b = kc.rot([0.2, -0.1, 1.0], 33.0), np.array([3.0, -7.0, 1.5])
    c = sc["cur"]
    X2, R2, T2 = (c["point_3d"].astype(np.float64) @ A.T + b).astype(np.float32), A @ c["vio_R"], A @ c["vio_T"] + b
    for s in (t, ref):
        s.set_geometry(cur, X2, R2, T2)
    second = t.findConnection(cur, idx, sc["qic"], sc["tic"], n_hypotheses=64)[0]
    compare_row(second, ref.findConnection(cur, idx, sc["qic"], sc["tic"], n_hypotheses=64)[0], "second geometry")
    assert not np.array_equal(first["R"], second["R"]) and second["has_loop"] and abs(second["relative_yaw"] - first["relative_yaw"]) < 0.5


# ---- invalid arguments ------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_leave_outputs_and_store_untouched(solver):
    from vil_fusion_amd.estimator import BackendSolver, kf_default_loop_params
    L, h = solver._L, solver._h
    sc = kc.scene(900, 50, [dict(m=40, outliers=0.2, deg=5.0, trans=1.0)])
    t, ref = make(solver)
    cur, idx = kc.load(t, sc)
    kc.load(ref, sc, check=ref)
    before = t.findConnection(cur, idx, sc["qic"], sc["tic"], n_hypotheses=64)[0]
    c = sc["cur"]
    X = np.ascontiguousarray(c["point_3d"], dtype=np.float32)
    vR, vT = np.ascontiguousarray(c["vio_R"].reshape(9)), np.ascontiguousarray(c["vio_T"])
    fp, dp = t._fp, abi.dptr
    # vilf_kf_set_geometry
    other = BackendSolver()
    try:
        assert other._L.vilf_kf_set_geometry(other._h, 0, fp(X), dp(vR), dp(vT)) == INV              # no store
        assert other._L.vilf_kf_find_connection(other._h, C.byref(kf_default_loop_params()), 0, 1, t._ip(np.zeros(1, dtype=np.int32)), (abi.KfLoopResult * 1)(), None, None) == INV
    finally:
        other.close()
    for index in (-1, len(t)):
        assert L.vilf_kf_set_geometry(h, index, fp(X), dp(vR), dp(vT)) == INV
    assert L.vilf_kf_set_geometry(h, cur, None, dp(vR), dp(vT)) == INV
    assert L.vilf_kf_set_geometry(h, cur, fp(X), None, dp(vT)) == INV
    assert L.vilf_kf_set_geometry(h, cur, fp(X), dp(vR), None) == INV
    for what, at, v in (("X", 7, np.nan), ("X", 3 * 50 - 1, np.inf), ("R", 4, np.nan), ("T", 2, -np.inf)):
        X2, R2, T2 = X.copy(), vR.copy(), vT.copy()
        {"X": X2.reshape(-1), "R": R2, "T": T2}[what][at] = v
        assert L.vilf_kf_set_geometry(h, cur, fp(X2), dp(R2), dp(T2)) == INV, (what, at)
    assert L.vilf_kf_set_geometry(h, idx[0], None, dp(vR), dp(vT)) == abi.VILF_OK                   # an old key frame has no window points: a null point_3d is fine
    compare_row(t.findConnection(cur, idx, sc["qic"], sc["tic"], n_hypotheses=64)[0], before, "after the refused geometries", exact=True)
    # vilf_kf_find_connection
    rows = (abi.KfLoopResult * 2)()
    C.memset(rows, 0x5a, C.sizeof(rows))
    image = bytes(rows)
    st, ptn = np.full(2 * 50, 9, dtype=np.uint8), np.full((2 * 50, 2), -3.0, dtype=np.float32)

    def call(p, cur_, olds, rows_=rows):
        o = np.array(list(olds) + [0], dtype=np.int32)
        return L.vilf_kf_find_connection(h, None if p is None else C.byref(p), cur_, len(olds), t._ip(o), rows_, t._u8(st), t._fp(ptn))

    good = kf_default_loop_params(sc["qic"], sc["tic"], n_hypotheses=64)
    for cur_, olds in ((len(t), idx), (-1, idx), (cur, [len(t)]), (cur, [-1]), (cur, []), (cur, [idx[0]] * (abi.VILF_KF_MAX_CANDIDATES + 1))):      # what vilf_kf_match refuses
        assert call(good, cur_, olds) == INV, (cur_, olds[:2])
    assert L.vilf_kf_find_connection(h, C.byref(good), cur, 1, None, rows, t._u8(st), t._fp(ptn)) == INV          # a null old_index
    assert call(None, cur, idx) == INV and call(good, cur, idx, None) == INV                                     # null parameters, null rows
    assert call(good, cur, idx) == abi.VILF_OK and bytes(rows) != image                                          # the same call, valid
    C.memset(rows, 0x5a, C.sizeof(rows))
    st[:], ptn[:] = 9, -3.0
    no_geo = t.add_loaded(c["keypoints"], c["keypoints_norm"], c["descriptors"], c["window_uv"], c["window_descriptors"])
    assert call(good, no_geo, idx) == INV                                                                         # cur without geometry
    nan, inf = float("nan"), float("inf")
    for over in (dict(n_hypotheses=0), dict(n_hypotheses=abi.VILF_TRACK_MAX_HYPOTHESES + 1), dict(hyp_iterations=0), dict(hyp_iterations=65), dict(refine_iterations=0),
                 dict(refine_iterations=65), dict(min_loop_num=4), dict(min_loop_num=-1), dict(lambda0=0.0), dict(lambda0=-1.0), dict(lambda0=nan), dict(lambda0=inf),
                 dict(reproj_threshold=0.0), dict(reproj_threshold=-0.1), dict(reproj_threshold=nan), dict(reproj_threshold=inf), dict(max_yaw=0.0), dict(max_yaw=nan),
                 dict(max_dist=0.0), dict(max_dist=-2.0), dict(max_dist=inf)):
        assert call(kf_default_loop_params(sc["qic"], sc["tic"], **over), cur, idx) == INV, over
    for field, at, v in (("qic", 4, nan), ("qic", 0, inf), ("tic", 2, nan), ("tic", 0, -inf)):
        p = kf_default_loop_params(sc["qic"], sc["tic"])
        getattr(p, field)[at] = v
        assert call(p, cur, idx) == INV, (field, at)
    assert bytes(rows) == image and (st == 9).all() and (ptn == -3.0).all()
    assert len(t) == no_geo + 1
    compare_row(t.findConnection(cur, idx, sc["qic"], sc["tic"], n_hypotheses=64)[0], before, "after the refused calls", exact=True)
    assert call(kf_default_loop_params(sc["qic"], sc["tic"], min_loop_num=5, n_hypotheses=1, hyp_iterations=64, refine_iterations=64), cur, idx) == abi.VILF_OK      # the ends of the ranges


def test_two_stores_on_two_handles(solver):
    from vil_fusion_amd.estimator import BackendSolver
    other = BackendSolver()
    try:
        sa = kc.scene(1000, 80, [dict(m=60, outliers=0.3, deg=5.0, trans=1.0)])
        sb = kc.scene(1001, 50, [dict(m=30, outliers=0.1, deg=9.0, trans=2.0)], identity=True)
        (a, ra), (b, rb) = make(solver), make(other)
        ca, ia = kc.load(a, sa)
        cb, ib = kc.load(b, sb)
        kc.load(ra, sa, check=ra), kc.load(rb, sb, check=rb)
        for _ in range(2):
            compare_row(a.findConnection(ca, ia, sa["qic"], sa["tic"], n_hypotheses=64)[0], ra.findConnection(ca, ia, sa["qic"], sa["tic"], n_hypotheses=64)[0], "first store")
            compare_row(b.findConnection(cb, ib, sb["qic"], sb["tic"], n_hypotheses=65, seed=9)[0], rb.findConnection(cb, ib, sb["qic"], sb["tic"], n_hypotheses=65, seed=9)[0], "second store")
    finally:
        other.close()


def test_profile_counts_only_while_profiling(solver):
    sc = kc.scene(1100, 80, [dict(m=60, outliers=0.2, deg=5.0, trans=1.0)])
    t, _ = make(solver)
    cur, idx = kc.load(t, sc)
    t.findConnection(cur, idx, sc["qic"], sc["tic"], n_hypotheses=64)
    assert all(cnt == 0 and ms == 0.0 for ms, cnt in t.loop_profile().values())
    match_before = t.profile()["match"][1]
    solver.set_profiling(True)
    try:
        t.findConnection(cur, idx, sc["qic"], sc["tic"], n_hypotheses=64)
        t.findConnection(cur, idx + idx, sc["qic"], sc["tic"], n_hypotheses=64)
        prof, match = t.loop_profile(), t.profile()["match"]
    finally:
        solver.set_profiling(False)
    print(prof)
    assert list(prof) == ["gather", "hypotheses", "score", "refine", "download"]
    assert all(ms >= 0.0 and cnt == 2 for ms, cnt in prof.values()), prof
    assert match[1] == match_before + 2                                           # the match of a findConnection is booked where vilf_kf_profile books a match
    t.findConnection(cur, idx, sc["qic"], sc["tic"], n_hypotheses=64)
    assert all(cnt == 0 for _, cnt in t.loop_profile().values())                  # the switch resets the record, and nothing is booked while it is off
