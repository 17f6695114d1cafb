"""The camera-IMU rotation calibration on the device (include/vilfusion.h, "Camera-IMU rotation calibration"): the C ABI against the numpy restatement
(tests/exrot_reference.py), every integer and every bit of every field of the result rows and of the histories. The restatement's own worth is measured without a
GPU in tests/test_exrot_reference.py. K = 64 except where a test says otherwise."""
import ctypes as C
import numpy as np
import pytest
import exrot_cases as ec
import exrot_reference as er
from vil_fusion_amd import abi

K = 64
ROW_KEYS = ("frame_count", "flags", "count", "best_k", "score", "front", "chosen", "ok", "Rc", "angle", "weight", "sigma", "x", "ric")
HIST_KEYS = ("count", "Rc", "Rimu", "Rcg", "angle", "weight")


@pytest.fixture(scope="module")
def solver():
    from vil_fusion_amd.estimator import BackendSolver
    s = BackendSolver()
    yield s
    s.close()


def same(got, want, keys, what):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and np.array_equal(g, w), (what, k, got[k], want[k])


def pair_of(pr):
    return None if pr is None else (pr["a"], pr["b"], pr["dq"])


def run_both(solver, pushes_per_slot, **params):
    """pushes_per_slot[s] = the pushes of slot s, None where the slot is skipped in that call; all lists equally long. Every row and, after every call, every
    history is compared. -> (the device's rows [call][slot], the restatement's calibrators)"""
    from vil_fusion_amd.estimator import ExRotation
    S, n_calls = len(pushes_per_slot), len(pushes_per_slot[0])
    dev = ExRotation(solver, S, **params)
    cals = [er.Calibrator(**params) for _ in range(S)]
    rows = []
    for c in range(n_calls):
        prs = [pushes_per_slot[s][c] for s in range(S)]
        got = dev.push([pair_of(pr) for pr in prs])
        assert len(got) == S
        for s in range(S):
            want = cals[s].skipped() if prs[s] is None else cals[s].push(prs[s]["a"], prs[s]["b"], prs[s]["dq"])
            same(got[s], want, ROW_KEYS, f"call {c} slot {s}")
            same(dev.history(s), cals[s].history(), HIST_KEYS, f"history after call {c} slot {s}")
        rows.append(got)
    return rows, cals


@pytest.mark.gpu
@pytest.mark.parametrize("m,k", [(8, K), (9, K), (150, K), (abi.VILF_MAX_FEATURES, 512)])
def test_gpu_correspondence_counts(solver, m, k):
    """two pushes each, so that the second runs with a ric other than the identity"""
    rows, _ = run_both(solver, [ec.make_pushes(100 + m, 2, m=m)], n_hypotheses=k, seed=3)
    for (r,) in rows:
        assert r["count"] == m
        if m == 8:                                            # below min_corres: the identity, nothing searched
            assert r["flags"] == 0 and r["best_k"] == -1 and r["chosen"] == -1 and np.array_equal(r["Rc"], np.eye(3))
        else:
            assert r["flags"] == abi.VILF_EXROT_SOLVED and 0 <= r["best_k"] < k and r["chosen"] in (0, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 2])
def test_gpu_push_counts_and_first_success(solver, seed):
    """pushes 1 .. 12: min_frames - 1 = 9 gives no success although its sigmas would do, min_frames = 10 gives the first"""
    rows, _ = run_both(solver, [ec.make_pushes(seed, 12)], n_hypotheses=K, seed=seed)
    rows = [r[0] for r in rows]
    assert [r["frame_count"] for r in rows] == list(range(1, 13))
    assert [r["ok"] for r in rows] == [False] * 9 + [True] * 3
    assert rows[8]["sigma"][2] > 0.25 and rows[9]["sigma"][2] > 0.25
    assert {r["chosen"] for r in rows} == {0, 1}              # both choices of R occur in each of the two cases
    assert ec.angle_between(rows[9]["ric"], ec.ric_true()) <= 7.9e-3          # the restatement's bound (test_exrot_reference.py: 10 x 7.9e-4 degrees)


@pytest.mark.gpu
def test_gpu_one_axis_rotation_never_succeeds(solver):
    rows, _ = run_both(solver, [ec.make_pushes(7, 12, one_axis=True)], n_hypotheses=K)
    for (r,) in rows:
        assert not r["ok"] and r["sigma"][2] < 0.25
    assert rows[-1][0]["sigma"][1] > 0.25


@pytest.mark.gpu
def test_gpu_huber_branch(solver):
    """an identity pair (m < 9) under a 20 degree IMU rotation has angle > 5 and weight 5 / angle, computed anew and unchanged on the later pushes; the pairs
    after it turn by 2 degrees, so Rc and Rc_g are at most 4 degrees apart whatever ric is by then, and weigh exactly 1.0"""
    from vil_fusion_amd.estimator import ExRotation
    pushes = ec.make_pushes(11, 1, m=8, deg=20.0) + ec.make_pushes(12, 3, deg=2.0)
    rows, cals = run_both(solver, [pushes], n_hypotheses=K)
    first = rows[0][0]
    assert first["flags"] == 0 and abs(first["angle"] - 20.0) < 1e-9 and first["weight"] == np.float64(5.0) / first["angle"]
    for (r,) in rows[1:]:
        assert 0.0 < r["angle"] < 5.0 and r["weight"] == 1.0
    h = cals[0].history()
    assert h["angle"][0] == first["angle"] and h["weight"][0] == first["weight"] and np.all(h["weight"][1:] == 1.0)
    dev = ExRotation(solver, 1, n_hypotheses=K)                # a second calibrator on the handle starts empty
    assert dev.history(0)["count"] == 0


@pytest.mark.gpu
def test_gpu_slots(solver):
    """three slots with histories of different lengths in one call, skipped slots, slot 0 alone against slot 0 among the three, reset"""
    from vil_fusion_amd.estimator import ExRotation
    p0, p1, p2 = ec.make_pushes(20, 4), ec.make_pushes(21, 4, m=60), ec.make_pushes(22, 4, m=25)
    sched = [[p0[0], p0[1], p0[2], p0[3]],
             [None, p1[0], None, p1[1]],
             [p2[0], None, None, p2[1]]]
    rows3, cals3 = run_both(solver, sched, n_hypotheses=K, seed=9)
    assert [cals3[s].frame_count for s in range(3)] == [4, 2, 2]
    # a skipped slot is unchanged bit for bit: run_both compares its history after every call; its row only reports
    assert rows3[2][1]["flags"] == abi.VILF_EXROT_SKIPPED and rows3[2][1]["frame_count"] == 1 and rows3[0][1]["frame_count"] == 0
    rows1, _ = run_both(solver, [sched[0]], n_hypotheses=K, seed=9)
    for c in range(4):
        same(rows1[c][0], rows3[c][0], ROW_KEYS, f"slot 0 alone, call {c}")
    dev = ExRotation(solver, 3, n_hypotheses=K, seed=9)
    dev.push([pair_of(p0[0]), None, pair_of(p2[0])])
    assert [dev.history(s)["count"] for s in range(3)] == [1, 0, 1]
    dev.reset()
    assert [dev.history(s)["count"] for s in range(3)] == [0, 0, 0]
    got = dev.push([pair_of(p0[0]), pair_of(p1[0]), pair_of(p2[0])])          # after the reset the first pushes give what they gave
    same(got[0], rows3[0][0], ROW_KEYS, "after reset, slot 0")
    same(got[2], rows3[0][2], ROW_KEYS, "after reset, slot 2")


@pytest.mark.gpu
def test_gpu_degenerate_points(solver):
    """all points identical: no hypothesis is valid, the flag says so, Rc = I and nothing in the history is not finite"""
    pr = ec.make_pushes(30, 3)
    for p in pr[1:]:
        p["a"] = np.tile(p["a"][:1], (40, 1)); p["b"] = np.tile(p["b"][:1], (40, 1))
    rows, cals = run_both(solver, [pr], n_hypotheses=K)
    for (r,) in rows[1:]:
        assert r["flags"] == abi.VILF_EXROT_COUNT and r["best_k"] == -1 and r["chosen"] == -1 and np.array_equal(r["Rc"], np.eye(3))
    h = cals[0].history()
    assert all(np.isfinite(h[k]).all() for k in HIST_KEYS[1:])
    assert all(np.isfinite(rows[-1][0][k]).all() for k in ("sigma", "x", "ric", "angle", "weight"))


@pytest.mark.gpu
def test_gpu_large_rotations_take_every_quaternion_branch(solver):
    """IMU rotations of 170 degrees about axes near x, y and z have a trace below 0, so quat(Rimu) and quat(Rc_g) go through the branches of the largest
    diagonal entry, each of the three; one delta_q is not a unit quaternion, which R(q) does not normalise. m = 0: Rc = I"""
    empty = np.zeros((0, 2))
    axes = ([1.0, 0.1, -0.2], [0.1, 1.0, 0.2], [-0.2, 0.1, 1.0], [0.3, -1.0, 0.1], [1.0, 0.9, 0.1], [0.1, 0.2, -1.0])
    pushes = [dict(a=empty, b=empty, dq=ec.quat_xyzw(ax, 170.0) * (1.001 if i == 3 else 1.0)) for i, ax in enumerate(axes)]
    largest = set()
    for pr in pushes:
        R = er.q_to_R(pr["dq"])
        assert np.trace(R) < 0.0
        largest.add(int(np.argmax(np.diag(R))))
    assert largest == {0, 1, 2}
    rows, _ = run_both(solver, [pushes], n_hypotheses=K)
    assert all(r["weight"] < 1.0 for (r,) in rows[:1])        # 170 degrees between Rc = I and Rc_g: the Huber branch


def raw_push(solver, params, n_slots, pairs, null=None):
    """the C call on pairs = [(n, a, b, dq)] with out filled with a pattern -> (status, whether out is untouched)"""
    from vil_fusion_amd.lib import lib
    arr = (abi.ExrotPair * max(len(pairs), 1))()
    keep = []
    for k, (n, a, b, dq) in enumerate(pairs):
        a = None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        b = None if b is None else np.ascontiguousarray(b, dtype=np.float64)
        keep.append((a, b))
        arr[k].n, arr[k].a, arr[k].b = n, abi.dptr(a), abi.dptr(b)
        arr[k].delta_q[:] = [float(v) for v in dq]
    out = (abi.ExrotResult * max(n_slots, len(pairs), 1))()
    C.memset(out, 0x5a, C.sizeof(out))
    before = bytes(out)
    rc = lib().vilf_exrot_push(solver._h, None if null == "params" else C.byref(params), n_slots, None if null == "pairs" else arr, None if null == "out" else out)
    return rc, bytes(out) == before


@pytest.mark.gpu
def test_gpu_refusals_leave_state_and_outputs_untouched(solver):
    from vil_fusion_amd.estimator import ExRotation, exrot_default_params
    from vil_fusion_amd.lib import lib
    pushes = ec.make_pushes(40, 3)
    dev = ExRotation(solver, 2, n_hypotheses=K)
    cal = er.Calibrator(n_hypotheses=K)
    want = cal.push(pushes[0]["a"], pushes[0]["b"], pushes[0]["dq"])
    same(dev.push([pair_of(pushes[0]), None])[0], want, ROW_KEYS, "first push")
    P = lambda **kw: exrot_default_params(**dict(dict(n_hypotheses=K), **kw))
    a, b, dq = pushes[1]["a"], pushes[1]["b"], pushes[1]["dq"]
    good, skip = (40, a, b, dq), (-1, None, None, [0, 0, 0, 1])
    bad_a, bad_b = a.copy(), b.copy()
    bad_a[7, 1] = np.nan; bad_b[39, 0] = np.inf
    big = np.zeros((abi.VILF_MAX_FEATURES + 1, 2))
    cases = {
        "null params": (P(), 2, [good, skip], "params"), "null pairs": (P(), 2, [good, skip], "pairs"), "null out": (P(), 2, [good, skip], "out"),
        "null a": (P(), 2, [(40, None, b, dq), skip], None), "null b": (P(), 2, [skip, (40, a, None, dq)], None),
        "n_slots 0": (P(), 0, [good, skip], None), "n_slots > max": (P(), abi.VILF_EXROT_MAX_SLOTS + 1, [good, skip], None),
        "n_slots other than the reset's": (P(), 1, [good], None),
        "n < -1": (P(), 2, [(-2, a, b, dq), skip], None), "n > max": (P(), 2, [(abi.VILF_MAX_FEATURES + 1, big, big, dq), skip], None),
        "coordinate nan": (P(), 2, [(40, bad_a, b, dq), skip], None), "coordinate inf": (P(), 2, [skip, (40, a, bad_b, dq)], None),
        "delta_q nan": (P(), 2, [(40, a, b, [0, np.nan, 0, 1]), skip], None), "delta_q inf": (P(), 2, [(0, None, None, [0, 0, np.inf, 1]), skip], None),
        "K 0": (P(n_hypotheses=0), 2, [good, skip], None), "K > max": (P(n_hypotheses=abi.VILF_TRACK_MAX_HYPOTHESES + 1), 2, [good, skip], None),
        "threshold 0": (P(ransac_threshold=0.0), 2, [good, skip], None), "threshold nan": (P(ransac_threshold=np.nan), 2, [good, skip], None),
        "huber 0": (P(huber_deg=0.0), 2, [good, skip], None), "huber inf": (P(huber_deg=np.inf), 2, [good, skip], None),
        "min_sigma < 0": (P(min_sigma=-0.25), 2, [good, skip], None), "min_sigma nan": (P(min_sigma=np.nan), 2, [good, skip], None),
        "min_corres < 0": (P(min_corres=-1), 2, [good, skip], None), "min_frames < 0": (P(min_frames=-1), 2, [good, skip], None),
    }
    for name, (p, n_slots, pairs, null) in cases.items():
        rc, clean = raw_push(solver, p, n_slots, pairs, null)
        assert rc == abi.VILF_ERR_INVALID_ARGUMENT and clean, (name, rc, clean)
    assert lib().vilf_exrot_reset(solver._h, 0) == abi.VILF_ERR_INVALID_ARGUMENT
    assert lib().vilf_exrot_reset(solver._h, abi.VILF_EXROT_MAX_SLOTS + 1) == abi.VILF_ERR_INVALID_ARGUMENT
    cnt = C.c_int(-7)
    assert lib().vilf_exrot_get_history(solver._h, 2, C.byref(cnt), None, None, None, None, None) == abi.VILF_ERR_INVALID_ARGUMENT and cnt.value == -7
    assert lib().vilf_exrot_get_history(solver._h, 0, None, None, None, None, None, None) == abi.VILF_ERR_INVALID_ARGUMENT
    # the state is what it was: the histories, and the next push gives what the restatement gives after one push
    same(dev.history(0), cal.history(), HIST_KEYS, "history after the refusals")
    assert dev.history(1)["count"] == 0
    want = cal.push(a, b, dq)
    same(dev.push([pair_of(pushes[1]), None])[0], want, ROW_KEYS, "the push after the refusals")


@pytest.mark.gpu
def test_gpu_full_slot_is_refused(solver):
    """VILF_EXROT_MAX_HISTORY pushes with m = 0 fill slot 0; slot 1 is pushed every 64th call. The next push into slot 0 is refused and changes nothing, a call
    that skips slot 0 still goes through"""
    from vil_fusion_amd.estimator import ExRotation, exrot_default_params
    H = abi.VILF_EXROT_MAX_HISTORY
    rng = np.random.default_rng(50)
    dev = ExRotation(solver, 2, n_hypotheses=K)
    cals = [er.Calibrator(keep=True, n_hypotheses=K), er.Calibrator(keep=True, n_hypotheses=K)]
    empty = np.zeros((0, 2))
    for c in range(H):
        axis, deg = ec.imu_rotation(rng)
        dq = ec.quat_xyzw(axis, deg)
        both = c % 64 == 63
        got = dev.push([(empty, empty, dq), (empty, empty, dq) if both else None])
        want = cals[0].push(empty, empty, dq)
        if both:
            cals[1].push(empty, empty, dq)
        if c % 32 == 31 or c == H - 1:
            same(got[0], want, ROW_KEYS, f"push {c + 1}")
    assert got[0]["frame_count"] == H and got[1]["frame_count"] == H // 64
    same(dev.history(0), cals[0].history(), HIST_KEYS, "the full history")
    same(dev.history(1), cals[1].history(), HIST_KEYS, "the other slot")
    dq = [0.0, 0.0, 0.0, 1.0]
    rc, clean = raw_push(solver, exrot_default_params(n_hypotheses=K), 2, [(0, None, None, dq), (0, None, None, dq)])
    assert rc == abi.VILF_ERR_INVALID_ARGUMENT and clean
    same(dev.history(0), cals[0].history(), HIST_KEYS, "the full history after the refusal")
    same(dev.history(1), cals[1].history(), HIST_KEYS, "the other slot after the refusal")
    got = dev.push([None, (empty, empty, dq)])
    same(got[1], cals[1].push(empty, empty, dq), ROW_KEYS, "the other slot still takes a push")
    same(got[0], cals[0].skipped(), ROW_KEYS, "the full slot, skipped")


@pytest.mark.gpu
def test_gpu_sliding_window_estimator_calibrates(solver):
    """hand-built image dicts through two SlidingWindowEstimators, one on the device (an ExRotation on the back-end's solver), one on the restatement: both
    calibrate at the same frame to the same ric, bit for bit"""
    from vil_fusion_amd import sequence as sq
    from vil_fusion_amd.lib import default_options

    class OnDevice:
        def __init__(self, s):
            self.s = s

    o = default_options()
    o.estimate_extrinsic = 2
    case = ec.make_images(5, sq.WINDOW_SIZE + 2)
    est_d, est_r = sq.SlidingWindowEstimator(o, OnDevice(solver)), sq.SlidingWindowEstimator(o, er.Backend())
    for k in range(sq.WINDOW_SIZE + 1):
        for est in (est_d, est_r):
            for dt, acc, gyr in case["imu"][k]:
                est.process_imu(dt, acc, gyr)
            solved = est.prepare_image(case["images"][k], case["stamps"][k])
            assert solved is (k == sq.WINDOW_SIZE)
    assert len(est_d.ex_rows) == len(est_r.ex_rows) == sq.WINDOW_SIZE
    for k, (g, w) in enumerate(zip(est_d.ex_rows, est_r.ex_rows)):
        same(g, w, ROW_KEYS, f"push {k + 1}")
    assert est_d.estimate_extrinsic == 1 and est_d.ex_calibrated == (sq.WINDOW_SIZE, sq.WINDOW_SIZE) and est_d.solver_flag == est_d.NON_LINEAR
    assert np.array_equal(est_d.ric, est_r.ric) and np.array_equal(est_d.ric, est_d.ex_rows[-1]["ric"])
    assert ec.angle_between(est_d.ric, ec.ric_true()) <= 0.013          # the bound of the gate test of test_exrot_reference.py: 10 x (5.1e-4 + 7.9e-4) degrees
