"""The third stage of the visual start-up, GlobalSFM's full bundle adjustment (include/vilfusion.h, "Visual start-up: GlobalSFM full BA"), and the hand-off of its
poses to visualInitialAlign.

CPU tests: what the numpy restatement (ba_reference.py) is worth against an independent solve (scipy's least_squares) and against ground truth, next to the chain
alone; the verdict's cases; the hand-off through SlidingWindowEstimator.initial_structure on a back-end assembled from the three restatements; the ctypes layouts.
GPU tests: the C ABI against the restatement, every integer and every bit.

The accuracy and hand-off bounds are twice, the solver-difference bounds ten times what the restatement itself showed on these scenes (the tables below and
DESIGN.md §3p); none of them comes from the HIP path."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import sfm_cases as sc
import ba_cases as bc
import ba_reference as ref
from vil_fusion_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUMMARY = ("ok", "flags", "iterations", "accepted", "n_camera", "n_members", "n_residuals", "l")


def run_ref(s, st, **params):
    return ref.bundle_adjust(s["win"], st["l"], st["R"], st["t"], st["state"], st["positions"], chain_ok=st.get("chain_ok", True), **params)


def line(r):
    return (f"ok {int(r['ok'])} flags {r['flags']} iterations {r['iterations']} accepted {r['accepted']} cost {float(r['cost0']):.3e} -> {float(r['cost1']):.3e} "
            f"lambda {float(r['lam']):.1e}")


# ---- against an independent solve ---------------------------------------------------------------------------------------------------------------------------
# measured with the restatement (ba_iterations 64, function_tolerance 1e-30, so that it runs on to the minimum as scipy does) on chain_scene(2000 + 10 * noise)
# from the chain's result, one run, rounded up to two digits: the largest rotation [deg] and position [baselines] difference of a frame and the largest relative
# difference of a point to scipy's least_squares (method lm, tolerances 1e-15, poses as a Rodrigues vector on the start's rotation, the same constants) from the
# same start on the same observations. The test asserts ten times these.
SOLVER_DIFFERENCE = {
    0.0: (1.8e-14, 1.7e-15, 2.9e-14),
    0.5: (3.7e-06, 3.0e-07, 3.1e-06),
}


def rodrigues(w):
    th = np.linalg.norm(w)
    if th < 1e-300:
        return np.eye(3)
    return sc.rot(w / th, np.rad2deg(th))


def scipy_ba(win, st):
    """the same problem in scipy's hands -> (R [nf][3][3], t [nf][3], X [n][3])"""
    from scipy.optimize import least_squares
    start, first, nobs, pts = ref.table(win)
    nf, l, newest = int(win["n_frames"]), st["l"], int(win["n_frames"]) - 1
    mem = np.nonzero(st["state"])[0]
    fo = np.array([(f, k) for f in mem for k in range(start[f], start[f] + nobs[f])])
    u = np.array([pts[first[f] + k - start[f]] for f, k in fo])
    col = {f: i for i, f in enumerate(mem)}
    ci = np.array([col[f] for f in fo[:, 0]])
    off = [ref.first_index(k, l) for k in range(nf)]
    nc = 6 * nf - 9

    def unpack(x):
        R, t = st["R"].copy(), st["t"].copy()
        for k in range(nf):
            nk = ref.free_count(k, l, newest)
            if nk:
                R[k] = rodrigues(x[off[k]:off[k] + 3]) @ st["R"][k]
            if nk == 6:
                t[k] = x[off[k] + 3:off[k] + 6]
        return R, t, x[nc:].reshape(-1, 3)

    def res(x):
        R, t, X = unpack(x)
        p = np.einsum("oij,oj->oi", R[fo[:, 1]], X[ci]) + t[fo[:, 1]]
        return (p[:, :2] / p[:, 2:3] - u).ravel()

    x0 = np.zeros(nc + 3 * len(mem))
    for k in range(nf):
        if ref.free_count(k, l, newest) == 6:
            x0[off[k] + 3:off[k] + 6] = st["t"][k]
    x0[nc:] = st["positions"][mem].ravel()
    sol = least_squares(res, x0, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, x_scale=1.0)
    R, t, Xm = unpack(sol.x)
    X = np.zeros((len(start), 3))
    X[mem] = Xm
    return R, t, X


@pytest.fixture(scope="module")
def accuracy_runs():
    """scene, chain, BA of the chain's result (the defaults) per noise level, computed once"""
    out = {}
    for nz in NOISES:
        s = sc.chain_scene(2000 + int(10 * nz), noise_px=nz)
        ch, ba = ref.construct(s["win"], s["l"], s["rel_R"], s["rel_T"])
        out[nz] = (s, ch, ba)
    return out


def chain_start(ch):
    return dict(l=ch["l"], R=np.array([f["R"] for f in ch["frames"]]), t=np.array([f["t"] for f in ch["frames"]]), state=ch["state"], positions=ch["positions"],
                chain_ok=ch["ok"])


def test_restatement_against_scipy_least_squares(accuracy_runs):
    bad = []
    for nz in (0.0, 0.5):
        s, ch, _ = accuracy_runs[nz]
        st = chain_start(ch)
        r = run_ref(s, st, ba_iterations=64, function_tolerance=1e-30)
        Rs, ts, Xs = scipy_ba(s["win"], st)
        m = r["state"] == 1
        got = (max(sc.rot_err_deg(f["R"], Rs[k]) for k, f in enumerate(r["frames"])), max(float(np.linalg.norm(f["t"] - ts[k])) for k, f in enumerate(r["frames"])),
               float((np.linalg.norm(r["positions"][m] - Xs[m], axis=1) / np.linalg.norm(Xs[m], axis=1)).max()))
        print(f"noise {nz:.1f} px: {line(r)}; vs scipy least_squares: {got[0]:.3e} deg, {got[1]:.3e} baselines, points {got[2]:.3e} relative")
        if any(g > 10.0 * b for g, b in zip(got, SOLVER_DIFFERENCE[nz])):
            bad.append((nz, got))
    assert not bad, bad


# ---- accuracy against ground truth, next to the chain alone ---------------------------------------------------------------------------------------------
NOISES = (0.0, 0.1, 0.5)
# measured with the restatement on chain_scene(2000 + 10 * noise, noise_px=noise), the scenes of the chain's table, chain then BA with the defaults,
# one run, rounded up to two digits: the largest rotation error of a frame [deg], the largest position error of a frame [baselines], the median and the largest
# relative error of a point. The test asserts twice these. The chain alone on the same scenes (§3o's table): 6.4e-07 / 0.021 / 0.097 deg, 7.6e-08 / 0.0039 / 0.0096
# baselines, points median 2.2e-08 / 0.0053 / 0.017, max 9.5e-07 / 0.093 / 0.44; the test prints both next to each other and asserts no ratio.
ACCURACY = {
    0.0: (2.3e-14, 3.7e-15, 4.7e-15, 2.9e-14),
    0.1: (0.013, 0.0017, 0.0019, 0.071),
    0.5: (0.077, 0.0084, 0.019, 0.35),
}


def errors(s, frames, state, positions):
    rot = [sc.rot_err_deg(f["Q"], s["Q"][k]) for k, f in enumerate(frames)]
    pos = [float(np.linalg.norm(f["T"] - s["T"][k])) for k, f in enumerate(frames)]
    ok = state == 1
    pt = np.linalg.norm(positions[ok] - s["X"][ok], axis=1) / np.linalg.norm(s["X"][ok], axis=1)
    return max(rot), max(pos), float(np.median(pt)), float(pt.max())


def test_restatement_accuracy_against_ground_truth(accuracy_runs):
    bad = []
    for nz, (s, ch, ba) in sorted(accuracy_runs.items()):
        assert ch["ok"] and ba["ok"] and ba["n_members"] == 150 and ba["n_camera"] == 57
        assert ba["cost1"] <= ba["cost0"]                        # the acceptance rule, not a measurement
        before, got = errors(s, ch["frames"], ch["state"], ch["positions"]), errors(s, ba["frames"], ba["state"], ba["positions"])
        print(f"noise {nz:.1f} px: {line(ba)}")
        print(f"  chain alone : rot {before[0]:.3e} deg, pos {before[1]:.3e}, points median {before[2]:.3e} max {before[3]:.3e}")
        print(f"  chain + BA  : rot {got[0]:.3e} deg, pos {got[1]:.3e}, points median {got[2]:.3e} max {got[3]:.3e}")
        if any(g > 2.0 * b for g, b in zip(got, ACCURACY[nz])):
            bad.append((nz, got))
    assert not bad, bad


@pytest.mark.parametrize("case", ["near", "far", "two_frame_tracks", "lonely_frame", "same_centre", "on_axis", "behind"])
def test_cost_never_rises(case):
    s, st = verdict_case(case)
    r = run_ref(s, st)
    assert r["cost1"] <= r["cost0"] or not np.isfinite(r["cost0"])
    assert r["accepted"] == sum(1 for w in r["rejections"] if w is None) and r["iterations"] == len(r["rejections"])


# ---- the verdict ------------------------------------------------------------------------------------------------------------------------------------------------
def verdict_case(name):
    if name == "truth":                                           # no noise, the start is the truth
        s = bc.scene(6000, noise_px=0.0)
        return s, bc.truth_start(s)
    if name == "near":                                            # 0.1 px of noise: the function tolerance ends the loop
        s = bc.scene(6001)
        return s, bc.near(s)
    if name == "far":                                             # steps are rejected, lambda rises
        s = bc.scene(6001)
        return s, bc.far(s)
    if name == "two_frame_tracks":
        s = bc.two_frame_tracks(6002)
        return s, bc.near(s)
    if name == "lonely_frame":
        s = bc.lonely_frame(6003)
        return s, bc.near(s)
    if name == "same_centre":
        s, st = bc.same_centre()
        return s, bc.perturbed(st, 3, rot_deg=0.3, pos=0.01, pt_rel=0.01)
    if name == "on_axis":
        return bc.same_centre(on_axis=True)
    if name == "behind":
        return bc.behind_the_camera()
    raise KeyError(name)


def test_verdict_by_cost_and_by_convergence():
    r = run_ref(*verdict_case("truth"))
    assert r["ok"] and r["flags"] & ref.COST and r["flags"] & ref.FINITE and 0.5 * r["cost1"] < 5e-3
    r = run_ref(*verdict_case("truth"), cost_threshold=1e-40)    # the same run without the cost's help: it did not end by the tolerance, so it fails
    assert not r["flags"] & ref.COST and r["ok"] == bool(r["flags"] & ref.CONVERGED)
    r = run_ref(*verdict_case("near"), cost_threshold=1e-12)     # a noisy scene: ok by convergence alone
    assert r["ok"] and r["flags"] == ref.CONVERGED | ref.FINITE and r["iterations"] < 20 and r["accepted"] == r["iterations"]
    print("near:", line(r))


def test_one_iteration_from_a_far_start_follows_the_cost_rule_alone():
    s, st = verdict_case("far")
    r = run_ref(s, st, ba_iterations=1)
    assert r["iterations"] == 1 and r["accepted"] <= 1 and not r["flags"] & ref.CONVERGED and r["flags"] & ref.FINITE
    assert not r["ok"] and not r["flags"] & ref.COST and 0.5 * r["cost1"] >= 5e-3
    half = np.float64(0.5) * r["cost1"]
    at = run_ref(s, st, ba_iterations=1, cost_threshold=float(half))                       # final_cost < cost_threshold is strict
    above = run_ref(s, st, ba_iterations=1, cost_threshold=float(np.nextafter(half, np.inf)))
    assert not at["ok"] and not at["flags"] & ref.COST and above["ok"] and above["flags"] == ref.COST | ref.FINITE
    assert at["cost1"] == r["cost1"] and above["cost1"] == r["cost1"]


def test_a_point_in_the_camera_plane_fails_by_finite():
    r = run_ref(*verdict_case("behind"))
    assert not r["ok"] and not r["flags"] & ref.FINITE and r["accepted"] == 0 and not np.isfinite(r["cost1"])
    assert all(np.isfinite(f[k]).all() for f in r["frames"] for k in ("R", "t", "Q", "T"))   # what it reached is still reported: the start


def test_zero_parallax_does_not_poison_the_step():
    s, st = verdict_case("same_centre")                           # damping keeps the rank-2 V solvable
    r = run_ref(s, st)
    assert r["ok"] and r["accepted"] >= 5 and "V" not in r["rejections"] and "S" not in r["rejections"] and r["cost1"] < 1e-6 * r["cost0"]
    assert np.isfinite(r["positions"]).all()
    others = np.arange(1, 60)
    assert (np.linalg.norm(r["positions"][others] - s["X"][others], axis=1) / np.linalg.norm(s["X"][others], axis=1)).max() < 1e-6
    s, st = verdict_case("on_axis")                               # the third pivot of feature 0's V is 0 at any lambda: the pivot rule rejects every step
    r = run_ref(s, st)
    assert r["rejections"] == ["V"] * 20 and r["accepted"] == 0 and r["cost1"] == r["cost0"] and r["ok"] and r["flags"] == ref.COST | ref.FINITE
    assert all(np.array_equal(f["R"], st["R"][k]) and np.array_equal(f["t"], st["t"][k]) for k, f in enumerate(r["frames"]))
    assert np.array_equal(r["positions"], st["positions"]) and float(r["lam"]) > 1e16


def test_rejected_steps_raise_lambda():
    r = run_ref(*verdict_case("far"))
    lam = [float(v) for v in r["lambdas"]]
    rises = sum(1 for a, b in zip(lam, lam[1:]) if b > a)
    assert rises >= 2 and rises == sum(1 for w in r["rejections"][:-1] if w is not None) and "cost" in r["rejections"] and 0 < r["accepted"] < r["iterations"] and r["ok"]
    print("far:", line(r), "lambdas", " ".join(f"{v:.0e}" for v in lam))


def test_skipped_windows():
    s, st = verdict_case("near")
    for kw in (dict(l=-1), dict(chain_ok=False)):
        r = run_ref(s, dict(st, **kw))
        assert not r["ok"] and r["flags"] == 0 and r["iterations"] == 0 and r["n_camera"] == 0 and r["l"] == kw.get("l", st["l"])
        assert not r["positions"].any() and not r["state"].any() and not any(f[k].any() for f in r["frames"] for k in ("R", "t", "Q", "T"))


def test_unknown_counts():
    for nf, l, want in ((2, 0, 3), (3, 0, 9), (3, 1, 9), (11, 5, 57)):
        s = bc.scene(6100 + nf, n_frames=nf, n=30, l=l)
        r = run_ref(s, bc.near(s), ba_iterations=2)
        assert r["n_camera"] == want and r["n_residuals"] == int(np.diff(s["win"]["first_obs"])[r["state"] == 1].sum())


# ---- the hand-off -------------------------------------------------------------------------------------------------------------------------------------------
# measured on make_sequence(11, WINDOW_SIZE + 1) with the three restatements (n_hypotheses 256), one run, rounded up to two digits: the largest rotation difference
# [deg] of a frame to make_sfm_frames(rot_noise=0, pos_noise=0) after both are referred to frame 0, and the largest position difference after the similarity
# (Umeyama) that maps one set of camera positions onto the other, in units of the path's length. The test asserts twice these. (The rotation difference grows
# along the window to its largest value at the newest frame: the BA holds c_t[newest] at the direction the first stage's RANSAC found, as the reference does.)
HAND_OFF = (0.48, 0.0059)


class RestatedBackend:
    """a back-end whose construct is the three numpy restatements; the alignment is the CPU oracle's"""

    def __init__(self, opts):
        import seq_backends
        self.oracle = seq_backends.OracleBackend(opts)

    def construct(self, tables, **params):
        import startup_reference as ref1
        stage1 = {k: params.pop(k) for k in list(params) if k in ("n_hypotheses", "seed")}
        out = []
        for tb in tables:
            r1 = ref1.relative_pose(tb, **stage1)
            ch, ba = ref.construct(tb, r1["l"] if r1["ok"] else -1, r1["R"], r1["T"], **params)
            out.append(dict(ba, chain=ch))
        return out

    def align(self, inputs):
        return self.oracle.align(inputs)


def umeyama(A, B):
    """the similarity (s, R, t) with B ~ s R A + t"""
    ma, mb = A.mean(axis=0), B.mean(axis=0)
    U, d, Vt = np.linalg.svd((B - mb).T @ (A - ma) / len(A))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    R = U @ D @ Vt
    s = float((d * np.diag(D)).sum() / ((A - ma) ** 2).sum() * len(A))
    return s, R, mb - s * R @ ma


def filled_estimator(backend_of):
    from vil_fusion_amd import sequence as sq
    from vil_fusion_amd.lib import default_options
    opts = default_options()
    seq = sq.make_sequence(11, sq.WINDOW_SIZE + 1, opts)
    est = sq.SlidingWindowEstimator(opts, backend_of(opts))
    est.process_imu(0.0, *seq["imu0"])
    for k in range(sq.WINDOW_SIZE):
        sq._feed_measurements(est, seq, k)
        assert est.process_image(seq["images"][k], seq["stamps"][k]) is None
    k = sq.WINDOW_SIZE
    sq._feed_measurements(est, seq, k)
    est.stamps[k] = seq["stamps"][k]
    est.f.add_feature_check_parallax(k, dict(sorted(seq["images"][k].items())), est.td)
    return sq, opts, seq, est


def hand_off_differences(sq, opts, seq, est, frames):
    want = sq.make_sfm_frames(seq, opts, est, rot_noise=0.0, pos_noise=0.0)
    assert len(frames) == len(want) == sq.WINDOW_SIZE + 1 and [f["stamp"] for f in frames] == [f["stamp"] for f in want]
    rot = max(sc.rot_err_deg(frames[0]["R"].T @ f["R"], want[0]["R"].T @ w["R"]) for f, w in zip(frames, want))
    A, B = np.array([f["T"] for f in frames]), np.array([w["T"] for w in want])
    s, R, t = umeyama(A, B)
    pos = float(np.linalg.norm(s * A @ R.T + t - B, axis=1).max() / np.linalg.norm(np.diff(B, axis=0), axis=1).sum())
    return rot, pos


def test_initial_structure_hands_frames_to_visual_initial_align():
    sq, opts, seq, est = filled_estimator(RestatedBackend)
    frames = est.initial_structure(n_hypotheses=256)
    assert frames is not None and est.structure["ok"] and est.structure["chain"]["ok"]
    got = hand_off_differences(sq, opts, seq, est, frames)
    print(f"hand-off: l {est.structure['l']}, {line(est.structure)}; vs make_sfm_frames without noise: {got[0]:.3e} deg, {got[1]:.3e} of the path")
    assert all(g <= 2.0 * b for g, b in zip(got, HAND_OFF)), got
    RIC = np.array(opts.RIC[:]).reshape(3, 3)
    for k, f in enumerate(frames):
        assert np.array_equal(f["R"], est.structure["frames"][k]["Q"] @ RIC.T) and np.array_equal(f["T"], est.structure["frames"][k]["T"]) and f["pre"] is not est.pre[k]
    assert est.visual_initial_align(frames) and est.alignment["ok"]


def test_initial_structure_returns_none_where_the_structure_fails():
    sq, opts, seq, est = filled_estimator(RestatedBackend)
    assert est.initial_structure(n_hypotheses=256, cost_threshold=1e-300, ba_iterations=1) is None and not est.structure["ok"]


def test_run_sequence_starts_up_through_the_device_route_on_request():
    from vil_fusion_amd import sequence as sq
    from vil_fusion_amd.lib import default_options
    import seq_backends

    class Backend(RestatedBackend):
        def solve(self, win):
            return self.oracle.solve(win)

        def marginalize(self, win, res):
            return self.oracle.marginalize(win, res)

        def reset(self):
            self.oracle.reset()

    opts = default_options()
    seq = sq.make_sequence(11, sq.WINDOW_SIZE + 3, opts)
    startup = dict(source="device", n_hypotheses=256)
    est = sq.run_sequence(seq, opts, Backend(opts), startup=startup)
    assert startup == dict(source="device", n_hypotheses=256)     # the caller's dict is left alone
    # a failed alignment slides the window and the next frame tries again, so the first solve may come a frame late
    assert est.initial_ok and est.solver_flag == est.NON_LINEAR and 1 <= est.events.count("solved") <= 3 and est.structure["ok"] and est.alignment["ok"]
    assert "reboot" not in est.events and len(est.trajectory) == est.events.count("solved")
    plain = sq.run_sequence(seq, opts, Backend(opts), startup=dict(rot_noise=0.0, pos_noise=0.0))     # without the option: the stand-in, as before
    assert not hasattr(plain, "structure") and plain.events.count("solved") == 3


def test_ctypes_mirrors_of_the_ba_match_the_c_layout(tmp_path):
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "vilfusion.h"', "int main(void) {"]
    checks = []
    for cname, ct in abi.STARTUP_BA_LAYOUTS.items():
        prog.append(f'  printf("%zu\\n", sizeof({cname}));')
        checks.append((cname, "sizeof", C.sizeof(ct)))
        for fname, _ in ct._fields_:
            prog.append(f'  printf("%zu\\n", offsetof({cname}, {abi.STARTUP_BA_C_NAMES.get(fname, fname)}));')
            checks.append((cname, fname, getattr(ct, fname).offset))
    for name in ("VILF_BA_CONVERGED", "VILF_BA_COST", "VILF_BA_FINITE"):
        prog.append(f'  printf("%d\\n", {name});')
        checks.append((name, "value", getattr(abi, name)))
    prog += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(prog))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert len(out) == len(checks)
    bad = [(c, f, int(o), e) for (c, f, e), o in zip(checks, out) if int(o) != e]
    assert not bad, bad
    assert (ref.CONVERGED, ref.COST, ref.FINITE) == (abi.VILF_BA_CONVERGED, abi.VILF_BA_COST, abi.VILF_BA_FINITE)


def test_library_exports_the_ba():
    from vil_fusion_amd import lib
    so = os.path.join(ROOT, "vil_fusion_amd", "csrc", "libvilfusion_hip.so")
    if not os.path.exists(so):
        lib.build()
    L = C.CDLL(so)
    names = ("vilf_startup_default_ba_params", "vilf_startup_ba", "vilf_startup_construct", "vilf_startup_get_ba_structure", "vilf_startup_ba_profile")
    assert all(hasattr(L, n) for n in names) and set(names) <= set(lib.EXPORTED)
    p = abi.StartupBaParams()
    L.vilf_startup_default_ba_params.restype = None
    L.vilf_startup_default_ba_params(C.byref(p))
    assert (p.ba_iterations, p.lambda0, p.function_tolerance, p.cost_threshold) == (20, 1e-3, 1e-6, 5e-3)
    assert ref.DEFAULTS == dict(ba_iterations=20, lambda0=1e-3, function_tolerance=1e-6, cost_threshold=5e-3)


# ---- GPU: the C ABI against the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver():
    from vil_fusion_amd.estimator import BackendSolver
    s = BackendSolver()
    yield s
    s.close()


def same_bits(a, b):
    """bit for bit; a NaN equals a NaN (the sign and payload of a NaN are not arithmetic)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64).ravel(), np.ascontiguousarray(b, dtype=np.float64).ravel()
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | nan))


def same_result(got, want, where):
    for k in SUMMARY:
        assert got[k] == want[k], (where, k, got[k], want[k])
    for k in ("cost0", "cost1", "lam"):
        assert same_bits(got[k], want[k]), (where, k, got[k], want[k])
    assert len(got["frames"]) == len(want["frames"])
    for i, (g, w) in enumerate(zip(got["frames"], want["frames"])):
        for k in ("R", "t", "Q", "T"):
            assert same_bits(g[k], w[k]), (where, i, k, g[k], w[k])
    assert np.array_equal(got["state"], want["state"]), (where, "state")
    assert same_bits(got["positions"], want["positions"]), (where, "positions")


def run_both(solver, cases, **params):
    from vil_fusion_amd.estimator import bundle_adjust
    got = bundle_adjust(solver, [s["win"] for s, _ in cases], [st for _, st in cases], **params)
    want = [run_ref(s, st, **params) for s, st in cases]
    for k, (g, w) in enumerate(zip(got, want)):
        same_result(g, w, k)
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize("n_frames,l", [(2, 0), (3, 0), (3, 1), (11, 0), (11, 5), (11, 9)])
def test_gpu_frame_counts_and_l(solver, n_frames, l):
    s = bc.scene(7000 + 10 * n_frames + l, n_frames=n_frames, n=90, l=l)
    got, _ = run_both(solver, [(s, bc.near(s, state=bc.interleaved_state(90)))])
    assert got[0]["ok"] and got[0]["n_camera"] == 6 * n_frames - 9 and 0 < got[0]["n_members"] <= 60 and got[0]["accepted"] >= 3


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_gpu_feature_counts(solver, n):
    s = bc.scene(7100 + n, n_frames=4, n=n, l=1)
    got, _ = run_both(solver, [(s, bc.near(s))])
    assert got[0]["n_members"] == n and got[0]["flags"] & ref.FINITE and got[0]["cost1"] <= got[0]["cost0"]


@pytest.mark.gpu
def test_gpu_full_window_of_1000_features(solver):
    s = bc.scene(7200, n=1000)
    got, _ = run_both(solver, [(s, bc.near(s, state=bc.interleaved_state(1000)))])
    assert got[0]["ok"] and got[0]["n_camera"] == 57 and got[0]["n_members"] > 600


@pytest.mark.gpu
def test_gpu_track_shapes(solver):
    two, lonely = bc.two_frame_tracks(6002), bc.lonely_frame(6003)
    nobs = np.diff(two["win"]["first_obs"])
    assert (nobs == 2).sum() >= 60 and int((lonely["start"] == 0).sum()) == 2
    got, _ = run_both(solver, [(two, bc.near(two)), (lonely, bc.near(lonely))])
    assert all(g["ok"] for g in got)


@pytest.mark.gpu
def test_gpu_verdict_cases(solver):
    names = ["truth", "near", "far", "same_centre", "on_axis", "behind"]
    got, want = run_both(solver, [verdict_case(k) for k in names])
    by = dict(zip(names, got))
    assert by["truth"]["flags"] & ref.COST and by["near"]["flags"] & ref.CONVERGED and not by["behind"]["flags"] & ref.FINITE and not by["behind"]["ok"]
    assert by["on_axis"]["accepted"] == 0 and by["on_axis"]["iterations"] == 20 and by["same_centre"]["ok"]
    lam = [float(v) for v in want[2]["lambdas"]]                 # the far start: rejected steps, lambda rises at least twice (asserted on the restatement)
    assert sum(1 for a, b in zip(lam, lam[1:]) if b > a) >= 2 and 0 < by["far"]["accepted"] < by["far"]["iterations"]
    run_both(solver, [verdict_case("truth")], cost_threshold=1e-40)
    run_both(solver, [verdict_case("near")], cost_threshold=1e-12)


@pytest.mark.gpu
def test_gpu_one_iteration_and_the_threshold_at_equality(solver):
    s, st = verdict_case("far")
    got, _ = run_both(solver, [(s, st)], ba_iterations=1)
    assert not got[0]["ok"] and got[0]["iterations"] == 1
    half = np.float64(0.5) * np.float64(got[0]["cost1"])
    at, _ = run_both(solver, [(s, st)], ba_iterations=1, cost_threshold=float(half))
    above, _ = run_both(solver, [(s, st)], ba_iterations=1, cost_threshold=float(np.nextafter(half, np.inf)))
    assert not at[0]["ok"] and above[0]["ok"]
    run_both(solver, [(s, st)], ba_iterations=64, function_tolerance=1e-30)


@pytest.mark.gpu
def test_gpu_skipped_windows_next_to_good_ones(solver):
    from vil_fusion_amd.estimator import bundle_adjust
    a, b, c = bc.scene(7300, n_frames=5, n=40, l=2), bc.scene(7301), bc.scene(7302, n_frames=3, n=30, l=0)
    cases = [(a, bc.near(a)), (b, dict(bc.near(b), l=-1)), (c, dict(bc.near(c), chain_ok=False)), (b, bc.near(b))]
    got, _ = run_both(solver, cases)
    assert [g["ok"] for g in got] == [True, False, False, True] and got[1]["l"] == -1 and got[2]["l"] == 0 and got[1]["iterations"] == got[2]["iterations"] == 0
    for k, (s, st) in enumerate(cases):                          # a window computes the same alone as in the batch
        same_result(bundle_adjust(solver, [s["win"]], [st])[0], got[k], ("alone", k))


@pytest.mark.gpu
def test_gpu_256_windows_in_one_call(solver):
    from vil_fusion_amd.estimator import bundle_adjust
    distinct = []
    for i in range(8):
        s = bc.scene(7400 + i, n_frames=3 + i, n=40 + 10 * i, l=i % 3)
        distinct.append((s, bc.near(s) if i != 5 else dict(bc.near(s), l=-1)))
    want = [run_ref(s, st) for s, st in distinct]
    got = bundle_adjust(solver, [distinct[k % 8][0]["win"] for k in range(256)], [distinct[k % 8][1] for k in range(256)])
    assert len(got) == 256
    for k, g in enumerate(got):
        same_result(g, want[k % 8], k)


@pytest.mark.gpu
def test_gpu_construct_equals_chain_then_ba(solver):
    from vil_fusion_amd.estimator import bundle_adjust, construct, global_sfm
    from test_startup_sfm import failing_scene
    none = sc.chain_scene(7501, n_frames=4, n=30, n_full=30)
    none.update(l=-1, rel_R=np.zeros((3, 3)), rel_T=np.zeros(3))
    scenes = [sc.chain_scene(7500, noise_px=0.1), failing_scene(0), none, sc.chain_scene(7502, n_frames=5, n=40, n_full=20, noise_px=0.5)]
    rel = [dict(l=s["l"], R=s["rel_R"], T=s["rel_T"]) for s in scenes]
    wins = [s["win"] for s in scenes]
    both = construct(solver, wins, rel=rel)
    chain = global_sfm(solver, wins, rel=rel, structure=True)
    after = bundle_adjust(solver, wins, [chain_start(ch) for ch in chain])
    assert [b["ok"] for b in both] == [True, False, False, True] and [b["chain"]["ok"] for b in both] == [True, False, False, True]
    assert both[1]["chain"]["fail_frame"] == 2 and both[1]["iterations"] == 0 and both[2]["l"] == -1
    for k in range(4):
        same_result(both[k], after[k], ("construct", k))
        for key in ("ok", "fail_frame", "n_triangulated", "l"):
            assert both[k]["chain"][key] == chain[k][key]
        for g, w in zip(both[k]["chain"]["frames"], chain[k]["frames"]):
            assert all(g[key] == w[key] for key in ("count", "flags", "accepted")) and all(same_bits(g[key], w[key]) for key in ("cost0", "cost1", "R", "t", "Q", "T"))
        ch, want = ref.construct(scenes[k]["win"], scenes[k]["l"], scenes[k]["rel_R"], scenes[k]["rel_T"])
        same_result(both[k], want, ("restatement", k))
    # the chain's own entry point afterwards still answers for its own last call
    again = global_sfm(solver, wins[:1], rel=rel[:1], structure=True)[0]
    assert same_bits(again["positions"], chain[0]["positions"])


@pytest.mark.gpu
def test_gpu_construct_runs_relative_pose_first(solver):
    from vil_fusion_amd.estimator import construct
    import startup_reference as ref1
    s = sc.chain_scene(5600, noise_px=0.1, step=(0.8, 1.0))      # enough parallax for the first stage's gate
    got = construct(solver, [s["win"]], n_hypotheses=128, seed=3)[0]
    r1 = ref1.relative_pose(s["win"], n_hypotheses=128, seed=3)
    assert r1["ok"] and got["l"] == r1["l"] and got["ok"]
    same_result(got, ref.construct(s["win"], r1["l"], r1["R"], r1["T"])[1], "rel=None")
    with pytest.raises(TypeError):
        construct(solver, [s["win"]], rel=[dict(l=s["l"], R=s["rel_R"], T=s["rel_T"])], n_hypotheses=128)
    with pytest.raises(TypeError):
        construct(solver, [s["win"]], no_such_parameter=1)


class _Backend:
    def __init__(self, solver):
        from seq_backends import HipBackend
        self.s, self.hip = solver, HipBackend(solver)

    def align(self, inputs):
        return self.hip.align(inputs)


@pytest.mark.gpu
def test_gpu_initial_structure_on_the_device(solver):
    sq, opts, seq, est = filled_estimator(lambda opts: _Backend(solver))
    frames = est.initial_structure(n_hypotheses=256)
    assert frames is not None
    cpu = RestatedBackend(opts).construct([est.structure_table], n_hypotheses=256)[0]
    same_result(est.structure, cpu, "driven window")
    got = hand_off_differences(sq, opts, seq, est, frames)
    assert all(g <= 2.0 * b for g, b in zip(got, HAND_OFF)), got
    assert est.visual_initial_align(frames)


def raw_call(solver, params, n_windows, cases, null=None, construct=False):
    """vilf_startup_ba (or vilf_startup_construct) with outputs full of a pattern -> (status, outputs untouched?)"""
    from vil_fusion_amd.estimator import startup_default_ba_params, startup_default_sfm_params
    from vil_fusion_amd.lib import lib
    L = lib()
    params = startup_default_ba_params() if params is None else params
    n = max(len(cases), 1)
    W, st, rl, keep = (abi.StartupWindow * n)(), (abi.StartupBaStart * n)(), (abi.StartupResult * n)(), []
    for k, (s, start) in enumerate(cases):
        w = s["win"]
        a = (np.ascontiguousarray(w["start_frame"], dtype=np.int32), np.ascontiguousarray(w["first_obs"], dtype=np.int32), np.ascontiguousarray(w["pts"], dtype=np.float64),
             np.ascontiguousarray(start["R"], dtype=np.float64), np.ascontiguousarray(start["t"], dtype=np.float64), np.ascontiguousarray(start["state"], dtype=np.uint8),
             np.ascontiguousarray(start["positions"], dtype=np.float64))
        keep.append(a)
        W[k].n_frames, W[k].n_features = int(w["n_frames"]), int(w.get("n_features", len(a[0])))
        W[k].start_frame, W[k].first_obs, W[k].pts = a[0].ctypes.data_as(C.POINTER(C.c_int32)), a[1].ctypes.data_as(C.POINTER(C.c_int32)), abi.dptr(a[2])
        st[k].l, st[k].chain_ok = int(start["l"]), 1
        st[k].R = abi.dptr(a[3]) if null != "R" else abi.c_double_p()
        st[k].t, st[k].state, st[k].positions = abi.dptr(a[4]), a[5].ctypes.data_as(C.POINTER(C.c_uint8)), abi.dptr(a[6])
        rl[k].l = int(start["l"])
        rl[k].R[:] = [float(v) for v in np.asarray(s["rel_R"]).reshape(9)]
        rl[k].T[:] = [float(v) for v in np.asarray(s["rel_T"]).reshape(3)]
    out = (abi.StartupBaResult * n)()
    rows = (abi.StartupBaFrame * (n * abi.VILF_MAX_FRAMES))()
    chain = (abi.StartupStructure * n)()
    crow = (abi.StartupFrame * (n * abi.VILF_MAX_FRAMES))()
    bufs = (out, rows, chain, crow)
    for b in bufs:
        C.memset(b, 0x5a, C.sizeof(b))
    pp = None if null == "params" else C.byref(params)
    if construct:
        sp = startup_default_sfm_params()
        rc = L.vilf_startup_construct(solver._h, None if null == "sfm_params" else C.byref(sp), pp, n_windows, None if null == "windows" else W,
                                      None if null == "start" else rl, None if null == "out" else out, rows, chain, crow)
    else:
        rc = L.vilf_startup_ba(solver._h, pp, n_windows, None if null == "windows" else W, None if null == "start" else st, None if null == "out" else out, rows)
    return rc, all(bytes(b) == b"\x5a" * C.sizeof(b) for b in bufs[:4 if construct else 2])


@pytest.mark.gpu
def test_gpu_refusals_leave_the_outputs_untouched(solver):
    from vil_fusion_amd.estimator import startup_default_ba_params as P
    from vil_fusion_amd.lib import lib
    base = bc.scene(7600, n_frames=4, n=30, l=1)
    good = bc.near(base)

    def changed(**kw):
        s, st = dict(base), dict(good, R=good["R"].copy(), t=good["t"].copy(), state=good["state"].copy(), positions=good["positions"].copy())
        s["win"] = dict(base["win"])
        s["win"]["pts"] = base["win"]["pts"].copy()
        for k, v in kw.items():
            if k in ("n_frames", "n_features"):
                s["win"][k] = v
            elif k == "pt":
                s["win"]["pts"][5, 1] = v
            elif k == "l":
                st["l"] = v
            elif k == "R11":
                st["R"][2, 1, 1] = v
            elif k == "t2":
                st["t"][0, 2] = v
            elif k == "X":
                st["positions"][int(np.nonzero(st["state"])[0][3]), 0] = v
            elif k == "state":
                st["state"][int(np.nonzero(st["state"])[0][2])] = v
            elif k == "one_observation":
                start, end = base["start"].copy(), base["end"].copy()
                end[4] = start[4]
                s["win"] = sc.make_window(base["X0"], base["poses"], start, end)
                st["state"][4] = 1
        return s, st

    cases = {
        "null params": (None, 1, [(base, good)], "params"), "null windows": (None, 1, [(base, good)], "windows"), "null start": (None, 1, [(base, good)], "start"),
        "null out": (None, 1, [(base, good)], "out"), "null R": (None, 1, [(base, good)], "R"),
        "n_windows 0": (None, 0, [(base, good)], None), "n_windows too large": (None, abi.VILF_STARTUP_MAX_WINDOWS + 1, [(base, good)], None),
        "n_frames 1": (None, 1, [changed(n_frames=1)], None), "n_features 1001": (None, 1, [changed(n_features=abi.VILF_MAX_FEATURES + 1)], None),
        "nan point": (None, 1, [changed(pt=np.nan)], None), "l -2": (None, 1, [changed(l=-2)], None), "l newest": (None, 1, [changed(l=3)], None),
        "R nan": (None, 1, [changed(R11=np.nan)], None), "t inf": (None, 1, [changed(t2=np.inf)], None), "X nan": (None, 1, [changed(X=np.nan)], None),
        "state 2": (None, 1, [changed(state=2)], None), "a member with one observation": (None, 1, [changed(one_observation=True)], None),
        "iterations 0": (P(ba_iterations=0), 1, [(base, good)], None), "iterations 65": (P(ba_iterations=65), 1, [(base, good)], None),
        "lambda 0": (P(lambda0=0.0), 1, [(base, good)], None), "lambda nan": (P(lambda0=float("nan")), 1, [(base, good)], None),
        "tolerance 0": (P(function_tolerance=0.0), 1, [(base, good)], None), "tolerance inf": (P(function_tolerance=float("inf")), 1, [(base, good)], None),
        "threshold -1": (P(cost_threshold=-1.0), 1, [(base, good)], None), "threshold nan": (P(cost_threshold=float("nan")), 1, [(base, good)], None),
        "second window bad": (None, 2, [(base, good), changed(l=3)], None),
    }
    for name, (params, n, cs, null) in cases.items():
        rc, clean = raw_call(solver, params, n, cs, null)
        assert rc == abi.VILF_ERR_INVALID_ARGUMENT and clean, (name, rc, clean)
    rc, clean = raw_call(solver, None, 1, [changed(l=2)])        # l = n_frames - 2 is the last valid one
    assert rc == abi.VILF_OK and not clean
    for name, (params, n, cs, null) in {"null sfm params": (None, 1, [(base, good)], "sfm_params"), "null params": (None, 1, [(base, good)], "params"),
                                        "null rel": (None, 1, [(base, good)], "start"), "null out": (None, 1, [(base, good)], "out"),
                                        "n_windows 0": (None, 0, [(base, good)], None), "l newest": (None, 1, [changed(l=3)], None),
                                        "iterations 65": (P(ba_iterations=65), 1, [(base, good)], None), "threshold 0": (P(cost_threshold=0.0), 1, [(base, good)], None),
                                        "nan point": (None, 1, [changed(pt=np.nan)], None)}.items():
        rc, clean = raw_call(solver, params, n, cs, null, construct=True)
        assert rc == abi.VILF_ERR_INVALID_ARGUMENT and clean, ("construct", name, rc, clean)
    # the structure of a refused call is not there to fetch, that of a good call is, with 0 behind n_features
    L, NX = lib(), abi.VILF_MAX_FEATURES
    got, _ = run_both(solver, [(base, good)])
    state = np.full((1, NX), 7, dtype=np.uint8); pos = np.full((1, NX, 3), 7.0)
    assert L.vilf_startup_get_ba_structure(solver._h, 2, state.ctypes.data_as(C.POINTER(C.c_uint8)), abi.dptr(pos)) == abi.VILF_ERR_INVALID_ARGUMENT
    assert (state == 7).all() and (pos == 7.0).all()
    assert L.vilf_startup_get_ba_structure(solver._h, 1, state.ctypes.data_as(C.POINTER(C.c_uint8)), abi.dptr(pos)) == 0
    assert np.array_equal(state[0, :30], got[0]["state"]) and not state[0, 30:].any() and not pos[0, 30:].any()


@pytest.mark.gpu
def test_gpu_full_size_stage_times(solver):
    from vil_fusion_amd.estimator import bundle_adjust, construct, global_sfm, startup_ba_profile, startup_sfm_profile
    s = sc.chain_scene(5700, n=1000, n_full=400, noise_px=0.1)
    rel = dict(l=s["l"], R=s["rel_R"], T=s["rel_T"])
    assert s["l"] == 5
    for W in (1, 256):
        wins, rels = [s["win"]] * W, [rel] * W
        construct(solver, wins, rel=rels)                        # allocations and the first launch
        starts = [chain_start(global_sfm(solver, wins[:1], rel=rels[:1], structure=True)[0])] * W
        bundle_adjust(solver, wins, starts, ba_iterations=20, function_tolerance=1e-30)
        solver.set_profiling(True)
        try:
            r = construct(solver, wins, rel=rels)
            ms_c, cnt_c = startup_ba_profile(solver)
            ms_s, cnt_s = startup_sfm_profile(solver)
            solver.set_profiling(False)
            solver.set_profiling(True)
            full = bundle_adjust(solver, wins, starts, ba_iterations=20, function_tolerance=1e-30)
            ms_f, cnt_f = startup_ba_profile(solver)
        finally:
            solver.set_profiling(False)
        print(f"GlobalSFM construct, 11 frames, 1000 features, l = 5, {W} window(s), one run [ms]: su_sfm_chain {ms_s[0]:.3f}, su_sfm_ba {ms_c[0]:.3f} "
              f"({r[0]['iterations']} iterations); su_sfm_ba alone with all 20 iterations {ms_f[0]:.3f}")
        assert cnt_c == [1] and cnt_s[0] == 1 and cnt_f == [1] and all(np.isfinite(v) and v >= 0 for v in ms_c + ms_f) and all(x["ok"] for x in r)
        assert all(x["iterations"] == 20 for x in full)
