"""The second stage of the visual start-up, GlobalSFM's frame chain (include/vilfusion.h, "Visual start-up: GlobalSFM frame chain").

CPU tests: the bookkeeping of the numpy restatement (sfm_reference.py) against a plain second walk written from initial_sfm.cpp:156-217, what the restatement is
worth against ground truth and against independent solves (numpy's SVD, scipy's least_squares), the edges of the chain, degenerate input, the ctypes layouts.
GPU tests: the C ABI against the restatement, every integer and every bit.

The accuracy bounds are twice, the solver-difference bounds ten times what the restatement itself showed on these scenes (the tables below and DESIGN.md §3o);
none of them comes from the HIP path."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import sfm_cases as sc
import sfm_reference as ref
from vil_fusion_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_ref(s, **params):
    return ref.global_sfm(s["win"], s["l"], s["rel_R"], s["rel_T"], **params)


# ---- the bookkeeping against a plain second walk ---------------------------------------------------------------------------------------------------------
def plain_walk(win, l):
    """initial_sfm.cpp:156-217 on lists of (frame, point) observations, the shape of sfm_f, without any arithmetic: which features each step triangulates
    and which each PnP uses. Every triangulation is taken to succeed and every PnP too (the poses are the ground truth's)."""
    nf, newest = int(win["n_frames"]), int(win["n_frames"]) - 1
    sfm_f = []
    for f in range(len(win["start_frame"])):
        a, b = int(win["first_obs"][f]), int(win["first_obs"][f + 1])
        sfm_f.append(dict(state=False, observation=[(int(win["start_frame"][f]) + o, tuple(win["pts"][a + o])) for o in range(b - a)]))
    trace = []

    def two_frames(frame0, frame1):
        done = []
        for j, it in enumerate(sfm_f):
            if it["state"]:
                continue
            has_0 = any(k == frame0 for k, _ in it["observation"])
            has_1 = any(k == frame1 for k, _ in it["observation"])
            if has_0 and has_1:
                it["state"] = True
                done.append(j)
        trace.append(("tri", frame0, frame1, done))

    def pnp(i):
        trace.append(("pnp", i, [j for j, it in enumerate(sfm_f) if it["state"] and any(k == i for k, _ in it["observation"])]))

    for i in range(l, nf - 1):
        if i > l:
            pnp(i)
        two_frames(i, newest)
    for i in range(l + 1, nf - 1):
        two_frames(l, i)
    for i in range(l - 1, -1, -1):
        pnp(i)
        two_frames(i, l)
    rest = []
    for j, it in enumerate(sfm_f):
        if not it["state"] and len(it["observation"]) >= 2:
            it["state"] = True
            rest.append(j)
    trace.append(("rest", rest))
    return trace, [it["state"] for it in sfm_f]


def mixed_scene(seed, n_frames, l):
    """mixed tracks: full ones, random ones, and by construction features that start after l, end before the newest, are seen in neither, have one observation
    and have none"""
    s = sc.chain_scene(seed, n_frames=n_frames, n=90, n_full=40, l=l)
    rng = np.random.default_rng(seed + 1)
    start, end = s["start"].copy(), s["end"].copy()
    pick = rng.permutation(90)[:12]
    newest = n_frames - 1
    start[pick[0:3]] = min(l + 1, newest); end[pick[0:3]] = newest                       # start after l
    start[pick[3:6]] = 0; end[pick[3:6]] = max(newest - 1, 0)                             # end before the newest
    if l + 1 <= newest - 1:
        start[pick[6:8]] = l + 1; end[pick[6:8]] = newest - 1                             # seen in neither l nor the newest
    start[pick[8:10]] = np.minimum(rng.integers(0, n_frames, 2), newest); end[pick[8:10]] = start[pick[8:10]]      # one observation
    start[pick[10:12]] = 1; end[pick[10:12]] = 0                                           # none
    s["win"] = sc.make_window(s["X0"], s["poses"], start, end)
    s["start"], s["end"] = start, end
    return s


@pytest.mark.parametrize("n_frames,l", [(11, 5), (11, 0), (11, 9), (6, 2), (3, 1), (2, 0)])
def test_structure_walk_equals_a_plain_second_walk(n_frames, l):
    s = mixed_scene(3000 + 10 * n_frames + l, n_frames, l)
    nobs = s["end"] - s["start"] + 1
    if n_frames >= 6:
        assert (s["start"] > l).any() and (s["end"] < n_frames - 1).any() and (nobs == 1).any() and (nobs == 0).any()
    r = run_ref(s, min_pnp_count=0)
    want, state = plain_walk(s["win"], l)
    assert r["ok"] and r["trace"] == want
    assert [bool(v) for v in r["state"]] == state and not r["state"][nobs < 2].any() and r["state"][nobs >= 2].all()
    assert r["n_triangulated"] == int((nobs >= 2).sum())
    kinds = [t[0] for t in want]
    assert kinds.count("pnp") == n_frames - 2 and kinds.count("tri") == (n_frames - 1 - l) + (n_frames - 2 - l) + l and kinds[-1] == "rest"


# ---- accuracy against ground truth -------------------------------------------------------------------------------------------------------------------------
NOISES = (0.0, 0.1, 0.5)
# measured with the restatement on chain_scene(2000 + 10 * noise, noise_px=noise) (11 frames, 150 features of which 60 full-length, l = 5, 1 - 2 deg and
# 0.3 - 0.5 m per frame), one run, rounded up to two digits: the largest rotation error of a frame [deg], the largest position error of a frame in units of the
# baseline (l, newest), the median and the largest relative error of a point. The test asserts twice these. The largest point error belongs to the features
# with the least parallax (two neighbouring frames, 40 m away); with noise it is theirs, not the method's.
ACCURACY = {
    0.0: (6.4e-07, 7.6e-08, 2.2e-08, 9.5e-07),
    0.1: (0.021, 0.0039, 0.0053, 0.093),
    0.5: (0.097, 0.0096, 0.017, 0.44),
}


@pytest.fixture(scope="module")
def accuracy_runs():
    out = {}
    for nz in NOISES:
        s = sc.chain_scene(2000 + int(10 * nz), noise_px=nz)
        out[nz] = (s, run_ref(s))
    return out


def errors(s, r):
    rot = [sc.rot_err_deg(f["Q"], s["Q"][k]) for k, f in enumerate(r["frames"])]
    pos = [float(np.linalg.norm(f["T"] - s["T"][k])) for k, f in enumerate(r["frames"])]
    ok = r["state"] == 1
    pt = np.linalg.norm(r["positions"][ok] - s["X"][ok], axis=1) / np.linalg.norm(s["X"][ok], axis=1)
    return rot, pos, pt


def test_restatement_accuracy_against_ground_truth(accuracy_runs):
    bad = []
    for nz, (s, r) in sorted(accuracy_runs.items()):
        assert r["ok"] and r["n_triangulated"] == 150 and abs(np.linalg.norm(s["rel_T"]) - 1.0) < 1e-12
        rot, pos, pt = errors(s, r)
        for k, f in enumerate(r["frames"]):
            print(f"noise {nz:.1f} px frame {k:2d}: members {f['count']:3d} flags {f['flags']:2d} accepted {f['accepted']:2d} cost {f['cost0']:.3e} -> {f['cost1']:.3e} "
                  f"rot {rot[k]:.3e} deg pos {pos[k]:.3e} baselines")
        got = (max(rot), max(pos), float(np.median(pt)), float(pt.max()))
        print(f"noise {nz:.1f} px: rot {got[0]:.3e} deg, pos {got[1]:.3e}, points median {got[2]:.3e} max {got[3]:.3e}")
        if any(g > 2.0 * b for g, b in zip(got, ACCURACY[nz])):
            bad.append((nz, got))
        assert all(f["accepted"] >= 1 for f in r["frames"] if f["flags"] & ref.PNP)
    assert not bad, bad


# ---- against independent solves, on the restatement's own members ---------------------------------------------------------------------------------------
# measured as above on the no-noise and the 0.5 px scene, one run, rounded up to two digits: the largest relative difference of a triangulated point to the
# right singular vector of numpy's SVD of the same 4 x 4 matrix, the largest rotation [deg] and translation [baselines] difference of a frame to scipy's
# least_squares (method lm, tolerances 1e-15) on the same float32 members from the same guess. The test asserts ten times these.
SOLVER_DIFFERENCE = {
    0.0: (4.2e-13, 2.0e-11, 5.3e-12),
    0.5: (2.2e-13, 4.7e-07, 2.0e-08),
}


def rodrigues(w):
    th = np.linalg.norm(w)
    if th < 1e-300:
        return np.eye(3)
    return sc.rot(w / th, np.rad2deg(th))


def scipy_pnp(X, u, R0, t0):
    from scipy.optimize import least_squares

    def res(x):
        p = X @ (rodrigues(x[:3]) @ R0).T + x[3:]
        return (p[:, :2] / p[:, 2:3] - u).ravel()
    sol = least_squares(res, np.concatenate([np.zeros(3), t0]), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
    return rodrigues(sol.x[:3]) @ R0, sol.x[3:]


def solver_differences(s, r):
    start, first, nobs, pts = ref.table(s["win"])
    P = [np.hstack([f["R"], f["t"].reshape(3, 1)]) for f in r["frames"]]
    dp, dr, dt = 0.0, 0.0, 0.0
    for step in r["trace"]:
        if step[0] == "pnp":
            i, members = step[1], np.array(step[2])
            guess = i - 1 if i > r["l"] else i + 1
            X = r["positions"][members].astype(np.float32).astype(np.float64)
            u = pts[first[members] + i - start[members]].astype(np.float32).astype(np.float64)
            Rs, ts = scipy_pnp(X, u, r["frames"][guess]["R"], r["frames"][guess]["t"])
            dr, dt = max(dr, sc.rot_err_deg(r["frames"][i]["R"], Rs)), max(dt, float(np.linalg.norm(r["frames"][i]["t"] - ts)))
            continue
        for f in step[-1]:
            a, b = (step[1], step[2]) if step[0] == "tri" else (start[f], start[f] + nobs[f] - 1)
            A = ref.design_matrix(P[a], P[b], pts[first[f] + a - start[f]], pts[first[f] + b - start[f]])
            v = np.linalg.svd(A)[2][3]
            dp = max(dp, float(np.linalg.norm(v[:3] / v[3] - r["positions"][f]) / np.linalg.norm(r["positions"][f])))
    return dp, dr, dt


def test_restatement_against_independent_solves(accuracy_runs):
    bad = []
    for nz in (0.0, 0.5):
        got = solver_differences(*accuracy_runs[nz])
        print(f"noise {nz:.1f} px: points vs numpy SVD {got[0]:.3e} relative, PnP vs scipy least_squares {got[1]:.3e} deg, {got[2]:.3e} baselines")
        if any(g > 10.0 * b for g, b in zip(got, SOLVER_DIFFERENCE[nz])):
            bad.append((nz, got))
    assert not bad, bad


# ---- the edges of the chain ---------------------------------------------------------------------------------------------------------------------------------
def cut_scene(m, seed=4100):
    """three frames, l = 0, 40 features; only m of them are seen before the newest frame, so (0, 2) triangulates m and the PnP of frame 1 has exactly m members"""
    s = sc.chain_scene(seed, n_frames=3, n=40, n_full=40, l=0)
    start, end = np.zeros(40, dtype=np.int32), np.full(40, 2, dtype=np.int32)
    start[m:] = 2
    s["win"] = sc.make_window(s["X0"], s["poses"], start, end)
    return s


def test_edges_of_the_chain():
    s = sc.chain_scene(4001, n_frames=2, n=30, n_full=30, l=0)                   # one triangulation, no PnP
    r = run_ref(s)
    assert r["ok"] and [t[0] for t in r["trace"]] == ["tri", "rest"] and r["n_triangulated"] == 30 and all(f["flags"] == ref.FIXED | ref.POSE for f in r["frames"])
    s = sc.chain_scene(4002, n_frames=6, n=60, n_full=40, l=0)                   # no backward walk
    r = run_ref(s)
    assert r["ok"] and [t[1] for t in r["trace"] if t[0] == "pnp"] == [1, 2, 3, 4]
    s = sc.chain_scene(4003, n_frames=6, n=60, n_full=40, l=4)                   # no forward PnP
    r = run_ref(s)
    assert r["ok"] and [t[1] for t in r["trace"] if t[0] == "pnp"] == [3, 2, 1, 0] and r["trace"][1][:2] == ("pnp", 3)
    for m, fails, few in ((9, True, True), (10, False, True), (14, False, True), (15, False, False)):
        r = run_ref(cut_scene(m))
        f = r["frames"][1]
        assert f["count"] == m and bool(f["flags"] & ref.FAIL_COUNT) == fails and bool(f["flags"] & ref.FEW) == few, (m, f["flags"])
        assert r["ok"] == (not fails) and r["fail_frame"] == (1 if fails else -1)
        if fails:
            assert not f["R"].any() and not f["flags"] & ref.POSE and r["trace"][-1][0] == "pnp" and r["n_triangulated"] == m       # step 5 is not run
    r = ref.global_sfm(s["win"], -1, np.zeros((3, 3)), np.zeros(3))             # rel.l = -1
    assert not r["ok"] and r["fail_frame"] == -1 and r["n_triangulated"] == 0 and not r["trace"] and all(f["flags"] == 0 for f in r["frames"])


def failing_scene(forward):
    """11 frames, l = 5, 8 full tracks; the other 52 start at frame 6 (forward: (5, 10) triangulates 8, the PnP of frame 6 fails; a forward failure can only
    be the first frame's, because what (l, newest) triangulates is seen in every frame between) or at frame 3 (backward: the frames 4 and 3 have 60 members,
    frame 2 has 8)"""
    s = sc.chain_scene(4200 + forward, n_frames=11, n=60, n_full=60, l=5)
    start, end = np.zeros(60, dtype=np.int32), np.full(60, 10, dtype=np.int32)
    start[8:] = 6 if forward else 3
    s["win"] = sc.make_window(s["X0"], s["poses"], start, end)
    return s


@pytest.mark.parametrize("forward", [1, 0])
def test_a_failing_frame_ends_the_chain(forward):
    r = run_ref(failing_scene(forward))
    at = 6 if forward else 2
    assert not r["ok"] and r["fail_frame"] == at and r["frames"][at]["count"] == 8 and r["frames"][at]["flags"] & ref.FAIL_COUNT
    reached = {5, 10} if forward else {5, 10, 6, 7, 8, 9, 4, 3}
    for k, f in enumerate(r["frames"]):
        assert bool(f["flags"] & ref.POSE) == (k in reached), k
        if k not in reached:
            assert not f["R"].any() and not f["t"].any() and not f["Q"].any() and not f["T"].any()
    assert r["trace"][-1][:2] == ("pnp", at) and not any(t[0] == "rest" for t in r["trace"])


# ---- defined on degenerate input ----------------------------------------------------------------------------------------------------------------------------
def degenerate_scene(name):
    s = sc.chain_scene(4300, n_frames=5, n=40, n_full=40, l=2, planar=(name == "planar"))
    if name == "same_point":
        s["win"] = sc.make_window(np.tile(s["X0"][:1], (40, 1)), s["poses"])
    elif name == "no_translation":
        s["rel_T"] = np.zeros(3)
    elif name == "parallel_rays":
        # feature 0 is at the same image point in l and the newest while the camera only translated between them: the rays are parallel
        s["rel_R"] = np.eye(3)
        p = s["win"]["pts"].copy()
        p[4] = p[2]
        s["win"]["pts"] = p
    return s


def check_defined(r):
    for f in r["frames"]:
        if f["flags"] & ref.POSE:
            for k in ("R", "t", "Q", "T", "cost0", "cost1"):
                assert np.isfinite(f[k]).all(), k
        else:
            assert not f["R"].any() and not f["t"].any() and not f["Q"].any() and not f["T"].any()
    assert np.isfinite(r["positions"]).all() and not r["positions"][r["state"] == 0].any()
    assert r["ok"] == (r["fail_frame"] < 0 and r["l"] >= 0) and r["n_triangulated"] == int(r["state"].sum())
    if r["ok"]:
        assert all(f["flags"] & ref.POSE for f in r["frames"])


@pytest.mark.parametrize("name", ["same_point", "planar", "no_translation", "parallel_rays"])
def test_degenerate_input_is_defined(name):
    s = degenerate_scene(name)
    r = run_ref(s)
    check_defined(r)
    print(name, "ok", r["ok"], "fail_frame", r["fail_frame"], "triangulated", r["n_triangulated"], "flags", [f["flags"] for f in r["frames"]])
    if name == "planar":
        assert r["ok"]


def test_an_lm_step_is_rejected_in_the_restatement(accuracy_runs):
    s, r = accuracy_runs[0.1]
    f = r["frames"][0]
    assert 0 < f["accepted"] < 10
    lam = [float(v) for v in f["lambdas"]]
    assert any(b > a for a, b in zip(lam, lam[1:])) and any(b < a for a, b in zip(lam, lam[1:]))


def test_ctypes_mirrors_of_the_sfm_match_the_c_layout(tmp_path):
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "vilfusion.h"', "int main(void) {"]
    checks = []
    for cname, ct in abi.STARTUP_SFM_LAYOUTS.items():
        prog.append(f'  printf("%zu\\n", sizeof({cname}));')
        checks.append((cname, "sizeof", C.sizeof(ct)))
        for fname, _ in ct._fields_:
            prog.append(f'  printf("%zu\\n", offsetof({cname}, {fname}));')
            checks.append((cname, fname, getattr(ct, fname).offset))
    for name in ("VILF_SFM_FIXED", "VILF_SFM_PNP", "VILF_SFM_FEW", "VILF_SFM_FAIL_COUNT", "VILF_SFM_FAIL_FINITE", "VILF_SFM_POSE", "VILF_STARTUP_MAX_PROBLEMS"):
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
    assert (ref.FIXED, ref.PNP, ref.FEW, ref.FAIL_COUNT, ref.FAIL_FINITE, ref.POSE) == (abi.VILF_SFM_FIXED, abi.VILF_SFM_PNP, abi.VILF_SFM_FEW, abi.VILF_SFM_FAIL_COUNT,
                                                                                       abi.VILF_SFM_FAIL_FINITE, abi.VILF_SFM_POSE)
    assert ref.MAX_FRAMES == abi.VILF_MAX_FRAMES and ref.MAX_FEATURES == abi.VILF_MAX_FEATURES


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


def same_frame(got, want, where):
    for k in ("count", "flags", "accepted"):
        assert got[k] == want[k], (where, k, got[k], want[k])
    for k in ("cost0", "cost1", "R", "t", "Q", "T"):
        assert same_bits(got[k], want[k]), (where, k, got[k], want[k])


def same_structure(got, want, where):
    for k in ("ok", "fail_frame", "n_triangulated", "l"):
        assert got[k] == want[k], (where, k, got[k], want[k])
    assert len(got["frames"]) == len(want["frames"])
    for i, (g, w) in enumerate(zip(got["frames"], want["frames"])):
        same_frame(g, w, (where, i))
    assert np.array_equal(got["state"], want["state"]), (where, "state")
    assert same_bits(got["positions"], want["positions"]), (where, "positions")


def rel_of(s):
    return dict(l=s["l"], R=s["rel_R"], T=s["rel_T"])


def run_both(solver, scenes, **params):
    from vil_fusion_amd.estimator import global_sfm
    got = global_sfm(solver, [s["win"] for s in scenes], rel=[rel_of(s) for s in scenes], structure=True, **params)
    want = [run_ref(s, **params) for s in scenes]
    for k, (g, w) in enumerate(zip(got, want)):
        same_structure(g, w, k)
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize("n", [9, 10, 11, 255, 256, 257, 1000])
def test_gpu_feature_counts(solver, n):
    s = sc.chain_scene(5000 + n, n_frames=3, n=n, n_full=n, l=0, noise_px=0.1)
    got, _ = run_both(solver, [s])
    assert got[0]["frames"][1]["count"] == n and got[0]["ok"] == (n >= 10) and got[0]["fail_frame"] == (-1 if n >= 10 else 1)


@pytest.mark.gpu
@pytest.mark.parametrize("n_frames,l", [(2, 0), (3, 0), (3, 1), (11, 0), (11, 5), (11, 9)])
def test_gpu_frame_counts_and_l(solver, n_frames, l):
    s = mixed_scene(5100 + 10 * n_frames + l, n_frames, l)
    got, _ = run_both(solver, [s])
    assert got[0]["ok"] and sum(1 for f in got[0]["frames"] if f["flags"] & ref.PNP) == n_frames - 2


@pytest.mark.gpu
@pytest.mark.parametrize("iterations", [1, 10])
def test_gpu_pnp_iterations_and_a_rejected_step(solver, iterations):
    s = sc.chain_scene(2001, noise_px=0.1)                       # the 0.1 px scene of the accuracy table: its frame 0 rejects steps (checked on the CPU above)
    got, want = run_both(solver, [s], pnp_iterations=iterations)
    acc = [f["accepted"] for f in got[0]["frames"] if f["flags"] & ref.PNP]
    assert all(a == 1 for a in acc) if iterations == 1 else all(0 < a < 10 for a in acc)


@pytest.mark.gpu
def test_gpu_three_windows_of_different_sizes(solver):
    from vil_fusion_amd.estimator import global_sfm
    none = sc.chain_scene(5201, n_frames=4, n=30, n_full=30)
    none.update(l=-1, rel_R=np.zeros((3, 3)), rel_T=np.zeros(3))
    scenes = [sc.chain_scene(5200, noise_px=0.1), failing_scene(0), none, sc.chain_scene(5202, n_frames=5, n=40, n_full=20)]
    got, _ = run_both(solver, scenes)
    assert [g["ok"] for g in got] == [True, False, False, True] and got[1]["fail_frame"] == 2 and got[2]["fail_frame"] == -1 and got[2]["n_triangulated"] == 0
    assert not any(f["flags"] for f in got[2]["frames"])
    for k, s in enumerate(scenes):                               # a window computes the same alone as in the batch
        alone = global_sfm(solver, [s["win"]], rel=[rel_of(s)], structure=True)[0]
        same_structure(alone, got[k], ("alone", k))


@pytest.mark.gpu
def test_gpu_degenerate_scenes(solver):
    got, _ = run_both(solver, [degenerate_scene(k) for k in ("same_point", "planar", "no_translation", "parallel_rays")])
    for g in got:
        check_defined(g)


@pytest.mark.gpu
def test_gpu_no_stale_state(solver):
    from vil_fusion_amd.estimator import BackendSolver, global_sfm
    from vil_fusion_amd.lib import lib
    big = [sc.chain_scene(5300, n=1000, n_full=400), sc.chain_scene(5301), sc.chain_scene(5302)]
    small = [sc.chain_scene(5303, n_frames=3, n=30, n_full=30, l=0)]
    global_sfm(solver, [s["win"] for s in big], rel=[rel_of(s) for s in big], structure=True)
    got, _ = run_both(solver, small)
    fresh = BackendSolver()
    try:
        same_structure(global_sfm(fresh, [small[0]["win"]], rel=[rel_of(small[0])], structure=True)[0], got[0], "fresh handle")
    finally:
        fresh.close()
    # the raw buffers: frames the window does not have and features behind n_features are 0
    L, NF, NX = lib(), abi.VILF_MAX_FRAMES, abi.VILF_MAX_FEATURES
    state = np.full((1, NX), 7, dtype=np.uint8); pos = np.full((1, NX, 3), 7.0)
    assert L.vilf_startup_get_structure(solver._h, 1, state.ctypes.data_as(C.POINTER(C.c_uint8)), abi.dptr(pos)) == 0
    assert state[0, :30].all() and not state[0, 30:].any() and not pos[0, 30:].any()
    assert L.vilf_startup_get_structure(solver._h, 2, state.ctypes.data_as(C.POINTER(C.c_uint8)), abi.dptr(pos)) == abi.VILF_ERR_INVALID_ARGUMENT
    rows = raw_call(solver, None, 1, [small[0]], keep_rows=True)
    assert all(bytes(rows[i]) == bytes(C.sizeof(abi.StartupFrame)) for i in range(3, NF))


def raw_call(solver, params, n_windows, scenes, null=None, keep_rows=False):
    """vilf_startup_sfm with outputs full of a pattern -> (status, outputs untouched?)"""
    from vil_fusion_amd.estimator import startup_default_sfm_params
    from vil_fusion_amd.lib import lib
    L = lib()
    params = startup_default_sfm_params() if params is None else params
    n = max(len(scenes), 1)
    W, rl, keep = (abi.StartupWindow * n)(), (abi.StartupResult * n)(), []
    for k, s in enumerate(scenes):
        w = s["win"]
        st, fo, pt = (np.ascontiguousarray(w["start_frame"], dtype=np.int32), np.ascontiguousarray(w["first_obs"], dtype=np.int32),
                      np.ascontiguousarray(w["pts"], dtype=np.float64))
        keep.append((st, fo, pt))
        W[k].n_frames, W[k].n_features = int(w["n_frames"]), int(w.get("n_features", len(st)))
        W[k].start_frame, W[k].first_obs = st.ctypes.data_as(C.POINTER(C.c_int32)), fo.ctypes.data_as(C.POINTER(C.c_int32))
        W[k].pts = abi.dptr(pt) if null != "pts" else abi.c_double_p()
        rl[k].l = int(s["l"])
        rl[k].R[:] = [float(v) for v in np.asarray(s["rel_R"]).reshape(9)]
        rl[k].T[:] = [float(v) for v in np.asarray(s["rel_T"]).reshape(3)]
    out = (abi.StartupStructure * n)()
    rows = (abi.StartupFrame * (n * abi.VILF_MAX_FRAMES))()
    C.memset(out, 0x5a, C.sizeof(out)); C.memset(rows, 0x5a, C.sizeof(rows))
    rc = L.vilf_startup_sfm(solver._h, None if null == "params" else C.byref(params), n_windows, None if null == "windows" else W, None if null == "rel" else rl,
                            None if null == "out" else out, rows)
    if keep_rows:
        assert rc == abi.VILF_OK
        return rows
    return rc, bytes(out) == b"\x5a" * C.sizeof(out) and bytes(rows) == b"\x5a" * C.sizeof(rows)


@pytest.mark.gpu
def test_gpu_refusals_leave_the_outputs_untouched(solver):
    from vil_fusion_amd.estimator import startup_default_sfm_params as P
    from vil_fusion_amd.lib import lib
    base = sc.chain_scene(5400, n_frames=4, n=30, n_full=20)

    def changed(**kw):
        s = dict(base)
        s["win"] = dict(base["win"])
        s["win"]["pts"] = base["win"]["pts"].copy()
        for k, v in kw.items():
            if k in ("n_frames", "n_features"):
                s["win"][k] = v
            elif k == "pt":
                s["win"]["pts"][5, 1] = v
            else:
                s[k] = v
        return s

    bad_R, bad_T = base["rel_R"].copy(), base["rel_T"].copy()
    bad_R[1, 1], bad_T[2] = np.nan, np.inf
    cases = {
        "null params": (None, 1, [base], "params"), "null windows": (None, 1, [base], "windows"), "null rel": (None, 1, [base], "rel"), "null out": (None, 1, [base], "out"),
        "null pts": (None, 1, [base], "pts"), "n_windows 0": (None, 0, [base], None), "n_windows too large": (None, abi.VILF_STARTUP_MAX_WINDOWS + 1, [base], None),
        "n_frames 1": (None, 1, [changed(n_frames=1)], None), "n_features 1001": (None, 1, [changed(n_features=abi.VILF_MAX_FEATURES + 1)], None),
        "nan point": (None, 1, [changed(pt=np.nan)], None),
        "l -2": (None, 1, [changed(l=-2)], None), "l newest": (None, 1, [changed(l=3)], None),
        "R nan": (None, 1, [changed(rel_R=bad_R)], None), "T inf": (None, 1, [changed(rel_T=bad_T)], None),
        "iterations 0": (P(pnp_iterations=0), 1, [base], None), "iterations 65": (P(pnp_iterations=65), 1, [base], None),
        "min count -1": (P(min_pnp_count=-1), 1, [base], None), "warn count -1": (P(warn_pnp_count=-1), 1, [base], None),
        "lambda 0": (P(lambda0=0.0), 1, [base], None), "lambda nan": (P(lambda0=float("nan")), 1, [base], None),
        "second window bad": (None, 2, [base, changed(l=3)], None),
    }
    for name, (params, n, scenes, null) in cases.items():
        rc, clean = raw_call(solver, params, n, scenes, null)
        assert rc == abi.VILF_ERR_INVALID_ARGUMENT and clean, (name, rc, clean)
    rc, clean = raw_call(solver, None, 1, [changed(l=2)])        # l = n_frames - 2 is the last valid one
    assert rc == abi.VILF_OK and not clean
    # the PnP entry point: the rows keep their pattern
    L = lib()
    X, u = np.ascontiguousarray(base["X"][:20]), np.zeros((20, 2))
    for name, (n, mc, x00, params) in {"n -1": (-1, 6, 1.0, P()), "n 1001": (1001, 6, 1.0, P()), "min_count -1": (20, -1, 1.0, P()), "nan": (20, 6, np.nan, P()),
                                      "iterations 0": (20, 6, 1.0, P(pnp_iterations=0))}.items():
        q = (abi.StartupPnpProblem * 1)()
        Xc = X.copy(); Xc[0, 0] = x00
        q[0].n, q[0].min_count, q[0].pts3, q[0].pts2 = n, mc, abi.dptr(Xc), abi.dptr(u)
        q[0].R[:] = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]
        out = (abi.StartupFrame * 1)()
        C.memset(out, 0x5a, C.sizeof(out))
        assert L.vilf_startup_pnp(solver._h, C.byref(params), 1, q, out) == abi.VILF_ERR_INVALID_ARGUMENT and bytes(out) == b"\x5a" * C.sizeof(out), name
    run_both(solver, [base])                                     # a valid call afterwards still works


def pnp_problem(seed, n, min_count=6):
    """n points 5 - 50 m in front of a camera 1.5 deg and 0.4 m from the guess, 0.1 px of noise"""
    rng = np.random.default_rng(seed)
    X = sc.points3d(rng, n)
    R, c = sc.rot(sc.RT_AXIS, 1.5), 0.4 * sc.T_DIR
    p = (X - c) @ R
    u = p[:, :2] / p[:, 2:3] + rng.normal(0, 0.1 / sc.FOCAL, (n, 2))
    return dict(pts3=X, pts2=u, R=np.eye(3), t=np.zeros(3), min_count=min_count)


@pytest.mark.gpu
def test_gpu_pnp_batch(solver):
    from vil_fusion_amd.estimator import frame_pnp
    probs = [pnp_problem(5500 + n, n) for n in (6, 64, 65, 1000)] + [pnp_problem(5510, 5), pnp_problem(5511, 12, min_count=13)]
    got = frame_pnp(solver, probs)
    for k, (g, q) in enumerate(zip(got, probs)):
        want = ref.pnp(q["pts3"], q["pts2"], q["R"], q["t"], q["min_count"])
        same_frame(g, want, ("problem", k))
    assert [bool(g["flags"] & ref.POSE) for g in got] == [True, True, True, True, False, False] and got[4]["flags"] & ref.FAIL_COUNT and got[0]["flags"] & ref.FEW
    assert sc.rot_err_deg(got[3]["R"].T, sc.rot(sc.RT_AXIS, 1.5)) < 0.05
    # the one chain frame with the same members and guess gives the same bits through both entry points
    s = sc.chain_scene(2001, noise_px=0.1)
    chain, want = run_both(solver, [s])
    step = next(t for t in want[0]["trace"] if t[0] == "pnp" and t[1] == 3)
    start, first, _, pts = ref.table(s["win"])
    members = np.array(step[2])
    one = frame_pnp(solver, [dict(pts3=chain[0]["positions"][members], pts2=pts[first[members] + 3 - start[members]], R=chain[0]["frames"][4]["R"],
                                  t=chain[0]["frames"][4]["t"], min_count=10)])[0]
    same_frame(one, chain[0]["frames"][3], "chain frame 3 through vilf_startup_pnp")


@pytest.mark.gpu
def test_gpu_global_sfm_runs_relative_pose_first(solver):
    from vil_fusion_amd.estimator import global_sfm
    import startup_reference as ref1
    s = sc.chain_scene(5600, noise_px=0.1, step=(0.8, 1.0))      # enough parallax for the first stage's gate
    got = global_sfm(solver, [s["win"]], structure=True, n_hypotheses=128, seed=3)[0]
    r1 = ref1.relative_pose(s["win"], n_hypotheses=128, seed=3)
    assert r1["ok"] and got["l"] == r1["l"]
    same_structure(got, ref.global_sfm(s["win"], r1["l"], r1["R"], r1["T"]), "rel=None")
    with pytest.raises(TypeError):
        global_sfm(solver, [s["win"]], rel=[rel_of(s)], n_hypotheses=128)


class _Backend:
    def __init__(self, solver):
        self.s = solver


@pytest.mark.gpu
def test_gpu_sliding_window_estimator_global_sfm(solver):
    from vil_fusion_amd import sequence as sq
    from vil_fusion_amd.lib import default_options
    import startup_reference as ref1
    opts = default_options()
    seq = sq.make_sequence(11, sq.WINDOW_SIZE + 1, opts)
    est = sq.SlidingWindowEstimator(opts, _Backend(solver))
    est.process_imu(0.0, *seq["imu0"])
    for k in range(sq.WINDOW_SIZE):
        sq._feed_measurements(est, seq, k)
        assert est.process_image(seq["images"][k], seq["stamps"][k]) is None
    k = sq.WINDOW_SIZE
    est.f.add_feature_check_parallax(k, dict(sorted(seq["images"][k].items())), est.td)
    got, table = est.global_sfm(n_hypotheses=256)
    r1 = ref1.relative_pose(table, n_hypotheses=256)
    assert r1["ok"] and got["ok"] and got["l"] == r1["l"]
    same_structure(got, ref.global_sfm(table, r1["l"], r1["R"], r1["T"]), "driven window")
    RIC = np.array(opts.RIC[:]).reshape(3, 3)
    Rc = seq["R"] @ RIC
    err = max(sc.rot_err_deg(f["Q"], Rc[got["l"]].T @ Rc[i]) for i, f in enumerate(got["frames"]))
    print(f"drive: l {got['l']}, triangulated {got['n_triangulated']} of {len(table['start_frame'])}, largest rotation error of a frame {err:.4f} deg")


@pytest.mark.gpu
def test_gpu_full_size_stage_times(solver):
    from vil_fusion_amd.estimator import global_sfm, frame_pnp, startup_sfm_profile
    s = sc.chain_scene(5700, n=1000, n_full=400, noise_px=0.1)
    probs = [pnp_problem(5701, 1000)]
    for W in (1, 256):
        wins, rel = [s["win"]] * W, [rel_of(s)] * W
        global_sfm(solver, wins, rel=rel)                        # allocations and the first launch
        frame_pnp(solver, probs * W)
        solver.set_profiling(True)
        try:
            r = global_sfm(solver, wins, rel=rel)
            frame_pnp(solver, probs * W)
            ms, cnt = startup_sfm_profile(solver)
        finally:
            solver.set_profiling(False)
        print(f"GlobalSFM chain, 11 frames, 1000 features, {W} window(s), one run [ms]: su_sfm_chain {ms[0]:.3f}, su_pnp_batch ({W} problems of 1000 points) {ms[1]:.3f}")
        assert cnt == [1, 1] and all(np.isfinite(v) and v >= 0 for v in ms) and all(x["ok"] for x in r)
