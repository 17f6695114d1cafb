"""FeatureManager::triangulate and getDepthVector on the device (include/vilfusion.h, "Feature manager: triangulate").

CPU tests: the scalar restatement (tri_reference.py) against the oracle's own FeatureManager::triangulate to the bit, against np.linalg.svd of the same design
matrix and against the existing host loop sequence.FeatureManager.triangulate; the host-loop wiring of the `triangulate` argument; the ctypes layouts.
GPU tests: every output of vilf_features_triangulate against the restatement to the bit on the whole case list (tri_cases.py), batch independence, the refusals,
the profile, the host loops with and without the argument, and one timing that is printed and not asserted.

"To the bit" compares the 64 bits of every double, except that any NaN equals any NaN: sign and payload of a NaN are not part of the text (0.0 / 0.0 is a
negative NaN on x86 and a positive one on the device).

None of the bounds comes from the HIP path: the SVD_DIFFERENCE table was measured with the restatement alone."""
import copy
import ctypes as C
import os
import subprocess
import time
import numpy as np
import pytest
import tri_cases as tc
import tri_reference as ref
from vil_fusion_amd import abi, sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(a, b):
    """elementwise: the same 64 bits, or both NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def differences(got, want):
    """the outputs of one table that differ -> list of names"""
    bad = [k for k in ("depth", "inv_depth") if not same_bits(got[k], want[k])]
    bad += [k for k in ("flags", "sweeps") if not np.array_equal(np.asarray(got[k]), np.asarray(want[k]))]
    if dict(got["result"]) != dict(want["result"]):
        bad.append("result")
    return bad


# ---- 1. the restatement against the oracle's own FeatureManager::triangulate ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_triangulate(oracle, tmp_path_factory):
    """builds tests/tri_oracle_main.cpp (it includes oracle/sequence.cpp unchanged) with the oracle Makefile's flags against liboracle_vilf.so -> a function
    tables -> [(depth [n], getDepthVector)]"""
    odir = os.path.join(ROOT, "oracle")
    exe = str(tmp_path_factory.mktemp("tri_oracle") / "tri_oracle_main")
    flags = "-O3 -march=native -std=c++17 -fPIC -Wall -Wno-unused-function -fno-fast-math -ffp-contract=off".split()
    subprocess.run(["g++"] + flags + [os.path.join(ROOT, "tests", "tri_oracle_main.cpp"), "-o", exe, "-L", odir, "-loracle_vilf", "-Wl,-rpath," + odir, "-lpthread"], check=True)

    def run(tables):
        hx = lambda v: " ".join(float(x).hex() for x in np.asarray(v, dtype=np.float64).reshape(-1))
        lines = [str(len(tables))]
        for t in tables:
            n = len(t["start_frame"])
            lines.append(f"{int(t['n_frames'])} {n} {float(tc.INIT_DEPTH).hex()}")
            lines += [hx(t["Ps"]), hx(t["Rs"]), hx(t["tic"]), hx(t["ric"])]
            pts = np.asarray(t["points"], dtype=np.float64).reshape(-1, 3)
            for f in range(n):
                a, b = int(t["first_obs"][f]), int(t["first_obs"][f + 1])
                lines.append(f"{int(t['start_frame'][f])} {b - a} {float(t['depth'][f]).hex()} {hx(pts[a:b])}")
        out = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.split("\n")
        res = []
        for k in range(len(tables)):
            depth = np.array([float.fromhex(w) for w in out[2 * k].split()], dtype=np.float64)
            inv = [float.fromhex(w) for w in out[2 * k + 1].split()[1:]]
            res.append((depth, np.array(inv, dtype=np.float64)))
        return res
    return run


def test_restatement_equals_the_oracle_to_the_bit(oracle_triangulate):
    """a condition, not a measurement: 0 mismatches on every table of the case list and on 200 seeded random features"""
    refs = tc.references()
    tables, wants = [], []
    for name, tabs in tc.cases():
        tables += tabs; wants += refs[name]
    rnd = tc.random_features(5, 200)
    tables += rnd; wants += [ref.triangulate(t, tc.WINDOW_SIZE, tc.INIT_DEPTH) for t in rnd]
    got = oracle_triangulate(tables)
    bad = [k for k, ((d, inv), w) in enumerate(zip(got, wants)) if not (same_bits(d, w["depth"]) and same_bits(inv, w["inv_depth"]))]
    n_cand = sum(w["result"]["n_candidates"] for w in wants)
    kinds = dict(depth=sum(int(((w["flags"] & ref.DONE) != 0).sum() - w["result"]["n_reset"] - w["result"]["n_nonfinite"]) for w in wants),
                 reset=sum(w["result"]["n_reset"] for w in wants), nonfinite=sum(w["result"]["n_nonfinite"] for w in wants))
    full = sum(int((w["sweeps"] == ref.SWEEPS).sum()) for w in wants)
    print(f"{len(tables)} tables, {n_cand} candidates ({kinds}), {full} ran all {ref.SWEEPS} sweeps; tables that differ from the oracle: {len(bad)}")
    assert kinds["depth"] > 0 and kinds["reset"] > 0 and kinds["nonfinite"] > 0         # the list reaches every kind of result
    assert not bad, bad


def test_case_list_reaches_its_edges():
    """what the list is there for: inf and NaN kept and flagged, the two sides of the reset threshold, candidate counts around a wave"""
    refs = tc.references()
    sp = refs["special"]
    assert np.isnan(sp[0]["depth"][:3]).all() and (sp[0]["flags"][:3] == ref.USED | ref.DONE | ref.NONFINITE).all()
    assert np.isposinf(sp[1]["depth"]).any() and sp[1]["result"]["n_nonfinite"] > 0
    edge = refs["edges step 0.005 noise 0.0"][0]
    t = tc.cases()[2][1][0]
    assert tc.cases()[2][0] == "edges step 0.005 noise 0.0"
    for td, reset in ((0.0999, True), (0.1001, False)):
        idx = np.nonzero(t["truth"] == td)[0]
        assert len(idx) == 2
        for f in idx:
            assert bool(edge["flags"][f] & ref.RESET) == reset, (td, f, edge["depth"][f])
            assert edge["depth"][f] == (tc.INIT_DEPTH if reset else edge["depth"][f]) and (reset or abs(edge["depth"][f] - td) < 1e-9)
    for n in (0, 1, 63, 64, 65):
        assert refs[f"{n} candidates"][0]["result"]["n_candidates"] == n
    st = [r["result"]["n_candidates"] for r in refs["straddle"]]
    assert st[0] < 64 < st[0] + st[3] and st[1] == st[2] == st[4] == 0 and st[5] > 0
    # one pose for all frames: the last column of A is 0 exactly. With noise the depth is 0 / 1 and is reset; without, the observations of a feature are the same
    # ray f, (f, 0) is a second null vector, a column in front of the last can reach a norm of 0 too and win the tie: V_3 = 0, inf or NaN, kept and flagged
    one, noisy = refs["edges step 0.0 noise 0.0"][0]["result"], refs["edges step 0.0 noise 0.5"][0]["result"]
    assert one["n_nonfinite"] > 0 and one["n_reset"] + one["n_nonfinite"] == one["n_candidates"]
    assert noisy["n_reset"] == noisy["n_candidates"] > 0


# ---- 2. the restatement against np.linalg.svd of the same design matrix -----------------------------------------------------------------------------------------
# measured with the restatement, one run, rounded up to two digits: the largest relative difference of the depth V_2 / V_3 (before the reset rule) between the
# Hestenes Jacobi of the text and np.linalg.svd (LAPACK gesdd) on the same design matrix, over the 40 features of svd_features(step, noise). The test asserts ten
# times these. At a step of 0 (one pose for all frames) the matrix has a null space of two or more dimensions and no depth is defined: any vector of it is a right
# answer, the two routines pick different ones, and the rows of the table are replaced by a condition: neither gives a feature a depth (each result is reset or is
# not finite).
SVD_DIFFERENCE = {
    (0.5, 0.0): 1.5e-14, (0.5, 0.5): 1.4e-13,
    (0.005, 0.0): 6.0e-15, (0.005, 0.5): 1.4e-13,
}


def svd_features(step, noise):
    """40 candidates of 2 to 11 observations; true depths of 4 to 30 m at 0.5 m steps, of 0.05 to 0.3 m at 5 mm steps (the same parallax)"""
    rng = np.random.default_rng(int(step * 1000) + int(noise * 10) + 1)
    b = tc.Builder(600 + int(step * 1000) + int(noise * 10), tc.NF, step if step else 0.5, one_pose=step == 0.0, noise_px=noise)
    for _ in range(40):
        start = int(rng.integers(0, tc.WINDOW_SIZE - 2))
        b.add(int(rng.integers(2, tc.NF - start + 1)), start, -1.0, true_depth=float(rng.uniform(4.0, 30.0)) * (0.01 if step == 0.005 else 1.0))
    return b.table()


def raw_depths(t):
    """per feature (the text's V_2 / V_3, np.linalg.svd's) on the same design matrix"""
    out = []
    for f in range(len(t["start_frame"])):
        A = ref.design_matrix_of(t, f)
        v, _ = ref.smallest_right_singular_vector(A.tolist())
        u = np.linalg.svd(A)[2][-1]
        out.append((ref.div(v[2], v[3]), ref.div(float(u[2]), float(u[3]))))
    return np.array(out)


def test_restatement_against_numpy_svd():
    bad = []
    for (step, noise), bound in SVD_DIFFERENCE.items():
        d = raw_depths(svd_features(step, noise))
        diff = np.abs(d[:, 0] - d[:, 1]) / np.abs(d[:, 1])
        print(f"step {step} m, noise {noise} px: largest relative depth difference to np.linalg.svd {diff.max():.2e} (table: {bound:.1e})")
        if not diff.max() <= 10.0 * bound:
            bad.append((step, noise, float(diff.max()), bound))
    for noise in (0.0, 0.5):
        d = raw_depths(svd_features(0.0, noise))
        no_depth = (d < 0.1) | ~np.isfinite(d)
        print(f"step 0 (one pose), noise {noise} px: features without a depth {int(no_depth[:, 0].sum())} (the text) and {int(no_depth[:, 1].sum())} (np.linalg.svd) of {len(d)}")
        if not no_depth.all():
            bad.append((0.0, noise, d[~no_depth.all(axis=1)].tolist()))
    assert not bad, bad


# ---- 3. the restatement against the existing host loop ----------------------------------------------------------------------------------------------------------
def first_solved_window(seq, opts):
    """the estimator in front of solveOdometry's triangulation of the first solved frame -> (table, the host loop's feature manager after its triangulate)"""
    est = sequence.SlidingWindowEstimator(opts, None)
    est.process_imu(0.0, *seq["imu0"])
    for k in range(sequence.WINDOW_SIZE + 1):
        sequence._feed_measurements(est, seq, k)
        solved = est.prepare_image(seq["images"][k], seq["stamps"][k], seq["init"][k])
    assert solved
    table = est.f.triangulation_table(est.Ps, est.Rs, est.tic, est.ric)
    host = copy.deepcopy(est.f)
    host.triangulate(est.Ps, est.Rs, est.tic, est.ric)
    return table, host


@pytest.mark.parametrize("profile", [dict(), dict(mean_speed=4.0, speed_modulation=0.8)], ids=["drive", "stop-and-go"])
def test_restatement_against_the_host_triangulate(opts, profile):
    """the first solved window of make_sequence(3, 40, opts) and of a stop-and-go profile: the same features triangulated and reset, the depths within ten times the
    table's figure of 0.5 m steps with noise (the frames are 0.4 to 1 m apart here, the observations carry 0.5 px). Every candidate is compared."""
    table, host = first_solved_window(sequence.make_sequence(3, 40, opts, **profile), opts)
    r = ref.triangulate(table, sequence.WINDOW_SIZE, sequence.INIT_DEPTH)
    hd = np.array([it.estimated_depth for it in host.feature])
    cand = (r["flags"] & ref.DONE) != 0
    changed = ~same_bits_each(hd, table["depth"])
    step = np.linalg.norm(np.diff(table["Ps"], axis=0), axis=1)
    print(f"{len(hd)} features, {int(cand.sum())} candidates, {r['result']['n_reset']} reset; frames {step.min():.2f} to {step.max():.2f} m apart")
    assert cand.sum() > 0
    assert same_bits(hd[~cand], r["depth"][~cand]) and not changed[~cand].any()                # the same features are triangulated ..
    reset_host = cand & (hd == sequence.INIT_DEPTH)
    assert np.array_equal(reset_host, (r["flags"] & ref.RESET) != 0)                                 # .. and reset
    raw = hd[cand & ~reset_host]
    assert not (np.abs(raw - 0.1) < 1e-9 * 0.1).any()                                             # no host depth at the threshold: none is left out
    rel = np.abs(r["depth"][cand] - hd[cand]) / np.abs(hd[cand])
    print(f"largest relative depth difference to the host loop {rel.max():.2e} (bound {10 * SVD_DIFFERENCE[(0.5, 0.5)]:.1e})")
    assert rel.max() <= 10 * SVD_DIFFERENCE[(0.5, 0.5)]


def same_bits_each(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


# ---- 4. the host-loop wiring ------------------------------------------------------------------------------------------------------------------------------------
def test_table_and_apply_round_trip():
    """every used / unused / candidate combination: the table holds the whole list in order, apply writes every depth back and nothing else"""
    fm = sequence.FeatureManager()
    specs = [(0, 1, -1.0), (0, 2, -1.0), (0, 2, 7.5), (7, 3, 0.0), (8, 3, -1.0), (8, 2, 6.0), (3, 1, 2.0), (2, 5, float("nan"))]
    for fid, (start, n_obs, depth) in enumerate(specs):
        it = sequence.FeaturePerId(fid, start, -1.0)
        it.estimated_depth = depth
        it.feature_per_frame = [sequence.FeaturePerFrame([0.01 * fid, 0.02 * o, 1.0, 0, 0, 0, 0, -1.0], 0.0) for o in range(n_obs)]
        fm.feature.append(it)
    Ps, Rs = tc.poses(3)
    t = fm.triangulation_table(Ps, Rs, tc.TIC, tc.RIC)
    assert t["n_frames"] == tc.NF and list(t["start_frame"]) == [s[0] for s in specs] and list(np.diff(t["first_obs"])) == [s[1] for s in specs]
    assert same_bits(t["depth"], [s[2] for s in specs]) and t["points"].shape == (sum(s[1] for s in specs), 3)
    assert t["points"][t["first_obs"][3] + 2].tolist() == [0.03, 0.04, 1.0]
    r = ref.triangulate(t, sequence.WINDOW_SIZE, sequence.INIT_DEPTH)
    assert list(r["flags"] & ref.USED) == [0, 1, 1, 1, 0, 0, 0, 1] and list((r["flags"] & ref.DONE) // ref.DONE) == [0, 1, 0, 1, 0, 0, 0, 1]
    before = [(it.feature_id, it.start_frame, len(it.feature_per_frame), it.solve_flag, it.lidar_depth_flag) for it in fm.feature]
    fm.apply_triangulation(r["depth"])
    assert before == [(it.feature_id, it.start_frame, len(it.feature_per_frame), it.solve_flag, it.lidar_depth_flag) for it in fm.feature]
    assert same_bits([it.estimated_depth for it in fm.feature], r["depth"])
    assert len(r["inv_depth"]) == fm.get_feature_count() and same_bits(r["inv_depth"], fm.get_depth_vector())


class Recorder:
    """a `triangulate` callable on the restatement that keeps what it was called with"""

    def __init__(self):
        self.calls = []

    def __call__(self, tables):
        tables = list(tables)
        self.calls.append([dict(n_features=len(t["start_frame"]), tic=np.array(t["tic"]).copy()) for t in tables])
        return [ref.triangulate(t, sequence.WINDOW_SIZE, sequence.INIT_DEPTH) for t in tables]


def test_estimator_calls_the_argument_once_per_solved_frame(opts, monkeypatch):
    import seq_backends
    seq = sequence.make_sequence(5, 14, opts, max_cnt=60, yaw_amplitude=0.3)
    host_calls = []
    orig = sequence.FeatureManager.triangulate
    monkeypatch.setattr(sequence.FeatureManager, "triangulate", lambda self, *a: (host_calls.append(1), orig(self, *a))[1])
    rec = Recorder()
    est = sequence.run_sequence(seq, opts, seq_backends.OracleBackend(opts), n_frames=13, triangulate=rec)
    assert est.events.count("solved") == 3 and len(rec.calls) == 3 and not host_calls
    assert all(len(c) == 1 and np.array_equal(c[0]["tic"], np.array(opts.TIC[:])) for c in rec.calls)
    # through visualInitialAlign: one more call, the first, on the camera positions (tic = 0)
    rec = Recorder()
    est = sequence.run_sequence(seq, opts, seq_backends.OracleBackend(opts), n_frames=12, startup=dict(seed=1, scale=3.7), triangulate=rec)
    assert est.initial_ok and est.events.count("solved") == 2 and len(rec.calls) == 3 and not host_calls
    assert not rec.calls[0][0]["tic"].any() and all(np.array_equal(c[0]["tic"], np.array(opts.TIC[:])) for c in rec.calls[1:])
    # without the argument the host loop runs and nothing else
    est = sequence.run_sequence(seq, opts, seq_backends.OracleBackend(opts), n_frames=12)
    assert est.triangulate is None and len(host_calls) == 2


class OracleBatch:
    """what run_sequences_lockstep needs from a solver, on the CPU oracle: one window_solve and one window_marginalize per slot"""

    def __init__(self, oracle, opts, n):
        self.oracle, self.o, self.priors = oracle, opts, [None] * n

    def set_prior(self, prior, slot=0):
        assert prior is None
        self.priors[slot] = None

    def batch_upload(self, windows):
        self.windows = windows

    def batch_solve(self, sync=True):
        self.results = [self.oracle.window_solve(self.o, w, p) for w, p in zip(self.windows, self.priors)]

    def batch_marginalize(self, sync=True):
        new = [self.oracle.window_marginalize(self.o, w, r, p) for w, r, p in zip(self.windows, self.results, self.priors)]
        self.priors = [p if p.valid else None for p in new]

    def batch_download(self):
        return self.results

    def marginalize_stats(self):
        return dict(new_prior=0, amm_cholesky=0, kept_cholesky=0, unchanged=0)


def test_lockstep_calls_the_argument_once_per_frame_with_all_live_segments(oracle, opts, monkeypatch):
    seqs = [sequence.make_sequence(11 + i, 13, opts, max_cnt=50) for i in range(2)]
    host_calls = []
    orig = sequence.FeatureManager.triangulate
    monkeypatch.setattr(sequence.FeatureManager, "triangulate", lambda self, *a: (host_calls.append(1), orig(self, *a))[1])
    rec = Recorder()
    ests = sequence.run_sequences_lockstep(seqs, opts, OracleBatch(oracle, opts, 2), triangulate=rec)
    assert [e.events.count("solved") for e in ests] == [3, 3]
    assert len(rec.calls) == 3 and all(len(c) == 2 for c in rec.calls) and not host_calls
    want = sequence.run_sequences_lockstep(seqs, opts, OracleBatch(oracle, opts, 2))
    assert len(host_calls) == 6
    for a, b in zip(ests, want):                                  # two triangulations, one loop: the same decisions
        assert a.events == b.events and a.flags == b.flags and feature_lists(a) == feature_lists(b)


def feature_lists(est):
    return [(it.feature_id, it.start_frame, len(it.feature_per_frame), it.solve_flag, it.lidar_depth_flag) for it in est.f.feature]


def test_ctypes_mirrors_match_the_c_layout(tmp_path):
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "vilfusion.h"', "int main(void) {"]
    checks = []
    for cname, ct in abi.TRI_LAYOUTS.items():
        prog.append(f'  printf("%zu\\n", sizeof({cname}));')
        checks.append((cname, "sizeof", C.sizeof(ct)))
        for fname, _ in ct._fields_:
            prog.append(f'  printf("%zu\\n", offsetof({cname}, {fname}));')
            checks.append((cname, fname, getattr(ct, fname).offset))
    prog += ['  printf("%d %d %d %d %d\\n", VILF_TRI_MAX_WINDOWS, VILF_TRI_USED, VILF_TRI_DONE, VILF_TRI_RESET, VILF_TRI_NONFINITE);', "  return 0;", "}"]
    src = tmp_path / "layout.c"; exe = tmp_path / "layout"
    src.write_text("\n".join(prog))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert len(out) == len(checks) + 5
    bad = [(c, f, int(o), e) for (c, f, e), o in zip(checks, out) if int(o) != e]
    assert not bad, bad
    assert [int(v) for v in out[-5:]] == [abi.VILF_TRI_MAX_WINDOWS, abi.VILF_TRI_USED, abi.VILF_TRI_DONE, abi.VILF_TRI_RESET, abi.VILF_TRI_NONFINITE]
    assert (ref.USED, ref.DONE, ref.RESET, ref.NONFINITE) == (abi.VILF_TRI_USED, abi.VILF_TRI_DONE, abi.VILF_TRI_RESET, abi.VILF_TRI_NONFINITE)


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver():
    from vil_fusion_amd.estimator import BackendSolver
    s = BackendSolver()
    assert s.options.window_size == tc.WINDOW_SIZE and s.options.init_depth == tc.INIT_DEPTH
    yield s
    s.close()


def device(solver, tables):
    from vil_fusion_amd.estimator import triangulate_features
    return triangulate_features(solver, tables)


@pytest.mark.gpu
def test_device_equals_the_restatement_to_the_bit(solver):
    """every output of vilf_features_triangulate (depth_out, inv_depth_out, flags_out, sweeps_out, the four counts) on the whole case list"""
    refs = tc.references()
    bad, n_cand = [], 0
    for name, tables in tc.cases():
        got = device(solver, tables)
        assert len(got) == len(tables)
        for w, (g, r) in enumerate(zip(got, refs[name])):
            n_cand += r["result"]["n_candidates"]
            d = differences(g, r)
            if d:
                bad.append((name, w, d))
    print(f"{len(tc.cases())} calls, {n_cand} candidates; tables with an output that differs: {len(bad)}")
    assert not bad, bad


@pytest.mark.gpu
def test_batch_independence(solver):
    """the batched call equals window-by-window calls to the bit, and a window's outputs do not change when windows in front of it are added or removed"""
    cases = dict(tc.cases())
    for name in ("straddle", "three windows", "special", "two windows"):
        tables = cases[name]
        batched = device(solver, tables)
        for w, t in enumerate(tables):
            alone = device(solver, [t])[0]
            assert not differences(alone, batched[w]), (name, w)
    tables = cases["straddle"]
    batched = device(solver, tables)
    for first in (1, 2, 3):                               # windows in front removed: window 3's candidates move from lanes 40 .. 79 to lane 0 ..
        got = device(solver, tables[first:])
        for w in range(first, len(tables)):
            assert not differences(got[w - first], batched[w]), (first, w)
    extra = cases["65 candidates"] + cases["1 candidates"]        # .. and added
    got = device(solver, extra + tables)
    for w in range(len(tables)):
        assert not differences(got[len(extra) + w], batched[w]), w
    order = [3, 0, 5, 1]
    got = device(solver, [tables[w] for w in order])
    for k, w in enumerate(order):
        assert not differences(got[k], batched[w]), w


PATTERN = 0xA5


class RawCall:
    """the ctypes arguments of one vilf_features_triangulate call from tables, every output filled with a pattern"""

    def __init__(self, tables):
        self.n = len(tables)
        self.W = (abi.TriWindow * self.n)()
        self.out = (abi.TriResult * self.n)()
        C.memset(self.out, PATTERN, C.sizeof(self.out))
        self.keep, self.outputs = [], []
        for k, t in enumerate(tables):
            m = len(t["start_frame"])
            a = dict(Ps=np.array(t["Ps"], dtype=np.float64).reshape(-1).copy(), Rs=np.array(t["Rs"], dtype=np.float64).reshape(-1).copy(),
                     start=np.array(t["start_frame"], dtype=np.int32), first=np.array(t["first_obs"], dtype=np.int32),
                     pts=np.array(t["points"], dtype=np.float64).reshape(-1, 3).copy(), din=np.array(t["depth"], dtype=np.float64))
            o = dict(depth=np.frombuffer(bytes([PATTERN]) * 8 * m, dtype=np.float64).copy(), inv=np.frombuffer(bytes([PATTERN]) * 8 * m, dtype=np.float64).copy(),
                     flags=np.full(m, PATTERN, dtype=np.uint8), sweeps=np.full(m, PATTERN, dtype=np.uint8))
            self.keep.append(a); self.outputs.append(o)
            w = self.W[k]
            w.n_frames, w.n_features = int(t["n_frames"]), m
            w.Ps, w.Rs = abi.dptr(a["Ps"]), abi.dptr(a["Rs"])
            w.tic[:] = np.asarray(t["tic"], dtype=np.float64).reshape(3).tolist()
            w.ric[:] = np.asarray(t["ric"], dtype=np.float64).reshape(9).tolist()
            w.start_frame, w.first_obs = a["start"].ctypes.data_as(C.POINTER(C.c_int32)), a["first"].ctypes.data_as(C.POINTER(C.c_int32))
            w.points, w.depth_in = abi.dptr(a["pts"]), abi.dptr(a["din"])
            w.depth_out, w.inv_depth_out = abi.dptr(o["depth"]), abi.dptr(o["inv"])
            w.flags_out, w.sweeps_out = o["flags"].ctypes.data_as(C.POINTER(C.c_uint8)), o["sweeps"].ctypes.data_as(C.POINTER(C.c_uint8))

    def untouched(self):
        if bytes(self.out) != bytes([PATTERN]) * C.sizeof(self.out):
            return False
        return all(v.tobytes() == bytes([PATTERN]) * v.nbytes for o in self.outputs for v in o.values())


def small_tables():
    """two windows, both with candidates; the second is the one the refusals spoil, so that `nothing written` covers a good window in front of a bad one. Its feature
    0 is used (3 observations from frame 0) and a candidate"""
    a = tc.Builder(71, noise_px=0.5).add(3, 0, -1.0).add(2, 1, 7.5).add(4, 2, 0.0).table()
    b = tc.Builder(72, noise_px=0.5).add(3, 0, -1.0).add(1, 9, -1.0).add(5, 3, -1.0).add(2, 7, 4.0).table()
    return [a, b]


NULLP = {"Ps": abi.c_double_p(), "Rs": abi.c_double_p(), "points": abi.c_double_p(), "depth_in": abi.c_double_p(), "depth_out": abi.c_double_p(),
         "first_obs": C.POINTER(C.c_int32)(), "start_frame": C.POINTER(C.c_int32)()}


def spoil_null(name):
    return lambda c: setattr(c.W[1], name, NULLP[name])


def spoil_array(key, index, value):
    def f(c):
        c.keep[1][key][index] = value
    return f


def spoil_field(name, index, value):
    def f(c):
        getattr(c.W[1], name)[index] = value
    return f


REFUSALS = {
    "n_frames 1": lambda c: setattr(c.W[1], "n_frames", 1), "n_frames 12": lambda c: setattr(c.W[1], "n_frames", abi.VILF_MAX_FRAMES + 1),
    "n_features -1": lambda c: setattr(c.W[1], "n_features", -1), "n_features 1001": lambda c: setattr(c.W[1], "n_features", abi.VILF_MAX_FEATURES + 1),
    "first_obs[0] = 1": spoil_array("first", 0, 1), "first_obs decreases": spoil_array("first", 2, 2),
    "used feature, start_frame -1": spoil_array("start", 0, -1), "used feature, start_frame + n_obs > n_frames": lambda c: setattr(c.W[1], "n_frames", 7),
    "null Ps": spoil_null("Ps"), "null Rs": spoil_null("Rs"), "null first_obs": spoil_null("first_obs"), "null start_frame": spoil_null("start_frame"),
    "null depth_in": spoil_null("depth_in"), "null depth_out": spoil_null("depth_out"), "null points": spoil_null("points"),
    "NaN in Ps": spoil_array("Ps", 4, float("nan")), "inf in Ps": spoil_array("Ps", 32, float("inf")), "NaN in Rs": spoil_array("Rs", 98, float("nan")),
    "inf in Rs": spoil_array("Rs", 0, float("-inf")), "NaN in tic": spoil_field("tic", 2, float("nan")), "inf in tic": spoil_field("tic", 0, float("inf")),
    "NaN in ric": spoil_field("ric", 8, float("nan")), "inf in ric": spoil_field("ric", 3, float("inf")),
}


@pytest.mark.gpu
def test_invalid_arguments_write_nothing(solver):
    L = solver._L
    tables = small_tables()
    want = [ref.triangulate(t, tc.WINDOW_SIZE, tc.INIT_DEPTH) for t in tables]
    assert want[1]["flags"][0] == ref.USED | ref.DONE and want[1]["flags"][2] & ref.USED             # "n_frames 7" cuts the used feature 2 (frames 3 .. 7) off
    bad = []
    for name, spoil in REFUSALS.items():
        c = RawCall(tables)
        spoil(c)
        rc = L.vilf_features_triangulate(solver._h, c.n, c.W, c.out)
        if rc != abi.VILF_ERR_INVALID_ARGUMENT or not c.untouched():
            bad.append((name, rc, c.untouched()))
    for name, args in {"null handle": lambda c: (None, c.n, c.W, c.out), "null windows": lambda c: (solver._h, c.n, None, c.out), "null out": lambda c: (solver._h, c.n, c.W, None),
                       "n_windows 0": lambda c: (solver._h, 0, c.W, c.out), "n_windows -1": lambda c: (solver._h, -1, c.W, c.out),
                       "n_windows 4097": lambda c: (solver._h, abi.VILF_TRI_MAX_WINDOWS + 1, c.W, c.out)}.items():
        c = RawCall(tables)
        rc = L.vilf_features_triangulate(*args(c))
        if rc != abi.VILF_ERR_INVALID_ARGUMENT or not c.untouched():
            bad.append((name, rc, c.untouched()))
    assert not bad, bad
    c = RawCall(tables)                                           # the same arguments unspoilt: accepted, and the optional outputs may be null
    for k in range(c.n):
        c.W[k].inv_depth_out, c.W[k].flags_out, c.W[k].sweeps_out = abi.c_double_p(), C.POINTER(C.c_uint8)(), C.POINTER(C.c_uint8)()
    assert L.vilf_features_triangulate(solver._h, c.n, c.W, c.out) == abi.VILF_OK
    for k in range(c.n):
        assert same_bits(c.outputs[k]["depth"], want[k]["depth"]) and c.out[k].n_candidates == want[k]["result"]["n_candidates"]
        assert all(c.outputs[k][key].tobytes() == bytes([PATTERN]) * c.outputs[k][key].nbytes for key in ("inv", "flags", "sweeps"))
    # a feature that is not used is not checked: one observation in a frame the window does not have
    t = tc.Builder(73).add(3, 0, -1.0).table()
    t["start_frame"] = np.array([0, 40], dtype=np.int32); t["first_obs"] = np.array([0, 3, 4], dtype=np.int32)
    t["points"] = np.vstack([t["points"], [[0.0, 0.0, 1.0]]]); t["depth"] = np.array([-1.0, -1.0])
    got = device(solver, [t])[0]
    assert list(got["flags"]) == [ref.USED | ref.DONE, 0] and got["depth"][1] == -1.0


@pytest.mark.gpu
def test_profile_counts_launches(solver):
    from vil_fusion_amd.estimator import features_profile
    tables = dict(tc.cases())["three windows"]
    solver.set_profiling(True)
    try:
        assert features_profile(solver) == ([0.0], [0])
        device(solver, tables); device(solver, tables)
        device(solver, dict(tc.cases())["0 candidates"])          # no candidate: nothing is launched
        ms, cnt = features_profile(solver)
        assert cnt == [4] and ms[0] > 0.0, (ms, cnt)
    finally:
        solver.set_profiling(False)
    assert features_profile(solver) == ([0.0], [0])
    device(solver, tables)
    assert features_profile(solver) == ([0.0], [0])


def run_frames(seq, opts, backend, triangulate):
    """run_sequence with the feature list kept after every frame"""
    est = sequence.SlidingWindowEstimator(opts, backend, triangulate)
    est.process_imu(0.0, *seq["imu0"])
    lists = []
    for k in range(len(seq["images"])):
        sequence._feed_measurements(est, seq, k)
        est.process_image(seq["images"][k], seq["stamps"][k], seq["init"][k] if est.solver_flag == est.INITIAL else None)
        lists.append(feature_lists(est))
    return est, lists


def compare_runs(got, want, label):
    assert got.events == want.events and got.flags == want.flags, label
    dP = max(np.abs(a[1] - b[1]).max() for a, b in zip(got.trajectory, want.trajectory))
    dq = max(min(np.abs(a[2] - b[2]).max(), np.abs(a[2] + b[2]).max()) for a, b in zip(got.trajectory, want.trajectory))
    ia, ib = [x["num_iterations"] for x in got.summaries], [x["num_iterations"] for x in want.summaries]
    first = next((k for k in range(len(ia)) if ia[k] != ib[k]), None)
    print(f"{label}: {len(got.trajectory)} solved frames, max|dP| {dP:.2e} m, max|dq| {dq:.2e}; iteration counts identical for the first {first if first is not None else len(ia)} frames")
    if first is not None:
        print(f"    first difference at frame {first}: {ia[first]} iterations with the device triangulation, {ib[first]} with the host loop")
        assert first >= 20, (label, first)
    assert dP < 1e-4 and dq < 1e-5, (label, dP, dq)


@pytest.mark.gpu
def test_host_loop_with_the_device_triangulation(opts):
    """run_sequence on the HIP path with and without triangulate=solver.triangulate_features: the same events, flags and feature lists after every frame, the
    trajectories within the bound of two correct routes (1e-4 m, 1e-5 quaternion), no iteration count differs before frame 20"""
    import seq_backends
    from vil_fusion_amd.estimator import BackendSolver
    seq = sequence.make_sequence(3, 40, opts)
    s = BackendSolver(opts)
    try:
        want, want_lists = run_frames(seq, opts, seq_backends.HipBackend(s), None)
        got, got_lists = run_frames(seq, opts, seq_backends.HipBackend(s), s.triangulate_features)
    finally:
        s.close()
    assert got_lists == want_lists
    assert len(got.trajectory) == 30
    compare_runs(got, want, "run_sequence")


@pytest.mark.gpu
def test_lockstep_with_one_device_triangulation_per_frame(opts):
    """run_sequences_lockstep, two segments of 25 frames: as above per segment, and one vilf_features_triangulate per frame for both segments (the profile's launch
    count: two kernels per call that has a candidate)"""
    from vil_fusion_amd.estimator import BackendSolver
    seqs = [sequence.make_sequence(21 + i, 25, opts) for i in range(2)]
    s = BackendSolver(opts)
    calls = []

    def tri(tables):
        res = s.triangulate_features(tables)
        calls.append((len(res), sum(r["result"]["n_candidates"] for r in res)))
        return res
    try:
        want_lists, got_lists = [], []
        want = sequence.run_sequences_lockstep(seqs, opts, s, on_frame=lambda i, k, e, r: want_lists.append((i, k, feature_lists(e))))
        s.set_profiling_features(True)
        got = sequence.run_sequences_lockstep(seqs, opts, s, on_frame=lambda i, k, e, r: got_lists.append((i, k, feature_lists(e))), triangulate=tri)
        ms, cnt = s.features_profile()
    finally:
        s.close()
    assert got_lists == want_lists
    assert len(calls) == 15 and all(c[0] == 2 for c in calls)                     # frames 10 .. 24, both segments in one call
    assert cnt[0] == 2 * sum(1 for c in calls if c[1] > 0) and cnt[0] > 0, (cnt, calls)
    print(f"{len(calls)} frames, {sum(c[1] for c in calls)} candidates, {cnt[0]} kernel launches, {ms[0]:.3f} ms on the device")
    for i, (a, b) in enumerate(zip(got, want)):
        compare_runs(a, b, f"lockstep segment {i}")


def manager_from_table(t):
    fm = sequence.FeatureManager()
    for f in range(len(t["start_frame"])):
        it = sequence.FeaturePerId(f, int(t["start_frame"][f]), -1.0)
        it.estimated_depth = float(t["depth"][f])
        it.feature_per_frame = [sequence.FeaturePerFrame(list(p) + [0, 0, 0, 0, -1.0], 0.0) for p in t["points"][t["first_obs"][f]:t["first_obs"][f + 1]]]
        fm.feature.append(it)
    return fm


@pytest.mark.gpu
def test_time_is_measured_not_asserted(solver):
    """one window of 150 features of which 15 are candidates, and 256 such windows in one call (8 different ones, 32 times each): HIP events around the two launches
    after one warm-up, the whole call on the host's clock, and the host loop sequence.FeatureManager.triangulate on the same tables. Printed, one run; no time is
    asserted, there is no earlier device path to compare with"""
    from vil_fusion_amd.estimator import features_profile
    distinct = [tc.count_window(900 + w, 150, 15, short=False) for w in range(8)]
    t0 = time.perf_counter()
    for t in distinct:
        manager_from_table(t).triangulate(t["Ps"], t["Rs"], t["tic"], t["ric"])
    host = (time.perf_counter() - t0) / len(distinct)
    rows = []
    for label, tables in (("1 window", distinct[:1]), ("256 windows", distinct * 32)):
        device(solver, tables)                                    # warm-up: the buffers grow here
        solver.set_profiling(True)
        t0 = time.perf_counter()
        got = device(solver, tables)
        wall = time.perf_counter() - t0
        ms, cnt = features_profile(solver)
        solver.set_profiling(False)
        n_cand = sum(r["result"]["n_candidates"] for r in got)
        rows.append((label, n_cand, ms[0], wall * 1e3, host * 1e3 * len(tables)))
        assert cnt == [2] and n_cand == 15 * len(tables)
    for label, n_cand, ms, wall, hst in rows:
        print(f"{label}: {n_cand} candidates; kernels {ms:.3f} ms, the call with packing and ctypes {wall:.2f} ms, the host loop {hst:.1f} ms (one run)")
