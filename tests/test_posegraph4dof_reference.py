"""tests/pg4_reference.py, the numpy restatement of the 4-DoF pose graph (include/vilfusion.h, "Visual loop closure, third stage"), measured against things that are
not the restatement: the 40-digit run of tests/pg4_exact.py after 1, 2 and 5 attempts, and scipy's least squares at convergence. Four deliberate errors, put one at a
time into a copy of the restatement, must each fail the first of these. VisualPoseGraph's bookkeeping runs here with the restatement as its back-end. No GPU."""
import ctypes as C
import math
import os
import re
import subprocess
import types

import numpy as np
import pytest
from scipy.optimize import least_squares

import pg4_cases as cs
import pg4_reference as ref
from vil_fusion_amd import abi
from vil_fusion_amd.sequence import R2ypr, ypr2R
from vil_fusion_amd.visual_posegraph import VisualPoseGraph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = list(cs.small_cases())
# the restatement run to convergence (max_iterations 64, tolerances 1e-15) against scipy's trust region with 3-point differences on the Huber cost, measured on the
# CPU over SCIPY_CASES (one run each): 4.7e-9 m (pitch_roll) and 2.2e-10 degrees (two_sequences). The tolerance is ten times that.
SCIPY_CASES = ["three_loops", "in_band", "pitch_roll", "huber", "two_sequences", "sequence0_fixed", "shared_old"]
SCIPY_TOL_M, SCIPY_TOL_DEG = 4.7e-8, 2.2e-9


def case_of(name):
    return cs.reject_case() if name == "reject" else cs.small_cases()[name]


def run(mod, c, **over):
    return mod.optimize(c["vio_R"], c["vio_T"], c["sequence"], c["fixed"], c["loops"], cs.params_of(c, **over))


def worst_against_exact(mod, name):
    """the figures of cs.compare over the snapshots of the exact run (decisions, counts and flags are asserted equal inside)"""
    worst = {}
    for k, snap in cs.exact(name).items():
        fig = cs.compare(run(mod, case_of(name), max_iterations=k), snap)
        for q, v in fig.items():
            worst[q] = max(worst.get(q, 0.0), v)
    return worst


@pytest.mark.parametrize("name", SMALL + ["reject"])
def test_restatement_against_exact_after_1_2_5_attempts(name):
    cs.check_margins(name)                       # no rho within 1e-6 of min_relative_decrease, no stop rule at equality
    worst = worst_against_exact(ref, name)
    tol = cs.CPU_TOL_REJECT if name == "reject" else cs.CPU_TOL
    print(name, {q: f"{v:.3e}" for q, v in worst.items()}, tol)
    assert cs.within(worst, tol), (worst, tol)


def test_cases_reach_the_branches_they_are_named_for():
    C_ = cs.small_cases()
    P = ref.default_params()
    yaw = np.array([ref.R2ypr(R)[0] for R in C_["wrap"]["vio_R"]])
    assert np.any((yaw > 179.5) & (yaw <= 180.0)) and np.any((yaw < -179.5) & (yaw >= -180.0))
    wrapped = run(ref, C_["wrap"])
    assert np.any(np.abs(wrapped["ypr"][:, 0] - yaw) > 300.0)            # an update crossed the wrap
    edges = ref.build_edges(C_["wrap"]["vio_R"], C_["wrap"]["vio_T"], C_["wrap"]["sequence"], C_["wrap"]["loops"])
    assert any(abs(yaw[e[1]] - yaw[e[0]] - e[3]) > 180.0 for e in edges if e[4])            # NormalizeAngle acts in a loop's residual
    h = C_["huber"]
    ypr = np.array([ref.R2ypr(R) for R in h["vio_R"]])
    edges = ref.build_edges(h["vio_R"], h["vio_T"], h["sequence"], h["loops"])
    norms = [np.linalg.norm(ref.edge_block(e, ypr[:, 0], h["vio_T"], ypr[:, 1], ypr[:, 2], dict(P, huber=1e300))[0]) for e in edges if e[4]]
    assert abs(norms[0] - 0.05) < 1e-9 and abs(norms[1] - 3.0) < 1e-9 and norms[0] < P["huber"] < norms[1]
    ypr = np.array([ref.R2ypr(R) for R in C_["pitch_roll"]["vio_R"]])
    assert abs(ypr[:, 1].mean() - 30.0) < 1.0 and abs(ypr[:, 2].mean() + 20.0) < 1.0
    two = C_["two_sequences"]
    assert not any(two["sequence"][e[0]] != two["sequence"][e[1]] for e in ref.build_edges(two["vio_R"], two["vio_T"], two["sequence"], []))
    none = run(ref, C_["no_loops"])
    assert none["result"]["flags"] == ref.F_GRADIENT | ref.F_FINITE and none["result"]["iterations"] == 0 and none["result"]["cost0"] < 1e-20
    assert np.array_equal(none["t"], C_["no_loops"]["vio_T"])
    zero = run(ref, C_["max_iterations_0"])
    assert zero["result"]["flags"] == ref.F_MAX_ITERATIONS | ref.F_FINITE and zero["result"]["iterations"] == 0 and zero["result"]["cost1"] == zero["result"]["cost0"] > 0


def test_reject_case_rejects_and_halves_the_radius():
    out = run(ref, cs.reject_case(), max_iterations=8)
    H = out["history"]
    k = int(np.argmax(H[:, 4] == 0.0))
    print("rho per attempt:", H[:, 2], "accepted:", H[:, 4], "mu:", H[:, 3])
    assert H[k, 4] == 0.0 and k == 4 and np.all(H[:k, 4] == 1.0)
    assert H[k + 1, 3] == H[k, 3] / 2.0 and H[k + 1, 0] == H[k, 0]          # the halved radius, the unchanged state
    if H[k + 1, 4] == 0.0:
        assert H[k + 2, 3] == H[k + 1, 3] / 4.0                             # the next rejection divides by the doubled factor


def scipy_converged(c):
    P = cs.params_of(c)
    n = len(c["vio_T"])
    ypr = np.array([ref.R2ypr(R) for R in c["vio_R"]])
    edges = ref.build_edges(c["vio_R"], c["vio_T"], c["sequence"], c["loops"])
    free = [k for k in range(n) if not c["fixed"][k]]
    plain = dict(P, huber=1e300)

    def unpack(x):
        yaw, t = ypr[:, 0].copy(), np.array(c["vio_T"], float)
        for a, k in enumerate(free):
            yaw[k], t[k] = x[4 * a], x[4 * a + 1:4 * a + 4]
        return yaw, t

    def fun(x):                                  # r sqrt(rho(s) / s) per block: the sum of squares is the Huber cost (scipy's own loss is per scalar)
        yaw, t = unpack(x)
        out = []
        for e in edges:
            r = ref.edge_block(e, yaw, t, ypr[:, 1], ypr[:, 2], plain)[0]
            s, a = float(r @ r), P["huber"]
            if e[4] and s > a * a:
                r = r * math.sqrt((2 * a * math.sqrt(s) - a * a) / s)
            out.append(r)
        return np.concatenate(out)

    x0 = np.concatenate([[ypr[k, 0], *c["vio_T"][k]] for k in free])
    sol = least_squares(fun, x0, method="trf", jac="3-point", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=2000)
    return unpack(sol.x), sol.cost


@pytest.mark.parametrize("name", SCIPY_CASES)
def test_restatement_converges_to_scipys_minimum(name):
    c = cs.small_cases()[name]
    out = run(ref, c, max_iterations=64, function_tolerance=1e-15, gradient_tolerance=1e-15, parameter_tolerance=1e-15)
    (yaw, t), cost = scipy_converged(c)
    dt, dy = float(np.max(np.abs(t - out["t"]))), cs.yaw_diff(yaw, out["ypr"][:, 0])
    print(name, f"iterations {out['result']['iterations']} flags {out['result']['flags']} |dt| {dt:.3e} m |dyaw| {dy:.3e} deg cost {out['result']['cost1']:.12g} scipy {cost:.12g}")
    assert dt <= SCIPY_TOL_M and dy <= SCIPY_TOL_DEG and abs(out["result"]["cost1"] - cost) <= 1e-12 * max(cost, 1.0)


# the four deliberate errors: (what, the text of the restatement it replaces, the replacement)
MUTATIONS = [
    ("pi / 180 missing from the yaw column", "    return D2R * np.array([[-sy * cp,", "    return np.array([[-sy * cp,"),
    ("sqrt(rho') replaced by rho'", "k = math.sqrt(rho1)", "k = rho1"),
    ("pitch / roll taken from `to`", "    pr = i\n", "    pr = j\n"),
    ("the loop's yaw scale on the translation rows", "r[:3] = R.T @ d - rel_t", "r[:3] = w * (R.T @ d - rel_t)"),
]


@pytest.mark.parametrize("what,old,new", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_a_deliberate_error_fails_the_exact_comparison(what, old, new):
    src = open(ref.__file__).read()
    assert src.count(old) == 1, (what, src.count(old))
    mod = types.ModuleType("pg4_reference_mutated")
    exec(compile(src.replace(old, new), "pg4_reference_mutated", "exec"), mod.__dict__)
    failed = []
    for name in SMALL:
        try:
            ok = cs.within(worst_against_exact(mod, name), cs.CPU_TOL)
        except AssertionError:                   # a decision, a count or a flag differs
            ok = False
        if not ok:
            failed.append(name)
    print(what, "-> fails", failed)
    assert failed, what


# ---- VisualPoseGraph with the restatement as its back-end ---------------------------------------------------------------------------------------------------------
class StubStore:
    """findConnection from a table {(cur, old): (relative_t, relative_q (w, x, y, z), relative_yaw)}; every other pair has no loop"""

    def __init__(self, table=None):
        self.table, self.calls, self.s = dict(table or {}), [], None

    def findConnection(self, cur, olds, qic, tic, params=None):
        self.calls.append((cur, list(olds)))
        rows = []
        for o in olds:
            hit = self.table.get((cur, o))
            rows.append(dict(has_loop=hit is not None, relative_t=hit[0] if hit else np.zeros(3), relative_q=hit[1] if hit else np.array([1.0, 0, 0, 0]),
                             relative_yaw=hit[2] if hit else 0.0))
        return rows


def quat_wxyz(R):
    from vil_fusion_amd import synth
    q = synth.R_to_q(R)
    return np.array([q[3], q[0], q[1], q[2]])


def loop_info(R_old, T_old, R_cur, T_cur):
    """relative_t, relative_q, relative_yaw as findConnection defines them (keyframe.cpp:472-487), from true poses"""
    return R_old.T @ (T_cur - T_old), quat_wxyz(R_old.T @ R_cur), ref.normalize_angle(R2ypr(R_cur)[0] - R2ypr(R_old)[0])


def world_path(n, seed):
    rng = np.random.default_rng(seed)
    yaw = np.cumsum(5.0 * rng.standard_normal(n))
    T = np.cumsum(np.stack([np.cos(yaw * ref.D2R), np.sin(yaw * ref.D2R), 0.02 * rng.standard_normal(n)], axis=1), axis=0)
    return [ypr2R(np.array([yaw[k], 1.5, -2.0])) for k in range(n)], T


def test_sequence_shift_on_a_cross_sequence_loop():
    Rw, Tw = world_path(12, 1)
    Rs, Ts = ypr2R(np.array([40.0, 0.0, 0.0])), np.array([5.0, -3.0, 0.4])                  # sequence 1 reports its poses in a frame of its own: world = Rs vio + Ts
    table = {(8, 2): loop_info(Rw[2], Tw[2], Rw[8], Tw[8]), (10, 3): loop_info(Rw[3], Tw[3], Rw[10], Tw[10])}
    g = VisualPoseGraph(StubStore(table), backend=ref.Backend())
    for k in range(6):
        assert g.addKeyFrame(k, 0, Rw[k], Tw[k]) == -1
    for k in range(6, 12):
        got = g.addKeyFrame(k, 1, Rs.T @ Rw[k], Rs.T @ (Tw[k] - Ts), candidates={7: [1], 8: [2], 10: [3]}.get(k, []))
        assert got == {8: 2, 10: 3}.get(k, -1)
        if k == 7:
            assert g.sequence_loop == [0, 0] and np.array_equal(g.w_r_vio, np.eye(3))      # verified, no loop: nothing moves
        if k >= 8:
            assert g.sequence_loop == [0, 1]
    assert g.earliest_loop_index == 2 and g.sequence_cnt == 1
    assert np.allclose(g.w_r_vio, Rs, atol=1e-12) and np.allclose(g.w_t_vio, Ts, atol=1e-9)
    for k in range(6, 12):                                                                   # the key frames before the loop, the looped one and the later ones
        T, R = g.getVioPose(k)
        assert np.allclose(T, Tw[k], atol=1e-9) and np.allclose(R, Rw[k], atol=1e-12), k
    res = g.optimize4DoF()
    assert res["nodes"] == list(range(2, 11)) and res["cost0"] < 1e-16                       # the shifted sequence agrees with the loops: nothing to do
    assert g.optimize4DoF() is None


def test_drift_is_applied_to_key_frames_after_an_optimisation():
    c = cs.make(14, 41, [(1, 10)])
    table = {(10, 1): (c["loops"][0][2], np.array([1.0, 0, 0, 0]), c["loops"][0][3])}
    g = VisualPoseGraph(StubStore(table), backend=ref.Backend())
    for k in range(11):
        g.addKeyFrame(k, 1, c["vio_R"][k], c["vio_T"][k], candidates=[1] if k == 10 else [], time_stamp=100.0 + 0.1 * k)
    for k in range(11):                                                                      # before the optimisation a pose is the VIO's
        assert np.array_equal(g.getPose(k)[0], c["vio_T"][k])
    g.addKeyFrame(11, 1, c["vio_R"][11], c["vio_T"][11])                                     # in the graph before the call, after the newest looped key frame
    res = g.optimize4DoF()
    want = ref.optimize(c["vio_R"][1:11], c["vio_T"][1:11], [1] * 10, [1] + [0] * 9, [(0, 9, c["loops"][0][2], c["loops"][0][3])])
    assert res["nodes"] == list(range(1, 11)) and res["iterations"] == want["result"]["iterations"] and res["cost1"] < res["cost0"]
    for k in range(1, 11):
        assert np.array_equal(g.getPose(k)[0], want["t"][k - 1]) and np.array_equal(g.getPose(k)[1], want["R"][k - 1])
    assert np.array_equal(g.getPose(0)[0], c["vio_T"][0])                                    # before earliest_loop_index: untouched
    yaw_drift = R2ypr(want["R"][9])[0] - R2ypr(c["vio_R"][10])[0]
    r_drift = ypr2R(np.array([yaw_drift, 0.0, 0.0]))
    t_drift = want["t"][9] - r_drift @ c["vio_T"][10]
    assert abs(g.yaw_drift - yaw_drift) < 1e-12 and np.allclose(g.r_drift, r_drift, atol=1e-14) and np.allclose(g.t_drift, t_drift, atol=1e-12)
    assert abs(g.yaw_drift) > 1e-3 and np.linalg.norm(g.t_drift) > 1e-3
    for k in (12, 13):
        g.addKeyFrame(k, 1, c["vio_R"][k], c["vio_T"][k])
    for k in (11, 12, 13):                                                                   # the one that was waiting and the ones added afterwards
        T, R = g.getPose(k)
        assert np.allclose(T, g.r_drift @ c["vio_T"][k] + g.t_drift, atol=1e-12) and np.allclose(R, g.r_drift @ c["vio_R"][k], atol=1e-14)
        assert np.array_equal(g.getVioPose(k)[0], c["vio_T"][k])


def test_no_loop_leaves_everything_untouched(tmp_path):
    c = cs.make(8, 42, [])
    store = StubStore()
    g = VisualPoseGraph(store, backend=ref.Backend())
    for k in range(8):
        assert g.addKeyFrame(k, 1, c["vio_R"][k], c["vio_T"][k], candidates=list(range(max(0, k - 3), k)), time_stamp=1403636579.763555527 + k) == -1
    assert len(store.calls) == 7 and store.calls[-1] == (7, [4, 5, 6])
    assert g.earliest_loop_index == -1 and g.optimize4DoF() is None and g.sequence_loop == [0, 0]
    for k in range(8):
        T, R = g.getPose(k)
        assert np.array_equal(T, c["vio_T"][k]) and np.array_equal(R, c["vio_R"][k])
    with pytest.raises(ValueError):
        g.addKeyFrame(3, 1, c["vio_R"][3], c["vio_T"][3])
    with pytest.raises(ValueError):
        g.addKeyFrame(9, 3, c["vio_R"][3], c["vio_T"][3])
    path = tmp_path / "loop_path.txt"
    g.save_tum(str(path))
    lines = path.read_text().splitlines()
    assert len(lines) == 8
    for k, line in enumerate(lines):                                                         # stamp with 9 digits, the rest with 5, single spaces, no trailing space
        assert re.fullmatch(r"\d+\.\d{9}( -?\d+\.\d{5}){7}", line), line
        v = [float(s) for s in line.split()]
        assert abs(v[0] - (1403636579.763555527 + k)) < 1e-6 and np.allclose(v[1:4], c["vio_T"][k], atol=5.1e-6)
        q = np.array(v[4:8])
        assert abs(np.linalg.norm(q) - 1.0) < 2e-5 and np.allclose(quat_wxyz(c["vio_R"][k])[[1, 2, 3, 0]], q, atol=5.1e-6)


def test_ctypes_mirrors_match_the_c_layout(tmp_path):
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "vilfusion.h"', "int main(void) {"]
    checks = []
    for cname, ct in (("vilf_pg4_params", abi.Pg4Params), ("vilf_pg4_loop", abi.Pg4Loop), ("vilf_pg4_result", abi.Pg4Result)):
        prog.append(f'  printf("%zu\\n", sizeof({cname}));')
        checks.append((cname, "sizeof", C.sizeof(ct)))
        for fname, _ in ct._fields_:
            prog.append(f'  printf("%zu\\n", offsetof({cname}, {"from" if fname == "from_" else fname}));')
            checks.append((cname, fname, getattr(ct, fname).offset))
    prog += ['  printf("%d %d %d %d %d %d %d\\n", VILF_PG4_BAND, VILF_PG4_MAX_ITERATIONS, VILF_PG4_FUNCTION, VILF_PG4_GRADIENT, VILF_PG4_PARAMETER, VILF_PG4_RADIUS, VILF_PG4_FINITE);',
             "  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(prog))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    flags = [abi.VILF_PG4_BAND, abi.VILF_PG4_MAX_ITERATIONS, abi.VILF_PG4_FUNCTION, abi.VILF_PG4_GRADIENT, abi.VILF_PG4_PARAMETER, abi.VILF_PG4_RADIUS, abi.VILF_PG4_FINITE]
    assert [int(v) for v in out[-7:]] == flags == [ref.BAND, ref.F_MAX_ITERATIONS, ref.F_FUNCTION, ref.F_GRADIENT, ref.F_PARAMETER, ref.F_RADIUS, ref.F_FINITE]
    for (cname, fname, want), got in zip(checks, out[:-7]):
        assert int(got) == want, (cname, fname, got, want)
