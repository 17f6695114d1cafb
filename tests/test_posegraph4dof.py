"""The 4-DoF pose graph of the visual loop closure on the device (vilf_pg4_optimize, BackendSolver.optimize4dof, VisualPoseGraph): the small cases against the
40-digit run of tests/pg4_exact.py, the reject branch attempt by attempt, the layout edges and the two laps against tests/pg4_reference.py (itself measured in
tests/test_posegraph4dof_reference.py), every refusal of the contract in include/vilfusion.h, and the stage's memory after vilf_destroy."""
import ctypes as C
import numpy as np
import pytest
import torch          # before the first handle: torch brings a HIP runtime of its own, and the one loaded first serves the process
import pg4_cases as cs
import pg4_reference as ref
from vil_fusion_amd import abi

pytestmark = pytest.mark.gpu
SMALL = list(cs.small_cases())
LAYOUT = cs.layout_cases()
INV, UNSUP = abi.VILF_ERR_INVALID_ARGUMENT, abi.VILF_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def solver():
    from vil_fusion_amd.estimator import BackendSolver
    s = BackendSolver()
    yield s
    s.close()


def run(solver, c, **over):
    return solver.optimize4dof(c["vio_R"], c["vio_T"], c["sequence"], c["fixed"], c["loops"], params=cs.params_of(c, **over))


def run_ref(c, **over):
    return ref.optimize(c["vio_R"], c["vio_T"], c["sequence"], c["fixed"], c["loops"], cs.params_of(c, **over))


def against_exact(solver, name, c, tol):
    worst = {}
    for k, snap in cs.exact(name).items():
        out = run(solver, c, max_iterations=k)
        fig = cs.compare(out, snap)                      # decisions, counts and flags are asserted equal inside
        for q, v in fig.items():
            worst[q] = max(worst.get(q, 0.0), v)
        assert np.allclose(out["R"], np.array([ref.ypr2R(*row) for row in out["ypr"]]), atol=1e-15)
        d = ref.drift(out["R"][-1], out["t"][-1], c["vio_R"][-1], c["vio_T"][-1])
        assert abs(out["result"]["yaw_drift"] - d["yaw_drift"]) <= 1e-12 and np.allclose(out["result"]["r_drift"], d["r_drift"], atol=1e-14)
        assert np.allclose(out["result"]["t_drift"], d["t_drift"], atol=1e-12 * max(1.0, float(np.max(np.abs(c["vio_T"])))))
    print(name, {q: f"{v:.3e}" for q, v in worst.items()}, tol)
    assert cs.within(worst, tol), (worst, tol)


@pytest.mark.parametrize("name", SMALL)
def test_small_cases_against_exact(solver, name):
    against_exact(solver, name, cs.small_cases()[name], cs.GPU_TOL)


def test_no_loops_returns_the_start(solver):
    c = cs.small_cases()["no_loops"]
    out = run(solver, c)
    r = out["result"]
    assert r["flags"] == abi.VILF_PG4_GRADIENT | abi.VILF_PG4_FINITE and r["iterations"] == 0 and r["cost0"] < 1e-20 and r["cost1"] == r["cost0"]
    assert np.array_equal(out["t"], c["vio_T"]) and np.allclose(out["R"], c["vio_R"], atol=1e-15) and len(out["history"]) == 0


def test_reject_branch(solver):
    c = cs.reject_case()
    against_exact(solver, "reject", c, cs.GPU_TOL_REJECT)
    out, want = run(solver, c, max_iterations=8), run_ref(c, max_iterations=8)
    H = out["history"]
    print("rho:", H[:, 2], "accepted:", H[:, 4], "mu:", H[:, 3])
    assert np.array_equal(H[:, 4], want["history"][:, 4]) and np.array_equal(H[:, 4], [1, 1, 1, 1, 0, 0, 0, 0])
    assert out["result"]["accepted"] == 4 and out["result"]["pivot_rejections"] == 0 and out["result"]["flags"] == abi.VILF_PG4_MAX_ITERATIONS | abi.VILF_PG4_FINITE
    assert H[4, 2] < 0.4 < H[3, 2]                                                   # the rejected attempt
    assert H[5, 3] == H[4, 3] / 2.0 and H[6, 3] == H[5, 3] / 4.0 and H[7, 3] == H[6, 3] / 8.0 and out["result"]["radius"] == H[7, 3] / 16.0      # the radius and the factor
    assert np.all(H[4:, 0] == H[4, 0]) and out["result"]["cost1"] == H[4, 0]         # the unchanged state
    four = run(solver, c, max_iterations=4)
    assert np.array_equal(out["t"], four["t"]) and np.array_equal(out["ypr"], four["ypr"])


@pytest.mark.parametrize("name", list(LAYOUT))
def test_layout_edges_against_the_restatement(solver, name):
    c = LAYOUT[name]
    one, want = run(solver, c, max_iterations=1), run_ref(c, max_iterations=1)
    dt, dy = float(np.max(np.abs(one["t"] - want["t"]))), cs.yaw_diff(one["ypr"][:, 0], want["ypr"][:, 0])
    print(name, f"one attempt: |dt| {dt:.3e} m |dyaw| {dy:.3e} deg")
    assert one["result"]["accepted"] == want["result"]["accepted"] == 1
    assert dt <= cs.LAYOUT_TOL["t"] and dy <= cs.LAYOUT_TOL["yaw"]
    five, want5 = run(solver, c), run_ref(c)
    assert np.array_equal(five["history"][:, 4], want5["history"][:, 4]) and five["result"]["flags"] == want5["result"]["flags"]
    assert five["result"]["iterations"] == want5["result"]["iterations"] and abs(five["result"]["cost1"] - want5["result"]["cost1"]) <= 1e-10 * want5["result"]["cost1"]


def raw_call(solver, c, P=None, n=None, loops=None, null=None, fixed=None, vio_R=None, vio_T=None):
    """vilf_pg4_optimize itself, with sentinel-filled outputs -> (status, whether anything was written)"""
    from vil_fusion_amd.estimator import pg4_default_params
    p = pg4_default_params(**(P or {}))
    R = np.ascontiguousarray(c["vio_R"] if vio_R is None else vio_R, dtype=np.float64).reshape(-1, 9)
    T = np.ascontiguousarray(c["vio_T"] if vio_T is None else vio_T, dtype=np.float64).reshape(-1, 3)
    seq = np.ascontiguousarray(c["sequence"], dtype=np.int32)
    fx = np.ascontiguousarray(c["fixed"] if fixed is None else fixed, dtype=np.int32)
    loops = c["loops"] if loops is None else loops
    arr = (abi.Pg4Loop * max(len(loops), 1))()
    for k, (a, b, rel_t, rel_yaw) in enumerate(loops):
        arr[k].from_, arr[k].to, arr[k].rel_yaw = int(a), int(b), float(rel_yaw)
        arr[k].rel_t[:] = [float(v) for v in rel_t]
    m = len(T)
    outs = [np.full((m, 3), 7.25), np.full((m, 3), 7.25), np.full((m, 9), 7.25), np.full((64, 5), 7.25)]
    res = abi.Pg4Result()
    C.memset(C.byref(res), 0x5a, C.sizeof(res))
    before = bytes(res)
    ip = C.POINTER(C.c_int)
    args = dict(p=C.byref(p), vio_R=abi.dptr(R), vio_T=abi.dptr(T), sequence=seq.ctypes.data_as(ip), fixed=fx.ctypes.data_as(ip), loops=arr, t_out=abi.dptr(outs[0]),
                ypr_out=abi.dptr(outs[1]), R_out=abi.dptr(outs[2]), result=C.byref(res))
    if null:
        args[null] = None
    rc = solver._L.vilf_pg4_optimize(solver._h, args["p"], m if n is None else n, args["vio_R"], args["vio_T"], args["sequence"], args["fixed"], len(loops), args["loops"],
                                     args["t_out"], args["ypr_out"], args["R_out"], args["result"], abi.dptr(outs[3]))
    return rc, any(np.any(o != 7.25) for o in outs) or bytes(res) != before


def test_refusals_write_nothing_and_leave_the_handle_good(solver):
    from vil_fusion_amd.estimator import BackendSolver
    c = cs.small_cases()["three_loops"]
    fresh = BackendSolver()
    try:
        want = run(fresh, c)
    finally:
        fresh.close()
    nan, inf = float("nan"), float("inf")
    bad_R, bad_T = np.array(c["vio_R"]), np.array(c["vio_T"])
    bad_R[3, 1, 2], bad_T[11, 0] = nan, inf
    L0 = c["loops"][0]
    refused = [dict(null=k) for k in ("p", "vio_R", "vio_T", "sequence", "fixed", "loops", "t_out", "ypr_out", "R_out", "result")]
    refused += [dict(n=0), dict(n=-3), dict(fixed=[0] + [1] * 11), dict(vio_R=bad_R), dict(vio_T=bad_T)]
    refused += [dict(loops=[bad]) for bad in ((5, 5, L0[2], L0[3]), (7, 3, L0[2], L0[3]), (-1, 4, L0[2], L0[3]), (2, 12, L0[2], L0[3]), (0, 11, [0.0, nan, 0.0], 1.0), (0, 11, L0[2], inf))]
    refused += [dict(P=P) for P in (dict(max_iterations=-1), dict(max_iterations=65), dict(initial_radius=0.0), dict(initial_radius=nan), dict(max_radius=-1.0), dict(min_radius=0.0),
                                    dict(huber=0.0), dict(huber=inf), dict(loop_yaw_scale=-0.1), dict(min_relative_decrease=-1e-3), dict(function_tolerance=nan),
                                    dict(gradient_tolerance=-1.0), dict(parameter_tolerance=inf))]
    for kw in refused:
        rc, written = raw_call(solver, c, **kw)
        assert rc == INV and not written, (kw, rc, written)
        again = run(solver, c)
        assert np.array_equal(again["t"], want["t"]) and np.array_equal(again["ypr"], want["ypr"]) and np.array_equal(again["history"], want["history"]), kw
    rc, written = raw_call(solver, c, loops=[L0] * 3073)                     # 4 n_loops = 12292 > 12288
    assert rc == UNSUP and not written
    assert b"3073 loops" in solver._L.vilf_last_error(solver._h)
    again = run(solver, c)
    assert np.array_equal(again["t"], want["t"]) and np.array_equal(again["ypr"], want["ypr"]) and np.array_equal(again["history"], want["history"])
    rc, written = raw_call(solver, c, loops=[L0] * 3)                        # and a good raw call does write
    assert rc == 0 and written


# a stage buffer holds at least its rounding pad (DBuf: bytes / 8 + 256)
SMALLEST_BUFFER = 256


def test_destroy_returns_the_stage_memory():
    from vil_fusion_amd.estimator import BackendSolver
    c = LAYOUT["L33"]
    first, free = None, []
    for k in range(3):
        s = BackendSolver()
        try:
            out = run(s, c)
        finally:
            s.close()
        first = out if first is None else first
        assert np.array_equal(out["t"], first["t"]) and np.array_equal(out["history"], first["history"])
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    print("free bytes after destroy 1, 2, 3:", free)
    assert free[0] - free[2] <= SMALLEST_BUFFER, free


class StubStore:
    def __init__(self, table):
        self.table, self.s = table, None

    def findConnection(self, cur, olds, qic, tic, params=None):
        return [dict(has_loop=(cur, o) in self.table, relative_t=self.table.get((cur, o), (np.zeros(3), 0.0))[0], relative_q=np.array([1.0, 0, 0, 0]),
                     relative_yaw=self.table.get((cur, o), (np.zeros(3), 0.0))[1]) for o in olds]


def ate(t, gt):
    return float(np.sqrt(np.mean(np.sum((np.asarray(t) - gt) ** 2, axis=1))))


def test_two_laps_end_to_end(solver):
    from vil_fusion_amd.visual_posegraph import VisualPoseGraph
    c = cs.two_laps()
    n, gt = len(c["vio_T"]), c["gt"][1]
    table = {(b, a): (rel_t, rel_yaw) for (a, b, rel_t, rel_yaw) in c["loops"]}
    graphs = [VisualPoseGraph(StubStore(table), backend=solver), VisualPoseGraph(StubStore(table), backend=ref.Backend())]
    results = []
    for g in graphs:
        for k in range(n):
            g.addKeyFrame(k, 1, c["vio_R"][k], c["vio_T"][k], candidates=[k - n // 2] if k >= n // 2 else [], time_stamp=0.1 * k)
        results.append(g.optimize4DoF())
    dev, want = results
    assert dev["nodes"] == want["nodes"] == list(range(0, c["loops"][-1][1] + 1)) and len(c["loops"]) == 14
    T = [np.array([g.getPose(k)[0] for k in range(n)]) for g in graphs]
    Y = [np.array([ref.R2ypr(g.getPose(k)[1])[0] for k in range(n)]) for g in graphs]
    dt, dy = float(np.max(np.abs(T[0] - T[1]))), cs.yaw_diff(Y[0], Y[1])
    print(f"two laps: |dt| {dt:.3e} m |dyaw| {dy:.3e} deg; cost {dev['cost0']:.6g} -> {dev['cost1']:.6g}; ATE {ate(c['vio_T'], gt):.4f} m -> {ate(T[0], gt):.4f} m "
          f"(restatement {ate(T[1], gt):.4f} m); iterations {dev['iterations']} flags {dev['flags']}")
    assert dt <= cs.LAYOUT_TOL["t"] and dy <= cs.LAYOUT_TOL["yaw"]
    assert dev["cost1"] <= dev["cost0"] and dev["iterations"] == want["iterations"] and dev["flags"] == want["flags"]
    assert np.array_equal(dev["history"][:, 4], want["history"][:, 4])
    direct = run(solver, dict(c, vio_R=c["vio_R"][:len(dev["nodes"])], vio_T=c["vio_T"][:len(dev["nodes"])], sequence=c["sequence"][:len(dev["nodes"])], fixed=c["fixed"][:len(dev["nodes"])]))
    assert np.array_equal(direct["t"], T[0][:len(dev["nodes"])])                    # the class adds nothing to the numbers
