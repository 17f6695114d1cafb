"""The scan-to-map pose solve (b_solve) per iteration, against a restatement of the reference's and Ceres' rules and an exact tier (tests/s2m_solve_reference.py) on
designed factor records (tests/s2m_solve_cases.py). DESIGN 3m says what each tier measures and which planted errors each test catches.

CPU: the cases hit their targets, every case is decided through its last iteration, the restatement meets the derived first-evaluation bound. GPU: the test hook
vilf_debug_s2m_solve (the production grid of b_solve's twin with a per-iteration trace) against the exact tier: row 0 within the derived bound, every later row's
flags, stop reason and iteration count equal, iterates, costs, radius within the measured tolerance (64 x the restatement's own error at that row); the refusals; the
proof that the hook leaves no trace; and one scene on which the two hooks, association then solve, reproduce vilf_scan2map_step pass by pass."""
import ctypes as C
import functools
import numpy as np
import mpmath as mp
import pytest
from vil_fusion_amd import abi
import s2m_solve_reference as R
import s2m_solve_cases as cases_mod
from s2m_scene import scene as _scene

CASES = cases_mod.all_cases()
CASE_BY_NAME = {c["name"]: c for c in CASES}
NAMES = [c["name"] for c in CASES]
TR = 64                                    # doubles per trace row (S2M_TR)
WHY = dict(parameter=R.STOP_PARAMETER, function=R.STOP_FUNCTION, gradient=R.STOP_GRADIENT, budget=R.STOP_BUDGET)
fpp = C.POINTER(C.c_float)
ipp = C.POINTER(C.c_int)
INVALID = -1                               # VILF_ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------------------------------------------------------ references, computed once and shared
def _prepare(c):
    if "mp" not in c:
        mp.mp.dps = R.MP_DIGITS
        src = c["mp_src"]
        c["mp"] = dict(kind=src["kind"], rec=R.MPF.arr(src["rec"]), cp=R.MPF.arr(src["cp"]), mult=src["mult"])
    return c


@functools.lru_cache(maxsize=None)
def tiers(name):
    """(restatement, exact tier) of a case"""
    c = _prepare(CASE_BY_NAME[name])
    r = R.restate(c)
    return r, R.exact(c, r)


def _sums(row0):
    return list(row0["H"]) + list(row0["g"]) + [row0["cost"]]


def _fl(v):
    return float(v)


def _err(a, b):
    """|a - b| of a float against an mpf, exactly"""
    return abs(float(mp.mpf(float(a)) - b))


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_cases_hit_their_targets():
    seen_why = set()
    for c in CASES:
        r, e = tiers(c["name"])
        t = c["target"]
        rows = e["rows"][1:]
        seen_why.add(e["why"])
        nq = c["n_edge_q"] + c["n_surf_q"]
        assert len(c["kind_slot"]) == nq and set(c["kind_slot"].tolist()) <= {0, 1, 2, 3}
        assert (c["kind_slot"][:c["n_edge_q"]] != 2).all() and (c["kind_slot"][c["n_edge_q"]:] != 1).all()
        assert (c["nfe"], c["nfs"]) == (int((c["kind_slot"] == 1).sum()), int((c["kind_slot"] == 2).sum()))
        if "its" in t:
            assert e["its"] == t["its"], c["name"]
        if "why" in t:
            assert e["why"] == WHY[t["why"]], (c["name"], e["why"])
        if "clamped" in t:
            assert rows and sum(rows[0]["clamped"]) == t["clamped"], (c["name"], rows[0]["clamped"])
        if "small" in t:
            assert rows[0]["small"] and _fl(rows[0]["theta"]) == 0.0 and all(_fl(v) == 0.0 for v in e["rows"][0]["g"][:3]), c["name"]
        if "n_valid" in t:
            assert c["n_valid"] == t["n_valid"]
        if "nfac" in t:
            assert nq == t["nfac"] and c["kind_slot"][-1] in (1, 2)
        if "nfe" in t:
            assert c["nfe"] == t["nfe"] and c["nfs"] == 0
        if "nfs" in t:
            assert c["nfs"] == t["nfs"] and c["nfe"] == 0
        if "reject_then_accept" in t:
            fl = [(w["valid"], w["accept"], w["stop"]) for w in rows]
            k = fl.index((1, 0, 0))
            assert (1, 1, 0) in fl[k + 1:], fl
        if "outer" in t:
            ev = R.evaluate(R.MPF, [mp.mpf(float(v)) for v in c["pose"]], c)
            assert int(np.sum(ev["outer"])) == t["outer"], c["name"]
            if t["outer"] == 0:                 # ON the threshold: s == a^2 exactly, in the exact tier and in float64
                evf = R.evaluate(R.F64, [float(v) for v in c["pose"]], c)
                assert all(s == mp.mpf(c["huber_a"]) ** 2 for s in ev["s"]) and (evf["s"] == c["huber_a"] ** 2).all()
        if "w_negative" in t:
            assert c["pose"][3] < 0
        if "far" in t:
            assert np.linalg.norm(c["pose"][4:]) > 300
        if c["name"].startswith("c_") and nq > 256 and c["name"] != "c_all_invalid":
            assert c["kind_slot"][-1] in (0, 3) and all(c["kind_slot"][k] in (0, 3) for k in range(0, nq, 256))
    assert {R.STOP_PARAMETER, R.STOP_FUNCTION, R.STOP_GRADIENT, R.STOP_BUDGET} <= seen_why
    assert {CASE_BY_NAME[n]["max_it"] for n in ("g_it0", "g_it1", "g_it4", "g_it50")} == {0, 1, 4, 50}
    assert {c["stream"] for c in CASES} == {2, -1}


def test_every_case_is_fully_decided():
    """no exemption: every decision of every iteration of every case, in the exact tier; the restatement takes the same decisions; no step is invalid"""
    for c in CASES:
        r, e = tiers(c["name"])
        assert e["all_decided"], (c["name"], e["undecided"])
        assert r["its"] == e["its"] and r["why"] == e["why"], c["name"]
        for a, b in zip(r["rows"][1:], e["rows"][1:]):
            assert (a["valid"], a["accept"], a["stop"], a["reason"], a["clamped"], a["small"]) == (b["valid"], b["accept"], b["stop"], b["reason"], b["clamped"], b["small"]), c["name"]
            assert b["valid"] == 1, c["name"]
        assert e["why"] != R.STOP_INVALID


def test_restatement_meets_the_first_evaluation_bound():
    worst = {}
    for c in CASES:
        r, e = tiers(c["name"])
        if not e["rows"]:
            continue
        B = e["rows"][0]["bound"]
        ratio = 0.0
        for k, (a, b) in enumerate(zip(_sums(r["rows"][0]), _sums(e["rows"][0]))):
            d = _err(a, b)
            assert d <= B[k], (c["name"], k, d, B[k])
            ratio = max(ratio, d / B[k] if B[k] > 0 else 0.0)
        rows = [R.tolerance_x(a["cand"], b["cand"]) / R.SAFETY for a, b in zip(r["rows"][1:], e["rows"][1:])]
        worst[c["name"]] = (ratio, max(rows) if rows else 0.0, R.tolerance_x(r["pose"], e["pose"]) / R.SAFETY)
    print("case: restatement error / first-evaluation bound, largest iterate error over the rows, final pose error")
    for k, v in worst.items():
        print(f"  {k:24s} {v[0]:.4f} {v[1]:.2e} {v[2]:.2e}")


def test_oracle_is_held_to_the_restatement():
    """oracle/scan2map.cpp's own cost functions and solve on the cases' records (vilo_s2m_solve_factors): identical iteration counts, pose and cost within the
    measured tolerance"""
    import oracle_lib
    L = oracle_lib.lib()
    fn = L.vilo_s2m_solve_factors
    fn.argtypes = [C.POINTER(abi.Options), abi.c_double_p, C.c_int, ipp, abi.c_double_p, fpp, C.c_int, ipp, abi.c_double_p]
    fn.restype = C.c_int
    worst = 0.0
    for c in CASES:
        r, e = tiers(c["name"])
        o = oracle_lib.default_options()
        o.huber_a = c["huber_a"]
        pose = c["pose"].copy(); its = np.zeros(1, dtype=np.int32); cost = np.zeros(1)
        kind = np.ascontiguousarray(c["kind_slot"]); rec = np.ascontiguousarray(c["rec_slot"]); cp = np.ascontiguousarray(c["cp_slot"], dtype=np.float32)
        assert fn(C.byref(o), abi.dptr(pose), len(kind), kind.ctypes.data_as(ipp), abi.dptr(rec), cp.ctypes.data_as(fpp), c["max_it"], its.ctypes.data_as(ipp), abi.dptr(cost)) == 0
        assert int(its[0]) == r["its"], (c["name"], int(its[0]), r["its"])
        d = np.sqrt(sum(_err(a, b) ** 2 for a, b in zip(pose, e["pose"])))
        tol = R.tolerance_x(r["pose"], e["pose"])
        worst = max(worst, d / tol)
        assert d <= tol, (c["name"], d, tol)
        if c["n_valid"]:
            assert _err(cost[0], e["cost"]) <= max(R.tolerance_scalar(r["cost"], e["cost"]), e["d_cost"]), c["name"]
    print(f"oracle against the exact tier: largest pose error / tolerance {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------ GPU
def hook_fn(L):
    fn = L.vilf_debug_s2m_solve
    fn.argtypes = [C.c_void_p, C.c_int, abi.c_double_p, C.c_int, C.c_int, ipp, abi.c_double_p, fpp, C.c_double, C.c_int, C.c_int,
                   abi.c_double_p, abi.c_double_p, ipp, ipp, ipp, abi.c_double_p, C.c_int]
    fn.restype = C.c_int
    return fn


def fresh_outputs(trace_rows):
    return dict(pose=np.full(7, -7.0), cost=np.full(1, -7.0), its=np.full(1, -7, dtype=np.int32), nfe=np.full(1, -7, dtype=np.int32), nfs=np.full(1, -7, dtype=np.int32),
                trace=np.full((max(trace_rows, 1), TR), -7.0))


def call_hook(solver, stream, pose, ne, ns, kind, rec, cp, huber_a, max_it, pass_=0, trace_rows=cases_mod.TRACE_ROWS, null=()):
    kind = np.ascontiguousarray(kind, dtype=np.int32); rec = np.ascontiguousarray(rec, dtype=np.float64); cp = np.ascontiguousarray(cp, dtype=np.float32)
    pose = np.ascontiguousarray(pose, dtype=np.float64)
    o = fresh_outputs(trace_rows)
    ip = lambda a: a.ctypes.data_as(ipp)
    args = dict(kind=ip(kind), rec=abi.dptr(rec), cp=cp.ctypes.data_as(fpp), pose_out=abi.dptr(o["pose"]), trace=abi.dptr(o["trace"]))
    for k in null:
        args[k] = None
    rc = hook_fn(solver._L)(solver._h, stream, abi.dptr(pose), ne, ns, args["kind"], args["rec"], args["cp"], huber_a, max_it, pass_,
                            args["pose_out"], abi.dptr(o["cost"]), ip(o["its"]), ip(o["nfe"]), ip(o["nfs"]), args["trace"], trace_rows)
    return rc, o


def run_case(solver, c, stream=None):
    return call_hook(solver, c["stream"] if stream is None else stream, c["pose"], c["n_edge_q"], c["n_surf_q"], c["kind_slot"], c["rec_slot"], c["cp_slot"], c["huber_a"], c["max_it"])


def _ring(n, r, z):
    a = np.arange(n) * (2 * np.pi / n)
    return np.column_stack([r * np.cos(a), r * np.sin(a), np.full(n, z), np.ones(n)]).astype(np.float32)


@pytest.fixture(scope="module")
def contexts(opts):
    """one handle with a batch of three streams (the cases run as stream 2) and the single-stream context, its scan capacities grown by one step"""
    from vil_fusion_amd.estimator import BackendSolver, Scan2MapBatch, Scan2Map
    s = BackendSolver(opts)
    b = Scan2MapBatch(s, 3, cases_mod.CAP_EDGE, cases_mod.CAP_SURF, 64, 64)
    one = Scan2Map(s)
    m = np.vstack([_ring(400, 6.0, z) for z in (0.0, 1.0)])
    one.localMapInited(m, m)
    one.optimation_processing(m[:400], m[:400])
    yield s, b, one
    s.close()


def compare(c, o):
    """the hook's outputs against the exact tier (tolerances from the restatement's own error) -> list of failure strings"""
    r, e = tiers(c["name"])
    bad = []
    tr = o["trace"]
    got = dict(pose=o["pose"], cost=o["cost"][0], its=int(o["its"][0]), nfe=int(o["nfe"][0]), nfs=int(o["nfs"][0]))
    if (got["nfe"], got["nfs"]) != (c["nfe"], c["nfs"]):
        bad.append(f"factor counts {got['nfe']}, {got['nfs']}, true {c['nfe']}, {c['nfs']}")
    if c["n_valid"] == 0:
        if got["its"] != 0 or got["cost"] != 0 or got["pose"].tobytes() != c["pose"].tobytes() or not np.isnan(tr).all():
            bad.append(f"no factor: its {got['its']} cost {got['cost']} pose {got['pose']}")
        return bad
    # row 0
    x0 = tr[0, 0:7]
    if x0.tobytes() != c["pose"].tobytes():
        bad.append("row 0: x is not the start pose")
    sums = list(tr[0, 14:35]) + list(tr[0, 8:14]) + [tr[0, 7]]
    B = e["rows"][0]["bound"]
    for k, (a, b_) in enumerate(zip(sums, _sums(e["rows"][0]))):
        d = _err(a, b_)
        print(f"{c['name']} row 0 sum {k}: error {d:.3e} bound {B[k]:.3e}")
        if not d <= B[k]:
            bad.append(f"row 0 sum {k}: error {d:.3e} > bound {B[k]:.3e}")
    for k in range(6):
        want = 1.0 / (1.0 + np.sqrt(tr[0, 14 + k * (k + 1) // 2 + k]))
        if abs(tr[0, 35 + k] - want) > 4 * R.U:
            bad.append(f"row 0 scale {k}: {tr[0, 35 + k]!r}, from the row's own H {want!r}")
    if (int(tr[0, 41]), int(tr[0, 42])) != (e["why"], e["its"] + 1):
        bad.append(f"loop ended by {tr[0, 41]} after {tr[0, 42] - 1} rows, exact tier {e['why']} after {e['its']}")
    if got["its"] != e["its"]:
        bad.append(f"its {got['its']}, exact tier {e['its']}")
        return bad
    # later rows
    for k, (rr, ee) in enumerate(zip(r["rows"][1:], e["rows"][1:]), start=1):
        row = tr[k]
        fl = (int(row[0]), int(row[1]), int(row[2]), int(row[3]))
        if fl != (ee["valid"], ee["accept"], ee["stop"], ee["reason"]):
            bad.append(f"row {k}: valid accept stop reason {fl}, exact tier {(ee['valid'], ee['accept'], ee['stop'], ee['reason'])}")
            break
        for a in range(6):
            if ee["clamped"][a]:
                if row[4 + a] != 1e-6:
                    bad.append(f"row {k}: diagonal {a} is {row[4 + a]!r}, the clamp 1e-6")
            elif _err(row[4 + a], ee["diag"][a]) > R.tolerance_scalar(rr["diag"][a], ee["diag"][a]):
                bad.append(f"row {k}: diagonal {a} error {_err(row[4 + a], ee['diag'][a]):.3e}")
        checks = [("step", row[10:16], rr["step"], ee["step"]), ("candidate", row[16:23], rr["cand"], ee["cand"])]
        for what, g_, r_, e_ in checks:
            d = np.sqrt(sum(_err(a, b_) ** 2 for a, b_ in zip(g_, e_)))
            tol = R.tolerance_x(r_, e_)
            print(f"{c['name']} row {k} {what}: error {d:.3e} tolerance {tol:.3e}")
            if not d <= tol:
                bad.append(f"row {k}: {what} error {d:.3e} > {tol:.3e}")
        if ee["small"] and any(row[10 + a] != 0.0 for a in range(3)):
            bad.append(f"row {k}: the rotational step must be exactly 0")
        for what, g_, r_, e_ in (("candidate cost", row[23], rr["cand_cost"], ee["cand_cost"]), ("model cost change", row[24], rr["mcc"], ee["mcc"]),
                                 ("radius", row[25], rr["radius"], ee["radius"]), ("decrease factor", row[26], rr["dfac"], ee["dfac"])):
            # (A cost and the model cost change carry the error of the candidate / the step they are evaluated at, which the restatement's own luck need not
            # show. Their measured tolerance is floored at the quantity's own rounding bound plus what the tolerance this very row allows on the candidate
            # (|g| tol_x + |H| tol_x^2) or on the step ((|gs| + |Hs y|) tol_y) makes of it: f_cc / f_mcc of the exact tier, not its forward bounds.)
            floor = dict(zip(("candidate cost", "model cost change"), (ee["f_cc"], ee["f_mcc"]))).get(what, 0.0)
            d, tol = _err(g_, e_), max(R.tolerance_scalar(r_, e_), floor)
            if floor:
                print(f"{c['name']} row {k} {what}: floor / (64 u max(1, |v|)) = {floor / (R.SAFETY * R.U * max(1.0, abs(float(e_)))):.3e}")
            print(f"{c['name']} row {k} {what}: error {d:.3e} tolerance {tol:.3e}")
            if not d <= tol:
                bad.append(f"row {k}: {what} error {d:.3e} > {tol:.3e}")
    if not np.isnan(tr[e["its"] + 1:]).all():
        bad.append("rows behind the last iteration were written")
    d = np.sqrt(sum(_err(a, b_) ** 2 for a, b_ in zip(got["pose"], e["pose"])))
    tol = R.tolerance_x(r["pose"], e["pose"])
    print(f"{c['name']} final pose: error {d:.3e} tolerance {tol:.3e}")
    if not d <= tol:
        bad.append(f"final pose error {d:.3e} > {tol:.3e}")
    d, tol = _err(got["cost"], e["cost"]), max(R.tolerance_scalar(r["cost"], e["cost"]), e["d_cost"])
    print(f"{c['name']} final cost: error {d:.3e} tolerance {tol:.3e}")
    if not d <= tol:
        bad.append(f"final cost error {d:.3e} > {tol:.3e}")
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_hook_matches_exact_tier(contexts, name):
    """row 0 within the derived bound, every later row's flags, stop reason and its equal to the exact tier's, iterates, costs, radius, the final pose and cost within
    the measured tolerance, the true factor counts (l_33000_planes and l_70000_edges are the sizes at which the packed 16-bit counters overflowed)"""
    s, b, one = contexts
    c = CASE_BY_NAME[name]
    rc, o = run_case(s, c)
    assert rc == 0, rc
    bad = compare(c, o)
    assert not bad, f"{name}: {len(bad)} differences:\n" + "\n".join(bad[:25])


@pytest.mark.gpu
def test_hook_streams_agree(contexts):
    """a stream's offsets (24 sid, sid capq) do not enter the result: stream 0, stream 2 and the single-stream context give the same bytes"""
    s, b, one = contexts
    c = CASE_BY_NAME["single_stream"]
    outs = [run_case(s, c, stream=k) for k in (0, 1, 2, -1)]
    assert all(rc == 0 for rc, _ in outs)
    for _, o in outs[1:]:
        assert all(o[k].tobytes() == outs[0][1][k].tobytes() for k in o)


@pytest.mark.gpu
def test_hook_refusals_leave_the_outputs_untouched(opts, contexts):
    from vil_fusion_amd.estimator import BackendSolver, Scan2MapBatch
    c = CASE_BY_NAME["c_1_300"]

    def refused(s, stream, ne=1, ns=300, max_it=4, pass_=0, trace_rows=8, null=()):
        rc, o = call_hook(s, stream, c["pose"], ne, ns, c["kind_slot"], c["rec_slot"], c["cp_slot"], 0.1, max_it, pass_, trace_rows, null)
        f = fresh_outputs(trace_rows)
        return rc == INVALID and all(o[k].tobytes() == f[k].tobytes() for k in o)
    s2 = BackendSolver(opts)
    assert refused(s2, -1) and refused(s2, 0)                   # neither context exists
    Scan2MapBatch(s2, 2, 8, 320, 64, 64)
    assert refused(s2, -1)                                       # the single-stream context still does not exist
    assert refused(s2, 2) and refused(s2, -2)                    # stream out of range
    assert refused(s2, 0, 9, 1) and refused(s2, 0, 1, 321)       # above the scan capacities
    assert refused(s2, 0, -1, 300) and refused(s2, 0, 1, -1)     # negative counts
    assert refused(s2, 0, pass_=2) and refused(s2, 0, pass_=-1)
    assert refused(s2, 0, max_it=8) and refused(s2, 0, max_it=-1)      # eight rows hold row 0 and seven iterations
    for k in ("kind", "rec", "cp"):
        assert refused(s2, 0, null=(k,))
    assert refused(s2, 0, 0, 0, null=("pose_out",)) and refused(s2, 0, 0, 0, null=("trace",))
    rc, o = call_hook(s2, 1, c["pose"], 0, 0, c["kind_slot"], c["rec_slot"], c["cp_slot"], 0.1, 4, null=("kind", "rec", "cp"))
    assert rc == 0 and o["its"][0] == 0                          # no query: the input pointers may be null
    rc, o = call_hook(s2, 1, c["pose"], 1, 300, c["kind_slot"], c["rec_slot"], c["cp_slot"], 0.1, 7, trace_rows=8)
    assert rc == 0 and o["nfe"][0] + o["nfs"][0] == c["n_valid"]
    s2.close()


def _one_per_leaf(pts, leaf):
    key = np.floor(pts[:, :3] * (np.float32(1.0) / np.float32(leaf))).astype(np.int64)
    _, first = np.unique(key, axis=0, return_index=True)
    return np.ascontiguousarray(pts[np.sort(first)])


def _voxel_order(pts, leaf):
    """a cloud with one point per leaf in the order PCL's voxel grid emits its leaves (the oracle's restatement; every centroid is its single point)"""
    import oracle_lib
    L = oracle_lib.lib()
    L.vilo_voxel_grid.argtypes = [fpp, C.c_int, C.c_float, fpp, C.c_int, ipp]
    out = np.zeros_like(pts); n = C.c_int(0)
    assert L.vilo_voxel_grid(pts.ctypes.data_as(fpp), len(pts), leaf, out.ctypes.data_as(fpp), len(pts), C.byref(n)) == 0 and n.value == len(pts)
    assert sorted(map(tuple, out)) == sorted(map(tuple, pts))
    return out


@pytest.mark.gpu
def test_step_is_reproduced_by_the_two_hooks(opts):
    """vilf_scan2map_step against vilf_debug_s2m_associate followed by vilf_debug_s2m_solve, pass by pass: factor counts, iteration counts, costs and the pose BIT
    FOR BIT — b_solve and its test twin b_solve_dbg compute the same bits. That needs the queries in the order the step's voxel filter emits its leaves (PCL's; one
    point per leaf, so every centroid is its point): handed over in another order the 28 sums add the same terms differently and the pose agrees within the
    summation bound only (measured 1.2e-16 against a tolerance of 9.4e-14). The tolerance comparison stays as the weaker statement the bitwise one implies."""
    from vil_fusion_amd.estimator import BackendSolver, Scan2Map
    import test_scan2map_association as TA
    s = BackendSolver(opts); dev = Scan2Map(s)
    me, ms = _scene(1)
    dev.localMapInited(me, ms)
    d = np.array([0.06, -0.04, 0.02, 0.0], dtype=np.float32)
    qe, qs = _one_per_leaf(me[::3] + d, opts.edge_leaf_size), _one_per_leaf(ms[::2] + d, opts.surf_leaf_size)
    qe, qs = _voxel_order(qe, opts.edge_leaf_size), _voxel_order(qs, opts.surf_leaf_size)
    pose = cases_mod.IDENT.copy()
    passes = []
    for p in range(2):
        rc, a = TA.call_hook(s, -1, pose, qe, qs)
        assert rc == 0
        nq = len(qe) + len(qs)
        cp = np.vstack([qe[:, :3], qs[:, :3]])
        passes.append(dict(pose=pose.copy(), kind=a["kind"][:nq].copy(), rec=a["rec"][:nq].copy(), cp=cp))
        rc2, o = call_hook(s, -1, pose, len(qe), len(qs), passes[-1]["kind"], passes[-1]["rec"], cp, opts.huber_a, opts.s2m_max_iterations, p)
        assert rc2 == 0
        passes[-1]["out"] = o
        pose = o["pose"].copy()
    r = dev.optimation_processing(qe, qs)
    assert (r.n_edge_ds, r.n_surf_ds) == (len(qe), len(qs))
    bitwise = True
    for p, ps in enumerate(passes):
        o = ps["out"]
        assert (r.n_edge_factors[p], r.n_surf_factors[p]) == (int(o["nfe"][0]), int(o["nfs"][0])) == (int((ps["kind"] == 1).sum()), int((ps["kind"] == 2).sum()))
        assert r.n_edge_factors[p] > 10 and r.n_surf_factors[p] > 50
        assert r.iterations[p] == int(o["its"][0])
        bitwise &= r.final_cost[p] == o["cost"][0]
    valid = (passes[1]["kind"] == 1) | (passes[1]["kind"] == 2)
    c = dict(name="step", pose=passes[1]["pose"], huber_a=opts.huber_a, max_it=opts.s2m_max_iterations, n_valid=int(valid.sum()), nfe=0, nfs=0,
             f64=dict(kind=passes[1]["kind"][valid], rec=passes[1]["rec"][valid], cp=passes[1]["cp"][valid].astype(np.float64), mult=np.ones(int(valid.sum()), dtype=int)),
             mp_src=dict(kind=passes[1]["kind"][valid], rec=passes[1]["rec"][valid], cp=passes[1]["cp"][valid].astype(np.float64), mult=np.ones(int(valid.sum()), dtype=int)))
    _prepare(c)
    rr = R.restate(c); ee = R.exact(c, rr)
    tol = R.tolerance_x(rr["pose"], ee["pose"])
    got = np.array(list(r.pose_qt))
    dd = float(np.linalg.norm(got - passes[1]["out"]["pose"]))
    bitwise &= got.tobytes() == passes[1]["out"]["pose"].tobytes()
    print(f"step against the two hooks: pose difference {dd:.3e}, tolerance {tol:.3e}, bit for bit: {bitwise}")
    assert dd <= tol
    assert bitwise
    assert abs(r.final_cost[1] - passes[1]["out"]["cost"][0]) <= R.tolerance_scalar(rr["cost"], ee["cost"])
    s.close()


@pytest.mark.gpu
def test_hook_leaves_no_trace(opts):
    """two batches, one with the hook before every step (and after the snapshot), across a snapshot and a rewind: equal results and map bytes"""
    from vil_fusion_amd.estimator import BackendSolver, Scan2MapBatch
    me, ms = _scene(2)
    rng = np.random.default_rng(5)
    scans = [(np.ascontiguousarray(me[rng.choice(len(me), 150, replace=False)] + np.append(rng.normal(0, 0.02, 3), 0).astype(np.float32)),
              np.ascontiguousarray(ms[rng.choice(len(ms), 400, replace=False)] + np.append(rng.normal(0, 0.02, 3), 0).astype(np.float32))) for _ in range(4)]
    cA, cB = CASE_BY_NAME["c_255_257"], CASE_BY_NAME["g_reject_then_accept"]
    outs = []
    for with_hook in (False, True):
        s = BackendSolver(opts); b = Scan2MapBatch(s, 2, 512, 512, 16384, 16384)
        b.localMapInited(0, me, ms); b.localMapInited(1, me[::2], ms[::2])
        rec = []
        for k, (e_, s_) in enumerate(scans):
            if with_hook:
                for stream, cc in ((0, cA), (1, cB)):
                    rc, _ = run_case(s, cc, stream=stream)
                    assert rc == 0
            if k == 2:
                b.snapshot()
            b.set_scan(0, e_, s_); b.set_scan(1, e_[:60], s_[:200])
            b.step()
            rec.append(b"".join(bytes(r) for r in b.results()))
        if with_hook:
            assert run_case(s, cA, stream=1)[0] == 0
        b.rewind()
        b.step()
        rec.append(b"".join(bytes(r) for r in b.results()))
        rec += [b.getMapCloud(i, w).tobytes() for i in (0, 1) for w in (0, 1)]
        outs.append(rec)
        s.close()
    assert outs[0] == outs[1]
