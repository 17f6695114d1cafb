"""The 11-frame window solve at the edges of its FACTOR layout: the class plan deals the 55 frame pairs to the four wave classes of k_linearize, sizes the window in
chunks of 56 slots per class, and a pair that runs over a chunk edge hands its accumulators on (in a split launch from workgroup to workgroup). The windows of
window_cases.py put pairs on those edges; every case asserts its edge through a Python mirror of the plan.

CPU: the mirror against the library's own plan (vilf_debug_class_plan: no device), every case's edge, the admission rule (the oracle keeps its counts under 1e-13
perturbations of its inputs), the oracle's counts and cost descent. GPU: every case at 1 and 8 iterations against the oracle, counts exactly and every state within
min(_compare's default, max(MARGIN x the oracle's own envelope of that case, 64 ulp)); the device against itself to the bit over its launch routes; slots uploaded
again; the dense solve kernel; a window without features through the Python binding."""
import ctypes as C
import inspect
import numpy as np
import pytest
import window_cases as wc
from window_cases import CASES, IDS

ITERS = (1, 8)
# _compare's defaults (test_gpu_parity.py), per quantity; the costs relative
DEFAULT = dict(Ps=1e-7, Rs=1e-8, Vs=1e-6, Bas=1e-6, Bgs=1e-7, depth=1e-5, final_cost=1e-7, initial_cost=1e-9)
MARGIN = 10.0        # x the envelope: a 1e-13 perturbation is ~1e3 ulp of the inputs, the device differs in the order of its sums only; four draws may underestimate a little
# Where the device leaves MARGIN x the envelope although its counts are the oracle's: the largest ratio of device-to-oracle deviation to envelope over the quantities,
# as measured in one run, (k_solve_sb, k_solve) per (case, iteration limit); k_solve only where test_dense_kernel runs the case. Both kernels leave it alike, with and
# without visual factors ("empty"), so it is no matter of the factor layout: the envelope perturbs para_pose and obs_point only, and the oracle's own answer moves 15
# to 40 times further after 8 iterations (20 to 85 times in the gyroscope bias after one, in the windows listed for one iteration) when its IMU records or speed-bias
# inputs are perturbed by the same 1e-13. The margin of such a case is twice its measured ratio; the bound never leaves _compare's defaults.
MEASURED = {
    ("ladder-17-c40", 1): (45.8, None),
    ("ladder-56-c0", 1): (27.5, None),
    ("ladder-56-c40", 1): (47.3, None),
    ("ladder-56-c100", 1): (35.7, None),
    ("ladder9-57-c0", 1): (26.3, None),
    ("start-56-c0", 1): (11.0, None),
    ("carry-c0", 1): (67.9, 58.5),
    ("carry-c40", 1): (9.3, 39.6),
    ("carry-c40-noprior", 1): (23.0, None),
    ("split-13-c0", 1): (5.2, 30.6),
    ("split-13-c40", 1): (13.8, 41.4),
    ("split-13-c40-noprior", 1): (89.1, None),
    ("empty-c0", 8): (40.9, 12.3),
    ("empty-c40", 8): (40.9, 12.3),
    ("single-c0", 8): (25.0, 69.3),
    ("single-c40", 8): (25.0, 69.3),
    ("single-c100", 8): (19.9, None),
    ("ladder-1-c0", 8): (14.1, None),
    ("ladder-1-c40", 8): (14.1, None),
    ("ladder9-1-c0", 8): (126.3, None),
    ("ladder9-1-c40", 8): (126.3, None),
    ("ladder-2-c40", 8): (10.3, None),
    ("ladder-3-c0", 8): (26.5, None),
    ("ladder-3-c40", 8): (19.3, None),
    ("ladder-4-c0", 8): (28.0, None),
    ("ladder-4-c40", 8): (34.8, None),
    ("ladder-5-c40", 8): (66.3, None),
    ("ladder-15-c0", 8): (27.6, None),
    ("ladder-16-c0", 8): (17.5, None),
    ("ladder-16-c40", 8): (21.6, None),
    ("ladder-17-c40", 8): (46.4, None),
    ("ladder-55-c0", 8): (28.2, None),
    ("ladder-55-c40", 8): (91.4, None),
    ("each-pair-once-c0", 8): (10.1, None),
    ("each-pair-once-c40", 8): (10.1, None),
    ("ladder-56-c100", 8): (10.3, None),
    ("ladder9-56-c40", 8): (12.3, None),
    ("ladder-57-c0", 8): (25.6, 17.0),
    ("ladder-57-c40", 8): (28.8, 16.5),
    ("ladder9-57-c0", 8): (33.9, None),
    ("ladder9-57-c40", 8): (11.3, None),
    ("late-c0", 8): (28.2, None),
    ("late-c40", 8): (67.6, None),
    ("ladder-111-c0", 8): (37.3, None),
    ("ladder-111-c40", 8): (16.3, None),
    ("ladder-112-c0", 8): (13.4, None),
    ("ladder-112-c40", 8): (23.6, None),
    ("ladder-113-c0", 8): (67.5, None),
    ("ladder-113-c40", 8): (13.6, None),
    ("start-55-c0", 8): (14.4, None),
    ("start-55-c40", 8): (26.7, None),
    ("start-56-c0", 8): (18.2, None),
    ("carry-c0", 8): (68.4, 124.8),
    ("carry-c40", 8): (44.8, 36.9),
    ("carry-c100", 8): (44.5, None),
    ("lopsided-c0", 8): (52.1, None),
    ("lopsided-c40", 8): (58.8, None),
    ("max-two-frame-c0", 8): (16.5, None),
    ("split-12-c0", 8): (24.2, None),
    ("split-12-c40", 8): (20.5, None),
    ("split-12-c100", 8): (18.5, None),
    ("split-13-c0", 8): (18.0, 56.9),
    ("split-13-c40", 8): (7.9, 50.3),
    ("max-full-c0", 8): (76.3, 152.9),
    ("max-full-c40", 8): (63.3, 96.4),
}
DENSE = ("empty", "single", "ladder-57", "carry", "split-13", "max-full")
STALE = ("empty", "single", "ladder-1", "late", "start-56")


def _with_iterations(opts, n):
    o = type(opts).from_buffer_copy(opts)
    o.max_num_iterations = n
    return o


# ---- the plan (CPU) ---------------------------------------------------------------------------------------------------------------------------------------
def _lib_plan(tracks):
    from vil_fusion_amd import lib as vlib
    L = vlib.lib()
    ip = C.POINTER(C.c_int)
    L.vilf_debug_class_plan.argtypes = [C.c_int, ip, ip, ip, ip, ip]
    F = len(tracks)
    start = np.array([t[0] for t in tracks] + [0], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum([t[1] for t in tracks])]).astype(np.int32)
    cls, cstart, ccount = (np.full(wc.NPAIR, -7, dtype=np.int32) for _ in range(3))
    nslot = L.vilf_debug_class_plan(F, start.ctypes.data_as(ip), offs.ctypes.data_as(ip), cls.ctypes.data_as(ip), cstart.ctypes.data_as(ip), ccount.ctypes.data_as(ip))
    assert nslot > 0, nslot
    return dict(cls=cls.tolist(), start=cstart.tolist(), count=ccount.tolist(), nslot=nslot)


def _assert_mirror(tracks):
    mine, theirs = wc.class_plan(tracks), _lib_plan(tracks)
    assert theirs["nslot"] == 4 * wc.CLS * mine["chunks"]
    for k in ("count", "cls", "start"):
        assert mine[k] == theirs[k], k


def _random_tracks(rng, F):
    start = rng.integers(0, 10, F)
    return [(int(s), int(rng.integers(2, wc.NF - s + 1))) for s in start]


def _tie_tables():
    rng = np.random.default_rng(11)
    out = [[(s, wc.NF - s) for s in range(10)] * k for k in (1, 2, 56, 57)]                       # all 55 pairs equal
    out += [[(s, 2) for s in range(10)] * k for k in (1, 7, 28, 100)]                             # ten equal pairs, 45 empty ones
    out += [[(s, 2) for s in range(10)] * 5 + [(s, 3) for s in range(9)] * 5, [(0, 11)] * 3 + [(1, 10)] * 3 + [(5, 6)] * 6]
    for _ in range(20):                                                                           # a few distinct counts, many pairs each
        levels = rng.integers(1, 4, 10)
        out.append([(s, wc.NF - s) for s in range(10) for _ in range(int(levels[s]))])
    return out


@pytest.mark.parametrize("k", range(len(wc.SHAPES)), ids=[s[0] for s in wc.SHAPES])
def test_case_has_its_edge_and_the_mirror_is_the_plan(k):
    name, tracks, check = wc.SHAPES[k]
    plan = wc.class_plan(tracks)
    print(name, "factors", sum(plan["count"]), "class lists", plan["lists"], "chunks", plan["chunks"])
    check(tracks, plan)
    _assert_mirror(tracks)


def test_mirror_is_the_plan_on_random_and_tied_tables():
    rng = np.random.default_rng(2024)
    tables = [_random_tracks(rng, int(rng.integers(0, wc.MAX_FEATURES + 1))) for _ in range(200)] + _tie_tables()
    tables += [[], _random_tracks(rng, wc.MAX_FEATURES)]
    for t in tables:
        _assert_mirror(t)
    assert sum(len(set(c for c in wc.pair_counts(t) if c)) < len([c for c in wc.pair_counts(t) if c]) for t in tables) > 100, "equal pair counts (the tie rule) are common"


def test_hook_rejects_what_check_window_rejects():
    from vil_fusion_amd import lib as vlib
    L = vlib.lib()
    ip = C.POINTER(C.c_int)
    L.vilf_debug_class_plan.argtypes = [C.c_int, ip, ip, ip, ip, ip]
    out = [np.zeros(wc.NPAIR, dtype=np.int32) for _ in range(3)]
    for s, n in ((9, 3), (-1, 2), (0, 1), (0, 12)):
        st, of = np.array([s], dtype=np.int32), np.array([0, n], dtype=np.int32)
        assert L.vilf_debug_class_plan(1, st.ctypes.data_as(ip), of.ctypes.data_as(ip), *[o.ctypes.data_as(ip) for o in out]) < 0, (s, n)


# ---- the windows and the oracle (CPU) ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(oracle, opts):
    """every case once: the window, and per iteration limit the oracle's solve and its envelope"""
    made = [c.make(opts) for c in CASES]
    o = {it: _with_iterations(opts, it) for it in ITERS}
    refs = {it: [oracle.window_solve(o[it], w, p) for w, p in made] for it in ITERS}
    envs = {it: [wc.envelope(o[it], w, p, ref=r) for (w, p), r in zip(made, refs[it])] for it in ITERS}
    return dict(wins=[m[0] for m in made], priors=[m[1] for m in made], opts=o, refs=refs, envs=envs)


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_oracle_accepts_and_descends(world, k):
    """the tables are what the case says, the oracle's counts are plausible and its cost falls; the admission rule: four perturbed solves keep the counts, and (this
    file's addition, see window_cases.SEEDS) 100 times the envelope stays inside _compare's defaults, so that the cap of the bound never cuts into the oracle's own noise"""
    case, win = CASES[k], world["wins"][k]
    assert [(int(s), int(b - a)) for s, a, b in zip(win.feature_start_frame, win.feature_obs_offset[:-1], win.feature_obs_offset[1:])] == list(case.tracks)
    assert win.n_features == len(case.tracks) and win.n_factors == case.n_factors
    nconst = int(np.count_nonzero(win.feature_const))
    assert nconst == (win.n_features if case.const >= 1.0 else 0 if case.const == 0.0 else nconst)
    if case.const == 0.4 and win.n_features >= 20: assert 0 < nconst < win.n_features
    for it in ITERS:
        s, (env, kept) = world["refs"][it][k].summary, world["envs"][it][k]
        print(f"{case.id} it {it}: counts {wc.counts(world['refs'][it][k])} cost {s['initial_cost']:.6e} -> {s['final_cost']:.6e}; envelope " + " ".join(f"{q} {v:.1e}" for q, v in env.items()))
        assert 1 <= s["num_iterations"] <= it and 0 <= s["num_successful_steps"] <= s["num_iterations"] and 1 <= s["num_linear_solves"] <= s["num_iterations"]
        assert s["final_cost"] <= s["initial_cost"] and (s["final_cost"] < s["initial_cost"]) == (s["num_successful_steps"] > 0)
        if not case.noisy:
            assert kept, "admission rule: a perturbed oracle solve changed its counts; change the case's seed (window_cases.SEEDS)"
            assert s["num_iterations"] == it
            wide = {q: v for q, v in env.items() if wc.ADMIT_SHAPE.get(case.shape, wc.ADMIT) * v > DEFAULT[q]}
            assert not wide, ("admission rule: the oracle's own envelope leaves _compare's default, the window is too ill-conditioned to compare; change the seed", wide)
    assert world["refs"][1][k].summary["initial_cost"] == world["refs"][8][k].summary["initial_cost"]


def test_rejecting_windows_reject(world):
    """the strongly perturbed leg was picked with the oracle for its rejected steps"""
    ks = [k for k, c in enumerate(CASES) if c.noisy]
    assert sorted(CASES[k].shape for k in ks) == sorted(wc.REJECTING)
    for k in ks:
        s = world["refs"][8][k].summary
        print(CASES[k].id, wc.counts(world["refs"][8][k]))
        assert s["num_successful_steps"] < s["num_iterations"], CASES[k].id


# ---- the device (GPU) -------------------------------------------------------------------------------------------------------------------------------------
BITS = ("Ps", "Rs", "Vs", "Bas", "Bgs", "para_feature")


def _bits(res, sm):
    return [np.concatenate([np.ravel(getattr(r, k)) for k in BITS] +
                           [np.array([s.num_iterations, s.num_successful_steps, s.num_linear_solves, s.termination, s.initial_cost, s.final_cost], dtype=np.float64)])
            for r, s in zip(res, sm)]


def _solve(s, wins, priors):
    s.batch_upload(wins, priors); s.batch_solve()
    res, sm = s.batch_download(), s.batch_summaries()
    for r, m in zip(res, sm):
        r.summary = dict(num_iterations=m.num_iterations, num_successful_steps=m.num_successful_steps, num_linear_solves=m.num_linear_solves,
                         initial_cost=m.initial_cost, final_cost=m.final_cost, termination=m.termination)
    return res, sm


def _groups_of_8():
    """the cases in batches of at most 8 (the largest split batch), small to large; split-12 and split-13 share one"""
    split = [k for k, c in enumerate(CASES) if c.shape in ("split-12", "split-13")]
    rest = [k for k in range(len(CASES)) if k not in split]
    assert 2 <= len(split) <= 8 and {CASES[k].shape for k in split} == {"split-12", "split-13"}
    return [rest[i:i + 8] for i in range(0, len(rest), 8)] + [split]


@pytest.fixture(scope="module")
def device(world):
    """per iteration limit a handle and its solve of ALL cases as one upload (route c: one workgroup per window; the per-window strides are max-full's), and the same
    in batches of 8 (route d)"""
    from vil_fusion_amd.estimator import BackendSolver
    wins, priors = world["wins"], world["priors"]
    out = {}
    for it in ITERS:
        s = BackendSolver(world["opts"][it])
        res, sm = _solve(s, wins, priors)
        eights = [None] * len(CASES)
        for ks in _groups_of_8():
            for k, b in zip(ks, _bits(*_solve(s, [wins[k] for k in ks], [priors[k] for k in ks]))):
                eights[k] = b
        out[it] = dict(solver=s, res=res, sm=sm, bits=_bits(res, sm), eights=eights)
    yield out
    for it in ITERS:
        out[it]["solver"].close()


def _bounds(ref, env, fconst, margin=MARGIN):
    """per quantity min(_compare's default, max(margin x envelope, 64 ulp of the largest magnitude compared)); the costs are relative: 64 ulp of 1"""
    var = np.asarray(fconst) == 0
    top = {k: float(np.abs(getattr(ref, k)).max()) for k in ("Ps", "Rs", "Vs", "Bas", "Bgs")}
    top["depth"] = float(np.abs(1.0 / ref.para_feature[var]).max()) if var.any() else 1.0
    top["final_cost"] = top["initial_cost"] = 1.0
    return {q: min(DEFAULT[q], max(margin * env[q], 64.0 * float(np.spacing(top[q])))) for q in wc.QUANTITIES}


def _margin(case, it, dense):
    r = MEASURED.get((case.id, it), (0.0, 0.0))[1 if dense else 0]
    assert r is not None, "no measurement of k_solve for this case"
    return max(MARGIN, 2.0 * r)


def _against_oracle(tag, case, got, ref, env, win, margin):
    from test_gpu_parity import _compare
    for name, p in inspect.signature(_compare).parameters.items():                     # DEFAULT restates _compare's
        if p.default is not inspect.Parameter.empty:
            assert p.default == {"tol_p": DEFAULT["Ps"], "tol_r": DEFAULT["Rs"], "tol_cost": DEFAULT["final_cost"]}[name]
    dev = wc.deviation(got, ref, win.feature_const)
    bound = DEFAULT if case.noisy else _bounds(ref, env, win.feature_const, margin)
    print(f"{tag} {case.id}: counts {wc.counts(got)} / oracle {wc.counts(ref)}, margin {margin:.1f}")
    for q in wc.QUANTITIES:
        print(f"    {q:13s} device-oracle {dev[q]:.2e}  envelope {env[q]:.2e}  bound {bound[q]:.2e}" + ("" if dev[q] <= bound[q] else "   <-- OUTSIDE") +
              (f"  ({dev[q] / env[q]:.1f} x envelope)" if env[q] > 0 else ""))
    assert wc.counts(got) == wc.counts(ref), (tag, case.id)
    bad = [q for q in wc.QUANTITIES if not dev[q] <= bound[q]]
    assert not bad, (tag, case.id, {q: (dev[q], bound[q]) for q in bad})
    if case.noisy: _compare(got, ref)
    c = win.feature_const != 0
    assert np.array_equal(got.para_feature[c], win.para_feature[c]), "a constant depth comes back as it went in"


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_device_matches_oracle(world, device, k):
    for it in ITERS:
        _against_oracle(f"it {it}", CASES[k], device[it]["res"][k], world["refs"][it][k], world["envs"][it][k][0], world["wins"][k], _margin(CASES[k], it, False))


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_launch_routes_give_the_same_bits(world, device, k, monkeypatch):
    """(a) alone through k_linearize_split (up to 12 chunks; beyond, one workgroup), (b) alone with one workgroup, (c) its slot of the all-cases upload, (d) its batch of 8"""
    win, prior = [world["wins"][k]], [world["priors"][k]]
    chunks = wc.class_plan(CASES[k].tracks)["chunks"]
    for it in ITERS:
        d = device[it]
        monkeypatch.delenv("VILF_NO_LIN_SPLIT", raising=False)
        a = _bits(*_solve(d["solver"], win, prior))[0]
        monkeypatch.setenv("VILF_NO_LIN_SPLIT", "1")
        b = _bits(*_solve(d["solver"], win, prior))[0]
        monkeypatch.delenv("VILF_NO_LIN_SPLIT")
        diff = {r: int(np.count_nonzero(x != d["bits"][k])) for r, x in (("a", a), ("b", b), ("d", d["eights"][k]))}
        print(f"it {it} {CASES[k].id}: {chunks} chunks, values differing from route (c): {diff}")
        assert np.array_equal(a, d["bits"][k]), (CASES[k].id, it, "alone, split" if chunks <= wc.MAXCH else "alone, too long to split")
        assert np.array_equal(b, d["bits"][k]), (CASES[k].id, it, "alone, one workgroup")
        assert np.array_equal(d["eights"][k], d["bits"][k]), (CASES[k].id, it, "batch of 8")


@pytest.mark.gpu
def test_slots_uploaded_again_with_smaller_windows(world, device, monkeypatch):
    """A handle that has solved the all-cases batch is given small windows in the same slots: a slot's unused factor slots must hold null records and nothing may be
    read beyond a window's own chunks, so the bits equal a fresh handle's and the all-cases batch's. Both launch kinds; and once beside max-full, which keeps the
    per-window strides of the first batch."""
    from vil_fusion_amd.estimator import BackendSolver
    small = [k for k, c in enumerate(CASES) if c.shape in STALE and c.const == 0.4 and c.with_prior]
    big = [k for k, c in enumerate(CASES) if c.id == "max-full-c0"]
    assert len(small) == len(STALE) and len(big) == 1
    wins, priors = world["wins"], world["priors"]
    for it in ITERS:
        used, fresh = BackendSolver(world["opts"][it]), BackendSolver(world["opts"][it])
        try:
            for ks, one_wg in ((small, False), (small, True), (small + big, False)):
                monkeypatch.delenv("VILF_NO_LIN_SPLIT", raising=False)
                _solve(used, wins, priors)
                if one_wg: monkeypatch.setenv("VILF_NO_LIN_SPLIT", "1")
                a = _bits(*_solve(used, [wins[k] for k in ks], [priors[k] for k in ks]))
                b = _bits(*_solve(fresh, [wins[k] for k in ks], [priors[k] for k in ks]))
                monkeypatch.delenv("VILF_NO_LIN_SPLIT", raising=False)
                for i, k in enumerate(ks):
                    assert np.array_equal(a[i], b[i]), (CASES[k].id, it, one_wg, len(ks), "used handle / fresh handle")
                    assert np.array_equal(a[i], device[it]["bits"][k]), (CASES[k].id, it, one_wg, len(ks), "again / all-cases batch")
        finally:
            used.close(); fresh.close()


@pytest.mark.gpu
def test_dense_kernel(world, device, monkeypatch):
    """k_solve (VILF_SOLVE_DENSE=1), the Cholesky of the whole system behind the same linearisation: k_solve_sb's counts, its states to the figures of
    test_speed_bias_first_kernel_equals_dense_kernel_and_oracle, and the oracle within this file's bound"""
    ks = [k for k, c in enumerate(CASES) if c.shape in DENSE and c.const in (0.0, 0.4) and c.with_prior and not c.noisy]
    assert len(ks) == 2 * len(DENSE)
    for it in ITERS:
        d = device[it]
        monkeypatch.setenv("VILF_SOLVE_DENSE", "1")
        res, _ = _solve(d["solver"], [world["wins"][k] for k in ks], [world["priors"][k] for k in ks])
        monkeypatch.delenv("VILF_SOLVE_DENSE")
        for got, k in zip(res, ks):
            sb = d["res"][k]
            dP, dV = np.abs(got.Ps - sb.Ps).max(), np.abs(got.Vs - sb.Vs).max()
            print(f"it {it} {CASES[k].id}: dense - speed-bias-first |dP| {dP:.2e} |dV| {dV:.2e}")
            assert wc.counts(got) == wc.counts(sb), (CASES[k].id, it)
            assert dP < 1e-8 and dV < 1e-7, (CASES[k].id, it, dP, dV)
            _against_oracle(f"dense it {it}", CASES[k], got, world["refs"][it][k], world["envs"][it][k][0], world["wins"][k], _margin(CASES[k], it, True))


@pytest.mark.gpu
def test_window_without_features_through_the_binding(world, device):
    """F = 0: empty numpy arrays through BackendSolver.optimization (the single-window call) as through batch_upload"""
    k = IDS.index("empty-c0")
    win, prior = world["wins"][k], world["priors"][k]
    assert win.n_features == 0 and win.n_obs == 0 and win.obs_point.shape == (0, 3)
    for it in ITERS:
        s = device[it]["solver"]
        s.set_prior(prior)
        got = s.optimization(win)
        assert got.para_feature.shape == (0,)
        _against_oracle(f"optimization() it {it}", CASES[k], got, world["refs"][it][k], world["envs"][it][k][0], win, _margin(CASES[k], it, False))
