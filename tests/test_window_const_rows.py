"""W, the H_pf rows of the 11-frame window solve, holds one row per feature whose depth is a VARIABLE; a feature with constant depth has no row, and nothing in
k_solve_sb / k_solve loops over one. The row map (f_wrow / row_feat / n_rows) is built by the upload; the kernels read the tables.

CPU: the row map itself (vilf_debug_w_row_map: no device). GPU: windows at the layout's edges — feature counts around the k-step of four rows and the three reduce
waves, constant patterns that empty a wave, a k-step or the whole of W — through the batch path against the CPU oracle at the tolerances of
test_gpu_parity._compare, on both solve kernels and both linearisation launches, and the zero invariant of W when a slot is uploaded again."""
import copy
import ctypes as C
import numpy as np
import pytest
from vil_fusion_amd import synth

N_FEATURES = (1, 3, 4, 5, 12, 13, 37)
PATTERNS = {                                  # feature index array -> 1 where the depth is constant
    "none": lambda f: np.zeros_like(f),
    "all": lambda f: np.ones_like(f),         # n_rows = 0
    "alternating": lambda f: f & 1,
    "only_first_variable": lambda f: (f != 0).astype(f.dtype),
    "only_last_variable": lambda f: (f != f[-1]).astype(f.dtype),
    "wave0_only": lambda f: ((f >> 2) % 3 != 0).astype(f.dtype),       # one reduce wave gets every row, the other two none
}
CASES = [(n, p, wp) for n in N_FEATURES for p in PATTERNS for wp in (True, False)]


def _pattern(name, n):
    return PATTERNS[name](np.arange(n, dtype=np.int64)).astype(np.uint8)


# ---- the row map (CPU) --------------------------------------------------------------------------------------------------------------------------------
def _row_map(fconst):
    from vil_fusion_amd import lib as vlib
    L = vlib.lib()
    L.vilf_debug_w_row_map.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_uint8), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    F = len(fconst)
    cap = max(4, (F + 3) & ~3)
    fc = np.ascontiguousarray(fconst, dtype=np.uint8)
    f_wrow = np.full(max(F, 1), -7, dtype=np.int32); row_feat = np.full(cap, -7, dtype=np.int32)
    n_rows = L.vilf_debug_w_row_map(F, cap, fc.ctypes.data_as(C.POINTER(C.c_uint8)), f_wrow.ctypes.data_as(C.POINTER(C.c_int)), row_feat.ctypes.data_as(C.POINTER(C.c_int)))
    assert n_rows >= 0, n_rows
    return f_wrow[:F], row_feat, n_rows


def _row_map_cases():
    rng = np.random.default_rng(5)
    out = [(f"{p}-{n}", _pattern(p, n)) for n in N_FEATURES + (230, 1000) for p in PATTERNS]
    out += [(f"random-{n}-{q}", (rng.uniform(size=n) < q).astype(np.uint8)) for n in (2, 7, 11, 24, 25, 59, 230, 999) for q in (0.1, 0.4, 0.9)]
    return out


@pytest.mark.parametrize("name,fconst", _row_map_cases(), ids=[c[0] for c in _row_map_cases()])
def test_row_map(name, fconst):
    F = len(fconst)
    f_wrow, row_feat, n_rows = _row_map(fconst)
    var = np.flatnonzero(fconst == 0)
    assert n_rows % 4 == 0 and 0 <= n_rows <= ((F + 3) & ~3)
    assert np.all(f_wrow[fconst != 0] == -1), "a constant feature has no row"
    assert np.all((f_wrow[var] >= 0) & (f_wrow[var] < n_rows))
    assert np.array_equal(row_feat[f_wrow[var]], var), "row_feat[f_wrow[f]] == f"
    assert np.all(row_feat[n_rows:] == -1) and np.count_nonzero(row_feat >= 0) == len(var), "every other row is a padding row"
    # the wave of a row (k-step = row >> 2, k-step s on wave s % 3) is the wave the feature had when rows were features, (f >> 2) % 3
    assert np.array_equal((f_wrow[var] >> 2) % 3, (var >> 2) % 3)
    steps = 0
    for c in range(3):
        rows = np.array([4 * s + q for s in range(c, n_rows // 4, 3) for q in range(4)], dtype=np.int64)       # the rows of wave c, in the order the wave visits them
        feats = row_feat[rows]
        mine = var[(var >> 2) % 3 == c]
        assert np.array_equal(feats[:len(mine)], mine), "ascending, packed four to a k-step"
        assert np.all(feats[len(mine):] == -1), "padding only at the end of a wave's rows"
        if len(mine):
            steps = max(steps, c + 3 * ((len(mine) - 1) // 4) + 1)
    assert n_rows == 4 * steps, "no k-step beyond the last one a wave needs"


# ---- the solve (GPU) ------------------------------------------------------------------------------------------------------------------------------------
def _make(opts, n, pattern, with_prior, seed):
    win, prior, _ = synth.make_window(seed, opts, synth.SynthConfig(n_features=n, with_prior=with_prior))
    win = copy.copy(win)
    win.feature_const = _pattern(pattern, n)
    return win, (prior if with_prior else None)


def _bits(res, sm):
    return [np.concatenate([np.ravel(getattr(r, k)) for k in ("Ps", "Rs", "Vs", "Bas", "Bgs", "para_pose", "para_speed_bias", "para_feature")] +
                           [np.array([s.num_iterations, s.num_successful_steps, s.num_linear_solves, s.termination, s.initial_cost, s.final_cost], dtype=np.float64)])
            for r, s in zip(res, sm)]


def _solve(s, wins, priors):
    s.batch_upload(wins, priors); s.batch_solve()
    res, sm = s.batch_download(), s.batch_summaries()
    for r, m in zip(res, sm):
        r.summary = dict(num_iterations=m.num_iterations, num_successful_steps=m.num_successful_steps, num_linear_solves=m.num_linear_solves,
                         initial_cost=m.initial_cost, final_cost=m.final_cost, termination=m.termination)
    return res, sm


@pytest.fixture(scope="module")
def world(oracle, opts):
    """every case once: the windows, the oracle's solves, and the device's solve of all of them as ONE batch (one workgroup per window)"""
    from vil_fusion_amd.estimator import BackendSolver
    made = [_make(opts, n, p, wp, 4200 + i) for i, (n, p, wp) in enumerate(CASES)]
    wins, priors = [m[0] for m in made], [m[1] for m in made]
    refs = [oracle.window_solve(opts, w, p) for w, p in made]
    s = BackendSolver(opts)
    res, sm = _solve(s, wins, priors)
    yield dict(solver=s, wins=wins, priors=priors, refs=refs, res=res, sm=sm)
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(CASES)), ids=[f"{n}-{p}-{'prior' if wp else 'noprior'}" for n, p, wp in CASES])
def test_window_matches_oracle(world, k):
    from test_gpu_parity import _compare
    got, ref, win = world["res"][k], world["refs"][k], world["wins"][k]
    print(f"iterations {got.summary['num_iterations']} / {ref.summary['num_iterations']}, successful {got.summary['num_successful_steps']} / {ref.summary['num_successful_steps']}, "
          f"|dP| {np.abs(got.Ps - ref.Ps).max():.3e} |dR| {np.abs(got.Rs - ref.Rs).max():.3e} |dV| {np.abs(got.Vs - ref.Vs).max():.3e} "
          f"cost rel {abs(got.summary['final_cost'] - ref.summary['final_cost']) / ref.summary['final_cost']:.3e}")
    _compare(got, ref)
    c = win.feature_const != 0
    assert np.array_equal(got.para_feature[c], win.para_feature[c]), "a constant depth comes back as it went in"


@pytest.mark.gpu
def test_dense_kernel(world, oracle, opts, monkeypatch):
    """the same through k_solve, the Cholesky of the whole system (VILF_SOLVE_DENSE), which shares W and the row map: one window of every pattern, the largest size"""
    from test_gpu_parity import _compare
    pick = [k for k, (n, p, wp) in enumerate(CASES) if n == 37 and wp] + [k for k, (n, p, wp) in enumerate(CASES) if n == 5 and not wp]
    monkeypatch.setenv("VILF_SOLVE_DENSE", "1")
    res, _ = _solve(world["solver"], [world["wins"][k] for k in pick], [world["priors"][k] for k in pick])
    monkeypatch.delenv("VILF_SOLVE_DENSE")
    for got, k in zip(res, pick):
        _compare(got, world["refs"][k])
        c = world["wins"][k].feature_const != 0
        assert np.array_equal(got.para_feature[c], world["wins"][k].para_feature[c])


@pytest.mark.gpu
def test_split_and_plain_launch_give_the_same_bits(world):
    """three windows at a time as a batch of 3 (k_linearize_split) and tiled to 12 (k_linearize): the same bits, copy by copy, and the bits of the one large batch"""
    s = world["solver"]
    ref = _bits(world["res"], world["sm"])
    for k0 in range(0, len(CASES), 3):
        ks = list(range(k0, min(k0 + 3, len(CASES))))
        wins, priors = [world["wins"][k] for k in ks], [world["priors"][k] for k in ks]
        small = _bits(*_solve(s, wins, priors))
        tiled = _bits(*_solve(s, wins * 4, priors * 4))
        for i, k in enumerate(ks):
            assert np.array_equal(small[i], ref[k]), (CASES[k], "split")
            for rep in range(4):
                assert np.array_equal(tiled[i + len(ks) * rep], ref[k]), (CASES[k], "tiled", rep)


@pytest.mark.gpu
def test_slots_uploaded_again_with_other_rows(world, opts):
    """The zero invariant of W: columns outside a feature's frames are never written and must read as zero. A handle that has solved a batch with many rows is given
    one with other constant patterns and fewer rows in the same slots: the solve must equal a fresh handle's bit for bit (both launch kinds)."""
    from vil_fusion_amd.estimator import BackendSolver
    big = [k for k, (n, p, wp) in enumerate(CASES) if n == 37 and p == "none"]
    small = [k for k, (n, p, wp) in enumerate(CASES) if (n, p) in ((37, "alternating"), (13, "only_last_variable"), (37, "wave0_only"), (12, "all"), (5, "none"), (37, "only_first_variable"))]
    assert len(big) == 2 and len(small) == 12
    used, fresh = BackendSolver(opts), BackendSolver(opts)
    try:
        for rep in (6, 2):                                  # 12 slots: one workgroup per window; 4 slots: the split launch
            first = [world["wins"][k] for k in big] * rep, [world["priors"][k] for k in big] * rep
            ks = small[:2 * rep]
            second = [world["wins"][k] for k in ks], [world["priors"][k] for k in ks]
            _solve(used, *first)
            a = _bits(*_solve(used, *second))
            b = _bits(*_solve(fresh, *second))
            for i, k in enumerate(ks):
                assert np.array_equal(a[i], b[i]), CASES[k]
                assert np.array_equal(a[i], _bits(world["res"], world["sm"])[k]), CASES[k]
    finally:
        used.close(); fresh.close()
