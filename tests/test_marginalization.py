"""The device marginalization (vilf_marg.hip: k_marg_prepare[_td], k_marg_schur fast / exact, k_mf_chol_tiles, k_mf_chol, k_mf_tridiag, k_mf_ql, k_mf_apply, k_marg_finish,
k_prior_keep) against an exact Schur complement (tests/marg_reference.py) AT THE DEVICE'S OWN SOLVED STATE, on windows shaped to the kernels' edges (tests/marg_cases.py).

Error measures (every block weighted by its own scale, both bounded by 1):
    e_Lam = max_ij |Lam - Lam_ref|_ij / sqrt(Lam_ref,ii Lam_ref,jj)          e_b = max_i |b - b_ref|_i / (sqrt(Lam_ref,ii) |r0_ref|)          e_r = | |r0|^2 - |r0_ref|^2 | / |r0_ref|^2
Tolerance, per case and per measure, nothing chosen in advance: 10 x max(e_oracle, e_pert) — the fp64 oracle marginalized at the same state, and the exact reference
recomputed with every row entry moved by one rounding (marg_reference.bound). DESIGN.md ("Marginalization against an exact reference") holds the table of figures.
The tests without the gpu mark check the reference itself: the figures of an independent measurement, the counts every case claims, the 1e-8 truncation precondition."""
import hashlib
import numpy as np
import pytest
from vil_fusion_amd import abi, synth
import marg_cases as mc
import marg_reference as mr


@pytest.fixture(scope="module")
def solver():
    from vil_fusion_amd.estimator import BackendSolver
    s = BackendSolver()          # raises VilfError when the HIP library / GPU is missing: no silent fallback
    yield s
    s.close()


@pytest.fixture(scope="module")
def solver_for(solver):
    """a handle per option set (use_lidar_const / estimate_td / estimate_extrinsic are the handle's), the default one shared with `solver`"""
    from vil_fusion_amd.estimator import BackendSolver
    made = {}

    def get(case, base):
        key = tuple(sorted(case.opt.items()))
        if not key:
            return solver
        if key not in made:
            made[key] = BackendSolver(case.options(base))
        return made[key]
    yield get
    for s in made.values():
        s.close()


_BUILT, _REFS = {}, {}


def built(case, base):
    """(options, window, prior) of a case, once per source window"""
    if case.source not in _BUILT:
        o = case.options(base)
        _BUILT[case.source] = (o,) + tuple(case.build(o))
    return _BUILT[case.source]


def reference(oracle, case, base, state):
    """exact reference, tolerance, e_oracle and e_pert of a case's window at `state`; computed once per (window, state) and left unchanged"""
    o, win, prior = built(case, base)
    h = hashlib.sha1()
    for a in (state.Ps, state.Rs, state.Vs, state.Bas, state.Bgs, state.para_feature, state.tic, state.ric, np.array([state.td])):
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    key = (case.source, h.hexdigest())
    if key not in _REFS:
        ref = mr.exact_prior_products(o, win, prior, state, near_cut=case.near_cut)
        tol, e_or, e_pe = mr.bound(o, win, prior, state, ref, oracle.window_marginalize(o, win, state, prior), near_cut=case.near_cut)
        _REFS[key] = (ref, tol, e_or, e_pe)
    return _REFS[key]


# ---- the reference itself (CPU) ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,n_features,scale,scaled,maxnorm", [(7, 50, None, 2.5e-6, 1.2e-7), (22, 120, None, 2.0e-7, 4.7e-8), (7, 50, 1e6, 3.6e-10, 1.9e-13)])
def test_reference_reproduces_the_measured_oracle_errors(oracle, opts, seed, n_features, scale, scaled, maxnorm):
    """the error of the fp64 oracle against the exact Schur complement, as measured independently when these tests were specified (mpmath at 50 digits on the same factor
    rows): scaled and max-normalised, at the default IMU covariance (Amm up to 2.5e14) and at the tempered one. Within a factor of 3."""
    win, prior, _ = synth.make_window(seed, opts, synth.SynthConfig(with_prior=True, n_features=n_features))
    if scale:
        mc.temper(win, scale)
    res = oracle.window_solve(opts, win, prior)
    p = oracle.window_marginalize(opts, win, res, prior)
    ref = mr.exact_prior_products(opts, win, prior, res)
    J0, r0, blocks = abi.prior_to_numpy(p)
    eL, eb, er = mr.prior_measures(p, ref)
    mx = np.abs(J0.T @ J0 - ref["Lam"]).max() / np.abs(ref["Lam"]).max()
    print(f"MARGREF seed {seed} F {n_features} scale {scale}: scaled {eL:.3e} (measured {scaled:.1e}) max-normalised {mx:.3e} (measured {maxnorm:.1e}) e_b {eb:.3e} e_r {er:.3e}")
    assert scaled / 3 < eL < scaled * 3 and maxnorm / 3 < mx < maxnorm * 3
    assert ref["m"] == p.m and ref["n"] == p.n and ref["rank"] == p.n
    assert [(b["id"], b["size"], b["idx"]) for b in blocks] == [(b["id"], b["size"], b["idx"]) for b in ref["blocks"]]
    assert all(np.array_equal(a["x0"], b["x0"]) for a, b in zip(blocks, ref["blocks"]))


@pytest.mark.parametrize("case", mc.SOURCES + mc.RAGGED + mc.TILED, ids=repr)
def test_case_window_has_its_counts_and_stays_clear_of_the_cut(oracle, opts, case):
    """every case's window has the dropped-feature count mf and the frame-0 factor count f0 it claims, and — at the oracle's solved state — the reference's own
    precondition holds: no eigenvalue of Amm or of the kept block in [1e-9, 1e-7] other than one placed there on purpose (marg_reference raises BadCase), the kept
    dimension, the dropped dimension and the rank deficiency are the claimed ones."""
    o, win, prior = built(case, opts)
    mf, f0 = mc.frame0_counts(win)
    assert (case.mf is None or mf == case.mf) and (case.f0 is None or f0 == case.f0), (mf, f0)
    assert win.n_frames == mc.NF
    ref = mr.exact_prior_products(o, win, prior, oracle.window_solve(o, win, prior), near_cut=case.near_cut)
    md = ref["m"] - (mf if win.marginalization_flag == abi.MARGIN_OLD else 0)
    print(f"MARGCASE {case.name}: mf {mf} f0 {f0} F {win.n_features} m {ref['m']} n {ref['n']} rank {ref['rank']} eig(Amm) {ref['eig_mm'][0]:.2e} .. {ref['eig_mm'][1]:.2e} "
          f"eig(kept) {ref['eig_kept'][0]:.2e} .. {ref['eig_kept'][1]:.2e}")
    assert case.n is None or ref["n"] == case.n
    assert case.md is None or md == case.md or (case.name == "f-null" and md == case.md - 9)       # f-null: no factor touches SpeedBias[0], the reference leaves it out
    assert (ref["rank"] < ref["n"]) == case.rank_deficient


def test_shape_window_selects_reanchors_and_trims(opts):
    win, _, _ = synth.make_window(5, opts, synth.SynthConfig(n_features=60))
    win = synth.with_td_inputs(win, 1)
    have = mc.frame0_counts(win)[0]
    w = mc.shape_window(win, have + 3, track_lengths=[2] * (have + 3), n_other=5)           # three more than there are: re-anchored
    assert mc.frame0_counts(w) == (have + 3, 2 * (have + 3)) and w.n_features == have + 8
    assert w.obs_velocity.shape == (w.n_obs, 2) and w.obs_row.shape == (w.n_obs,) and w.feature_const.shape == (w.n_features,)
    k = int(np.where(w.feature_start_frame == 0)[0][0])
    src = int(np.where(win.para_feature == w.para_feature[k])[0][0])
    o0, s0 = int(w.feature_obs_offset[k]), int(win.feature_obs_offset[src])
    assert np.array_equal(w.obs_point[o0:o0 + 3], win.obs_point[s0:s0 + 3]) and w.feature_const[k] == win.feature_const[src]
    assert mc.spread(20, 161) == [9] + [8] * 19 and sum(mc.spread(104, 1025)) == 1025 and max(mc.spread(104, 1025)) == 10


def test_measures_see_a_wrong_row_in_a_small_block(oracle, opts):
    """what the max-normalised criterion hides: one dropped feature's Schur term left out changes a pose block by far more than the scaled tolerance and stays below 2e-5 of
    the largest entry of a prior whose largest entry is the bias information"""
    case = mc.BY_NAME["a-50-old"]
    o, win, prior = built(case, opts)
    res = oracle.window_solve(o, win, prior)
    ref = mr.exact_prior_products(o, win, prior, res)
    tol, e_or, e_pe = mr.bound(o, win, prior, res, ref, oracle.window_marginalize(o, win, res, prior))
    Lam = ref["Lam"].copy()
    Lam[0, 0] *= 1.0 + 1e-6                                              # a translation entry of the first kept pose, 1e2 .. 1e4 against 2.7e6
    eL, _, _ = mr.measures(Lam, ref["b"], ref["r0sq"], ref)
    assert eL > 100 * tol[0] and np.abs(Lam - ref["Lam"]).max() / np.abs(ref["Lam"]).max() < 2e-5
    assert all(t < 1e-7 for t in tol), tol                                # the tempered window: the rule's bound lies orders of magnitude inside 2e-5


# ---- the device (GPU) ---------------------------------------------------------------------------------------------------------------------------------------------------
def run_device(s, wins, priors, env, monkeypatch):
    """upload, solve, download the solved windows, marginalize with the hooks `env` set: (states, priors, path counters)"""
    s.batch_upload(wins, priors); s.batch_solve()
    states = s.batch_download()
    for k in env:
        monkeypatch.setenv(k, "1" if k != "VILF_MARG_POOL" else "2")
    try:
        s.batch_marginalize()
    finally:
        for k in env:
            monkeypatch.delenv(k)
    return states, [s.get_prior(i) for i in range(len(wins))], s.marginalize_stats()


def check_prior(oracle, base, case, state, pg, tag=""):
    """one device prior against the exact reference of its window at the device's state; prints the figures, then asserts"""
    ref, tol, e_or, e_pe = reference(oracle, case, base, state)
    J0, r0, blocks = abi.prior_to_numpy(pg)
    e = mr.prior_measures(pg, ref)
    rank = int(np.count_nonzero(np.abs(J0).max(axis=1) > 0))
    dx0 = max(float(np.abs(a["x0"] - b["x0"]).max()) for a, b in zip(blocks, ref["blocks"])) if len(blocks) == len(ref["blocks"]) else np.nan
    print(f"MARG {case.name}{tag}: m {pg.m} n {pg.n} rank {rank}/{ref['rank']} | e_oracle {e_or[0]:.2e} {e_or[1]:.2e} {e_or[2]:.2e} | e_pert {e_pe[0]:.2e} {e_pe[1]:.2e} {e_pe[2]:.2e} | "
          f"device {e[0]:.2e} {e[1]:.2e} {e[2]:.2e} | max|dx0| {dx0:.1e}")
    assert pg.valid == 1 and pg.n == ref["n"] and (case.n is None or pg.n == case.n)
    assert [(b["id"], b["size"], b["idx"]) for b in blocks] == [(b["id"], b["size"], b["idx"]) for b in ref["blocks"]]
    for a, b in zip(blocks, ref["blocks"]):
        assert np.array_equal(a["x0"], b["x0"]), (a["id"], a["x0"] - b["x0"])
    assert rank == ref["rank"] == np.linalg.matrix_rank(J0), "J0 has the reference's rank"
    for name, got, t in zip(("e_Lam", "e_b", "e_r"), e, tol):
        assert got <= t, f"{case.name}{tag}: {name} {got:.3e} > 10 x max(e_oracle, e_pert) = {t:.3e}"
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("case", mc.CASES, ids=repr)
def test_marginalization_against_exact_reference(solver_for, oracle, opts, monkeypatch, case):
    """one window per case: upload, solve and marginalize on the device, then the exact reference at the downloaded state. The path counters prove which kernels ran:
    Amm by the arrow Cholesky or the Jacobi eigen-solver, the kept block in Cholesky form or by the eigen-solver."""
    o, win, prior = built(case, opts)
    s = solver_for(case, opts)
    states, priors, st = run_device(s, [win], [prior], case.env, monkeypatch)
    print(f"MARG {case.name}: counters {st} hooks {case.env}")
    assert st["new_prior"] == 1 and st["unchanged"] == 0
    assert st["amm_cholesky"] == (1 if case.amm == "arrow" else 0), "Amm path"
    assert st["kept_cholesky"] == (1 if case.kept == "chol" else 0), "kept-block path"
    ref = check_prior(oracle, opts, case, states[0], priors[0])
    J0, _, _ = abi.prior_to_numpy(priors[0])
    if case.kept == "chol":
        assert np.array_equal(J0, np.triu(J0)) and (np.diag(J0) > 0).all(), "J0 = L^T"
    mf = mc.frame0_counts(win)[0] if win.marginalization_flag == abi.MARGIN_OLD else 0
    assert priors[0].m == case.md + mf
    assert (ref["rank"] < ref["n"]) == case.rank_deficient


@pytest.mark.gpu
def test_ragged_batch_against_exact_reference(solver, oracle, opts, monkeypatch):
    """3, 40, 150 and 400 features in one upload: the per-window strides (Fmax, FACmax) of every marginalization array"""
    made = [built(c, opts) for c in mc.RAGGED]
    states, priors, st = run_device(solver, [m[1] for m in made], [m[2] for m in made], (), monkeypatch)
    assert st["new_prior"] == 4 and st["amm_cholesky"] == 4 and st["kept_cholesky"] == 4, st
    for c, state, pg in zip(mc.RAGGED, states, priors):
        check_prior(oracle, opts, c, state, pg)


@pytest.mark.gpu
@pytest.mark.parametrize("env", [(), (mc.NO_CHOL,), (mc.EXACT, "VILF_MARG_POOL")], ids=["chol", "eig", "jacobi-pool2"])
def test_batch_of_65_against_exact_reference(solver, oracle, opts, monkeypatch, env):
    """65 windows tiled from 5: above 64 windows the kept-block kernels are launched per dimension class. Every slot against the reference of its source window, replicas
    bit-equal; with the Jacobi path forced through a pool of two workspace slots (33 rounds) the counters show that no window took the arrow path."""
    made = [built(c, opts) for c in mc.TILED]
    wins = [made[i % 5][1] for i in range(65)]; pri = [made[i % 5][2] for i in range(65)]
    states, priors, st = run_device(solver, wins, pri, env, monkeypatch)
    print(f"MARG g-tiled {env}: counters {st}")
    assert st["new_prior"] == 65 and st["unchanged"] == 0
    assert st["amm_cholesky"] == (0 if mc.EXACT in env else 65) and st["kept_cholesky"] == (0 if mc.NO_CHOL in env else 65), st
    for i in range(65):
        if i >= 5:
            assert bytes(priors[i]) == bytes(priors[i % 5]), f"slot {i} differs from its replica {i % 5}"
            assert np.array_equal(states[i].Ps, states[i % 5].Ps) and np.array_equal(states[i].para_feature, states[i % 5].para_feature)
        else:
            check_prior(oracle, opts, mc.TILED[i], states[i], priors[i], tag=f" {'+'.join(env) or 'default'}")


@pytest.mark.gpu
def test_second_new_without_its_pose_leaves_the_prior_untouched(solver, oracle, opts, monkeypatch):
    """MARGIN_SECOND_NEW and a prior without Pose[WINDOW_SIZE - 1] (estimator.cpp:982-983): status 2, the prior comes back byte for byte, counted as unchanged; a window
    that does marginalize, in the same batch, is not disturbed"""
    win, prior = mc.second_new_without_its_pose(opts)
    case = mc.BY_NAME["a-50-2nd"]
    o, w2, p2 = built(case, opts)
    assert mr.factor_rows(opts, win, prior, oracle.window_solve(opts, win, prior)) is None
    states, priors, st = run_device(solver, [win, w2], [prior, p2], (), monkeypatch)
    assert st == dict(new_prior=1, amm_cholesky=1, kept_cholesky=1, unchanged=1), st
    assert bytes(priors[0]) == bytes(prior)
    check_prior(oracle, opts, case, states[1], priors[1], tag=" beside an unchanged prior")


@pytest.mark.gpu
def test_prior_with_a_late_speed_bias_is_refused_and_the_handle_lives_on(solver, oracle, opts, monkeypatch):
    """a prior carrying SpeedBias[3] (id >= NF + 2) has no place in the marginalization's layout: status 3 -> VILF_ERR_UNSUPPORTED with the block table / dimension
    message; the next upload, solve and marginalization on the same handle are as good as ever"""
    from vil_fusion_amd.lib import VilfError
    win, prior = mc.prior_with_a_late_speed_bias(opts)
    solver.batch_upload([win], [prior]); solver.batch_solve()
    with pytest.raises(VilfError, match="block table / dimension") as ei:
        solver.batch_marginalize()
    assert f"status {abi.VILF_ERR_UNSUPPORTED}" in str(ei.value)
    assert solver.marginalize_stats() == dict(new_prior=0, amm_cholesky=0, kept_cholesky=0, unchanged=1)
    case = mc.BY_NAME["a-50-old"]
    o, w2, p2 = built(case, opts)
    states, priors, st = run_device(solver, [w2], [p2], (), monkeypatch)
    assert st == dict(new_prior=1, amm_cholesky=1, kept_cholesky=1, unchanged=0), st
    check_prior(oracle, opts, case, states[0], priors[0], tag=" after a refusal")
