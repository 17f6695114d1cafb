"""GPU parity tests proper: the HIP path (through the C ABI) against the CPU oracle on identical seeded inputs.
Run on the MI355X box: python -m pytest tests -m gpu."""
import copy
import ctypes as C
import numpy as np
import pytest
from vil_fusion_amd import abi, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    from vil_fusion_amd.estimator import BackendSolver
    s = BackendSolver()          # raises VilfError when the HIP library / GPU is missing: no silent fallback
    yield s
    s.close()


def rand_pose(rng, scale=1.0):
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    return np.concatenate([rng.normal(0, scale, 3), q])


def test_projection_factor_hook(solver, oracle, opts):
    rng = np.random.default_rng(0)
    for _ in range(10):
        Pi = rand_pose(rng); Pj = rand_pose(rng); Pj[:3] = Pi[:3] + rng.normal(0, 0.5, 3)
        Pj[3:] = synth.q_mul(Pi[3:], synth.q_exp(rng.normal(0, 0.1, 3)))
        ex = np.concatenate([np.array(opts.TIC[:]), synth.R_to_q(np.array(opts.RIC[:]).reshape(3, 3))])
        lam = np.array([1.0 / rng.uniform(4, 30)])
        pi = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.2, 0.2), 1.0]); pj = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.2, 0.2), 1.0])
        r, J = solver.eval_projection([Pi, Pj, ex, lam], pi, pj)
        r0, J0 = oracle.eval_factor("projection", opts, [Pi, Pj, ex, lam], pi, pj, sizes=[7, 7, 7, 1], nres=2)
        assert np.allclose(r, r0, rtol=1e-11, atol=1e-10)
        for k in (0, 1, 2, 3):            # Pose_i, Pose_j, Ex_Pose (projection_factor.cpp:97-104), inverse depth
            assert np.allclose(J[k], J0[k], rtol=1e-10, atol=1e-9 * max(1, np.abs(J0[k]).max()))


def test_imu_factor_hook(solver, oracle, opts):
    """IMUFactor::Evaluate (imu_factor.h:19-178) in its parts. (i) residual and Jacobians BEFORE sqrt_info — pure geometry, HIP vs oracle at 1e-11; (ii) sqrt_info =
    LLT(cov^-1).L^T: entries ~1e6..1e7 from a 15 x 15 inverse + Cholesky of an ill-conditioned covariance computed by two different fp64 algorithms, so the comparable
    quantity is the information matrix sqrt_info^T sqrt_info against cov^-1 (numpy), 1e-9 relative, for both; (iii) the product, at the tolerance (ii) allows."""
    rng = np.random.default_rng(1)
    for _ in range(4):
        win, _, _ = synth.make_window(int(rng.integers(1 << 30)), opts, synth.SynthConfig(n_features=20, with_prior=False))
        j = int(rng.integers(1, win.n_frames))
        pre = abi.ImuPreint.from_buffer_copy(win.imu[j].tobytes())
        params = [win.para_pose[j - 1], win.para_speed_bias[j - 1], win.para_pose[j], win.para_speed_bias[j]]
        rr, Jr, S = solver.eval_imu_raw(params, pre)
        rr0, Jr0 = oracle.eval_factor("imu_raw", opts, params, pre, sizes=[7, 9, 7, 9], nres=15)
        assert np.abs(rr - rr0).max() <= 1e-11 * max(1.0, np.abs(rr0).max())
        for a, b in zip(Jr, Jr0):
            assert np.abs(a - b).max() <= 1e-11 * max(1.0, np.abs(b).max())
        cov = np.array(pre.covariance[:]).reshape(15, 15)
        info = np.linalg.inv(cov)
        S0 = np.zeros(225); oracle.lib().vilo_imu_sqrt_info(C.byref(pre), abi.dptr(S0)); S0 = S0.reshape(15, 15)
        for M in (S, S0):
            assert np.allclose(M, np.triu(M)), "sqrt_info = L^T is upper triangular"
            assert np.abs(M.T @ M - info).max() <= 1e-9 * np.abs(info).max()
        r, J = solver.eval_imu(params, pre)
        r0, J0 = oracle.eval_factor("imu", opts, params, pre, sizes=[7, 9, 7, 9], nres=15)
        assert np.abs(r - r0).max() <= 1e-7 * max(1.0, np.abs(r0).max())
        for a, b in zip(J, J0):
            assert np.abs(a - b).max() <= 1e-7 * np.abs(b).max()
        assert np.abs(r - S @ rr).max() <= 1e-12 * max(1.0, np.abs(r).max()), "the whitened residual is the product of the two parts"


def test_lidar_edge_surf_plus_hooks(solver, oracle, opts):
    rng = np.random.default_rng(2)
    L = oracle.lib()
    for _ in range(5):
        Pi = rand_pose(rng); Pj = rand_pose(rng)
        c = abi.LidarConstraint()
        q = synth.q_exp(rng.normal(0, 0.05, 3))
        for k in range(4):
            c.q[k] = q[k]
        for k in range(3):
            c.t[k] = rng.normal()
        r, J = solver.eval_lidar_between([Pi, Pj], c)
        r0, J0 = oracle.eval_factor("lidar_between", opts, [Pi, Pj], c, sizes=[7, 7], nres=6)
        assert np.allclose(r, r0, rtol=1e-11, atol=1e-10)
        for a, b in zip(J, J0):
            assert np.allclose(a, b, rtol=1e-11, atol=1e-11)
        q = rng.normal(size=4); q /= np.linalg.norm(q)
        pose = np.concatenate([q, rng.normal(0, 2, 3)])
        cp = rng.normal(0, 5, 3); a = rng.normal(0, 5, 3); b = a + rng.normal(0, 0.2, 3)
        r, J = solver.eval_edge(pose, cp, a, b)
        r0 = np.zeros(3); J0 = np.zeros((3, 7))
        L.vilo_eval_edge(abi.dptr(pose), abi.dptr(cp), abi.dptr(a), abi.dptr(b), abi.dptr(r0), abi.dptr(J0))
        assert np.allclose(r, r0, rtol=1e-11, atol=1e-11) and np.allclose(J, J0, rtol=1e-11, atol=1e-10)
        n = rng.normal(size=3); n /= np.linalg.norm(n); d = float(rng.normal())
        r, J = solver.eval_surf(pose, cp, n, d)
        r0 = np.zeros(1); J0 = np.zeros((1, 7))
        L.vilo_eval_surf.argtypes = [abi.c_double_p, abi.c_double_p, abi.c_double_p, C.c_double, abi.c_double_p, abi.c_double_p]
        L.vilo_eval_surf(abi.dptr(pose), abi.dptr(cp), abi.dptr(n), d, abi.dptr(r0), abi.dptr(J0))
        assert np.allclose(r, r0, rtol=1e-12, atol=1e-12) and np.allclose(J, J0, rtol=1e-12, atol=1e-12)
        x = rand_pose(rng); dl = rng.normal(0, 0.1, 6); o = np.zeros(7)
        L.vilo_pose_plus(abi.dptr(x), abi.dptr(dl), abi.dptr(o))
        assert np.allclose(solver.pose_plus(x, dl), o, atol=1e-15)
        L.vilo_se3_plus(abi.dptr(pose), abi.dptr(dl), abi.dptr(o))
        assert np.allclose(solver.pose_plus(pose, dl, se3=True), o, atol=1e-14)


def _compare(got, ref, tol_p=1e-7, tol_r=1e-8, tol_cost=1e-7):
    assert got.summary["num_iterations"] == ref.summary["num_iterations"]
    assert got.summary["num_successful_steps"] == ref.summary["num_successful_steps"]
    assert abs(got.summary["initial_cost"] - ref.summary["initial_cost"]) <= 1e-9 * ref.summary["initial_cost"]
    assert abs(got.summary["final_cost"] - ref.summary["final_cost"]) <= tol_cost * ref.summary["final_cost"]
    assert np.abs(got.Ps - ref.Ps).max() < tol_p
    assert np.abs(got.Rs - ref.Rs).max() < tol_r
    assert np.abs(got.Vs - ref.Vs).max() < 10 * tol_p
    assert np.abs(got.Bas - ref.Bas).max() < 1e-6 and np.abs(got.Bgs - ref.Bgs).max() < 1e-7
    assert np.abs(1.0 / got.para_feature - 1.0 / ref.para_feature).max() < 1e-5   # depth, metres


@pytest.mark.parametrize("seed,with_prior,use_lidar", [(1, False, True), (2, True, True), (3, True, False), (4, False, False)])
def test_window_solve_matches_oracle(solver, oracle, seed, with_prior, use_lidar):
    """configs[1]/[2] back-end: one 11-frame window, visual + IMU (+ LiDAR between-factors, + prior): pose-trajectory
    equality with the CPU restatement. Tolerances: |dP| < 1e-7 m, |dR| < 1e-8, relative cost 1e-7 after 8 iterations."""
    from vil_fusion_amd.estimator import BackendSolver
    o = oracle.default_options()
    o.use_lidar_const = 1 if use_lidar else 0
    s = BackendSolver(o)
    win, prior, _ = synth.make_window(seed, o, synth.SynthConfig(use_lidar=use_lidar, with_prior=with_prior))
    s.set_prior(prior if with_prior else None)
    got = s.optimization(win)
    ref = oracle.window_solve(o, win, prior if with_prior else None)
    _compare(got, ref)
    s.close()


def test_edge_cases(solver, oracle, opts):
    # all features constant (no Schur block), very few features, and a strongly perturbed window (rejected steps: test_rejected_steps_match_oracle)
    for cfg in (synth.SynthConfig(const_fraction=1.0, n_features=40), synth.SynthConfig(n_features=3, const_fraction=0.0),
                synth.SynthConfig(n_features=150, state_noise=(0.5, np.deg2rad(5.0), 0.5))):
        win, prior, _ = synth.make_window(9, opts, cfg)
        solver.set_prior(prior)
        got = solver.optimization(win)
        ref = oracle.window_solve(opts, win, prior)
        _compare(got, ref, tol_p=1e-6, tol_r=1e-7, tol_cost=1e-6)


def test_rejected_steps_match_oracle(solver, oracle, opts):
    """Windows whose trust-region loop REJECTS steps (found with the oracle: strongly perturbed states): 6 or 7 successful steps out of 8 iterations, with and without a
    re-used Gauss-Newton step. The device takes the step inside k_linearize, which linearises at the candidate into the second workspace and keeps x, its cost and its
    workspace when the step is rejected — this is the path these windows exercise. Same iteration / accepted-step / linear-solve counts and the same state as the oracle,
    one window at a time and as a batch."""
    cases = [(1.5, 15.0, 409), (3.0, 25.0, 405), (3.0, 25.0, 408), (3.0, 25.0, 431), (3.0, 25.0, 400)]
    made = [synth.make_window(seed, opts, synth.SynthConfig(n_features=60, state_noise=(nz, np.deg2rad(deg), nz))) for nz, deg, seed in cases]
    refs = [oracle.window_solve(opts, w, p) for w, p, _ in made]
    assert any(r.summary["num_successful_steps"] < r.summary["num_iterations"] for r in refs), "the cases were picked for their rejected steps"
    assert any(r.summary["num_linear_solves"] < r.summary["num_iterations"] for r in refs), "... and for a re-used Gauss-Newton step"
    for (w, p, _), ref in zip(made, refs):
        solver.set_prior(p)
        got = solver.optimization(w)
        for k in ("num_iterations", "num_successful_steps", "num_linear_solves"):
            assert got.summary[k] == ref.summary[k], k
        assert abs(got.summary["final_cost"] - ref.summary["final_cost"]) <= 1e-4 * ref.summary["final_cost"]
        # states (these windows are far from convergence and hold near-zero / negative inverse depths: the inverse depths themselves are compared, not the depths)
        assert np.abs(got.Ps - ref.Ps).max() < 1e-4 and np.abs(got.Rs - ref.Rs).max() < 1e-5 and np.abs(got.Vs - ref.Vs).max() < 1e-3      # costs of 1e8..1e9 after 8 iterations: rounding differences are amplified
        assert np.abs(got.para_feature - ref.para_feature).max() < 1e-4             # ill-conditioned by construction (costs ~ 1e9, near-singular steps): the counts above are the point
    solver.batch_upload([m[0] for m in made], [m[1] for m in made])
    solver.batch_solve()
    for got, sm, ref in zip(solver.batch_download(), solver.batch_summaries(), refs):
        assert (sm.num_iterations, sm.num_successful_steps, sm.num_linear_solves) == (ref.summary["num_iterations"], ref.summary["num_successful_steps"], ref.summary["num_linear_solves"])
        assert np.abs(got.Ps - ref.Ps).max() < 1e-4


def test_batch_matches_single_and_rewind_is_deterministic(solver, oracle, opts):
    wins, priors = synth.make_batch(5, 12, opts, synth.SynthConfig(n_features=80), distinct=6)
    solver.batch_upload(wins, priors)
    solver.batch_solve()
    res1 = solver.batch_download()
    solver.batch_rewind()
    solver.batch_solve()
    res2 = solver.batch_download()
    for i, (a, b) in enumerate(zip(res1, res2)):
        assert np.array_equal(a.Ps, b.Ps) and np.array_equal(a.para_feature, b.para_feature), "re-run must be bit-identical"
        ref = oracle.window_solve(opts, wins[i], priors[i])
        _compare(a, ref)
    for i in range(6):
        assert np.array_equal(res1[i].Ps, res1[i + 6].Ps), "identical windows in different slots must give identical results"


def test_solve_to_convergence_matches_oracle(oracle):
    """Both solvers run until they stop by themselves (budget 1000 iterations; FUNCTION_TOLERANCE after ~120): the fixed point, not just eight steps towards it. The
    oracle's fixed point is pinned to scipy's minimiser of the independently restated problem in tests/test_fixed_point_scipy.py; here the HIP path reaches the same
    point: same termination, final cost to 1e-7 relative, poses to 1e-5 m (over ~120 iterations the two trust-region histories may part by an iteration)."""
    from vil_fusion_amd.estimator import BackendSolver
    o = oracle.default_options(); o.max_num_iterations = 1000
    s = BackendSolver(o)
    made = [synth.make_window(7001 + k, o, synth.SynthConfig(n_features=60)) for k in range(5)]
    s.batch_upload([m[0] for m in made], [m[1] for m in made]); s.batch_solve()
    for got, sm, (win, prior, _) in zip(s.batch_download(), s.batch_summaries(), made):
        ref = oracle.window_solve(o, win, prior)
        assert sm.termination == ref.summary["termination"] == 1
        assert abs(sm.num_iterations - ref.summary["num_iterations"]) <= 2, (sm.num_iterations, ref.summary["num_iterations"])
        assert abs(sm.final_cost - ref.summary["final_cost"]) <= 1e-7 * ref.summary["final_cost"]
        assert np.abs(got.Ps - ref.Ps).max() < 1e-5 and np.abs(got.Rs - ref.Rs).max() < 1e-6
    s.close()


def test_live_window_lists_leave_every_result_untouched(oracle, monkeypatch):
    """A batch in which windows stop at different iterations (half of them start at their own fixed point: FUNCTION_TOLERANCE in iteration 1; the others run the
    budget) in an interleaved arrangement: once something has stopped, k_linearize lists the windows still running and the later launches address them through
    that list (the finished ones' workgroups leave from the end of the grid: the saving no longer depends on where they sit in the batch). Which workgroup takes
    which window is all that changes: every state, cost and count equal bit for bit to the run with the lists switched off (VILF_NO_LIVE_LIST)."""
    import copy
    from vil_fusion_amd.estimator import BackendSolver
    o = oracle.default_options()
    made = [synth.make_window(7101 + k, o, synth.SynthConfig(n_features=70 + 5 * k)) for k in range(8)]
    o2 = oracle.default_options(); o2.max_num_iterations = 1000
    pre = BackendSolver(o2); pre.batch_upload([m[0] for m in made[:4]], [m[1] for m in made[:4]]); pre.batch_solve(); fixed = pre.batch_download(); pre.close()
    wins, priors = [], []
    for k in range(8):
        w = made[k][0]
        if k < 4:
            w = copy.deepcopy(w)
            w.para_pose = np.ascontiguousarray(np.asarray(fixed[k].para_pose).reshape(-1, 7)); w.para_speed_bias = np.ascontiguousarray(np.asarray(fixed[k].para_speed_bias).reshape(-1, 9))
            w.para_feature = np.ascontiguousarray(fixed[k].para_feature)
        wins.append(w); priors.append(made[k][1])
    order = [(3 * i + i // 5) % 8 for i in range(96)]            # finished and running windows interleaved, 96 slots
    def run():
        s = BackendSolver(o)
        s.batch_upload([wins[k] for k in order], [priors[k] for k in order]); s.batch_solve()
        out = s.batch_download(); sm = [(x.num_iterations, x.num_successful_steps, x.termination, x.final_cost) for x in s.batch_summaries()]
        s.close()
        return out, sm
    a, sa = run()
    monkeypatch.setenv("VILF_NO_LIVE_LIST", "1")
    b, sb = run()
    monkeypatch.delenv("VILF_NO_LIVE_LIST")
    assert sa == sb
    its = [x[0] for x in sa]
    assert min(its) <= 2 and max(its) == 8, its                   # windows that stop at once beside windows that use the budget
    for x, y in zip(a, b):
        for key in ("Ps", "Rs", "Vs", "Bas", "Bgs", "para_feature", "para_pose", "para_speed_bias"):
            assert np.array_equal(getattr(x, key), getattr(y, key)), key
    for slot, k in enumerate(order):                             # and each window against the oracle, whatever its neighbours did
        if k >= 4:
            ref = oracle.window_solve(o, wins[k], priors[k])
            assert a[slot].summary["num_iterations"] == ref.summary["num_iterations"] and np.abs(a[slot].Ps - ref.Ps).max() < 1e-7


def _prior_products(p):
    J0, r0, blocks = abi.prior_to_numpy(p)
    return J0.T @ J0, J0.T @ r0, blocks


@pytest.mark.parametrize("seed,with_prior,flag", [(21, False, abi.MARGIN_OLD), (22, True, abi.MARGIN_OLD), (23, True, abi.MARGIN_SECOND_NEW)])
def test_marginalization_matches_oracle(solver, oracle, opts, seed, with_prior, flag):
    """MarginalizationInfo on the device (estimator.cpp:863-1046) vs the CPU restatement: compare the eigenvector-sign/order free
    products J0^T J0 and J0^T r0 and the shifted block table. Amm spans ~14 decades (IMU bias information), so two fp64
    eigen-solvers agree to ~1e-6 relative (same bound as oracle vs numpy in tests/test_oracle_solver.py)."""
    win, prior, _ = synth.make_window(seed, opts, synth.SynthConfig(with_prior=with_prior, marginalization_flag=flag, n_features=120))
    solver.set_prior(prior if with_prior else None)
    got = solver.optimization(win)
    solver.marginalize()
    pg = solver.get_prior()
    ref = oracle.window_solve(opts, win, prior if with_prior else None)
    pr = oracle.window_marginalize(opts, win, ref, prior if with_prior else None)
    assert pg.valid == pr.valid and pg.n == pr.n and pg.n_blocks == pr.n_blocks
    Lg, bg, blg = _prior_products(pg)
    Lr, br_, blr = _prior_products(pr)
    assert [b["id"] for b in blg] == [b["id"] for b in blr]
    assert [b["idx"] for b in blg] == [b["idx"] for b in blr]
    for a, b in zip(blg, blr):
        assert np.allclose(a["x0"], b["x0"], atol=1e-9)
    assert np.abs(Lg - Lr).max() / np.abs(Lr).max() < 2e-5
    assert np.abs(bg - br_).max() / np.abs(br_).max() < 2e-5


def test_solve_marginalize_solve_chain(solver, oracle, opts):
    """window k solve -> marginalize (prior stays on the device) -> window k+1 solve with that prior."""
    cfg = synth.SynthConfig(with_prior=False, n_features=100)
    win, _, _ = synth.make_window(31, opts, cfg)
    solver.set_prior(None)
    solver.optimization(win)
    solver.marginalize()
    win2, _, _ = synth.make_window(31, opts, cfg)     # same geometry re-used as the "next" window (block ids are already shifted)
    got2 = solver.optimization(win2)                  # uses the device-resident prior of slot 0
    ref = oracle.window_solve(opts, win, None)
    pr = oracle.window_marginalize(opts, win, ref, None)
    ref2 = oracle.window_solve(opts, win2, pr)
    assert got2.summary["num_iterations"] == ref2.summary["num_iterations"]
    assert abs(got2.summary["final_cost"] - ref2.summary["final_cost"]) <= 1e-5 * ref2.summary["final_cost"]
    assert np.abs(got2.Ps - ref2.Ps).max() < 1e-5 and np.abs(got2.Rs - ref2.Rs).max() < 1e-6


def test_replicas_and_reruns_are_bit_identical(solver, opts):
    """Race detector: 512 resident windows tiled from 8 distinct ones; every replica and every re-run after a rewind must be
    bit-identical (LDS scatter-adds of different factor families into the same tile entry must be barrier-separated)."""
    wins, priors = synth.make_batch(5, 512, opts, synth.SynthConfig(n_features=80), distinct=8)
    solver.batch_upload(wins, priors)
    base = None
    for rep in range(6):
        if rep:
            solver.batch_rewind()
        solver.batch_solve()
        P = np.stack([np.concatenate([r.Ps.ravel(), r.Vs.ravel(), r.Bas.ravel(), r.Bgs.ravel()]) for r in solver.batch_download()])
        if base is None:
            base = P
            assert all(np.array_equal(P[i], P[i % 8]) for i in range(512)), "replicas of the same window differ"
        else:
            assert np.array_equal(P, base), f"re-run {rep} differs"
    # the marginalization of replicas (fast path: fixed summation orders, no atomics) is bit-identical too, and a rewind restores the priors
    solver.batch_marginalize()
    pri = [solver.get_prior(i) for i in (0, 8, 16, 3, 11)]
    assert bytes(pri[0]) == bytes(pri[1]) == bytes(pri[2]) and bytes(pri[3]) == bytes(pri[4]) and bytes(pri[0]) != bytes(pri[3])
    solver.batch_rewind(); solver.batch_solve()
    P2 = np.stack([np.concatenate([r.Ps.ravel(), r.Vs.ravel(), r.Bas.ravel(), r.Bgs.ravel()]) for r in solver.batch_download()])
    assert np.array_equal(P2, base), "rewind after a marginalization must restore the uploaded priors"
    # the upload of 512 windows packs on the host threads and copies in quarters; eight windows are packed by the calling thread: same bytes on the device, same results
    solver.batch_upload(wins[:8], priors[:8])
    solver.batch_solve()
    P3 = np.stack([np.concatenate([r.Ps.ravel(), r.Vs.ravel(), r.Bas.ravel(), r.Bgs.ravel()]) for r in solver.batch_download()])
    assert np.array_equal(P3, base[:8]), "threaded / chunked upload and serial upload differ"


def test_asynchronous_upload_over_two_handles_gives_the_same_results(opts):
    """vilf_set_async_upload: the upload returns once its copies are enqueued, the solve (sync = 0) queues behind them, and the NEXT upload of the handle waits before it
    rewrites the pinned staging. A stream of different batches alternating over two such handles — the loop bench.py's pcie_inclusive.stream_of_batches measures — must
    return, batch for batch, the bits of the synchronous path; so must two uploads of one handle directly after each other (the first one's copies still in flight)."""
    from vil_fusion_amd.estimator import BackendSolver
    nb = 320                                                                   # >= 256: host threads pack, the copies go out in quarters
    batches = [synth.make_batch(40 + k, nb, opts, synth.SynthConfig(n_features=60 + 10 * k), distinct=16) for k in range(4)]
    flat = lambda rs: np.stack([np.concatenate([r.Ps.ravel(), r.Rs.ravel(), r.Vs.ravel(), r.Bas.ravel(), r.Bgs.ravel()]) for r in rs])
    ref = BackendSolver(opts)
    want = []
    for wins, priors in batches:
        ref.batch_upload(wins, priors); ref.batch_solve(); want.append(flat(ref.batch_download()))
    ref.close()
    hs = [BackendSolver(opts), BackendSolver(opts)]
    for h in hs:
        h.set_async_upload(True)
    got, pending = [None] * 4, [None, None]
    for k, (wins, priors) in enumerate(batches):                               # batch k on handle k % 2
        h = hs[k % 2]
        if pending[k % 2] is not None:
            got[pending[k % 2]] = flat(h.batch_download())
        h.batch_upload(wins, priors); h.batch_solve(sync=False); pending[k % 2] = k
    for j in range(2):
        got[pending[j]] = flat(hs[j].batch_download())
    for k in range(4):
        assert np.array_equal(got[k], want[k]), f"batch {k}"
    # two uploads back to back on one handle, nothing in between: the second waits for the first one's copies before it packs into the same staging
    hs[0].batch_upload(*batches[0]); hs[0].batch_upload(*batches[3]); hs[0].batch_solve(sync=False)
    assert np.array_equal(flat(hs[0].batch_download()), want[3])
    hs[0].set_async_upload(False)
    hs[0].batch_upload(*batches[1]); hs[0].batch_solve()
    assert np.array_equal(flat(hs[0].batch_download()), want[1])
    for h in hs:
        h.close()


def test_every_upload_path_puts_the_same_batch_on_the_device(opts, monkeypatch):
    """The four ways an upload reaches the device — (a) B = 8: one host image + the span copy kernel, (b) B = 8 with VILF_NO_STAGED_UPLOAD=1: one packing pass + a copy per
    array (the download takes its per-array arm too), (c) 96 slots: packed by the host threads, (d) 300 slots: packers overlapped with the copies of four chunks — each
    with and without vilf_set_async_upload. Eight distinct windows (different feature counts: the padding up to Fmax / FACmax differs per window) with priors are uploaded,
    solved, marginalized and downloaded; every slot i must return, to the bit, the state, the summary counts and the new prior that (a) returns for window i % 8."""
    from vil_fusion_amd.estimator import BackendSolver
    base = [synth.make_window(7100 + i, opts, synth.SynthConfig(n_features=40 + 23 * i, marginalization_flag=1 if i % 3 == 2 else 0)) for i in range(8)]
    fields = ("para_pose", "para_speed_bias", "para_feature", "Ps", "Rs", "Vs", "Bas", "Bgs", "tic", "ric")

    def run(s, n, no_staged):
        if no_staged: monkeypatch.setenv("VILF_NO_STAGED_UPLOAD", "1")
        try:
            s.batch_upload([base[i % 8][0] for i in range(n)], [base[i % 8][1] for i in range(n)])
            s.batch_solve(); s.batch_marginalize()
            res, sums = s.batch_download(), s.batch_summaries()
        finally:
            if no_staged: monkeypatch.delenv("VILF_NO_STAGED_UPLOAD")
        out = []
        for i in range(n):
            state = np.concatenate([np.asarray(getattr(res[i], k), dtype=np.float64).ravel() for k in fields] + [[res[i].td]])
            counts = np.array([sums[i].num_iterations, sums[i].num_successful_steps, sums[i].num_linear_solves, sums[i].termination])
            out.append((state, counts, np.frombuffer(bytes(s.get_prior(i)), dtype=np.uint8)))
        return out

    s = BackendSolver(opts)
    try:
        want = run(s, 8, False)
        assert any(not np.array_equal(want[0][0][:77], want[i][0][:77]) for i in range(1, 8)), "the eight windows must differ"
        for asynchronous in (False, True):
            s.set_async_upload(asynchronous)
            for arm, (n, no_staged) in dict(staged=(8, False), one_pass=(8, True), threaded=(96, False), chunked=(300, False)).items():
                got = run(s, n, no_staged)
                for i in range(n):
                    for part, g, w in zip(("state", "summary counts", "prior"), got[i], want[i % 8]):
                        assert np.array_equal(g, w), (arm, asynchronous, i, part)
    finally:
        s.close()


def test_prior_factor_hook(solver, oracle, opts):
    """MarginalizationFactor::Evaluate on the device vs the oracle: residual r0 + J0 dx (quaternion sign flip) and J0 column blocks."""
    rng = np.random.default_rng(12)
    win, prior, _ = synth.make_window(5, opts)
    _, _, blocks = abi.prior_to_numpy(prior)
    params = []
    for b in blocks:
        x = win.para_pose[b["id"]] if b["size"] == 7 and b["id"] < 11 else (win.para_ex_pose if b["size"] == 7 else win.para_speed_bias[b["id"] - 11])
        x = np.array(x, dtype=np.float64)
        if b["size"] == 7 and rng.uniform() < 0.5:
            x[3:] = -x[3:]                      # same rotation, opposite quaternion sign: exercises the w < 0 branch
        params.append(x)
    sizes = [b["size"] for b in blocks]
    r, J = solver.eval_prior(prior, params)
    r0, J0 = oracle.eval_factor("prior", None, params, prior, sizes=sizes, nres=prior.n)
    assert np.allclose(r, r0, rtol=1e-11, atol=1e-10 * max(1.0, np.abs(r0).max()))
    for a, b in zip(J, J0):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("n_features", [120, 1000])       # 1000: Amm (m ~ 160) no longer fits the LDS eigen-solver -> global-memory variant
def test_marginalization_exact_path(solver, oracle, opts, monkeypatch, n_features):
    """The arrow fast path is what well-conditioned windows take; VILF_MARG_FORCE_EXACT sends them through the exact path instead
    (Jacobi eigen-decomposition of Amm with the reference's 1e-8 truncation). Both must agree with the oracle and with each other."""
    win, prior, _ = synth.make_window(22, opts, synth.SynthConfig(with_prior=True, n_features=n_features))
    res = {}
    for tag in ("fast", "exact"):
        if tag == "exact":
            monkeypatch.setenv("VILF_MARG_FORCE_EXACT", "1")
        solver.set_prior(prior)
        solver.optimization(win)
        solver.marginalize()
        res[tag] = _prior_products(solver.get_prior())
    monkeypatch.delenv("VILF_MARG_FORCE_EXACT")
    ref = oracle.window_solve(opts, win, prior)
    Lr, br_, _ = _prior_products(oracle.window_marginalize(opts, win, ref, prior))
    for tag in ("fast", "exact"):
        Lg, bg, _ = res[tag]
        assert np.abs(Lg - Lr).max() / np.abs(Lr).max() < 2e-5 and np.abs(bg - br_).max() / np.abs(br_).max() < 2e-5, tag
    assert np.abs(res["fast"][0] - res["exact"][0]).max() / np.abs(Lr).max() < 2e-5
    assert not np.array_equal(res["fast"][0], res["exact"][0]), "the hook did not switch paths (two different algorithms cannot agree bit for bit)"


def test_marginalization_exact_path_workspace_pool(solver, opts, monkeypatch):
    """The exact path's workspace (rotation log, Amm, X) is a pool of slots shared by the flagged windows, taken in rounds when the pool is smaller than the batch
    (VILF_MARG_POOL forces that on a small batch): the priors must not depend on the pool size."""
    wins, priors = synth.make_batch(31, 7, opts, distinct=7)
    monkeypatch.setenv("VILF_MARG_FORCE_EXACT", "1")
    out = {}
    for pool in ("7", "3", "1"):
        monkeypatch.setenv("VILF_MARG_POOL", pool)
        solver.batch_upload(wins, priors)
        solver.batch_solve()
        solver.batch_marginalize()
        out[pool] = [_prior_products(solver.get_prior(slot=k)) for k in range(7)]
    monkeypatch.delenv("VILF_MARG_POOL"); monkeypatch.delenv("VILF_MARG_FORCE_EXACT")
    for pool in ("3", "1"):
        for k in range(7):
            assert np.array_equal(out[pool][k][0], out["7"][k][0]) and np.array_equal(out[pool][k][1], out["7"][k][1]), (pool, k)


def test_projection_td_factor_hook(solver, oracle, opts):
    """ProjectionTdFactor on the device (factor level; the device solve itself does not estimate td) vs the oracle, all five blocks."""
    import test_oracle_factors as tof
    rng = np.random.default_rng(22)
    for _ in range(10):
        params, pi, pj, vi, vj, tdi, tdj, ri, rj = tof._td_case(rng, opts)
        r, J = solver.eval_projection_td(params, pi, pj, vi, vj, tdi, tdj, ri, rj)
        r0, J0 = oracle.eval_factor("projection_td", opts, params, pi, pj, vi, vj, tdi, tdj, ri, rj, sizes=[7, 7, 7, 1, 1], nres=2)
        assert np.allclose(r, r0, rtol=1e-11, atol=1e-10)
        for a, b in zip(J, J0):
            assert np.allclose(a, b, rtol=1e-10, atol=1e-9 * max(1, np.abs(b).max()))


def test_ragged_batch_and_maximum_sizes(solver, oracle, opts):
    """One batch of windows with very different sizes — 3, 40, 150 and the ABI maximum of 1000 features (NUM_OF_F) — plus a window whose
    features all start in frame 0 and one whose first IMU interval is invalid (sum_dt > 10 s: the reference skips that IMUFactor,
    estimator.cpp:745): every slot must match the oracle; solve + marginalization of the 1000-feature window included."""
    cfgs = [synth.SynthConfig(n_features=3, const_fraction=0.0), synth.SynthConfig(n_features=40), synth.SynthConfig(n_features=150),
            synth.SynthConfig(n_features=1000), synth.SynthConfig(n_features=60)]
    built = [synth.make_window(40 + k, opts, c) for k, c in enumerate(cfgs)]
    wins = [b[0] for b in built]; priors = [b[1] for b in built]
    assert wins[3].n_features == 1000
    # all tracks from frame 0: re-anchor the feature table of the last window (keeps the observations, drops tracks that would not fit)
    w4 = wins[4]
    n_obs = np.diff(w4.feature_obs_offset)
    w4.feature_start_frame[:] = 0
    keep = n_obs <= 11
    assert keep.all()
    # an extra window with an invalid first IMU interval
    w5, p5, _ = synth.make_window(46, opts, synth.SynthConfig(n_features=50))
    w5.imu[1, 0] = 12.0                                          # sum_dt of pre_integrations[1]
    wins.append(w5); priors.append(p5)
    solver.batch_upload(wins, priors)
    solver.batch_solve()
    got = solver.batch_download()
    for i, (w, p) in enumerate(zip(wins, priors)):
        ref = oracle.window_solve(opts, w, p)
        _compare(got[i], ref, tol_p=1e-6, tol_r=1e-7, tol_cost=1e-6)
    solver.batch_marginalize()
    pg = solver.get_prior(3)
    pr = oracle.window_marginalize(opts, wins[3], oracle.window_solve(opts, wins[3], priors[3]), priors[3])
    Lg, bg, blg = _prior_products(pg); Lr, br_, blr = _prior_products(pr)
    assert [b["id"] for b in blg] == [b["id"] for b in blr] and pg.m == pr.m
    assert np.abs(Lg - Lr).max() / np.abs(Lr).max() < 2e-5 and np.abs(bg - br_).max() / np.abs(br_).max() < 2e-5


def test_device_preintegration_batch(solver, opts):
    """IntegrationBase for many intervals on the device (one lane per interval, the same routine as the host
    vilf_imu_preintegrate) against the independent numpy restatement: ragged sample counts, including an empty interval."""
    from vil_fusion_amd.estimator import imu_preintegrate_batch
    rng = np.random.default_rng(31)
    n, mx, dt = 37, 20, 0.01
    ns = rng.integers(0, mx + 1, n); ns[0] = 0; ns[1] = mx
    acc = rng.normal(0, 1.0, (n, mx + 1, 3)) + np.array([0, 0, 9.8]); gyr = rng.normal(0, 0.2, (n, mx + 1, 3))
    ba = rng.normal(0, 0.02, (n, 3)); bg = rng.normal(0, 0.002, (n, 3))
    noise = abi.ImuNoise(synth.ACC_N, synth.GYR_N, synth.ACC_W, synth.GYR_W)
    got = imu_preintegrate_batch(solver, noise, acc[:, 0], gyr[:, 0], ba, bg, ns, np.full((n, mx), dt), acc[:, 1:], gyr[:, 1:])
    for i in range(n):
        k = int(ns[i])
        if k == 0:
            ref = np.zeros(abi.IMU_DOUBLES); ref[abi.IMU_OFF["delta_q"][0] + 3] = 1.0
            ref[abi.IMU_OFF["linearized_ba"][0]:abi.IMU_OFF["linearized_ba"][1]] = ba[i]; ref[abi.IMU_OFF["linearized_bg"][0]:abi.IMU_OFF["linearized_bg"][1]] = bg[i]
            j0 = abi.IMU_OFF["jacobian"][0]
            ref[j0:j0 + 225] = np.eye(15).ravel()
        else:
            ref = synth.preintegrate(acc[i:i + 1, :k + 1], gyr[i:i + 1, :k + 1], dt, ba[i:i + 1], bg[i:i + 1])[0]
        assert np.allclose(got[i], ref, rtol=1e-11, atol=1e-13 * max(1.0, np.abs(ref).max())), i


@pytest.mark.gpu
def test_benchmark_windows_translation_equivariance_and_cost_descent(solver, oracle, opts):
    """Size-independent properties at the benchmark's window configuration (230 features, IMU + LiDAR between-factors, no prior):
    every factor is relative, so moving the whole window by t moves the solution by t and leaves every cost unchanged; the trust-region
    solve never raises the cost; and one of the windows is checked against the oracle outright."""
    cfg = synth.SynthConfig(n_features=230, with_prior=False)
    base = [synth.make_window(300 + k, opts, cfg)[0] for k in range(4)]
    shifts = [np.zeros(3), np.array([100.0, -50.0, 7.0]), np.array([-1234.5, 987.25, -60.0])]
    wins = []
    for w in base:
        for t in shifts:
            v = copy.deepcopy(w)
            v.para_pose[:, :3] += t
            if v.gauge_P0 is not None:
                v.gauge_P0 = v.gauge_P0 + t
            wins.append(v)
    solver.batch_upload(wins, [None] * len(wins))
    solver.batch_solve()
    got = solver.batch_download()
    for k in range(len(base)):
        g0 = got[3 * k]
        assert g0.summary["final_cost"] <= g0.summary["initial_cost"]
        for j in (1, 2):
            g = got[3 * k + j]
            assert g.summary["num_iterations"] == g0.summary["num_iterations"]
            assert abs(g.summary["final_cost"] - g0.summary["final_cost"]) <= 1e-7 * g0.summary["final_cost"]
            assert np.abs((g.Ps - shifts[j]) - g0.Ps).max() < 1e-7           # metres, at |t| ~ 1.5 km: eps * |t| * condition
            assert np.abs(g.Rs - g0.Rs).max() < 1e-8 and np.abs(g.Vs - g0.Vs).max() < 1e-7
    _compare(got[0], oracle.window_solve(opts, wins[0], None))
    _compare(got[5], oracle.window_solve(opts, wins[5], None))


def test_marginalization_eigen_solver_fallback(solver, oracle, opts, monkeypatch):
    """the eigen-solver runs in three launches with a bounded rotation log; a window whose log overflows is redone by the
    single-workgroup kernel. Force that path (VILF_MARG_FORCE_QL_FALLBACK) and compare both with the oracle and with the split path."""
    wins, priors = synth.make_batch(77, 6, opts, synth.SynthConfig(n_features=120), distinct=6)
    monkeypatch.setenv("VILF_MARG_NO_CHOL", "1")            # these well-conditioned windows would take the Cholesky form of the kept block otherwise
    solver.batch_upload(wins, priors); solver.batch_solve(); solver.batch_marginalize()
    assert solver.marginalize_stats()["kept_cholesky"] == 0
    split = [_prior_products(solver.get_prior(i)) for i in range(6)]
    monkeypatch.setenv("VILF_MARG_FORCE_QL_FALLBACK", "1")
    solver.batch_upload(wins, priors); solver.batch_solve(); solver.batch_marginalize()
    for i in range(6):
        Lg, bg, _ = _prior_products(solver.get_prior(i))
        pr = oracle.window_marginalize(opts, wins[i], oracle.window_solve(opts, wins[i], priors[i]), priors[i])
        Lr, br_, _ = _prior_products(pr)
        assert np.abs(Lg - Lr).max() / np.abs(Lr).max() < 2e-5 and np.abs(bg - br_).max() / np.abs(br_).max() < 2e-5
        assert np.abs(Lg - split[i][0]).max() / np.abs(Lr).max() < 1e-9        # same arithmetic in both paths up to FMA contraction of the replay


def test_marginalization_kept_block_cholesky_form_and_its_guard(solver, oracle, opts, monkeypatch):
    """marginalize() ends in an eigen-decomposition of the kept block with a 1e-8 truncation (marginalization_factor.cpp:283-291). Where nothing is truncated
    (positive pivots and trace(A^-1) < 1e8 => lambda_min > 1e-8) the library writes J0 = L^T, r0 = L^-1 b from a Cholesky factorisation instead: same J0^T J0,
    J0^T r0 and |r0|^2, which is all the next solve / marginalization sees of a prior. Both forms against the oracle and against each other, the path counters, and
    the guard: windows without a prior leave the gauge (yaw + position) unobserved, their kept block is singular, and they must take the eigen-solver."""
    wins, priors = synth.make_batch(91, 6, opts, synth.SynthConfig(n_features=120), distinct=6)
    free, _ = synth.make_batch(92, 2, opts, synth.SynthConfig(n_features=120, with_prior=False), distinct=2)
    wins = wins + free; priors = priors + [None, None]
    out = {}
    for tag in ("chol", "eig"):
        if tag == "eig":
            monkeypatch.setenv("VILF_MARG_NO_CHOL", "1")
        solver.batch_upload(wins, priors); solver.batch_solve(); solver.batch_marginalize()
        st = solver.marginalize_stats()
        assert st["new_prior"] == 8 and st["kept_cholesky"] == (6 if tag == "chol" else 0), st
        out[tag] = [solver.get_prior(i) for i in range(8)]
    monkeypatch.delenv("VILF_MARG_NO_CHOL")
    for i in range(8):
        pr = oracle.window_marginalize(opts, wins[i], oracle.window_solve(opts, wins[i], priors[i]), priors[i])
        Lr, br_, blr = _prior_products(pr)
        J0r, r0r, _ = abi.prior_to_numpy(pr)
        for tag in ("chol", "eig"):
            pg = out[tag][i]
            Lg, bg, blg = _prior_products(pg)
            assert pg.n == pr.n and [b["id"] for b in blg] == [b["id"] for b in blr] and [b["idx"] for b in blg] == [b["idx"] for b in blr]
            for a, b in zip(blg, blr):
                assert np.allclose(a["x0"], b["x0"], atol=1e-9)
            assert np.abs(Lg - Lr).max() / np.abs(Lr).max() < 2e-5 and np.abs(bg - br_).max() / np.abs(br_).max() < 2e-5, (tag, i)
        if i < 6:
            J0, r0, _ = abi.prior_to_numpy(out["chol"][i])
            assert np.allclose(J0, np.triu(J0)) and (np.diag(J0) > 0).all(), "J0 = L^T is upper triangular"
            assert abs(r0 @ r0 - r0r @ r0r) <= 1e-6 * (r0r @ r0r), "|r0|^2 = b^T A^-1 b in both forms"
            Lc, bc, _ = _prior_products(out["chol"][i]); Le, be, _ = _prior_products(out["eig"][i])
            assert np.abs(Lc - Le).max() / np.abs(Le).max() < 2e-5 and np.abs(bc - be).max() / np.abs(be).max() < 2e-5
        else:
            assert bytes(out["chol"][i]) == bytes(out["eig"][i]), "a window that fails the guard goes through the same eigen-solver in both runs"


@pytest.mark.parametrize("n_frames,n_features,tol", [(21, 400, 1e-7), (51, 2500, 1e-6)])
def test_large_window_solve_matches_oracle(oracle, n_frames, n_features, tol):
    """BASELINE configs[4]: the synthetic 51-frame / ~50 k-factor stress window (reduced system 765 x 765) — and a 21-frame one — through
    vilf_window_solve's general path (one window spread over the device: factor lanes with fp64 atomics, MFMA SYRK Schur reduce,
    the path's own blocked Cholesky, trust-region loop on the device) against the oracle. The atomics' summation order is free: tolerances, not bits."""
    from vil_fusion_amd.estimator import BackendSolver
    o = oracle.default_options()
    o.window_size = n_frames - 1
    cfg = synth.SynthConfig(n_frames=n_frames, n_features=n_features, with_prior=False)
    win, _, _ = synth.make_window(60 + n_frames, o, cfg)
    nfac = len(win.obs_point) - win.n_features
    assert nfac > (40000 if n_frames == 51 else 3000)
    ref = oracle.window_solve(o, win, None)
    s = BackendSolver(o)
    got = s.optimization(win)
    s.close()
    assert got.summary["num_iterations"] == ref.summary["num_iterations"] and got.summary["num_successful_steps"] == ref.summary["num_successful_steps"]
    assert abs(got.summary["initial_cost"] - ref.summary["initial_cost"]) <= 1e-9 * ref.summary["initial_cost"]
    assert abs(got.summary["final_cost"] - ref.summary["final_cost"]) <= 1e-6 * ref.summary["final_cost"]
    assert np.abs(got.Ps - ref.Ps).max() < tol and np.abs(got.Rs - ref.Rs).max() < tol and np.abs(got.Vs - ref.Vs).max() < 10 * tol
    assert np.abs(1.0 / got.para_feature - 1.0 / ref.para_feature).max() < 1e-4


def test_window_solve_group_matches_the_oracle_window_by_window(oracle, monkeypatch):
    """vilf_window_solve_group: windows of DIFFERENT sizes (13 / 21 / 16 / 26 / 14 / 15 frames; two picked for their rejected steps, one with every feature constant, one with three features) in one
    chain of launches — every kernel finds its window in blockIdx.z, grids are sized for the largest, the blocked Cholesky runs as many block columns as the largest needs.
    Each window against the oracle with the counts and tolerances of the single-window tests; then the same group with one window forced through the host-loop fallback."""
    from vil_fusion_amd.estimator import BackendSolver
    o = oracle.default_options()
    cases = [(13, 60, 502, (3.0, np.deg2rad(25.0), 3.0), {}), (21, 400, 81, None, {}), (16, 150, 82, None, {}), (26, 700, 83, None, {}), (13, 60, 500, (1.5, np.deg2rad(15.0), 1.5), {}),
             (14, 40, 84, None, {"const_fraction": 1.0}), (15, 3, 85, None, {"const_fraction": 0.0})]      # + every feature constant (no Schur block), + three features
    wins, refs = [], []
    for nf, nfeat, seed, noise, extra in cases:
        oo = oracle.default_options(); oo.window_size = nf - 1
        cfg = synth.SynthConfig(n_frames=nf, n_features=nfeat, with_prior=False, **({"state_noise": noise} if noise else {}), **extra)
        w, _, _ = synth.make_window(seed, oo, cfg)
        wins.append(w); refs.append(oracle.window_solve(oo, w, None))
    assert refs[0].summary["num_successful_steps"] < refs[0].summary["num_iterations"], "one window of the group has rejected steps"
    o.window_size = 12                      # a group takes every window's own n_frames (vilf_window_solve insists on options.window_size + 1)
    s = BackendSolver(o)
    got = s.optimization_group(wins)
    single = []
    for w in wins:
        oo = oracle.default_options(); oo.window_size = w.n_frames - 1
        s1 = BackendSolver(oo); single.append(s1.optimization(w)); s1.close()
    monkeypatch.setenv("VILF_LW_FORCE_FALLBACK", "1")
    fb = s.optimization_group(wins[:2])
    monkeypatch.delenv("VILF_LW_FORCE_FALLBACK")
    s.close()
    for k, (g, r) in enumerate(zip(got + fb, refs + refs[:2])):
        for key in ("num_iterations", "num_successful_steps", "num_linear_solves", "termination"):
            assert g.summary[key] == r.summary[key], (k, key)
        loose = k in (0, 4, 7)              # the ill-conditioned 13-frame windows (7 = window 0 again, in the fallback group): tolerances of test_large_window_device_trust_region_loop
        assert abs(g.summary["initial_cost"] - r.summary["initial_cost"]) <= 1e-9 * r.summary["initial_cost"]
        assert abs(g.summary["final_cost"] - r.summary["final_cost"]) <= (1e-4 if loose else 1e-6) * r.summary["final_cost"]
        tol = 1e-4 if loose else 1e-7
        assert np.abs(g.Ps - r.Ps).max() < tol and np.abs(g.Rs - r.Rs).max() < tol and np.abs(g.Vs - r.Vs).max() < 10 * tol, k
    for g, one in zip(got, single):         # a group of one is the same code, and since round 4 no sum on this path depends on an order the hardware picks: bit for bit
        assert g.summary["num_iterations"] == one.summary["num_iterations"]
        for key in ("Ps", "Rs", "Vs", "Bas", "Bgs", "para_feature"):
            assert np.array_equal(getattr(g, key), getattr(one, key)), key
        assert g.summary["final_cost"] == one.summary["final_cost"] and g.summary["initial_cost"] == one.summary["initial_cost"]


def test_general_path_is_bit_reproducible(oracle):
    """The general path (vilf_lw.hip) without atomics: the feature rows of W / h_f / g_f by wave sums in a fixed tree (lw_feature_rows), the pose-pose blocks through
    host-assigned slots summed in slot order (lw_visual -> lw_assemble), the IMU / LiDAR blocks by one writer per entry (frame-major lw_imu_lidar), the Schur
    reduce's K-split partials summed in split order (lw_syrk_mfma -> lw_schur_prep), the cost from per-workgroup partials in slot order (tr_cost_sum). A 31-frame /
    1500-feature window solved three times alone and once inside a group of three: every output bit equal."""
    from vil_fusion_amd.estimator import BackendSolver
    o = oracle.default_options(); o.window_size = 30
    w, _, _ = synth.make_window(321, o, synth.SynthConfig(n_frames=31, n_features=1500, with_prior=False))
    o2 = oracle.default_options(); o2.window_size = 20
    w2, _, _ = synth.make_window(322, o2, synth.SynthConfig(n_frames=21, n_features=400, with_prior=False))
    s = BackendSolver(o)
    runs = [s.optimization(w) for _ in range(3)]
    grp = s.optimization_group([w2, w, w2])
    s.close()
    ref = oracle.window_solve(o, w, None)
    assert runs[0].summary["num_iterations"] == ref.summary["num_iterations"] and np.abs(runs[0].Ps - ref.Ps).max() < 1e-6
    for other in runs[1:] + [grp[1]]:
        for key in ("Ps", "Rs", "Vs", "Bas", "Bgs", "para_feature", "para_pose", "para_speed_bias"):
            assert np.array_equal(getattr(runs[0], key), getattr(other, key)), key
        for key in ("initial_cost", "final_cost", "final_radius", "num_iterations", "num_successful_steps"):
            assert runs[0].summary[key] == other.summary[key], key
    assert np.array_equal(grp[0].Ps, grp[2].Ps)


def test_feature_rows_four_per_wave_give_the_same_bits_as_a_wave_per_feature(oracle, monkeypatch):
    """lw_feature_rows deals FOUR features to a wave (16 lanes each) for windows of up to 17 frames — a track has at most 16 factors there — and a wave per feature
    otherwise; the 16-lane sums are the first four stages of the wave sum's tree, so a 13-frame window must come out bit for bit the same through both
    (VILF_LW_FEATURE_WAVES=1 forces the wave-per-feature form)."""
    from vil_fusion_amd.estimator import BackendSolver
    o = oracle.default_options()
    o.window_size = 12
    win, _, _ = synth.make_window(611, o, synth.SynthConfig(n_frames=13, n_features=150, with_prior=False))
    def run():
        s = BackendSolver(o)
        try:
            return s.optimization(win)
        finally:
            s.close()
    a = run()
    monkeypatch.setenv("VILF_LW_FEATURE_WAVES", "1")
    b = run()
    for key in ("Ps", "Rs", "Vs", "Bas", "Bgs", "para_feature", "para_pose", "para_speed_bias"):
        assert np.array_equal(getattr(a, key), getattr(b, key)), key
    for key in ("initial_cost", "final_cost", "final_radius", "num_iterations", "num_successful_steps"):
        assert a.summary[key] == b.summary[key], key
    ref = oracle.window_solve(o, win, None)
    assert a.summary["num_iterations"] == ref.summary["num_iterations"] and np.abs(a.Ps - ref.Ps).max() < 1e-6


@pytest.mark.parametrize("noise,deg,seed", [(1.5, 15.0, 500), (3.0, 25.0, 502), (3.0, 25.0, 503)])
def test_large_window_device_trust_region_loop(oracle, monkeypatch, noise, deg, seed):
    """The general single-window path keeps its trust-region loop on the device (lw_tr_*: every iteration enqueued at once, skip flags instead of host decisions).
    13-frame windows picked with the oracle for REJECTED steps and re-used Gauss-Newton steps: same iteration / accepted-step / linear-solve counts as the oracle; the
    host loop (VILF_LW_HOST_LOOP, also the path a failed factorisation falls back to: VILF_LW_FORCE_FALLBACK) gives the same counts and the same state."""
    from vil_fusion_amd.estimator import BackendSolver
    o = oracle.default_options()
    o.window_size = 12
    win, _, _ = synth.make_window(seed, o, synth.SynthConfig(n_frames=13, n_features=60, with_prior=False, state_noise=(noise, np.deg2rad(deg), noise)))
    ref = oracle.window_solve(o, win, None)
    assert ref.summary["num_successful_steps"] < ref.summary["num_iterations"], "the case was picked for its rejected steps"
    def run():
        s = BackendSolver(o)
        try:
            return s.optimization(win)
        finally:
            s.close()
    dev = run()
    monkeypatch.setenv("VILF_LW_HOST_LOOP", "1")
    host = run()
    monkeypatch.delenv("VILF_LW_HOST_LOOP")
    monkeypatch.setenv("VILF_LW_FORCE_FALLBACK", "1")
    fb = run()
    for got in (dev, host, fb):
        for k in ("num_iterations", "num_successful_steps", "num_linear_solves", "termination"):
            assert got.summary[k] == ref.summary[k], k
        assert abs(got.summary["initial_cost"] - ref.summary["initial_cost"]) <= 1e-9 * ref.summary["initial_cost"]
        assert abs(got.summary["final_cost"] - ref.summary["final_cost"]) <= 1e-4 * ref.summary["final_cost"]
        assert np.abs(got.Ps - ref.Ps).max() < 1e-4 and np.abs(got.Rs - ref.Rs).max() < 1e-5 and np.abs(got.Vs - ref.Vs).max() < 1e-3
    # (the factor lanes add with fp64 atomics: two runs of the same loop differ in the last bits, amplified by these ill-conditioned windows)
    for other in (host, fb):
        assert np.abs(dev.Ps - other.Ps).max() < 1e-5 and abs(dev.summary["final_radius"] - other.summary["final_radius"]) <= 1e-6 * other.summary["final_radius"]


def test_frame_without_host_round_trips_between_its_stages(oracle, opts):
    """One handle per stage, as INTEGRATION.md wires them: the LiDAR stage is enqueued asynchronously on its handle, the solver's stream takes a device-side dependency
    on it (vilf_wait_for), solve + marginalization are enqueued asynchronously too and the host waits once. Profiling stays on: the per-kernel spans of asynchronous calls
    are read by the next call that waits for the stream. Same results as the synchronous calls, and every profiled group has its launches."""
    from vil_fusion_amd.estimator import BackendSolver, Scan2MapBatch
    me, ms, scans, pl = synth.make_lidar_bench_case(7000)
    wins, priors = synth.make_batch(41, 6, opts, synth.SynthConfig(n_features=80), distinct=6)
    def run(asynchronous):
        solver, lidar = BackendSolver(opts), BackendSolver(opts)
        try:
            b = Scan2MapBatch(lidar, 2, len(scans[0][0]) + 64, len(scans[0][1]) + 64, len(me) + len(scans[0][0]) + 64, len(ms) + len(scans[0][1]) + 64)
            for i in range(2):
                b.localMapInited(i, me, ms, None, pl)
                b.set_scan(i, *scans[0])
            solver.batch_upload(wins, priors)
            solver.set_profiling(True); lidar.set_profiling(True)
            for _ in range(2):                                   # twice: the second frame reuses the event pool
                b.snapshot() if _ == 0 else b.rewind()
                b.step(sync=not asynchronous)
                if asynchronous:
                    solver.wait_for(lidar)
                solver.batch_rewind()
                solver.batch_solve(sync=not asynchronous)
                solver.batch_marginalize(sync=not asynchronous)
                solver.synchronize(); lidar.synchronize()
            prof = (solver.get_profile(), solver.get_profile_marginalize(), lidar.get_profile_scan2map())
            poses = [np.array(r.pose_qt[:]) for r in b.results()]
            return solver.batch_download(), [solver.get_prior(i) for i in range(6)], poses, prof
        finally:
            solver.close(); lidar.close()
    res_s, pri_s, pose_s, prof_s = run(False)
    res_a, pri_a, pose_a, prof_a = run(True)
    for a, b_ in zip(res_a, res_s):
        assert np.array_equal(a.Ps, b_.Ps) and np.array_equal(a.para_feature, b_.para_feature)
    for a, b_ in zip(pri_a, pri_s):
        assert np.array_equal(_prior_products(a)[0], _prior_products(b_)[0])
    for a, b_ in zip(pose_a, pose_s):
        assert np.array_equal(a, b_)
    for pa, ps in zip(prof_a, prof_s):
        assert {k: v["launches"] for k, v in pa.items()} == {k: v["launches"] for k, v in ps.items()}
        assert all(v["ms"] > 0 for v in pa.values() if v["launches"] > 0)
    assert prof_a[0]["k_linearize"]["launches"] > 0 and prof_a[1]["k_marg_prepare"]["launches"] == 2 and prof_a[2]["s2m_associate"]["launches"] > 0


def test_error_behaviour_of_the_newer_entry_points(solver, oracle, opts):
    """loud failures instead of silent fall-backs: a pose graph without a complete odometry chain, an edge to a missing node, a non-positive
    sigma; a window whose frame count does not match options.window_size; a batched call with a non-11-frame window"""
    from vil_fusion_amd.estimator import posegraph_optimize
    from vil_fusion_amd.lib import VilfError
    from vil_fusion_amd import posegraph
    truth, x0, edges = posegraph.make_synthetic_graph(1, 8)
    ps = np.full(6, 1e-6)
    with pytest.raises(VilfError, match="no odometry edge"):
        posegraph_optimize(solver, x0, ps, edges[:3] + edges[4:])
    bad = list(edges); i, j, q, t, sg, rb = bad[0]; bad[0] = (i, 99, q, t, sg, rb)
    with pytest.raises(VilfError, match="out of range"):
        posegraph_optimize(solver, x0, ps, bad)
    bad = list(edges); bad[1] = (bad[1][0], bad[1][1], bad[1][2], bad[1][3], np.array([1e-3, 1e-3, 0.0, 1e-2, 1e-2, 1e-2]), 0)
    with pytest.raises(VilfError, match="sigma"):
        posegraph_optimize(solver, x0, ps, bad)
    # 21-frame window handed to a handle configured for the reference's WINDOW_SIZE = 10
    o21 = oracle.default_options(); o21.window_size = 20
    win21, _, _ = synth.make_window(3, o21, synth.SynthConfig(n_frames=21, n_features=60, with_prior=False))
    with pytest.raises(VilfError, match="window_size"):
        solver.optimization(win21)
    with pytest.raises(VilfError):
        solver.batch_upload([win21], [None])


def _with_td_inputs(win, seed, td_true=0.004):
    """ProjectionTdFactor inputs for a synthetic window: pixel velocities on the normalised plane, zero per-observation td, image rows;
    the observations are shifted as a camera running `td_true` seconds late would have seen them."""
    rng = np.random.default_rng(seed)
    vel = rng.normal(0.0, 0.4, (win.n_obs, 2))
    pts = win.obs_point.copy()
    pts[:, :2] += td_true * vel
    return abi.Window(win.para_pose, win.para_speed_bias, win.para_ex_pose, win.para_feature, win.feature_const, win.feature_start_frame,
                      win.feature_obs_offset, pts, win.imu, win.lidar, para_td=0.0, marginalization_flag=win.marginalization_flag,
                      obs_velocity=vel, obs_cur_td=np.zeros(win.n_obs), obs_row=rng.uniform(0.0, 370.0, win.n_obs))


def test_estimate_td_batch_continues_from_the_resident_state_and_async_solve_time(oracle):
    """Like the batched LDS kernels, the estimate_td slots (general path, one group of launches) solve from the RESIDENT state: a second vilf_batch_solve without a
    rewind starts where the first ended (its initial cost = the first's final cost), a rewind restores the uploaded state. And: a solve enqueued with sync = 0
    reports its own device time through the next call that waits for the stream (usec_solve was stale there)."""
    from vil_fusion_amd.estimator import BackendSolver
    o = oracle.default_options(); o.estimate_td = 1
    cfg = synth.SynthConfig(with_prior=False, n_features=100)
    wins = [_with_td_inputs(synth.make_window(70 + k, o, cfg)[0], 30 + k) for k in range(3)]
    s = BackendSolver(o)
    s.batch_upload(wins, None)
    s.batch_solve(); s1 = s.batch_summaries()
    s.batch_solve(); s2 = s.batch_summaries()
    s.batch_rewind(); s.batch_solve(); s3 = s.batch_summaries()
    s.close()
    for a, b, c in zip(s1, s2, s3):
        assert abs(b.initial_cost - a.final_cost) <= 1e-9 * a.final_cost and b.final_cost <= a.final_cost * (1 + 1e-12)
        assert abs(c.initial_cost - a.initial_cost) <= 1e-12 * a.initial_cost and c.num_iterations == a.num_iterations
    p = BackendSolver(oracle.default_options())
    pw, pp = synth.make_batch(11, 4, oracle.default_options(), synth.SynthConfig(n_features=80), distinct=4)
    p.batch_upload(pw, pp)
    p.batch_solve(sync=True); t_sync = p.batch_summaries()[0].usec_solve
    p.batch_rewind(); p.batch_solve(sync=False); t_async = p.batch_summaries()[0].usec_solve
    p.close()
    assert t_sync > 0 and t_async > 0 and 0.3 < t_async / t_sync < 3.0, (t_sync, t_async)


def _perturbed_extrinsic(win, seed):
    rng = np.random.default_rng(seed)
    ex = win.para_ex_pose.copy()
    ex[:3] += rng.normal(0.0, 0.01, 3)
    ex[3:] = synth.q_mul(ex[3:], synth.q_exp(rng.normal(0.0, np.deg2rad(0.3), 3)))
    win.para_ex_pose = ex / np.concatenate([np.ones(3), np.full(4, np.linalg.norm(ex[3:]))])
    return win


@pytest.mark.parametrize("n_frames,est_ex,est_td,with_prior", [(11, 1, 0, True), (11, 0, 1, False), (11, 1, 1, False), (6, 1, 1, False)])
def test_extrinsic_and_td_estimation_match_oracle(oracle, n_frames, est_ex, est_td, with_prior):
    """estimate_extrinsic / estimate_td (estimator.cpp:701-717, 765-777; off in the KITTI configuration): Ex_Pose and td as variables of the
    window solve, ProjectionTdFactor instead of ProjectionFactor — through vilf_window_solve's general single-window path, with the
    marginalization prior for an 11-frame window. Against the oracle's solve of the same problem."""
    from vil_fusion_amd.estimator import BackendSolver
    o = oracle.default_options()
    o.window_size = n_frames - 1
    o.estimate_extrinsic, o.estimate_td = est_ex, est_td
    cfg = synth.SynthConfig(n_frames=n_frames, n_features=120, with_prior=with_prior)
    win, prior, _ = synth.make_window(70 + n_frames + est_td, o, cfg)
    if est_td:
        win = _with_td_inputs(win, 5)
    if est_ex:
        win = _perturbed_extrinsic(win, 6)
    s = BackendSolver(o)
    s.set_prior(prior if with_prior else None)
    got = s.optimization(win)
    ref = oracle.window_solve(o, win, prior if with_prior else None)
    s.close()
    assert got.summary["num_iterations"] == ref.summary["num_iterations"] and got.summary["num_successful_steps"] == ref.summary["num_successful_steps"]
    assert abs(got.summary["initial_cost"] - ref.summary["initial_cost"]) <= 1e-9 * ref.summary["initial_cost"]
    assert abs(got.summary["final_cost"] - ref.summary["final_cost"]) <= 1e-6 * ref.summary["final_cost"]
    assert np.abs(got.Ps - ref.Ps).max() < 1e-6 and np.abs(got.Rs - ref.Rs).max() < 1e-7 and np.abs(got.Vs - ref.Vs).max() < 1e-5
    assert np.abs(got.tic - ref.tic).max() < 1e-6 and np.abs(got.ric - ref.ric).max() < 1e-7 and abs(got.td - ref.td) < 1e-7
    if est_ex:
        assert np.abs(got.tic - win.para_ex_pose[:3]).max() > 1e-5, "the extrinsic must have moved"
    if est_td:
        assert abs(got.td) > 1e-4, "td must have moved"


def test_extrinsic_estimation_solve_marginalize_solve_chain(oracle):
    """estimate_extrinsic = 1 over two frames: solve (general path) -> device marginalization (Ex_Pose is a kept block whose linearisation
    point is the estimated extrinsic) -> next solve with that prior, Ex_Pose columns of the prior active."""
    from vil_fusion_amd.estimator import BackendSolver
    o = oracle.default_options()
    o.estimate_extrinsic = 1
    cfg = synth.SynthConfig(with_prior=True, n_features=100)      # the synthetic prior pins the (weakly observable) extrinsic
    win, prior0, _ = synth.make_window(33, o, cfg)
    win = _perturbed_extrinsic(win, 7)
    s = BackendSolver(o)
    s.set_prior(prior0)
    got1 = s.optimization(win)
    s.marginalize()
    pg = s.get_prior()
    ref1 = oracle.window_solve(o, win, prior0)
    pr = oracle.window_marginalize(o, win, ref1, prior0)
    assert pg.valid == pr.valid and pg.n == pr.n and pg.n_blocks == pr.n_blocks
    Lg, bg, blg = _prior_products(pg)
    Lr, br_, blr = _prior_products(pr)
    assert [b["id"] for b in blg] == [b["id"] for b in blr]
    assert np.abs(Lg - Lr).max() / np.abs(Lr).max() < 2e-5 and np.abs(bg - br_).max() / np.abs(br_).max() < 2e-5
    win2, _, _ = synth.make_window(33, o, cfg)
    win2.para_ex_pose = np.concatenate([got1.tic, synth.R_to_q(got1.ric)])
    got2 = s.optimization(win2)
    ref2 = oracle.window_solve(o, win2, pr)
    s.set_prior(pr)                                   # the same solve from the ORACLE's prior: isolates the solve from the two eigen-solvers' 2e-5
    got3 = s.optimization(win2)
    s.close()
    assert got2.summary["num_iterations"] == ref2.summary["num_iterations"] == got3.summary["num_iterations"]
    assert abs(got2.summary["final_cost"] - ref2.summary["final_cost"]) <= 1e-5 * ref2.summary["final_cost"]
    # the extrinsic is weakly observable over one window: the priors' 2e-5 relative difference shows as a few 1e-5 m along the window
    assert np.abs(got2.Ps - ref2.Ps).max() < 1e-4 and np.abs(got2.Rs - ref2.Rs).max() < 1e-5 and np.abs(got2.tic - ref2.tic).max() < 1e-4
    assert np.abs(got3.Ps - ref2.Ps).max() < 1e-6 and np.abs(got3.Rs - ref2.Rs).max() < 1e-7 and np.abs(got3.tic - ref2.tic).max() < 1e-6


@pytest.mark.parametrize("est_ex", [0, 1])
def test_td_estimation_solve_marginalize_solve_chain_single_and_batched(oracle, est_ex):
    """estimate_td = 1 (ProjectionTdFactor, estimator.cpp:713-717,772-777) through a frame chain: solve -> device marginalization (td is a kept block of the new
    prior, the dropped features' factors are ProjectionTdFactors: :930-935,968-969) -> next solve with that prior; through vilf_window_solve and through the batched
    entry points (several windows, different seeds), against the oracle."""
    from vil_fusion_amd.estimator import BackendSolver
    from vil_fusion_amd.lib import VilfError
    o = oracle.default_options()
    o.estimate_td = 1; o.estimate_extrinsic = est_ex
    cfg = synth.SynthConfig(with_prior=bool(est_ex), n_features=100)
    s = BackendSolver(o)
    plain, _, _ = synth.make_window(2, o, cfg)
    with pytest.raises(VilfError):                       # td factor constants missing
        s.optimization(plain)
    made = [synth.make_window(60 + k, o, cfg) for k in range(3)]
    wins = [_with_td_inputs(m[0], 10 + k) for k, m in enumerate(made)]
    if est_ex:
        wins = [_perturbed_extrinsic(w, 20 + k) for k, w in enumerate(wins)]
    priors = [m[1] if est_ex else None for m in made]
    # single window
    s.set_prior(priors[0])
    got1 = s.optimization(wins[0])
    ref1 = oracle.window_solve(o, wins[0], priors[0])
    assert got1.summary["num_iterations"] == ref1.summary["num_iterations"]
    assert np.abs(got1.Ps - ref1.Ps).max() < 1e-6 and abs(got1.td - ref1.td) < 1e-7
    s.marginalize()
    pg = s.get_prior()
    pr = oracle.window_marginalize(o, wins[0], ref1, priors[0])
    assert pg.valid == pr.valid and pg.n == pr.n and pg.n_blocks == pr.n_blocks
    Lg, bg, blg = _prior_products(pg)
    Lr, br_, blr = _prior_products(pr)
    assert [b["id"] for b in blg] == [b["id"] for b in blr] and 23 in [b["id"] for b in blg]          # block 23 = para_Td
    assert np.abs(Lg - Lr).max() / np.abs(Lr).max() < 2e-5 and np.abs(bg - br_).max() / np.abs(br_).max() < 2e-5
    win2 = _with_td_inputs(synth.make_window(60, o, cfg)[0], 10)
    win2.para_td = got1.td
    if est_ex:
        win2.para_ex_pose = np.concatenate([got1.tic, synth.R_to_q(got1.ric)])
    s.set_prior(pr)                                   # the solve from the ORACLE's prior: isolates it from the two eigen-solvers' 2e-5
    got2 = s.optimization(win2)
    ref2 = oracle.window_solve(o, win2, pr)
    assert got2.summary["num_iterations"] == ref2.summary["num_iterations"]
    assert np.abs(got2.Ps - ref2.Ps).max() < 1e-6 and np.abs(got2.Rs - ref2.Rs).max() < 1e-7 and abs(got2.td - ref2.td) < 1e-7
    # batched entry points: upload / solve / marginalize / download of three windows
    s.batch_upload(wins, priors)
    s.batch_solve()
    res = s.batch_download()
    s.batch_marginalize()
    for k in range(3):
        ref = oracle.window_solve(o, wins[k], priors[k])
        assert res[k].summary["num_iterations"] == ref.summary["num_iterations"]
        assert np.abs(res[k].Ps - ref.Ps).max() < 1e-6 and abs(res[k].td - ref.td) < 1e-7
        pgk = s.get_prior(k)
        prk = oracle.window_marginalize(o, wins[k], ref, priors[k])
        Lg, bg, blg = _prior_products(pgk)
        Lr, br_, blr = _prior_products(prk)
        assert [b["id"] for b in blg] == [b["id"] for b in blr]
        assert np.abs(Lg - Lr).max() / np.abs(Lr).max() < 2e-5 and np.abs(bg - br_).max() / np.abs(br_).max() < 2e-5
    s.close()


# ---- round 2: speed-bias-first solve kernel, boundary behaviour --------------------------------------------------------------------------------
def test_speed_bias_first_kernel_equals_dense_kernel_and_oracle(solver, oracle, opts, monkeypatch):
    """k_solve_sb (block-tridiagonal speed-bias chain eliminated first) against k_solve (Cholesky of the whole 165 x 165 system, VILF_SOLVE_DENSE=1) and the
    oracle: the same iterations / accepted steps / linear solves in every window, states equal to rounding; windows with and without a prior, with constant
    features only, strongly perturbed."""
    cfgs = [synth.SynthConfig(n_features=230), synth.SynthConfig(n_features=90, with_prior=False), synth.SynthConfig(const_fraction=1.0, n_features=40),
            synth.SynthConfig(n_features=150, state_noise=(0.5, np.deg2rad(5.0), 0.5)), synth.SynthConfig(n_features=3, const_fraction=0.0)]
    made = [synth.make_window(300 + i, opts, c) for i, c in enumerate(cfgs)]
    wins, priors = [m[0] for m in made], [m[1] for m in made]

    def run():
        solver.batch_upload(wins, priors); solver.batch_solve()
        return solver.batch_download(), solver.batch_summaries()
    monkeypatch.delenv("VILF_SOLVE_DENSE", raising=False)
    r_sb, s_sb = run()
    monkeypatch.setenv("VILF_SOLVE_DENSE", "1")
    r_de, s_de = run()
    monkeypatch.delenv("VILF_SOLVE_DENSE")
    for i in range(len(wins)):
        a, b = s_sb[i], s_de[i]
        assert (a.num_iterations, a.num_successful_steps, a.num_linear_solves, a.termination) == (b.num_iterations, b.num_successful_steps, b.num_linear_solves, b.termination)
        assert np.abs(r_sb[i].Ps - r_de[i].Ps).max() < 1e-8 and np.abs(r_sb[i].Vs - r_de[i].Vs).max() < 1e-7
        _compare(r_sb[i], oracle.window_solve(opts, wins[i], priors[i]), tol_p=1e-6, tol_r=1e-7, tol_cost=1e-6)


def test_prior_with_other_speed_bias_blocks_takes_the_dense_kernel(oracle, opts):
    """the chain elimination assumes SpeedBias[0] is the only speed-bias block of the prior (all the reference ever produces); an imported prior that also holds
    SpeedBias[3] must still be solved correctly — the handle switches to the dense kernel"""
    from vil_fusion_amd.estimator import BackendSolver
    win, prior, _ = synth.make_window(41, opts, synth.SynthConfig(n_features=80))
    rng = np.random.default_rng(3)
    n = 6 * 3 + 9 * 2
    p = abi.Prior()
    p.valid = 1; p.n = n; p.m = 0; p.n_blocks = 5
    ids, sizes = [2, 4, 7, 11, 14], [7, 7, 7, 9, 9]         # three poses, SpeedBias[0], SpeedBias[3]
    idx = 0
    for k, (bid, sz) in enumerate(zip(ids, sizes)):
        p.block_id[k] = bid; p.block_size[k] = sz; p.block_idx[k] = idx
        x0 = win.para_pose[bid] if bid < 11 else win.para_speed_bias[bid - 11]
        for q in range(sz):
            p.block_x0[k][q] = x0[q]
        idx += 6 if sz == 7 else sz
    J = rng.normal(0, 3.0, (n, n)); r = rng.normal(0, 0.1, n)
    for i in range(n):
        p.linearized_residuals[i] = r[i]
        for j in range(n):
            p.linearized_jacobians[i * n + j] = J[i, j]
    s = BackendSolver(opts)
    s.set_prior(p)
    got = s.optimization(win)
    _compare(got, oracle.window_solve(opts, win, p), tol_p=1e-6, tol_r=1e-7, tol_cost=1e-6)
    s.close()


def test_max_solver_time_is_honoured(oracle):
    """options.max_solver_time (estimator.cpp:847-850): a limit that has already passed stops the solve at the top of the first iteration (state = initial state,
    NO_CONVERGENCE, like Ceres); a generous limit changes nothing"""
    from vil_fusion_amd.estimator import BackendSolver
    o = oracle.default_options()
    win, prior, _ = synth.make_window(5, o, synth.SynthConfig(n_features=60))
    o.max_solver_time = 1e-9
    s = BackendSolver(o); s.set_prior(prior)
    got = s.optimization(win)
    assert got.summary["num_iterations"] == 0 and got.summary["termination"] == 0    # VILF_TERM_NO_CONVERGENCE
    assert np.allclose(got.para_pose, win.para_pose, atol=0, rtol=0)
    s.close()
    o.max_solver_time = 100.0
    s = BackendSolver(o); s.set_prior(prior)
    got = s.optimization(win)
    o.max_solver_time = -1.0
    _compare(got, oracle.window_solve(o, win, prior))
    s.close()


def test_cauchy_scale_other_than_one_on_both_paths(oracle):
    """CauchyLoss(a), a != 1 (the reference uses 1.0, estimator.cpp:694): b = a^2 in rho(s) = b log(1 + s / b) on the batched AND the general path"""
    from vil_fusion_amd.estimator import BackendSolver
    o = oracle.default_options()
    o.cauchy_a = 0.5
    win, prior, _ = synth.make_window(6, o, synth.SynthConfig(n_features=60))
    s = BackendSolver(o); s.set_prior(prior)
    _compare(s.optimization(win), oracle.window_solve(o, win, prior))
    s.close()
    o6 = oracle.default_options(); o6.cauchy_a = 0.5; o6.window_size = 5
    win6, _, _ = synth.make_window(7, o6, synth.SynthConfig(n_frames=6, n_features=50, with_prior=False))
    s = BackendSolver(o6)
    _compare(s.optimization(win6), oracle.window_solve(o6, win6, None), tol_p=1e-6, tol_r=1e-7, tol_cost=1e-6)
    s.close()


def test_malformed_inputs_are_rejected(solver, opts):
    """the ABI never aborts: an observation CSR that does not cover [0, n_obs) and a prior block table outside [0, n) return INVALID_ARGUMENT"""
    from vil_fusion_amd.lib import VilfError
    win, prior, _ = synth.make_window(8, opts, synth.SynthConfig(n_features=20))
    bad = copy.deepcopy(win)
    bad.feature_obs_offset = bad.feature_obs_offset.copy(); bad.feature_obs_offset[-1] += 3
    with pytest.raises(VilfError):
        solver.batch_upload([bad], [None])
    bad = copy.deepcopy(win)
    bad.feature_obs_offset = bad.feature_obs_offset.copy(); bad.feature_obs_offset[0] = 1
    with pytest.raises(VilfError):
        solver.batch_upload([bad], [None])
    p = copy.deepcopy(prior)
    p.block_idx[p.n_blocks - 1] = p.n - 2
    with pytest.raises(VilfError):
        solver.set_prior(p)
    solver.set_prior(None)


def test_state_download_equals_the_full_download(solver, opts):
    """vilf_batch_download_states (Ps / Rs / Vs / Bas / Bgs + summaries into contiguous arrays, the per-frame download) against vilf_batch_download"""
    wins, priors = synth.make_batch(9, 7, opts, synth.SynthConfig(n_features=60), distinct=7)
    solver.batch_upload(wins, priors); solver.batch_solve()
    full = solver.batch_download()
    st = solver.batch_download_states(first=2, n=4)
    for i in range(4):
        r = full[2 + i]
        assert np.array_equal(st["Ps"][i], r.Ps) and np.array_equal(st["Rs"][i], r.Rs) and np.array_equal(st["Vs"][i], r.Vs)
        assert np.array_equal(st["Bas"][i], r.Bas) and np.array_equal(st["Bgs"][i], r.Bgs)
        assert st["summaries"][i].num_iterations == r.summary["num_iterations"] and st["summaries"][i].final_cost == r.summary["final_cost"]


def test_double2vector_euler_singular_branch_and_gauge_override(solver, oracle, opts):
    """double2vector's two rarely taken branches (estimator.cpp:549-596), HIP (k_finalize) vs oracle:
    (i) frame-0 pitch within 1 degree of +-90: rot_diff = Rs[0] * R(para_Pose[0])^T instead of the yaw-only rotation (:567-574) — a window from a
        drive that climbs at 89.6 / -89.5 degrees; asserted that the oracle's own R2ypr sees the singular pitch before AND after the solve, and that
        the result differs from what the yaw-only branch would give (so the branch was really taken);
    (ii) vilf_window_in.gauge_R0 / gauge_P0 (the failure_occur override, :554-559): the window is re-gauged to a frame-0 pose that is NOT the
        pre-solve one."""
    from vil_fusion_amd import sequence
    for seed, pitch in ((11, np.deg2rad(89.6)), (12, np.deg2rad(-89.5))):
        win, prior, _ = synth.make_window(seed, opts, synth.SynthConfig(n_features=120, pitch_offset=pitch))
        solver.set_prior(prior)
        got = solver.optimization(win)
        ref = oracle.window_solve(opts, win, prior)
        p_before = sequence.R2ypr(synth.q_to_R(win.para_pose[0, 3:]))[1]
        p_after = sequence.R2ypr(synth.q_to_R(ref.para_pose[0, 3:]))[1]
        assert abs(abs(p_before) - 90) < 1.0 and abs(abs(p_after) - 90) < 1.0, (p_before, p_after)
        # the singular branch: Rs[0] comes back EXACTLY as the pre-solve rotation (rot_diff * R(para_Pose[0]) = Rs[0]); the yaw-only branch would not do that
        R0 = synth.q_to_R(win.para_pose[0, 3:])
        assert np.abs(ref.Rs[0] - R0).max() < 1e-12 and np.abs(got.Rs[0] - R0).max() < 1e-12
        y_only = sequence.ypr2R(np.array([sequence.R2ypr(R0)[0] - sequence.R2ypr(synth.q_to_R(ref.para_pose[0, 3:]))[0], 0, 0])) @ synth.q_to_R(ref.para_pose[0, 3:])
        assert np.abs(y_only - R0).max() > 1e-6, "the yaw-only gauge fix would have left a roll / pitch change at frame 0: the branches differ on this window"
        assert got.summary["num_iterations"] == ref.summary["num_iterations"] and got.summary["num_successful_steps"] == ref.summary["num_successful_steps"]
        assert np.abs(got.Ps - ref.Ps).max() < 1e-7 and np.abs(got.Rs - ref.Rs).max() < 1e-8 and np.abs(got.Vs - ref.Vs).max() < 1e-7
    # (ii) gauge override
    rng = np.random.default_rng(5)
    win, prior, _ = synth.make_window(13, opts, synth.SynthConfig(n_features=120))
    Rg = synth.q_to_R(synth.q_mul(win.para_pose[0, 3:], synth.q_exp(np.array([0.0, 0.0, 0.4]))))          # a frame-0 attitude 0.4 rad of yaw away
    Pg = win.para_pose[0, :3] + rng.normal(0, 3.0, 3)
    plain_ref = oracle.window_solve(opts, win, prior)
    win.gauge_R0, win.gauge_P0 = np.ascontiguousarray(Rg), np.ascontiguousarray(Pg)
    solver.set_prior(prior)
    got = solver.optimization(win)
    ref = oracle.window_solve(opts, win, prior)
    assert np.abs(ref.Ps[0] - Pg).max() < 1e-12 and np.abs(got.Ps[0] - Pg).max() < 1e-12                   # origin_P0 = last_P0
    assert abs(sequence.R2ypr(got.Rs[0])[0] - sequence.R2ypr(Rg)[0]) < 1e-9                                # frame-0 yaw = last_R0's yaw
    assert np.abs(ref.Ps - plain_ref.Ps).max() > 1.0, "the override moved the window"
    assert np.abs(got.Ps - ref.Ps).max() < 1e-7 and np.abs(got.Rs - ref.Rs).max() < 1e-8 and np.abs(got.Vs - ref.Vs).max() < 1e-7

@pytest.mark.gpu
def test_split_linearisation_of_small_batches_is_bit_identical(oracle, opts):
    """Batches of up to 8 windows (the real-time case is one) spread every window's linearisation over several workgroups (k_linearize_split: one per chunk of factor
    slots, one for the IMU factors, one for the LiDAR factors + the prior's cost; the last to arrive assembles). Pair products whose factors span chunks hand their MFMA
    accumulators from workgroup to workgroup, per-thread cost sums are re-added in the single workgroup's order: states, counts, costs and the new priors must equal the
    one-workgroup-per-window launch (VILF_NO_LIN_SPLIT=1) to the bit — windows of mixed shape, with rejected steps, with and without prior."""
    import os
    from vil_fusion_amd.estimator import BackendSolver
    rng = np.random.default_rng(21)
    s = BackendSolver(opts)
    try:
        for B in (1, 3, 8):
            wins, priors = [], []
            for i in range(B):
                nz = float(rng.choice([0.05, 0.2, 0.8, 2.0]))
                c = synth.SynthConfig(n_features=int(rng.integers(3, 330)), with_prior=bool(rng.random() < 0.8), const_fraction=float(rng.choice([0.0, 0.4, 1.0])),
                                      marginalization_flag=(0 if rng.random() < 0.7 else 1), state_noise=(nz, np.deg2rad(10.0 * nz), nz))
                w, p, _ = synth.make_window(int(rng.integers(1, 10**6)), opts, c)
                wins.append(w); priors.append(p)
            got = []
            for one_wg in (False, True):
                if one_wg: os.environ["VILF_NO_LIN_SPLIT"] = "1"
                else: os.environ.pop("VILF_NO_LIN_SPLIT", None)
                s.batch_upload(wins, priors); s.batch_solve(); s.batch_marginalize()
                got.append((s.batch_download(), s.batch_summaries(), s.batch_download_priors() if hasattr(s, "batch_download_priors") else None))
            for i in range(B):
                a, b_ = got[0][0][i], got[1][0][i]
                for k in ("Ps", "Rs", "Vs", "Bas", "Bgs", "para_feature"):
                    assert np.array_equal(getattr(a, k), getattr(b_, k)), (B, i, k)
                sa, sb_ = got[0][1][i], got[1][1][i]
                assert (sa.num_iterations, sa.num_successful_steps, sa.num_linear_solves, sa.final_cost, sa.termination) == (sb_.num_iterations, sb_.num_successful_steps, sb_.num_linear_solves, sb_.final_cost, sb_.termination)
    finally:
        os.environ.pop("VILF_NO_LIN_SPLIT", None)
        s.close()


def test_split_hand_over_wait_is_bounded_and_reported(oracle, opts):
    """k_linearize_split's consumers wait for the previous chunk's accumulators behind a flag that carries the launch's generation. The wait is BOUNDED: a producer that
    never publishes (fault injection: VILF_SPLIT_FAULT=1 makes chunk 0 skip its flag stores) must not hang the device — the window is marked, every reader of its
    results returns VILF_ERR_DEVICE, and the next solve on the same handle (new generation: nothing the dead hand-over left behind is mistaken for a flag) is exact."""
    import os
    from vil_fusion_amd.estimator import BackendSolver
    from vil_fusion_amd.lib import VilfError
    w, p, _ = synth.make_window(5150, opts, synth.SynthConfig(n_features=300))       # several factor chunks: pairs run on from chunk to chunk
    ref = oracle.window_solve(opts, w, p)
    s = BackendSolver(opts)
    try:
        s.batch_upload([w], [p]); s.batch_solve()
        good = s.batch_download()[0]
        assert good.summary["num_iterations"] == ref.summary["num_iterations"] and np.abs(good.Ps - ref.Ps).max() < 1e-7
        os.environ["VILF_SPLIT_FAULT"] = "1"
        s.batch_rewind(); s.batch_solve()
        with pytest.raises(VilfError):
            s.batch_summaries()
        with pytest.raises(VilfError):
            s.batch_download()
        os.environ.pop("VILF_SPLIT_FAULT")
        s.batch_rewind(); s.batch_solve()
        again = s.batch_download()[0]
        for k in ("Ps", "Rs", "Vs", "Bas", "Bgs", "para_feature"):
            assert np.array_equal(getattr(again, k), getattr(good, k)), k
    finally:
        os.environ.pop("VILF_SPLIT_FAULT", None)
        s.close()


def test_split_linearisation_under_contention(opts):
    """200 single-window solves (k_linearize_split: the window's chunks on several workgroups, hand-overs through generation flags) on one handle while a second handle,
    on its own stream and host thread, keeps the device full with 2048-window batches: every one of the 200 results equals the first to the bit, nothing hangs and no
    window is marked. (The split relies on the writer of a hand-over having the LOWER workgroup index; the wait is bounded and reported if that ever fails.)"""
    import threading
    from vil_fusion_amd.estimator import BackendSolver
    w, p, _ = synth.make_window(5150, opts, synth.SynthConfig(n_features=300))
    a = BackendSolver(opts); bsolver = BackendSolver(opts)
    stop = threading.Event()
    try:
        wins, priors = synth.make_batch(77, 2048, opts, synth.SynthConfig(n_features=120), distinct=8)
        bsolver.batch_upload(wins, priors)
        def load():
            while not stop.is_set():
                bsolver.batch_rewind(); bsolver.batch_solve()
        th = threading.Thread(target=load); th.start()
        a.batch_upload([w], [p]); a.batch_solve()
        first = a.batch_download()[0]
        for _ in range(200):
            a.batch_rewind(); a.batch_solve()
            got = a.batch_download()[0]
            for k in ("Ps", "Rs", "Vs", "Bas", "Bgs", "para_feature"):
                assert np.array_equal(getattr(got, k), getattr(first, k)), k
            assert got.summary["num_iterations"] == first.summary["num_iterations"]
        stop.set(); th.join()
        assert all(x.num_iterations > 0 for x in bsolver.batch_summaries())
    finally:
        stop.set()
        a.close(); bsolver.close()


def test_solve_after_a_time_limited_solve(oracle, opts):
    """options.max_solver_time cuts a (split) solve short between two iterations (k_time_limit, termination NO_CONVERGENCE, state = last accepted point); the next solves
    on the same handle run under the same limit and are unaffected by what the interrupted one left in the hand-over buffers: every result is a valid state of the
    window's own iteration sequence (its cost is one of the costs the unlimited solve passes through)."""
    import copy
    from vil_fusion_amd.estimator import BackendSolver
    w, p, _ = synth.make_window(5150, opts, synth.SynthConfig(n_features=300))
    o1 = copy.deepcopy(opts); o1.max_num_iterations = 1
    costs = []
    for it in range(1, 9):
        o1.max_num_iterations = it
        costs.append(oracle.window_solve(o1, w, p).summary["final_cost"])
    lim = copy.deepcopy(opts); lim.max_solver_time = 3e-4            # a few iterations' worth: the solve stops somewhere in the middle
    s = BackendSolver(lim)
    try:
        for rep in range(6):
            s.batch_upload([w], [p]); s.batch_solve()
            got = s.batch_download()[0]
            assert np.isfinite(got.Ps).all()
            c = got.summary["final_cost"]
            assert got.summary["num_iterations"] <= 8 and min(abs(c - x) / x for x in costs + [oracle.window_solve(opts, w, p).summary["initial_cost"]]) < 1e-6, (rep, c, costs)
    finally:
        s.close()
