"""the global_fusion pose-graph back-end (poseGraphOptimization.cpp) — PriorFactor + BetweenFactor<Pose3> graph with
robust loop edges, ISAM2 restated as batch Gauss-Newton. CPU: the oracle's factor against finite differences, its solve against a dense
numpy Gauss-Newton built from the same factors, loop closure removes odometry drift; the oracle against an exact reference that shares none of its
closed forms (pg_reference.py: mpmath at 40 digits, finite-difference Jacobians, dense solve) on graphs that reach the small-angle and pi branches, large
residual rotations, outliers, reversed / doubled / anisotropic edges. GPU: HIP == oracle; HIP against the same exact reference; block and panel edges."""
import ctypes as C
import functools

import numpy as np
import pytest
import pg_reference as R
from vil_fusion_amd import abi, posegraph, synth

PRIOR_SIGMA = np.full(6, 1e-6)                                   # variances 1e-12 (poseGraphOptimization.cpp:123-126)
ODOM_SIGMA = np.sqrt(np.array([1e-6] * 3 + [1e-4] * 3))          # :128-130
LOOP_SIGMA = np.sqrt(np.full(6, 0.5))                            # :132-138


def rand_pose(rng, rot=1.0, trans=5.0):
    q = synth.q_exp(rng.normal(0, rot, 3))
    return np.concatenate([q / np.linalg.norm(q), rng.normal(0, trans, 3)])


def test_oracle_between_factor_against_finite_differences(oracle):
    rng = np.random.default_rng(0)
    for trial in range(20):
        pi, pj = rand_pose(rng), rand_pose(rng)
        meas = posegraph.between(pi, pj) if trial % 2 else rand_pose(rng, 0.5, 2.0)
        if trial % 2:                                             # a measurement close to the truth: small residual
            meas = oracle.pg_retract(meas, rng.normal(0, 0.05, 6))
        sigma = rng.uniform(0.1, 2.0, 6)
        for robust in (0, 1):
            e, A, B, c = oracle.pg_between(pi, pj, meas, sigma, robust)
            if not robust:
                assert abs(c - 0.5 * e @ e) < 1e-12
                h = 1e-6
                for k in range(6):
                    d = np.zeros(6); d[k] = h
                    ep = oracle.pg_between(oracle.pg_retract(pi, d), pj, meas, sigma, 0)[0]; em = oracle.pg_between(oracle.pg_retract(pi, -d), pj, meas, sigma, 0)[0]
                    assert np.abs((ep - em) / (2 * h) - A[:, k]).max() < 2e-7 * max(1.0, np.abs(A).max())
                    ep = oracle.pg_between(pi, oracle.pg_retract(pj, d), meas, sigma, 0)[0]; em = oracle.pg_between(pi, oracle.pg_retract(pj, -d), meas, sigma, 0)[0]
                    assert np.abs((ep - em) / (2 * h) - B[:, k]).max() < 2e-7 * max(1.0, np.abs(B).max())
            else:                                                 # Robust(Cauchy(1)): the whitened factor scaled by sqrt(1 / (1 + r^2))
                e0, A0, B0, c0 = oracle.pg_between(pi, pj, meas, sigma, 0)
                w = np.sqrt(1.0 / (1.0 + e0 @ e0))
                assert np.allclose(e, w * e0, rtol=1e-13) and np.allclose(A, w * A0, rtol=1e-13) and np.allclose(B, w * B0, rtol=1e-13)
                assert abs(c - 0.5 * np.log1p(e0 @ e0)) < 1e-12


def _dense_gauss_newton(oracle, x, edges, iters):
    """reference solve: the same factors (through the oracle's factor hook), dense normal equations with numpy"""
    x = x.copy(); K = len(x); x0 = x[0].copy()
    for _ in range(iters):
        H = np.zeros((6 * K, 6 * K)); g = np.zeros(6 * K)
        ident = np.array([0, 0, 0, 1, 0, 0, 0.0])
        e, A, B, _ = oracle.pg_between(x0, x[0], ident, PRIOR_SIGMA, 0)          # prior = between(prior pose, x0) with identity measurement: B is its Jacobian
        H[:6, :6] += B.T @ B; g[:6] -= B.T @ e
        for (i, j, q, t, sg, rb) in edges:
            e, A, B, _ = oracle.pg_between(x[i], x[j], np.concatenate([q, t]), sg, rb)
            si, sj = slice(6 * i, 6 * i + 6), slice(6 * j, 6 * j + 6)
            H[si, si] += A.T @ A; H[sj, sj] += B.T @ B; H[si, sj] += A.T @ B; H[sj, si] += B.T @ A
            g[si] -= A.T @ e; g[sj] -= B.T @ e
        d = np.linalg.solve(H, g)
        for k in range(K):
            x[k] = oracle.pg_retract(x[k], d[6 * k: 6 * k + 6])
    return x


def test_oracle_solve_matches_dense_numpy_gauss_newton(oracle):
    truth, x0, edges = posegraph.make_synthetic_graph(3, 24, loops=[(2, 20), (5, 23), (0, 12)], odom_noise=(0.01, 0.05), loop_noise=(0.002, 0.01))
    for iters in (1, 3):
        got, it, _ = oracle.posegraph_optimize(x0, PRIOR_SIGMA, edges, max_iterations=iters, tol=0.0)
        ref = _dense_gauss_newton(oracle, x0, edges, iters)
        assert it == iters
        assert np.abs(got[:, 4:] - ref[:, 4:]).max() < 1e-8 and posegraph.max_rotation_difference(got, ref) < 1e-9


def test_oracle_loop_closure_removes_drift(oracle):
    truth, x0, edges = posegraph.make_synthetic_graph(7, 200, loops=[(3, 190), (10, 199), (40, 150)], odom_noise=(0.002, 0.02), loop_noise=(0.0005, 0.005))
    drift0 = np.linalg.norm(x0[-1, 4:] - truth[-1, 4:])
    got, it, cost = oracle.posegraph_optimize(x0, PRIOR_SIGMA, edges, max_iterations=30, tol=1e-9)
    drift1 = np.linalg.norm(got[-1, 4:] - truth[-1, 4:])
    # the reference's loop noise (variance 0.5, Cauchy) is weak against 190 odometry edges of variance 1e-4 / 1e-6: a partial correction
    assert it < 30 and drift0 > 0.5 and drift1 < 0.7 * drift0, (it, drift0, drift1)
    # the same loops trusted like odometry close the loop properly
    tight = [(i, j, q, t, sg if abs(i - j) == 1 else ODOM_SIGMA, 0) for (i, j, q, t, sg, rb) in edges]
    got2, it2, _ = oracle.posegraph_optimize(x0, PRIOR_SIGMA, tight, max_iterations=30, tol=1e-9)
    assert it2 < 30 and np.linalg.norm(got2[-1, 4:] - truth[-1, 4:]) < 0.1 * drift0
    # without loop edges the optimum is the odometry chain itself: nothing moves
    chain = [e for e in edges if abs(e[0] - e[1]) == 1]
    same, it3, cost2 = oracle.posegraph_optimize(x0, PRIOR_SIGMA, chain, max_iterations=5, tol=1e-9)
    assert it3 <= 2 and np.abs(same - x0).max() < 1e-8 and cost2 < 1e-12


def test_keyframe_gate_and_tum_writer(tmp_path):
    """key-frame selection (2 m / 10 deg accumulated since the last key frame, poseGraphOptimization.cpp:517-536) and the TUM writer (:88-110)"""
    pg = posegraph.PoseGraph(backend=None)
    poses = []
    for k in range(40):
        yaw = 0.02 * k
        q = synth.R_to_q(synth.euler_R(np.array(yaw), np.array(0.0), np.array(0.0)))
        poses.append(np.concatenate([q, [0.5 * k, 0.0, 0.0]]))
    keys = [pg.add_odometry(0.1 * k, p) for k, p in enumerate(poses)]
    # first frame is always a key frame (the accumulators start huge, :50-51); then every 5th (4 x 0.5 m = 2 m is not > 2 m)
    assert keys[0] and [k for k, f in enumerate(keys) if f][:4] == [0, 5, 10, 15]
    assert len(pg.edges) == len(pg.nodes) - 1 and all(e[0] + 1 == e[1] for e in pg.edges)
    pg.add_loop(0, len(pg.nodes) - 1, np.array([0, 0, 0, 1, 0.1, 0, 0.0]))
    assert pg.edges[-1][5] == 1 and np.allclose(pg.edges[-1][4], LOOP_SIGMA)
    path = tmp_path / "fs_loam_loop.txt"
    pg.save_tum(str(path))
    rows = np.loadtxt(str(path))
    assert rows.shape == (len(pg.nodes), 8) and np.allclose(rows[:, 0], [n["stamp"] for n in pg.nodes], atol=1e-9)
    assert np.allclose(rows[:, 1], [n["pose"][0] for n in pg.nodes], atol=1e-5) and np.allclose(np.linalg.norm(rows[:, 4:], axis=1), 1.0, atol=1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("K,loops", [(1, []), (2, []), (24, [(2, 20), (5, 23), (0, 12)]), (400, [(3, 390), (10, 399), (40, 150), (41, 151), (100, 300)]), (1500, [(k, 1490 - k) for k in range(0, 400, 10)])])
def test_posegraph_matches_oracle(oracle, K, loops):
    from vil_fusion_amd.estimator import BackendSolver, posegraph_optimize
    truth, x0, edges = posegraph.make_synthetic_graph(11 + K, K, loops=loops, odom_noise=(0.002, 0.02), loop_noise=(0.0005, 0.005))
    ref, it_ref, cost_ref = oracle.posegraph_optimize(x0, PRIOR_SIGMA, edges, max_iterations=30, tol=1e-9)
    s = BackendSolver()
    got, it, cost = posegraph_optimize(s, x0, PRIOR_SIGMA, edges, max_iterations=30, tol=1e-9)
    s.close()
    assert it == it_ref
    assert np.abs(got[:, 4:] - ref[:, 4:]).max() < 1e-7 and posegraph.max_rotation_difference(got, ref) < 1e-9
    assert abs(cost - cost_ref) <= 1e-6 * max(cost_ref, 1e-9)


@pytest.mark.gpu
def test_posegraph_many_loop_edges_and_the_documented_limit(oracle):
    """680 loop edges: the 4080 x 4080 loop-closure block needs more than 64 KB of LDS in the back substitution of the library's dense Cholesky (launch attribute set
    by the library) — one Gauss-Newton iteration against the oracle; beyond the documented 2048 loop edges the call refuses before doing any work."""
    from vil_fusion_amd.estimator import BackendSolver, posegraph_optimize
    from vil_fusion_amd.lib import VilfError
    K, L = 700, 680
    truth, x0, edges = posegraph.make_synthetic_graph(5, K, loops=[(k, K - 5 - k) for k in range(L // 2)] + [(k, k + 7) for k in range(L - L // 2)], odom_noise=(0.002, 0.02), loop_noise=(0.0005, 0.005))
    ref, it_ref, cost_ref = oracle.posegraph_optimize(x0, PRIOR_SIGMA, edges, max_iterations=1, tol=0.0)
    s = BackendSolver()
    got, it, cost = posegraph_optimize(s, x0, PRIOR_SIGMA, edges, max_iterations=1, tol=0.0)
    assert it == it_ref == 1
    assert np.abs(got[:, 4:] - ref[:, 4:]).max() < 1e-7 and posegraph.max_rotation_difference(got, ref) < 1e-9
    K2 = 2200
    truth, x0, edges = posegraph.make_synthetic_graph(6, K2, loops=[(k, k + 50) for k in range(2049)], odom_noise=(0.002, 0.02), loop_noise=(0.0005, 0.005))
    with pytest.raises(VilfError, match="loop edges"):
        posegraph_optimize(s, x0, PRIOR_SIGMA, edges, max_iterations=1, tol=0.0)
    s.close()


# ---- the exact reference (pg_reference.py) as the yardstick: the oracle on the CPU, the HIP solve on the GPU ---------------------------------------------
SMALL_NOISE = (0.0, 1e-12, 1e-9, 1e-6, 3e-4)
DENSE_LOOPS = [(0, 2), (1, 4), (2, 6), (3, 5), (4, 8), (5, 9), (6, 11), (7, 10), (8, 11), (0, 11), (3, 9)]
EXACT_CASES = ["synthetic", "mixed", "outlier"] + ["small_%g" % n for n in SMALL_NOISE] + ["dense_11", "dense_10"]


def _reversed_edge(e):
    """the same constraint stored the other way round: (j, i, meas^-1)"""
    i, j, q, t, sg, rb = e
    m = posegraph.inverse(np.concatenate([q, t]))
    return (j, i, m[:4], m[4:], sg, rb)


@functools.lru_cache(maxsize=None)
def _exact_graph(name):
    """(x0, edges) of one case. Edge order of the K = 12 graphs: odometry 0 .. 10, then the loops (2, 9), (0, 11), (4, 7)"""
    if name.startswith("small_"):                     # residuals from float64 rounding up to 3e-4: across th < 1e-10, tr - 3 >= -1e-7, phi <= 1e-5, th2 <= eps, th2 < 1e-20
        n = float(name[6:])
        _, x0, edges = posegraph.make_synthetic_graph(4, 6, loops=[(0, 4)], odom_noise=(n, n), loop_noise=(n, n))
        return x0, edges
    if name.startswith("dense_"):                     # 11 loops on 12 key frames: 36 L = 396 > 6 K = 72 in pg_build_rhs, NC = 1 + 6 L = 67 (two blocks of pg_chain_solve); 10: NC = 61
        _, x0, edges = posegraph.make_synthetic_graph(3, 12, loops=DENSE_LOOPS[:int(name[6:])])
        return x0, edges
    truth, x0, edges = posegraph.make_synthetic_graph(3, 12, loops=[(2, 9), (0, 11), (4, 7)])
    if name == "mixed":
        rng = np.random.default_rng(17)
        edges[4] = _reversed_edge(edges[4])                                      # odometry stored as (k + 1, k): kind 2 through the A side
        i, j, q, t, sg, rb = _reversed_edge(edges[11])
        edges[11] = (i, j, q, t, rng.uniform(0.2, 1.5, 6), rb)                   # a loop with i > j and anisotropic trust
        edges.append(edges[12])                                                  # the same loop twice
        edges[7] = edges[7][:5] + (1,)                                           # a robust odometry edge
        edges[13] = edges[13][:5] + (0,)                                         # a loop that is not robust
    elif name == "outlier":                           # a wrong ICP result: residual rotation |[1.5, -1.2, 1.4]| = 2.38 rad, Cauchy weight ~ 1 / 40
        m = posegraph.compose(posegraph.between(truth[1], truth[8]), R.exp_qt([1.5, -1.2, 1.4, 3.0, -2.0, 1.0]))
        edges.append((1, 8, m[:4], m[4:], LOOP_SIGMA, 1))
    else:
        assert name == "synthetic"
    return x0, edges


def _exact_iterations(name):
    return (0, 1, 3) if name == "synthetic" else (0, 1)


@functools.lru_cache(maxsize=None)
def _exact_reference(name, iters):
    """the reference after `iters` Gauss-Newton steps: (mp poses, cost there). Computed once per process, shared by the CPU and the GPU tests"""
    x0, edges = _exact_graph(name)
    prior = R.from_qt(x0[0])
    x = [R.from_qt(p) for p in x0] if iters == 0 else R.step(_exact_reference(name, iters - 1)[0], prior, PRIOR_SIGMA, edges)[0]
    return x, float(R.cost(x, prior, PRIOR_SIGMA, edges))


def _cost_matches(name, cost, cost_ref, rtol=1e-10):
    """below 1e-6 (and in the small-residual cases) the float64 rounding of the input poses, divided by sigmas of 1e-3 .. 1e-6, is the whitened residual: poses only"""
    return name.startswith("small_") or cost_ref <= 1e-6 or abs(cost - cost_ref) <= rtol * cost_ref


def test_reference_log_against_matrix_logarithm():
    """the reference's own closed forms (Rodrigues exp / log, V and V^-1) against mp.logm of the 4 x 4 matrix"""
    import mpmath as mp
    rng = np.random.default_rng(5)
    with mp.workdps(R.DPS):
        for _ in range(3):
            xi = rng.normal(0, 1, 6)
            T = R.se3_exp(xi)
            got, M = R.se3_log(T), mp.logm(R.to_matrix4(T))
            want = [M[2, 1], M[0, 2], M[1, 0], M[0, 3], M[1, 3], M[2, 3]]
            assert max(abs(got[k] - want[k]) for k in range(6)) < mp.mpf(10) ** -35
            assert max(abs(got[k] - mp.mpf(float(xi[k]))) for k in range(6)) < mp.mpf(10) ** -35


@pytest.mark.parametrize("name", EXACT_CASES)
def test_oracle_matches_exact_reference(oracle, name):
    """The oracle (same closed forms as the kernels) against the reference that has none of them: 1e-12 m, 1e-13 rad, cost to 1e-10 relative.
    Measured (translation m / rotation rad, after one step): synthetic 1.6e-14 / 8.9e-16 (three steps 6.5e-15 / 8.0e-16), mixed 9.5e-15 / 7.1e-16, outlier 7.6e-15 / 1.0e-15,
    small_* <= 4.2e-15 / 1.2e-15, dense_11 2.9e-14 / 8.4e-16, dense_10 8.8e-15 / 7.5e-16; the rotation figure is already 3e-16 .. 4e-16 at zero iterations (the poses
    come back as float64 quaternions). The bound is 34x / 80x the worst of them: room for other libm versions and summation orders, none for a wrong formula (the sign
    of one Q coefficient moves the outlier case by far more, as does a dropped [t]x R block, a Cauchy weight on the rows, or a swapped Jacobian on a reversed edge)."""
    x0, edges = _exact_graph(name)
    for iters in _exact_iterations(name):
        x_ref, cost_ref = _exact_reference(name, iters)
        got, it, cost = oracle.posegraph_optimize(x0, PRIOR_SIGMA, edges, max_iterations=iters, tol=0.0)
        dt, dr = R.deviation(x_ref, got)
        print("oracle %s iters %d: |dt| %.2e m, angle %.2e rad, cost %.17g (reference %.17g)" % (name, iters, dt, dr, cost, cost_ref))
        assert it == iters
        assert dt < 1e-12 and dr < 1e-13, (dt, dr)
        assert _cost_matches(name, cost, cost_ref), (cost, cost_ref)


PI_SIGMA = np.array([0.3, 0.7, 1.3, 0.5, 0.9, 1.1])


def _pi_graph(axis):
    """two key frames a rotation by exactly pi about `axis` apart, odometry measurement identity: the cost is pi^2 / (2 sigma_axis^2) whatever sign Logmap gives the axis.
    The quaternions (1,0,0,0), (0,1,0,0), (0,0,1,0) are exact in float64 and take the three sub-branches of so3_log's tr + 1 < 1e-10"""
    x0 = np.zeros((2, 7)); x0[0, 3] = 1.0; x0[1, axis] = 1.0
    edges = [(0, 1, np.array([0, 0, 0, 1.0]), np.zeros(3), PI_SIGMA, 0)]
    return x0, edges, 0.5 * np.pi ** 2 / PI_SIGMA[axis] ** 2


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_oracle_cost_at_a_rotation_by_exactly_pi(oracle, axis):
    x0, edges, want = _pi_graph(axis)
    got, it, cost = oracle.posegraph_optimize(x0, PRIOR_SIGMA, edges, max_iterations=0, tol=0.0)
    assert it == 0 and np.array_equal(got, x0)
    assert abs(cost - want) <= 1e-12 * want, (cost, want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", EXACT_CASES)
def test_posegraph_matches_exact_reference(oracle, name):
    """HIP against pg_reference. Bound per case: max(1e-11 m, 1000 x the oracle's own deviation) and max(1e-12 rad, 1000 x ...), the oracle measured in the same run: the
    kernels reach the step by chain Cholesky + Woodbury in another order of arithmetic than the oracle, and the prior's weight of 1e12 beside a loop's 2 leaves a dense
    float64 solve a few digits fewer than the 40-digit one.
    Measured on an MI355X (translation m / rotation rad; oracle in brackets), worst of the iteration counts run:
      synthetic    7.2e-15 / 9.6e-16  (1.6e-14 / 8.9e-16)      small_1e-12  3.7e-15 / 9.2e-16  (3.4e-15 / 9.1e-16)      dense_11  1.2e-14 / 8.5e-16  (2.9e-14 / 8.4e-16)
      mixed        9.9e-15 / 9.3e-16  (9.5e-15 / 7.1e-16)      small_1e-09  3.6e-15 / 7.4e-16  (3.3e-15 / 7.4e-16)      dense_10  7.2e-15 / 1.3e-15  (8.8e-15 / 7.5e-16)
      outlier      7.8e-15 / 8.9e-16  (7.6e-15 / 1.0e-15)      small_1e-06  6.0e-15 / 1.0e-15  (3.3e-15 / 7.1e-16)
      small_0      3.6e-15 / 9.5e-16  (3.2e-15 / 1.2e-15)      small_0.0003 7.5e-15 / 6.4e-16  (4.2e-15 / 9.1e-16)
    i.e. the device solve is as close to the exact step as the oracle is, and three orders inside the bound. Below a cost of 1e-6 the cost is not compared: after one
    step of small_0 the device reports 2.5e-20 where the reference has 5.9e-30 — node 0 is stored as a float64 quaternion between iterations, and 1e-16 of rounding
    against the prior's sigma of 1e-6 is a whitened residual of 1e-10."""
    from vil_fusion_amd.estimator import BackendSolver, posegraph_optimize
    x0, edges = _exact_graph(name)
    s = BackendSolver()
    try:
        for iters in _exact_iterations(name):
            x_ref, cost_ref = _exact_reference(name, iters)
            ref, _, _ = oracle.posegraph_optimize(x0, PRIOR_SIGMA, edges, max_iterations=iters, tol=0.0)
            odt, odr = R.deviation(x_ref, ref)
            got, it, cost = posegraph_optimize(s, x0, PRIOR_SIGMA, edges, max_iterations=iters, tol=0.0)
            dt, dr = R.deviation(x_ref, got)
            print("hip %s iters %d: |dt| %.2e m (oracle %.2e), angle %.2e rad (oracle %.2e), cost %.17g (reference %.17g)" % (name, iters, dt, odt, dr, odr, cost, cost_ref))
            assert it == iters
            assert dt < max(1e-11, 1000 * odt) and dr < max(1e-12, 1000 * odr), (dt, dr, odt, odr)
            assert _cost_matches(name, cost, cost_ref), (cost, cost_ref)
        if name == "synthetic":
            _, it_ref, _ = oracle.posegraph_optimize(x0, PRIOR_SIGMA, edges, max_iterations=30, tol=1e-9)
            _, it, _ = posegraph_optimize(s, x0, PRIOR_SIGMA, edges, max_iterations=30, tol=1e-9)
            assert it == it_ref and 1 < it < 30
    finally:
        s.close()


@pytest.mark.gpu
def test_posegraph_cost_at_a_rotation_by_exactly_pi():
    from vil_fusion_amd.estimator import BackendSolver, posegraph_optimize
    s = BackendSolver()
    try:
        for axis in range(3):
            x0, edges, want = _pi_graph(axis)
            got, it, cost = posegraph_optimize(s, x0, PRIOR_SIGMA, edges, max_iterations=0, tol=0.0)
            assert it == 0 and np.array_equal(got, x0)
            assert abs(cost - want) <= 1e-12 * want, (axis, cost, want)
    finally:
        s.close()


def _two_loops(K):
    return [(2, K - 3), (K // 3, 2 * K // 3)]


# 64-thread blocks: pg_assemble / pg_update over K = 63, 64, 65, 129; pg_linearize over n_edges + 1 = 64 (K = 63, one loop) and 65 (K = 63, two loops).
# lw_chol_panel / lw_chol_step / lw_chol_back work in 64-column blocks (CH_NB): 6 L = 60, 66 either side of one block, 126, 132 either side of two (64 and 128 are no
# multiple of 6); with the right-hand side as row 6 L the factor has 61, 67, 127, 133 rows. K = 6 * 22 + 8 = 140, loops (k, k + 7).
EDGE_GRAPHS = [("K63_nF64", 63, [(2, 60)]), ("K63_nF65", 63, _two_loops(63)), ("K64", 64, _two_loops(64)), ("K65", 65, _two_loops(65)), ("K129", 129, _two_loops(129))] + \
              [("L%d" % L, 140, [(k, k + 7) for k in range(L)]) for L in (10, 11, 21, 22)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,K,loops", EDGE_GRAPHS, ids=[g[0] for g in EDGE_GRAPHS])
def test_posegraph_block_and_panel_edges(oracle, name, K, loops):
    """HIP against the oracle (which test_oracle_matches_exact_reference anchors to the exact reference; these graphs are too large for an mp dense solve) where a
    thread block or a Cholesky panel ends: one Gauss-Newton iteration, K = 65 also run to convergence. 1e-10 m, 1e-11 rad.
    Measured on an MI355X (translation m / rotation rad): K63_nF64 3.1e-14 / 6.7e-16, K63_nF65 2.8e-14 / 1.2e-15, K64 3.5e-14 / 1.4e-15, K65 6.6e-14 / 1.4e-15 (converged
    in 7 iterations like the oracle: 2.8e-14 / 8.9e-16), K129 1.8e-12 / 2.9e-14, L10 4.3e-14 / 1.1e-15, L11 6.4e-14 / 1.6e-15, L21 9.6e-14 / 1.6e-15, L22 7.1e-14 / 1.1e-15;
    cost equal to 1.6e-13 relative or better. The difference grows with the chain length (K129), which is why the 1e-7 m of the K = 1500 and L = 680 tests above is left
    as it is: nothing here measures those sizes."""
    from vil_fusion_amd.estimator import BackendSolver, posegraph_optimize
    truth, x0, edges = posegraph.make_synthetic_graph(21 + K + len(loops), K, loops=loops)
    assert len(edges) == K - 1 + len(loops)
    s = BackendSolver()
    try:
        for iters, tol in [(1, 0.0)] + ([(30, 1e-9)] if name == "K65" else []):
            ref, it_ref, cost_ref = oracle.posegraph_optimize(x0, PRIOR_SIGMA, edges, max_iterations=iters, tol=tol)
            got, it, cost = posegraph_optimize(s, x0, PRIOR_SIGMA, edges, max_iterations=iters, tol=tol)
            dt, dr = np.abs(got[:, 4:] - ref[:, 4:]).max(), posegraph.max_rotation_difference(got, ref)
            print("hip %s max_iterations %d: %d iterations, |dt| %.2e m, angle %.2e rad, cost %.17g (oracle %.17g)" % (name, iters, it, dt, dr, cost, cost_ref))
            assert it == it_ref and (it == 1 if tol == 0.0 else 1 < it < 30)
            assert dt < 1e-10 and dr < 1e-11, (dt, dr)
            assert cost_ref > 1e-6 and abs(cost - cost_ref) <= 1e-10 * cost_ref, (cost, cost_ref)
    finally:
        s.close()


@pytest.mark.gpu
def test_posegraph_refused_calls_leave_poses_and_solver_intact(oracle):
    """a call the entry point refuses returns an error, writes nothing into the caller's poses and leaves the handle usable (a good call follows each)"""
    from vil_fusion_amd.estimator import BackendSolver, posegraph_optimize
    truth, x0, edges = posegraph.make_synthetic_graph(1, 8, loops=[(1, 6)])
    ref, it_ref, _ = oracle.posegraph_optimize(x0, PRIOR_SIGMA, edges, max_iterations=1, tol=0.0)
    i, j, q, t, sg, rb = edges[-1]
    zero_sigma = np.array(sg); zero_sigma[4] = 0.0
    refused = {"i == j": (edges[:-1] + [(3, 3, q, t, sg, rb)], 1), "endpoint == K": (edges[:-1] + [(i, 8, q, t, sg, rb)], 1), "sigma of 0": (edges[:-1] + [(i, j, q, t, zero_sigma, rb)], 1),
               "missing odometry link": (edges[:3] + edges[4:], 1), "max_iterations < 0": (edges, -1)}
    s = BackendSolver()
    try:
        L = s._L
        L.vilf_posegraph_optimize.argtypes = [C.c_void_p, C.c_int, abi.c_double_p, abi.c_double_p, C.c_int, C.POINTER(abi.PgEdge), C.c_int, C.c_double, C.POINTER(C.c_int), abi.c_double_p]
        for what, (bad, iters) in refused.items():
            x = np.ascontiguousarray(x0).copy()
            it, cost = C.c_int(-7), np.zeros(1)
            rc = L.vilf_posegraph_optimize(s._h, len(x), abi.dptr(x), abi.dptr(PRIOR_SIGMA), len(bad), oracle.make_pg_edges(bad), iters, 0.0, C.byref(it), abi.dptr(cost))
            assert rc != 0, what
            assert np.array_equal(x, x0) and it.value == -7, what
            got, n, _ = posegraph_optimize(s, x0, PRIOR_SIGMA, edges, max_iterations=1, tol=0.0)
            assert n == 1 and np.abs(got[:, 4:] - ref[:, 4:]).max() < 1e-10 and posegraph.max_rotation_difference(got, ref) < 1e-11, what
    finally:
        s.close()
