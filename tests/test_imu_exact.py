"""IMU pre-integration, sqrt_info and the IMU factor against exact references (tests/imu_exact.py: mpmath at 50 digits, written from the
reference's text) on the case list of tests/imu_cases.py. The exact pre-integration rows are stored in tests/golden/imu_exact.npz
(double-double pairs, tests/golden/make_imu_exact.py); sqrt_info and the factor outputs are cheap and computed here once.

Error measure: per field group, max|got - exact| / max|exact|. CPU tests pin the oracle and the host routine vilf_imu_preintegrate with
bounds from rounding analysis (stated at each bound); they also yield the oracle's error figures. GPU tests allow the device four times
the oracle's error on the same case and group, plus 16 units in the last place of the group's largest magnitude (device code contracts
multiply-adds and sums in another order; a wrong coefficient, sign, stride or pivot rule is off by many orders of magnitude). Measured
figures: DESIGN.md, "IMU chain against an exact reference"."""
import ctypes as C
import functools
import os
import numpy as np
import pytest
import imu_cases
import imu_exact
from vil_fusion_amd import abi

EPS = float(np.finfo(np.float64).eps)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "imu_exact.npz")
INPUT_KEYS = ("noise", "acc_0", "gyr_0", "ba", "bg", "dt", "acc", "gyr")
PRE_GROUPS = {k: abi.IMU_OFF[k] for k in ("sum_dt", "delta_p", "delta_q", "delta_v", "jacobian", "covariance")}
RAW_BLOCKS = {"J_pose_i": (0, 6), "J_speed_bias_i": (6, 15), "J_pose_j": (15, 21), "J_speed_bias_j": (21, 30)}
FACTOR = 4.0
FLOOR = 16.0 * EPS


# ---- shared data (computed once, never modified) ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture():
    d = np.load(GOLDEN)
    return {k: d[k] for k in d.files}


@functools.lru_cache(maxsize=None)
def intervals():
    return imu_cases.intervals()


def exact_row(name):
    """(hi, lo) of the exact row"""
    f = fixture()
    return f["hi/" + name], f["lo/" + name]


def rows_f64():
    return {n: exact_row(n)[0] for n in intervals()}


def dd_err(got, hi, lo):
    """max|got - exact| / max|exact| for exact = hi + lo; got - hi is formed first, so the difference keeps the low part. 0 / 0 = 0."""
    got, hi, lo = np.ravel(got), np.ravel(hi), np.ravel(lo)
    with np.errstate(invalid="ignore"):
        d = np.abs((got - hi) - lo)
    if not np.isfinite(d).all():
        return float("inf")
    scale = np.abs(hi).max(initial=0.0)
    return 0.0 if d.max(initial=0.0) == 0.0 else float(d.max() / scale) if scale > 0 else float("inf")


def pre_errors(row, name):
    hi, lo = exact_row(name)
    return {g: dd_err(row[a:b], hi[a:b], lo[a:b]) for g, (a, b) in PRE_GROUPS.items()}


def noise_of(case):
    return abi.ImuNoise(*case["noise"])


def oracle_row(oracle, case):
    return oracle.imu_preintegrate(noise_of(case), *[case[k] for k in INPUT_KEYS[1:]])


def host_row(case):
    from vil_fusion_amd.estimator import imu_preintegrate
    out = imu_preintegrate(noise_of(case), *[case[k] for k in INPUT_KEYS[1:]])
    return np.frombuffer(bytes(out), dtype=np.float64).copy()


@functools.lru_cache(maxsize=None)
def covariances():
    """name -> 15 x 15 float64: the rounded exact covariance of every interval that has an inverse, then the constructed matrices"""
    c = {}
    for n in intervals():
        if n not in imu_cases.SINGULAR:
            a, b = abi.IMU_OFF["covariance"]
            c["interval:" + n] = exact_row(n)[0][a:b].reshape(15, 15).copy()
    for n, (A, _) in imu_cases.constructed_covariances().items():
        c[n] = A
    return c


@functools.lru_cache(maxsize=None)
def sqrt_info_exact(name):
    """U as (mpf rows, hi, lo)"""
    U = imu_exact.sqrt_info_exact(covariances()[name])
    hi, lo = imu_exact.to_dd([x for r in U for x in r])
    return U, hi.reshape(15, 15), lo.reshape(15, 15)


@functools.lru_cache(maxsize=None)
def factor_cases():
    return imu_cases.factor_cases(rows_f64())


@functools.lru_cache(maxsize=None)
def factor_exact(name):
    """raw and whitened exact outputs of one evaluation, and the exact sqrt_info of its covariance: dict of (hi, lo) pairs"""
    c = factor_cases()[name]
    r, J = imu_exact.imu_raw_exact(c["params"], c["pre"], c["G"])
    out = {"r": imu_exact.to_dd(r), "J": tuple(a.reshape(15, 30) for a in imu_exact.to_dd([x for row in J for x in row]))}
    U = imu_exact.sqrt_info_exact(c["pre"][abi.IMU_OFF["covariance"][0]:].reshape(15, 15))
    rw, Jw = imu_exact.imu_whitened_exact(U, r, J)
    out["rw"] = imu_exact.to_dd(rw)
    out["Jw"] = tuple(a.reshape(15, 30) for a in imu_exact.to_dd([x for row in Jw for x in row]))
    out["U"] = tuple(a.reshape(15, 15) for a in imu_exact.to_dd([x for row in U for x in row]))
    return out


def local30(jacs):
    """the four Ceres blocks (15 x 7, 9, 7, 9) -> 15 x 30 in local size; the 7th column of a pose block must be zero"""
    assert not jacs[0][:, 6].any() and not jacs[2][:, 6].any()
    return np.concatenate([jacs[0][:, :6], jacs[1], jacs[2][:, :6], jacs[3]], axis=1)


def factor_errors(ex, r=None, J=None, rw=None, Jw=None, S=None):
    e = {}
    if r is not None:
        e["raw_residual"] = dd_err(r, *ex["r"])
    if J is not None:
        for g, (a, b) in RAW_BLOCKS.items():
            e["raw_" + g] = dd_err(J[:, a:b], ex["J"][0][:, a:b], ex["J"][1][:, a:b])
    if rw is not None:
        e["whitened_residual"] = dd_err(rw, *ex["rw"])
    if Jw is not None:
        e["whitened_jacobian"] = dd_err(Jw, *ex["Jw"])
    if S is not None:
        e["sqrt_info"] = dd_err(S, *ex["U"])
    return e


def pre_struct(row):
    return abi.ImuPreint.from_buffer_copy(np.ascontiguousarray(row, dtype=np.float64).tobytes())


def oracle_sqrt_info(oracle, cov):
    pre = abi.ImuPreint()
    pre.covariance[:] = list(np.ravel(cov))
    S = np.zeros(225)
    oracle.lib().vilo_imu_sqrt_info(C.byref(pre), abi.dptr(S))
    return S.reshape(15, 15)


def oracle_factor(oracle, opts, case):
    import copy
    o = copy.copy(opts)
    o.G[:] = list(case["G"])
    pre = pre_struct(case["pre"])
    r, J = oracle.eval_factor("imu_raw", o, case["params"], pre, sizes=[7, 9, 7, 9], nres=15)
    rw, Jw = oracle.eval_factor("imu", o, case["params"], pre, sizes=[7, 9, 7, 9], nres=15)
    return r, local30(J), rw, local30(Jw)


def assert_within(dev, ref, what):
    """device errors against the oracle's on the same case: 4 x + 16 ulp of the group's largest magnitude"""
    bad = {g: (dev[g], ref[g]) for g in dev if not dev[g] <= FACTOR * ref[g] + FLOOR}
    assert not bad, (what, bad)


# ---- bounds of the CPU tests (from rounding analysis, not from what the code gives) ------------------------------------------------
def pre_bound(n_samples):
    """Every step forms each entry of F J, F P F^T + V N V^T by dot products of 15, 15 and 18 terms whose |F| row sums stay near 1, so a step
    adds at most about 48 eps of the group's magnitude and n steps add at most 48 n eps (worst case, linear growth; sum_dt: n eps / 2)."""
    return 48.0 * (n_samples + 1) * EPS


def scaled_cond(cov):
    d = np.sqrt(np.diag(cov))
    return float(np.linalg.cond(cov / np.outer(d, d)))


def sqrt_info_bound(cov):
    """Inverse and Cholesky of D C D lose what the unit-diagonal C loses (the bounds for Cholesky-type factorisations hold for the scaled matrix,
    within a factor n of the best diagonal scaling): n^2 eps cond(C), n = 15."""
    return 225.0 * EPS * scaled_cond(cov)


def residual_scale(case):
    """largest term that enters the residual sums before they cancel (positions, V T, G T^2 / 2, the deltas)"""
    p, pre, g = case["params"], case["pre"], case["G"]
    T = abs(pre[0])
    return max(1.0, np.abs(p[0][:3]).max(), np.abs(p[2][:3]).max(), np.abs(p[1][:3]).max() * T, np.abs(p[3][:3]).max(), 0.5 * np.abs(g).max() * T * T,
               np.abs(g).max() * T, np.abs(pre[1:4]).max(), np.abs(pre[8:11]).max())


def assert_factor_bounds(name, e, ex, case):
    """absolute bounds: 64 eps of the largest term for the raw outputs (sums of a few products of such terms); the whitened outputs are 15-term
    products with sqrt_info and inherit its bound"""
    M = residual_scale(case)
    mx = lambda pair: float(np.abs(pair[0]).max())
    raw_r_abs = 64.0 * EPS * M
    assert e["raw_residual"] * mx(ex["r"]) <= raw_r_abs, (name, "raw_residual", e["raw_residual"])
    for g, (a, b) in RAW_BLOCKS.items():
        sc = float(np.abs(ex["J"][0][:, a:b]).max())
        assert e["raw_" + g] * sc <= 64.0 * EPS * max(M, sc), (name, g, e["raw_" + g])
    if "whitened_residual" in e:
        cov = case["pre"][abi.IMU_OFF["covariance"][0]:].reshape(15, 15)
        u_rel = sqrt_info_bound(cov) + FLOOR
        U = mx(ex["U"])
        assert e["whitened_residual"] * mx(ex["rw"]) <= 15.0 * U * (raw_r_abs + u_rel * mx(ex["r"])), (name, "whitened_residual", e["whitened_residual"])
        Jmax = float(np.abs(ex["J"][0]).max())
        assert e["whitened_jacobian"] * mx(ex["Jw"]) <= 15.0 * U * (64.0 * EPS * max(M, Jmax) + u_rel * Jmax), (name, "whitened_jacobian", e["whitened_jacobian"])


# the intervals whose covariance has no inverse. n0 and zero_noise: exactly zero. n1: after ONE sample the position rows of V are dt / 2 times its
# velocity rows (integration_base.h:109-118), so V N V^T has rank 12 for every input; its rounded covariance inverts to garbage, not to a reference.
NO_SQRT_INFO = imu_cases.SINGULAR + ("n1",)


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------
def test_fixture_matches_its_generator():
    """Every interval regenerates to the stored input digest; every interval of at most 40 samples is recomputed here and must equal the stored
    double-double pairs, inputs included."""
    f = fixture()
    assert list(f["names"]) == list(intervals())
    for name, case in intervals().items():
        assert str(f["digest/" + name]) == imu_cases.digest(case), name
        if len(case["dt"]) <= imu_cases.REGEN_MAX_SAMPLES:
            for k in INPUT_KEYS:
                assert np.array_equal(f["in/%s/%s" % (name, k)], np.asarray(case[k], dtype=np.float64)), (name, k)
            hi, lo = imu_exact.to_dd(imu_exact.preintegrate_exact(*[case[k] for k in INPUT_KEYS]))
            assert np.array_equal(hi, f["hi/" + name]) and np.array_equal(lo, f["lo/" + name]), name
    assert os.path.getsize(GOLDEN) <= 153533, "no larger than the largest earlier fixture"


def test_case_list_holds_what_it_claims():
    """The properties the cases are there for, proved on the exact values: delta_q.w < 0 after 8 rad, sum_dt of 2000 x 0.005 lands ABOVE 10.0 (exactly:
    float(0.005) > 0.005; and in fp64 accumulation: 10.000000000000163), the singular covariances, the pivot paths of the constructed matrices
    (mp restatement of PartialPivLU), the signs and angles of the factor cases."""
    rows = rows_f64()
    for n in ("gyro8_fixed_axis", "gyro8_moving_axis"):
        assert rows[n][abi.IMU_OFF["delta_q"][0] + 3] < 0, n
    hi, lo = exact_row("n2000_5ms")
    assert hi[0] == 10.0 and lo[0] > 0
    assert float(np.cumsum(intervals()["n2000_5ms"]["dt"])[-1]) > 10.0
    c = intervals()
    assert [len(c[n]["dt"]) for n in ("n0", "n1", "n2", "n3", "n20", "n200", "n2000_5ms")] == [0, 1, 2, 3, 20, 200, 2000]
    assert c["zero_dt_mid"]["dt"][2] == 0.0 and 1e-6 in c["dt_1e-6"]["dt"] and 0.1 in c["dt_0.1"]["dt"]
    assert all(len(set(c[n]["dt"])) > 1 for n in c if len(c[n]["dt"]) > 1 and n != "n2000_5ms"), "non-uniform dt"
    a, b = abi.IMU_OFF["covariance"]
    for n in imu_cases.SINGULAR:
        assert not rows[n][a:b].any() and not exact_row(n)[1][a:b].any()
    P1 = rows["n1"][a:b].reshape(15, 15); half_dt = 0.5 * c["n1"]["dt"][0]
    assert np.allclose(P1[0:3], half_dt * P1[6:9], rtol=1e-14, atol=0.0), "one sample: position rows = dt / 2 times velocity rows, rank 12"
    for n, (A, want) in imu_cases.constructed_covariances().items():
        piv, margin = imu_exact.pivot_sequence(A)
        swaps = [k for k, p in enumerate(piv) if p != k]
        assert swaps == want["swaps"], (n, swaps)
        if "tie" in want:
            assert margin[want["tie"]] == 1.0 and A[0, 0] == A[1, 0], "an exact tie, and the first row keeps the pivot"
        else:
            assert min(margin) > 1e3, "no near-tie: fp64 takes the same path"
        assert 1e-9 <= np.sqrt(np.diag(A)).min() and np.sqrt(np.diag(A)).max() <= 1e-2
    f = factor_cases()
    assert f["negative_w"]["params"][0][6] < 0 and f["negative_w"]["params"][2][6] < 0 and f["negative_w_j_only"]["params"][2][6] < 0
    for n in ("residual_179deg", "residual_181deg"):
        r = np.asarray(factor_exact(n)["r"][0])[3:6]                   # 2 vec(q): |r| = 2 sin(angle / 2); 2 sin(89 deg) = 1.99970
        assert 1.9996 < np.linalg.norm(r) <= 2.0, (n, np.linalg.norm(r))
    w179 = _residual_w("residual_179deg"); w181 = _residual_w("residual_181deg")
    assert 0 < w179 < 0.02 and -0.02 < w181 < 0, (w179, w181)
    assert np.isclose(np.linalg.norm(f["bias_at_threshold"]["params"][1][3:6] - f["bias_at_threshold"]["pre"][11:14]), 0.1, rtol=1e-12)
    assert np.isclose(np.linalg.norm(f["bias_at_threshold"]["params"][1][6:9] - f["bias_at_threshold"]["pre"][14:17]), 0.01, rtol=1e-12)
    assert np.isclose(np.linalg.norm(f["bias_10x_threshold"]["params"][1][3:6] - f["bias_10x_threshold"]["pre"][11:14]), 1.0, rtol=1e-12)
    assert np.abs(f["far_5km"]["params"][0][:3]).max() > 2000 and f["sum_dt_0.05"]["pre"][0] == 0.05 and f["sum_dt_10"]["pre"][0] == 10.0
    assert np.count_nonzero(f["G_three_components"]["G"]) == 3


def _residual_w(name):
    """w of corrected_delta_q^-1 Qi^-1 Qj in fp64 (sign only)"""
    c = factor_cases()[name]
    qi, qj, dq = c["params"][0][3:7], c["params"][2][3:7], c["pre"][4:8]
    conj = lambda q: np.array([-q[0], -q[1], -q[2], q[3]])
    return float(imu_cases.qmul(conj(dq), imu_cases.qmul(conj(qi), qj))[3])


def test_oracle_and_host_preintegration_against_exact(oracle):
    """vilo_imu_preintegrate and vilf_imu_preintegrate (host routine, no handle) on every interval, all 467 fields. Biases are copied: equal. The two are
    NOT bit-identical to each other (different association in the 3 x 3 products); both sit within a few eps of the exact row (107 eps for the
    covariance after 2000 samples)."""
    for name, case in intervals().items():
        hi, lo = exact_row(name)
        for who, row in (("oracle", oracle_row(oracle, case)), ("host", host_row(case))):
            assert np.isfinite(row).all(), (who, name)
            assert np.array_equal(row[11:17], hi[11:17]), (who, name, "linearized biases")
            e = pre_errors(row, name)
            bad = {g: v for g, v in e.items() if not v <= pre_bound(len(case["dt"]))}
            assert not bad, (who, name, bad)
        if len(case["dt"]) == 0:
            assert np.array_equal(row[17:242], np.eye(15).ravel()) and not row[242:].any() and row[7] == 1.0 and not row[:7].any()


def test_oracle_sqrt_info_against_exact(oracle):
    """vilo_imu_sqrt_info on the covariances of the intervals and on the constructed D C D matrices: upper triangular, positive diagonal, within
    n^2 eps cond(C) of the exact factor. The 2000-sample covariance has cond 1.3e11 (97.6 after scaling to unit diagonal); the constructed ones reach
    1.3e14 (3 scaled). max|U^T U cov - I| is measured in mp and reported (it is the yardstick of the device test), not bounded here."""
    for name, A in covariances().items():
        if name[9:] in NO_SQRT_INFO:
            continue
        _, hi, lo = sqrt_info_exact(name)
        S = oracle_sqrt_info(oracle, A)
        assert np.array_equal(S, np.triu(S)) and (np.diag(S) > 0).all(), name
        assert dd_err(S, hi, lo) <= sqrt_info_bound(A), (name, dd_err(S, hi, lo))


def test_oracle_factor_against_exact(oracle, opts):
    """eval_factor("imu_raw") and eval_factor("imu") on every evaluation case: 15 residuals and the 15 x 30 local Jacobian, raw and whitened"""
    for name, case in factor_cases().items():
        ex = factor_exact(name)
        r, J, rw, Jw = oracle_factor(oracle, opts, case)
        assert_factor_bounds(name, factor_errors(ex, r, J, rw, Jw), ex, case)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver():
    from vil_fusion_amd.estimator import BackendSolver
    s = BackendSolver()          # raises VilfError when the HIP library / GPU is missing: no silent fallback
    yield s
    s.close()


def device_rows(solver, cases, max_samples):
    """vilf_imu_preintegrate_batch on interval dicts that share one noise setting; every slot behind n_samples[i] is NaN"""
    from vil_fusion_amd.estimator import imu_preintegrate_batch
    assert len({c["noise"] for c in cases}) == 1
    b = imu_cases.padded_batch(cases, max_samples)
    return imu_preintegrate_batch(solver, noise_of(cases[0]), b["acc_0"], b["gyr_0"], b["ba"], b["bg"], b["n_samples"], b["dt"], b["acc"], b["gyr"])


@functools.lru_cache(maxsize=None)
def _oracle_pre_errors(name):
    import oracle_lib
    return pre_errors(oracle_row(oracle_lib, intervals()[name]), name)


def check_device_row(row, name, what):
    hi, _ = exact_row(name)
    assert np.isfinite(row).all(), (what, name, "finite wherever the exact row is")
    assert np.array_equal(row[11:17], hi[11:17]), (what, name, "linearized biases")
    assert_within(pre_errors(row, name), _oracle_pre_errors(name), (what, name))


@pytest.mark.gpu
def test_device_preintegration_against_exact(solver, oracle):
    """vilf_imu_preintegrate_batch on the whole interval list, NaN behind every interval: one batch of the 13 intervals that share the noise setting
    (0 .. 200 samples in 200 slots), the zero-noise interval, and the 2000-sample interval as a batch of one. Against the exact rows at 4 x the oracle's
    error + 16 ulp, and against the host routine on the same intervals (same source, compiled twice: the device contracts multiply-adds, so the two agree
    to rounding, not to the bit; the host routine's own error is pinned by the CPU test)."""
    c = intervals()
    shared = [n for n in c if c[n]["noise"] == imu_cases.NOISE and n != "n2000_5ms"]
    assert len(shared) == 13
    got = dict(zip(shared, device_rows(solver, [c[n] for n in shared], 200)))
    got["zero_noise"] = device_rows(solver, [c["zero_noise"]], 20)[0]
    got["n2000_5ms"] = device_rows(solver, [c["n2000_5ms"]], 2000)[0]
    assert set(got) == set(c)
    for name, row in got.items():
        check_device_row(row, name, "device")
        host = host_row(c[name]); e_host = pre_errors(host, name); hi = exact_row(name)[0]
        for g, (a, b) in PRE_GROUPS.items():             # triangle inequality: what the device may be off the exact row, plus what the host routine is
            allowed = (FACTOR * _oracle_pre_errors(name)[g] + FLOOR + e_host[g]) * np.abs(hi[a:b]).max()
            assert np.abs(row[a:b] - host[a:b]).max() <= allowed, (name, g, "device against host routine")
    # the intervals without an inverse covariance: what the fields are
    for name in ("n0",):
        row = got[name]
        assert row[0] == 0.0 and not row[1:7].any() and row[7] == 1.0 and not row[8:11].any()
        assert np.array_equal(row[17:242], np.eye(15).ravel()) and not row[242:].any()
    assert not got["zero_noise"][242:].any(), "zero noise: the covariance is exactly zero"
    assert got["gyro8_fixed_axis"][7] < 0 and got["gyro8_moving_axis"][7] < 0, "delta_q.w goes negative after 8 rad"
    assert got["n2000_5ms"][0] > 10.0, "2000 x 0.005 accumulates to 10.000000000000163: above the validity limit"


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_device_preintegration_batch_sizes(solver, oracle, n):
    """Batches across the 64-lane workgroup boundary, built by cycling the intervals of at most 20 samples (0 and max_samples = 20 among them) from a
    different start for every size, NaN in every unused slot: interval i must equal, bit for bit, the same interval run as a batch of one, and its exact row
    within the device tolerance. A wrong per-interval stride on dt / acc / gyr or a read past n_samples[i] lands in a neighbour's data or in NaN."""
    c = intervals()
    small = [k for k in c if len(c[k]["dt"]) <= 20 and c[k]["noise"] == imu_cases.NOISE]
    assert {len(c[k]["dt"]) for k in small} >= {0, 1, 2, 3, 5, 20}
    names = [small[(i * 7 + n) % len(small)] for i in range(n)]
    rows = device_rows(solver, [c[k] for k in names], 20)
    single = {k: device_rows(solver, [c[k]], 20)[0] for k in sorted(set(names))}
    for i, k in enumerate(names):
        assert np.array_equal(rows[i], single[k]), (n, i, k, "batch entry != batch of one")
    for k, row in single.items():
        check_device_row(row, k, "batch of one")


@pytest.mark.gpu
def test_device_preintegration_batch_argument_edges(solver):
    """max_samples = 0 with null sample pointers integrates nothing (identity Jacobian, zero covariance, the biases passed through); n_samples[i] > max_samples
    is refused with VILF_ERR_INVALID_ARGUMENT before anything is launched."""
    L = solver._L
    L.vilf_imu_preintegrate_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(abi.ImuNoise), abi.c_double_p, abi.c_double_p, abi.c_double_p, abi.c_double_p,
                                              C.POINTER(C.c_int), C.c_int, abi.c_double_p, abi.c_double_p, abi.c_double_p, C.c_void_p]
    n = 65
    rng = np.random.default_rng(3)
    a0, g0, ba, bg = [np.ascontiguousarray(rng.random((n, 3))) for _ in range(4)]
    ns = np.zeros(n, dtype=np.int32)
    out = np.full((n, abi.IMU_DOUBLES), np.nan)
    noise = abi.ImuNoise(*imu_cases.NOISE)
    rc = L.vilf_imu_preintegrate_batch(solver._h, n, C.byref(noise), abi.dptr(a0), abi.dptr(g0), abi.dptr(ba), abi.dptr(bg), ns.ctypes.data_as(C.POINTER(C.c_int)), 0,
                                       None, None, None, out.ctypes.data)
    assert rc == abi.VILF_OK
    want = np.zeros((n, abi.IMU_DOUBLES)); want[:, 7] = 1.0; want[:, 11:14] = ba; want[:, 14:17] = bg; want[:, 17:242] = np.eye(15).ravel()
    assert np.array_equal(out, want)
    c = intervals()["n3"]
    b = imu_cases.padded_batch([c, c], 3)
    b["n_samples"][1] = 4
    out2 = np.zeros((2, abi.IMU_DOUBLES))
    rc = L.vilf_imu_preintegrate_batch(solver._h, 2, C.byref(noise), abi.dptr(b["acc_0"]), abi.dptr(b["gyr_0"]), abi.dptr(b["ba"]), abi.dptr(b["bg"]),
                                       b["n_samples"].ctypes.data_as(C.POINTER(C.c_int)), 3, abi.dptr(b["dt"]), abi.dptr(b["acc"]), abi.dptr(b["gyr"]), out2.ctypes.data)
    assert rc == abi.VILF_ERR_INVALID_ARGUMENT and not out2.any()


def device_sqrt_info(solver, covs):
    """vilf_debug_imu_sqrt_info: k_imu_prep launched as the batch upload launches it"""
    L = solver._L
    L.vilf_debug_imu_sqrt_info.argtypes = [C.c_void_p, C.c_int, abi.c_double_p, abi.c_double_p]
    A = np.ascontiguousarray(np.array(covs, dtype=np.float64).reshape(len(covs), 225))
    out = np.full((len(covs), 225), np.nan)
    assert L.vilf_debug_imu_sqrt_info(solver._h, len(covs), abi.dptr(A), abi.dptr(out)) == abi.VILF_OK
    return out.reshape(len(covs), 15, 15)


@pytest.mark.gpu
def test_device_sqrt_info_against_exact(solver, oracle):
    """k_imu_prep on every covariance of the list in ONE launch (17 factors: five workgroups, all four lane groups, a tail of three idle groups) against the exact
    factor, and max|U^T U cov - I| in mp, each at 4 x the oracle's figure + 16 ulp. The list holds no swap, a swap in column 0, in column 13, in five columns,
    and an exact tie (tests/imu_cases.py, proved by test_case_list_holds_what_it_claims); the 2000-sample covariance has cond 1.3e11."""
    names = [n for n in covariances() if n[9:] not in NO_SQRT_INFO]
    assert len(names) == 17
    got = device_sqrt_info(solver, [covariances()[n] for n in names])
    for n, S in zip(names, got):
        A = covariances()[n]
        _, hi, lo = sqrt_info_exact(n)
        S0 = oracle_sqrt_info(oracle, A)
        assert np.array_equal(S, np.triu(S)) and (np.diag(S) > 0).all(), n
        dev = {"sqrt_info": dd_err(S, hi, lo), "defect": imu_exact.info_defect(S, A)}
        ref = {"sqrt_info": dd_err(S0, hi, lo), "defect": imu_exact.info_defect(S0, A)}
        assert_within(dev, ref, n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 9])
def test_device_sqrt_info_lane_groups(solver, n):
    """Factor k of a launch of n distinct matrices equals, bit for bit, the same matrix launched alone: lane groups 1-3, a second and third workgroup and the
    id >= n tail compute what lane group 0 computes."""
    names = [k for k in covariances() if k[9:] not in NO_SQRT_INFO]
    pick = [names[(3 * i + n) % len(names)] for i in range(n)]
    assert len(set(pick)) == n
    got = device_sqrt_info(solver, [covariances()[k] for k in pick])
    for i, k in enumerate(pick):
        alone = device_sqrt_info(solver, [covariances()[k]])[0]
        assert np.isfinite(alone).all() and np.array_equal(got[i], alone), (n, i, k)


def device_factor(solver, case):
    from vil_fusion_amd.estimator import BackendSolver
    o = solver.options if list(case["G"]) == list(solver.options.G[:]) else None
    s = solver
    if o is None:
        import copy
        o = copy.copy(solver.options); o.G[:] = list(case["G"])
        s = BackendSolver(o)
    try:
        pre = pre_struct(case["pre"])
        r, J, S = s.eval_imu_raw(case["params"], pre)
        rw, Jw = s.eval_imu(case["params"], pre)
    finally:
        if s is not solver:
            s.close()
    return r, local30(J), rw, local30(Jw), S


@pytest.mark.gpu
def test_device_factor_against_exact(solver, oracle, opts):
    """vilf_eval_imu_raw (residual, Jacobian blocks, sqrt_info) and vilf_eval_imu on every evaluation case, at 4 x the oracle's error + 16 ulp per group; the whitened
    residual must be the product of the two parts the raw hook returns."""
    for name, case in factor_cases().items():
        ex = factor_exact(name)
        r, J, rw, Jw, S = device_factor(solver, case)
        r0, J0, rw0, Jw0 = oracle_factor(oracle, opts, case)
        S0 = oracle_sqrt_info(oracle, case["pre"][abi.IMU_OFF["covariance"][0]:])
        for a in (r, J, rw, Jw, S):
            assert np.isfinite(a).all(), name
        assert_within(factor_errors(ex, r, J, rw, Jw, S), factor_errors(ex, r0, J0, rw0, Jw0, S0), name)
        assert np.abs(rw - S @ r).max() <= 1e-12 * max(1.0, np.abs(rw).max()), name


@pytest.mark.gpu
def test_device_intervals_without_sqrt_info(solver, oracle, opts):
    """The zero-sample, the zero-noise and the one-sample interval have a singular covariance (exactly zero for the first two; rank 12 for the third: see
    NO_SQRT_INFO). Raw residual and raw Jacobians are still exact; sqrt_info is what include/vilfusion.h states: no error, and for a zero covariance NaN in
    the whole upper triangle (zeros below it)."""
    rows = rows_f64()
    for k, name in enumerate(NO_SQRT_INFO):
        case = imu_cases._state(np.random.default_rng(700 + k), rows[name], imu_cases.G)
        r_ex, J_ex = imu_exact.imu_raw_exact(case["params"], case["pre"], case["G"])
        ex = {"r": imu_exact.to_dd(r_ex), "J": tuple(a.reshape(15, 30) for a in imu_exact.to_dd([x for row in J_ex for x in row]))}
        pre = pre_struct(case["pre"])
        r, J, S = solver.eval_imu_raw(case["params"], pre)
        r0, J0 = oracle.eval_factor("imu_raw", opts, case["params"], pre, sizes=[7, 9, 7, 9], nres=15)
        assert np.isfinite(r).all() and all(np.isfinite(j).all() for j in J), name
        assert_within(factor_errors(ex, r, local30(J)), factor_errors(ex, r0, local30(J0)), name)
        if name in imu_cases.SINGULAR:
            iu = np.triu_indices(15)
            assert np.isnan(S[iu]).all() and not S[np.tril_indices(15, -1)].any(), name
            assert np.isnan(device_sqrt_info(solver, [np.zeros((15, 15))])[0][iu]).all()


@pytest.mark.gpu
def test_validity_gate_boundary(solver, oracle, opts):
    """estimator.cpp:745 skips an IMU factor whose sum_dt > 10.0: a window whose imu[1].sum_dt is exactly 10.0 keeps the factor, one at the next double above
    drops it. Each initial cost against the oracle's at 1e-9 relative, and the two costs differ."""
    from vil_fusion_amd import synth
    costs = []
    for T in (10.0, float(np.nextafter(10.0, 11.0))):
        win, _, _ = synth.make_window(77, opts, synth.SynthConfig(n_features=20, with_prior=False))
        win.imu[1, 0] = T
        solver.set_prior(None)
        got = solver.optimization(win)
        ref = oracle.window_solve(opts, win, None)
        print("sum_dt %r: initial cost device %r oracle %r" % (T, got.summary["initial_cost"], ref.summary["initial_cost"]))
        assert abs(got.summary["initial_cost"] - ref.summary["initial_cost"]) <= 1e-9 * ref.summary["initial_cost"]
        costs.append(got.summary["initial_cost"])
    assert costs[0] != costs[1] and costs[0] > costs[1]
