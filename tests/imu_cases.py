"""Case list of the IMU tests (tests/test_imu_exact.py, tests/golden/make_imu_exact.py): pre-integration intervals, covariances for sqrt_info,
IMU factor evaluations. Each case is the smallest that can still go wrong. Inputs are built from numpy's PCG64 uniform stream and
+ - * / sqrt only (no libm), so they are the same floats everywhere; the fixture stores a digest of every interval's inputs."""
import hashlib
from collections import OrderedDict
import numpy as np

NOISE = (0.08, 0.004, 0.00004, 2.0e-6)            # acc_n, gyr_n, acc_w, gyr_w
DT_SET = np.array([0.004, 0.005, 0.0051, 0.01])
G = np.array([0.0, 0.0, 9.8])
G3 = np.array([0.35, -0.21, 9.79])                # "G with three non-zero components"
REGEN_MAX_SAMPLES = 40                            # intervals up to this size are recomputed in-process by the CPU test
# cos / sin of 89.5 and 90.5 degrees (half of 179 / 181), as literals
C895, S895 = 0.008726535498373935, 0.9999619230641713
C905, S905 = -0.008726535498373935, 0.9999619230641713


# ---- arithmetic-only quaternion helpers (x y z w) -------------------------------------------------------------------------------
def qmul(a, b):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
                     a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
                     a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def qnorm(q):
    q = np.asarray(q, dtype=np.float64)
    return q / np.sqrt(np.sum(q * q))


def qrot(q, v):
    u = q[:3]
    uv = 2.0 * np.cross(u, v)
    return v + q[3] * uv + np.cross(u, uv)


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.sqrt(np.sum(v * v))


# ---- pre-integration intervals ---------------------------------------------------------------------------------------------------
def _interval(seed, n, dt=None, acc_scale=1.0, gyr_scale=0.2, ba=0.02, bg=0.002, noise=NOISE, gyr=None):
    rng = np.random.default_rng(seed)
    u = lambda *shape: 2.0 * rng.random(shape) - 1.0
    acc_all = acc_scale * u(n + 1, 3) + G
    gyr_all = gyr_scale * u(n + 1, 3) if gyr is None else gyr(rng, n + 1)
    dts = DT_SET[rng.integers(0, 4, n)] if dt is None else np.asarray(dt, dtype=np.float64)
    assert dts.shape == (n,)
    return dict(noise=tuple(noise), acc_0=acc_all[0].copy(), gyr_0=gyr_all[0].copy(), ba=ba * u(3), bg=bg * u(3),
                dt=dts.copy(), acc=acc_all[1:].copy(), gyr=gyr_all[1:].copy())


def _with_dt(seed, n, at, value):
    rng = np.random.default_rng(1000 + seed)
    dts = DT_SET[rng.integers(0, 4, n)]
    dts[at] = value
    return _interval(seed, n, dt=dts)


def _gyro8_fixed(rng, m):
    return np.tile(8.0 * _unit([1.0, 2.0, -2.0]), (m, 1))


def _gyro8_moving(rng, m):
    a = 2.0 * rng.random((m, 3)) - 1.0 + np.array([0.0, 0.0, 1.5])       # axes spread around +z, so the turn accumulates
    return 8.0 * a / np.sqrt(np.sum(a * a, axis=1))[:, None]


def _dt_one_second():
    return np.tile(DT_SET, 42)[:166]                                     # 41 * 0.0241 + 0.004 + 0.005 = 0.9971 s


def intervals():
    """name -> dict(noise, acc_0, gyr_0, ba, bg, dt[n], acc[n][3], gyr[n][3]); dt is non-uniform from DT_SET unless the name says otherwise"""
    c = OrderedDict()
    for k, n in enumerate((0, 1, 2, 3, 20, 200)):
        c["n%d" % n] = _interval(10 + k, n)
    c["n2000_5ms"] = _interval(16, 2000, dt=np.full(2000, 0.005))        # sum_dt = 10 up to rounding: the validity limit
    c["zero_dt_mid"] = _with_dt(20, 5, 2, 0.0)                           # duplicate stamp
    c["dt_1e-6"] = _with_dt(21, 5, 3, 1e-6)
    c["dt_0.1"] = _with_dt(22, 5, 1, 0.1)
    c["gyro8_fixed_axis"] = _interval(23, 166, dt=_dt_one_second(), gyr=_gyro8_fixed)
    c["gyro8_moving_axis"] = _interval(24, 166, dt=_dt_one_second(), gyr=_gyro8_moving)
    c["bias_0.5_0.05"] = _interval(25, 20, ba=0.5, bg=0.05)
    c["bias_0.5_0.05"]["ba"] = 0.5 * _unit(c["bias_0.5_0.05"]["ba"]); c["bias_0.5_0.05"]["bg"] = 0.05 * _unit(c["bias_0.5_0.05"]["bg"])
    c["zero_noise"] = _interval(26, 20, noise=(0.0, 0.0, 0.0, 0.0))
    c["acc_50"] = _interval(27, 20, acc_scale=50.0)
    return c


# the two intervals whose covariance is exactly zero: no finite sqrt_info, no finite whitened output
SINGULAR = ("n0", "zero_noise")


def digest(case):
    h = hashlib.sha256()
    for k in ("noise", "acc_0", "gyr_0", "ba", "bg", "dt", "acc", "gyr"):
        h.update(np.ascontiguousarray(case[k], dtype=np.float64).tobytes())
    return h.hexdigest()


def padded_batch(cases, max_samples, fill=np.nan):
    """the arrays of vilf_imu_preintegrate_batch for a list of interval dicts: every slot behind n_samples[i] holds `fill`"""
    n = len(cases)
    ns = np.array([len(c["dt"]) for c in cases], dtype=np.int32)
    assert ns.max(initial=0) <= max_samples
    dt = np.full((n, max_samples), fill); acc = np.full((n, max_samples, 3), fill); gyr = np.full((n, max_samples, 3), fill)
    for i, c in enumerate(cases):
        dt[i, :ns[i]] = c["dt"]; acc[i, :ns[i]] = c["acc"]; gyr[i, :ns[i]] = c["gyr"]
    stack = lambda k: np.array([c[k] for c in cases], dtype=np.float64).reshape(n, 3)
    return dict(acc_0=stack("acc_0"), gyr_0=stack("gyr_0"), ba=stack("ba"), bg=stack("bg"), n_samples=ns, dt=dt, acc=acc, gyr=gyr)


# ---- covariances for sqrt_info ---------------------------------------------------------------------------------------------------
def _dcd(d, pairs):
    """D C D: C = identity plus the listed correlations (i, j, c); symmetric by construction"""
    d = np.asarray(d, dtype=np.float64)
    A = np.diag(d * d)
    for i, j, c in pairs:
        A[i, j] = A[j, i] = (d[i] * d[j]) * c
    return A


def constructed_covariances():
    """name -> (15 x 15 SPD matrix, expected pivot property). Diagonal scales 1e-9 .. 1e-2. Column k of PartialPivLU swaps when a later row holds
    a larger entry: d_j c_jk > d_k for a pair (k, j) of a small and a large scale."""
    ramp = np.array([10.0 ** (-9 + e / 2.0) for e in range(15)])         # 1e-9 .. 1e-2
    mid = np.full(15, 1e-5)
    c = OrderedDict()
    c["diagonal"] = (_dcd(ramp, []), dict(swaps=[]))
    d = mid.copy(); d[0], d[1] = 1e-9, 1e-2
    c["swap_col0"] = (_dcd(d, [(0, 1, 0.5)]), dict(swaps=[0]))
    d = mid.copy(); d[13], d[14] = 1e-8, 1e-3
    c["swap_col13"] = (_dcd(d, [(13, 14, 0.5)]), dict(swaps=[13]))
    d = ramp.copy(); pairs = []
    for k in (0, 2, 4, 6, 8):
        d[k], d[k + 1] = 1e-9 * (k + 1), 1e-3 * (k + 1); pairs.append((k, k + 1, 0.5 if k % 4 else -0.5))
    c["swap_five"] = (_dcd(d, pairs), dict(swaps=[0, 2, 4, 6, 8]))
    d = np.array([2.0 ** (-10 - (k % 5)) for k in range(15)]); d[0], d[1] = 2.0 ** -20, 2.0 ** -10
    c["tie_col0"] = (_dcd(d, [(0, 1, 2.0 ** -10)]), dict(swaps=[], tie=0))            # a00 = a10 = 2^-40 exactly: the first row keeps the pivot
    return c


# ---- IMU factor evaluations ------------------------------------------------------------------------------------------------------
def _state(rng, pre, g, dba=0.0, dbg=0.0, qi_sign=1.0, qj_sign=None, q_res=None, far=0.0, sum_dt=None):
    """parameter blocks around a pre-integration row: frame j sits where the row predicts it, up to small offsets and the residual rotation q_res"""
    pre = np.array(pre, dtype=np.float64)
    if sum_dt is not None:
        pre[0] = sum_dt
    u = lambda *shape: 2.0 * rng.random(shape) - 1.0
    T, dp, dq, dv = pre[0], pre[1:4], pre[4:8], pre[8:11]
    Qi = qnorm(u(4)); Qi = Qi * (qi_sign * (1.0 if Qi[3] > 0 else -1.0))
    Pi = 3.0 * u(3) + far * _unit([2.0, -1.0, 0.5]); Vi = 2.0 * u(3)
    Bai = pre[11:14] + dba * _unit(u(3)); Bgi = pre[14:17] + dbg * _unit(u(3))
    Pj = Pi + Vi * T - 0.5 * g * T * T + qrot(Qi, dp) + 0.01 * u(3)
    Vj = Vi - g * T + qrot(Qi, dv) + 0.01 * u(3)
    small = qnorm(np.concatenate([0.005 * u(3), [1.0]])) if q_res is None else qnorm(q_res)
    Qj = qnorm(qmul(qmul(Qi, dq), small))                              # sign as the product gives it, unless the case forces one
    if qj_sign is not None:
        Qj = Qj * (qj_sign * (1.0 if Qj[3] > 0 else -1.0))
    Baj = Bai + 1e-3 * u(3); Bgj = Bgi + 1e-4 * u(3)
    params = [np.concatenate([Pi, Qi]), np.concatenate([Vi, Bai, Bgi]), np.concatenate([Pj, Qj]), np.concatenate([Vj, Baj, Bgj])]
    return dict(params=params, pre=pre, G=np.array(g, dtype=np.float64))


def factor_cases(rows):
    """rows: name -> 467 float64 (the exact pre-integration rows, rounded). name -> dict(params[4], pre[467], G[3])"""
    r20, r200, r2000 = rows["n20"], rows["n200"], rows["n2000_5ms"]
    ax = _unit([0.6, -0.3, 0.74])
    c = OrderedDict()
    mk = lambda seed, pre, g=G, **kw: _state(np.random.default_rng(500 + seed), pre, g, **kw)
    c["zero_bias_delta"] = mk(0, r200)
    c["bias_at_threshold"] = mk(1, r200, dba=0.1, dbg=0.01)              # imu_factor.h:53-54, the disabled repropagate thresholds
    c["bias_10x_threshold"] = mk(2, r200, dba=1.0, dbg=0.1)
    c["negative_w"] = mk(3, r200, qi_sign=-1.0, qj_sign=-1.0)
    c["negative_w_j_only"] = mk(4, r20, qj_sign=-1.0)
    c["residual_179deg"] = mk(5, r20, q_res=np.concatenate([S895 * ax, [C895]]))
    c["residual_181deg"] = mk(6, r20, q_res=np.concatenate([S905 * ax, [C905]]))
    c["far_5km"] = mk(7, r200, far=5000.0)
    c["sum_dt_0.05"] = mk(8, r20, sum_dt=0.05)
    c["sum_dt_10"] = mk(9, r2000)
    c["G_three_components"] = mk(10, r200, g=G3)
    c["gyro8_delta_q_negative_w"] = mk(11, rows["gyro8_fixed_axis"], dbg=0.01)
    return c
