"""Plain high-precision reference of the pose-graph Gauss-Newton step (TEST INFRASTRUCTURE), written from the definitions in mpmath at 40 digits.

It shares no closed form with oracle/pose_graph.cpp or vilf_pg.hip beyond Rodrigues' exp and log: no series branch (40 digits need none), no
LogmapDerivative, no Q, no adjoint. The Jacobians are central differences in mp (h = 1e-15: truncation ~1e-30, rounding ~1e-25), the normal
equations are dense and solved by mp.cholesky_solve — no chain Cholesky, no Woodbury.

  pose          (R, t), mp.matrix 3x3 / 3x1, from float64 [qx qy qz qw tx ty tz] (quaternion normalised in mp)
  tangent       [omega, v] (gtsam Pose3), retract T * Exp(delta)
  between       e = Log(meas^-1 Ti^-1 Tj), whitened by 1 / sigma; Robust(Cauchy(1)): w = 1 / (1 + r^2) on J^T J and J^T e, cost log(1 + r^2) / 2
  prior         the same expression with Ti = the prior pose, meas = identity, only node 0 free
An mp-solved graph costs ~0.1 s per key frame and step: keep K <= 24."""
import functools

import mpmath as mp
import numpy as np

DPS = 40
H = mp.mpf(10) ** -15


def _hp(fn):
    """run at 40 digits without touching the process-wide mp context"""
    @functools.wraps(fn)
    def wrapped(*a, **kw):
        with mp.workdps(DPS):
            return fn(*a, **kw)
    return wrapped


def _skew(w):
    return mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def _vec(v):
    return mp.matrix([mp.mpf(float(a)) if not isinstance(a, mp.mpf) else a for a in v])


@_hp
def from_qt(p):
    x, y, z, w = [mp.mpf(float(v)) for v in p[:4]]
    n = mp.sqrt(x * x + y * y + z * z + w * w)
    x, y, z, w = x / n, y / n, z / n, w / n
    R = mp.matrix([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                   [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return R, mp.matrix([mp.mpf(float(v)) for v in p[4:7]])


def compose(a, b):
    return a[0] * b[0], a[0] * b[1] + a[1]


def inverse(a):
    Rt = a[0].T
    return Rt, -(Rt * a[1])


@_hp
def se3_exp(xi):
    xi = _vec(xi)
    w, v = xi[0:3], xi[3:6]
    th2 = w[0] ** 2 + w[1] ** 2 + w[2] ** 2
    if th2 == 0:
        return mp.eye(3), mp.matrix(v)
    th = mp.sqrt(th2)
    a, b, c = mp.sin(th) / th, (1 - mp.cos(th)) / th2, (th - mp.sin(th)) / (th2 * th)
    W = _skew(w); WW = W * W
    return mp.eye(3) + a * W + b * WW, (mp.eye(3) + b * W + c * WW) * mp.matrix(v)


@_hp
def se3_log(T):
    """valid away from a rotation by pi"""
    R, t = T
    v = mp.matrix([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])       # vee(R - R^T) = 2 sin(theta) axis
    s = mp.sqrt(v[0] ** 2 + v[1] ** 2 + v[2] ** 2) / 2
    out = mp.zeros(6, 1)
    if s == 0:
        out[3], out[4], out[5] = t[0], t[1], t[2]
        return out
    th = mp.atan2(s, (R[0, 0] + R[1, 1] + R[2, 2] - 1) / 2)
    w = v * (th / (2 * s))
    W = _skew(w)
    u = (mp.eye(3) - W / 2 + (1 / th ** 2 - (1 + mp.cos(th)) / (2 * th * mp.sin(th))) * (W * W)) * t
    for k in range(3):
        out[k], out[3 + k] = w[k], u[k]
    return out


def _error(Ti, Tj, meas_inv):
    return se3_log(compose(meas_inv, compose(inverse(Ti), Tj)))


def _delta(k, sign):
    d = mp.zeros(6, 1); d[k] = sign * H
    return se3_exp(d)


def _factor(Ti, Tj, meas, sigma, robust, free_i=True):
    """whitened residual e (6x1), Jacobians A = de / d delta_i, B = de / d delta_j (central differences), Cauchy weight, cost"""
    mi = inverse(meas)
    e = _error(Ti, Tj, mi)
    A, B = mp.zeros(6, 6), mp.zeros(6, 6)
    for k in range(6):
        Ep, Em = _delta(k, 1), _delta(k, -1)
        if free_i:
            da = (_error(compose(Ti, Ep), Tj, mi) - _error(compose(Ti, Em), Tj, mi)) / (2 * H)
        db = (_error(Ti, compose(Tj, Ep), mi) - _error(Ti, compose(Tj, Em), mi)) / (2 * H)
        for r in range(6):
            if free_i:
                A[r, k] = da[r] / sigma[r]
            B[r, k] = db[r] / sigma[r]
    r2 = mp.mpf(0)
    for r in range(6):
        e[r] = e[r] / sigma[r]; r2 += e[r] ** 2
    if robust:
        return e, A, B, 1 / (1 + r2), mp.log(1 + r2) / 2
    return e, A, B, mp.mpf(1), r2 / 2


def _factor_cost(Ti, Tj, meas, sigma, robust):
    e = _error(Ti, Tj, inverse(meas))
    r2 = sum((e[r] / sigma[r]) ** 2 for r in range(6))
    return mp.log(1 + r2) / 2 if robust else r2 / 2


def _sig(s):
    return [mp.mpf(float(v)) for v in s]


def _ident():
    return mp.eye(3), mp.zeros(3, 1)


@_hp
def cost(x, prior, prior_sigma, edges):
    c = _factor_cost(prior, x[0], _ident(), _sig(prior_sigma), 0)
    for (i, j, q, t, sg, rb) in edges:
        c += _factor_cost(x[i], x[j], from_qt(list(q) + list(t)), _sig(sg), rb)
    return c


@_hp
def step(x, prior, prior_sigma, edges):
    """one Gauss-Newton step on mp poses: (x_new, cost at x)"""
    K = len(x)
    Hm, g = mp.zeros(6 * K, 6 * K), mp.zeros(6 * K, 1)

    def add(i, Ji, j, Jj, w):
        for (a, Ja) in ((i, Ji), (j, Jj)):
            if Ja is None:
                continue
            for (b, Jb) in ((i, Ji), (j, Jj)):
                if Jb is None:
                    continue
                blk = (Ja.T * Jb) * w
                for r in range(6):
                    for c in range(6):
                        Hm[6 * a + r, 6 * b + c] += blk[r, c]

    e, _, B, w, c = _factor(prior, x[0], _ident(), _sig(prior_sigma), 0, free_i=False)
    total = c
    add(0, None, 0, B, w)
    gb = (B.T * e) * w
    for r in range(6):
        g[r] -= gb[r]
    for (i, j, q, t, sg, rb) in edges:
        e, A, B, w, c = _factor(x[i], x[j], from_qt(list(q) + list(t)), _sig(sg), rb)
        total += c
        add(i, A, j, B, w)
        ga, gb = (A.T * e) * w, (B.T * e) * w
        for r in range(6):
            g[6 * i + r] -= ga[r]; g[6 * j + r] -= gb[r]
    d = mp.cholesky_solve(Hm, g)
    return [compose(x[k], se3_exp(d[6 * k: 6 * k + 6])) for k in range(K)], total


@_hp
def run(x0, prior_sigma, edges, iters):
    """`iters` Gauss-Newton steps from float64 poses x0 (n, 7), the prior on node 0 at x0[0]: (mp poses, cost at them)"""
    x = [from_qt(p) for p in x0]
    prior = x[0]
    for _ in range(iters):
        x, _ = step(x, prior, prior_sigma, edges)
    return x, cost(x, prior, prior_sigma, edges)


@_hp
def deviation(x_ref, poses_qt):
    """(max |dt| in metres, max rotation angle in rad) of float64 poses (n, 7) against mp poses, as floats"""
    dt = dr = mp.mpf(0)
    for (R, t), p in zip(x_ref, poses_qt):
        Rp, tp = from_qt(p)
        d = tp - t
        dt = max(dt, mp.sqrt(d[0] ** 2 + d[1] ** 2 + d[2] ** 2))
        w = se3_log((R.T * Rp, mp.zeros(3, 1)))
        dr = max(dr, mp.sqrt(w[0] ** 2 + w[1] ** 2 + w[2] ** 2))
    return float(dt), float(dr)


@_hp
def exp_qt(xi):
    """Exp(xi) as a float64 pose [qx qy qz qw tx ty tz] (for building measurements)"""
    xi = _vec(xi)
    th = mp.sqrt(xi[0] ** 2 + xi[1] ** 2 + xi[2] ** 2)
    s = mp.sin(th / 2) / th if th != 0 else mp.mpf(1) / 2
    _, t = se3_exp(xi)
    return np.array([float(s * xi[0]), float(s * xi[1]), float(s * xi[2]), float(mp.cos(th / 2)), float(t[0]), float(t[1]), float(t[2])])


@_hp
def to_matrix4(T):
    M = mp.eye(4)
    for r in range(3):
        M[r, 3] = T[1][r]
        for c in range(3):
            M[r, c] = T[0][r, c]
    return M
