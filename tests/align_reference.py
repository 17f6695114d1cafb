"""Plain exact reference of the visual-IMU alignment (TEST INFRASTRUCTURE), written from the definitions of VisualIMUAlignment
(initial/initial_aligment.cpp:3-207) in mpmath at 40 digits. It covers the alignment algebra only: the pre-integrated intervals (delta_p, delta_v,
delta_q, sum_dt, d delta_q / d bg) are inputs, taken from vilf_imu_preint rows; pre-integration has tests of its own.

It shares no structure with oracle/initial_alignment.cpp or vilf_init.hip: no 3 x 3 or 10 x 10 blocks, no scatter, no running sums, no LDLT.

  gyro bias        the 3 (n - 1) x 3 stack  J_k x = 2 vec(dq_k^-1 (x) q(R_i^T R_j)),  least squares by mp.qr_solve. The quaternion of a rotation is taken
                   from its axis and angle (w = cos(theta / 2) >= 0), which is the reference's conversion while trace(R) > 0 (rotations below 120 degrees)
  LinearAlignment  the tall 6 (n - 1) x (3 n + 4) matrix, one position and one velocity equation per interval and axis, unknowns [v_0 .. v_{n-1}, g, 100 s]
  RefineGravity    the reference never clears A and b between its 4 sweeps and multiplies them by 1000 after each, so sweep k solves the weighted least
                   squares problem over the stacked rows of sweeps 1 .. k, sweep j weighted by 1000^(k - j + 1) and built with its own g0 and tangent basis;
                   unknowns [v_0 .. v_{n-1}, w1, w2, 100 s]. g0 is renormalised to |G| after each sweep
  gates            ||g| - |G|| > 1 or s < 0 after LinearAlignment: refused, x has 3 n + 4 entries, scale not divided; otherwise x has 3 n + 3 entries, the
                   last divided by 100, and ok = not (s < 0)

The normal equations are block-tridiagonal plus an arrow and are kept sparse. A column that is identically zero (no translation at all: the scale column)
has an exactly zero pivot; the reference's LDLT returns 0 for it, and so does solve_normal. The solve factors the Jacobi-scaled matrix once in float64 and
refines with the residual computed in mp until it is below 1e-30 of the right-hand side, which it asserts. With n = 3 LinearAlignment has 13 unknowns and 12
equations: its answer is not determined by the mathematics (the reference returns whatever rounding leaves in the last pivot), and align() says so by
raising Underdetermined; the gyro bias of such a case is still available from gyro_bias()."""
import functools

import mpmath as mp
import numpy as np

DPS = 40
RESIDUAL = mp.mpf(10) ** -30

# columns of a vilf_imu_preint row (include/vilfusion.h): sum_dt, delta_p[3], delta_q[4] (x y z w), delta_v[3], linearized_ba[3], linearized_bg[3], jacobian[15 x 15]
_SUM_DT, _DP, _DQ, _DV, _JAC = 0, 1, 4, 8, 17
_O_R, _O_BG = 3, 12


class Underdetermined(Exception):
    pass


def _hp(fn):
    """run at 40 digits without touching the process-wide mp context"""
    @functools.wraps(fn)
    def wrapped(*a, **kw):
        with mp.workdps(DPS):
            return fn(*a, **kw)
    return wrapped


def _f(v):
    return mp.mpf(float(v))


def _mat(a):
    return [[_f(a[r][c]) for c in range(3)] for r in range(3)]


def _vec(a):
    return [_f(v) for v in a]


def _mtm(A, B):
    """A^T B"""
    return [[sum(A[k][r] * B[k][c] for k in range(3)) for c in range(3)] for r in range(3)]


def _mtv(A, v):
    """A^T v"""
    return [sum(A[k][r] * v[k] for k in range(3)) for r in range(3)]


def _norm(v):
    return mp.sqrt(sum(a * a for a in v))


def _quat_of_rotation(R):
    """(w, x, y, z) of a rotation matrix by axis and angle; valid below a rotation by pi"""
    v = [R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]]                    # 2 sin(theta) axis
    s = _norm(v) / 2
    if s == 0:
        return [mp.mpf(1), mp.mpf(0), mp.mpf(0), mp.mpf(0)]
    th = mp.atan2(s, (R[0][0] + R[1][1] + R[2][2] - 1) / 2)
    k = mp.sin(th / 2) / (2 * s)
    return [mp.cos(th / 2), v[0] * k, v[1] * k, v[2] * k]


def _quat_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return [aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw]


def _quat_inv(q):
    n2 = sum(a * a for a in q)
    return [q[0] / n2, -q[1] / n2, -q[2] / n2, -q[3] / n2]


@_hp
def gyro_bias(frame_R, pre):
    """solveGyroscopeBias: delta_bg (3 mp numbers) from the intervals as first integrated (at their linearisation biases)"""
    n = len(frame_R)
    rows, rhs = [], []
    for k in range(n - 1):
        q_ij = _quat_of_rotation(_mtm(_mat(frame_R[k]), _mat(frame_R[k + 1])))
        dq = [_f(pre[k][_DQ + 3]), _f(pre[k][_DQ]), _f(pre[k][_DQ + 1]), _f(pre[k][_DQ + 2])]
        e = _quat_mul(_quat_inv(dq), q_ij)
        for r in range(3):
            rows.append([_f(pre[k][_JAC + (_O_R + r) * 15 + _O_BG + c]) for c in range(3)])
            rhs.append(2 * e[1 + r])
    x = mp.qr_solve(mp.matrix(rows), mp.matrix(rhs))[0]
    return [x[0], x[1], x[2]]


@_hp
def tangent_basis(g0):
    """TangentBasis: two unit vectors spanning the plane normal to g0; the helper axis is z, or x when g0 / |g0| is exactly (0, 0, 1)"""
    g0 = [a if isinstance(a, mp.mpf) else _f(a) for a in g0]
    n = _norm(g0)
    a = [v / n for v in g0]
    t = [mp.mpf(0), mp.mpf(0), mp.mpf(1)]
    if a[0] == 0 and a[1] == 0 and a[2] == 1:
        t = [mp.mpf(1), mp.mpf(0), mp.mpf(0)]
    d = sum(a[k] * t[k] for k in range(3))
    u = [t[k] - a[k] * d for k in range(3)]
    un = _norm(u)
    b = [v / un for v in u]
    c = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    return b, c


def _interval_rows(n, R, T, pre, TIC, g0=None, basis=None):
    """the 6 (n - 1) equations as (dict column -> coefficient, right-hand side). g0 is None: LinearAlignment, gravity columns 3 n .. 3 n + 2, scale column
    3 n + 3; otherwise RefineGravity about g0: tangent columns 3 n, 3 n + 1, scale column 3 n + 2."""
    out = []
    sc = 3 * n + (3 if g0 is None else 2)
    for i in range(n - 1):
        Ri, Rj = R[i], R[i + 1]
        dt = _f(pre[i][_SUM_DT])
        dp, dv = [_f(pre[i][_DP + r]) for r in range(3)], [_f(pre[i][_DV + r]) for r in range(3)]
        RR = _mtm(Ri, Rj)
        dT = _mtv(Ri, [T[i + 1][r] - T[i][r] for r in range(3)])
        lever = [sum(RR[r][c] * TIC[c] for c in range(3)) - TIC[r] for r in range(3)]
        for r in range(3):
            RiT_r = [Ri[c][r] for c in range(3)]                                    # row r of R_i^T
            # position: -dt v_i + R_i^T dt^2 / 2 g + R_i^T (T_j - T_i) / 100 (100 s) = delta_p + R_i^T R_j TIC - TIC
            # velocity: -v_i + R_i^T R_j v_j + R_i^T dt g = delta_v
            pos, vel = {3 * i + r: -dt, sc: dT[r] / 100}, {3 * i + r: mp.mpf(-1)}
            for c in range(3):
                vel[3 * (i + 1) + c] = RR[r][c]
            bp, bv = dp[r] + lever[r], dv[r]
            if g0 is None:
                for c in range(3):
                    pos[3 * n + c] = RiT_r[c] * dt * dt / 2
                    vel[3 * n + c] = RiT_r[c] * dt
            else:
                for k, l in enumerate(basis):
                    pos[3 * n + k] = sum(RiT_r[c] * l[c] for c in range(3)) * dt * dt / 2
                    vel[3 * n + k] = sum(RiT_r[c] * l[c] for c in range(3)) * dt
                bp -= sum(RiT_r[c] * g0[c] for c in range(3)) * dt * dt / 2
                bv -= sum(RiT_r[c] * g0[c] for c in range(3)) * dt
            out.append((pos, bp))
            out.append((vel, bv))
    return out


def _normal_equations(ns, rows):
    """N = sum a a^T over the rows as a list of dict rows, y = sum a rhs"""
    N, y = [dict() for _ in range(ns)], [mp.mpf(0)] * ns
    for coef, rhs in rows:
        items = list(coef.items())
        for (a, va) in items:
            y[a] += va * rhs
            Na = N[a]
            for (b, vb) in items:
                Na[b] = Na.get(b, 0) + va * vb
    return N, y


def _weighted(parts):
    """sum of w (N, y) over parts [(w, (N, y))]: the normal equations of the stacked rows, each stack weighted by w"""
    ns = len(parts[0][1][0])
    N, y = [dict() for _ in range(ns)], [mp.mpf(0)] * ns
    for w, (Nj, yj) in parts:
        for a in range(ns):
            y[a] += w * yj[a]
            for b, v in Nj[a].items():
                N[a][b] = N[a].get(b, 0) + w * v
    return N, y


def solve_normal(N, y):
    """x with N x = y for the sparse symmetric positive definite N (list of dict rows); 0 where a column of the tall system is identically zero.
    One float64 factorisation of the Jacobi-scaled matrix, refined with the mp residual down to RESIDUAL of |y|, asserted."""
    ns = len(N)
    keep = [i for i in range(ns) if N[i].get(i, 0) != 0]
    pos = {i: k for k, i in enumerate(keep)}
    d = [1 / mp.sqrt(N[i][i]) for i in keep]
    S = [{pos[j]: v * d[pos[i]] * d[pos[j]] for j, v in N[i].items() if j in pos} for i in keep]
    z = [y[i] * d[pos[i]] for i in keep]
    m = len(keep)
    Sf = np.zeros((m, m))
    for i, row in enumerate(S):
        for j, v in row.items():
            Sf[i, j] = float(v)
    Sinv = np.linalg.inv(Sf)
    zmax = max([abs(v) for v in z] + [mp.mpf(0)])
    x = [mp.mpf(0)] * m
    if zmax != 0:
        for it in range(40):
            r = [z[i] - sum(v * x[j] for j, v in S[i].items()) for i in range(m)]
            rel = max(abs(v) for v in r) / zmax
            if rel < RESIDUAL:
                break
            # the correction in float64, on the residual scaled into range
            c = Sinv @ np.array([float(v / (rel * zmax)) for v in r])
            x = [x[i] + _f(c[i]) * rel * zmax for i in range(m)]
        assert rel < RESIDUAL, "iterative refinement stalled at a relative residual of %s" % mp.nstr(rel, 5)
    out = [mp.mpf(0)] * ns
    for i in keep:
        out[i] = x[pos[i]] * d[pos[i]]
    return out


@_hp
def tall_system(frame_R, frame_T, pre, TIC):
    """LinearAlignment's tall matrix and right-hand side as dense mp matrices (for a cross-check with mp.qr_solve on a small case)"""
    n = len(frame_R)
    rows = _interval_rows(n, [_mat(a) for a in frame_R], [_vec(a) for a in frame_T], pre, _vec(TIC))
    A, b = mp.zeros(len(rows), 3 * n + 4), mp.zeros(len(rows), 1)
    for k, (coef, rhs) in enumerate(rows):
        b[k] = rhs
        for c, v in coef.items():
            A[k, c] = v
    return A, b


@_hp
def linear_alignment(frame_R, frame_T, pre, TIC):
    """the 3 n + 4 unknowns of LinearAlignment (mp), scale column still times 100"""
    n = len(frame_R)
    if 6 * (n - 1) < 3 * n + 4:
        raise Underdetermined("LinearAlignment with %d frames: %d equations for %d unknowns" % (n, 6 * (n - 1), 3 * n + 4))
    rows = _interval_rows(n, [_mat(a) for a in frame_R], [_vec(a) for a in frame_T], pre, _vec(TIC))
    return solve_normal(*_normal_equations(3 * n + 4, rows))


@_hp
def align(frame_R, frame_T, pre, TIC, Gnorm):
    """LinearAlignment, its gate, RefineGravity and the last gate on the re-integrated intervals `pre`: dict(ok, g, x) of mp numbers, shaped and scaled
    as the reference leaves them in each case"""
    n = len(frame_R)
    x = linear_alignment(frame_R, frame_T, pre, TIC)
    R, T, tic, G = [_mat(a) for a in frame_R], [_vec(a) for a in frame_T], _vec(TIC), _f(Gnorm)
    g = x[3 * n: 3 * n + 3]
    if abs(_norm(g) - G) > 1 or x[-1] / 100 < 0:
        return dict(ok=False, g=g, x=x)
    gn = _norm(g)
    g0 = [v / gn * G for v in g]
    sweeps = []
    for k in range(1, 5):
        basis = tangent_basis(g0)
        sweeps.append(_normal_equations(3 * n + 3, _interval_rows(n, R, T, pre, tic, g0, basis)))
        x = solve_normal(*_weighted([(mp.mpf(1000) ** (k - j + 1), sweeps[j - 1]) for j in range(1, k + 1)]))
        gk = [g0[c] + basis[0][c] * x[3 * n] + basis[1][c] * x[3 * n + 1] for c in range(3)]
        gn = _norm(gk)
        g0 = [v / gn * G for v in gk]
    x[-1] = x[-1] / 100
    return dict(ok=not x[-1] < 0, g=g0, x=x)


@_hp
def deviation(exact, values):
    """largest |float64 value - exact value| over the entries, as a float"""
    return float(max(abs(_f(v) - e) for e, v in zip(exact, values)))


@_hp
def max_abs(exact):
    return float(max(abs(e) for e in exact))
