"""Exact references for the IMU chain, restated from the reference's text in mpmath at 50 digits:
  preintegrate_exact   IntegrationBase::push_back / propagate / midPointIntegration   (factor/integration_base.h:30-158)
  sqrt_info_exact      LLT(covariance.inverse()).matrixL().transpose()                 (factor/imu_factor.h:64)
  pivot_sequence       the row choices of Eigen's PartialPivLU (what covariance.inverse() runs for a 15 x 15 matrix)
  imu_raw_exact        IMUFactor::Evaluate before the multiplication by sqrt_info      (imu_factor.h:19-179, integration_base.h:160-186,
                       utility/utility.h deltaQ / Qleft / Qright)
  imu_whitened_exact   sqrt_info times the two outputs of imu_raw_exact
Inputs are the float64 values handed to the code under test, converted exactly. Nothing here is derived from the project's own
routines, its oracle or its data generator. Quaternions are (x, y, z, w) lists as in vilf_imu_preint; Eigen's conventions are kept:
a vector is rotated as v + w (2u x v) + u x (2u x v), the rotation matrix of an un-normalised quaternion comes from Eigen's
toRotationMatrix formula, inverse() is conjugate / squaredNorm.

Results travel as double-double pairs (hi = float(x), lo = float(x - hi), about 106 bits): to_dd / from_dd."""
import numpy as np
from mpmath import mp, mpf

mp.dps = 50
ZERO, ONE, TWO, HALF, QUARTER = mpf(0), mpf(1), mpf(2), mpf(0.5), mpf(0.25)
O_P, O_R, O_V, O_BA, O_BG = 0, 3, 6, 9, 12


def M(x):
    """float64 -> mpf, exactly"""
    return mpf(float(x))


def vec(a):
    return [M(x) for x in np.asarray(a, dtype=np.float64).ravel()]


def to_dd(values):
    """mpf values -> (hi, lo) float64 arrays"""
    flat = list(values)
    hi = np.array([float(x) for x in flat], dtype=np.float64)
    lo = np.array([float(x - mpf(h)) if np.isfinite(h) else 0.0 for x, h in zip(flat, hi)], dtype=np.float64)
    return hi, lo


def from_dd(hi, lo):
    """(hi, lo) float64 arrays -> list of mpf"""
    return [mpf(float(h)) + mpf(float(l)) for h, l in zip(np.ravel(hi), np.ravel(lo))]


# ---- 3-vectors, quaternions, 3 x 3 blocks (lists of mpf / lists of rows) -------------------------------------------------------
def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return [aw * bx + ax * bw + ay * bz - az * by,
            aw * by + ay * bw + az * bx - ax * bz,
            aw * bz + az * bw + ax * by - ay * bx,
            aw * bw - ax * bx - ay * by - az * bz]


def qinv(q):
    n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    return [-q[0] / n2, -q[1] / n2, -q[2] / n2, q[3] / n2]


def qrot(q, v):
    u = q[:3]
    uv = [TWO * c for c in cross(u, v)]
    uuv = cross(u, uv)
    return [v[k] + q[3] * uv[k] + uuv[k] for k in range(3)]


def q_to_R(q):
    x, y, z, w = q
    tx, ty, tz = TWO * x, TWO * y, TWO * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[ONE - (tyy + tzz), txy - twz, txz + twy],
            [txy + twz, ONE - (txx + tzz), tyz - twx],
            [txz - twy, tyz + twx, ONE - (txx + tyy)]]


def skew(v):
    return [[ZERO, -v[2], v[1]], [v[2], ZERO, -v[0]], [-v[1], v[0], ZERO]]


def eye3():
    return [[ONE if i == j else ZERO for j in range(3)] for i in range(3)]


def m3mul(a, b):
    return [[a[i][0] * b[0][j] + a[i][1] * b[1][j] + a[i][2] * b[2][j] for j in range(3)] for i in range(3)]


def m3add(a, b):
    return [[a[i][j] + b[i][j] for j in range(3)] for i in range(3)]


def m3scl(a, s):
    return [[a[i][j] * s for j in range(3)] for i in range(3)]


def m3vec(a, v):
    return [a[i][0] * v[0] + a[i][1] * v[1] + a[i][2] * v[2] for i in range(3)]


def _setb(A, r0, c0, b):
    for i in range(3):
        for j in range(3):
            A[r0 + i][c0 + j] = b[i][j]


def _matmul(A, B, n, m, p):
    """(n x m) (m x p); zero entries of A are skipped (exact: they contribute nothing)"""
    out = []
    for i in range(n):
        nz = [(k, A[i][k]) for k in range(m) if A[i][k] != 0]
        out.append([sum((a * B[k][j] for k, a in nz), ZERO) for j in range(p)])
    return out


def _transpose(A):
    return [list(r) for r in zip(*A)]


# ---- IntegrationBase ------------------------------------------------------------------------------------------------------------
def preintegrate_exact(noise, acc_0, gyr_0, ba, bg, dt, acc, gyr):
    """noise = (acc_n, gyr_n, acc_w, gyr_w). Returns the 467 fields of a vilf_imu_preint row as mpf."""
    acc_n, gyr_n, acc_w, gyr_w = [M(x) for x in noise]
    nz = [acc_n * acc_n] * 3 + [gyr_n * gyr_n] * 3 + [acc_n * acc_n] * 3 + [gyr_n * gyr_n] * 3 + [acc_w * acc_w] * 3 + [gyr_w * gyr_w] * 3
    a0, g0, ba, bg = vec(acc_0), vec(gyr_0), vec(ba), vec(bg)
    dts = vec(dt)
    accs = np.asarray(acc, dtype=np.float64).reshape(-1, 3)
    gyrs = np.asarray(gyr, dtype=np.float64).reshape(-1, 3)
    sum_dt = ZERO
    dp, dv, dq = [ZERO] * 3, [ZERO] * 3, [ZERO, ZERO, ZERO, ONE]
    J = [[ONE if i == j else ZERO for j in range(15)] for i in range(15)]
    P = [[ZERO] * 15 for _ in range(15)]
    I3 = eye3()
    for s, h in enumerate(dts):
        a1, g1 = vec(accs[s]), vec(gyrs[s])
        # midPointIntegration :63-71
        un_acc_0 = qrot(dq, [a0[k] - ba[k] for k in range(3)])
        un_gyr = [HALF * (g0[k] + g1[k]) - bg[k] for k in range(3)]
        rq = qmul(dq, [un_gyr[0] * h / TWO, un_gyr[1] * h / TWO, un_gyr[2] * h / TWO, ONE])
        un_acc_1 = qrot(rq, [a1[k] - ba[k] for k in range(3)])
        un_acc = [HALF * (un_acc_0[k] + un_acc_1[k]) for k in range(3)]
        rp = [dp[k] + dv[k] * h + HALF * un_acc[k] * h * h for k in range(3)]
        rv = [dv[k] + un_acc[k] * h for k in range(3)]
        # :75-120
        w_x = un_gyr
        a_0_x = [a0[k] - ba[k] for k in range(3)]
        a_1_x = [a1[k] - ba[k] for k in range(3)]
        R_w_x, R_a_0_x, R_a_1_x = skew(w_x), skew(a_0_x), skew(a_1_x)
        Rd, Rr = q_to_R(dq), q_to_R(rq)                      # result_delta_q is not normalised here
        ImRw = m3add(I3, m3scl(R_w_x, -h))
        RdA0, RrA1 = m3mul(Rd, R_a_0_x), m3mul(Rr, R_a_1_x)
        RrA1I = m3mul(RrA1, ImRw)
        F = [[ZERO] * 15 for _ in range(15)]
        _setb(F, 0, 0, I3)
        _setb(F, 0, 3, m3add(m3scl(RdA0, -QUARTER * h * h), m3scl(RrA1I, -QUARTER * h * h)))
        _setb(F, 0, 6, m3scl(I3, h))
        _setb(F, 0, 9, m3scl(m3add(Rd, Rr), -QUARTER * h * h))
        _setb(F, 0, 12, m3scl(RrA1, -QUARTER * h * h * -h))
        _setb(F, 3, 3, ImRw)
        _setb(F, 3, 12, m3scl(I3, -h))
        _setb(F, 6, 3, m3add(m3scl(RdA0, -HALF * h), m3scl(RrA1I, -HALF * h)))
        _setb(F, 6, 6, I3)
        _setb(F, 6, 9, m3scl(m3add(Rd, Rr), -HALF * h))
        _setb(F, 6, 12, m3scl(RrA1, -HALF * h * -h))
        _setb(F, 9, 9, I3)
        _setb(F, 12, 12, I3)
        V = [[ZERO] * 18 for _ in range(15)]
        V03 = m3scl(RrA1, -QUARTER * h * h * HALF * h)
        V63 = m3scl(RrA1, -HALF * h * HALF * h)
        _setb(V, 0, 0, m3scl(Rd, QUARTER * h * h)); _setb(V, 0, 3, V03); _setb(V, 0, 6, m3scl(Rr, QUARTER * h * h)); _setb(V, 0, 9, V03)
        _setb(V, 3, 3, m3scl(I3, HALF * h)); _setb(V, 3, 9, m3scl(I3, HALF * h))
        _setb(V, 6, 0, m3scl(Rd, HALF * h)); _setb(V, 6, 3, V63); _setb(V, 6, 6, m3scl(Rr, HALF * h)); _setb(V, 6, 9, V63)
        _setb(V, 9, 12, m3scl(I3, h)); _setb(V, 12, 15, m3scl(I3, h))
        # :124-125
        J = _matmul(F, J, 15, 15, 15)
        FP = _matmul(F, P, 15, 15, 15)
        FPFt = _transpose(_matmul(F, _transpose(FP), 15, 15, 15))           # (F (F P)^T)^T = F P F^T
        VN = [[V[i][k] * nz[k] for k in range(18)] for i in range(15)]
        VNVt = _matmul(VN, _transpose(V), 15, 18, 15)
        P = [[FPFt[i][j] + VNVt[i][j] for j in range(15)] for i in range(15)]
        # propagate :148-156
        nq = mp.sqrt(rq[0] * rq[0] + rq[1] * rq[1] + rq[2] * rq[2] + rq[3] * rq[3])
        dq = [c / nq for c in rq]
        dp, dv = rp, rv
        sum_dt = sum_dt + h
        a0, g0 = a1, g1
    return [sum_dt] + dp + dq + dv + ba + bg + [x for r in J for x in r] + [x for r in P for x in r]


# ---- sqrt_info ------------------------------------------------------------------------------------------------------------------
def _inverse(A):
    """Gauss-Jordan in mp at 120 digits, pivot = largest remaining entry of the column"""
    n = len(A)
    with mp.workdps(120):
        W = [[+A[i][j] for j in range(n)] + [ONE if i == j else ZERO for j in range(n)] for i in range(n)]
        for k in range(n):
            p = max(range(k, n), key=lambda i: abs(W[i][k]))
            if W[p][k] == 0:
                raise ZeroDivisionError("singular matrix")
            W[k], W[p] = W[p], W[k]
            piv = W[k][k]
            W[k] = [x / piv for x in W[k]]
            for i in range(n):
                if i != k and W[i][k] != 0:
                    f = W[i][k]
                    W[i] = [x - f * y for x, y in zip(W[i], W[k])]
        return [[+W[i][n + j] for j in range(n)] for i in range(n)]


def sqrt_info_exact(cov):
    """cov: 225 float64 (row-major). Returns U (15 rows of mpf), upper triangular, positive diagonal, U^T U = cov^-1.
    Raises ZeroDivisionError / ValueError for a singular or indefinite matrix."""
    A = [[M(x) for x in row] for row in np.asarray(cov, dtype=np.float64).reshape(15, 15)]
    with mp.workdps(120):
        inv = _inverse(A)
        n = 15
        L = [[ZERO] * n for _ in range(n)]
        for j in range(n):
            d = inv[j][j] - sum((L[j][k] * L[j][k] for k in range(j)), ZERO)
            if d <= 0:
                raise ValueError("inverse is not positive definite")
            L[j][j] = mp.sqrt(d)
            for i in range(j + 1, n):
                L[i][j] = (inv[i][j] - sum((L[i][k] * L[j][k] for k in range(j)), ZERO)) / L[j][j]
        return [[+L[j][i] for j in range(n)] for i in range(n)]


def pivot_sequence(cov):
    """Eigen PartialPivLU on the 15 x 15 matrix, in mp: for every column k the row (>= k) taken as pivot, the first row with the
    largest |a_ik|. Returns (rows[15], margins[15]); margins[k] = largest / second largest candidate (inf when there is none or it is 0,
    1 for an exact tie)."""
    A = [[M(x) for x in row] for row in np.asarray(cov, dtype=np.float64).reshape(15, 15)]
    n = 15
    rows, margins = [], []
    for k in range(n):
        cand = [abs(A[i][k]) for i in range(k, n)]
        best = max(cand)
        p = k + cand.index(best)                                  # index() = the first maximum
        rest = sorted(cand[:p - k] + cand[p - k + 1:], reverse=True)
        margins.append(float(best / rest[0]) if rest and rest[0] != 0 else float("inf"))
        rows.append(p)
        if best == 0:
            raise ZeroDivisionError("zero pivot")
        A[k], A[p] = A[p], A[k]
        for i in range(k + 1, n):
            f = A[i][k] / A[k][k]
            A[i] = [ZERO if j <= k else A[i][j] - f * A[k][j] for j in range(n)]
    return rows, margins


def info_defect(U, cov):
    """max |U^T U cov - I| in mp, for a float64 U (15 x 15) and the float64 covariance"""
    Um = [[M(x) for x in row] for row in np.asarray(U, dtype=np.float64).reshape(15, 15)]
    C = [[M(x) for x in row] for row in np.asarray(cov, dtype=np.float64).reshape(15, 15)]
    UtU = _matmul(_transpose(Um), Um, 15, 15, 15)
    Pm = _matmul(UtU, C, 15, 15, 15)
    return float(max(abs(Pm[i][j] - (ONE if i == j else ZERO)) for i in range(15) for j in range(15)))


# ---- IMUFactor::Evaluate --------------------------------------------------------------------------------------------------------
def _qleft(q):
    x, y, z, w = q
    return [[w, -x, -y, -z], [x, w, -z, y], [y, z, w, -x], [z, -y, x, w]]


def _qright(p):
    x, y, z, w = p
    return [[w, -x, -y, -z], [x, w, z, -y], [y, -z, w, x], [z, y, -x, w]]


def _bottom_right(A):
    return [[A[i][j] for j in (1, 2, 3)] for i in (1, 2, 3)]


def _delta_q(theta):
    return [theta[0] / TWO, theta[1] / TWO, theta[2] / TWO, ONE]


def imu_raw_exact(params, pre, G):
    """params = [pose_i (P, q xyzw), speed_bias_i (V, Ba, Bg), pose_j, speed_bias_j], pre = 467 float64 (vilf_imu_preint), G[3].
    Returns (r[15], J[15][30]): the residual and the Jacobian before sqrt_info, columns in local size as vilf_eval_imu_raw lays its four
    blocks out (pose_i 0-5, speed_bias_i 6-14, pose_j 15-20, speed_bias_j 21-29; the 7th, zero column of a pose block is not carried)."""
    p0, p1, p2, p3 = [vec(a) for a in params]
    Pi, Qi, Vi, Bai, Bgi = p0[:3], p0[3:7], p1[:3], p1[3:6], p1[6:9]
    Pj, Qj, Vj, Baj, Bgj = p2[:3], p2[3:7], p3[:3], p3[3:6], p3[6:9]
    pre = vec(pre)
    G = vec(G)
    sum_dt, delta_p, delta_q, delta_v, lin_ba, lin_bg = pre[0], pre[1:4], pre[4:8], pre[8:11], pre[11:14], pre[14:17]
    Jm = [pre[17 + 15 * i: 17 + 15 * i + 15] for i in range(15)]
    blk = lambda r0, c0: [[Jm[r0 + i][c0 + j] for j in range(3)] for i in range(3)]
    dp_dba, dp_dbg, dq_dbg, dv_dba, dv_dbg = blk(O_P, O_BA), blk(O_P, O_BG), blk(O_R, O_BG), blk(O_V, O_BA), blk(O_V, O_BG)
    add = lambda a, b: [a[k] + b[k] for k in range(3)]
    sub = lambda a, b: [a[k] - b[k] for k in range(3)]
    # IntegrationBase::evaluate :173-184
    dba, dbg = sub(Bai, lin_ba), sub(Bgi, lin_bg)
    cdq = qmul(delta_q, _delta_q(m3vec(dq_dbg, dbg)))
    cdv = add(add(delta_v, m3vec(dv_dba, dba)), m3vec(dv_dbg, dbg))
    cdp = add(add(delta_p, m3vec(dp_dba, dba)), m3vec(dp_dbg, dbg))
    Qi_inv = qinv(Qi)
    tp = [HALF * G[k] * sum_dt * sum_dt + Pj[k] - Pi[k] - Vi[k] * sum_dt for k in range(3)]
    tv = [G[k] * sum_dt + Vj[k] - Vi[k] for k in range(3)]
    rp = sub(qrot(Qi_inv, tp), cdp)
    rq = [TWO * c for c in qmul(qinv(cdq), qmul(Qi_inv, Qj))[:3]]
    rv = sub(qrot(Qi_inv, tv), cdv)
    r = rp + rq + rv + sub(Baj, Bai) + sub(Bgj, Bgi)
    # imu_factor.h:86-173 without the sqrt_info lines
    J = [[ZERO] * 30 for _ in range(15)]
    RiT = q_to_R(Qi_inv)
    neg = lambda A: m3scl(A, -ONE)
    I3 = eye3()
    _setb(J, O_P, 0 + O_P, neg(RiT))
    _setb(J, O_P, 0 + O_R, skew(qrot(Qi_inv, tp)))
    _setb(J, O_R, 0 + O_R, neg(_bottom_right(_mat4mul(_qleft(qmul(qinv(Qj), Qi)), _qright(cdq)))))
    _setb(J, O_V, 0 + O_R, skew(qrot(Qi_inv, tv)))
    _setb(J, O_P, 6 + 0, m3scl(neg(RiT), sum_dt))
    _setb(J, O_P, 6 + 3, neg(dp_dba))
    _setb(J, O_P, 6 + 6, neg(dp_dbg))
    _setb(J, O_R, 6 + 6, m3mul(neg(_bottom_right(_qleft(qmul(qmul(qinv(Qj), Qi), delta_q)))), dq_dbg))
    _setb(J, O_V, 6 + 0, neg(RiT))
    _setb(J, O_V, 6 + 3, neg(dv_dba))
    _setb(J, O_V, 6 + 6, neg(dv_dbg))
    _setb(J, O_BA, 6 + 3, neg(I3))
    _setb(J, O_BG, 6 + 6, neg(I3))
    _setb(J, O_P, 15 + O_P, RiT)
    _setb(J, O_R, 15 + O_R, _bottom_right(_qleft(qmul(qmul(qinv(cdq), Qi_inv), Qj))))
    _setb(J, O_V, 21 + 0, RiT)
    _setb(J, O_BA, 21 + 3, I3)
    _setb(J, O_BG, 21 + 6, I3)
    return r, J


def _mat4mul(a, b):
    return [[sum((a[i][k] * b[k][j] for k in range(4)), ZERO) for j in range(4)] for i in range(4)]


def imu_whitened_exact(U, r, J):
    """sqrt_info (15 rows of mpf) times the raw residual and the raw Jacobian"""
    rw = [sum((U[i][k] * r[k] for k in range(i, 15)), ZERO) for i in range(15)]
    Jw = [[sum((U[i][k] * J[k][j] for k in range(i, 15)), ZERO) for j in range(30)] for i in range(15)]
    return rw, Jw
