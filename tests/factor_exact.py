"""Exact references for the visual, LiDAR and prior factors and the two Plus operations, restated from the reference's text in mpmath at
50 digits (not from oracle/ and not from vilf_device.hpp):
  projection_exact      ProjectionFactor::Evaluate, the branch without UNIT_SPHERE_ERROR     (factor/projection_factor.cpp:21-121)
  projection_td_exact   ProjectionTdFactor, constructor and Evaluate                          (factor/projection_td_factor.cpp:6-20, 34-141)
  lidar_between_exact   lidarFactor::Evaluate with qil = Quaterniond(RIC RCL), til = RIC TCL + TIC (factor/lidar_factor.h:19-78)
  prior_exact           MarginalizationFactor::Evaluate; positify returns its argument        (factor/marginalization_factor.cpp:333-381)
  edge_exact, surf_exact EdgeCostFunction / SurfCostFunction                                   (feature_tracker/include/lidarFactor.hpp:21-102)
  pose_plus_exact       PoseLocalParameterization::Plus with Utility::deltaQ                  (factor/pose_local_parameterization.cpp:3-19)
  se3_plus_exact        LocalSE3Parameterization::Plus with getTransformFromSe3               (EstimationMapping.hpp:34-49, common.h:137-176)
Inputs are the float64 values handed to the code under test, converted exactly. Eigen's conventions are those of tests/imu_exact.py (q * v by
_transformVector, inverse() = conjugate / squaredNorm, toRotationMatrix without normalisation) plus Quaterniond(Matrix3d) with its four branches.
The Jacobians are the reference's analytic expressions, quirks included (the lidar factor's are unweighted, the prior's is J0 itself).

Every function returns (groups, terms): groups maps an output group to its list of mpf, terms maps the same name to a float, the largest term of the
sums that form the group. The arithmetic runs on pairs (value, e): e is the largest magnitude met on the way to the value, carried through the later
operations as a rounding error of that size would be (sum: max(ea, eb, |v|); product: max(|a| eb, |b| ea, |v|); quotient: max(ea / |b|, |a| eb / b^2, |v|);
sqrt: max(ea / (2 v), v); cos, sin: max(derivative times ea, |v|)); inputs and exact zeros carry nothing, a multiplication by a power of two only scales. e
is the largest term of the sums that form the entry, and stays large where an earlier sum cancelled (5 km positions, a 1e-9 residual left of terms of size
100, (1 - cos t) / t^2): an fp64 evaluation errs by a small multiple (the depth of the expression) of 2^-53 e. terms[g] is the largest e
of group g. Results travel as double-double pairs (imu_exact.to_dd)."""
import numpy as np
from mpmath import mp, mpf
import imu_exact as ix
from imu_exact import M, ZERO, ONE, TWO, HALF, to_dd, from_dd  # noqa: F401  (re-exported for the tests)

mp.dps = 50


# ---- (value, running error bound) ---------------------------------------------------------------------------------------------------------
def _pow2(c):
    return c == 0 or abs(c.man) == 1


class E:
    __slots__ = ("v", "e")

    def __init__(self, v, e=ZERO):
        self.v, self.e = v, e

    def exact_zero(self):
        return self.v == 0 and self.e == 0

    def __neg__(self):
        return E(-self.v, self.e)

    def __add__(self, o):
        if not isinstance(o, E):
            o = E(mpf(o))
        if o.exact_zero():
            return self
        if self.exact_zero():
            return o
        v = self.v + o.v
        return E(v, max(self.e, o.e, abs(v)))

    __radd__ = __add__

    def __sub__(self, o):
        return self + (-o if isinstance(o, E) else -mpf(o))

    def __rsub__(self, o):
        return (-self) + o

    def __mul__(self, o):
        if not isinstance(o, E):
            o = E(mpf(o))
        if self.exact_zero() or o.exact_zero():
            return E(ZERO)
        v = self.v * o.v
        if o.e == 0 and _pow2(o.v):
            return E(v, self.e * abs(o.v))
        if self.e == 0 and _pow2(self.v):
            return E(v, o.e * abs(self.v))
        return E(v, max(abs(self.v) * o.e, abs(o.v) * self.e, abs(v)))

    __rmul__ = __mul__

    def __truediv__(self, o):
        if not isinstance(o, E):
            o = E(mpf(o))
        if self.exact_zero():
            return E(ZERO)
        v = self.v / o.v
        if o.e == 0 and _pow2(o.v):
            return E(v, self.e / abs(o.v))
        return E(v, max(self.e / abs(o.v), abs(self.v) * o.e / (o.v * o.v), abs(v)))

    def __rtruediv__(self, o):
        return E(mpf(o)) / self


def esqrt(a):
    v = mp.sqrt(a.v)
    if a.e == 0 and v * v == a.v and _pow2(v):
        return E(v)
    return E(v, max(a.e / (TWO * v) if v != 0 else (ZERO if a.e == 0 else mpf("inf")), v))


def ecos(a):
    v = mp.cos(a.v)
    return E(v) if a.exact_zero() else E(v, max(abs(mp.sin(a.v)) * a.e, abs(v)))


def esin(a):
    v = mp.sin(a.v)
    return E(v) if a.exact_zero() else E(v, max(abs(mp.cos(a.v)) * a.e, abs(v)))


def ev(a):
    """float64 array -> list of exact E"""
    return [E(M(x)) for x in np.asarray(a, dtype=np.float64).ravel()]


def _out(groups):
    """{name: list of E} -> ({name: [mpf]}, {name: float})"""
    return ({g: [x.v for x in xs] for g, xs in groups.items()},
            {g: float(max([x.e for x in xs] + [ZERO])) for g, xs in groups.items()})


def _flat(A):
    return [x for r in A for x in r]


def _neg3(A):
    return [[-x for x in r] for r in A]


def _T(A):
    return [list(r) for r in zip(*A)]


def _m23(A, B):
    """(2 x 3)(3 x k)"""
    return [[A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j] for j in range(len(B[0]))] for i in range(2)]


def quat_from_matrix(m):
    """Eigen Quaterniond(Matrix3d) (Quaternion.h, quaternionbase_assign_impl): (q xyzw, branch); branch 3 = trace > 0, else the index of the largest
    diagonal entry as Eigen picks it (i = 0; if m11 > m00: i = 1; if m22 > m_ii: i = 2)."""
    t = m[0][0] + m[1][1] + m[2][2]
    q = [None] * 4
    if t.v > 0:
        t = esqrt(t + ONE)
        q[3] = HALF * t
        t = HALF / t
        q[0] = (m[2][1] - m[1][2]) * t
        q[1] = (m[0][2] - m[2][0]) * t
        q[2] = (m[1][0] - m[0][1]) * t
        return q, 3
    i = 0
    if m[1][1].v > m[0][0].v:
        i = 1
    if m[2][2].v > m[i][i].v:
        i = 2
    j = (i + 1) % 3
    k = (j + 1) % 3
    t = esqrt(m[i][i] - m[j][j] - m[k][k] + ONE)
    q[i] = HALF * t
    t = HALF / t
    q[3] = (m[k][j] - m[j][k]) * t
    q[j] = (m[j][i] + m[i][j]) * t
    q[k] = (m[k][i] + m[i][k]) * t
    return q, i


def _pose(p):
    p = ev(p)
    return p[:3], p[3:7]


# ---- ProjectionFactor / ProjectionTdFactor ------------------------------------------------------------------------------------------------
def _projection(params, pts_i_td, pts_j_td, sqrt_info, velocity_i=None, velocity_j=None):
    Pi, Qi = _pose(params[0])
    Pj, Qj = _pose(params[1])
    tic, qic = _pose(params[2])
    inv_dep_i = ev(params[3])[0]
    add = lambda a, b: [a[k] + b[k] for k in range(3)]
    sub = lambda a, b: [a[k] - b[k] for k in range(3)]
    pts_camera_i = [c / inv_dep_i for c in pts_i_td]
    pts_imu_i = add(ix.qrot(qic, pts_camera_i), tic)
    pts_w = add(ix.qrot(Qi, pts_imu_i), Pi)
    pts_imu_j = ix.qrot(ix.qinv(Qj), sub(pts_w, Pj))
    pts_camera_j = ix.qrot(ix.qinv(qic), sub(pts_imu_j, tic))
    dep_j = pts_camera_j[2]
    residual = [sqrt_info * (pts_camera_j[k] / dep_j - pts_j_td[k]) for k in range(2)]
    Ri, Rj, ric = ix.q_to_R(Qi), ix.q_to_R(Qj), ix.q_to_R(qic)
    z = E(ZERO)
    reduce = [[sqrt_info * (ONE / dep_j), z, sqrt_info * (-pts_camera_j[0] / (dep_j * dep_j))],
              [z, sqrt_info * (ONE / dep_j), sqrt_info * (-pts_camera_j[1] / (dep_j * dep_j))]]
    ricT, RjT = _T(ric), _T(Rj)
    ricT_RjT = ix.m3mul(ricT, RjT)
    # pose i :78-82
    right = ix.m3mul(ix.m3mul(ricT_RjT, Ri), _neg3(ix.skew(pts_imu_i)))
    J_i = _m23(reduce, [ricT_RjT[r] + right[r] for r in range(3)])
    # pose j :90-94
    left = ix.m3mul(ricT, _neg3(RjT))
    right = ix.m3mul(ricT, ix.skew(pts_imu_j))
    J_j = _m23(reduce, [left[r] + right[r] for r in range(3)])
    # extrinsic :100-105
    RjT_Ri = ix.m3mul(RjT, Ri)
    left = ix.m3mul(ricT, [[RjT_Ri[r][c] - (ONE if r == c else ZERO) for c in range(3)] for r in range(3)])
    tmp_r = ix.m3mul(ix.m3mul(ricT_RjT, Ri), ric)
    inner = sub(ix.m3vec(RjT, sub(add(ix.m3vec(Ri, tic), Pi), Pj)), tic)
    right = ix.m3add(ix.m3add(ix.m3mul(_neg3(tmp_r), ix.skew(pts_camera_i)), ix.skew(ix.m3vec(tmp_r, pts_camera_i))), ix.skew(ix.m3vec(ricT, inner)))
    J_ex = _m23(reduce, [left[r] + right[r] for r in range(3)])
    # inverse depth :112 / :129 (left to right: (((((reduce ricT) RjT) Ri) ric) pts) * -1.0 / (inv_dep^2))
    chain = _m23(_m23(_m23(_m23(reduce, ricT), RjT), Ri), ric)
    J_f = [(chain[r][0] * pts_i_td[0] + chain[r][1] * pts_i_td[1] + chain[r][2] * pts_i_td[2]) * -ONE / (inv_dep_i * inv_dep_i) for r in range(2)]
    groups = {"residual": residual, "J_pose_i": _flat(J_i), "J_pose_j": _flat(J_j), "J_ex_pose": _flat(J_ex), "J_feature": J_f}
    if velocity_i is not None:                                                                    # :134-135
        J_td = [(chain[r][0] * velocity_i[0] + chain[r][1] * velocity_i[1] + chain[r][2] * velocity_i[2]) / inv_dep_i * -ONE + sqrt_info * velocity_j[r]
                for r in range(2)]
        groups["J_td"] = J_td
    groups["pts_camera_j"] = pts_camera_j
    return groups


def _sqrt_info(focal_length):
    """FOCAL_LENGTH / 1.5 is formed in fp64 when the estimator sets ProjectionFactor::sqrt_info (estimator.cpp): the rounded quotient is the input"""
    return E(M(float(focal_length) / 1.5))


def projection_exact(focal_length, params, pts_i, pts_j):
    """params = [Pose_i, Pose_j, Ex_Pose, [inv_dep]]. Groups: residual[2], J_pose_i / J_pose_j / J_ex_pose [2 x 6 row-major, local size], J_feature[2],
    and pts_camera_j[3] (not an output of the factor: what the cases assert their z on)."""
    return _out(_projection(params, ev(pts_i), ev(pts_j), _sqrt_info(focal_length)))


def projection_td_exact(focal_length, TR, ROW, params, pts_i, pts_j, vel_i, vel_j, td_i, td_j, row_i, row_j):
    """params = [Pose_i, Pose_j, Ex_Pose, [inv_dep], [td]]; row_* as the constructor takes them (uv.y); adds the group J_td[2]"""
    pts_i, pts_j = ev(pts_i), ev(pts_j)
    velocity_i = ev(vel_i) + [E(ZERO)]
    velocity_j = ev(vel_j) + [E(ZERO)]
    ROW_, TR_ = E(M(ROW)), E(M(TR))
    row_ic = E(M(row_i)) - ROW_ / TWO                                                            # :18-19
    row_jc = E(M(row_j)) - ROW_ / TWO
    td = ev(params[4])[0]
    si = td - E(M(td_i)) + TR_ / ROW_ * row_ic                                                  # :51-52
    sj = td - E(M(td_j)) + TR_ / ROW_ * row_jc
    pts_i_td = [pts_i[k] - si * velocity_i[k] for k in range(3)]
    pts_j_td = [pts_j[k] - sj * velocity_j[k] for k in range(3)]
    return _out(_projection(params, pts_i_td, pts_j_td, _sqrt_info(focal_length), velocity_i, velocity_j))


# ---- lidarFactor --------------------------------------------------------------------------------------------------------------------------
def lidar_extrinsic_exact(RIC, TIC, RCL, TCL):
    """(qil xyzw, til, branch) as lidar_factor.h:28-29 forms them; E lists"""
    ric = [ev(r) for r in np.asarray(RIC, dtype=np.float64).reshape(3, 3)]
    rcl = [ev(r) for r in np.asarray(RCL, dtype=np.float64).reshape(3, 3)]
    qil, branch = quat_from_matrix(ix.m3mul(ric, rcl))
    til = [a + b for a, b in zip(ix.m3vec(ric, ev(TCL)), ev(TIC))]
    return qil, til, branch


def lidar_between_exact(RIC, TIC, RCL, TCL, params, lidar_q, lidar_t):
    """params = [Pose_i, Pose_j]; lidar_q xyzw. Groups: residual[6] (weighted 10 / 100), J_pose_i, J_pose_j [6 x 6 row-major, local size, unweighted]."""
    Pi, Qi = _pose(params[0])
    Pj, Qj = _pose(params[1])
    qil, til, _ = lidar_extrinsic_exact(RIC, TIC, RCL, TCL)
    lq, lt = ev(lidar_q), ev(lidar_t)
    sub = lambda a, b: [a[k] - b[k] for k in range(3)]
    qli = ix.qinv(qil)
    tli = [-c for c in ix.qrot(ix.qinv(qil), til)]
    Qi_inv = ix.qinv(Qi)
    dP = ix.qrot(Qi_inv, sub(Pj, Pi))
    rp = sub(ix.qrot(qli, sub(sub(dP, til), ix.qrot(ix.qmul(qil, lq), tli))), lt)                # :36
    cdq = ix.qmul(ix.qmul(qil, lq), qli)
    rq = [TWO * c for c in ix.qmul(ix.qinv(cdq), ix.qmul(Qi_inv, Qj))[:3]]                       # :37
    w_p, w_q = E(M(1.0 / 0.1)), E(M(1.0 / 0.01))                                                 # :40-41: formed in fp64, exactly 10 and 100
    residual = [w_p * c for c in rp] + [w_q * c for c in rq]
    Ji = [[E(ZERO)] * 6 for _ in range(6)]
    Jj = [[E(ZERO)] * 6 for _ in range(6)]
    Rm = ix.q_to_R(ix.qmul(qli, Qi_inv))
    ix._setb(Ji, 0, 0, _neg3(Rm))                                                                # :52
    ix._setb(Ji, 0, 3, ix.m3mul(ix.q_to_R(qli), ix.skew(dP)))                                    # :53
    ix._setb(Ji, 3, 3, _neg3(ix._bottom_right(ix._mat4mul(ix._qleft(ix.qmul(ix.qinv(Qj), Qi)), ix._qright(cdq)))))   # :57
    ix._setb(Jj, 0, 0, Rm)                                                                       # :69
    ix._setb(Jj, 3, 3, ix._bottom_right(ix._qleft(ix.qmul(ix.qmul(ix.qinv(cdq), Qi_inv), Qj))))  # :73
    return _out({"residual": residual, "J_pose_i": _flat(Ji), "J_pose_j": _flat(Jj)})


# ---- MarginalizationFactor ----------------------------------------------------------------------------------------------------------------
def prior_dx_exact(blocks, params, n):
    """dx[n] (E) of marginalization_factor.cpp:346-363 and, per size-7 block, w of x0^-1 x (mpf)"""
    dx = [E(ZERO)] * n
    ws = {}
    for i, (b, x) in enumerate(zip(blocks, params)):
        size, idx = int(b["size"]), int(b["idx"])
        x, x0 = ev(x)[:size], ev(b["x0"])[:size]
        if size != 7:
            for k in range(size):
                dx[idx + k] = x[k] - x0[k]
        else:
            for k in range(3):
                dx[idx + k] = x[k] - x0[k]
            dq = ix.qmul(ix.qinv(x0[3:7]), x[3:7])
            ws[i] = dq[3].v
            s = TWO if dq[3].v >= 0 else -TWO
            for k in range(3):
                dx[idx + 3 + k] = s * dq[k]
    return dx, ws


def prior_exact(J0, r0, blocks, params):
    """J0 [n, n], r0 [n] float64; blocks = dicts(size, idx, x0) as abi.prior_to_numpy gives them. Groups: residual[n] and dx[n]; the Jacobian blocks are J0's
    columns, which the tests compare to the bit. Returns (groups, terms, ws): ws[i] = w of x0^-1 x for pose block i."""
    J0 = np.asarray(J0, dtype=np.float64)
    n = J0.shape[0]
    dx, ws = prior_dx_exact(blocks, params, n)
    r0 = ev(r0)
    residual = []
    for r in range(n):
        acc = r0[r]
        for c in range(n):
            if J0[r, c] != 0.0:
                acc = acc + E(M(J0[r, c])) * dx[c]
        residual.append(acc)
    groups, terms = _out({"residual": residual, "dx": dx})
    return groups, terms, ws


# ---- F-LOAM edge / surf -------------------------------------------------------------------------------------------------------------------
def _world_point(pose_qt, cp):
    p = ev(pose_qt)
    q, t = p[:4], p[4:7]
    return [a + b for a, b in zip(ix.qrot(q, ev(cp)), t)]


def edge_exact(pose_qt, cp, a, b):
    """pose = [qx qy qz qw tx ty tz]. Groups: residual[3], J[3 x 6 row-major: rotation | translation]"""
    lp = _world_point(pose_qt, cp)
    a, b = ev(a), ev(b)
    sub = lambda x, y: [x[k] - y[k] for k in range(3)]
    nu = ix.cross(sub(lp, a), sub(lp, b))
    ab = sub(a, b)
    ab_norm = esqrt(ab[0] * ab[0] + ab[1] * ab[1] + ab[2] * ab[2])
    residual = [c / ab_norm for c in nu]
    J_se3 = [_neg3(ix.skew(lp))[r] + [E(ONE if r == c else ZERO) for c in range(3)] for r in range(3)]      # :40-42
    nsab = _neg3(ix.skew(ab))
    J = [[(nsab[r][0] * J_se3[0][c] + nsab[r][1] * J_se3[1][c] + nsab[r][2] * J_se3[2][c]) / ab_norm for c in range(6)] for r in range(3)]   # :47
    return _out({"residual": residual, "J": _flat(J)})


def surf_exact(pose_qt, cp, n, d):
    """Groups: residual[1], J[1 x 6]"""
    pw = _world_point(pose_qt, cp)
    n = ev(n)
    residual = [n[0] * pw[0] + n[1] * pw[1] + n[2] * pw[2] + E(M(d))]
    J_se3 = [_neg3(ix.skew(pw))[r] + [E(ONE if r == c else ZERO) for c in range(3)] for r in range(3)]
    J = [n[0] * J_se3[0][c] + n[1] * J_se3[1][c] + n[2] * J_se3[2][c] for c in range(6)]
    return _out({"residual": residual, "J": J})


# ---- Plus ---------------------------------------------------------------------------------------------------------------------------------
def pose_plus_exact(x, delta):
    """x = [P, q xyzw], delta[6]. Groups: p[3], q[4]"""
    P, q = _pose(x)
    d = ev(delta)
    dq = [d[3] / TWO, d[4] / TWO, d[5] / TWO, E(ONE)]
    prod = ix.qmul(q, dq)
    nrm = esqrt(prod[0] * prod[0] + prod[1] * prod[1] + prod[2] * prod[2] + prod[3] * prod[3])
    return _out({"p": [P[k] + d[k] for k in range(3)], "q": [c / nrm for c in prod]})


def se3_theta(delta):
    """omega.norm() in fp64, as getTransformFromSe3 forms it: what `theta < 1e-10` compares"""
    w = np.asarray(delta, dtype=np.float64)[:3]
    return float(np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]))


def se3_plus_exact(x_qt, delta):
    """x = [q xyzw, t], delta = [omega, upsilon]. Groups: q[4], t[3]. The reference's own formulas with its literal coefficients; the branch is the one the
    float64 theta takes."""
    p = ev(x_qt)
    quater, trans = p[:4], p[4:7]
    d = ev(delta)
    omega, upsilon = d[:3], d[3:6]
    small = se3_theta(delta) < 1e-10
    theta = esqrt(omega[0] * omega[0] + omega[1] * omega[1] + omega[2] * omega[2])
    half_theta = HALF * theta
    real = ecos(half_theta)
    if small:
        theta_sq = theta * theta
        theta_po4 = theta_sq * theta_sq
        imag = E(HALF) - E(M(0.0208333)) * theta_sq + E(M(0.000260417)) * theta_po4
    else:
        imag = esin(half_theta) / theta
    dq = [imag * omega[0], imag * omega[1], imag * omega[2], real]
    if small:
        J = ix.q_to_R(dq)
    else:
        Om = ix.skew(omega)
        Om2 = ix.m3mul(Om, Om)
        a = (ONE - ecos(theta)) / (theta * theta)
        b = (theta - esin(theta)) / (theta * theta * theta)
        J = [[(ONE if r == c else ZERO) + a * Om[r][c] + b * Om2[r][c] for c in range(3)] for r in range(3)]
    delta_t = ix.m3vec(J, upsilon)
    rt = ix.qrot(dq, trans)
    return _out({"q": ix.qmul(dq, quater), "t": [rt[k] + delta_t[k] for k in range(3)]})
