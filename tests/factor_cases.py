"""Named cases for tests/test_factor_exact.py: inputs of the visual, LiDAR and prior factors and of the two Plus operations at the edges the hook tests of
tests/test_gpu_parity.py never reach. Every number comes from PCG64's uniform doubles and + - x / sqrt (trigonometric values are literals), so the
float64 inputs are the same bits everywhere. Quaternions are (x, y, z, w); a pose is [P, q], an F-LOAM pose [q, t]."""
import copy
import numpy as np

# cos(angle / 2) of the rotations the cases use
COS_HALF = {0.05: 0.9996875162757026, 0.1: 0.9987502603949663, 0.6: 0.955336489125606, 1.0: 0.8775825618903728, 3.0: 0.0707372016677029,
            170.0: 0.08715574274765814}   # the last one in degrees


def rng_of(seed):
    return np.random.Generator(np.random.PCG64(seed))


def uni(rng, lo, hi, n=None):
    return lo + (hi - lo) * rng.random(n)


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.sqrt(np.sum(v * v))


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def qconj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]])


def q_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def eigen_q(m):
    """Eigen's Quaterniond(Matrix3d) in fp64, not normalised (only used to build and select inputs)"""
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0:
        s = np.sqrt(t + 1.0)
        return np.array([(m[2, 1] - m[1, 2]) * 0.5 / s, (m[0, 2] - m[2, 0]) * 0.5 / s, (m[1, 0] - m[0, 1]) * 0.5 / s, 0.5 * s])
    i = 0
    if m[1, 1] > m[0, 0]:
        i = 1
    if m[2, 2] > m[i, i]:
        i = 2
    j = (i + 1) % 3; k = (j + 1) % 3
    s = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
    q = np.zeros(4)
    q[i] = 0.5 * s; q[3] = (m[k, j] - m[j, k]) * 0.5 / s; q[j] = (m[j, i] + m[i, j]) * 0.5 / s; q[k] = (m[k, i] + m[i, k]) * 0.5 / s
    return q


def R_to_q(m):
    return unit(eigen_q(m))


def q_rot(axis, cos_half):
    """rotation about `axis` whose half angle has the cosine cos_half"""
    return unit(np.concatenate([unit(axis) * np.sqrt(1.0 - cos_half * cos_half), [cos_half]]))


def q_rand(rng):
    return unit(uni(rng, -1.0, 1.0, 4))


def q_small(rng, cos_half):
    return q_rot(uni(rng, -1.0, 1.0, 3), cos_half)


def rot(q, v):
    return q_to_R(q) @ np.asarray(v, dtype=np.float64)


# ---- option sets --------------------------------------------------------------------------------------------------------------------------
OPTION_NAMES = ("default", "alt", "alt7", "br0", "br1", "br2")


def option_sets(default):
    """name -> Options. default: as given. alt: another camera (focal length, TR, ROW) and general extrinsics. alt7: alt's matrices rounded to 7 decimals
    (a yaml calibration), which leaves qil off unit norm. br0 / br1 / br2: RIC RCL a 170 degree rotation about an axis whose largest component is x / y / z,
    so that Quaterniond(Matrix3d) leaves its trace-positive branch."""
    rng = rng_of(9000)
    out = {"default": copy.copy(default)}
    ric0 = np.array(default.RIC[:]).reshape(3, 3)
    alt = copy.copy(default)
    alt.focal_length, alt.TR, alt.ROW = 718.856, 0.033, 375.0
    ric = ric0 @ q_to_R(q_rot([1.0, 2.0, 3.0], COS_HALF[1.0]))
    while True:                  # an RCL for which the 7-decimal rounding (alt7) shows in the norm of qil: the deviation is first order in the rounding, but can cancel
        rcl = q_to_R(q_rand(rng))
        q7 = eigen_q(np.round(ric, 7) @ np.round(rcl, 7))
        if abs(np.sqrt(np.sum(q7 * q7)) - 1.0) > 3e-8:
            break
    alt.RIC[:] = list(ric.ravel()); alt.RCL[:] = list(rcl.ravel())
    alt.TIC[:] = [0.3, -0.2, 0.1]; alt.TCL[:] = list(uni(rng, -0.5, 0.5, 3))
    out["alt"] = alt
    alt7 = copy.copy(alt)
    for name in ("RIC", "RCL", "TIC", "TCL"):
        getattr(alt7, name)[:] = list(np.round(np.array(getattr(alt, name)[:]), 7))
    out["alt7"] = alt7
    for i in range(3):
        axis = np.array([0.3, -0.4, 0.25]); axis[i] = 1.0
        target = q_to_R(q_rot(axis, COS_HALF[170.0]))
        o = copy.copy(default)
        o.RCL[:] = list((ric0.T @ target).ravel())
        o.TCL[:] = list(uni(rng, -0.5, 0.5, 3))
        out["br%d" % i] = o
    return out


def ex_pose(o):
    return np.concatenate([np.array(o.TIC[:]), R_to_q(np.array(o.RIC[:]).reshape(3, 3))])


# ---- projection ---------------------------------------------------------------------------------------------------------------------------
def _project(params, pts_i):
    """pts_camera_j in fp64 (only to place pts_j near the projection)"""
    Pi, Pj, ex, lam = params
    p = rot(ex[3:], np.asarray(pts_i) / lam[0]) + ex[:3]
    p = rot(Pi[3:], p) + Pi[:3]
    p = rot(qconj(Pj[3:]), p - Pj[:3])
    return rot(qconj(ex[3:]), p - ex[:3])


def _proj_case(rng, o, opt, origin=(0.0, 0.0, 0.0), baseline=0.5, rel=None, inv_dep=None, pts_i=None, same_pose=False):
    ex = ex_pose(o)
    Pi = np.concatenate([np.asarray(origin) + uni(rng, -2.0, 2.0, 3), q_rand(rng)])
    if same_pose:
        Pj = Pi.copy()
    else:
        qrel = q_small(rng, COS_HALF[0.1]) if rel is None else rel
        Pj = np.concatenate([Pi[:3] + unit(uni(rng, -1.0, 1.0, 3)) * baseline, unit(qmul(Pi[3:], qrel))])
    lam = np.array([1.0 / uni(rng, 4.0, 30.0) if inv_dep is None else inv_dep])
    pi = np.array([uni(rng, -0.5, 0.5), uni(rng, -0.2, 0.2), 1.0]) if pts_i is None else np.asarray(pts_i, dtype=np.float64)
    params = [Pi, Pj, ex, lam]
    pc = _project(params, pi)
    pj = np.array([pc[0] / pc[2] + uni(rng, -0.003, 0.003), pc[1] / pc[2] + uni(rng, -0.003, 0.003), 1.0])
    return dict(opt=opt, params=params, pts_i=pi, pts_j=pj)


def _negated(case, which):
    c = dict(case); c["params"] = [p.copy() for p in case["params"]]
    for k in which:
        c["params"][k][3:] = -c["params"][k][3:]
    return c


def projection_cases(sets):
    """name -> dict(opt, params, pts_i, pts_j[, same_as]). same_as names the case whose device result this one must equal to the bit."""
    rng = rng_of(9100)
    d, a = sets["default"], sets["alt"]
    c = {}
    for k in range(8):
        c["plain%d" % k] = _proj_case(rng, d, "default")
    c["alt_extrinsic"] = _proj_case(rng, a, "alt")
    c["far_5km"] = _proj_case(rng, d, "default", origin=(4000.0, -5000.0, 3000.0), baseline=0.5)
    c["inv_dep_2"] = _proj_case(rng, d, "default", inv_dep=2.0)
    c["inv_dep_1e-3"] = _proj_case(rng, d, "default", inv_dep=1e-3)
    c["inv_dep_1e-6"] = _proj_case(rng, d, "default", inv_dep=1e-6)
    c["inv_dep_negative"] = _proj_case(rng, d, "default", inv_dep=-0.2)
    c["same_pose"] = _proj_case(rng, d, "default", same_pose=True)
    # 0.6 rad about the camera's y axis, expressed in the body frame; the point sits 45 degrees off the optical axis on the side the rotation turns away from
    ex = ex_pose(d)
    best = None
    for sgn in (1.0, -1.0):
        qcam = q_rot([0.0, sgn, 0.0], COS_HALF[0.6])
        rel = qmul(qmul(ex[3:], qcam), qconj(ex[3:]))
        cand = _proj_case(rng_of(9101), d, "default", rel=rel, inv_dep=0.1, pts_i=[1.0, 0.05, 1.0], baseline=0.2)
        z = _project(cand["params"], cand["pts_i"])[2]
        if best is None or (0 < z < best[0]):
            best = (z, cand)
    c["low_z"] = best[1]
    base = c["plain0"]
    for name, which in (("neg_Qi", (0,)), ("neg_Qj", (1,)), ("neg_qic", (2,)), ("neg_all", (0, 1, 2))):
        c[name] = _negated(base, which); c[name]["same_as"] = "plain0"
    return c


def projection_td_cases(sets):
    """name -> dict(opt, params (with [td]), pts_i, pts_j, vel_i, vel_j, td_i, td_j, row_i, row_j[, same_as])"""
    rng = rng_of(9200)
    c = {}
    for opt in ("default", "alt"):
        o = sets[opt]
        ROW = float(o.ROW)

        def make(vel_i=(2.0, -1.5), vel_j=(-2.0, 1.5), td=0.03, td_i=0.01, td_j=-0.02, row_i=None, row_j=None):
            b = _proj_case(rng, o, opt)
            b["params"] = b["params"] + [np.array([td])]
            b.update(vel_i=np.array(vel_i, dtype=np.float64), vel_j=np.array(vel_j, dtype=np.float64), td_i=td_i, td_j=td_j,
                     row_i=float(np.floor(uni(rng, 0.0, ROW))) if row_i is None else row_i, row_j=float(np.floor(uni(rng, 0.0, ROW))) if row_j is None else row_j)
            return b
        c["plain_" + opt] = make()
        c["velocity_signs_" + opt] = make(vel_i=(-2.0, -1.5), vel_j=(2.0, 1.5))
        c["row_0_" + opt] = make(row_i=0.0, row_j=0.0)
        c["row_last_" + opt] = make(row_i=ROW - 1.0, row_j=ROW - 1.0)
        c["row_half_" + opt] = make(row_i=ROW / 2, row_j=ROW / 2)
        c["velocity_zero_at_i_" + opt] = make(vel_i=(0.0, 0.0))
        c["velocity_zero_at_j_" + opt] = make(vel_j=(0.0, 0.0))
    # td = td_i = td_j and TR = 0: the shift is exactly zero, so the result is that of the same call with zero velocities (J_td apart: it keeps the velocities)
    z = c["plain_default"]
    deg = dict(z); deg.update(td_i=0.03, td_j=0.03)
    c["degenerate_default"] = deg
    zero = dict(deg); zero.update(vel_i=np.zeros(2), vel_j=np.zeros(2))
    c["degenerate_zero_velocity_default"] = zero
    c["degenerate_default"]["same_as"] = "degenerate_zero_velocity_default"
    return c


# ---- lidar between ------------------------------------------------------------------------------------------------------------------------
def _lidar_case(rng, opt, origin=(0.0, 0.0, 0.0), qc=None, tc=None, qrel=None, same=False):
    Pi = np.concatenate([np.asarray(origin) + uni(rng, -2.0, 2.0, 3), q_rand(rng)])
    if same:
        Pj = Pi.copy()
    else:
        Pj = np.concatenate([Pi[:3] + uni(rng, -1.0, 1.0, 3), unit(qmul(Pi[3:], q_small(rng, COS_HALF[0.1]) if qrel is None else qrel))])
    return dict(opt=opt, params=[Pi, Pj], q=q_small(rng, COS_HALF[0.05]) if qc is None else np.asarray(qc, dtype=np.float64),
                t=uni(rng, -1.0, 1.0, 3) if tc is None else np.asarray(tc, dtype=np.float64))


def lidar_cases(sets):
    rng = rng_of(9300)
    c = {}
    for k in range(6):
        c["plain%d" % k] = _lidar_case(rng, "default")
    c["same_pose_identity"] = _lidar_case(rng, "default", qc=[0.0, 0.0, 0.0, 1.0], tc=[0.0, 0.0, 0.0], same=True)
    c["far_5km"] = _lidar_case(rng, "default", origin=(4000.0, -5000.0, 3000.0))
    c["lidar_q_negative_w"] = _lidar_case(rng, "default", qc=-q_small(rng, COS_HALF[0.05]))
    c["residual_3rad"] = _lidar_case(rng, "default", qrel=q_small(rng, COS_HALF[3.0]), qc=[0.0, 0.0, 0.0, 1.0])
    c["translation_30m"] = _lidar_case(rng, "default", tc=unit(uni(rng, -1.0, 1.0, 3)) * 30.0)
    for opt in ("alt", "alt7", "br0", "br1", "br2"):
        for k in range(2):
            c["%s_%d" % (opt, k)] = _lidar_case(rng, opt)
    return c


# ---- edge / surf --------------------------------------------------------------------------------------------------------------------------
def _s2m_pose(rng, q=None, t_scale=2.0):
    return np.concatenate([q_rand(rng) if q is None else q, uni(rng, -t_scale, t_scale, 3)])


def edge_cases():
    rng = rng_of(9400)
    c = {}

    def make(pose=None, cp=None, a=None, d_ab=0.2):
        pose = _s2m_pose(rng) if pose is None else pose
        cp = uni(rng, -5.0, 5.0, 3) if cp is None else cp
        a = uni(rng, -5.0, 5.0, 3) if a is None else a
        return dict(pose=pose, cp=cp, a=a, b=a + unit(uni(rng, -1.0, 1.0, 3)) * d_ab)
    for k in range(4):
        c["plain%d" % k] = make()
    c["ab_1e-3"] = make(d_ab=1e-3)
    c["ab_50"] = make(d_ab=50.0)
    c["cp_80m_1rad"] = make(pose=_s2m_pose(rng, q=q_small(rng, COS_HALF[1.0])), cp=unit(uni(rng, -1.0, 1.0, 3)) * 80.0)
    e = make()
    lp = e["a"] + 0.37 * (e["b"] - e["a"])
    e["cp"] = rot(qconj(e["pose"][:4]), lp - e["pose"][4:])
    c["point_on_line"] = e
    c["ab_5km"] = make(a=np.array([4000.0, -5000.0, 3000.0]) + uni(rng, -1.0, 1.0, 3), d_ab=0.5)
    return c


def surf_cases():
    rng = rng_of(9500)
    c = {}

    def make(pose=None, cp=None):
        return dict(pose=_s2m_pose(rng) if pose is None else pose, cp=uni(rng, -5.0, 5.0, 3) if cp is None else cp, n=unit(uni(rng, -1.0, 1.0, 3)),
                    d=float(uni(rng, -1.0, 1.0)))
    for k in range(4):
        c["plain%d" % k] = make()
    c["cp_80m_1rad"] = make(pose=_s2m_pose(rng, q=q_small(rng, COS_HALF[1.0])), cp=unit(uni(rng, -1.0, 1.0, 3)) * 80.0)
    s = make()
    pw = rot(s["pose"][:4], s["cp"]) + s["pose"][4:]
    s["cp"] = s["cp"] + rot(qconj(s["pose"][:4]), s["n"] * (100.0 - float(s["n"] @ pw)))     # moves the world point to n . p = 100
    pw = rot(s["pose"][:4], s["cp"]) + s["pose"][4:]
    s["d"] = -float(s["n"] @ pw) + 1e-9
    c["cancels_to_1e-9"] = s
    return c


# ---- Plus ---------------------------------------------------------------------------------------------------------------------------------
def pose_plus_cases():
    rng = rng_of(9600)
    c = {}
    for name, mag in (("dtheta_0", 0.0), ("dtheta_1e-12", 1e-12), ("dtheta_1e-3", 1e-3), ("dtheta_0.5", 0.5), ("dtheta_3", 3.0)):
        c[name] = dict(x=np.concatenate([uni(rng, -2.0, 2.0, 3), q_rand(rng)]), delta=np.concatenate([uni(rng, -0.1, 0.1, 3), unit(uni(rng, -1.0, 1.0, 3)) * mag]))
    q = q_rand(rng)
    c["negative_w"] = dict(x=np.concatenate([uni(rng, -2.0, 2.0, 3), -q if q[3] > 0 else q]), delta=uni(rng, -0.1, 0.1, 6))
    c["far_5km"] = dict(x=np.concatenate([[4000.0, -5000.0, 3000.0] + uni(rng, -1.0, 1.0, 3), q_rand(rng)]), delta=uni(rng, -0.1, 0.1, 6))
    return c


SE3_THETAS = (0.0, 1e-12, 9e-11, 1.1e-10, 1e-9, 1e-8, 1e-6, 1e-4, 1e-2, 1.0, 3.1, 6.0)


def se3_plus_cases():
    """(theta, |upsilon|) -> dict(x [q, t of 100 m], delta [omega, upsilon])"""
    rng = rng_of(9700)
    c = {}
    for th in SE3_THETAS:
        for ups in (1e-3, 10.0):
            x = np.concatenate([q_rand(rng), unit(uni(rng, -1.0, 1.0, 3)) * 100.0])
            c["theta_%g_upsilon_%g" % (th, ups)] = dict(x=x, theta=th, upsilon=ups,
                                                         delta=np.concatenate([unit(uni(rng, -1.0, 1.0, 3)) * th, unit(uni(rng, -1.0, 1.0, 3)) * ups]))
    return c


# ---- prior --------------------------------------------------------------------------------------------------------------------------------
HALF_QUATS = [np.array(v, dtype=np.float64) for v in
              ([0.5, 0.5, 0.5, 0.5], [0.5, -0.5, 0.5, 0.5], [-0.5, 0.5, 0.5, -0.5], [0.0, 0.0, 0.0, 1.0], [0.0, 1.0, 0.0, 0.0], [0.5, 0.5, -0.5, -0.5],
               [0.0, 0.0, -1.0, 0.0], [-0.5, -0.5, -0.5, 0.5], [1.0, 0.0, 0.0, 0.0], [0.5, -0.5, -0.5, 0.5], [0.0, 0.0, 0.0, -1.0], [-0.5, 0.5, -0.5, 0.5])]
DECADES = (1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1.0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6)
LAYOUT_11 = [7] * 11 + [7, 9]             # the fixed path's prior: 11 poses, Ex, one speed-bias (n = 81)
LAYOUT_157 = [7] * 10 + [9] * 10 + [7, 1]  # poses, speed-biases, Ex, td: 22 blocks, n = 60 + 90 + 6 + 1


def _prior_case(rng, layout, perturb, exact_quats=False, decades=False, dq=None, negate=()):
    """J0 [n, n], r0 [n], blocks (id, size, idx, x0), params. perturb: size of the step of every block; dq: relative rotation of the pose blocks (instead of
    a small one); negate: block numbers whose parameter quaternion changes sign"""
    blocks, params, idx = [], [], 0
    for i, size in enumerate(layout):
        if size == 7:
            q0 = HALF_QUATS[i % len(HALF_QUATS)] if exact_quats else q_rand(rng)
            x0 = np.concatenate([uni(rng, -3.0, 3.0, 3), q0])
        else:
            x0 = uni(rng, -1.0, 1.0, size)
        x = x0.copy()
        if perturb:
            if size == 7:
                x[:3] += uni(rng, -perturb, perturb, 3)
                step = dq if dq is not None else unit(np.concatenate([uni(rng, -perturb, perturb, 3), [1.0]]))
                x[3:] = unit(qmul(x0[3:], step))
            else:
                x += uni(rng, -perturb, perturb, size)
        if i in negate:
            x[3:] = -x[3:]
        blocks.append(dict(id=i, size=size, idx=idx, x0=x0)); params.append(x)
        idx += 6 if size == 7 else size
    n = idx
    J0 = uni(rng, -1.0, 1.0, (n, n))
    if decades:
        J0 = J0 * np.array(DECADES)[rng.integers(0, len(DECADES), (n, n))]
    return dict(J0=J0, r0=uni(rng, -1.0, 1.0, n), blocks=blocks, params=params, n=n)


def prior_cases():
    rng = rng_of(9800)
    c = {}
    c["x_equals_x0"] = _prior_case(rng, LAYOUT_11, 0.0, exact_quats=True)
    c["small_step"] = _prior_case(rng, LAYOUT_11, 0.01)
    c["negated_quaternions"] = _prior_case(rng_of(9801), LAYOUT_11, 0.01, negate=range(12))
    c["negated_quaternions"]["same_as"] = "negated_quaternions_base"
    c["negated_quaternions_base"] = _prior_case(rng_of(9801), LAYOUT_11, 0.01)
    axis = unit([0.2, -0.7, 0.4])
    for name, w in (("w_plus_1e-3", 1e-3), ("w_minus_1e-3", -1e-3)):
        c[name] = _prior_case(rng, LAYOUT_11, 0.01, dq=np.concatenate([axis * np.sqrt(1.0 - w * w), [w]]))
    c["n_157"] = _prior_case(rng, LAYOUT_157, 0.01)
    c["n_1"] = _prior_case(rng, [1], 0.01)
    c["J0_1e-6_to_1e6"] = _prior_case(rng, LAYOUT_11, 0.01, decades=True)
    return c
