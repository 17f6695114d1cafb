"""numpy restatement of the 4-DoF pose graph of include/vilfusion.h ("Visual loop closure, third stage"), fp64, dense normal equations (TEST INFRASTRUCTURE).

It is what the layout-edge and end-to-end GPU tests compare vilf_pg4_optimize with, and the CPU back-end of the VisualPoseGraph tests (Backend). It is itself
measured against tests/pg4_exact.py, which shares no formula with it. No chain, no Woodbury: J is dense, H = J^T J, the damped system goes through
numpy's Cholesky.

  unknowns     per node [yaw (degrees), tx, ty, tz]; pitch and roll from R2ypr(vio_R), constant; columns of fixed nodes are dropped
  edge         r[0..2] = R(yaw_i, pitch_i, roll_i)^T (t_j - t_i) - rel_t, r[3] = w NormalizeAngle(yaw_j - yaw_i - rel_yaw); w = 1 (sequential), loop_yaw_scale (loop)
  loss         loops only: Huber(a) on s = |r|^2, rows scaled by sqrt(rho')
  minimiser    the Levenberg-Marquardt rule of the header, word for word"""
import math

import numpy as np

BAND = 4
F_MAX_ITERATIONS, F_FUNCTION, F_GRADIENT, F_PARAMETER, F_RADIUS, F_FINITE = 1, 2, 4, 8, 16, 32
D2R = math.pi / 180.0


def default_params():
    return dict(max_iterations=5, initial_radius=1e4, max_radius=1e16, min_radius=1e-32, min_relative_decrease=1e-3, function_tolerance=1e-6,
                gradient_tolerance=1e-10, parameter_tolerance=1e-8, huber=0.1, loop_yaw_scale=0.1)


def normalize_angle(a):
    """NormalizeAngle of pose_graph.h: one turn at the most"""
    if a > 180.0:
        return a - 360.0
    if a < -180.0:
        return a + 360.0
    return a


def R2ypr(R):
    y = math.atan2(R[1, 0], R[0, 0])
    p = math.atan2(-R[2, 0], R[0, 0] * math.cos(y) + R[1, 0] * math.sin(y))
    r = math.atan2(R[0, 2] * math.sin(y) - R[1, 2] * math.cos(y), -R[0, 1] * math.sin(y) + R[1, 1] * math.cos(y))
    return np.array([y, p, r]) / math.pi * 180.0


def ypr2R(y, p, r):
    """YawPitchRollToRotationMatrix (pose_graph.h:120-137), degrees, in closed form"""
    y, p, r = y * D2R, p * D2R, r * D2R
    cy, sy, cp, sp, cr, sr = math.cos(y), math.sin(y), math.cos(p), math.sin(p), math.cos(r), math.sin(r)
    return np.array([[cy * cp, -sy * cr + cy * sp * sr, sy * sr + cy * sp * cr],
                     [sy * cp, cy * cr + sy * sp * sr, -cy * sr + sy * sp * cr],
                     [-sp, cp * sr, cp * cr]])


def dR_dyaw(y, p, r):
    """d ypr2R / d yaw, per degree"""
    y, p, r = y * D2R, p * D2R, r * D2R
    cy, sy, cp, sp, cr, sr = math.cos(y), math.sin(y), math.cos(p), math.sin(p), math.cos(r), math.sin(r)
    return D2R * np.array([[-sy * cp, -cy * cr - sy * sp * sr, cy * sr - sy * sp * cr],
                           [cy * cp, -sy * cr + cy * sp * sr, sy * sr + cy * sp * cr],
                           [0.0, 0.0, 0.0]])


def build_edges(vio_R, vio_T, sequence, loops):
    """the edge list in the header's order: the sequential edges of node 0, 1, ... (j = 1 .. 4 each), then the loops. Rows (i, j, rel_t, rel_yaw, is_loop)."""
    n = len(vio_T)
    yaw0 = [R2ypr(np.asarray(vio_R[k]).reshape(3, 3))[0] for k in range(n)]
    edges = []
    for i in range(n):
        for j in range(1, BAND + 1):
            if i - j >= 0 and sequence[i] == sequence[i - j]:
                rel_t = np.asarray(vio_R[i - j]).reshape(3, 3).T @ (np.asarray(vio_T[i], float) - np.asarray(vio_T[i - j], float))
                edges.append((i - j, i, rel_t, yaw0[i] - yaw0[i - j], 0))
    for (a, b, rel_t, rel_yaw) in loops:
        edges.append((int(a), int(b), np.asarray(rel_t, float), float(rel_yaw), 1))
    return edges


def edge_block(e, yaw, t, pitch, roll, P):
    """robustified residual [4], Jacobians wrt node i and node j [4][4] each, rho of the block"""
    i, j, rel_t, rel_yaw, is_loop = e
    pr = i
    R = ypr2R(yaw[i], pitch[pr], roll[pr])
    d = t[j] - t[i]
    w = P["loop_yaw_scale"] if is_loop else 1.0
    r = np.empty(4)
    r[:3] = R.T @ d - rel_t
    r[3] = w * normalize_angle(yaw[j] - yaw[i] - rel_yaw)
    Ji, Jj = np.zeros((4, 4)), np.zeros((4, 4))
    Ji[:3, 0] = dR_dyaw(yaw[i], pitch[pr], roll[pr]).T @ d
    Ji[:3, 1:] = -R.T
    Jj[:3, 1:] = R.T
    Ji[3, 0], Jj[3, 0] = -w, w
    s = float(r @ r)
    rho = s
    if is_loop:
        a = P["huber"]
        if s > a * a:
            rho = 2.0 * a * math.sqrt(s) - a * a
            rho1 = a / math.sqrt(s)
            k = math.sqrt(rho1)
            r, Ji, Jj = k * r, k * Ji, k * Jj
    return r, Ji, Jj, rho


def linearize(edges, yaw, t, pitch, roll, col, m, P):
    """cost, J [4 E][m], r [4 E] over the free columns (col[k] = first column of node k, or -1)"""
    J, r = np.zeros((4 * len(edges), m)), np.zeros(4 * len(edges))
    cost = 0.0
    for k, e in enumerate(edges):
        rb, Ji, Jj, rho = edge_block(e, yaw, t, pitch, roll, P)
        r[4 * k:4 * k + 4] = rb
        if col[e[0]] >= 0:
            J[4 * k:4 * k + 4, col[e[0]]:col[e[0]] + 4] = Ji
        if col[e[1]] >= 0:
            J[4 * k:4 * k + 4, col[e[1]]:col[e[1]] + 4] = Jj
        cost += rho
    return 0.5 * cost, J, r


def cost_only(edges, yaw, t, pitch, roll, P):
    return 0.5 * sum(edge_block(e, yaw, t, pitch, roll, P)[3] for e in edges)


def solve_damped(H, g, mu):
    """(H + diag(H) / mu) delta = -g by Cholesky; None on a non-positive pivot"""
    A = H + np.diag(np.diag(H) / mu)
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None
    if not np.all(np.isfinite(L)):
        return None
    y = np.linalg.solve(L, -g)
    return np.linalg.solve(L.T, y)


def check(vio_R, vio_T, sequence, fixed, loops, P):
    """what the header refuses; returns None or the reason"""
    n = len(vio_T)
    if n < 1 or not fixed[0]:
        return "n < 1 or node 0 free"
    if not (np.all(np.isfinite(np.asarray(vio_R, float))) and np.all(np.isfinite(np.asarray(vio_T, float)))):
        return "input not finite"
    for (a, b, rel_t, rel_yaw) in loops:
        if not (0 <= a < b < n):
            return "loop endpoints"
        if not (np.all(np.isfinite(np.asarray(rel_t, float))) and math.isfinite(rel_yaw)):
            return "input not finite"
    if not 0 <= P["max_iterations"] <= 64:
        return "max_iterations"
    for k in ("initial_radius", "max_radius", "min_radius", "huber", "loop_yaw_scale"):
        if not (math.isfinite(P[k]) and P[k] > 0):
            return k
    for k in ("min_relative_decrease", "function_tolerance", "gradient_tolerance", "parameter_tolerance"):
        if not (math.isfinite(P[k]) and P[k] >= 0):
            return k
    return None


def optimize(vio_R, vio_T, sequence, fixed, loops, params=None):
    """-> dict(t [n][3], ypr [n][3], R [n][3][3], result, history [iterations][5]); raises ValueError on what the header refuses"""
    P = default_params()
    P.update(params or {})
    why = check(vio_R, vio_T, sequence, fixed, loops, P)
    if why:
        raise ValueError("pg4: " + why)
    vio_R = np.asarray(vio_R, float).reshape(-1, 3, 3)
    vio_T = np.asarray(vio_T, float).reshape(-1, 3)
    n = len(vio_T)
    ypr = np.array([R2ypr(vio_R[k]) for k in range(n)])
    yaw, pitch, roll, t = ypr[:, 0].copy(), ypr[:, 1].copy(), ypr[:, 2].copy(), vio_T.copy()
    edges = build_edges(vio_R, vio_T, sequence, loops)
    col, m = [], 0
    for k in range(n):
        col.append(-1 if fixed[k] else m)
        m += 0 if fixed[k] else 4
    free = [k for k in range(n) if not fixed[k]]

    def xnorm(yaw, t):
        return math.sqrt(sum(yaw[k] ** 2 + float(t[k] @ t[k]) for k in free))

    cost, J, r = linearize(edges, yaw, t, pitch, roll, col, m, P)
    H, g = J.T @ J, J.T @ r
    gmax = float(np.max(np.abs(g))) if m else 0.0
    res = dict(iterations=0, accepted=0, pivot_rejections=0, flags=0, cost0=cost, cost1=cost, radius=P["initial_radius"])
    history = []
    mu, factor, flags = P["initial_radius"], 2.0, 0
    if gmax <= P["gradient_tolerance"]:
        flags |= F_GRADIENT
    while not flags:
        if res["iterations"] >= P["max_iterations"]:
            flags |= F_MAX_ITERATIONS
            break
        res["iterations"] += 1
        mu_before = mu
        delta = solve_damped(H, g, mu) if m else np.zeros(0)
        ok, cost_c, rho = delta is not None, cost, 0.0
        if ok:
            yaw_c, t_c = yaw.copy(), t.copy()
            for k in free:
                yaw_c[k] = normalize_angle(yaw[k] + delta[col[k]])
                t_c[k] = t[k] + delta[col[k] + 1:col[k] + 4]
            cost_c = cost_only(edges, yaw_c, t_c, pitch, roll, P)
            Jd = J @ delta
            model = -(float(delta @ g) + 0.5 * float(Jd @ Jd))
            ok = math.isfinite(cost_c)
            if ok:
                rho = (cost - cost_c) / model
        if not ok:
            res["pivot_rejections"] += 1
            cost_c, rho = cost, 0.0
        accepted = ok and rho > P["min_relative_decrease"]
        history.append([cost, cost_c, rho, mu_before, (1.0 if accepted else 0.0) if ok else -1.0])
        if accepted:
            res["accepted"] += 1
            xn, dn = xnorm(yaw, t), float(np.linalg.norm(delta))
            decrease = cost - cost_c
            yaw, t = yaw_c, t_c
            mu = min(mu / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3), P["max_radius"])
            factor = 2.0
            if decrease <= P["function_tolerance"] * cost:
                flags |= F_FUNCTION
            cost, J, r = linearize(edges, yaw, t, pitch, roll, col, m, P)
            H, g = J.T @ J, J.T @ r
            if float(np.max(np.abs(g))) <= P["gradient_tolerance"]:
                flags |= F_GRADIENT
            if dn <= P["parameter_tolerance"] * (xn + P["parameter_tolerance"]):
                flags |= F_PARAMETER
        else:
            mu /= factor
            factor *= 2.0
            if mu < P["min_radius"]:
                flags |= F_RADIUS
    Rout = np.array([ypr2R(yaw[k], pitch[k], roll[k]) for k in range(n)])
    if np.all(np.isfinite(t)) and np.all(np.isfinite(yaw)) and math.isfinite(cost):
        flags |= F_FINITE
    res.update(flags=flags, cost1=cost, radius=mu)
    res.update(drift(Rout[n - 1], t[n - 1], vio_R[n - 1], vio_T[n - 1]))
    return dict(t=t, ypr=np.stack([yaw, pitch, roll], axis=1), R=Rout, result=res, history=np.array(history, float).reshape(-1, 5))


def drift(R_out, t_out, vio_R, vio_T):
    """pose_graph.cpp:552-560 for the last node"""
    yaw_drift = R2ypr(np.asarray(R_out))[0] - R2ypr(np.asarray(vio_R))[0]
    r_drift = ypr2R(yaw_drift, 0.0, 0.0)
    return dict(yaw_drift=yaw_drift, r_drift=r_drift, t_drift=np.asarray(t_out, float) - r_drift @ np.asarray(vio_T, float))


class Backend:
    """stands for BackendSolver.optimize4dof in the CPU tests of VisualPoseGraph"""

    def optimize4dof(self, vio_R, vio_T, sequence, fixed, loops, params=None, history=False):
        out = optimize(vio_R, vio_T, sequence, fixed, loops, params)
        return out
