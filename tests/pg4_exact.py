"""High-precision yardstick of the 4-DoF pose graph (TEST INFRASTRUCTURE): the text of include/vilfusion.h written from the definitions in mpmath at 40 digits.

It shares no formula with tests/pg4_reference.py or vilf_pg4.hip: a rotation is the product of three elementary rotations, a Jacobian is a central
difference in mp (h = 1e-15: truncation ~1e-30, rounding ~1e-25), the normal equations are dense and solved by mp.cholesky_solve. Only the
Levenberg-Marquardt rule itself is, necessarily, the same rule. A graph costs about 0.3 s per attempt at n = 12: keep n <= 16.

run(case, snapshots) makes ONE run of max(snapshots) attempts and records the state after each snapshot count: the state of a run with max_iterations = k
is the state of a longer run after k attempts, with VILF_PG4_MAX_ITERATIONS set if no other rule has ended it by then."""
import functools

import mpmath as mp
import numpy as np

DPS = 40
F_MAX_ITERATIONS, F_FUNCTION, F_GRADIENT, F_PARAMETER, F_RADIUS, F_FINITE = 1, 2, 4, 8, 16, 32


def _f(v):
    return mp.mpf(float(v))


def _norm_angle(a):
    if a > 180:
        return a - 360
    if a < -180:
        return a + 360
    return a


@functools.lru_cache(maxsize=4096)
def _rot(y, p, r):
    y, p, r = [v * mp.pi / 180 for v in (y, p, r)]
    Rz = mp.matrix([[mp.cos(y), -mp.sin(y), 0], [mp.sin(y), mp.cos(y), 0], [0, 0, 1]])
    Ry = mp.matrix([[mp.cos(p), 0, mp.sin(p)], [0, 1, 0], [-mp.sin(p), 0, mp.cos(p)]])
    Rx = mp.matrix([[1, 0, 0], [0, mp.cos(r), -mp.sin(r)], [0, mp.sin(r), mp.cos(r)]])
    return Rz * Ry * Rx


def _ypr(R):
    y = mp.atan2(R[1, 0], R[0, 0])
    p = mp.atan2(-R[2, 0], R[0, 0] * mp.cos(y) + R[1, 0] * mp.sin(y))
    r = mp.atan2(R[0, 2] * mp.sin(y) - R[1, 2] * mp.cos(y), -R[0, 1] * mp.sin(y) + R[1, 1] * mp.cos(y))
    return [v * 180 / mp.pi for v in (y, p, r)]


def _residual(x8, pitch, roll, rel_t, rel_yaw, w):
    """x8 = yaw_i, t_i, yaw_j, t_j"""
    R = _rot(x8[0], pitch, roll)
    d = mp.matrix([x8[5] - x8[1], x8[6] - x8[2], x8[7] - x8[3]])
    e = R.T * d
    return [e[0] - rel_t[0], e[1] - rel_t[1], e[2] - rel_t[2], w * _norm_angle(x8[4] - x8[0] - rel_yaw)]


def _rho(s, a):
    """(rho, rho') of Huber(a); a None: no loss"""
    if a is None or s <= a * a:
        return s, mp.mpf(1)
    return 2 * a * mp.sqrt(s) - a * a, a / mp.sqrt(s)


class _Graph:
    def __init__(self, vio_R, vio_T, sequence, fixed, loops, P):
        n = len(vio_T)
        self.n, self.P = n, P
        Rm = [mp.matrix([[_f(np.asarray(vio_R[k]).reshape(3, 3)[a, b]) for b in range(3)] for a in range(3)]) for k in range(n)]
        self.t0 = [[_f(v) for v in np.asarray(vio_T[k]).reshape(3)] for k in range(n)]
        e = [_ypr(Rm[k]) for k in range(n)]
        self.yaw0, self.pitch, self.roll = [v[0] for v in e], [v[1] for v in e], [v[2] for v in e]
        self.edges = []
        for i in range(n):
            for j in range(1, 5):
                if i - j >= 0 and sequence[i] == sequence[i - j]:
                    d = mp.matrix([self.t0[i][c] - self.t0[i - j][c] for c in range(3)])
                    rt = Rm[i - j].T * d
                    self.edges.append((i - j, i, [rt[0], rt[1], rt[2]], self.yaw0[i] - self.yaw0[i - j], mp.mpf(1), None))
        for (a, b, rel_t, rel_yaw) in loops:
            self.edges.append((int(a), int(b), [_f(v) for v in rel_t], _f(rel_yaw), _f(P["loop_yaw_scale"]), _f(P["huber"])))
        self.col, self.m = [], 0
        for k in range(n):
            self.col.append(-1 if fixed[k] else self.m)
            self.m += 0 if fixed[k] else 4
        self.free = [k for k in range(n) if not fixed[k]]

    def x8(self, e, yaw, t):
        i, j = e[0], e[1]
        return [yaw[i]] + list(t[i]) + [yaw[j]] + list(t[j])

    def cost(self, yaw, t):
        c = mp.mpf(0)
        for e in self.edges:
            r = _residual(self.x8(e, yaw, t), self.pitch[e[0]], self.roll[e[0]], e[2], e[3], e[4])
            c += _rho(sum(v * v for v in r), e[5])[0]
        return c / 2

    def linearize(self, yaw, t):
        """cost, H, g over the free columns; central differences of the plain residual, then the robust scaling"""
        h = mp.mpf(10) ** -15
        m = self.m
        H, g, c = mp.zeros(max(m, 1), max(m, 1)), mp.zeros(max(m, 1), 1), mp.mpf(0)
        for e in self.edges:
            x = self.x8(e, yaw, t)
            args = (self.pitch[e[0]], self.roll[e[0]], e[2], e[3], e[4])
            r = _residual(x, *args)
            rho, rho1 = _rho(sum(v * v for v in r), e[5])
            c += rho
            k = mp.sqrt(rho1)
            cols, J = [], []
            for side, node in ((0, e[0]), (1, e[1])):
                if self.col[node] < 0:
                    continue
                for u in range(4):
                    xp, xm = list(x), list(x)
                    xp[4 * side + u] += h
                    xm[4 * side + u] -= h
                    rp, rm = _residual(xp, *args), _residual(xm, *args)
                    cols.append(self.col[node] + u)
                    J.append([k * (rp[a] - rm[a]) / (2 * h) for a in range(4)])
            for a, ca in enumerate(cols):
                g[ca] += sum(J[a][q] * k * r[q] for q in range(4))
                for b, cb in enumerate(cols):
                    H[ca, cb] += sum(J[a][q] * J[b][q] for q in range(4))
        return c / 2, H, g


def _solve(H, g, mu, m):
    A = H.copy()
    for a in range(m):
        A[a, a] += H[a, a] / mu
    try:
        return mp.cholesky_solve(A, -g)
    except (ValueError, ZeroDivisionError):
        return None


def run(vio_R, vio_T, sequence, fixed, loops, P, snapshots=(1, 2, 5)):
    """-> {k: dict(t, yaw, flags, cost1, radius, iterations, accepted, history [..][5])} for k in snapshots (and k = 0 when asked for)"""
    with mp.workdps(DPS):
        return _run(vio_R, vio_T, sequence, fixed, loops, P, tuple(snapshots))


def _run(vio_R, vio_T, sequence, fixed, loops, P, snapshots):
    G = _Graph(vio_R, vio_T, sequence, fixed, loops, P)
    m = G.m
    yaw, t = list(G.yaw0), [list(v) for v in G.t0]
    cost, H, g = G.linearize(yaw, t)
    gmax = max([abs(g[a]) for a in range(m)] or [mp.mpf(0)])
    mu, factor, flags = _f(P["initial_radius"]), mp.mpf(2), 0
    it = accepted_n = 0
    history, out = [], {}
    cost0 = cost

    def snap(k, stopped):
        out[k] = dict(t=np.array([[float(v) for v in row] for row in t]), yaw=np.array([float(v) for v in yaw]),
                      flags=(flags if stopped else F_MAX_ITERATIONS) | F_FINITE, cost0=float(cost0), cost1=float(cost), radius=float(mu),
                      iterations=it, accepted=accepted_n, history=np.array(history, float).reshape(-1, 5),
                      margins=list(margins))

    margins = []          # how far every decision of the run was from its threshold (relative): the case file asserts they are not at equality
    if gmax <= _f(P["gradient_tolerance"]):
        flags |= F_GRADIENT
    for k in snapshots:
        if k == 0:
            snap(0, bool(flags))
    while not flags and it < max(snapshots):
        it += 1
        mu_before = mu
        delta = _solve(H, g, mu, m) if m else mp.zeros(1, 1)
        if delta is None:
            history.append([float(cost), float(cost), 0.0, float(mu_before), -1.0])
            accepted = False
        else:
            yaw_c = list(yaw)
            t_c = [list(v) for v in t]
            for k in G.free:
                c0 = G.col[k]
                yaw_c[k] = _norm_angle(yaw[k] + delta[c0])
                t_c[k] = [t[k][u] + delta[c0 + 1 + u] for u in range(3)]
            cost_c = G.cost(yaw_c, t_c)
            dg = sum(delta[a] * g[a] for a in range(m))
            Hd = H * delta if m else mp.zeros(1, 1)
            model = -(dg + sum(delta[a] * Hd[a] for a in range(m)) / 2)
            rho = (cost - cost_c) / model
            mrd = _f(P["min_relative_decrease"])
            accepted = rho > mrd
            margins.append(("rho", float(abs(rho - mrd) / mrd) if mrd else 1.0))
            history.append([float(cost), float(cost_c), float(rho), float(mu_before), 1.0 if accepted else 0.0])
        if accepted:
            accepted_n += 1
            xn = mp.sqrt(sum(yaw[k] ** 2 + sum(v * v for v in t[k]) for k in G.free))
            dn = mp.sqrt(sum(delta[a] ** 2 for a in range(m)))
            decrease = cost - cost_c
            old_cost = cost
            yaw, t = yaw_c, t_c
            mu = min(mu / max(mp.mpf(1) / 3, 1 - (2 * rho - 1) ** 3), _f(P["max_radius"]))
            factor = mp.mpf(2)
            ftol, gtol, ptol = _f(P["function_tolerance"]), _f(P["gradient_tolerance"]), _f(P["parameter_tolerance"])
            if decrease <= ftol * old_cost:
                flags |= F_FUNCTION
            cost, H, g = G.linearize(yaw, t)
            gmax = max(abs(g[a]) for a in range(m))
            if gmax <= gtol:
                flags |= F_GRADIENT
            if dn <= ptol * (xn + ptol):
                flags |= F_PARAMETER
            for name, lhs, rhs in (("function", decrease, ftol * old_cost), ("gradient", gmax, gtol), ("parameter", dn, ptol * (xn + ptol))):
                if rhs > 0:
                    margins.append((name, float(abs(lhs - rhs) / rhs)))
        else:
            mu /= factor
            factor *= 2
            if mu < _f(P["min_radius"]):
                flags |= F_RADIUS
        if it in snapshots:
            snap(it, bool(flags))
    for k in snapshots:                  # the run ended before these counts: the state is the final one
        if k not in out:
            snap(k, True)
    return out
