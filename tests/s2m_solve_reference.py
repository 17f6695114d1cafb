"""The scan-to-map pose solve restated from the reference's text and from what Ceres documents, for tests/test_scan2map_solve.py. numpy and mpmath only;
written from lidarFactor.hpp (EdgeCostFunction :21-52, SurfCostFunction :79-102), EstimationMapping.hpp:34-49 (LocalSE3Parameterization::Plus), common.h:137-176
(getTransformFromSe3) and Ceres' trust-region / Levenberg-Marquardt documentation — not from the kernel and not from oracle/solver.cpp.

Rules (each was checked against b_solve; DESIGN 3m lists the result):
  R1  residuals. lp = q * cp + t with Eigen's q * v (uv = 2 qv x v; v + w uv + qv x uv, no normalisation). Edge: (lp - pa) x (lp - pb) / |pa - pb|, jacobian
      [skew(pa - pb) skew(lp) | -skew(pa - pb)] / |pa - pb| (rotation first). Plane: n . lp + d, jacobian [-(n x lp) | n]. The local parameterisation's jacobian is
      the identity on the six tangent coordinates.
  R2  Huber(a): s = |r|^2; s > a^2: rho0 = 2 a sqrt(s) - a^2, rho1 = a / sqrt(s); otherwise rho0 = s, rho1 = 1. Residual and jacobian are scaled by sqrt(rho1)
      (rho2 <= 0: Ceres' corrector has no second-order part). cost = 1/2 sum rho0; g = J^T r; H = J^T J of the scaled rows.
  R3  Jacobi scaling 1 / (1 + sqrt(H_cc)), fixed at the first evaluation.
  R4  the diagonal of the scaled H clamped to [1e-6, 1e32]; after a rejected step the diagonal of the previous iteration is reused.
  R5  the step solves (Hs + D / radius) y = -gs; delta = y * scale. radius starts at 1e4, decrease_factor at 2.
  R6  model cost change = -y . (gs + Hs y / 2); a step is valid when it is > 0 (five invalid steps in a row end the loop).
  R7  candidate = Plus(x, delta): theta = |omega|; imag = sin(theta / 2) / theta, below 1e-10: 1/2 - 0.0208333 theta^2 + 0.000260417 theta^4; real =
      cos(theta / 2); dq = (imag omega, real); J = I + (1 - cos theta) / theta^2 Omega + (theta - sin theta) / theta^3 Omega^2, below 1e-10: dq's matrix (Eigen's
      toRotationMatrix); q+ = dq q; t+ = dq * t + J upsilon.
  R8  parameter stop: |x - candidate| <= 1e-8 (|x| + 1e-8), norms over the seven ambient coordinates; then the function stop: |cost - candidate cost| <= 1e-6 cost.
      Both end the loop WITHOUT taking the candidate.
  R9  rd = (cost - candidate cost) / model cost change; accepted when rd > 1e-3: radius = min(1e16, radius / max(1/3, 1 - (2 rd - 1)^3)), decrease_factor = 2;
      rejected: radius /= decrease_factor, decrease_factor *= 2.
  R10 before an iteration: the budget (iterations >= max_it), the gradient stop max |x - Plus(x, -g)| <= 1e-10, the minimum radius 1e-32.
  its counts every iteration begun, accepted or not.

Two tiers run the same rules through one piece of code (`solve`) over two kinds of number: the RESTATEMENT in float64 (every factor of every slot, vectorised, the 28
sums in slot order — numpy's cumulative sum) and the EXACT TIER in mpmath at 60 digits over the distinct factors of a case with a multiplicity each.

First-evaluation bound: first_bounds() derives it and states the operation counts (C_SUM = 9, C_OPS = 12).

Decisions. A decision is DECIDED when the exact quantity is further from its threshold than SAFETY = 64 x a bound on the evaluated quantity's rounding error. The
bounds are propagated forward: B(x) are the first-evaluation bounds of the 28 sums at x, including to first order the error x itself carries; the step inherits
|A^-1| (|dA| |y| + |dg| + 50 u |A| |y|) componentwise; model cost change, candidate, candidate cost, rd follow by the product rule (solve() has the formulas next to
the quantities). The error an iterate carries into the next row is the tolerance the tests hold it to at that row (tolerance_x), not the forward bound. A case named exact_* sits ON a threshold with every operation involved exact in fp64 (s2m_solve_cases says which); there the
decision is counted as decided when the exact quantity EQUALS the threshold value the case states and the restatement reproduces it to the bit."""
import math
import numpy as np
import mpmath as mp

U = 2.0 ** -53
SAFETY = 64.0
C_SUM = 9
C_OPS = 12
MP_DIGITS = 60
STOP_NONE, STOP_PARAMETER, STOP_FUNCTION, STOP_GRADIENT, STOP_BUDGET, STOP_RADIUS, STOP_INVALID = range(7)
LOW = [(a, b) for a in range(6) for b in range(a + 1)]          # lower-packed order of H: (0,0) (1,0) (1,1) (2,0) ...


class F64:
    """the number kind of the restatement"""
    name = "f64"

    @staticmethod
    def num(v):
        return float(v)

    @staticmethod
    def arr(a):
        return np.asarray(a, dtype=np.float64)

    sqrt = staticmethod(math.sqrt)
    sin = staticmethod(math.sin)
    cos = staticmethod(math.cos)

    @staticmethod
    def vsqrt(a):
        return np.sqrt(a)

    @staticmethod
    def total(terms, mult):
        """Sum in slot order over 256 strided partial sums (term j joins partial j mod 256, each partial a serial sum in slot order), then a binary tree over the
        partials: the serial depth ceil(n / 256) that the first-evaluation bound assumes. One serial sum over 33 000 equal terms exceeds that bound."""
        n = len(terms)
        if n == 0:
            return np.zeros(terms.shape[1:])
        m = -(-n // 256)
        pad = np.zeros((m * 256,) + terms.shape[1:])
        pad[:n] = terms
        part = np.cumsum(pad.reshape((m, 256) + terms.shape[1:]), axis=0)[-1]
        while len(part) > 1:
            part = part[0::2] + part[1::2]
        return part[0]


class MPF:
    """the number kind of the exact tier: object arrays of mpf"""
    name = "mp"

    @staticmethod
    def num(v):
        return mp.mpf(v)

    @staticmethod
    def arr(a):
        a = np.asarray(a)
        return np.array([mp.mpf(float(v)) if not isinstance(v, mp.mpf) else v for v in a.ravel()], dtype=object).reshape(a.shape)

    sqrt = staticmethod(mp.sqrt)
    sin = staticmethod(mp.sin)
    cos = staticmethod(mp.cos)

    @staticmethod
    def vsqrt(a):
        return np.array([mp.sqrt(v) for v in a.ravel()], dtype=object).reshape(a.shape)

    @staticmethod
    def total(terms, mult):
        out = [mp.mpf(0)] * terms.shape[1]
        for i in range(terms.shape[0]):
            m = int(mult[i])
            out = [o + m * t for o, t in zip(out, terms[i])]
        return np.array(out, dtype=object)


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _lp(x, cp):
    """R1: q * cp + t"""
    qv, w, t = [x[0], x[1], x[2]], x[3], [x[4], x[5], x[6]]
    uv = [2 * c for c in _cross(qv, cp)]
    k = _cross(qv, uv)
    return [cp[a] + w * uv[a] + k[a] + t[a] for a in range(3)]


def factor_rows(K, x, kind, rec, cp):
    """R1 for every factor given: residual rows [3] and jacobian rows [3][6] (a plane uses row 0, its other rows are zeros), s = |r|^2.
    kind [n] (1 edge, 2 plane), rec [n, 6], cp [n, 3] as arrays of K's numbers; x a list of 7."""
    cpl = [cp[:, a] for a in range(3)]
    r6 = [rec[:, a] for a in range(6)]
    lp = _lp(x, cpl)
    is_e = kind == 1
    pa, pb = r6[0:3], r6[3:6]
    u = [lp[a] - pa[a] for a in range(3)]
    v = [lp[a] - pb[a] for a in range(3)]
    ab = [pa[a] - pb[a] for a in range(3)]
    nrm2 = ab[0] * ab[0] + ab[1] * ab[1] + ab[2] * ab[2]
    nrm2 = np.where(is_e, nrm2, nrm2 * 0 + 1)
    nrm = K.vsqrt(nrm2)                                        # the reference divides by ab_norm (lidarFactor.hpp:31-33, :47); it forms no reciprocal
    re = [c / nrm for c in _cross(u, v)]

    def skew(w_):
        z = w_[0] * 0
        return [[z, -w_[2], w_[1]], [w_[2], z, -w_[0]], [-w_[1], w_[0], z]]
    Sab, Slp = skew(ab), skew(lp)
    Je = [[(Sab[i][0] * Slp[0][j] + Sab[i][1] * Slp[1][j] + Sab[i][2] * Slp[2][j]) / nrm for j in range(3)] + [-Sab[i][j] / nrm for j in range(3)] for i in range(3)]
    nv, d = r6[0:3], r6[3]
    rs = nv[0] * lp[0] + nv[1] * lp[1] + nv[2] * lp[2] + d
    nxl = _cross(nv, lp)
    Js = [-nxl[a] for a in range(3)] + [nv[a] for a in range(3)]
    zero = rs * 0
    rows_r = [np.where(is_e, re[0], rs), np.where(is_e, re[1], zero), np.where(is_e, re[2], zero)]
    rows_J = [[np.where(is_e, Je[0][c], Js[c]) for c in range(6)], [np.where(is_e, Je[1][c], zero) for c in range(6)], [np.where(is_e, Je[2][c], zero) for c in range(6)]]
    s = rows_r[0] * rows_r[0] + rows_r[1] * rows_r[1] + rows_r[2] * rows_r[2]
    return dict(rows_r=rows_r, rows_J=rows_J, s=s, lp=lp, nrm=nrm, u=u, v=v, ab=ab)


def _weights(K, s, huber_a):
    """R2 -> (outer, rho0, sqrt(rho1))"""
    a = K.num(huber_a)
    b = a * a
    outer = np.array(s > b, dtype=bool)
    one = s * 0 + 1
    r = K.vsqrt(np.where(outer, s, one))
    rho0 = np.where(outer, 2 * a * r - b, s)
    sw = K.vsqrt(np.where(outer, a / r, one))
    return outer, rho0, sw


def evaluate(K, x, case):
    """cost, g, H at x over the valid factors of a case, in K's numbers. K = F64: every slot; K = MPF: the distinct factors with their multiplicities.
    -> dict(sums [28] (H lower-packed, g, cost), s [n], outer [n])"""
    f = case["f64" if K is F64 else "mp"]
    kind, rec, cp, mult = f["kind"], f["rec"], f["cp"], f["mult"]
    if len(kind) == 0:
        return dict(sums=np.array([K.num(0)] * 28, dtype=object if K is MPF else np.float64), s=np.zeros(0), outer=np.zeros(0, dtype=bool))
    t = factor_rows(K, x, kind, rec, cp)
    outer, rho0, sw = _weights(K, t["s"], case["huber_a"])
    jr = [[sw * t["rows_J"][k][c] for c in range(6)] for k in range(3)]
    rk = [sw * t["rows_r"][k] for k in range(3)]
    cols = [jr[0][p] * jr[0][q] + jr[1][p] * jr[1][q] + jr[2][p] * jr[2][q] for (p, q) in LOW]
    cols += [jr[0][c] * rk[0] + jr[1][c] * rk[1] + jr[2][c] * rk[2] for c in range(6)]
    cols.append(rho0 / 2)
    return dict(sums=K.total(np.stack(cols, axis=1), mult), s=t["s"], outer=outer)


def first_bounds(case, x, dx=0.0):
    """The derived bound on the rounding error of the 28 sums of an evaluation at x (first-order, float64 arithmetic on the distinct factors and their multiplicities),
    for an x that itself carries an error of at most dx. -> (B [28], es [n]: the bound on each factor's s)

      B_k = (ceil(n_valid / 256) + C_SUM) u sum |term| + sum E(term)

    The first part is the summation (a lane's serial sum of ceil(n / 256) terms, six butterfly levels, three wave partials: C_SUM = 9) and the term's own C_OPS = 12
    products and sums after its inputs (weight twice, two products, two additions, the square roots and the division of the weight). E(term) is what the inputs
    carry into the term: lp = q * cp + t comes with e_lp = 8 u (|R||cp| + |t|) (depth 8) — an ABSOLUTE error, so it does not shrink with lp - pa or n . lp + d,
    which is why no bound of the form c u |term| holds for a map a few hundred metres from the origin; from there by the product rule: edge residual
    ((|u| + |v|) e_lp + 4 u |u||v|) / |ab| + 8 u |r|, its rotational jacobian e_lp + 4 u |lp| + 8 u |J|, plane residual |n|_1 e_lp + 4 u (|n||lp| + |d|),
    its rotational jacobian |n| e_lp + 3 u |n||lp|, s: 2 |r| e_r + 4 u s, the weight beyond a^2: e_s / (2 s) + 3 u relative."""
    src = case["mp_src"]
    kind, rec, cp, mult = src["kind"], src["rec"], src["cp"], src["mult"].astype(np.float64)
    xf = [float(v) for v in x]
    if len(kind) == 0:
        return np.zeros(28), np.zeros(0)
    t = factor_rows(F64, xf, kind, F64.arr(rec), F64.arr(cp))
    is_e = kind == 1
    qn = sum(v * v for v in xf[:4])
    cpn = np.linalg.norm(cp, axis=1)
    tn = math.sqrt(sum(v * v for v in xf[4:]))
    lpn = np.sqrt(t["lp"][0] ** 2 + t["lp"][1] ** 2 + t["lp"][2] ** 2)
    el = 8 * U * (3 * qn * cpn + tn) + 2 * dx * (1 + cpn)
    un = np.sqrt(t["u"][0] ** 2 + t["u"][1] ** 2 + t["u"][2] ** 2); vn = np.sqrt(t["v"][0] ** 2 + t["v"][1] ** 2 + t["v"][2] ** 2)
    abn = t["nrm"]
    rows_r = [np.abs(r) for r in t["rows_r"]]
    rows_J = [[np.abs(j) for j in row] for row in t["rows_J"]]
    rn = np.sqrt(t["s"])
    nn1 = np.abs(rec[:, 0]) + np.abs(rec[:, 1]) + np.abs(rec[:, 2])
    er = np.where(is_e, ((un + vn) * el + 4 * U * un * vn) / abn + 8 * U * rn, nn1 * el + 4 * U * (nn1 * lpn + np.abs(rec[:, 3])))
    ej_rot = np.where(is_e, el + 4 * U * lpn, nn1 * el + 3 * U * nn1 * lpn)
    ej = [[(ej_rot if c < 3 else 0.0) + 8 * U * rows_J[k][c] for c in range(6)] for k in range(3)]
    es = 2 * rn * er + 4 * U * t["s"]
    outer, rho0, sw = _weights(F64, t["s"], case["huber_a"])
    dw2 = np.where(outer, es / (2 * np.where(outer, t["s"], 1.0)) + 3 * U, 0.0)
    w2 = sw * sw
    nrows = np.where(is_e, 3, 1)
    depth = (math.ceil(case["n_valid"] / 256) + C_SUM + C_OPS) * U
    B = np.zeros(28)
    for e, (p, q) in enumerate(LOW):
        ta = w2 * sum(rows_J[k][p] * rows_J[k][q] for k in range(3))
        E = w2 * sum((rows_J[k][p] * ej[k][q] + rows_J[k][q] * ej[k][p]) * (k < nrows) for k in range(3)) + dw2 * ta
        B[e] = float(np.sum(mult * (depth * ta + E)))
    for c in range(6):
        ta = w2 * sum(rows_J[k][c] * rows_r[k] for k in range(3))
        E = w2 * sum((rows_J[k][c] * er + rows_r[k] * ej[k][c]) * (k < nrows) for k in range(3)) + dw2 * ta
        B[21 + c] = float(np.sum(mult * (depth * ta + E)))
    a = float(case["huber_a"])
    ta = np.where(outer, a * rn + a * a / 2, t["s"] / 2)
    E = np.where(outer, a * rn * es / (2 * np.where(outer, t["s"], 1.0)), es / 2)
    B[27] = float(np.sum(mult * (depth * ta + E)))
    return B, es


def se3_plus(K, x, d):
    """R7. -> (x+ [7], small: the theta < 1e-10 branch, theta)"""
    om, up = d[0:3], d[3:6]
    th = K.sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2])
    small = th < 1e-10
    real = K.cos(th / 2)
    if small:
        t2 = th * th
        imag = K.num(0.5) - K.num(0.0208333) * t2 + K.num(0.000260417) * (t2 * t2)
    else:
        imag = K.sin(th / 2) / th
    dq = [imag * om[0], imag * om[1], imag * om[2], real]
    if small:
        qx, qy, qz, qw = dq
        tx, ty, tz = 2 * qx, 2 * qy, 2 * qz
        twx, twy, twz = tx * qw, ty * qw, tz * qw
        txx, txy, txz = tx * qx, ty * qx, tz * qx
        tyy, tyz, tzz = ty * qy, tz * qy, tz * qz
        J = [[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]]
    else:
        O = [[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]]
        O2 = [[sum(O[i][k] * O[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
        ca = (1 - K.cos(th)) / (th * th)
        cb = (th - K.sin(th)) / (th * th * th)
        J = [[(1 if i == j else 0) + ca * O[i][j] + cb * O2[i][j] for j in range(3)] for i in range(3)]
    dt = [J[i][0] * up[0] + J[i][1] * up[1] + J[i][2] * up[2] for i in range(3)]
    a, b = dq, x[0:4]                                                  # Eigen's quaternion product dq * q, (x y z w)
    qn = [a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
          a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
          a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
          a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]]
    t = list(x[4:7])
    uv = [2 * c for c in _cross(dq[0:3], t)]
    k = _cross(dq[0:3], uv)
    rt = [t[i] + dq[3] * uv[i] + k[i] for i in range(3)]
    return qn + [rt[i] + dt[i] for i in range(3)], bool(small), th


def _chol_solve(K, A, b):
    """Cholesky of the 6 x 6 SPD matrix, two triangular solves; None when a pivot is not positive"""
    n = 6
    L = [[K.num(0)] * n for _ in range(n)]
    for j in range(n):
        sd = A[j][j] - sum(L[j][k] * L[j][k] for k in range(j))
        if not sd > 0:
            return None
        L[j][j] = K.sqrt(sd)
        for i in range(j + 1, n):
            L[i][j] = (A[i][j] - sum(L[i][k] * L[j][k] for k in range(j))) / L[j][j]
    y = [K.num(0)] * n
    for i in range(n):
        y[i] = (b[i] - sum(L[i][k] * y[k] for k in range(i))) / L[i][i]
    z = [K.num(0)] * n
    for i in reversed(range(n)):
        z[i] = (y[i] - sum(L[k][i] * z[k] for k in range(i + 1, n))) / L[i][i]
    return z


def _unpack(sums):
    H = [[None] * 6 for _ in range(6)]
    for e, (a, b) in enumerate(LOW):
        H[a][b] = H[b][a] = sums[e]
    return H, [sums[21 + c] for c in range(6)], sums[27]


def _f(v):
    return float(v)


def _norm(v):
    return math.sqrt(sum(_f(c) ** 2 for c in v))


def cost_bound(case, x, dx, g, H):
    """the cost at an x that carries dx: its own rounding, and the cost's change over dx to second order (a tangent step of at most 2 dx)"""
    return first_bounds(case, x)[0][27] + 2 * dx * _norm(g) + 2 * dx * dx * _norm([c for row in H for c in row])


def solve(K, case, decisions=False, rest=None):
    """The loop R3 .. R10 in K's numbers. -> dict(rows, pose, cost, its, why, nfe, nfs). rows[0]: x cost g H scale (+ bound [28] with decisions); rows[k]: valid
    accept stop reason diag step cand cand_cost mcc radius decrease_factor small theta (+ decided: dict of booleans, with decisions)."""
    n_valid = case["n_valid"]
    x = [K.num(v) for v in case["pose"]]
    out = dict(rows=[], nfe=case["nfe"], nfs=case["nfs"], pose=x, cost=K.num(0), its=0, why=STOP_NONE, all_decided=True, undecided=[])
    if n_valid == 0:
        return out
    a2 = _f(case["huber_a"]) ** 2
    ev = evaluate(K, x, case)
    H, g, cost = _unpack(ev["sums"])
    scale = [1 / (1 + K.sqrt(H[c][c])) for c in range(6)]
    row0 = dict(x=list(x), cost=cost, g=g, H=[H[a][b] for a, b in LOW], scale=scale)
    dx = 0.0                                       # bound on the error the iterate itself carries (ambient 2-norm)
    d_cost = 0.0

    def huber_decided(ev_, es_):
        ok = True
        for i in range(len(ev_["s"])):
            if ev_["s"][i] == mp.mpf(case["huber_a"]) ** 2 and case.get("exact_huber"):
                continue                           # ON the threshold with every operation exact (s2m_solve_cases): both branches give the same values there
            if not abs(_f(ev_["s"][i]) - a2) > SAFETY * es_[i]:
                ok = False
        return ok
    B = None
    if decisions:
        B, es0 = first_bounds(case, x)
        row0["bound"] = B
        d_cost = B[27]
        if not huber_decided(ev, es0):
            out["all_decided"] = False; out["undecided"].append((0, "huber"))
    out["rows"].append(row0)
    radius, dfac, reuse, diag = K.num(1e4), K.num(2), False, None
    x_norm = K.sqrt(sum(v * v for v in x))
    it, invalid, why = 0, 0, STOP_NONE
    max_it = case["max_it"]
    while True:
        dec = {}
        if it >= max_it:
            why = STOP_BUDGET
            break
        xp, _, _ = se3_plus(K, x, [-v for v in g])
        gm = max(abs(x[k] - xp[k]) for k in range(7))
        if decisions:
            bg = _norm(B[21:27])
            dec["gradient"] = abs(_f(gm) - 1e-10) > SAFETY * (bg * (1 + _norm(x[4:7])) + 8 * U * _norm(x))
        if gm <= 1e-10:
            why = STOP_GRADIENT
            if decisions and not dec["gradient"]:
                out["all_decided"] = False; out["undecided"].append((it, "gradient"))
            break
        if radius <= 1e-32:
            why = STOP_RADIUS
            break
        it += 1
        Hs = [[H[a][b] * scale[a] * scale[b] for b in range(6)] for a in range(6)]
        gs = [g[c] * scale[c] for c in range(6)]
        if decisions:
            BH = np.zeros((6, 6))
            for e, (a, b) in enumerate(LOW):
                BH[a][b] = BH[b][a] = B[e]
            BHs = BH * np.outer([_f(s) for s in scale], [_f(s) for s in scale])
            Bgs = B[21:27] * np.array([_f(s) for s in scale])
        if not reuse:
            diag = [min(max(Hs[c][c], K.num(1e-6)), K.num(1e32)) for c in range(6)]
            if decisions:
                # an exactly empty row (no factor touches the coordinate) is exact in every evaluation
                dec["clamp"] = all((_f(Hs[c][c]) == 0.0 and BHs[c][c] == 0.0) or abs(_f(Hs[c][c]) - 1e-6) > SAFETY * BHs[c][c] for c in range(6))
        A = [[Hs[a][b] + (diag[a] / radius if a == b else 0) for b in range(6)] for a in range(6)]
        y = _chol_solve(K, A, gs)
        reuse = True
        valid, accept, stop, reason = False, False, False, STOP_NONE
        row = dict(diag=list(diag), valid=0, accept=0, stop=0, reason=0, step=None, cand=None, cand_cost=None, mcc=None, small=None, theta=None, clamped=[bool(d == 1e-6) for d in diag])
        if y is not None:
            step = [-v for v in y]
            Hy = [sum(Hs[a][b] * step[b] for b in range(6)) for a in range(6)]
            mcc = -sum(step[a] * gs[a] for a in range(6)) - sum(step[a] * Hy[a] for a in range(6)) / 2
            row["step"], row["mcc"] = step, mcc
            valid = mcc > 0
        if not valid:
            invalid += 1
            radius = radius / dfac; dfac = dfac * 2
            row["radius"], row["dfac"] = radius, dfac
            out["rows"].append(row)
            if invalid >= 5:
                why = STOP_INVALID
                break
            continue
        invalid = 0
        row["valid"] = 1
        delta = [step[c] * scale[c] for c in range(6)]
        cand, small, th = se3_plus(K, x, delta)
        evc = evaluate(K, cand, case)
        Hc, gc, cc = _unpack(evc["sums"])
        row.update(cand=cand, cand_cost=cc, small=small, theta=th)
        sn = K.sqrt(sum((x[k] - cand[k]) * (x[k] - cand[k]) for k in range(7)))
        rd = None
        if decisions:
            # the step: |dy| <= |A^-1| (|dA| |y| + |dg| + 50 u |A| |y|) componentwise (the inputs' bounds and the Cholesky solve's own backward error)
            Af = np.array([[_f(v) for v in r_] for r_ in A])
            ya = np.abs(np.array([_f(v) for v in step]))
            sc = np.array([_f(s_) for s_ in scale])
            dyv = np.abs(np.linalg.inv(Af)) @ (BHs @ ya + Bgs + 50 * U * (np.abs(Af) @ ya))
            gsa = np.abs(np.array([_f(v) for v in gs])); Hya = np.abs(np.array([_f(v) for v in Hy]))
            d_mcc = float((gsa + Hya) @ dyv + ya @ Bgs + 0.5 * ya @ BHs @ ya + 20 * U * (ya @ gsa + 0.5 * ya @ Hya))
            dd = dyv * sc
            d_rot, d_trans = float(np.linalg.norm(dd[:3])), float(np.linalg.norm(dd[3:]))
            tn = _norm(x[4:7])
            d_delta = d_rot
            d_cand_x = d_rot * (1 + tn) + d_trans + 2 * dx * (1 + _norm(delta)) + 32 * U * (_norm(x) + _norm(delta))
            Bc, esc = first_bounds(case, cand, d_cand_x)
            d_cc = cost_bound(case, cand, d_cand_x, gc, Hc)
            # the rotational part of an exactly decoupled system is exact: gs, Hs rows of zeros give a step of zeros in every evaluation
            rot_exact = all(_f(gs[c]) == 0.0 and Bgs[c] == 0.0 for c in range(3)) and all(_f(Hs[a][b]) == 0.0 for a in range(3) for b in range(6) if a != b)
            dec["theta"] = rot_exact or abs(_f(th) - 1e-10) > SAFETY * d_delta
            dec["parameter"] = abs(_f(sn) - 1e-8 * (_f(x_norm) + 1e-8)) > SAFETY * (d_cand_x + dx + 8 * U * _norm(x))
            dec["function"] = abs(abs(_f(cost) - _f(cc)) - 1e-6 * _f(cost)) > SAFETY * (d_cost + d_cc)
            dec["huber"] = huber_decided(evc, esc)
            # What the tests floor their measured tolerance of this row's candidate cost and model cost change at: the same formulas fed with the tolerance the
            # candidate and the step are themselves held to at this row (tolerance_x), NOT with the forward bounds d_cand_x / dyv above, which serve the decisions only
            if rest is not None and len(rest["rows"]) > it and rest["rows"][it]["cand"] is not None:
                tol_y = tolerance_x(rest["rows"][it]["step"], step)
                row["f_cc"] = cost_bound(case, cand, tolerance_x(rest["rows"][it]["cand"], cand), gc, Hc)
                row["f_mcc"] = float(np.linalg.norm(gsa + Hya) * tol_y + ya @ Bgs + 0.5 * ya @ BHs @ ya + 20 * U * (ya @ gsa + 0.5 * ya @ Hya))
            else:
                row["f_cc"], row["f_mcc"] = d_cc, d_mcc
        if sn <= 1e-8 * (x_norm + 1e-8):
            stop, reason = True, STOP_PARAMETER
        elif abs(cost - cc) <= 1e-6 * cost:
            stop, reason = True, STOP_FUNCTION
        else:
            rd = (cost - cc) / mcc
            if decisions:
                dec["accept"] = abs(_f(rd) - 1e-3) > SAFETY * ((d_cost + d_cc) / _f(mcc) + abs(_f(rd)) * d_mcc / _f(mcc))
            if rd > 1e-3:
                accept = True
                radius = radius / max(K.num(1) / 3, 1 - (2 * rd - 1) ** 3)
                radius = min(K.num(1e16), radius)
                dfac = K.num(2); reuse = False
            else:
                radius = radius / dfac; dfac = dfac * 2
        row.update(accept=int(accept), stop=int(stop), reason=reason, radius=radius, dfac=dfac, rd=rd)
        if decisions:
            row["decided"] = dec
            for k_, v_ in dec.items():
                if not v_:
                    out["all_decided"] = False; out["undecided"].append((it, k_))
        out["rows"].append(row)
        if stop:
            why = reason
            break
        if accept:
            x, H, g, cost = cand, Hc, gc, cc
            x_norm = K.sqrt(sum(v * v for v in x))
            if decisions:
                # The iterate the next row starts from: whoever is compared with this tier is held to tolerance_x(row) on it first (the tests assert that), so
                # that tolerance IS the error the next row's inputs carry — not the forward bound d_cand_x, which a Newton-like iteration does not realise
                dx = tolerance_x(rest["rows"][it]["cand"], cand) if rest is not None and len(rest["rows"]) > it and rest["rows"][it]["cand"] is not None else d_cand_x
                B, _ = first_bounds(case, cand, dx)
                d_cost = cost_bound(case, cand, dx, gc, Hc)
    out.update(pose=x, cost=cost, its=it, why=why, d_cost=d_cost)
    return out


def tolerance_x(x_rest, x_exact):
    """the tolerance on an iterate: SAFETY x the restatement's own error against the exact tier at that row, floored at SAFETY u max(1, |x|) (2-norms over the seven)"""
    err = math.sqrt(sum(_f(mp.mpf(float(a)) - b) ** 2 for a, b in zip(x_rest, x_exact)))
    return SAFETY * max(err, U * max(1.0, _norm(x_exact)))


def tolerance_scalar(v_rest, v_exact, scale_=None):
    """the same for a scalar (a cost, the radius): floored at SAFETY u |v|"""
    return SAFETY * max(abs(_f(mp.mpf(float(v_rest)) - v_exact)), U * abs(_f(v_exact)) if scale_ is None else U * scale_)


def exact(case, rest=None):
    mp.mp.dps = MP_DIGITS
    return solve(MPF, case, decisions=True, rest=rest)


def restate(case):
    return solve(F64, case)
