"""numpy restatement of the third stage of the visual start-up, GlobalSFM's full bundle adjustment, written from the contract text in include/vilfusion.h ("Visual
start-up: GlobalSFM full BA").

Every float operation is one numpy elementwise operation on float64 values, so it is rounded on its own; sums are written out in the text's order. A feature that
does not take part in a sum contributes 0.0 to it, which leaves a sum that started from 0.0 as it is, bit for bit. residuals, total, candidate and output_pose are
sfm_reference's, imported and not copied; the two earlier stages come from there too. No code is shared with csrc."""
import numpy as np
from sfm_reference import residuals, total, candidate, output_pose, table, global_sfm, relative_pose  # noqa: F401  (the earlier stages, for the callers that run all)

CONVERGED, COST, FINITE = 1, 2, 4
DEFAULTS = dict(ba_iterations=20, lambda0=1e-3, function_tolerance=1e-6, cost_threshold=5e-3)
UPPER = [(a, b) for a in range(6) for b in range(a, 6)]
UPPER3 = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


def sym(r, c):
    """the place of entry (r, c) of a symmetric 3 x 3 matrix in its upper triangle"""
    return UPPER3.index((min(r, c), max(r, c)))


def free_count(k, l, newest):
    return 0 if k == l else (3 if k == newest else 6)


def first_index(k, l):
    return 6 * (k - (1 if k > l else 0))


def observation(P, X, u):
    """the paragraphs residual and Jacobian for all features at once under the pose P [3][4] -> (J0 [6], J1 [6], P0 [3], P1 [3], e0, e1), each entry [n]"""
    R, t = P[:, :3], P[:, 3]
    q, iz, xn, yn, e0, e1 = residuals(R, t, X, u)
    c0, c1 = xn * iz, yn * iz
    zero = np.zeros(len(X))
    J0 = [-(c0 * q[1]), iz * q[2] + c0 * q[0], -(iz * q[1]), iz, zero, -c0]
    J1 = [-(iz * q[2] + c1 * q[1]), c1 * q[0], iz * q[0], zero, iz, -c1]
    P0 = [iz * R[0, c] - c0 * R[2, c] for c in range(3)]
    P1 = [iz * R[1, c] - c1 * R[2, c] for c in range(3)]
    return J0, J1, P0, P1, e0, e1


def coupling(J0, J1, P0, P1):
    return [[J0[a] * P0[c] + J1[a] * P1[c] for c in range(3)] for a in range(6)]


def masked_total(terms, mask):
    """the paragraph "sums over features": terms a list of [n] arrays, mask [n] -> one total per term"""
    if len(mask) == 0:
        return np.zeros(len(terms))
    return total(np.where(mask[:, None], np.stack(terms, axis=1), 0.0))


class Window:
    def __init__(self, win, state):
        self.start, self.first, self.nobs, self.pts = table(win)
        self.nf, self.n = int(win["n_frames"]), len(self.start)
        self.member = np.asarray(state, dtype=np.uint8)[:self.n] != 0

    def seen(self, k):
        return self.member & (self.start <= k) & (k < self.start + self.nobs)

    def points(self, k):
        """p(f, k) for every feature, any row where f is not seen in k"""
        if len(self.pts) == 0:
            return np.zeros((self.n, 2))
        return self.pts[np.clip(self.first[:-1] + k - self.start, 0, len(self.pts) - 1)]


def cost_of(W, Pose, X):
    c = np.float64(0.0)
    for k in range(W.nf):
        _, _, _, _, e0, e1 = residuals(Pose[k, :, :3], Pose[k, :, 3], X, W.points(k))
        c = c + masked_total([e0 * e0 + e1 * e1], W.seen(k))[0]
    return c


def ldlt_solve(S, b):
    """the paragraph solve at the size of S, S read in its upper triangle -> x or None if a pivot is not > 0. The subtractions of entry (j, i) happen column by
    column in ascending k, as the text orders them."""
    nc = len(b)
    A, L, d = S.copy(), np.zeros((nc, nc)), np.zeros(nc)
    for k in range(nc):
        d[k] = A[k, k]
        if not d[k] > 0:
            return None
        L[k + 1:, k] = A[k, k + 1:] / d[k]
        A[k + 1:, k + 1:] = A[k + 1:, k + 1:] - A[k, k + 1:][None, :] * L[k + 1:, k][:, None]
    x = np.array(b, dtype=np.float64)
    for k in range(nc):
        x[k + 1:] = x[k + 1:] - L[k + 1:, k] * x[k]
    x = x / d
    for k in range(nc - 1, 0, -1):
        x[:k] = x[:k] - L[k, :k] * x[k]
    return x


def point_terms(W, Pose, X, lam, l):
    """-> (Vi [6] upper of the inverse, gp [3], pivots all > 0 among the members)"""
    n = W.n
    v, gp = [np.zeros(n) for _ in range(6)], [np.zeros(n) for _ in range(3)]
    for k in range(W.nf):
        s = W.seen(k)
        _, _, P0, P1, e0, e1 = observation(Pose[k], X, W.points(k))
        for i, (c, d) in enumerate(UPPER3):
            v[i] = np.where(s, v[i] + (P0[c] * P0[d] + P1[c] * P1[d]), v[i])
        for c in range(3):
            gp[c] = np.where(s, gp[c] + (P0[c] * e0 + P1[c] * e1), gp[c])
    v00, v11, v22 = v[0] + lam * v[0], v[3] + lam * v[3], v[5] + lam * v[5]
    d0 = v00
    L10, L20 = v[1] / d0, v[2] / d0
    d1 = v11 - v[1] * L10
    u = v[4] - v[2] * L10
    L21 = u / d1
    d2 = (v22 - v[2] * L20) - u * L21
    good = bool(np.all(((d0 > 0) & (d1 > 0) & (d2 > 0))[W.member]))
    i0, i1, i2 = 1.0 / d0, 1.0 / d1, 1.0 / d2
    m10, m21, m20 = -L10, -L21, L21 * L10 - L20
    Vi22 = i2
    Vi12, Vi02 = m21 * i2, m20 * i2
    Vi11 = i1 + m21 * Vi12
    Vi01 = m10 * i1 + m21 * Vi02
    Vi00 = (i0 + m10 * (m10 * i1)) + m20 * Vi02
    return [Vi00, Vi01, Vi02, Vi11, Vi12, Vi22], gp, good


def bundle_adjust(win, l, R, t, state, positions, chain_ok=True, **params):
    """the BA of one window from the start given -> dict(ok, flags, iterations, accepted, n_camera, n_members, n_residuals, l, cost0, cost1, lam, frames (dicts of
    R, t, Q, T), state, positions, lambdas: the damping of every iteration, rejections: per iteration None or what rejected its step, "V" a pivot of a member's V,
    "S" a pivot of the reduced system, "cost" a candidate that is no better)"""
    P = dict(DEFAULTS, **params)
    n = len(np.asarray(win["start_frame"]))
    nf = int(win["n_frames"])
    zero_frame = lambda: dict(R=np.zeros((3, 3)), t=np.zeros(3), Q=np.zeros((3, 3)), T=np.zeros(3))
    res = dict(ok=False, flags=0, iterations=0, accepted=0, n_camera=0, n_members=0, n_residuals=0, l=int(l), cost0=np.float64(0.0), cost1=np.float64(0.0),
               lam=np.float64(0.0), frames=[zero_frame() for _ in range(nf)], state=np.zeros(n, dtype=np.uint8), positions=np.zeros((n, 3)), lambdas=[], rejections=[])
    if l < 0 or not chain_ok:
        return res
    newest = nf - 1
    assert l <= nf - 2
    W = Window(win, state)
    X = np.where(W.member[:, None], np.asarray(positions, dtype=np.float64).reshape(-1, 3)[:n], 0.0)
    Pose = np.zeros((nf, 3, 4))
    Pose[:, :, :3] = np.asarray(R, dtype=np.float64).reshape(-1, 3, 3)[:nf]
    Pose[:, :, 3] = np.asarray(t, dtype=np.float64).reshape(-1, 3)[:nf]
    nc = 6 * nf - 9
    free = [(k, free_count(k, l, newest), first_index(k, l)) for k in range(nf) if free_count(k, l, newest) > 0]
    lam, ftol = np.float64(P["lambda0"]), np.float64(P["function_tolerance"])
    cost = cost0 = np.float64(0.0)
    converged = False
    with np.errstate(all="ignore"):
        for it in range(int(P["ba_iterations"])):
            res["iterations"] += 1
            res["lambdas"].append(lam)
            Vi, gp, good = point_terms(W, Pose, X, lam, l)
            obs = [observation(Pose[k], X, W.points(k)) for k in range(nf)]
            U, g, cost = {}, {}, np.float64(0.0)
            for k in range(nf):
                J0, J1, _, _, e0, e1 = obs[k]
                s = masked_total([J0[a] * J0[b] + J1[a] * J1[b] for a, b in UPPER] + [J0[a] * e0 + J1[a] * e1 for a in range(6)] + [e0 * e0 + e1 * e1], W.seen(k))
                U[k], g[k], cost = {ab: s[i] for i, ab in enumerate(UPPER)}, s[21:27], cost + s[27]
            if it == 0:
                cost0 = cost
            ok, why = good, None if good else "V"
            if ok:
                Wc = {k: coupling(*obs[k][:4]) for k, _, _ in free}
                Y = {k: [[(Wc[k][a][0] * Vi[sym(0, c)] + Wc[k][a][1] * Vi[sym(1, c)]) + Wc[k][a][2] * Vi[sym(2, c)] for c in range(3)] for a in range(6)] for k, _, _ in free}
                S, rhs = np.zeros((nc, nc)), np.zeros(nc)
                for j, nj, oj in free:
                    for k, nk, ok_ in free:
                        if k < j:
                            continue
                        both = W.seen(j) & W.seen(k)
                        idx = [(a, b) for a in range(nj) for b in range(nk) if j != k or a <= b]
                        T = masked_total([(Y[j][a][0] * Wc[k][b][0] + Y[j][a][1] * Wc[k][b][1]) + Y[j][a][2] * Wc[k][b][2] for a, b in idx], both)
                        for (a, b), tv in zip(idx, T):
                            if j == k:
                                Uab = U[k][(a, b)]
                                S[oj + a, ok_ + b] = ((Uab + lam * Uab) if a == b else Uab) - tv
                            else:
                                S[oj + a, ok_ + b] = -tv
                    Tg = masked_total([(Y[j][a][0] * gp[0] + Y[j][a][1] * gp[1]) + Y[j][a][2] * gp[2] for a in range(nj)], W.seen(j))
                    for a in range(nj):
                        rhs[oj + a] = -(g[j][a] - Tg[a])
                x = ldlt_solve(S, rhs)
                ok, why = x is not None, None if x is not None else "S"
            if ok:
                Pn = Pose.copy()
                for k, nk, o in free:
                    x6 = np.concatenate([x[o:o + 3], x[o + 3:o + 6] if nk == 6 else np.zeros(3)])
                    Rn, tn = candidate(Pose[k, :, :3], Pose[k, :, 3], x6)
                    Pn[k, :, :3] = Rn
                    if nk == 6:
                        Pn[k, :, 3] = tn
                s = [gp[c].copy() for c in range(3)]
                for k, nk, o in free:
                    sk = W.seen(k)
                    for a in range(nk):
                        for c in range(3):
                            s[c] = np.where(sk, s[c] + Wc[k][a][c] * x[o + a], s[c])
                dX = [-((Vi[0] * s[0] + Vi[1] * s[1]) + Vi[2] * s[2]), -((Vi[1] * s[0] + Vi[3] * s[1]) + Vi[4] * s[2]), -((Vi[2] * s[0] + Vi[4] * s[1]) + Vi[5] * s[2])]
                Xn = np.where(W.member[:, None], np.stack([X[:, c] + dX[c] for c in range(3)], axis=1), 0.0)
                cn = cost_of(W, Pn, Xn)
                ok, why = bool(cn < cost), None if cn < cost else "cost"
            res["rejections"].append(why)
            if ok:
                converged = bool(cost - cn <= ftol * cost)
                Pose, X, cost, lam = Pn, Xn, cn, lam / np.float64(10.0)
                res["accepted"] += 1
                if converged:
                    break
            else:
                lam = lam * np.float64(10.0)
        fin = bool(np.isfinite(Pose).all() and np.isfinite(X[W.member]).all() and np.isfinite(cost))
        flags = (CONVERGED if converged else 0) | (COST if np.float64(0.5) * cost < np.float64(P["cost_threshold"]) else 0) | (FINITE if fin else 0)
    frames = []
    for k in range(nf):
        Q, T = output_pose(Pose[k, :, :3], Pose[k, :, 3])
        frames.append(dict(R=Pose[k, :, :3].copy(), t=Pose[k, :, 3].copy(), Q=Q, T=T))
    res.update(ok=bool(fin and flags & (CONVERGED | COST)), flags=flags, n_camera=nc, n_members=int(W.member.sum()), n_residuals=int(W.nobs[W.member].sum()),
               cost0=cost0, cost1=cost, lam=lam, frames=frames, state=W.member.astype(np.uint8), positions=X)
    return res


def construct(win, l, rel_R, rel_T, sfm_params=None, **params):
    """chain then BA -> (the chain's result, the BA's result)"""
    ch = global_sfm(win, l, rel_R, rel_T, **(sfm_params or {}))
    R = np.array([f["R"] for f in ch["frames"]])
    t = np.array([f["t"] for f in ch["frames"]])
    return ch, bundle_adjust(win, l, R, t, ch["state"], ch["positions"], chain_ok=ch["ok"], **params)
