"""numpy restatement of the second stage of the visual start-up, GlobalSFM's frame chain, written from the contract text in include/vilfusion.h ("Visual start-up:
GlobalSFM frame chain").

Every float operation is one numpy elementwise operation on float64 values, so it is rounded on its own; sums are written out in the text's order. The Jacobi is
frontend_reference's, imported and not copied; the first stage comes from startup_reference. No code is shared with csrc. Besides the rows, flags and structure
global_sfm returns a trace: per step of the chain the features it triangulated or the members of its PnP."""
import numpy as np
from frontend_reference import jacobi
from startup_reference import relative_pose  # noqa: F401  (the first stage, for the callers that run both)

FIXED, PNP, FEW, FAIL_COUNT, FAIL_FINITE, POSE = 1, 2, 4, 8, 16, 32
DEFAULTS = dict(min_pnp_count=10, warn_pnp_count=15, pnp_iterations=10, lambda0=1e-3)
MAX_FRAMES, MAX_FEATURES = 11, 1000
NT = 256
UPPER = [(a, b) for a in range(6) for b in range(a, 6)]


def table(win):
    start, first = np.asarray(win["start_frame"], dtype=np.int64), np.asarray(win["first_obs"], dtype=np.int64)
    return start, first, first[1:] - first[:-1], np.asarray(win["pts"], dtype=np.float64).reshape(-1, 2)


def triangulate_points(P0, P1, p0, p1):
    """P0, P1 [K][3][4] (or [3][4] for all), p0, p1 [K][2] -> (positions [K][3], finite [K]): the paragraph triangulatePoint, K features at once"""
    K = len(p0)
    P0, P1 = np.broadcast_to(P0, (K, 3, 4)), np.broadcast_to(P1, (K, 3, 4))
    with np.errstate(all="ignore"):
        A = np.zeros((K, 4, 4))
        for c in range(4):
            A[:, 0, c] = p0[:, 0] * P0[:, 2, c] - P0[:, 0, c]
            A[:, 1, c] = p0[:, 1] * P0[:, 2, c] - P0[:, 1, c]
            A[:, 2, c] = p1[:, 0] * P1[:, 2, c] - P1[:, 0, c]
            A[:, 3, c] = p1[:, 1] * P1[:, 2, c] - P1[:, 1, c]
        G = np.zeros((K, 4, 4))
        for p in range(4):
            for q in range(p, 4):
                acc = np.zeros(K)
                for r in range(4):
                    acc = acc + A[:, r, p] * A[:, r, q]
                G[:, p, q] = G[:, q, p] = acc
        V = jacobi(G, 4)
        best, at = G[:, 0, 0].copy(), np.zeros(K, dtype=np.int64)
        for i in range(1, 4):
            less = G[:, i, i] < best
            best, at = np.where(less, G[:, i, i], best), np.where(less, i, at)
        v = V[np.arange(K), :, at]
        X = np.stack([v[:, 0] / v[:, 3], v[:, 1] / v[:, 3], v[:, 2] / v[:, 3]], axis=1)
    return X, np.isfinite(X).all(axis=1)


def design_matrix(P0, P1, p0, p1):
    """the 4 x 4 matrix A of one point, for the tests that solve it independently"""
    return np.array([p0[0] * P0[2] - P0[0], p0[1] * P0[2] - P0[1], p1[0] * P1[2] - P1[0], p1[1] * P1[2] - P1[1]])


def total(terms):
    """terms [m][k] -> [k]: 256 strided partial sums, the butterfly within each 64, then ((0 + 1) + 2) + 3"""
    m, k = terms.shape
    s = np.zeros((NT, k))
    for base in range(0, m, NT):
        chunk = terms[base:base + NT]
        s[:len(chunk)] = s[:len(chunk)] + chunk
    s = s.reshape(4, 64, k)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, np.arange(64) ^ o]
    return ((s[0, 0] + s[1, 0]) + s[2, 0]) + s[3, 0]


def residuals(R, t, X, u):
    q = [(R[r, 0] * X[:, 0] + R[r, 1] * X[:, 1]) + R[r, 2] * X[:, 2] for r in range(3)]
    p = [q[r] + t[r] for r in range(3)]
    iz = 1.0 / p[2]
    xn, yn = p[0] * iz, p[1] * iz
    return q, iz, xn, yn, xn - u[:, 0], yn - u[:, 1]


def cost_of(R, t, X, u):
    _, _, _, _, e0, e1 = residuals(R, t, X, u)
    return total((e0 * e0 + e1 * e1).reshape(-1, 1))[0]


def linearise(R, t, X, u):
    """-> (H [6][6] upper, g [6], cost)"""
    q, iz, xn, yn, e0, e1 = residuals(R, t, X, u)
    c0, c1 = xn * iz, yn * iz
    zero = np.zeros(len(X))
    J0 = [-(c0 * q[1]), iz * q[2] + c0 * q[0], -(iz * q[1]), iz, zero, -c0]
    J1 = [-(iz * q[2] + c1 * q[1]), c1 * q[0], iz * q[0], zero, iz, -c1]
    terms = [J0[a] * J0[b] + J1[a] * J1[b] for a, b in UPPER] + [J0[a] * e0 + J1[a] * e1 for a in range(6)] + [e0 * e0 + e1 * e1]
    s = total(np.stack(terms, axis=1))
    H = np.zeros((6, 6))
    for k, (a, b) in enumerate(UPPER):
        H[a, b] = s[k]
    return H, s[21:27].copy(), s[27]


def ldlt_solve(Hd, b):
    """-> x or None if a pivot is not > 0; Hd is read in its upper triangle"""
    L, U, d = np.zeros((6, 6)), np.zeros((6, 6)), np.zeros(6)
    for j in range(6):
        s = Hd[j, j]
        for k in range(j):
            s = s - U[j, k] * L[j, k]
        d[j] = s
        if not d[j] > 0:
            return None
        for i in range(j + 1, 6):
            s = Hd[j, i]
            for k in range(j):
                s = s - U[i, k] * L[j, k]
            U[i, j] = s
            L[i, j] = s / d[j]
    y, z, x = np.zeros(6), np.zeros(6), np.zeros(6)
    for i in range(6):
        s = b[i]
        for k in range(i):
            s = s - L[i, k] * y[k]
        y[i] = s
    for i in range(6):
        z[i] = y[i] / d[i]
    for i in range(5, -1, -1):
        s = z[i]
        for k in range(i + 1, 6):
            s = s - L[k, i] * x[k]
        x[i] = s
    return x


def candidate(R, t, x6):
    a = [np.float64(0.5) * x6[i] for i in range(3)]
    n = np.sqrt(((1.0 + a[0] * a[0]) + a[1] * a[1]) + a[2] * a[2])
    s, x, y, z = 1.0 / n, a[0] / n, a[1] / n, a[2] / n
    Q = np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - s * z), 2.0 * (x * z + s * y)],
                  [2.0 * (x * y + s * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - s * x)],
                  [2.0 * (x * z - s * y), 2.0 * (y * z + s * x), 1.0 - 2.0 * (x * x + y * y)]])
    Rn = np.array([[(Q[r, 0] * R[0, c] + Q[r, 1] * R[1, c]) + Q[r, 2] * R[2, c] for c in range(3)] for r in range(3)])
    return Rn, np.array([t[r] + x6[3 + r] for r in range(3)])


def output_pose(R, t):
    Q = R.T.copy()
    return Q, np.array([-((Q[r, 0] * t[0] + Q[r, 1] * t[1]) + Q[r, 2] * t[2]) for r in range(3)])


def empty_row():
    return dict(count=0, flags=0, accepted=0, cost0=np.float64(0.0), cost1=np.float64(0.0), R=np.zeros((3, 3)), t=np.zeros(3), Q=np.zeros((3, 3)), T=np.zeros(3))


def pose_row(row, R, t):
    Q, T = output_pose(R, t)
    row.update(R=R.copy(), t=t.copy(), Q=Q, T=T)
    row["flags"] |= POSE
    return row


def pnp(pts3, pts2, R0, t0, min_count, **params):
    """the paragraph solveFrameByPnP on the members given in their order -> the frame's row (and 'lambdas', the damping of every iteration)"""
    P = dict(DEFAULTS, **params)
    X = np.asarray(pts3, dtype=np.float64).reshape(-1, 3).astype(np.float32).astype(np.float64)
    u = np.asarray(pts2, dtype=np.float64).reshape(-1, 2).astype(np.float32).astype(np.float64)
    m = len(X)
    row = empty_row()
    row.update(count=m, flags=PNP | (FEW if m < P["warn_pnp_count"] else 0), lambdas=[])
    if m < min_count:
        row["flags"] |= FAIL_COUNT
        return row
    R, t, lam = np.asarray(R0, dtype=np.float64).reshape(3, 3).copy(), np.asarray(t0, dtype=np.float64).copy(), np.float64(P["lambda0"])
    cost = np.float64(0.0)
    with np.errstate(all="ignore"):
        for it in range(int(P["pnp_iterations"])):
            H, g, cost = linearise(R, t, X, u)
            if it == 0:
                row["cost0"] = cost
            row["lambdas"].append(lam)
            Hd = H.copy()
            for a in range(6):
                Hd[a, a] = H[a, a] + lam * H[a, a]
            x6 = ldlt_solve(Hd, -g)
            ok = False
            if x6 is not None:
                Rn, tn = candidate(R, t, x6)
                cn = cost_of(Rn, tn, X, u)
                ok = bool(cn < cost)
            if ok:
                R, t, cost, lam = Rn, tn, cn, lam / np.float64(10.0)
                row["accepted"] += 1
            else:
                lam = lam * np.float64(10.0)
    row["cost1"] = cost
    if not (np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(cost)):
        row["flags"] |= FAIL_FINITE
        return row
    return pose_row(row, R, t)


def global_sfm(win, l, rel_R, rel_T, **params):
    """the chain -> dict(ok, fail_frame, n_triangulated, l, frames [n_frames] rows, state [n] uint8, positions [n][3], trace)
    trace: a list of ("tri", a, b, [features]) / ("pnp", i, [members]) / ("rest", [features]) in the order of the chain"""
    P = dict(DEFAULTS, **params)
    start, first, nobs, pts = table(win)
    nf, n = int(win["n_frames"]), len(start)
    newest = nf - 1
    frames = [empty_row() for _ in range(nf)]
    state, pos, trace = np.zeros(n, dtype=np.uint8), np.zeros((n, 3)), []
    res = dict(ok=False, fail_frame=-1, n_triangulated=0, l=int(l), frames=frames, state=state, positions=pos, trace=trace)
    if l < 0:
        return res
    assert l <= nf - 2
    R, T = np.asarray(rel_R, dtype=np.float64).reshape(3, 3), np.asarray(rel_T, dtype=np.float64)
    Pose = np.zeros((nf, 3, 4))
    Pose[l, :, :3] = np.eye(3)
    Pose[newest, :, :3] = R.T
    Pose[newest, :, 3] = [-((R[0, r] * T[0] + R[1, r] * T[1]) + R[2, r] * T[2]) for r in range(3)]
    for k in (l, newest):
        frames[k]["flags"] = FIXED
        pose_row(frames[k], Pose[k, :, :3], Pose[k, :, 3])

    def seen(k):
        return (start <= k) & (k < start + nobs)

    def point(f, k):
        return pts[first[f] + k - start[f]]

    def two_frames(a, b):
        f = np.nonzero((state == 0) & seen(a) & seen(b))[0]
        if len(f):
            X, fin = triangulate_points(Pose[a], Pose[b], point(f, a), point(f, b))
            state[f[fin]], pos[f[fin]] = 1, X[fin]
            f = f[fin]
        trace.append(("tri", a, b, [int(v) for v in f]))

    def frame_pnp(i, guess):
        f = np.nonzero((state == 1) & seen(i))[0]
        trace.append(("pnp", i, [int(v) for v in f]))
        row = pnp(pos[f], point(f, i), Pose[guess, :, :3], Pose[guess, :, 3], P["min_pnp_count"], **params)
        frames[i] = row
        if not row["flags"] & POSE:
            res["fail_frame"] = i
            return False
        Pose[i, :, :3], Pose[i, :, 3] = row["R"], row["t"]
        return True

    def chain():
        two_frames(l, newest)
        for i in range(l + 1, newest):
            if not frame_pnp(i, i - 1):
                return False
            two_frames(i, newest)
        for i in range(l + 1, newest):
            two_frames(l, i)
        for i in range(l - 1, -1, -1):
            if not frame_pnp(i, i + 1):
                return False
            two_frames(i, l)
        f = np.nonzero((state == 0) & (nobs >= 2))[0]
        if len(f):
            a, b = start[f], start[f] + nobs[f] - 1
            X, fin = triangulate_points(Pose[a], Pose[b], pts[first[f]], pts[first[f] + nobs[f] - 1])
            state[f[fin]], pos[f[fin]] = 1, X[fin]
            f = f[fin]
        trace.append(("rest", [int(v) for v in f]))
        return True

    res["ok"] = chain()
    res["n_triangulated"] = int(state.sum())
    return res
