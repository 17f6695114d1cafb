"""numpy restatement of the first stage of the visual start-up, relativePose, written from the contract text in include/vilfusion.h ("Visual start-up: relativePose").

Every float operation is one numpy elementwise operation on float64 values (the points are rounded to float32 first, as the text says), so it is rounded on its
own; sums are written out in the text's order. The search is frontend_reference's (samples inside hypotheses, hypotheses, inliers), imported and not copied, and
so are its Jacobi and its tie rule. No code is shared with csrc."""
import numpy as np
from frontend_reference import hypotheses, inliers, jacobi, samples, MAX_HYPOTHESES  # noqa: F401  (samples: the draw that hypotheses uses, re-exported for the tests)

COUNT, PARALLAX, SOLVE_COUNT, HYPOTHESIS, FINITE, INLIERS, PASS = 1, 2, 4, 8, 16, 32, 63
SEARCHED = COUNT | PARALLAX | SOLVE_COUNT
DEFAULTS = dict(n_hypotheses=512, seed=0, min_count=20, min_solve_count=15, min_inliers=12, ransac_threshold=0.3 / 460.0, focal_length=460.0, min_parallax=30.0,
                distance_threshold=50.0)


def correspondences(win, i):
    """(feature indices int64 [m], a float32 [m][2], b float32 [m][2]) of the pair (i, newest), in feature order"""
    start, first = np.asarray(win["start_frame"], dtype=np.int64), np.asarray(win["first_obs"], dtype=np.int64)
    pts = np.asarray(win["pts"], dtype=np.float64).reshape(-1, 2)
    newest = int(win["n_frames"]) - 1
    nobs = first[1:] - first[:-1]
    member = (start <= i) & (start + nobs - 1 >= newest) if i < newest else np.zeros(len(start), dtype=bool)
    f = np.nonzero(member)[0]
    a = pts[first[f] + i - start[f]].astype(np.float32).reshape(-1, 2)
    b = pts[first[f] + newest - start[f]].astype(np.float32).reshape(-1, 2)
    return f, a, b


def parallax(a, b, focal):
    """the number the parallax gate compares: 64 strided partial sums, the fixed butterfly, the mean, times the focal length"""
    m = len(a)
    if m == 0:
        return np.float64(0.0)
    dx, dy = a[:, 0].astype(np.float64) - b[:, 0].astype(np.float64), a[:, 1].astype(np.float64) - b[:, 1].astype(np.float64)
    d = np.sqrt(dx * dx + dy * dy)
    p = np.zeros(64)
    for j in range(m):                       # lane j % 64 meets its terms in ascending order
        p[j % 64] = p[j % 64] + d[j]
    for o in (32, 16, 8, 4, 2, 1):
        p = p + p[np.arange(64) ^ o]
    return (p[0] / np.float64(m)) * np.float64(focal)


def cross(p, q):
    return np.array([p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]])


def decompose(E):
    """E [9] -> (R1 [3][3], R2 [3][3], t [3]), the recoverPose paragraph"""
    E = np.asarray(E, dtype=np.float64).reshape(3, 3)
    with np.errstate(all="ignore"):
        G = np.zeros((1, 3, 3))
        for p in range(3):
            for q in range(p, 3):
                acc = np.float64(0.0)
                for r in range(3):
                    acc = acc + E[r, p] * E[r, q]
                G[0, p, q] = G[0, q, p] = acc
        V = jacobi(G, 3)[0]
        g = [G[0, 0, 0], G[0, 1, 1], G[0, 2, 2]]
        i3 = 0
        for i in (1, 2):
            if g[i] < g[i3]:
                i3 = i
        r0, r1 = [i for i in range(3) if i != i3]
        i1, i2 = (r1, r0) if g[r1] > g[r0] else (r0, r1)
        v1, v2 = V[:, i1].copy(), V[:, i2].copy()
        v3 = cross(v1, v2)
        us = []
        for v in (v1, v2):
            w = np.array([(E[r, 0] * v[0] + E[r, 1] * v[1]) + E[r, 2] * v[2] for r in range(3)])
            us.append(w / np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]))
        u1, u2 = us
        u3 = cross(u1, u2)
        R1, R2 = np.zeros((3, 3)), np.zeros((3, 3))
        for r in range(3):
            for c in range(3):
                p21, p12, p33 = u2[r] * v1[c], u1[r] * v2[c], u3[r] * v3[c]
                R1[r, c] = (p21 - p12) + p33
                R2[r, c] = (p12 - p21) + p33
    return R1, R2, u3


def depths(R, t, a, b):
    """(z1 [m], z2 [m]) of the cheirality paragraph"""
    ax, ay, bx, by = (v.astype(np.float64) for v in (a[:, 0], a[:, 1], b[:, 0], b[:, 1]))
    with np.errstate(all="ignore"):
        r0, r1, r2 = (R[0, 0] * ax + R[0, 1] * ay) + R[0, 2], (R[1, 0] * ax + R[1, 1] * ay) + R[1, 2], (R[2, 0] * ax + R[2, 1] * ay) + R[2, 2]
        rr = (r0 * r0 + r1 * r1) + r2 * r2
        xx = (bx * bx + by * by) + 1.0
        rx = (r0 * bx + r1 * by) + r2
        rt = (r0 * t[0] + r1 * t[1]) + r2 * t[2]
        xt = (bx * t[0] + by * t[1]) + t[2]
        det = rr * xx - rx * rx
        return (rx * xt - xx * rt) / det, (rr * xt - rx * rt) / det


def good(z1, z2, dist):
    with np.errstate(all="ignore"):
        return (z1 > 0.0) & (z1 < dist) & (z2 > 0.0) & (z2 < dist)


def candidates(E):
    R1, R2, t = decompose(E)
    return [(R1, t), (R2, t), (R1, -t), (R2, -t)]


def pair(win, i, **params):
    """the row of the pair (i, newest) with its per-correspondence outputs"""
    P = dict(DEFAULTS, **params)
    K = int(P["n_hypotheses"])
    assert 1 <= K <= MAX_HYPOTHESES
    f, a, b = correspondences(win, i)
    m = len(f)
    par = parallax(a, b, P["focal_length"])
    flags = (COUNT if m > P["min_count"] else 0) | (PARALLAX if par > P["min_parallax"] else 0) | (SOLVE_COUNT if m >= P["min_solve_count"] and m >= 8 else 0)
    row = dict(count=m, flags=flags, best_k=-1, score=0, cheirality=[0, 0, 0, 0], chosen=-1, inlier_cnt=0, parallax=par, F=np.zeros(9), R=np.zeros((3, 3)),
               T=np.zeros(3), feature=f.astype(np.int32), mask=np.zeros(m, dtype=np.uint8), points=np.zeros((m, 3)), a=a, b=b)
    if flags & SEARCHED != SEARCHED:
        return row
    F, valid = hypotheses(a, b, K, (int(P["seed"]) + i) & 0xffffffff)
    inl = inliers(F, a, b, P["ransac_threshold"])
    score = np.where(valid, inl.sum(axis=1), -1)
    k = int(np.argmax(score))                                # the first maximum: ties to the lower k
    if score[k] < 0:
        return row
    E, mask = F[k].copy(), inl[k]
    row.update(flags=flags | HYPOTHESIS, best_k=k, score=int(score[k]), F=E, mask=mask.astype(np.uint8))
    cand = candidates(E)
    if not all(np.isfinite(R).all() and np.isfinite(t).all() for R, t in cand):
        return row
    dist = np.float64(P["distance_threshold"])
    zs = [depths(R, t, a, b) for R, t in cand]
    counts = [int((good(z1, z2, dist) & mask).sum()) for z1, z2 in zs]
    c = counts.index(max(counts))                            # the first maximum, OpenCV's >= chain
    R, t = cand[c]
    z1, z2 = zs[c]
    ok = good(z1, z2, dist) & mask
    pts = np.zeros((m, 3))
    pts[ok, 0], pts[ok, 1], pts[ok, 2] = (z1 * a[:, 0].astype(np.float64))[ok], (z1 * a[:, 1].astype(np.float64))[ok], z1[ok]
    T = np.array([-((R[0, r] * t[0] + R[1, r] * t[1]) + R[2, r] * t[2]) for r in range(3)])
    flags = row["flags"] | FINITE | (INLIERS if counts[c] > P["min_inliers"] else 0)
    row.update(flags=flags, cheirality=counts, chosen=c, inlier_cnt=counts[c], R=R.T.copy(), T=T, mask=(mask.astype(np.uint8) | (ok.astype(np.uint8) << 1)), points=pts)
    return row


def relative_pose(win, **params):
    """dict(ok, l, R, T, inlier_cnt, pairs): l = the lowest i whose pair passes every gate, -1 if none does"""
    pairs = [pair(win, i, **params) for i in range(int(win["n_frames"]) - 1)]
    l = next((i for i, r in enumerate(pairs) if r["flags"] == PASS), -1)
    if l < 0:
        return dict(ok=False, l=-1, R=np.zeros((3, 3)), T=np.zeros(3), inlier_cnt=0, pairs=pairs)
    return dict(ok=True, l=l, R=pairs[l]["R"], T=pairs[l]["T"], inlier_cnt=pairs[l]["inlier_cnt"], pairs=pairs)
