"""numpy restatement of the two optional steps of the image feature tracker, CLAHE and rejectWithF, written from the contract text in include/vilfusion.h
("Image feature tracker", paragraphs CLAHE and rejectWithF).

Every float operation is one numpy elementwise operation on float32 or float64 values, so it is rounded on its own exactly as the text demands; where an array
holds one value per hypothesis, per point or per pixel, the operation is the same scalar operation done for each of them (no reductions over floats, no BLAS,
no linalg). No code is shared with csrc. track_reference.py is imported as it is; FeatureTracker below inserts the two steps at the reference's places."""
import numpy as np
import track_reference as tr

f32 = np.float32
JACOBI_SWEEPS = 10
MAX_HYPOTHESES = 2048
MAX_TILES = 1024
_M32 = np.uint64(0xffffffff)


# ---- CLAHE ---------------------------------------------------------------------------------------------------------------
def clahe_geometry(w, h, tx, ty):
    """(W', H', tw, th) of the padded image and its tiles"""
    if w % tx == 0 and h % ty == 0:
        wp, hp = w, h
    else:
        wp, hp = w + (tx - w % tx), h + (ty - h % ty)          # a whole extra tx or ty in a direction that does divide
    return wp, hp, wp // tx, hp // ty


def clahe_limit(clip, area):
    if not clip > 0:
        return 0
    return max(1, int((np.float64(clip) * np.float64(area)) / np.float64(256.0)))


def clahe_luts(img, clip, tx, ty):
    """uint8 [ty][tx][256]"""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape
    wp, hp, tw, th = clahe_geometry(w, h, tx, ty)
    area = tw * th
    limit = clahe_limit(clip, area)
    scale = f32(255.0) / f32(area)
    pad = img[tr.reflect(np.arange(hp), h)][:, tr.reflect(np.arange(wp), w)]
    luts = np.zeros((ty, tx, 256), dtype=np.uint8)
    for j in range(ty):
        for i in range(tx):
            hist = np.bincount(pad[j * th:(j + 1) * th, i * tw:(i + 1) * tw].ravel(), minlength=256).astype(np.int64)
            if limit > 0:
                excess = int(np.maximum(hist - limit, 0).sum())
                hist = np.minimum(hist, limit)
                batch = excess // 256
                residual = excess - 256 * batch
                hist = hist + batch
                if residual > 0:
                    step = max(256 // residual, 1)
                    k = 0
                    while k < 256 and residual > 0:
                        hist[k] += 1
                        k += step
                        residual -= 1
            cum = np.cumsum(hist)
            v = np.rint(cum.astype(np.float32) * scale)
            luts[j, i] = np.clip(v, 0, 255).astype(np.uint8)
    return luts


def clahe(img, clip=3.0, tx=8, ty=8):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape
    _, _, tw, th = clahe_geometry(w, h, tx, ty)
    luts = clahe_luts(img, clip, tx, ty)

    def axis(n, t, nt):
        f = np.arange(n, dtype=np.float32) * (f32(1.0) / f32(t)) - f32(0.5)          # float32 multiply, then float32 subtract
        i1 = np.floor(f)
        a = (f - i1).astype(np.float32)
        i1 = i1.astype(np.int64)
        return np.clip(i1, 0, nt - 1), np.clip(i1 + 1, 0, nt - 1), a

    x1, x2, xa = axis(w, tw, tx)
    y1, y2, ya = axis(h, th, ty)
    one = f32(1.0)
    X1, X2, XA = x1[None, :], x2[None, :], xa[None, :]
    Y1, Y2, YA = y1[:, None], y2[:, None], ya[:, None]
    v = img.astype(np.int64)
    l11, l12 = luts[Y1, X1, v].astype(np.float32), luts[Y1, X2, v].astype(np.float32)
    l21, l22 = luts[Y2, X1, v].astype(np.float32), luts[Y2, X2, v].astype(np.float32)
    top = l11 * (one - XA) + l12 * XA
    bot = l21 * (one - XA) + l22 * XA
    res = top * (one - YA) + bot * YA
    assert res.dtype == np.float32
    return np.clip(np.rint(res), 0, 255).astype(np.uint8)


# ---- rejectWithF -----------------------------------------------------------------------------------------------------------
def mix32(x):
    """the 32-bit mixing function of the text; x: uint64 array holding values < 2^32"""
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & _M32
    return x ^ (x >> np.uint64(16))


def draw(seed, k, d):
    k = np.asarray(k, dtype=np.uint64)
    a = mix32(np.asarray((int(seed) + 0x9e3779b9) & 0xffffffff, dtype=np.uint64))
    return mix32((mix32((a + k) & _M32) + np.uint64(d)) & _M32)


def samples(n, K, seed):
    """int64 [K][8]: the eight distinct indices of every hypothesis"""
    assert n >= 8
    k = np.arange(K, dtype=np.uint64)
    S = np.zeros((K, 8), dtype=np.int64)
    for j in range(8):
        idx = ((draw(seed, k, j) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)
        for _ in range(j):                                   # a duplicate steps to the next index; at most j steps are ever needed
            dup = (idx[:, None] == S[:, :j]).any(axis=1)
            idx = np.where(dup, (idx + 1) % n, idx)
        S[:, j] = idx
    return S


def lift(pts, cam, w, h, focal):
    """float32 [n][2]: liftProjective in fp64 (the undistortion text), then FOCAL_LENGTH x + W / 2, rounded to float32"""
    fx, fy, cx, cy, k1, k2, p1, p2 = (np.float64(v) for v in cam)
    pts = np.asarray(pts, dtype=np.float32).reshape(-1, 2)
    u, v = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    mx, my = (1.0 / fx) * u + (-cx / fx), (1.0 / fy) * v + (-cy / fy)
    ux, uy = mx, my
    if k1 != 0 or k2 != 0 or p1 != 0 or p2 != 0:
        for _ in range(8):
            x2, y2, xy = ux * ux, uy * uy, ux * uy
            rho2 = x2 + y2
            rad = k1 * rho2 + (k2 * rho2) * rho2
            dx = (ux * rad + (2.0 * p1) * xy) + p2 * (rho2 + 2.0 * x2)
            dy = (uy * rad + (2.0 * p2) * xy) + p1 * (rho2 + 2.0 * y2)
            ux, uy = mx - dx, my - dy
    fl = np.float64(focal)
    return np.stack([fl * ux + np.float64(w) / 2.0, fl * uy + np.float64(h) / 2.0], axis=1).astype(np.float32)


def jacobi(A, n):
    """cyclic Jacobi of the symmetric matrices A [K][n][n] (changed in place) -> V [K][n][n], the eigenvectors in the columns"""
    K = A.shape[0]
    V = np.zeros((K, n, n))
    for i in range(n):
        V[:, i, i] = 1.0
    for _ in range(JACOBI_SWEEPS):
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = A[:, p, q].copy()
                skip = apq == 0.0
                theta = (A[:, q, q] - A[:, p, p]) / (2.0 * apq)
                t = np.where(theta < 0.0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                for r in range(n):
                    if r != p and r != q:
                        arp, arq = A[:, r, p].copy(), A[:, r, q].copy()
                        np_ = np.where(skip, arp, c * arp - s * arq)
                        nq_ = np.where(skip, arq, s * arp + c * arq)
                        A[:, r, p] = A[:, p, r] = np_
                        A[:, r, q] = A[:, q, r] = nq_
                A[:, p, p] = np.where(skip, A[:, p, p], A[:, p, p] - t * apq)
                A[:, q, q] = np.where(skip, A[:, q, q], A[:, q, q] + t * apq)
                A[:, p, q] = A[:, q, p] = np.where(skip, apq, 0.0)          # a skipped pair keeps its zero, sign and all
                for r in range(n):
                    vrp, vrq = V[:, r, p].copy(), V[:, r, q].copy()
                    V[:, r, p] = np.where(skip, vrp, c * vrp - s * vrq)
                    V[:, r, q] = np.where(skip, vrq, s * vrp + c * vrq)
    return V


def smallest(A, V, n):
    """the column of V under the smallest diagonal entry of A, ties (and entries that are not numbers) to the lower index"""
    K = A.shape[0]
    best, at = A[:, 0, 0].copy(), np.zeros(K, dtype=np.int64)
    for i in range(1, n):
        less = A[:, i, i] < best
        best = np.where(less, A[:, i, i], best)
        at = np.where(less, i, at)
    return V[np.arange(K), :, at]


def normalise(P):
    """Hartley: P [K][8][2] -> (normalised points, cx, cy, s)"""
    K = P.shape[0]
    cx, cy = np.zeros(K), np.zeros(K)
    for j in range(8):
        cx = cx + P[:, j, 0]
        cy = cy + P[:, j, 1]
    cx, cy = cx / 8.0, cy / 8.0
    md = np.zeros(K)
    for j in range(8):
        dx, dy = P[:, j, 0] - cx, P[:, j, 1] - cy
        md = md + np.sqrt(dx * dx + dy * dy)
    md = md / 8.0
    s = np.sqrt(np.float64(2.0)) / md
    N = np.zeros_like(P)
    N[:, :, 0] = (P[:, :, 0] - cx[:, None]) * s[:, None]
    N[:, :, 1] = (P[:, :, 1] - cy[:, None]) * s[:, None]
    return N, cx, cy, s


def hypotheses(ua, ub, K, seed):
    """F [K][9] (row-major, x'^T F x = 0 with x from ua and x' from ub) and valid [K]"""
    n = len(ua)
    S = samples(n, K, seed)
    with np.errstate(all="ignore"):
        A1, cx1, cy1, s1 = normalise(ua[S].astype(np.float64))
        A2, cx2, cy2, s2 = normalise(ub[S].astype(np.float64))
        x, y, xp, yp = A1[:, :, 0], A1[:, :, 1], A2[:, :, 0], A2[:, :, 1]
        one = np.ones_like(x)
        R = np.stack([xp * x, xp * y, xp, yp * x, yp * y, yp, x, y, one], axis=2)          # [K][8][9]
        M = np.zeros((K, 9, 9))
        for p in range(9):
            for q in range(p, 9):
                acc = np.zeros(K)
                for j in range(8):
                    acc = acc + R[:, j, p] * R[:, j, q]
                M[:, p, q] = M[:, q, p] = acc
        V = jacobi(M, 9)
        Fh = smallest(M, V, 9).reshape(K, 3, 3).copy()
        G = np.zeros((K, 3, 3))
        for p in range(3):
            for q in range(p, 3):
                acc = np.zeros(K)
                for r in range(3):
                    acc = acc + Fh[:, r, p] * Fh[:, r, q]
                G[:, p, q] = G[:, q, p] = acc
        V3 = jacobi(G, 3)
        v3 = smallest(G, V3, 3)                               # [K][3]
        for r in range(3):
            wr = (Fh[:, r, 0] * v3[:, 0] + Fh[:, r, 1] * v3[:, 1]) + Fh[:, r, 2] * v3[:, 2]
            for c in range(3):
                Fh[:, r, c] = Fh[:, r, c] - wr * v3[:, c]
        # F = T'^T Fh T, T = [[s, 0, -s cx], [0, s, -s cy], [0, 0, 1]]
        t1x, t1y, t2x, t2y = s1 * cx1, s1 * cy1, s2 * cx2, s2 * cy2
        B = np.zeros((K, 3, 3))
        for r in range(3):
            B[:, r, 0] = Fh[:, r, 0] * s1
            B[:, r, 1] = Fh[:, r, 1] * s1
            B[:, r, 2] = (Fh[:, r, 2] - Fh[:, r, 0] * t1x) - Fh[:, r, 1] * t1y
        F = np.zeros((K, 3, 3))
        for c in range(3):
            F[:, 0, c] = s2 * B[:, 0, c]
            F[:, 1, c] = s2 * B[:, 1, c]
            F[:, 2, c] = (B[:, 2, c] - t2x * B[:, 0, c]) - t2y * B[:, 1, c]
        F = F.reshape(K, 9)
        valid = np.isfinite(s1) & np.isfinite(s2) & np.isfinite(F).all(axis=1)
    return F, valid


def inliers(F, ua, ub, thr):
    """bool [K][n] for F [K][9]"""
    x, y = ua[:, 0].astype(np.float64)[None, :], ua[:, 1].astype(np.float64)[None, :]
    xp, yp = ub[:, 0].astype(np.float64)[None, :], ub[:, 1].astype(np.float64)[None, :]
    f = [F[:, i][:, None] for i in range(9)]
    with np.errstate(all="ignore"):
        lp0, lp1, lp2 = (f[0] * x + f[1] * y) + f[2], (f[3] * x + f[4] * y) + f[5], (f[6] * x + f[7] * y) + f[8]
        l0, l1 = (f[0] * xp + f[3] * yp) + f[6], (f[1] * xp + f[4] * yp) + f[7]
        d = (xp * lp0 + yp * lp1) + lp2
        d2 = d * d
        e1, e2 = d2 / (lp0 * lp0 + lp1 * lp1), d2 / (l0 * l0 + l1 * l1)
        t2 = np.float64(thr) * np.float64(thr)
        return (e1 <= t2) & (e2 <= t2)                       # err = max(e1, e2) <= thr^2; a NaN compares false


def reject_f(cur_pts, forw_pts, cam, w, h, focal=460.0, thr=1.0, K=512, seed=0):
    """-> (status uint8 [n], best, n_inliers, F float64 [9]); best = -1 (F = 0, every status 1) when n < 8 or no hypothesis is valid"""
    cur_pts = np.asarray(cur_pts, dtype=np.float32).reshape(-1, 2)
    forw_pts = np.asarray(forw_pts, dtype=np.float32).reshape(-1, 2)
    n = len(cur_pts)
    assert len(forw_pts) == n and 1 <= K <= MAX_HYPOTHESES
    none = (np.ones(n, dtype=np.uint8), -1, n, np.zeros(9))
    if n < 8:
        return none
    ua, ub = lift(cur_pts, cam, w, h, focal), lift(forw_pts, cam, w, h, focal)
    F, valid = hypotheses(ua, ub, K, seed)
    inl = inliers(F, ua, ub, thr)
    score = np.where(valid, inl.sum(axis=1), -1)
    best = int(np.argmax(score))                             # the first maximum: ties to the lower k
    if score[best] < 0:
        return none
    return inl[best].astype(np.uint8), best, int(score[best]), F[best].copy()


class FeatureTracker(tr.FeatureTracker):
    """track_reference.FeatureTracker with CLAHE in front of everything and rejectWithF between the inBorder drop and setMask (feature_tracker.cpp:125-131, :171)"""

    def __init__(self, width, height, camera, max_cnt=200, min_dist=20, equalize=False, f_threshold=None, focal_length=460.0, clahe=(3.0, 8, 8),
                 n_hypotheses=512, seed=0):
        self.equalize, self.f_threshold, self.focal_length = bool(equalize), f_threshold, float(focal_length)
        self.clahe_params, self.n_hypotheses, self.seed = (float(clahe[0]), int(clahe[1]), int(clahe[2])), int(n_hypotheses), int(seed)
        self.rejected = []                                   # per frame: how many points rejectWithF dropped
        super().__init__(width, height, camera, max_cnt=max_cnt, min_dist=min_dist)

    def clahe(self, img):
        return clahe(img, *self.clahe_params)

    def reject_f(self, cur_pts, forw_pts):
        return reject_f(cur_pts, forw_pts, self.camera, self.width, self.height, self.focal_length, 1.0 if self.f_threshold is None else self.f_threshold,
                        self.n_hypotheses, self.seed)

    def readImage(self, img, stamp):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        assert img.shape == (self.height, self.width)
        if self.equalize:
            img = self.clahe(img)
        pts, ids, cnt = self.cur_pts, self.ids, self.track_cnt
        if len(pts):
            fw, st = tr.lk(self.cur_img, img, pts)
            keep = (st != 0) & tr.in_border(fw, self.width, self.height)
            cur, pts, ids, cnt = pts[keep], fw[keep], ids[keep], cnt[keep]
            if self.f_threshold is not None:
                ok = self.reject_f(cur, pts)[0] != 0
                self.rejected.append(int((~ok).sum()))
                pts, ids, cnt = pts[ok], ids[ok], cnt[ok]
        cnt = cnt + 1
        kept = tr.set_mask(pts, cnt, self.min_dist)
        pts, ids, cnt = pts[kept].reshape(-1, 2), ids[kept], cnt[kept]
        new = tr.detect(img, pts, self.max_cnt - len(pts), self.min_dist)
        pts = np.concatenate([pts, new]).astype(np.float32)
        ids = np.concatenate([ids, np.full(len(new), -1)]).astype(np.int32)
        cnt = np.concatenate([cnt, np.ones(len(new))]).astype(np.int32)
        for i in range(len(ids)):
            if ids[i] == -1:
                ids[i] = self.n_id
                self.n_id += 1
        un = tr.undistort(pts, self.camera)
        vel = np.zeros((len(pts), 2), dtype=np.float32)
        if self.cur_time is not None:
            dt = np.float64(stamp) - np.float64(self.cur_time)
            for i, k in enumerate(ids):
                if int(k) in self.prev_un:
                    with np.errstate(all="ignore"):
                        vel[i] = ((un[i].astype(np.float64) - self.prev_un[int(k)].astype(np.float64)) / dt).astype(np.float32)
        self.prev_un = {int(k): un[i].copy() for i, k in enumerate(ids)}
        self.cur_img, self.cur_time = img, stamp
        self.ids, self.track_cnt, self.cur_pts, self.cur_un_pts, self.pts_velocity = ids, cnt, pts, un, vel
        return len(ids)
