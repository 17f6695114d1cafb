"""numpy restatement of the image feature tracker, written from the contract text in include/vilfusion.h ("Image feature tracker").

int64 / float64 arithmetic (float32 where the text says float32), np.rint, no code shared with csrc. The class has the shape of
vil_fusion_amd.estimator.FeatureTracker, so a test drives both with the same calls and compares bit for bit."""
import numpy as np

WIN = 21
HALF = 10
MAX_ITERS = 30
f32 = np.float32
K5 = np.array([1, 4, 6, 4, 1], dtype=np.int64)


def reflect(i, n):
    """R(i, n): reflect-101, periodic with period 2 (n - 1); arrays or scalars"""
    i = np.asarray(i, dtype=np.int64)
    p = 2 * (n - 1)
    m = np.mod(i, p)
    return np.where(m < n, m, p - m)


def level_sizes(w, h):
    """[(W_L, H_L)] for the levels 0 .. Lmax"""
    out = [(w, h)]
    while len(out) < 4:
        w, h = (w + 1) // 2, (h + 1) // 2
        if not (w > WIN and h > WIN):
            break
        out.append((w, h))
    return out


def pyr_down(img):
    h, w = img.shape
    w2, h2 = (w + 1) // 2, (h + 1) // 2
    I = img.astype(np.int64)
    acc = np.zeros((h2, w2), dtype=np.int64)
    ys, xs = 2 * np.arange(h2), 2 * np.arange(w2)
    for j in range(-2, 3):
        rows = I[reflect(ys + j, h)]
        for i in range(-2, 3):
            acc += K5[i + 2] * K5[j + 2] * rows[:, reflect(xs + i, w)]
    return ((acc + 128) >> 8).astype(np.uint8)


def build_pyramid(img):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    levels = [img]
    for _ in level_sizes(img.shape[1], img.shape[0])[1:]:
        levels.append(pyr_down(levels[-1]))
    return levels


def read(img, x, y):
    """I(R(x), R(y)) as int64"""
    h, w = img.shape
    return img[reflect(y, h), reflect(x, w)].astype(np.int64)


def scharr(img, x, y):
    """(Gx, Gy) at the positions (x, y); 0 outside the image"""
    x, y = np.asarray(x, dtype=np.int64), np.asarray(y, dtype=np.int64)
    h, w = img.shape
    gx = 3 * (read(img, x + 1, y - 1) - read(img, x - 1, y - 1)) + 10 * (read(img, x + 1, y) - read(img, x - 1, y)) + 3 * (read(img, x + 1, y + 1) - read(img, x - 1, y + 1))
    gy = 3 * (read(img, x - 1, y + 1) - read(img, x - 1, y - 1)) + 10 * (read(img, x, y + 1) - read(img, x, y - 1)) + 3 * (read(img, x + 1, y + 1) - read(img, x + 1, y - 1))
    inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
    return np.where(inside, gx, 0), np.where(inside, gy, 0)


def corner(p, w, h):
    """top-left corner of the window around the float32 point p: (ix, iy, (w00, w01, w10, w11)) or None when out of bounds"""
    cx, cy = f32(p[0]) - f32(HALF), f32(p[1]) - f32(HALF)
    fx, fy = np.floor(cx), np.floor(cy)
    if not (np.isfinite(cx) and np.isfinite(cy)):
        return None
    if fx < -WIN or fx >= w or fy < -WIN or fy >= h:
        return None
    a, b = f32(cx - fx), f32(cy - fy)
    one, s = f32(1), f32(16384)
    w00 = int(np.rint(f32(f32(one - a) * f32(one - b)) * s))
    w01 = int(np.rint(f32(a * f32(one - b)) * s))
    w10 = int(np.rint(f32(f32(one - a) * b) * s))
    return int(fx), int(fy), (w00, w01, w10, 16384 - w00 - w01 - w10)


_U, _V = np.meshgrid(np.arange(WIN, dtype=np.int64), np.arange(WIN, dtype=np.int64))


def bilinear_image(img, ix, iy, wt):
    x, y = ix + _U, iy + _V
    s = wt[0] * read(img, x, y) + wt[1] * read(img, x + 1, y) + wt[2] * read(img, x, y + 1) + wt[3] * read(img, x + 1, y + 1)
    return (s + 256) >> 9


def bilinear_gradient(img, ix, iy, wt):
    x, y = ix + _U, iy + _V
    g = [scharr(img, x + dx, y + dy) for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1))]
    sx = sum(wt[k] * g[k][0] for k in range(4))
    sy = sum(wt[k] * g[k][1] for k in range(4))
    return (sx + 8192) >> 14, (sy + 8192) >> 14


def lk_point(pyr_prev, pyr_next, pt):
    """one point through the levels Lmax .. 0 -> ((x, y) float32, status)"""
    lmax = len(pyr_prev) - 1
    status = 1
    q = None
    for L in range(lmax, -1, -1):
        prev, nxt = pyr_prev[L], pyr_next[L]
        h, w = prev.shape
        scale = f32(1.0 / (1 << L))
        pL = (f32(f32(pt[0]) * scale), f32(f32(pt[1]) * scale))
        q = pL if L == lmax else (f32(f32(2) * q[0]), f32(f32(2) * q[1]))
        c = corner(pL, w, h)
        if c is None:
            if L == 0:
                status = 0
            continue
        ix, iy, wt = c
        T = bilinear_image(prev, ix, iy, wt)
        Tx, Ty = bilinear_gradient(prev, ix, iy, wt)
        sc = 2.0 ** -20
        a11, a12, a22 = float(np.sum(Tx * Tx)) * sc, float(np.sum(Tx * Ty)) * sc, float(np.sum(Ty * Ty)) * sc
        D = a11 * a22 - a12 * a12
        d = a11 - a22
        e = (a11 + a22 - np.sqrt(d * d + 4.0 * a12 * a12)) / 882.0
        if e < 1e-4 or D < 1.1920929e-7:
            if L == 0:
                status = 0
            continue
        inv = 1.0 / D
        prev_d = (0.0, 0.0)
        for it in range(MAX_ITERS):
            c = corner(q, w, h)
            if c is None:
                if L == 0:
                    status = 0
                break
            jx, jy, jw = c
            diff = bilinear_image(nxt, jx, jy, jw) - T
            b1, b2 = float(np.sum(diff * Tx)) * sc, float(np.sum(diff * Ty)) * sc
            dx, dy = (a12 * b2 - a22 * b1) * inv, (a12 * b1 - a11 * b2) * inv
            q = (f32(np.float64(q[0]) + dx), f32(np.float64(q[1]) + dy))
            if dx * dx + dy * dy <= 1e-4:
                break
            if it > 0 and abs(dx + prev_d[0]) < 0.01 and abs(dy + prev_d[1]) < 0.01:
                q = (f32(np.float64(q[0]) - dx * 0.5), f32(np.float64(q[1]) - dy * 0.5))
                break
            prev_d = (dx, dy)
    return q, status


def lk(img_prev, img_next, pts):
    pts = np.asarray(pts, dtype=np.float32).reshape(-1, 2)
    pp, pn = build_pyramid(img_prev), build_pyramid(img_next)
    out, st = np.zeros((len(pts), 2), dtype=np.float32), np.zeros(len(pts), dtype=np.uint8)
    for i, p in enumerate(pts):
        q, s = lk_point(pp, pn, p)
        out[i] = q
        st[i] = s
    return out, st


def pixel(pts):
    """(rint x, rint y) as int64 [n][2]"""
    return np.rint(np.asarray(pts, dtype=np.float32).reshape(-1, 2)).astype(np.int64)


def in_border(pts, w, h):
    p = pixel(pts)
    return (p[:, 0] >= 1) & (p[:, 0] <= w - 2) & (p[:, 1] >= 1) & (p[:, 1] <= h - 2)


def eigen_map(img):
    """lambda of every pixel (float64 [H][W])"""
    h, w = img.shape
    ys, xs = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    sx = (read(img, xs + 1, ys - 1) + 2 * read(img, xs + 1, ys) + read(img, xs + 1, ys + 1)) - (read(img, xs - 1, ys - 1) + 2 * read(img, xs - 1, ys) + read(img, xs - 1, ys + 1))
    sy = (read(img, xs - 1, ys + 1) + 2 * read(img, xs, ys + 1) + read(img, xs + 1, ys + 1)) - (read(img, xs - 1, ys - 1) + 2 * read(img, xs, ys - 1) + read(img, xs + 1, ys - 1))
    P, Q, S = np.zeros((h, w), dtype=np.int64), np.zeros((h, w), dtype=np.int64), np.zeros((h, w), dtype=np.int64)
    for j in (-1, 0, 1):
        for i in (-1, 0, 1):
            yy, xx = reflect(ys + j, h), reflect(xs + i, w)
            a, b = sx[yy, xx], sy[yy, xx]
            P += a * a
            Q += a * b
            S += b * b
    Pd, Qd, Sd = P.astype(np.float64), Q.astype(np.float64), S.astype(np.float64)
    d = Pd - Sd
    return (Pd + Sd) - np.sqrt(d * d + 4.0 * Qd * Qd)


def allowed_mask(w, h, kept_pts, min_dist):
    ys, xs = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    ok = np.ones((h, w), dtype=bool)
    for px, py in pixel(kept_pts):
        ok &= (xs - px) ** 2 + (ys - py) ** 2 > min_dist * min_dist
    return ok


def detect(img, kept_pts, n_max, min_dist):
    """new corners, float32 [n][2], in the order they are accepted"""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape
    out = np.zeros((0, 2), dtype=np.float32)
    if n_max <= 0:
        return out
    lam = eigen_map(img)
    ok = allowed_mask(w, h, kept_pts, min_dist)
    if not ok.any():
        return out
    lmax = lam[ok].max()
    cand = ok & (lam > 0.01 * lmax)
    cand[0, :] = cand[-1, :] = False
    cand[:, 0] = cand[:, -1] = False
    for j in (-1, 0, 1):
        for i in (-1, 0, 1):
            if i == 0 and j == 0:
                continue
            nb = np.full((h, w), -np.inf)
            nb[max(0, -j):h - max(0, j), max(0, -i):w - max(0, i)] = lam[max(0, j):h - max(0, -j), max(0, i):w - max(0, -i)]
            cand &= lam >= nb
    idx = np.flatnonzero(cand.ravel())
    order = idx[np.lexsort((idx, -lam.ravel()[idx]))]
    acc = []
    for k in order:
        if len(acc) >= n_max:
            break
        x, y = int(k % w), int(k // w)
        if all((x - ax) ** 2 + (y - ay) ** 2 >= min_dist * min_dist for ax, ay in acc):
            acc.append((x, y))
    return np.array(acc, dtype=np.float32).reshape(-1, 2)


def set_mask(pts, track_cnt, min_dist):
    """indices of the kept points, in keeping order"""
    order = sorted(range(len(pts)), key=lambda i: (-int(track_cnt[i]), i))
    px = pixel(pts)
    kept = []
    for i in order:
        if all((px[i, 0] - px[k, 0]) ** 2 + (px[i, 1] - px[k, 1]) ** 2 > min_dist * min_dist for k in kept):
            kept.append(i)
    return kept


def undistort(pts, cam):
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
    return np.stack([ux, uy], axis=1).astype(np.float32)


class FeatureTracker:
    def __init__(self, width, height, camera, max_cnt=200, min_dist=20):
        self.width, self.height, self.camera, self.max_cnt, self.min_dist = int(width), int(height), tuple(camera), int(max_cnt), int(min_dist)
        self.reset()

    def reset(self):
        self.ids = np.zeros(0, dtype=np.int32)
        self.track_cnt = np.zeros(0, dtype=np.int32)
        self.cur_pts = np.zeros((0, 2), dtype=np.float32)
        self.cur_un_pts = np.zeros((0, 2), dtype=np.float32)
        self.pts_velocity = np.zeros((0, 2), dtype=np.float32)
        self.n_id = 0
        self.cur_img, self.cur_time, self.prev_un = None, None, {}

    def pyramid(self, img, level):
        return build_pyramid(img)[level]

    def lk(self, img_prev, img_next, pts):
        return lk(img_prev, img_next, pts)

    def detect(self, img, kept_pts, n_max):
        return detect(img, kept_pts, n_max, self.min_dist)

    def readImage(self, img, stamp):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        assert img.shape == (self.height, self.width)
        pts, ids, cnt = self.cur_pts, self.ids, self.track_cnt
        if len(pts):
            fw, st = lk(self.cur_img, img, pts)
            keep = (st != 0) & in_border(fw, self.width, self.height)
            pts, ids, cnt = fw[keep], ids[keep], cnt[keep]
        cnt = cnt + 1
        kept = set_mask(pts, cnt, self.min_dist)
        pts, ids, cnt = pts[kept].reshape(-1, 2), ids[kept], cnt[kept]
        new = detect(img, pts, self.max_cnt - len(pts), self.min_dist)
        pts = np.concatenate([pts, new]).astype(np.float32)
        ids = np.concatenate([ids, np.full(len(new), -1)]).astype(np.int32)
        cnt = np.concatenate([cnt, np.ones(len(new))]).astype(np.int32)
        for i in range(len(ids)):
            if ids[i] == -1:
                ids[i] = self.n_id
                self.n_id += 1
        un = undistort(pts, self.camera)
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

    def feature_message(self, depths=None):
        rows = [i for i in range(len(self.ids)) if self.track_cnt[i] > 1]
        assert depths is None or len(depths) == len(rows)
        return {int(self.ids[i]): (float(self.cur_un_pts[i, 0]), float(self.cur_un_pts[i, 1]), 1.0, float(self.cur_pts[i, 0]), float(self.cur_pts[i, 1]),
                                   float(self.pts_velocity[i, 0]), float(self.pts_velocity[i, 1]), -1.0 if depths is None else float(depths[k]))
                for k, i in enumerate(rows)}


# ---- test images: seeded sums of 2-D sinusoids, rendered exactly at any warp -------------------------------------------
def texture(seed, n_waves=24, min_period=6.0, max_period=60.0):
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0, 2 * np.pi, n_waves)
    per = rng.uniform(min_period, max_period, n_waves)
    return dict(kx=2 * np.pi * np.cos(ang) / per, ky=2 * np.pi * np.sin(ang) / per, ph=rng.uniform(0, 2 * np.pi, n_waves), amp=rng.uniform(0.5, 1.0, n_waves))


def render(tex, width, height, shift=(0.0, 0.0), affine=None, flat=None):
    """uint8 image of the texture sampled at A (x, y) + shift (the scene moves by -shift: a point at p in the unshifted image appears at A^-1 (p - shift));
    flat = (x0, y0, x1, y1): a constant patch, drawn in image coordinates"""
    ys, xs = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    A = np.eye(2) if affine is None else np.asarray(affine, dtype=np.float64)
    sx = A[0, 0] * xs + A[0, 1] * ys + shift[0]
    sy = A[1, 0] * xs + A[1, 1] * ys + shift[1]
    v = np.zeros((height, width))
    for kx, ky, ph, amp in zip(tex["kx"], tex["ky"], tex["ph"], tex["amp"]):
        v += amp * np.sin(kx * sx + ky * sy + ph)
    v = 128.0 + v * (100.0 / np.sum(tex["amp"]) * 2.2)
    img = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    if flat is not None:
        img[flat[1]:flat[3], flat[0]:flat[2]] = 128
    return img
