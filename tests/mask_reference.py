"""numpy restatement of the dynamic-object mask and the fisheye mask of the image feature tracker, written from the contract text in include/vilfusion.h
("Image feature tracker", paragraphs mask image, erode, probe, rejectWithF_mask, fisheye mask, detection under the dynamic mask, frame order).

Built on track_reference.py and frontend_reference.py, which are imported as they are. Every float operation is one numpy elementwise operation on float64
values, rounded on its own. No code is shared with csrc."""
import numpy as np
import track_reference as tr
import frontend_reference as fr

MAX_ERODE = 16


# ---- erode ---------------------------------------------------------------------------------------------------------------------
def half_widths(r):
    """hw(d) for d = 0 .. r"""
    return [int(np.rint(np.sqrt(np.float64(r * r - d * d)))) for d in range(r + 1)]


def element(r):
    """the structuring element as a bool array (2 r + 1, 2 r + 1), [dy + r][dx + r]"""
    hw = half_widths(r)
    el = np.zeros((2 * r + 1, 2 * r + 1), dtype=bool)
    for dy in range(-r, r + 1):
        el[dy + r, r - hw[abs(dy)]:r + hw[abs(dy)] + 1] = True
    return el


def erode(mask, r=5):
    """E: 255 where every element offset that lies inside the image hits a mask pixel != 0, else 0"""
    assert 0 <= r <= MAX_ERODE
    mask = np.asarray(mask, dtype=np.uint8)
    h, w = mask.shape
    pad = np.ones((h + 2 * r, w + 2 * r), dtype=bool)          # outside the image does not erode
    pad[r:r + h, r:r + w] = mask != 0
    out = np.ones((h, w), dtype=bool)
    hw = half_widths(r)
    for dy in range(-r, r + 1):
        for dx in range(-hw[abs(dy)], hw[abs(dy)] + 1):
            out &= pad[r + dy:r + dy + h, r + dx:r + dx + w]
    return np.where(out, 255, 0).astype(np.uint8)


# ---- probe ---------------------------------------------------------------------------------------------------------------------
def probe(E, pts, d=5):
    """uint8 [n]: 1 = static"""
    E = np.asarray(E, dtype=np.uint8)
    h, w = E.shape
    out = np.ones(len(np.asarray(pts).reshape(-1, 2)), dtype=np.uint8)
    for i, (x, y) in enumerate(tr.pixel(pts)):
        x, y = int(x), int(y)
        if x > d and y > d and x < w - d and y < h - d:
            out[i] = 1 if (E[y - d, x] != 0 and E[y + d, x] != 0 and E[y, x - d] != 0 and E[y, x + d] != 0) else 0
    return out


# ---- rejectWithF_mask ------------------------------------------------------------------------------------------------------------
def reject_f_mask(cur_pts, forw_pts, is_static, cam, w, h, focal=460.0, f_thr=0.1, epi_thr=1.0, K=512, seed=0):
    """-> (status uint8 [n], best, n_static_inliers, F float64 [9]); best = -1 (F = 0, every status 1, the count of the static pairs) when fewer than 8 pairs are
    static or no hypothesis is valid"""
    cur_pts = np.asarray(cur_pts, dtype=np.float32).reshape(-1, 2)
    forw_pts = np.asarray(forw_pts, dtype=np.float32).reshape(-1, 2)
    st = np.asarray(is_static).reshape(-1) != 0
    n, m = len(cur_pts), int(st.sum())
    assert len(forw_pts) == n and len(st) == n and 1 <= K <= fr.MAX_HYPOTHESES
    none = (np.ones(n, dtype=np.uint8), -1, m, np.zeros(9))
    if m < 8:
        return none
    ua, ub = fr.lift(cur_pts, cam, w, h, focal), fr.lift(forw_pts, cam, w, h, focal)
    sa, sb = ua[st], ub[st]                                    # S in list order; the sample indices address S
    F, valid = fr.hypotheses(sa, sb, K, seed)
    score = np.where(valid, fr.inliers(F, sa, sb, f_thr).sum(axis=1), -1)
    best = int(np.argmax(score))
    if score[best] < 0:
        return none
    f = F[best]
    x, y, xp, yp = (v.astype(np.float64) for v in (ua[:, 0], ua[:, 1], ub[:, 0], ub[:, 1]))
    with np.errstate(all="ignore"):
        A = (f[0] * x + f[1] * y) + f[2]
        B = (f[3] * x + f[4] * y) + f[5]
        Cc = (f[6] * x + f[7] * y) + f[8]
        dd = np.abs((A * xp + B * yp) + Cc) / np.sqrt(A * A + B * B)
        drop = dd > np.float64(epi_thr)                        # a NaN compares false: kept
    return np.where(drop, 0, 1).astype(np.uint8), best, int(score[best]), f.copy()


# ---- detection with an extra allowed mask, setMask with a fisheye image ---------------------------------------------------------------
def detect(img, kept_pts, n_max, min_dist, allowed=None):
    """track_reference.detect with `allowed` (bool [H][W] or None) and-ed into the allowed pixels"""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape
    out = np.zeros((0, 2), dtype=np.float32)
    if n_max <= 0:
        return out
    lam = tr.eigen_map(img)
    ok = tr.allowed_mask(w, h, kept_pts, min_dist)
    if allowed is not None:
        ok = ok & np.asarray(allowed, dtype=bool)
    if not ok.any():
        return out
    lmax = lam[ok].max()
    cand = ok & (lam > 0.01 * lmax)
    cand[0, :] = cand[-1, :] = False
    cand[:, 0] = cand[:, -1] = False
    ys, xs = np.nonzero(cand)
    keep = np.ones(len(ys), dtype=bool)
    for j in (-1, 0, 1):
        for i in (-1, 0, 1):
            keep &= lam[ys, xs] >= lam[ys + j, xs + i]          # candidates are inner pixels, so every neighbour exists
    idx = ys[keep] * w + xs[keep]
    order = idx[np.lexsort((idx, -lam.ravel()[idx]))]
    acc = []
    for k in order:
        if len(acc) >= n_max:
            break
        x, y = int(k % w), int(k // w)
        if all((x - ax) ** 2 + (y - ay) ** 2 >= min_dist * min_dist for ax, ay in acc):
            acc.append((x, y))
    return np.array(acc, dtype=np.float32).reshape(-1, 2)


def allowed_pixels(E=None, fisheye=None):
    """what the masks allow the detection (bool [H][W]), None if there is neither"""
    ok = None
    for m in (E, fisheye):
        if m is not None:
            ok = (np.asarray(m) != 0) if ok is None else ok & (np.asarray(m) != 0)
    return ok


def set_mask(pts, track_cnt, min_dist, fisheye=None):
    """indices of the kept points, in keeping order; with a fisheye image only the points whose pixel holds 255 there take part"""
    if fisheye is None:
        return tr.set_mask(pts, track_cnt, min_dist)
    px = tr.pixel(pts)
    rows = [i for i in range(len(px)) if fisheye[px[i, 1], px[i, 0]] == 255]
    if not rows:
        return []
    sub = tr.set_mask(np.asarray(pts, dtype=np.float32).reshape(-1, 2)[rows], np.asarray(track_cnt)[rows], min_dist)
    return [rows[k] for k in sub]


class FeatureTracker(fr.FeatureTracker):
    """frontend_reference.FeatureTracker with readImage_mask and the fisheye mask. Both entry points run the one frame below, so they share all state."""

    def __init__(self, *args, **kw):
        self.mask_params = dict(erode_radius=5, probe=5, reject=True, f_threshold=0.1, epi_threshold=1.0)
        self.fisheye = None
        self.stats = []                                      # per masked frame with a previous one: (survivors, static, rejected, rejected non-static)
        self.new_pts, self.E_frames = [], []                 # per frame: the new corners, E (None for a plain frame)
        self.last_E = None
        super().__init__(*args, **kw)

    def configure_mask(self, erode_radius=5, probe=5, reject=True, f_threshold=0.1, epi_threshold=1.0):
        self.mask_params = dict(erode_radius=int(erode_radius), probe=int(probe), reject=bool(reject), f_threshold=float(f_threshold), epi_threshold=float(epi_threshold))

    def set_fisheye_mask(self, mask):
        self.fisheye = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8).copy()

    def erode(self, mask):
        return erode(mask, self.mask_params["erode_radius"])

    def probe(self, eroded, pts):
        return probe(eroded, pts, self.mask_params["probe"])

    def reject_f_mask(self, cur_pts, forw_pts, is_static):
        return reject_f_mask(cur_pts, forw_pts, is_static, self.camera, self.width, self.height, self.focal_length, self.mask_params["f_threshold"],
                             self.mask_params["epi_threshold"], self.n_hypotheses, self.seed)

    def detect(self, img, kept_pts, n_max):
        return detect(img, kept_pts, n_max, self.min_dist, allowed_pixels(None, self.fisheye))

    def detect_masked(self, img, eroded, kept_pts, n_max):
        return detect(img, kept_pts, n_max, self.min_dist, allowed_pixels(eroded, self.fisheye))

    def readImage(self, img, stamp):
        return self._frame(img, None, stamp)

    def readImage_mask(self, img, mask, stamp):
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        assert mask.shape == (self.height, self.width)
        return self._frame(img, mask, stamp)

    def _frame(self, img, mask, stamp):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        assert img.shape == (self.height, self.width)
        if self.equalize:
            img = self.clahe(img)
        E = None if mask is None else self.erode(mask)
        self.last_E = E
        self.E_frames.append(E)
        pts, ids, cnt = self.cur_pts, self.ids, self.track_cnt
        if len(pts):
            fw, st = tr.lk(self.cur_img, img, pts)
            keep = (st != 0) & tr.in_border(fw, self.width, self.height)
            cur, pts, ids, cnt = pts[keep], fw[keep], ids[keep], cnt[keep]
            if mask is None:
                if self.f_threshold is not None:
                    ok = self.reject_f(cur, pts)[0] != 0
                    self.rejected.append(int((~ok).sum()))
                    pts, ids, cnt = pts[ok], ids[ok], cnt[ok]
            else:
                static = self.probe(E, pts) != 0
                ok = np.ones(len(pts), dtype=bool)
                if self.mask_params["reject"]:
                    ok = self.reject_f_mask(cur, pts, static)[0] != 0
                self.stats.append((len(pts), int(static.sum()), int((~ok).sum()), int((~ok & ~static).sum())))
                pts, ids, cnt = pts[ok], ids[ok], cnt[ok]
        cnt = cnt + 1
        kept = set_mask(pts, cnt, self.min_dist, self.fisheye)
        pts, ids, cnt = pts[kept].reshape(-1, 2), ids[kept], cnt[kept]
        new = detect(img, pts, self.max_cnt - len(pts), self.min_dist, allowed_pixels(E, self.fisheye))
        self.new_pts.append(new.copy())
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
