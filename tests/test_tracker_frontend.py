"""CLAHE and rejectWithF of the image feature tracker (vilf_track_configure / _clahe / _reject_f, estimator.FeatureTracker(equalize=, f_threshold=)) against
tests/frontend_reference.py, the numpy restatement of the two paragraphs of the contract in include/vilfusion.h. No tolerance anywhere: integers and bits.
The CPU tests measure the restatement against things that are not the restatement (plain histogram equalisation in integer arithmetic, the labels of a two-view
scene built from 3-D points); the GPU tests compare the kernels with the restatement."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import track_reference as tr
import frontend_reference as fr
from vil_fusion_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(64, 48), (64, 50), (70, 50), (22, 23)]
SW, SH, FOCAL = 752, 480, 460.0
SCAM0 = (461.6, 460.3, 363.0, 248.1, 0.0, 0.0, 0.0, 0.0)
SCAM1 = (461.6, 460.3, 363.0, 248.1, -0.05, 0.01, 1.0e-4, -2.0e-4)
QW, QH = 160, 120
QCAM = (150.0, 149.0, 80.3, 60.1, -0.05, 0.01, 1.0e-4, -2.0e-4)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(bits(got), bits(want)), (what, np.flatnonzero((bits(got) != bits(want)).reshape(len(got), -1).any(axis=1))[:8])


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def clahe_images(w, h):
    """a texture with one patch of 255 and one of 0 (their bins exceed any clip limit), uniform noise, a constant"""
    tex = tr.render(tr.texture(13, min_period=5.0, max_period=40.0), w, h)
    tex[2:h // 2, 3:w // 3] = 255
    tex[h // 2 + 1:h - 1, w // 2:w - 2] = 0
    return {"texture": tex, "noise": np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w), dtype=np.uint8), "constant": np.full((h, w), 93, dtype=np.uint8)}


def project(m, cam):
    """normalised image points [n][2] -> pixels (PinholeCamera::spaceToPlane)"""
    fx, fy, cx, cy, k1, k2, p1, p2 = cam
    x, y = m[:, 0], m[:, 1]
    r2 = x * x + y * y
    rad = k1 * r2 + k2 * r2 * r2
    dx = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    dy = y * rad + 2 * p2 * x * y + p1 * (r2 + 2 * y * y)
    return np.stack([fx * (x + dx) + cx, fy * (y + dy) + cy], axis=1)


def two_view_scene(n, cam, seed, noise=0.0, outliers=0.3):
    """-> (cur [n][2] float32, forw [n][2] float32, truth uint8 [n]): 3-D points 5 - 50 m deep seen from two poses, a translation with a rotation. 70 % are exact
    projections rounded to float32 (plus Gaussian noise of `noise` px if asked for); the second point of the others is moved 10 - 40 px off its epipolar line,
    measured where rejectWithF measures it: in the pixels of the virtual camera of focal length FOCAL."""
    rng = np.random.default_rng(seed)
    ang = np.array([0.012, -0.02, 0.015])
    th = np.linalg.norm(ang)
    k = ang / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)
    t = np.array([0.5, 0.06, 0.3])
    m1, m2 = np.zeros((0, 2)), np.zeros((0, 2))
    while len(m1) < n:
        z = rng.uniform(5.0, 50.0, 4 * n)
        a = np.stack([rng.uniform(-0.85, 0.85, 4 * n), rng.uniform(-0.55, 0.55, 4 * n)], axis=1)
        P2 = np.concatenate([a * z[:, None], z[:, None]], axis=1) @ R.T + t
        b = P2[:, :2] / P2[:, 2:]
        pa, pb = project(a, cam), project(b, cam)
        ok = (np.minimum(pa, pb).min(axis=1) >= 2) & (np.maximum(pa[:, 0], pb[:, 0]) <= SW - 3) & (np.maximum(pa[:, 1], pb[:, 1]) <= SH - 3)
        m1, m2 = np.concatenate([m1, a[ok]]), np.concatenate([m2, b[ok]])
    m1, m2 = m1[:n].copy(), m2[:n].copy()
    truth = np.ones(n, dtype=np.uint8)
    truth[rng.permutation(n)[:int(round(outliers * n))]] = 0
    E = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R
    line = np.concatenate([m1, np.ones((n, 1))], axis=1) @ E.T          # l' = E x, in normalised coordinates
    nrm = line[:, :2] / np.linalg.norm(line[:, :2], axis=1)[:, None]
    off = rng.uniform(10.0, 40.0, n) * rng.choice([-1.0, 1.0], n) / FOCAL
    m2 = m2 + np.where(truth[:, None] == 0, nrm * off[:, None], 0.0)
    pa, pb = project(m1, cam), project(m2, cam)
    if noise > 0:
        g = rng.normal(0.0, noise, (2, n, 2))
        pa, pb = pa + np.where(truth[:, None] == 1, g[0], 0.0), pb + np.where(truth[:, None] == 1, g[1], 0.0)
    return pa.astype(np.float32), pb.astype(np.float32), truth


def moving_square_sequence(n=6):
    """160 x 120: a background that drifts one way (with a little rotation) and two 40 x 40 textured squares that move across it in two other directions. One
    moving square on a flat background would not do: a plane's motion leaves the epipole free, and F = [e']x H with e' at infinity along the square's relative
    motion explains the square as well. Two relative motions cannot share an epipole, so the square with fewer points is rejected."""
    tex, sq = tr.texture(7, min_period=6.0, max_period=40.0), tr.texture(19, min_period=5.0, max_period=16.0)
    out = []
    for k in range(n):
        img = tr.render(tex, QW, QH, shift=(1.3 * k, -0.7 * k), affine=[[1.0, 0.004 * k], [-0.003 * k, 1.0]])
        for (x0, y0), (vx, vy) in (((20, 22), (0.5 * k, 2.0 * k)), ((104, 66), (-2.0 * k, -1.0 * k))):
            obj = tr.render(sq, QW, QH, shift=(-vx, -vy))          # the texture moves with its square
            xa, ya = int(x0 + vx), int(y0 + vy)
            img[ya:ya + 40, xa:xa + 40] = obj[ya:ya + 40, xa:xa + 40]
        out.append(img)
    return out


FRONT = dict(equalize=True, f_threshold=1.0, focal_length=FOCAL, clahe=(3.0, 8, 8), n_hypotheses=512, seed=0)


# ---- CPU: what the restatement is worth ----------------------------------------------------------------------------------------
def plain_equalisation(img):
    """rint(cdf 255 / area) in integer arithmetic (round half to even), nothing shared with the restatement"""
    area = img.size
    cum = np.cumsum(np.bincount(img.ravel(), minlength=256)).astype(np.int64) * 255
    q, r = cum // area, cum % area
    lut = q + ((2 * r > area) | ((2 * r == area) & (q % 2 == 1)))
    return lut[img].astype(np.uint8)


def test_clahe_one_tile_clip_0_is_histogram_equalisation():
    # 64 x 48: area 3072 = 3 * 2^10, so 255 / area = 85 / 1024 and every product cum * (255 / area) are exact in float32: the float32 text and the integer
    # arithmetic round the same exact number
    rng = np.random.default_rng(5)
    noise = rng.integers(0, 256, (48, 64), dtype=np.uint8)
    two = np.where(rng.uniform(size=(48, 64)) < 0.37, 40, 200).astype(np.uint8)
    for img in (noise, two):
        assert fr.clahe_geometry(64, 48, 1, 1) == (64, 48, 64, 48) and fr.clahe_limit(0.0, 3072) == 0
        same(fr.clahe(img, 0.0, 1, 1), plain_equalisation(img))
    assert sorted(set(fr.clahe(two, 0.0, 1, 1).ravel().tolist())) == sorted({int(np.rint(255 * (two == 40).mean())), 255})


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("clip,tx,ty", [(3.0, 8, 8), (0.0, 8, 8), (40.0, 2, 2), (3.0, 3, 5), (1.0, 1, 1)])
def test_clahe_monotone_and_constant(w, h, clip, tx, ty):
    imgs = clahe_images(w, h)
    _, _, tw, th = fr.clahe_geometry(w, h, tx, ty)
    for name in ("texture", "noise"):
        img = imgs[name]
        luts, out = fr.clahe_luts(img, clip, tx, ty), fr.clahe(img, clip, tx, ty)
        assert (np.diff(luts.astype(np.int64), axis=2) >= 0).all()          # a tile's curve never falls ...
        if tw % 2 == 0 and th % 2 == 0:                                      # ... and at a tile's centre pixel the output is that curve alone (weights 1 and 0, up to the rounding of 1 / tw, which rint absorbs)
            for j in range(ty):
                for i in range(tx):
                    x, y = i * tw + tw // 2, j * th + th // 2
                    if x < w and y < h:
                        assert out[y, x] == luts[j, i, img[y, x]]
    const = fr.clahe(imgs["constant"], clip, tx, ty)
    assert (const == const[0, 0]).all()


def test_clahe_geometry_and_limit():
    assert fr.clahe_geometry(64, 48, 8, 8) == (64, 48, 8, 6)                 # no padding
    assert fr.clahe_geometry(64, 50, 8, 8) == (72, 56, 9, 7)                 # y pads 6, x a whole 8: tw = 9, not 8
    assert fr.clahe_geometry(70, 50, 8, 8) == (72, 56, 9, 7)
    assert fr.clahe_geometry(22, 23, 8, 8) == (24, 24, 3, 3)
    assert fr.clahe_limit(3.0, 9) == 1 and fr.clahe_limit(3.0, 48) == 1 and fr.clahe_limit(3.0, 7238) == 84 and fr.clahe_limit(0.0, 9) == 0
    assert fr.clahe_geometry(1226, 370, 8, 8) == (1232, 376, 154, 47)
    # the padded columns are reflections: widening the image by what the padding would add changes no tile's curve
    img = clahe_images(64, 50)["texture"]
    pad = img[tr.reflect(np.arange(56), 50)][:, tr.reflect(np.arange(72), 64)]
    same(fr.clahe_luts(img, 3.0, 8, 8), fr.clahe_luts(pad, 3.0, 8, 8))


@pytest.mark.parametrize("cam", [SCAM0, SCAM1], ids=["pinhole", "distorted"])
def test_reject_f_recovers_the_labels(cam):
    cur, forw, truth = two_view_scene(200, cam, 1)
    st, best, n_in, F = fr.reject_f(cur, forw, cam, SW, SH, FOCAL, 1.0, 512, 0)
    assert truth.sum() == 140 and np.array_equal(st, truth) and n_in == 140 and 0 <= best < 512
    assert np.isfinite(F).all() and abs(np.linalg.det(F.reshape(3, 3) / np.abs(F).max())) < 1e-9          # rank 2


@pytest.mark.parametrize("cam", [SCAM0, SCAM1], ids=["pinhole", "distorted"])
def test_reject_f_with_noise_rejects_every_displaced_point(cam):
    cur, forw, truth = two_view_scene(200, cam, 1, noise=0.3)
    st, best, n_in, _ = fr.reject_f(cur, forw, cam, SW, SH, FOCAL, 1.0, 512, 0)
    print(f"0.3 px noise: {int(st[truth == 1].sum())} of {int(truth.sum())} true inliers kept ({st[truth == 1].mean():.3f}), hypothesis {best}")
    assert not st[truth == 0].any() and n_in == st.sum()


def test_reject_f_camera_at_rest_keeps_everything():
    # measured on the CPU first: the null space of A holds the skew matrices, x^T F x = 0 for each of them, and every point is an inlier of hypothesis 0
    cur, _, _ = two_view_scene(100, SCAM1, 2)
    st, best, n_in, F = fr.reject_f(cur, cur, SCAM1, SW, SH, FOCAL, 1.0, 512, 0)
    assert st.all() and best == 0 and n_in == 100
    Fm = F.reshape(3, 3)
    assert np.abs(Fm + Fm.T).max() <= 1e-9 * np.abs(Fm).max()


def test_reject_f_small_counts_and_degenerate_input():
    cur, forw, truth = two_view_scene(200, SCAM1, 1)
    a, b = cur[truth == 1], forw[truth == 1]
    st, best, n_in, F = fr.reject_f(a[:7], b[:7], SCAM1, SW, SH, FOCAL, 1.0, 512, 0)
    assert st.all() and len(st) == 7 and best == -1 and n_in == 7 and not F.any()
    st, best, n_in, F = fr.reject_f(a[:8], b[:8], SCAM1, SW, SH, FOCAL, 1.0, 512, 0)          # every sample is these eight points: inliers of their own model
    assert st.all() and best == 0 and n_in == 8 and F.any()
    same_pt = np.tile(a[:1], (50, 1))
    st, best, n_in, F = fr.reject_f(same_pt, same_pt, SCAM1, SW, SH, FOCAL, 1.0, 512, 0)      # mean distance 0: no scale, no valid hypothesis
    assert st.all() and best == -1 and n_in == 50 and not F.any()


@pytest.mark.parametrize("n", [8, 9, 1000])
def test_samples_are_distinct_and_in_range(n):
    S = fr.samples(n, fr.MAX_HYPOTHESES, 0)
    assert S.shape == (2048, 8) and S.min() >= 0 and S.max() < n
    assert (np.diff(np.sort(S, axis=1), axis=1) > 0).all()
    assert np.array_equal(S[:512], fr.samples(n, 512, 0))                    # hypothesis k does not depend on K
    assert (fr.samples(n, 2048, 1) != S).any(axis=1).mean() > (0.9 if n > 9 else 0.5)
    if n == 1000:
        assert len(np.unique(S)) > 990                                       # the indices are spread over the list


def test_track_frontend_layout(tmp_path):
    ct = abi.TrackFrontend
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "vilfusion.h"', "int main(void) {", '  printf("%zu\\n", sizeof(vilf_track_frontend));']
    want = [C.sizeof(ct)]
    for fname, _ in ct._fields_:
        prog.append(f'  printf("%zu\\n", offsetof(vilf_track_frontend, {fname}));')
        want.append(getattr(ct, fname).offset)
    prog += ['  printf("%d\\n%d\\n", VILF_TRACK_MAX_TILES, VILF_TRACK_MAX_HYPOTHESES);', "  return 0;", "}"]
    want += [abi.VILF_TRACK_MAX_TILES, abi.VILF_TRACK_MAX_HYPOTHESES]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(prog))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want and fr.MAX_TILES == abi.VILF_TRACK_MAX_TILES and fr.MAX_HYPOTHESES == abi.VILF_TRACK_MAX_HYPOTHESES


def test_moving_square_is_rejected_by_the_restatement():
    """the seed of the GPU sequence test is fixed here: rejectWithF drops something in some frame, and the result differs from the tracker without it"""
    ref, plain = fr.FeatureTracker(QW, QH, QCAM, max_cnt=60, min_dist=10, **FRONT), fr.FeatureTracker(QW, QH, QCAM, max_cnt=60, min_dist=10, equalize=True)
    for k, img in enumerate(moving_square_sequence()):
        ref.readImage(img, 0.05 * k)
        plain.readImage(img, 0.05 * k)
    print("rejected per frame:", ref.rejected)
    assert len(ref.rejected) == 5 and sum(ref.rejected) >= 1 and not np.array_equal(ref.ids, plain.ids)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver():
    from vil_fusion_amd.estimator import BackendSolver
    s = BackendSolver()
    yield s
    s.close()


def make(solver, w, h, cam, max_cnt=200, min_dist=20, **front):
    from vil_fusion_amd.estimator import FeatureTracker
    return FeatureTracker(solver, w, h, cam, max_cnt=max_cnt, min_dist=min_dist, **front), fr.FeatureTracker(w, h, cam, max_cnt=max_cnt, min_dist=min_dist, **front)


def compare_state(t, ref, what):
    same(t.ids, ref.ids, what + " ids")
    same(t.track_cnt, ref.track_cnt, what + " track_cnt")
    same(t.cur_pts, ref.cur_pts, what + " cur_pts")
    same(t.cur_un_pts, ref.cur_un_pts, what + " cur_un_pts")
    same(t.pts_velocity, ref.pts_velocity, what + " pts_velocity")


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
def test_clahe_sizes(solver, w, h):
    t, ref = make(solver, w, h, QCAM)
    for name, img in clahe_images(w, h).items():
        same(t.clahe(img), ref.clahe(img), name)
    wide = np.random.default_rng(3).integers(0, 256, (h, w + 13), dtype=np.uint8)
    view = wide[:, 5:5 + w]
    assert view.strides[0] > w
    same(t.clahe(view), ref.clahe(np.ascontiguousarray(view)), "row stride")


@pytest.mark.gpu
@pytest.mark.parametrize("clip,tx,ty", [(0.0, 8, 8), (3.0, 1, 1), (3.0, 3, 5), (40.0, 32, 32)])
def test_clahe_clip_and_tiles(solver, clip, tx, ty):
    for w, h in ((64, 50), (70, 50)):
        t, ref = make(solver, w, h, QCAM, clahe=(clip, tx, ty))
        for name, img in clahe_images(w, h).items():
            same(t.clahe(img), ref.clahe(img), f"{w} x {h} {name}")


@pytest.fixture(scope="module")
def scene1000():
    return two_view_scene(1000, SCAM1, 4)


def compare_reject(t, ref, cur, forw, what):
    st, best, n_in, F = t.reject_f(cur, forw)
    rst, rbest, rn_in, rF = ref.reject_f(cur, forw)
    assert (best, n_in) == (rbest, rn_in), (what, best, n_in, rbest, rn_in)
    same(st, rst, what + " status")
    same(F, rF, what + " F")
    return st, best


@pytest.mark.gpu
@pytest.mark.parametrize("n", [7, 8, 9, 63, 64, 65, 200, 1000])
def test_reject_f_counts(solver, scene1000, n):
    cur, forw, truth = scene1000
    t, ref = make(solver, SW, SH, SCAM1, **FRONT)
    st, best = compare_reject(t, ref, cur[:n], forw[:n], f"n = {n}")
    assert (best == -1) == (n < 8)
    if n >= 63:
        assert np.array_equal(st, truth[:n])


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 64, 512, 2048])
def test_reject_f_hypothesis_counts(solver, scene1000, K):
    cur, forw, _ = scene1000
    t, ref = make(solver, SW, SH, SCAM0, f_threshold=1.0, n_hypotheses=K, seed=3)
    _, best = compare_reject(t, ref, cur[:65], forw[:65], f"K = {K}")
    assert 0 <= best < K


@pytest.mark.gpu
def test_reject_f_at_rest_and_all_equal(solver, scene1000):
    cur = scene1000[0]
    t, ref = make(solver, SW, SH, SCAM1, **FRONT)
    st, best = compare_reject(t, ref, cur[:100], cur[:100], "at rest")
    assert st.all() and best == 0
    same_pt = np.tile(cur[:1], (50, 1))
    st, best = compare_reject(t, ref, same_pt, same_pt, "all equal")
    assert st.all() and best == -1


@pytest.mark.gpu
def test_moving_square_sequence(solver):
    t, ref = make(solver, QW, QH, QCAM, max_cnt=60, min_dist=10, **FRONT)
    for k, img in enumerate(moving_square_sequence()):
        stamp = 100.0 + 0.05 * k
        assert t.readImage(img, stamp) == ref.readImage(img, stamp)
        compare_state(t, ref, f"frame {k}")
    assert sum(ref.rejected) >= 1


@pytest.mark.gpu
def test_nothing_existing_moved(solver):
    """a tracker that never configured and one configured with both steps off: both are the tracker of track_reference.py"""
    from vil_fusion_amd.estimator import FeatureTracker
    imgs = moving_square_sequence()
    for front in (dict(), dict(equalize=False, f_threshold=None, clahe=(2.0, 4, 4), n_hypotheses=64, seed=5)):
        t, ref = FeatureTracker(solver, QW, QH, QCAM, max_cnt=60, min_dist=10, **front), tr.FeatureTracker(QW, QH, QCAM, max_cnt=60, min_dist=10)
        assert bool(front) == (t.frontend.clahe_tiles_x == 4)
        for k, img in enumerate(imgs):
            assert t.readImage(img, 0.05 * k) == ref.readImage(img, 0.05 * k)
            compare_state(t, ref, f"{'configured off' if front else 'never configured'}, frame {k}")


@pytest.mark.gpu
def test_refusals(solver):
    from vil_fusion_amd.estimator import BackendSolver
    L, h = solver._L, solver._h
    imgs = moving_square_sequence(3)
    t, ref = make(solver, QW, QH, QCAM, max_cnt=60, min_dist=10, **FRONT)
    for k in range(2):
        t.readImage(imgs[k], 0.05 * k)
        ref.readImage(imgs[k], 0.05 * k)
    good = dict(equalize=1, clahe_clip=3.0, clahe_tiles_x=8, clahe_tiles_y=8, reject_f=1, f_threshold=1.0, focal_length=FOCAL, n_hypotheses=512, seed=0)
    bad = [dict(clahe_tiles_x=0), dict(clahe_tiles_y=-1), dict(clahe_tiles_x=33, clahe_tiles_y=32), dict(clahe_clip=-0.5), dict(clahe_clip=float("nan")), dict(clahe_clip=float("inf")),
           dict(f_threshold=0.0), dict(f_threshold=-1.0), dict(f_threshold=float("inf")), dict(focal_length=0.0), dict(focal_length=float("nan")),
           dict(n_hypotheses=0), dict(n_hypotheses=2049),
           dict(equalize=0, reject_f=0, n_hypotheses=0)]                       # every field is checked, whether its step is on or not
    for b in bad:
        fe = abi.TrackFrontend(**{**good, **b})
        assert L.vilf_track_configure(h, C.byref(fe)) == abi.VILF_ERR_INVALID_ARGUMENT, b
    assert L.vilf_track_configure(h, None) == abi.VILF_ERR_INVALID_ARGUMENT
    # rejectWithF: outputs untouched
    cur, forw, _ = two_view_scene(20, QCAM, 1)
    fp, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    nan_pt, inf_pt = forw.copy(), cur.copy()
    nan_pt[13, 1], inf_pt[0, 0] = np.nan, np.inf
    big = np.zeros((abi.VILF_MAX_FEATURES + 1, 2), dtype=np.float32)
    for a, b, n in ((cur, forw, -1), (big, big, abi.VILF_MAX_FEATURES + 1), (cur, nan_pt, 20), (inf_pt, forw, 20)):
        st, F, best, n_in = np.full(len(a), 77, dtype=np.uint8), np.full(9, -3.5), C.c_int(-7), C.c_int(-9)
        rc = L.vilf_track_reject_f(h, a.ctypes.data_as(fp), b.ctypes.data_as(fp), n, st.ctypes.data_as(u8p), abi.dptr(F), C.byref(best), C.byref(n_in))
        assert rc == abi.VILF_ERR_INVALID_ARGUMENT and (st == 77).all() and (F == -3.5).all() and best.value == -7 and n_in.value == -9, n
    out = np.full((QH, QW), 55, dtype=np.uint8)
    assert L.vilf_track_clahe(h, imgs[2].ctypes.data_as(u8p), QW - 1, out.ctypes.data_as(u8p)) == abi.VILF_ERR_INVALID_ARGUMENT and (out == 55).all()
    # a handle without a tracker
    other = BackendSolver()
    try:
        fe = abi.TrackFrontend(**good)
        st, F, best, n_in = np.full(20, 77, dtype=np.uint8), np.full(9, -3.5), C.c_int(-7), C.c_int(-9)
        ms, cnt = (C.c_double * 2)(-1.0, -1.0), (C.c_long * 2)(-1, -1)
        assert L.vilf_track_configure(other._h, C.byref(fe)) == abi.VILF_ERR_INVALID_ARGUMENT
        assert L.vilf_track_clahe(other._h, imgs[2].ctypes.data_as(u8p), QW, out.ctypes.data_as(u8p)) == abi.VILF_ERR_INVALID_ARGUMENT and (out == 55).all()
        assert L.vilf_track_reject_f(other._h, cur.ctypes.data_as(fp), forw.ctypes.data_as(fp), 20, st.ctypes.data_as(u8p), abi.dptr(F), C.byref(best), C.byref(n_in)) == abi.VILF_ERR_INVALID_ARGUMENT
        assert (st == 77).all() and (F == -3.5).all() and best.value == -7 and n_in.value == -9
    finally:
        other.close()
    # the stateless calls and the refused ones left the tracker alone: the next frame still agrees with the restatement
    compare_reject(t, ref, cur, forw, "between frames")
    same(t.clahe(imgs[0]), ref.clahe(imgs[0]), "between frames")
    assert t.readImage(imgs[2], 0.1) == ref.readImage(imgs[2], 0.1)
    compare_state(t, ref, "after the refused calls")
    # a later vilf_track_init returns to "both off"
    t2, ref2 = make(solver, QW, QH, QCAM, max_cnt=60, min_dist=10)
    for k in range(2):
        assert t2.readImage(imgs[k], 0.05 * k) == ref2.readImage(imgs[k], 0.05 * k)
        compare_state(t2, ref2, f"after a new init, frame {k}")


@pytest.mark.gpu
def test_full_size_frame_pair_with_both_steps(solver):
    w, h = 1226, 370
    assert fr.clahe_geometry(w, h, 8, 8) == (1232, 376, 154, 47)             # pads 6 / 6
    tex = tr.texture(21, n_waves=40, min_period=8.0, max_period=120.0)
    imgs = [tr.render(tex, w, h), tr.render(tex, w, h, shift=(3.7, -1.4))]
    cam = (718.856, 718.856, 607.19, 185.22, -0.05, 0.01, 1.0e-4, -2.0e-4)
    t, ref = make(solver, w, h, cam, max_cnt=100, min_dist=30, **FRONT)
    solver.set_profiling(True)
    try:
        for k, img in enumerate(imgs):
            assert t.readImage(img, 0.1 * k) == ref.readImage(img, 0.1 * k)
            compare_state(t, ref, f"frame {k}")
            print(f"1226 x 370, frame {k}: {len(t.ids)} points; stage ms " + ", ".join(f"{name} {ms:.3f}" for name, (ms, _) in t.profile().items()) +
                  "; front-end ms " + ", ".join(f"{name} {ms:.3f} ({cnt})" for name, (ms, cnt) in t.profile_frontend().items()))
        assert t.profile_frontend()["clahe"][1] == 1 and t.profile_frontend()["reject_f"][1] == 1          # one span each in the last frame
    finally:
        solver.set_profiling(False)
    assert len(t.ids) == 100 and (t.track_cnt > 1).sum() >= 50
