"""Image feature tracker (vilf_track_*, vil_fusion_amd.estimator.FeatureTracker) against tests/track_reference.py, the numpy restatement of the contract in
include/vilfusion.h. The CPU tests pin the restatement itself (against rendered ground truth); the GPU tests compare the kernels with it bit for bit: uint8 and
int outputs with array_equal, float32 outputs as uint32 views."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import track_reference as tr
from vil_fusion_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 185, 93
CAM0 = (92.0, 91.5, 92.3, 46.1, 0.0, 0.0, 0.0, 0.0)
CAM1 = (92.0, 91.5, 92.3, 46.1, -0.28, 0.07, 1.9e-4, -1.7e-5)
SHIFTS = {"sub": (0.37, -0.21), "3px": (2.4, -1.8), "12px": (-10.5, 5.8)}
# worst error of the restatement against the rendered shift over the status-1 points of grid_points(), measured on the CPU; the test asserts twice it
REF_ERR = {"sub": 0.0257, "3px": 0.0206, "12px": 0.0231}
FLAT = (120, 30, 170, 80)          # a constant patch of the textured image: no texture, the eigenvalue gate


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(bits(got), bits(want)), (what, np.flatnonzero((bits(got) != bits(want)).reshape(len(got), -1).any(axis=1))[:8])


def grid_points():
    gx, gy = np.meshgrid(np.arange(30, W - 30, 12.5), np.arange(25, H - 25, 9.5))
    return np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float32) + np.float32(0.25)


@pytest.fixture(scope="module")
def images():
    tex = tr.texture(7)
    d = {"base": tr.render(tex, W, H), "flat": tr.render(tex, W, H, flat=FLAT)}
    for k, sh in SHIFTS.items():
        d[k] = tr.render(tex, W, H, shift=sh)
        d[k + "_flat"] = tr.render(tex, W, H, shift=sh, flat=FLAT)
    d["small0"] = tr.render(tr.texture(11, min_period=5.0, max_period=20.0), 23, 22)
    d["small1"] = tr.render(tr.texture(11, min_period=5.0, max_period=20.0), 23, 22, shift=(0.4, 0.3))
    return d


def many_points(n, seed=3):
    """points of every kind: within 10 px of each border and in each corner, on the flat patch, and spread over the image"""
    rng = np.random.default_rng(seed)
    edge = [(0.0, 0.0), (W - 1.0, 0.0), (0.0, H - 1.0), (W - 1.0, H - 1.0), (3.5, 4.25), (W - 4.5, 5.0), (2.0, H - 3.0), (W - 2.75, H - 6.5),
            (5.0, 40.0), (W - 6.0, 50.5), (90.0, 4.0), (77.7, H - 5.5), (9.99, 9.99), (W - 10.0, H - 10.0)]
    flat = [(FLAT[0] + 14 + 3.0 * i, FLAT[1] + 14 + 2.5 * i) for i in range(8)]
    rest = np.stack([rng.uniform(12, W - 12, n), rng.uniform(12, H - 12, n)], 1)
    return np.concatenate([np.array(edge), np.array(flat), rest])[:n].astype(np.float32)


# ---- CPU: the restatement itself -------------------------------------------------------------------------------------------
def test_constant_image_stays_constant_through_the_pyramid():
    lv = tr.build_pyramid(np.full((370, 1226), 77, dtype=np.uint8))
    assert len(lv) == 4 and all((l == 77).all() for l in lv)


@pytest.mark.parametrize("w,h,lmax,sizes", [(185, 93, 2, [(185, 93), (93, 47), (47, 24)]), (23, 22, 0, [(23, 22)]),
                                            (1226, 370, 3, [(1226, 370), (613, 185), (307, 93), (154, 47)])])
def test_level_sizes_and_lmax(w, h, lmax, sizes):
    assert tr.level_sizes(w, h) == sizes and len(sizes) - 1 == lmax
    assert [l.shape[::-1] for l in tr.build_pyramid(np.zeros((h, w), dtype=np.uint8))] == sizes


def test_reflect_is_periodic():
    assert list(tr.reflect(np.arange(-7, 9), 4)) == [1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2]


def test_weights_sum_to_16384():
    rng = np.random.default_rng(0)
    for p in rng.uniform(-5, 60, (200, 2)).astype(np.float32):
        ix, iy, wt = tr.corner(p, 80, 80)
        assert sum(wt) == 16384 and min(wt[:3]) >= 0 and wt[3] >= -1
    assert tr.corner(np.float32([10.0, 10.0]), 80, 80) == (0, 0, (16384, 0, 0, 0))
    assert tr.corner(np.float32([-11.5, 10.0]), 80, 80) is None and tr.corner(np.float32([90.0, 10.0]), 80, 80) is None
    assert tr.corner(np.float32([-11.0, 10.0]), 80, 80)[0] == -21


@pytest.mark.parametrize("name", ["sub", "3px", "12px"])
def test_reference_recovers_rendered_translation(images, name):
    pts = grid_points()
    out, st = tr.lk(images["base"], images[name], pts)
    assert st.sum() * 2 >= len(st)
    err = np.abs(out.astype(np.float64) - (pts.astype(np.float64) - np.array(SHIFTS[name]))).max(axis=1)[st == 1].max()
    print(f"reference LK, shift {name}: worst error {err:.4f} px over {int(st.sum())} points")
    assert err <= 2 * REF_ERR[name]


def test_track_params_layout(tmp_path):
    ct = abi.TrackParams
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "vilfusion.h"', "int main(void) {", '  printf("%zu\\n", sizeof(vilf_track_params));']
    want = [C.sizeof(ct)]
    for fname, _ in ct._fields_:
        prog.append(f'  printf("%zu\\n", offsetof(vilf_track_params, {fname}));')
        want.append(getattr(ct, fname).offset)
    prog += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(prog))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want


# ---- GPU -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver():
    from vil_fusion_amd.estimator import BackendSolver
    s = BackendSolver()
    yield s
    s.close()


def make(solver, w=W, h=H, cam=CAM0, max_cnt=200, min_dist=20):
    from vil_fusion_amd.estimator import FeatureTracker
    return FeatureTracker(solver, w, h, cam, max_cnt=max_cnt, min_dist=min_dist), tr.FeatureTracker(w, h, cam, max_cnt=max_cnt, min_dist=min_dist)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(185, 93), (23, 22), (64, 64), (1226, 370)])
def test_pyramid_levels(solver, w, h):
    img = tr.render(tr.texture(5), w, h)
    t, ref = make(solver, w, h)
    for level in range(len(tr.level_sizes(w, h))):
        same(t.pyramid(img, level), ref.pyramid(img, level), f"level {level}")
    with pytest.raises(Exception):
        t.pyramid(img, len(tr.level_sizes(w, h)))


@pytest.mark.gpu
def test_pyramid_row_stride(solver):
    wide = tr.render(tr.texture(5), W + 19, H)
    t, ref = make(solver)
    view = wide[:, 3:3 + W]
    assert view.strides[0] > W
    for level in range(3):
        same(t.pyramid(view, level), ref.pyramid(np.ascontiguousarray(view), level), f"level {level}")


@pytest.fixture(scope="module")
def lk_reference(images):
    """the restatement for 1000 points of every kind on the 3 px pair; points are independent, so a prefix of the points has the prefix of the results"""
    pts = many_points(1000)
    out, st = tr.lk(images["flat"], images["3px_flat"], pts)
    return pts, out, st


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 200, 1000])
def test_lk_counts(solver, images, lk_reference, n):
    pts, out, st = lk_reference
    t, _ = make(solver)
    got, gst = t.lk(images["flat"], images["3px_flat"], pts[:n])
    same(gst, st[:n], "status")
    same(got, out[:n], "points")
    if n >= 63:
        assert st[:n].sum() * 2 >= n and (st[:n] == 0).any()          # the flat patch and the corners fail, most points do not


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sub", "12px"])
def test_lk_motions(solver, images, name):
    pts = many_points(200, seed=4)
    t, ref = make(solver)
    out, st = ref.lk(images["flat"], images[name + "_flat"], pts)
    got, gst = t.lk(images["flat"], images[name + "_flat"], pts)
    same(gst, st, "status")
    same(got, out, "points")
    assert st.sum() * 2 >= len(st)
    flat = (pts[:, 0] > FLAT[0] + 12) & (pts[:, 0] < FLAT[2] - 12) & (pts[:, 1] > FLAT[1] + 12) & (pts[:, 1] < FLAT[3] - 12)
    assert flat.sum() >= 8 and not st[flat].any()                      # no texture: the eigenvalue gate


@pytest.mark.gpu
def test_lk_motion_leaves_the_image(solver, images):
    # the scene moves by (+10.5, -5.8): points at the right and upper rims leave; points far outside start out of bounds
    pts = np.float32([[W - 2.0, 40.0], [W - 1.0, 2.0], [100.0, 1.5], [W + 30.0, 40.0], [-40.0, -40.0], [50.0, H + 25.0], [1.0e9, 5.0], [np.nan, 5.0], [60.0, 50.0], [70.0, 40.0]])
    t, ref = make(solver)
    out, st = ref.lk(images["base"], images["12px"], pts)
    got, gst = t.lk(images["base"], images["12px"], pts)
    same(gst, st, "status")
    same(got, out, "points")
    assert not st[3:8].any() and st[8:].all()


@pytest.mark.gpu
def test_lk_single_level(solver, images):
    pts = np.float32([[11.0, 11.0], [8.5, 12.25], [14.0, 9.0], [0.0, 0.0], [22.0, 21.0], [11.5, 3.0], [4.0, 16.0], [17.0, 17.0]])
    t, ref = make(solver, 23, 22)
    out, st = ref.lk(images["small0"], images["small1"], pts)
    got, gst = t.lk(images["small0"], images["small1"], pts)
    same(gst, st, "status")
    same(got, out, "points")
    assert st.sum() * 2 >= len(st)


def check_corners(c, kept, md):
    c = c.astype(np.int64)
    for i in range(len(c)):
        assert (((c[i] - c[:i]) ** 2).sum(axis=1) >= md * md).all()
        if len(kept):
            assert (((c[i] - tr.pixel(kept)) ** 2).sum(axis=1) > md * md).all()


@pytest.mark.gpu
@pytest.mark.parametrize("md", [20, 5])
def test_detect(solver, images, md):
    img = images["base"]
    t, ref = make(solver, min_dist=md)
    none = np.zeros((0, 2), dtype=np.float32)
    kept = np.float32([[2.0, 3.0], [W - 2.0, H - 3.0], [60.4, 40.5], [-3.0, 50.0], [100.0, H + 4.0], [130.0, 20.0]])      # discs that cross the border
    total = len(ref.detect(img, none, 1000))
    assert total >= 10
    for kp, n_max in ((none, 1000), (none, total - 3), (none, 1), (kept, 1000), (kept, 4), (kept, 1)):
        want = ref.detect(img, kp, n_max)
        got = t.detect(img, kp, n_max)
        same(got, want, f"{len(kp)} kept, n_max {n_max}")
        assert len(want) == min(n_max, len(ref.detect(img, kp, 1000))) and len(want) >= 1
        check_corners(got, kp, md)


@pytest.mark.gpu
def test_detect_flat_and_ties(solver, images):
    t, ref = make(solver, min_dist=7)
    none = np.zeros((0, 2), dtype=np.float32)
    assert len(t.detect(np.full((H, W), 93, dtype=np.uint8), none, 50)) == 0
    # a mirror image: the pixels (x, y) and (W - 1 - x, y) have the same lambda, so every accepted corner has a twin of equal score; the lower index goes first
    img = images["base"].copy()
    img[:, W // 2:] = img[:, :W // 2 + 1][:, ::-1]
    lam = tr.eigen_map(img)
    assert np.array_equal(lam, lam[:, ::-1])
    want = ref.detect(img, none, 40)
    px = want.astype(np.int64)
    score, index = lam[px[:, 1], px[:, 0]], px[:, 1] * W + px[:, 0]
    tie = np.flatnonzero(score[:-1] == score[1:])
    assert len(want) == 40 and len(tie) >= 3 and (index[tie] < index[tie + 1]).all()
    same(t.detect(img, none, 40), want, "ties")
    # a texture of period 3: the same lambda > 0 at every inner pixel, every one of them a candidate (more than W * H / 4)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    img3 = (40 + 50 * ((xx % 3 == 0) & (yy % 3 == 0)) + 90 * ((xx % 3 == 1) & (yy % 3 == 2))).astype(np.uint8)
    lam3 = tr.eigen_map(img3)
    assert lam3[2, 2] > 0 and (lam3[2:-2, 2:-2] == lam3[2, 2]).all()
    same(t.detect(img3, none, 30), ref.detect(img3, none, 30), "plateau")


def sequence_images(w, h, n, seed=7):
    tex = tr.texture(seed)
    return [tr.render(tex, w, h, shift=(1.3 * k, -0.7 * k), affine=[[1.0, 0.004 * k], [-0.003 * k, 1.0]]) for k in range(n)]


def compare_state(t, ref, what):
    same(t.ids, ref.ids, what + " ids")
    same(t.track_cnt, ref.track_cnt, what + " track_cnt")
    same(t.cur_pts, ref.cur_pts, what + " cur_pts")
    same(t.cur_un_pts, ref.cur_un_pts, what + " cur_un_pts")
    same(t.pts_velocity, ref.pts_velocity, what + " pts_velocity")
    assert t.feature_message() == ref.feature_message(), what


@pytest.mark.gpu
@pytest.mark.parametrize("cam", [CAM0, CAM1], ids=["pinhole", "distorted"])
@pytest.mark.parametrize("max_cnt", [8, 200])
def test_six_frame_sequence(solver, cam, max_cnt):
    t, ref = make(solver, cam=cam, max_cnt=max_cnt)
    seen, prev_ids, full, refill = set(), np.zeros(0, dtype=np.int32), 0, 0
    for k, img in enumerate(sequence_images(W, H, 6)):
        stamp = 100.0 + 0.05 * k + 0.001 * (k % 2)
        assert t.readImage(img, stamp) == ref.readImage(img, stamp)
        compare_state(t, ref, f"frame {k}")
        ids = t.ids
        assert len(ids) <= max_cnt and len(set(ids.tolist())) == len(ids)
        new = np.array([i not in seen for i in ids.tolist()], dtype=bool)
        assert (np.diff(ids[new]) > 0).all() and (not new.any() or not seen or ids[new].min() > max(seen))      # new ids ascend, behind every older id
        assert not t.pts_velocity[new].any() and (k > 0 or new.all())
        assert set(ids[~new].tolist()) <= set(prev_ids.tolist()) and (t.track_cnt[~new] > 1).all() and (t.track_cnt[new] == 1).all()
        if k > 0:
            assert (~new).sum() >= 4 and t.pts_velocity[~new].any()                       # ids persist across frames and move
            full += int((~new).sum() == max_cnt)
            refill += int(new.any())
        seen |= set(ids.tolist())
        prev_ids = ids.copy()
    assert (full > 0) if max_cnt == 8 else (refill > 0)


@pytest.mark.gpu
def test_handle_life(solver):
    from vil_fusion_amd.estimator import FeatureTracker, FeatureExtraction
    from vil_fusion_amd.lib import VilfError
    L, h = solver._L, solver._h
    imgs = sequence_images(W, H, 3)
    t, ref = make(solver)
    for k in range(2):
        t.readImage(imgs[k], 0.1 * k)
        ref.readImage(imgs[k], 0.1 * k)
    # refused parameters leave the tracker as it was
    for bad in (dict(width=21), dict(height=21), dict(max_cnt=0), dict(max_cnt=abi.VILF_MAX_FEATURES + 1), dict(min_dist=0), dict(fx=0.0), dict(fy=-1.0)):
        p = abi.TrackParams(W, H, 200, 20, *CAM0)
        for name, v in bad.items():
            setattr(p, name, v)
        assert L.vilf_track_init(h, C.byref(p)) == abi.VILF_ERR_INVALID_ARGUMENT, bad
    # a too small cap writes nothing
    n = C.c_int(-7)
    ids = np.full(4, -5, dtype=np.int32)
    assert len(t.ids) > 4
    assert L.vilf_track_get(h, 4, ids.ctypes.data_as(C.POINTER(C.c_int)), None, None, None, None, C.byref(n)) == abi.VILF_ERR_INVALID_ARGUMENT
    assert n.value == -7 and (ids == -5).all()
    assert L.vilf_track_read_image(h, imgs[2].ctypes.data_as(C.POINTER(C.c_uint8)), W - 1, 0.2, C.byref(n)) == abi.VILF_ERR_INVALID_ARGUMENT and n.value == -7
    with pytest.raises(VilfError):
        t.pyramid(imgs[2], 3)
    # ... and the next frame still agrees with the restatement
    assert t.readImage(imgs[2], 0.2) == ref.readImage(imgs[2], 0.2)
    compare_state(t, ref, "after the refused calls")
    # reset: a fresh tracker
    t.reset()
    first = tr.FeatureTracker(W, H, CAM0)
    assert t.readImage(imgs[2], 5.0) == first.readImage(imgs[2], 5.0)
    compare_state(t, first, "after reset")
    assert t.ids[0] == 0 and not t.pts_velocity.any()
    # another size on the same handle
    t2, ref2 = make(solver, 64, 64, max_cnt=30, min_dist=9)
    for k, img in enumerate(sequence_images(64, 64, 2, seed=9)):
        assert t2.readImage(img, 1.0 + k) == ref2.readImage(img, 1.0 + k)
        compare_state(t2, ref2, f"64 x 64 frame {k}")
    # an older entry point on the same handle
    rng = np.random.default_rng(1)
    d = rng.uniform(4.0, 6.0, 4000)
    uv = rng.uniform(-0.4, 0.4, (4000, 2))
    cloud = np.concatenate([uv * d[:, None], d[:, None], np.zeros((4000, 1))], axis=1).astype(np.float32)
    depth = FeatureExtraction(solver).getFeatureDepth(cloud, np.float32([[0.0, 0.0, 1.0], [0.1, -0.1, 1.0]]))
    assert depth.shape == (2,) and (depth > 3.9).all() and (depth < 6.1).all()


@pytest.mark.gpu
def test_full_size_frame_pair(solver):
    w, h = 1226, 370
    tex = tr.texture(21, n_waves=40, min_period=8.0, max_period=120.0)
    imgs = [tr.render(tex, w, h), tr.render(tex, w, h, shift=(3.7, -1.4))]
    cam = (718.856, 718.856, 607.19, 185.22, -0.05, 0.01, 1.0e-4, -2.0e-4)
    t, ref = make(solver, w, h, cam=cam)
    solver.set_profiling(True)
    try:
        for k, img in enumerate(imgs):
            assert t.readImage(img, 0.1 * k) == ref.readImage(img, 0.1 * k)
            compare_state(t, ref, f"frame {k}")
            print(f"1226 x 370, frame {k}: {len(t.ids)} points; stage ms " + ", ".join(f"{name} {ms:.3f}" for name, (ms, _) in t.profile().items()))
    finally:
        solver.set_profiling(False)
    assert len(t.ids) == 200 and (t.track_cnt > 1).sum() >= 100
