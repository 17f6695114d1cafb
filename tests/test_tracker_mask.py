"""The dynamic-object mask and the fisheye mask of the image feature tracker (vilf_track_read_image_mask / _configure_mask / _set_fisheye_mask / _erode / _probe /
_reject_f_mask / _detect_masked, estimator.FeatureTracker.readImage_mask) against tests/mask_reference.py, the numpy restatement of the contract's paragraphs in
include/vilfusion.h. No tolerance anywhere: integers and bits. The CPU tests measure the restatement against things that are not the restatement (scipy's binary
erosion, the labels of a two-view scene, the footprints of the moving squares); the GPU tests compare the kernels with the restatement."""
import ctypes as C
import functools
import os
import subprocess
import numpy as np
import pytest
import track_reference as tr
import mask_reference as mr
from test_tracker_frontend import FOCAL, QCAM, QH, QW, SCAM0, SCAM1, SH, SW, compare_state, moving_square_sequence, same, two_view_scene
from vil_fusion_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(64, 48), (64, 50), (70, 50), (22, 23)]
RADII = [0, 1, 5, 16]
SEQ = dict(max_cnt=60, min_dist=10)
NEW = ["vilf_track_configure_mask", "vilf_track_set_fisheye_mask", "vilf_track_read_image_mask", "vilf_track_erode", "vilf_track_probe", "vilf_track_reject_f_mask",
       "vilf_track_detect_masked", "vilf_track_profile_mask"]


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def square_masks(n=6):
    """255 everywhere but 0 over the 40 x 40 footprints of the two squares of moving_square_sequence(), frame by frame"""
    out = []
    for k in range(n):
        m = np.full((QH, QW), 255, dtype=np.uint8)
        for (x0, y0), (vx, vy) in (((20, 22), (0.5 * k, 2.0 * k)), ((104, 66), (-2.0 * k, -1.0 * k))):
            xa, ya = int(x0 + vx), int(y0 + vy)
            m[ya:ya + 40, xa:xa + 40] = 0
        out.append(m)
    return out


def fisheye_ring(w=QW, h=QH, r_in=42, r_out=54):
    """255 inside a disc, a ring of 254 around it, 0 outside"""
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    d2 = (xs - w // 2) ** 2 + (ys - h // 2) ** 2
    return np.where(d2 <= r_in * r_in, 255, np.where(d2 <= r_out * r_out, 254, 0)).astype(np.uint8)


def erode_masks(w, h):
    rng = np.random.default_rng(w * 100 + h)
    out = {"all 255": np.full((h, w), 255, dtype=np.uint8), "all 0": np.zeros((h, w), dtype=np.uint8)}
    for name, (x, y) in {"top left": (0, 0), "top right": (w - 1, 0), "bottom left": (0, h - 1), "bottom right": (w - 1, h - 1), "top edge": (w // 2, 0),
                         "bottom edge": (w // 3, h - 1), "left edge": (0, h // 2), "right edge": (w - 1, h // 3), "middle": (w // 2, h // 2)}.items():
        m = np.full((h, w), 255, dtype=np.uint8)
        m[y, x] = 0
        out["zero at " + name] = m
    sparse = np.where(rng.uniform(size=(h, w)) < 0.004, 0, 255).astype(np.uint8)
    out["sparse zeros"] = sparse
    out["values 1 and 254"] = np.where(sparse == 0, 0, rng.choice(np.array([1, 254], dtype=np.uint8), size=(h, w))).astype(np.uint8)
    return out


def static_flags(truth, m):
    """m points flagged static, the true inliers first (in list order), then the others; m = None: every point"""
    st = np.zeros(len(truth), dtype=np.uint8)
    order = np.concatenate([np.flatnonzero(truth == 1), np.flatnonzero(truth != 1)])
    st[order[:len(truth) if m is None else m]] = 1
    return st


@functools.lru_cache(maxsize=None)
def scene(n, cam, seed, noise=0.0):
    return two_view_scene(n, cam, seed, noise)


@functools.lru_cache(maxsize=None)
def reference_sequence(kind):
    """the restatement run over the moving squares, once per configuration: (tracker, [state after every frame])"""
    imgs, masks = moving_square_sequence(), square_masks()
    front = dict(equalize=True) if kind == "clahe" else {}
    ref = mr.FeatureTracker(QW, QH, QCAM, **SEQ, **front)
    calls = sequence_calls(kind)
    if kind == "r0":
        ref.configure_mask(erode_radius=0)
    if kind in ("reject off", "all 255"):
        ref.configure_mask(reject=False)
    if kind == "fisheye":
        ref.set_fisheye_mask(fisheye_ring())
    states = []
    for k, masked in enumerate(calls):
        mask = np.full((QH, QW), 255, dtype=np.uint8) if kind == "all 255" else masks[k]
        n = ref.readImage_mask(imgs[k], mask, 100.0 + 0.05 * k) if masked else ref.readImage(imgs[k], 100.0 + 0.05 * k)
        states.append((n, ref.ids.copy(), ref.track_cnt.copy(), ref.cur_pts.copy(), ref.cur_un_pts.copy(), ref.pts_velocity.copy()))
    return ref, states


def sequence_calls(kind):
    """per frame: True = the masked entry point"""
    return [True, False, True, True, False, True] if kind in ("alternating", "fisheye") else [True] * 6


# ---- CPU: what the restatement is worth ----------------------------------------------------------------------------------------
def test_erode_element_and_radius_0():
    assert mr.half_widths(5) == [5, 5, 5, 4, 3, 0]
    assert mr.half_widths(0) == [0] and mr.half_widths(1) == [1, 0]
    m = np.random.default_rng(1).integers(0, 3, (23, 22)).astype(np.uint8) * 127
    same(mr.erode(m, 0), np.where(m != 0, 255, 0).astype(np.uint8))


@pytest.mark.parametrize("r", [1, 2, 5, 8])
def test_erode_equals_scipy(r):
    from scipy import ndimage
    rng = np.random.default_rng(r)
    for p in (0.01, 0.05):
        m = np.where(rng.uniform(size=(23, 22)) < p, 0, rng.integers(1, 256, (23, 22))).astype(np.uint8)
        want = ndimage.binary_erosion(m != 0, structure=mr.element(r), border_value=1)
        same(mr.erode(m, r), np.where(want, 255, 0).astype(np.uint8), f"r = {r}")


@pytest.mark.parametrize("cam", [SCAM0, SCAM1], ids=["pinhole", "distorted"])
@pytest.mark.parametrize("noise", [0.0, 0.05])
@pytest.mark.parametrize("n", [65, 200, 1000])
def test_reject_f_mask_recovers_the_labels(n, noise, cam):
    cur, forw, truth = scene(n, cam, 5, noise)
    half = np.zeros(n, dtype=np.uint8)
    half[np.flatnonzero(truth == 1)[::2]] = 1
    for name, static in (("true labels", truth), ("every second inlier", half)):
        st, best, n_in, F = mr.reject_f_mask(cur, forw, static, cam, SW, SH, FOCAL, 0.1, 1.0, 512, 0)
        assert np.array_equal(st, truth) and 0 <= best < 512 and n_in <= static.sum() and np.isfinite(F).all(), (name, int((st != truth).sum()))


def test_reject_f_mask_seven_static_points_reject_nothing():
    cur, forw, truth = scene(200, SCAM1, 5)
    st, best, n_in, F = mr.reject_f_mask(cur, forw, static_flags(truth, 7), SCAM1, SW, SH, FOCAL, 0.1, 1.0, 512, 0)
    assert st.all() and len(st) == 200 and best == -1 and n_in == 7 and not F.any()


def test_detect_without_an_extra_mask_is_the_plain_detection():
    img = moving_square_sequence(1)[0]
    kept = np.array([[30.2, 40.7], [100.0, 20.0]], dtype=np.float32)
    same(mr.detect(img, kept, 40, 10), tr.detect(img, kept, 40, 10))
    same(mr.detect(img, kept, 40, 10, np.ones((QH, QW), dtype=bool)), tr.detect(img, kept, 40, 10))
    assert mr.set_mask(kept, np.array([2, 3]), 10) == tr.set_mask(kept, np.array([2, 3]), 10) == [1, 0]


def test_masked_sequence_by_the_restatement():
    """prototype figures per frame, as (survivors, static, rejected, rejected non-static): (58, 44, 6, 6), (60, 50, 1, 0), (60, 52, 1, 1), (60, 53, 5, 5), (57, 50, 5, 5)"""
    ref, _ = reference_sequence("r5")
    print("(survivors, static, rejected, rejected non-static) per frame:", ref.stats)
    assert len(ref.stats) == 5 and all(s[1] >= 8 for s in ref.stats)
    rejected, non_static = sum(s[2] for s in ref.stats), sum(s[3] for s in ref.stats)
    assert rejected >= 1 and 2 * non_static > rejected
    plain = mr.FeatureTracker(QW, QH, QCAM, **SEQ)
    for k, img in enumerate(moving_square_sequence()):
        plain.readImage_mask(img, np.full((QH, QW), 255, dtype=np.uint8), 100.0 + 0.05 * k)
        px = tr.pixel(ref.new_pts[k])
        assert len(px) and (ref.E_frames[k][px[:, 1], px[:, 0]] != 0).all(), k          # no new corner where E is 0
        same(ref.E_frames[k], mr.erode(square_masks()[k], 5))
    assert not np.array_equal(ref.ids, plain.ids)


def test_fisheye_ring_drops_tracked_points_and_admits_corners():
    fish = fisheye_ring()
    pts = np.array([[80.0, 60.0], [80.0 + 48.0, 60.0], [80.0, 60.0 - 30.0]], dtype=np.float32)
    assert [int(fish[int(y), int(x)]) for x, y in pts] == [255, 254, 255]
    assert mr.set_mask(pts, np.array([2, 5, 3]), 10, fish) == [2, 0] and mr.set_mask(pts, np.array([2, 5, 3]), 10) == [1, 2, 0]
    img = moving_square_sequence(1)[0]
    on_ring = mr.detect(img, np.zeros((0, 2), dtype=np.float32), 20, 10, fish == 254)
    px = tr.pixel(on_ring)
    assert len(px) >= 1 and (fish[px[:, 1], px[:, 0]] == 254).all()
    ref, _ = reference_sequence("fisheye")
    px = tr.pixel(ref.cur_pts)
    v = fish[px[:, 1], px[:, 0]]
    assert (v != 0).all() and (v[ref.track_cnt > 1] == 255).all() and (v[ref.track_cnt == 1] == 254).any()


def test_track_mask_params_layout(tmp_path):
    ct = abi.TrackMaskParams
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "vilfusion.h"', "int main(void) {", '  printf("%zu\\n", sizeof(vilf_track_mask_params));']
    want = [C.sizeof(ct)]
    for fname, _ in ct._fields_:
        prog.append(f'  printf("%zu\\n", offsetof(vilf_track_mask_params, {fname}));')
        want.append(getattr(ct, fname).offset)
    prog += ['  printf("%d\\n", VILF_TRACK_MAX_ERODE);', "  return 0;", "}"]
    want += [abi.VILF_TRACK_MAX_ERODE]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(prog))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want and mr.MAX_ERODE == abi.VILF_TRACK_MAX_ERODE == 16


def test_new_entry_points_are_exported():
    assert all(name in lib.EXPORTED for name in NEW)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver():
    from vil_fusion_amd.estimator import BackendSolver
    s = BackendSolver()
    yield s
    s.close()


def make(solver, w, h, cam, max_cnt=200, min_dist=20, **front):
    from vil_fusion_amd.estimator import FeatureTracker
    return FeatureTracker(solver, w, h, cam, max_cnt=max_cnt, min_dist=min_dist, **front), mr.FeatureTracker(w, h, cam, max_cnt=max_cnt, min_dist=min_dist, **front)


def compare_tuple(t, n, state, what):
    assert n == state[0], (what, n, state[0])
    for got, want, name in zip((t.ids, t.track_cnt, t.cur_pts, t.cur_un_pts, t.pts_velocity), state[1:], ("ids", "track_cnt", "cur_pts", "cur_un_pts", "pts_velocity")):
        same(got, want, f"{what} {name}")


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
def test_erode_sizes_radii_and_masks(solver, w, h):
    t, ref = make(solver, w, h, QCAM)
    masks = erode_masks(w, h)
    wide = np.where(np.random.default_rng(3).uniform(size=(h, w + 13)) < 0.01, 0, 255).astype(np.uint8)
    view = wide[:, 5:5 + w]
    assert view.strides[0] > w
    for r in RADII:
        t.configure_mask(erode_radius=r)
        ref.configure_mask(erode_radius=r)
        for name, m in masks.items():
            same(t.erode(m), ref.erode(m), f"r = {r}, {name}")
        same(t.erode(view), ref.erode(np.ascontiguousarray(view)), f"r = {r}, row stride")
    assert not ref.erode(masks["zero at middle"])[h // 2, w // 2] and (ref.erode(masks["all 255"]) == 255).all()


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,d", [(160, 120, 1), (160, 120, 5), (160, 140, 64), (100, 90, 64)])
def test_probe_guard_edges(solver, w, h, d):
    t, ref = make(solver, w, h, QCAM)
    t.configure_mask(probe=d)
    ref.configure_mask(probe=d)
    rng = np.random.default_rng(d)
    E = np.where(rng.uniform(size=(h, w)) < 0.2, 0, 255).astype(np.uint8)
    xs = [0, d - 1, d, d + 1, d + 2, w // 2, w - d - 2, w - d - 1, w - d, w - d + 1, w - 1]
    ys = [0, d - 1, d, d + 1, d + 2, h // 2, h - d - 2, h - d - 1, h - d, h - d + 1, h - 1]
    pts = np.array([(x, y) for x in xs for y in ys if 0 <= x < w and 0 <= y < h], dtype=np.float32)
    pts = np.concatenate([pts, pts + np.float32(0.5), pts - np.float32(0.25), rng.uniform(0, [w - 1, h - 1], (200, 2)).astype(np.float32)])
    got, want = t.probe(E, pts), ref.probe(E, pts)
    same(got, want, f"d = {d}")
    if 2 * d >= min(w, h):
        assert want.all()                                    # the guard never holds
    else:
        assert 0 < want.sum() < len(want)
    for img in (np.zeros((h, w), dtype=np.uint8), np.full((h, w), 255, dtype=np.uint8)):
        same(t.probe(img, pts), ref.probe(img, pts), f"d = {d}, constant E")


def compare_reject_mask(t, ref, cur, forw, static, what):
    st, best, n_in, F = t.reject_f_mask(cur, forw, static)
    rst, rbest, rn_in, rF = ref.reject_f_mask(cur, forw, static)
    assert (best, n_in) == (rbest, rn_in), (what, best, n_in, rbest, rn_in)
    same(st, rst, what + " status")
    same(F, rF, what + " F")
    return st, best


@pytest.mark.gpu
@pytest.mark.parametrize("n", [9, 65, 200, 1000])
def test_reject_f_mask_static_counts(solver, n):
    cur, forw, truth = scene(1000, SCAM1, 4)
    cur, forw, truth = cur[:n], forw[:n], truth[:n]
    t, ref = make(solver, SW, SH, SCAM1)
    for m in (0, 7, 8, 9, 63, 64, 65, None):
        if m is not None and m > n:
            continue
        st, best = compare_reject_mask(t, ref, cur, forw, static_flags(truth, m), f"n = {n}, static {m}")
        assert (best == -1) == (m is not None and m < 8)
        if m is not None and 63 <= m <= truth.sum():
            assert np.array_equal(st, truth)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 512, 2048])
@pytest.mark.parametrize("cam", [SCAM0, SCAM1], ids=["pinhole", "distorted"])
def test_reject_f_mask_hypothesis_counts_and_thresholds(solver, cam, K):
    cur, forw, truth = scene(200, cam, 5, 0.05)
    t, ref = make(solver, SW, SH, cam, n_hypotheses=K, seed=3)
    _, best = compare_reject_mask(t, ref, cur, forw, static_flags(truth, 65), f"K = {K}")
    assert 0 <= best < K
    for kw in (dict(f_threshold=0.5, epi_threshold=0.3), dict(f_threshold=0.02, epi_threshold=5.0)):
        t.configure_mask(**kw)
        ref.configure_mask(**kw)
        compare_reject_mask(t, ref, cur, forw, truth, f"K = {K}, {kw}")


@pytest.mark.gpu
def test_reject_f_mask_all_points_equal(solver):
    cur = scene(1000, SCAM1, 4)[0]
    t, ref = make(solver, SW, SH, SCAM1)
    same_pt = np.tile(cur[:1], (50, 1))
    st, best = compare_reject_mask(t, ref, same_pt, same_pt, np.ones(50, dtype=np.uint8), "all equal")
    assert st.all() and best == -1


@pytest.mark.gpu
@pytest.mark.parametrize("fisheye", [False, True], ids=["no fisheye", "fisheye"])
def test_detect_masked(solver, fisheye):
    img = moving_square_sequence(1)[0]
    t, ref = make(solver, QW, QH, QCAM, **SEQ)
    if fisheye:
        t.set_fisheye_mask(fisheye_ring())
        ref.set_fisheye_mask(fisheye_ring())
    kept = np.array([[30.2, 40.7], [100.0, 20.0], [81.5, 62.5]], dtype=np.float32)
    full, none = np.full((QH, QW), 255, dtype=np.uint8), np.zeros((QH, QW), dtype=np.uint8)
    plain = t.detect(img, kept, 60)
    same(plain, ref.detect(img, kept, 60), "vilf_track_detect")
    same(t.detect_masked(img, full, kept, 60), plain, "E all 255")
    px = tr.pixel(plain)
    assert len(plain) >= 10 and (not fisheye or (fisheye_ring()[px[:, 1], px[:, 0]] != 0).all())
    assert len(t.detect_masked(img, none, kept, 60)) == 0 and len(ref.detect_masked(img, none, kept, 60)) == 0
    one = none.copy()
    one[int(plain[3, 1]), int(plain[3, 0])] = 1
    got = t.detect_masked(img, one, kept, 60)
    same(got, ref.detect_masked(img, one, kept, 60), "a single allowed pixel")
    same(got, plain[3:4], "a single allowed pixel")
    ys, xs = np.meshgrid(np.arange(QH), np.arange(QW), indexing="ij")
    for name, E in (("pixel checkerboard", ((xs + ys) % 2 * 255).astype(np.uint8)), ("block checkerboard", ((xs // 8 + ys // 8) % 2 * 77).astype(np.uint8))):
        got = t.detect_masked(img, E, kept, 60)
        same(got, ref.detect_masked(img, E, kept, 60), name)
        px = tr.pixel(got)
        assert len(px) >= 5 and (E[px[:, 1], px[:, 0]] != 0).all()
    same(t.detect_masked(img, full, np.zeros((0, 2), dtype=np.float32), 7), ref.detect_masked(img, full, np.zeros((0, 2), dtype=np.float32), 7), "no kept point")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["r5", "r0", "clahe", "reject off", "alternating", "all 255", "fisheye"])
def test_masked_sequences(solver, kind):
    from vil_fusion_amd.estimator import FeatureTracker
    imgs, masks = moving_square_sequence(), square_masks()
    ref, states = reference_sequence(kind)
    t = FeatureTracker(solver, QW, QH, QCAM, **SEQ, **(dict(equalize=True) if kind == "clahe" else {}))
    if kind == "r0":
        t.configure_mask(erode_radius=0)
    if kind in ("reject off", "all 255"):
        t.configure_mask(reject=False)
    if kind == "fisheye":
        t.set_fisheye_mask(fisheye_ring())
    for k, masked in enumerate(sequence_calls(kind)):
        mask = np.full((QH, QW), 255, dtype=np.uint8) if kind == "all 255" else masks[k]
        n = t.readImage_mask(imgs[k], mask, 100.0 + 0.05 * k) if masked else t.readImage(imgs[k], 100.0 + 0.05 * k)
        compare_tuple(t, n, states[k], f"{kind}, frame {k}")
    if kind == "all 255":                                    # nothing is dynamic and nothing is rejected: the plain entry point on a second tracker
        t2 = FeatureTracker(solver, QW, QH, QCAM, **SEQ)
        for k in range(6):
            compare_tuple(t2, t2.readImage(imgs[k], 100.0 + 0.05 * k), states[k], f"readImage, frame {k}")
    if kind in ("r5", "r0"):
        assert sum(s[2] for s in ref.stats) >= 1


@pytest.mark.gpu
def test_nothing_existing_moved(solver):
    """the fisheye mask set and cleared again, the mask parameters configured: readImage is the tracker of track_reference.py"""
    imgs = moving_square_sequence()
    t, _ = make(solver, QW, QH, QCAM, **SEQ)
    ref = tr.FeatureTracker(QW, QH, QCAM, **SEQ)
    t.set_fisheye_mask(fisheye_ring())
    t.set_fisheye_mask(None)
    t.configure_mask(erode_radius=3, probe=9, reject=True, f_threshold=0.3, epi_threshold=2.0)
    for k, img in enumerate(imgs):
        assert t.readImage(img, 0.05 * k) == ref.readImage(img, 0.05 * k)
        compare_state(t, ref, f"frame {k}")
        if k == 2:
            same(t.detect(img, t.cur_pts[:5], 20), ref.detect(img, ref.cur_pts[:5], 20), "detect, fisheye mask cleared")


@pytest.mark.gpu
def test_refusals(solver):
    from vil_fusion_amd.estimator import BackendSolver
    L, h = solver._L, solver._h
    imgs, masks = moving_square_sequence(3), square_masks(3)
    t, ref = make(solver, QW, QH, QCAM, **SEQ)
    for k in range(2):
        t.readImage_mask(imgs[k], masks[k], 0.05 * k)
        ref.readImage_mask(imgs[k], masks[k], 0.05 * k)
    fp, u8p, ip = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_int)
    INV = abi.VILF_ERR_INVALID_ARGUMENT

    def unchanged(what):
        n = C.c_int(-1)
        ids = np.zeros(max(len(ref.ids), 1), dtype=np.int32)
        pts = np.zeros((max(len(ref.ids), 1), 2), dtype=np.float32)
        assert L.vilf_track_get(h, len(ids), ids.ctypes.data_as(ip), None, pts.ctypes.data_as(fp), None, None, C.byref(n)) == abi.VILF_OK
        assert n.value == len(ref.ids), what
        same(ids[:n.value], ref.ids, what)
        same(pts[:n.value], ref.cur_pts, what)

    good = dict(erode_radius=5, probe=5, reject=1, f_threshold=0.1, epi_threshold=1.0)
    for b in (dict(erode_radius=-1), dict(erode_radius=17), dict(probe=0), dict(probe=65), dict(reject=2), dict(reject=-1), dict(f_threshold=0.0), dict(f_threshold=float("nan")),
              dict(f_threshold=float("inf")), dict(epi_threshold=-1.0), dict(epi_threshold=float("inf")), dict(epi_threshold=float("nan"))):
        mp = abi.TrackMaskParams(**{**good, **b})
        assert L.vilf_track_configure_mask(h, C.byref(mp)) == INV, b
    assert L.vilf_track_configure_mask(h, None) == INV
    unchanged("configure_mask")
    img, mask = imgs[2], masks[2]
    n = C.c_int(-7)
    for a, sa, m, sm in ((None, QW, mask, QW), (img, QW, None, QW), (img, QW - 1, mask, QW), (img, QW, mask, QW - 1)):
        rc = L.vilf_track_read_image_mask(h, None if a is None else a.ctypes.data_as(u8p), sa, None if m is None else m.ctypes.data_as(u8p), sm, 0.1, C.byref(n))
        assert rc == INV and n.value == -7
    assert L.vilf_track_set_fisheye_mask(h, mask.ctypes.data_as(u8p), QW - 1) == INV
    out = np.full((QH, QW), 55, dtype=np.uint8)
    assert L.vilf_track_erode(h, mask.ctypes.data_as(u8p), QW - 1, out.ctypes.data_as(u8p)) == INV and (out == 55).all()
    assert L.vilf_track_erode(h, None, QW, out.ctypes.data_as(u8p)) == INV and L.vilf_track_erode(h, mask.ctypes.data_as(u8p), QW, None) == INV
    unchanged("read_image_mask, set_fisheye_mask, erode")
    cur, forw, _ = two_view_scene(20, QCAM, 1)
    nan_pt, inf_pt = forw.copy(), cur.copy()
    nan_pt[13, 1], inf_pt[0, 0] = np.nan, np.inf
    big = np.zeros((abi.VILF_MAX_FEATURES + 1, 2), dtype=np.float32)
    flags = np.ones(abi.VILF_MAX_FEATURES + 1, dtype=np.uint8)
    for p, cnt in ((cur, -1), (big, abi.VILF_MAX_FEATURES + 1), (nan_pt, 20), (inf_pt, 20)):
        st = np.full(len(p), 77, dtype=np.uint8)
        assert L.vilf_track_probe(h, mask.ctypes.data_as(u8p), p.ctypes.data_as(fp), cnt, st.ctypes.data_as(u8p)) == INV and (st == 77).all(), cnt
    st = np.full(20, 77, dtype=np.uint8)
    assert L.vilf_track_probe(h, None, cur.ctypes.data_as(fp), 20, st.ctypes.data_as(u8p)) == INV and (st == 77).all()
    for a, b, cnt in ((cur, forw, -1), (big, big, abi.VILF_MAX_FEATURES + 1), (cur, nan_pt, 20), (inf_pt, forw, 20)):
        st, F, best, n_in = np.full(len(a), 77, dtype=np.uint8), np.full(9, -3.5), C.c_int(-7), C.c_int(-9)
        rc = L.vilf_track_reject_f_mask(h, a.ctypes.data_as(fp), b.ctypes.data_as(fp), flags.ctypes.data_as(u8p), cnt, st.ctypes.data_as(u8p), abi.dptr(F), C.byref(best), C.byref(n_in))
        assert rc == INV and (st == 77).all() and (F == -3.5).all() and best.value == -7 and n_in.value == -9, cnt
    st, F, best, n_in = np.full(20, 77, dtype=np.uint8), np.full(9, -3.5), C.c_int(-7), C.c_int(-9)
    assert L.vilf_track_reject_f_mask(h, cur.ctypes.data_as(fp), forw.ctypes.data_as(fp), None, 20, st.ctypes.data_as(u8p), abi.dptr(F), C.byref(best), C.byref(n_in)) == INV and (st == 77).all()
    pts_out, cnt_out = np.full((5, 2), -2.0, dtype=np.float32), C.c_int(-7)
    assert L.vilf_track_detect_masked(h, img.ctypes.data_as(u8p), None, None, 0, 5, pts_out.ctypes.data_as(fp), C.byref(cnt_out)) == INV and cnt_out.value == -7 and (pts_out == -2.0).all()
    assert L.vilf_track_detect_masked(h, img.ctypes.data_as(u8p), mask.ctypes.data_as(u8p), nan_pt.ctypes.data_as(fp), 20, 5, pts_out.ctypes.data_as(fp), C.byref(cnt_out)) == INV
    assert L.vilf_track_detect_masked(h, img.ctypes.data_as(u8p), mask.ctypes.data_as(u8p), None, -1, 5, pts_out.ctypes.data_as(fp), C.byref(cnt_out)) == INV and cnt_out.value == -7
    unchanged("probe, reject_f_mask, detect_masked")
    # a handle without a tracker
    other = BackendSolver()
    try:
        mp = abi.TrackMaskParams(**good)
        ms, cnt = (C.c_double * 2)(-1.0, -1.0), (C.c_long * 2)(-1, -1)
        assert L.vilf_track_configure_mask(other._h, C.byref(mp)) == INV and L.vilf_track_set_fisheye_mask(other._h, mask.ctypes.data_as(u8p), QW) == INV
        assert L.vilf_track_read_image_mask(other._h, img.ctypes.data_as(u8p), QW, mask.ctypes.data_as(u8p), QW, 0.1, C.byref(n)) == INV and n.value == -7
        assert L.vilf_track_erode(other._h, mask.ctypes.data_as(u8p), QW, out.ctypes.data_as(u8p)) == INV and (out == 55).all()
        st = np.full(20, 77, dtype=np.uint8)
        assert L.vilf_track_probe(other._h, mask.ctypes.data_as(u8p), cur.ctypes.data_as(fp), 20, st.ctypes.data_as(u8p)) == INV and (st == 77).all()
        assert L.vilf_track_detect_masked(other._h, img.ctypes.data_as(u8p), mask.ctypes.data_as(u8p), None, 0, 5, pts_out.ctypes.data_as(fp), C.byref(cnt_out)) == INV
        assert L.vilf_track_profile_mask(other._h, ms, cnt) == abi.VILF_OK and ms[0] == 0.0 and cnt[1] == 0
    finally:
        other.close()
    # the refused calls and the stateless ones left the tracker alone: the next frame still agrees with the restatement
    same(t.erode(mask), ref.erode(mask), "between frames")
    same(t.probe(ref.erode(mask), cur), ref.probe(ref.erode(mask), cur), "between frames")
    assert t.readImage_mask(img, mask, 0.1) == ref.readImage_mask(img, mask, 0.1)
    compare_state(t, ref, "after the refused calls")
    # vilf_track_reset keeps the mask parameters and the fisheye mask, a later vilf_track_init returns to the defaults and drops the fisheye mask
    for tt in (t, ref):
        tt.configure_mask(erode_radius=2, probe=3)
        tt.set_fisheye_mask(fisheye_ring())
        tt.reset()
    for k in range(2):
        assert t.readImage_mask(imgs[k], masks[k], 0.05 * k) == ref.readImage_mask(imgs[k], masks[k], 0.05 * k)
        compare_state(t, ref, f"after a reset, frame {k}")
    t2, ref2 = make(solver, QW, QH, QCAM, **SEQ)
    for k in range(2):
        assert t2.readImage_mask(imgs[k], masks[k], 0.05 * k) == ref2.readImage_mask(imgs[k], masks[k], 0.05 * k)
        compare_state(t2, ref2, f"after a new init, frame {k}")


@pytest.mark.gpu
def test_full_size_frame_pair_under_a_mask(solver):
    w, h = SW, SH
    tex = tr.texture(21, n_waves=40, min_period=8.0, max_period=120.0)
    imgs = [tr.render(tex, w, h), tr.render(tex, w, h, shift=(3.7, -1.4))]
    mask = np.full((h, w), 255, dtype=np.uint8)
    mask[150:330, 250:520] = 0
    t, ref = make(solver, w, h, SCAM1, max_cnt=100, min_dist=30)
    solver.set_profiling(True)
    try:
        for k, img in enumerate(imgs):
            assert t.readImage_mask(img, mask, 0.1 * k) == ref.readImage_mask(img, mask, 0.1 * k)
            compare_state(t, ref, f"frame {k}")
            print(f"{w} x {h}, masked frame {k}: {len(t.ids)} points; stage ms " + ", ".join(f"{name} {ms:.3f}" for name, (ms, _) in t.profile().items()) +
                  "; front-end ms " + ", ".join(f"{name} {ms:.3f} ({cnt})" for name, (ms, cnt) in t.profile_frontend().items()) +
                  "; mask ms " + ", ".join(f"{name} {ms:.3f} ({cnt})" for name, (ms, cnt) in t.profile_mask().items()))
        assert t.profile_mask()["erode"][1] == 1 and t.profile_mask()["probe_reject"][1] == 1 and t.profile_frontend()["reject_f"][1] == 0
    finally:
        solver.set_profiling(False)
    px = tr.pixel(t.cur_pts[t.track_cnt == 1])
    assert len(t.ids) >= 50 and (t.track_cnt > 1).sum() >= 25 and (ref.last_E[px[:, 1], px[:, 0]] != 0).all()
