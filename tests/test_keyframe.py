"""The first stage of the visual loop closure on the device (vilf_kf_*, estimator.KeyFrameStore) against tests/kf_reference.py, the numpy restatement of the
contract in include/vilfusion.h. No tolerance anywhere: every comparison is on integers or float bits. The restatement itself is measured in
tests/test_keyframe_reference.py."""
import ctypes as C
import numpy as np
import pytest
import track_reference as tr
import kf_reference as kr
from vil_fusion_amd import abi

pytestmark = pytest.mark.gpu
SIZES = [(64, 48), (70, 50), (22, 23), (41, 25)]          # 32 x 8 tiles: whole ones, a ragged edge, narrower than two tiles, straddling a tile in both directions
QW, QH = 160, 120
QCAM = (150.0, 149.0, 80.3, 60.1, -0.05, 0.01, 1.0e-4, -2.0e-4)
CAM0 = (61.6, 60.3, 31.0, 24.1, 0.0, 0.0, 0.0, 0.0)
CH = abi.VILF_KF_MATCH_CHUNK
NMAX = abi.VILF_MAX_FEATURES
PATTERN = kr.read_pattern()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(bits(got), bits(want)), (what, np.flatnonzero((bits(got) != bits(want)).reshape(len(got), -1).any(axis=1))[:8])


@pytest.fixture(scope="module")
def solver():
    from vil_fusion_amd.estimator import BackendSolver
    s = BackendSolver()
    yield s
    s.close()


def make(solver, w, h, cam, pattern=PATTERN, cap_keyframes=8, cap_keypoints=4096, **over):
    from vil_fusion_amd.estimator import KeyFrameStore
    return KeyFrameStore(solver, w, h, cam, pattern, cap_keyframes=cap_keyframes, cap_keypoints=cap_keypoints, **over), \
        kr.KeyFrameStore(w, h, cam, pattern, cap_keyframes=cap_keyframes, cap_keypoints=cap_keypoints, **over)


def images(w, h):
    """a texture, uniform noise, a constant, and 255 / 0 patches that touch all four borders"""
    patches = np.full((h, w), 128, dtype=np.uint8)
    patches[0:h // 3, 0:w // 4] = 255
    patches[0:5, w // 2:w] = 0
    patches[h - 6:h, 0:w // 2] = 0
    patches[h // 2:h, w - 7:w] = 255
    patches[h // 2 - 2:h // 2 + 3, w // 2 - 2:w // 2 + 3] = 255          # flat patches score in plateaus: the 3 x 3 rule removes them all
    patches[h // 2, 3], patches[h // 2 - 1, w - 4], patches[4, 4], patches[h // 2 + 2, 2] = 255, 0, 0, 255      # single pixels in the first and last tested column, and one outside
    return {"texture": tr.render(tr.texture(13, min_period=5.0, max_period=40.0), w, h), "noise": np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w), dtype=np.uint8),
            "constant": np.full((h, w), 93, dtype=np.uint8), "patches": patches}


def compare_frame(got, want, what):
    for k in ("keypoints", "keypoints_norm", "descriptors", "window_uv", "window_descriptors"):
        same(got[k], want[k], f"{what} {k}")


def compare_match(got, want, what):
    for k in ("status", "pt_old", "pt_old_norm", "best_index", "best_dist", "n_matched"):
        same(got[k], want[k], f"{what} {k}")


# ---- blur and FAST ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
def test_blur_and_fast_sizes(solver, w, h):
    t, ref = make(solver, w, h, CAM0)
    for name, img in images(w, h).items():
        same(t.blur(img), ref.blur(img), f"{name} blur")
        pts, sc = t.fast(img)
        rpts, rsc = ref.fast(img)
        print(f"{w} x {h} {name}: {len(rpts)} key points")
        same(pts, rpts, f"{name} key points and their order")
        same(sc, rsc, f"{name} scores")
    wide = np.random.default_rng(3).integers(0, 256, (h, w + 13), dtype=np.uint8)
    view = wide[:, 5:5 + w]
    assert view.strides[0] > w
    same(t.blur(view), ref.blur(np.ascontiguousarray(view)), "row stride blur")
    same(t.fast(view)[0], ref.fast(np.ascontiguousarray(view))[0], "row stride key points")
    assert len(ref.fast(images(w, h)["noise"])[0]) > 0 and len(ref.fast(images(w, h)["constant"])[0]) == 0


def test_fast_threshold_parameter(solver):
    img = images(70, 50)["noise"]
    for thr in (1, 60, 254):
        t, ref = make(solver, 70, 50, CAM0, fast_threshold=thr)
        same(t.fast(img)[0], ref.fast(img)[0], f"threshold {thr}")
        same(t.fast(img)[1], ref.fast(img)[1], f"threshold {thr} scores")


def test_fast_over_cap_writes_nothing(solver):
    from vil_fusion_amd.lib import VilfError
    t, ref = make(solver, 64, 48, CAM0)
    img = images(64, 48)["noise"]
    n_ref = len(ref.fast(img)[0])
    assert n_ref > 32
    with pytest.raises(VilfError):
        t.fast(img, cap=32)
    pts, sc, n = np.full((32, 2), -7.0, dtype=np.float32), np.full(32, 201, dtype=np.uint8), C.c_int(-5)
    rc = solver._L.vilf_kf_fast(solver._h, t._u8(img), 64, 32, t._fp(pts), t._u8(sc), C.byref(n))
    assert rc == abi.VILF_ERR_INVALID_ARGUMENT and n.value == -5 and (pts == -7.0).all() and (sc == 201).all()
    same(t.fast(img, cap=n_ref)[0], ref.fast(img)[0], "cap == n")                # the exact capacity is enough


# ---- descriptors -----------------------------------------------------------------------------------------------------------------
def test_descriptors_at_the_edges(solver):
    w, h = 64, 48
    t, ref = make(solver, w, h, CAM0)
    special = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (-0.5, -0.5), (w - 1 + 0.7, 10.2), (-0.99, 20.0), (30.0, -1.0), (-30.0, 70.0), (31.5, 23.5)]
    for r in (23, 24, 25):                               # the pattern reaches 24 pixels
        special += [(r, 24), (w - 1 - r, 24), (32, r), (32, h - 1 - r), (r, r), (w - 1 - r, h - 1 - r), (r + 0.999, h - 1 - r - 0.999)]
    rng = np.random.default_rng(11)
    pool = np.concatenate([np.array(special, dtype=np.float32), rng.uniform(-6.0, 70.0, (65, 2)).astype(np.float32)])
    for name, img in images(w, h).items():
        if name == "constant":
            assert not t.brief(img, pool).any()         # nothing is < itself
            continue
        want = ref.brief(img, pool)
        assert want.any(axis=1).sum() > len(pool) // 2
        same(t.brief(img, pool), want, f"{name} all")
        for n in (1, 63, 64, 65):                        # the edges of a workgroup of four waves and of a wave's worth of points
            same(t.brief(img, pool[:n]), want[:n], f"{name} {n} points")
            same(t.brief(img, pool[-n:]), want[-n:], f"{name} last {n} points")
    assert t.brief(images(w, h)["noise"], np.zeros((0, 2), dtype=np.float32)).shape == (0, 4)


# ---- a key frame from an image -----------------------------------------------------------------------------------------------------
def test_keyframe_from_image(solver):
    t, ref = make(solver, QW, QH, QCAM)
    tex = tr.texture(21, n_waves=40, min_period=4.0, max_period=30.0)
    rng = np.random.default_rng(12)
    windows = [np.zeros((0, 2), dtype=np.float32), np.array([[80.25, 60.75]], dtype=np.float32), rng.uniform(-5.0, 165.0, (300, 2)).astype(np.float32)]
    for k, w in enumerate(windows):
        img = tr.render(tex, QW, QH, shift=(2.0 * k, 1.0 * k))
        got, want = t.add_keyframe(img, w), ref.add_keyframe(img, w)
        assert got == want and got[1] > 50, (got, want)
    assert len(t) == len(ref) == 3
    for k in range(3):
        compare_frame(t.get(k), ref.get(k), f"key frame {k}")
    assert np.any(bits(t.get(0)["keypoints_norm"]) != bits(tr.undistort(t.get(0)["keypoints"], QCAM[:4] + (0, 0, 0, 0))))       # the distortion acts
    # a strided image gives the same key frame
    wide = np.zeros((QH, QW + 9), dtype=np.uint8)
    wide[:, 4:4 + QW] = tr.render(tex, QW, QH)
    assert t.add_keyframe(wide[:, 4:4 + QW], windows[1])[1] == ref.get(0)["keypoints"].shape[0]
    same(t.get(3)["descriptors"], ref.get(0)["descriptors"], "row stride")


# ---- the search, on crafted descriptors ------------------------------------------------------------------------------------------------
def rand_desc(rng, n):
    return rng.integers(0, 1 << 63, (n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (n, 4), dtype=np.uint64)


def flip(d, nbits, rng):
    """d with nbits random positions flipped: at distance exactly nbits"""
    d = np.array(d, dtype=np.uint64)
    for i in rng.permutation(256)[:nbits]:
        d[i // 64] ^= np.uint64(1) << np.uint64(int(i) % 64)
    return d


def far_from(d, n, rng):
    """n descriptors at distance >= 200 from d"""
    return np.stack([flip(~np.asarray(d, dtype=np.uint64), int(rng.integers(0, 57)), rng) for _ in range(n)]).reshape(n, 4)


@pytest.fixture(scope="module")
def crafted(solver):
    """ten key frames through add_loaded. Old ones F0 .. F5 with 0, 1, CH - 1, CH, CH + 1, 3 CH + 7 descriptors, their special entries placed against window
    descriptors 0 .. 3; current ones C1, C64, C65, C1000 (indices 6 .. 9) whose window descriptors are the first 1, 64, 65, VILF_MAX_FEATURES rows of one array."""
    rng = np.random.default_rng(13)
    W = rand_desc(rng, NMAX)
    ones = np.uint64(0xFFFFFFFFFFFFFFFF)
    W[:NMAX // 2, 3], W[NMAX // 2:, 3] = ones << np.uint64(6), 0      # against F5 (last word all ones): the first half 6 + Binomial(192, 1 / 2) away, whose minimum over F5 straddles the 80 of a match; the second half about 160: no index
    uv = rng.uniform(0.0, 100.0, (NMAX, 2)).astype(np.float32)
    w0 = W[0]
    olds = [np.zeros((0, 4), dtype=np.uint64),
            flip(w0, 79, rng).reshape(1, 4),                                                       # F1: exactly 79 -> a match
            np.concatenate([far_from(w0, CH - 2, rng), flip(w0, 80, rng).reshape(1, 4)]),          # F2: exactly 80 at the last index of a short chunk -> an index, no match
            far_from(w0, CH, rng), far_from(w0, CH + 1, rng), rand_desc(rng, 3 * CH + 7)]
    olds[3][64] = flip(w0, 127, rng)                     # F3: exactly 127 at the first entry of wave 1 -> an index, no match
    olds[4][CH] = flip(w0, 128, rng)                     # F4: exactly 128, alone in the second chunk -> no index
    olds[5][:, 3] = ones
    f5, m5 = olds[5], 3 * CH + 7                         # F5: random ones (ties of the minimum occur), and duplicates of a best
    d0, d1, d2, d3 = (flip(W[k], 10, rng) for k in range(4))
    f5[0], f5[m5 - 1] = d0, d0                           # the lowest and the highest index
    f5[70], f5[130], f5[CH + 3] = d1, d1, d1             # waves 1 and 2 of the first chunk, wave 0 of the second
    f5[2 * CH + 200], f5[3 * CH + 6] = d2, d2            # wave 3 of the third chunk, the ragged fourth
    f5[CH + 100], f5[200] = d3, d3                       # the lower index sits in the higher wave
    t, ref = make(solver, 64, 48, CAM0, cap_keyframes=10, cap_keypoints=8 * CH + 600)
    frames = [(o, np.zeros((0, 4), dtype=np.uint64), uv[:0]) for o in olds]
    for n in (1, 64, 65, NMAX):                          # a current key frame has key points of its own: it may be its own candidate
        own = rand_desc(rng, 100)
        own[37] = flip(W[min(n, 5) - 1], 3, rng)
        frames.append((own, W[:n], uv[:n]))
    for kd, wd, wuv in frames:
        kp = rng.uniform(0.0, 60.0, (len(kd), 2)).astype(np.float32)
        kn = rng.uniform(-1.0, 1.0, (len(kd), 2)).astype(np.float32)
        assert t.add_loaded(kp, kn, kd, wuv, wd) == ref.add_loaded(kp, kn, kd, wuv, wd)
    return t, ref


def test_loaded_keyframes_come_back(crafted):
    t, ref = crafted
    assert len(t) == len(ref) == 10
    for k in range(10):
        compare_frame(t.get(k), ref.get(k), f"key frame {k}")


@pytest.mark.parametrize("cur,n", [(6, 1), (7, 64), (8, 65), (9, NMAX)])
def test_match_crafted(crafted, cur, n):
    t, ref = crafted
    assert len(ref.get(cur)["window_descriptors"]) == n
    for olds in ([5], [0, 1, 2, 3, 4], [5, 5, cur, 0, 3]):
        got, want = t.searchByBRIEFDes(cur, olds), ref.searchByBRIEFDes(cur, olds)
        compare_match(got, want, f"cur {cur} olds {olds}")
    # what the inputs were built for, stated on the restatement's result (window point 0 against F0 .. F4, the duplicates in F5)
    r = ref.searchByBRIEFDes(cur, [0, 1, 2, 3, 4, 5])
    assert [(int(r["status"][k, 0]), int(r["best_index"][k, 0]), int(r["best_dist"][k, 0])) for k in range(5)] == \
        [(0, -1, 128), (1, 0, 79), (0, CH - 2, 80), (0, 64, 127), (0, -1, 128)]
    want5 = [(0, 10), (70, 10), (2 * CH + 200, 10), (200, 10)][:min(n, 4)]
    assert [(int(r["best_index"][5, i]), int(r["best_dist"][5, i])) for i in range(len(want5))] == want5
    if n == NMAX:
        assert (r["best_index"][5] == -1).sum() > 100 and (r["best_index"][5] >= 0).sum() > 100 and 50 < r["n_matched"][5] < NMAX // 2 - 50
    own = ref.searchByBRIEFDes(cur, [cur])
    assert (int(own["best_index"][0, min(n, 5) - 1]), int(own["best_dist"][0, min(n, 5) - 1])) == (37, 3)


def test_match_thresholds_are_parameters(solver):
    rng = np.random.default_rng(14)
    t, ref = make(solver, 64, 48, CAM0, match_max_dist=100, match_accept_dist=101)
    W = rand_desc(rng, 3)
    old = np.stack([flip(W[0], 99, rng), flip(W[1], 100, rng), flip(W[2], 30, rng)])
    for s in (t, ref):
        s.add_loaded(np.ones((3, 2)), np.ones((3, 2)), old, np.zeros((3, 2)), W)
    got, want = t.searchByBRIEFDes(0, [0]), ref.searchByBRIEFDes(0, [0])
    compare_match(got, want, "thresholds")
    assert want["best_index"][0].tolist() == [0, -1, 2] and want["best_dist"][0].tolist() == [99, 100, 30] and want["status"][0].tolist() == [1, 0, 1]


# ---- the search, on images -----------------------------------------------------------------------------------------------------------
def test_match_natural(solver):
    img0, img1, w = kr.natural_pair()
    t, ref = make(solver, kr.NAT_W, kr.NAT_H, QCAM)
    for s in (t, ref):
        s.add_keyframe(img0, np.zeros((0, 2), dtype=np.float32))
        s.add_keyframe(img1, w)
    for k in range(2):
        compare_frame(t.get(k), ref.get(k), f"key frame {k}")
    want = ref.searchByBRIEFDes(1, [0])
    assert int(want["n_matched"][0]) >= 26              # a condition on the input (MIN_LOOP_NUM + 1), not on the kernel
    compare_match(t.searchByBRIEFDes(1, [0]), want, "natural")
    compare_match(t.searchByBRIEFDes(1, [0, 1]), ref.searchByBRIEFDes(1, [0, 1]), "natural, two candidates")
    same(t.searchByBRIEFDes(0, [1])["status"], np.zeros((1, 0), dtype=np.uint8), "no window points")


# ---- the store -------------------------------------------------------------------------------------------------------------------------
def test_capacity_exhaustion_leaves_the_store_alone(solver):
    from vil_fusion_amd.lib import VilfError
    tex = tr.texture(21, n_waves=40, min_period=4.0, max_period=30.0)
    img0, img1 = tr.render(tex, QW, QH), tr.render(tex, QW, QH, shift=(5.0, 2.0))
    n0, n1 = len(kr.fast(img0)[0]), len(kr.fast(img1)[0])
    assert n0 > 50 and n1 > 10
    w = np.random.default_rng(15).uniform(0.0, 120.0, (7, 2)).astype(np.float32)
    t, ref = make(solver, QW, QH, QCAM, cap_keyframes=3, cap_keypoints=n0 + n1 - 1)
    assert t.add_keyframe(img0, w) == ref.add_keyframe(img0, w) == (0, n0)
    before = t.get(0)
    with pytest.raises(VilfError):                       # one key point too many: never truncated
        t.add_keyframe(img1, w)
    with pytest.raises(VilfError):
        t.add_loaded(np.zeros((n1, 2)), np.zeros((n1, 2)), np.zeros((n1, 4), dtype=np.uint64), w[:0], np.zeros((0, 4), dtype=np.uint64))
    assert len(t) == 1
    compare_frame(t.get(0), before, "after the refused key frames")
    small = (np.ones((n1 - 1, 2), dtype=np.float32), np.ones((n1 - 1, 2), dtype=np.float32), np.full((n1 - 1, 4), 5, dtype=np.uint64), w, np.full((7, 4), 9, dtype=np.uint64))
    assert t.add_loaded(*small) == ref.add_loaded(*small) == 1          # exactly the free key points
    img2 = np.full((QH, QW), 50, dtype=np.uint8)                         # no key points: it needs a free key frame only
    assert t.add_keyframe(img2, w) == ref.add_keyframe(img2, w) == (2, 0)
    with pytest.raises(VilfError):                       # no free key frame
        t.add_keyframe(img2, w)
    with pytest.raises(VilfError):
        t.add_loaded(np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0, 4), dtype=np.uint64), w[:0], np.zeros((0, 4), dtype=np.uint64))
    assert len(t) == 3
    for k in range(3):
        compare_frame(t.get(k), ref.get(k), f"key frame {k}")
    compare_match(t.searchByBRIEFDes(2, [0, 1, 2]), ref.searchByBRIEFDes(2, [0, 1, 2]), "after the refused key frames")


def test_two_stores_on_two_handles(solver):
    from vil_fusion_amd.estimator import BackendSolver
    other = BackendSolver()
    try:
        rng = np.random.default_rng(16)
        pat2 = tuple(rng.integers(-64, 65, 256) for _ in range(4))                 # another pattern, to the limit of its range
        a, ra = make(solver, 70, 50, QCAM)
        b, rb = make(other, 64, 48, CAM0, pattern=pat2, fast_threshold=35)
        ia, ib = images(70, 50), images(64, 48)
        wa, wb = rng.uniform(0, 50, (20, 2)).astype(np.float32), rng.uniform(0, 48, (33, 2)).astype(np.float32)
        for name in ("texture", "noise", "patches"):
            assert a.add_keyframe(ia[name], wa) == ra.add_keyframe(ia[name], wa)
            assert b.add_keyframe(ib[name], wb) == rb.add_keyframe(ib[name], wb)
        for k in range(3):
            compare_frame(a.get(k), ra.get(k), f"first store, key frame {k}")
            compare_frame(b.get(k), rb.get(k), f"second store, key frame {k}")
        compare_match(a.searchByBRIEFDes(1, [0, 2]), ra.searchByBRIEFDes(1, [0, 2]), "first store")
        compare_match(b.searchByBRIEFDes(1, [0, 2]), rb.searchByBRIEFDes(1, [0, 2]), "second store")
    finally:
        other.close()


def test_profile(solver):
    t, _ = make(solver, QW, QH, QCAM)
    img0, img1, w = kr.natural_pair()
    solver.set_profiling(True)
    try:
        t.add_keyframe(img0, w[:3])
        t.add_keyframe(img1, w)
        t.searchByBRIEFDes(1, [0, 1])
        prof = t.profile()
    finally:
        solver.set_profiling(False)
    print(prof)
    assert list(prof) == ["upload_blur", "fast", "brief_lift", "match", "download"]
    assert all(ms >= 0.0 and cnt > 0 for ms, cnt in prof.values()), prof


# ---- invalid arguments -------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_leave_the_outputs_untouched(solver):
    from vil_fusion_amd.estimator import KeyFrameStore, kf_default_params
    from vil_fusion_amd.lib import VilfError
    L, h = solver._L, solver._h
    t, ref = make(solver, 64, 48, CAM0)
    img = images(64, 48)["texture"]
    w = np.zeros((NMAX + 1, 2), dtype=np.float32)
    fp, ip, u8p = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_uint8)
    idx, nkp = C.c_int(-5), C.c_int(-6)
    INV = abi.VILF_ERR_INVALID_ARGUMENT
    assert L.vilf_kf_add_keyframe(h, None, 64, t._fp(w), 1, C.byref(idx), C.byref(nkp)) == INV                   # a NULL image
    assert L.vilf_kf_add_keyframe(h, t._u8(img), 64, t._fp(w), NMAX + 1, C.byref(idx), C.byref(nkp)) == INV     # too many window points
    assert L.vilf_kf_add_keyframe(h, t._u8(img), 63, t._fp(w), 1, C.byref(idx), C.byref(nkp)) == INV            # a stride below the width
    bad = w[:2].copy()
    bad[1, 0] = np.nan
    assert L.vilf_kf_add_keyframe(h, t._u8(img), 64, t._fp(bad), 2, C.byref(idx), C.byref(nkp)) == INV
    assert (idx.value, nkp.value, len(t)) == (-5, -6, 0)
    out = np.full((48, 64), 77, dtype=np.uint8)
    assert L.vilf_kf_blur(h, None, 64, t._u8(out)) == INV and (out == 77).all()
    desc = np.full((2, 4), 3, dtype=np.uint64)
    assert L.vilf_kf_brief(h, t._u8(img), 64, t._fp(bad), 2, t._u64(desc)) == INV and (desc == 3).all()
    # an old index out of range, cur out of range, no candidates
    assert t.add_keyframe(img, w[:4]) == ref.add_keyframe(img, w[:4])
    st, bi, nm = np.full(8, 9, dtype=np.uint8), np.full(8, -9, dtype=np.int32), np.full(2, -9, dtype=np.int32)
    pt = np.full((8, 2), -3.0, dtype=np.float32)
    for cur, olds in ((0, [0, 1]), (0, [-1, 0]), (1, [0, 0]), (0, [])):
        o = np.array(olds + [0], dtype=np.int32)
        assert L.vilf_kf_match(h, cur, len(olds), t._ip(o), t._u8(st), t._fp(pt), t._fp(pt), t._ip(bi), t._ip(bi), t._ip(nm)) == INV, (cur, olds)
    assert (st == 9).all() and (bi == -9).all() and (nm == -9).all() and (pt == -3.0).all()
    assert L.vilf_kf_get(h, 1, 0, None, None, None, C.byref(idx), 0, None, None, None) == INV and idx.value == -5
    kp = np.full((1, 2), -3.0, dtype=np.float32)
    assert L.vilf_kf_get(h, 0, 1, t._fp(kp), None, None, C.byref(idx), 0, None, None, None) == INV and (kp == -3.0).all() and idx.value == -5      # a short capacity
    compare_frame(t.get(0), ref.get(0), "after the refused calls")
    # creation: a pattern entry of 65, a side of 21, a threshold of 0 — the existing store stays
    pat = [a.copy() for a in PATTERN]
    pat[2][255] = 65
    with pytest.raises(VilfError):
        KeyFrameStore(solver, 64, 48, CAM0, tuple(pat))
    pat[2][255] = -65
    with pytest.raises(VilfError):
        KeyFrameStore(solver, 64, 48, CAM0, tuple(pat))
    for wd, ht in ((21, 48), (64, 21)):
        with pytest.raises(VilfError):
            KeyFrameStore(solver, wd, ht, CAM0, PATTERN)
    for over in (dict(fast_threshold=0), dict(fast_threshold=255), dict(match_max_dist=258), dict(match_accept_dist=-1)):
        with pytest.raises(VilfError):
            KeyFrameStore(solver, 64, 48, CAM0, PATTERN, **over)
    with pytest.raises(VilfError):
        KeyFrameStore(solver, 64, 48, CAM0, PATTERN, cap_keyframes=0)
    assert len(t) == 1
    compare_frame(t.get(0), ref.get(0), "after the refused creations")
    KeyFrameStore(solver, 22, 22, CAM0, PATTERN)                                   # the smallest image is fine
