"""The numpy restatement of the visual loop closure's first stage (tests/kf_reference.py) measured against things that are not the restatement: scipy's
correlation for the blur, an explicit search over thresholds and arcs for the FAST score, hand-made images for the key points, np.unpackbits for the Hamming
distance, the reference's own loop for the search. Integers and bits only. The kernels are compared with the restatement in tests/test_keyframe.py."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import kf_reference as kr
from vil_fusion_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QCAM = (150.0, 149.0, 80.3, 60.1, -0.05, 0.01, 1.0e-4, -2.0e-4)


@pytest.fixture(scope="module")
def pattern():
    return kr.read_pattern()


def test_pattern_fixture(pattern):
    assert len(pattern) == 4 and all(a.shape == (256,) for a in pattern)
    reach = max(int(np.abs(a).max()) for a in pattern)
    assert reach == 24 and reach <= abi.VILF_KF_MAX_OFFSET


def test_blur_taps():
    g = np.exp(-np.arange(-4, 5) ** 2 / (2.0 * 2.0 ** 2))
    assert np.array_equal(kr.Q, np.rint(256.0 * g / g.sum()).astype(np.int64))
    assert int(kr.Q.sum()) == 256


@pytest.mark.parametrize("w,h", [(64, 48), (22, 23), (41, 25)])
def test_blur_against_scipy(w, h):
    from scipy.ndimage import correlate1d
    for img in (np.random.default_rng(w * 100 + h).integers(0, 256, (h, w), dtype=np.uint8), np.full((h, w), 93, dtype=np.uint8)):
        hp = correlate1d(img.astype(np.int64), kr.Q, axis=1, mode="mirror")
        v = correlate1d(hp, kr.Q, axis=0, mode="mirror")
        assert np.array_equal(kr.blur(img), ((v + 32768) >> 16).astype(np.uint8))
    assert np.array_equal(kr.blur(np.full((h, w), 93, dtype=np.uint8)), np.full((h, w), 93, dtype=np.uint8))
    assert np.array_equal(kr.blur(np.full((h, w), 255, dtype=np.uint8)), np.full((h, w), 255, dtype=np.uint8))


def brute_score(img):
    """for every pixel the largest t' in 0 .. 254 at which the 9-contiguous test holds, -1 if it holds at none; untested pixels -1"""
    h, w = img.shape
    I = img.astype(int)
    out = np.full((h, w), -1, dtype=int)
    for y in range(3, h - 3):
        for x in range(3, w - 3):
            ring = [I[y + dy, x + dx] for dx, dy in kr.CIRCLE]
            for t in range(254, -1, -1):
                brighter = [v > I[y, x] + t for v in ring]
                darker = [v < I[y, x] - t for v in ring]
                if any(all(f[(a + j) % 16] for j in range(9)) for f in (brighter, darker) for a in range(16)):
                    out[y, x] = t
                    break
    return out


def test_fast_score_against_brute_force():
    img = np.random.default_rng(2223).integers(0, 256, (23, 22), dtype=np.uint8)
    brute = brute_score(img)
    assert (brute >= 20).sum() >= 20 and (brute < 20).sum() >= 20          # both sides of the default threshold occur
    for t in (1, 20, 100, 254):
        assert np.array_equal(kr.fast_score(img, t), np.where(brute >= t, brute, 0).astype(np.uint8)), t


def test_keypoints_of_hand_made_images():
    h, w = 30, 33
    assert len(kr.fast(np.full((h, w), 140, dtype=np.uint8))[0]) == 0
    dot = np.full((h, w), 10, dtype=np.uint8)
    dot[12, 17] = 250
    pts, sc = kr.fast(dot)
    assert pts.dtype == np.float32 and pts.tolist() == [[17.0, 12.0]] and sc.tolist() == [239]
    plateau = dot.copy()
    plateau[12, 18] = 250
    assert kr.fast_score(plateau)[12, 17] == kr.fast_score(plateau)[12, 18] == 239
    assert len(kr.fast(plateau)[0]) == 0
    two = dot.copy()
    two[20, 5] = 200                                   # row-major order: (17, 12) before (5, 20)
    assert kr.fast(two)[0].tolist() == [[17.0, 12.0], [5.0, 20.0]]
    edge = np.full((h, w), 10, dtype=np.uint8)
    edge[2, 17] = edge[12, 2] = edge[h - 3, 9] = edge[9, w - 3] = 250      # outside 3 <= x < W - 3, 3 <= y < H - 3
    assert len(kr.fast(edge)[0]) == 0


def test_descriptor_truncation_and_layout(pattern):
    img = np.random.default_rng(5).integers(0, 256, (48, 64), dtype=np.uint8)
    b = kr.blur(img)
    x1, y1, x2, y2 = pattern
    for px, py in ((-0.5, -0.5), (30.0, 20.0), (63.7, 10.2), (0.0, 47.0)):
        d = kr.brief(b, [(px, py)], pattern)[0]
        for i in range(256):
            c = [int(np.float32(px) + np.float32(x1[i])), int(np.float32(py) + np.float32(y1[i])), int(np.float32(px) + np.float32(x2[i])), int(np.float32(py) + np.float32(y2[i]))]
            want = 0 <= c[0] < 64 and 0 <= c[1] < 48 and 0 <= c[2] < 64 and 0 <= c[3] < 48 and b[c[1], c[0]] < b[c[3], c[2]]
            assert bool((int(d[i // 64]) >> (i % 64)) & 1) == bool(want), (px, py, i)
    assert int(np.float32(-0.5) + np.float32(0.0)) == 0               # toward zero: -0.5 passes the range check


def rand_desc(rng, n):
    return rng.integers(0, 1 << 63, (n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (n, 4), dtype=np.uint64)


def flip(d, bits):
    """d with the given bit positions flipped"""
    d = np.array(d, dtype=np.uint64)
    for i in bits:
        d[i // 64] ^= np.uint64(1) << np.uint64(i % 64)
    return d


def test_hamming_against_unpackbits():
    rng = np.random.default_rng(8)
    a, b = rand_desc(rng, 50), rand_desc(rng, 50)
    want = np.unpackbits(np.bitwise_xor(a, b).view(np.uint8), axis=1).sum(axis=1)
    assert np.array_equal(kr.hamming(a, b), want)
    assert int(kr.hamming(a[0], flip(a[0], [0, 63, 64, 255]))) == 4


def test_match_rules():
    rng = np.random.default_rng(9)
    w = rand_desc(rng, 1)
    pts, nrm = np.arange(12, dtype=np.float32).reshape(6, 2) + 1, -np.arange(12, dtype=np.float32).reshape(6, 2) - 1
    far = flip(w[0], range(0, 200))
    # the tie goes to the lower index
    old = np.stack([far, flip(w[0], range(30)), flip(w[0], range(100, 130)), far, far, far])
    for fn in (kr.match, kr.match_fast):
        st, pt, ptn, bi, bd = fn(w, old, pts, nrm)
        assert (st[0], bi[0], bd[0]) == (1, 1, 30) and pt[0].tolist() == pts[1].tolist() and ptn[0].tolist() == nrm[1].tolist()
        # 79 matches, 80 does not; 127 has an index, 128 has none
        for dist, want in ((79, (1, 2, 79)), (80, (0, 2, 80)), (127, (0, 2, 127)), (128, (0, -1, 128)), (200, (0, -1, 128))):
            o = np.stack([far, far, flip(w[0], range(dist)), far, far, far])
            st, pt, ptn, bi, bd = fn(w, o, pts, nrm)
            assert (st[0], bi[0], bd[0]) == want, (dist, st[0], bi[0], bd[0])
            assert pt[0].tolist() == (pts[2].tolist() if want[0] else [0.0, 0.0])
        st, pt, ptn, bi, bd = fn(w, np.zeros((0, 4), dtype=np.uint64), pts[:0], nrm[:0])
        assert (st[0], bi[0], bd[0]) == (0, -1, 128)


def test_matrix_search_equals_the_reference_loop():
    rng = np.random.default_rng(10)
    base = rand_desc(rng, 8)
    old = np.stack([flip(base[rng.integers(8)], rng.permutation(256)[:rng.integers(0, 140)]) for _ in range(70)])
    w = np.stack([flip(base[rng.integers(8)], rng.permutation(256)[:rng.integers(0, 100)]) for _ in range(40)])
    pts, nrm = rng.random((70, 2), dtype=np.float32), rng.random((70, 2), dtype=np.float32)
    for max_dist, accept in ((128, 80), (40, 20)):
        a, b = kr.match(w, old, pts, nrm, max_dist, accept), kr.match_fast(w, old, pts, nrm, max_dist, accept)
        assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))
        assert 0 < a[0].sum() < 40
    assert (a[3] == -1).any() and (a[3] >= 0).any()


def test_natural_pair_is_a_good_input(pattern):
    """a condition on the input of the GPU test, not on any kernel: the restatement finds more than MIN_LOOP_NUM = 25 matches"""
    img0, img1, w = kr.natural_pair()
    s = kr.KeyFrameStore(kr.NAT_W, kr.NAT_H, QCAM, pattern)
    s.add_keyframe(img0, np.zeros((0, 2), dtype=np.float32))
    s.add_keyframe(img1, w)
    r = s.searchByBRIEFDes(1, [0])
    assert int(r["n_matched"][0]) >= 26
    ok = r["status"][0] == 1
    assert np.array_equal(r["pt_old"][0][ok], (w + np.array([kr.NAT_SHIFT, 0], dtype=np.float32))[ok])       # the matches are the true ones


def test_library_surface():
    """the C ABI and the Python class of the stage exist and the ctypes mirror has the C layout (no GPU is touched)"""
    from vil_fusion_amd import estimator
    names = ["vilf_kf_default_params", "vilf_kf_create", "vilf_kf_add_keyframe", "vilf_kf_add_loaded", "vilf_kf_get", "vilf_kf_size", "vilf_kf_match", "vilf_kf_blur",
             "vilf_kf_fast", "vilf_kf_brief", "vilf_kf_profile"]
    assert set(names) <= set(lib.EXPORTED)
    for m in ("add_keyframe", "add_loaded", "get", "searchByBRIEFDes", "blur", "fast", "brief", "profile"):
        assert callable(getattr(estimator.KeyFrameStore, m))
    if not os.path.exists(lib.SO_PATH):
        lib.build()
    L = C.CDLL(lib.SO_PATH)
    assert all(hasattr(L, n) for n in names)
    p = abi.KfParams()
    p.width = 7
    L.vilf_kf_default_params.argtypes = [C.POINTER(abi.KfParams)]
    L.vilf_kf_default_params.restype = None
    L.vilf_kf_default_params(C.byref(p))
    assert (p.width, p.fast_threshold, p.match_max_dist, p.match_accept_dist, p.x1[0], p.y2[255]) == (0, 20, 128, 80, 0, 0)


def test_ctypes_mirror_matches_the_c_layout(tmp_path):
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "vilfusion.h"', "int main(void) {"]
    checks = []
    for cname, ct in abi.KF_LAYOUTS.items():
        prog.append(f'  printf("%zu\\n", sizeof({cname}));')
        checks.append((cname, "sizeof", C.sizeof(ct)))
        for fname, _ in ct._fields_:
            prog.append(f'  printf("%zu\\n", offsetof({cname}, {fname}));')
            checks.append((cname, fname, getattr(ct, fname).offset))
    prog += ['  printf("%d %d %d %d\\n", VILF_KF_BITS, VILF_KF_WORDS, VILF_KF_MATCH_CHUNK, VILF_KF_MAX_CANDIDATES);', "  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(prog))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out[-4:]] == [abi.VILF_KF_BITS, abi.VILF_KF_WORDS, abi.VILF_KF_MATCH_CHUNK, abi.VILF_KF_MAX_CANDIDATES]
    bad = [(c, f, int(o), e) for (c, f, e), o in zip(checks, out[:-4]) if int(o) != e]
    assert len(out) - 4 == len(checks) and not bad, bad
