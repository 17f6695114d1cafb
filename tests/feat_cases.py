"""Designed inputs for the LiDAR front-end tests (tests/test_lidar_features.py): ring-boundary probes, a cloud whose rings hit every
sector size at which fe_sector changes its path, rings that force ties, the 21st pick, suppression into the halo and gaps, and depth
clouds for every exit of getFeatureDepth. Built point by point with numpy only (no LidarScene), deterministic, cached: the CPU tests
(oracle against the restatement) and the GPU tests (device against both) share them."""
import functools
import math

import numpy as np

F = np.float32


def ring_centre_deg(r, n_scans):
    """the vertical angle in the middle of ring r of the reference's ring model"""
    if n_scans == 16:
        return 2.0 * r - 15.0
    if n_scans == 32:
        return (r + 0.5) * 4.0 / 3.0 - 92.0 / 3.0
    return 2.0 - r / 3.0 if r < 32 else -8.83 - (r - 32) / 2.0


# ------------------------------------------------------------------------------------------------------------------- ring probes
PROBE_XY = ((10.0, 0.0), (6.0, 8.0), (3.0, 4.0), (7.3, 5.1))           # three exact dxy (10, 10, 5) and an inexact one


def ring_boundaries(n_scans):
    """[(label, angle in degrees)] of every decision of the ring model: the integer values of t from -1 to n_scans, and for 64 rings
    the seam of the two formulas, the cuts, and the place just behind the seam where the upper formula would step to 33"""
    if n_scans == 16:
        return [(f"t={k}", 2.0 * (k - 0.5) - 15.0) for k in range(-1, 17)]
    if n_scans == 32:
        return [(f"t={k}", (4.0 * k - 92.0) / 3.0) for k in range(-1, 33)]
    b = [(f"upper t={k}", 2.0 - (k - 0.5) / 3.0) for k in range(-1, 33)]
    b += [(f"lower t={k}", -8.83 - (k - 0.5) / 2.0) for k in range(1, 33)]
    # upper t=33 would be at -8.8333, behind the seam: no decision of the model, but where a misplaced seam shows
    return b + [("seam -8.83", -8.83), ("cut 2", 2.0), ("cut -24.33", -24.33), ("upper t=33 behind the seam", 2.0 - 32.5 / 3.0)]


@functools.lru_cache(maxsize=None)
def ring_probes(n_scans):
    """(points float32 (n, 4), labels): per boundary and per (x, y) the float32 z nearest the boundary and its +-8 float32 neighbours.
    Where the boundary is z = 0 (t is then an integer exactly, and the neighbours of 0 are denormals) the 17 probes are moved to
    j * 2^-23, j = -8 .. -1, 1 .. 9: about the spacing the ladders of the other boundaries have."""
    pts, labels = [], []
    for label, ang in ring_boundaries(n_scans):
        for x, y in PROBE_XY:
            dxy = float(np.sqrt(F(x) * F(x) + F(y) * F(y)))
            zb = F(dxy * math.tan(math.radians(ang)))
            if zb == 0:
                zs = [F(j * 2.0 ** -23) for j in list(range(-8, 0)) + list(range(1, 10))]
            else:
                up, dn = [zb], [zb]
                for _ in range(8):
                    up.append(np.nextafter(up[-1], F(np.inf))); dn.append(np.nextafter(dn[-1], F(-np.inf)))
                zs = dn[:0:-1] + up
            for z in zs:
                pts.append((x, y, z, 1.0)); labels.append(label)
    return np.array(pts, dtype=F), labels


def gate_probes():
    """[(points, min_range, max_range)] for the range gate and the non-finite inputs, 16 rings"""
    na = lambda v, to: float(np.nextafter(F(v), F(to)))
    a = []
    for x, y in ((3.0, 0.0), (na(3, 0), 0.0), (na(3, 4), 0.0), (60.0, 80.0), (na(60, 0), 80.0), (na(60, 99), 80.0), (60.0, na(80, 0)), (60.0, na(80, 99)),
                 (100.0, 0.0), (na(100, 0), 0.0), (na(100, 200), 0.0), (0.0, -3.0), (0.0, 100.0)):
        for z in (0.0, 0.5, -0.5):
            a.append((x, y, z, 1.0))
    for z in (np.nan, np.inf, -np.inf):
        a.append((10.0, 0.0, z, 1.0))
    a += [(np.inf, 0.0, 0.0, 1.0), (-np.inf, 1.0, 0.0, 1.0), (np.nan, 0.0, 0.0, 1.0), (10.0, np.nan, 0.0, 1.0), (1e30, 1e30, 0.0, 1.0), (10.0, 0.0, 1e38, 1.0)]
    b = [(0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 1.0, 1.0), (0.0, 0.0, -1.0, 1.0), (-0.0, 0.0, 0.0, 1.0), (1e-30, 0.0, 0.0, 1.0), (1e-30, 0.0, 1e-31, 1.0), (1e-20, 1e-20, -1e-21, 1.0),
         (5.0, 0.0, 0.1, 1.0), (100.0, 0.0, 1.0, 1.0)]
    return [(np.array(a, dtype=F), 3.0, 100.0), (np.array(b, dtype=F), 0.0, 100.0)]


# ------------------------------------------------------------------------------------------------------------------ whole clouds
def make_ring(r, n_scans, cnt, dxy, az0=0.0, sweep=2.0 * math.pi):
    """cnt points of ring r in firing order: azimuth sweep, horizontal distance dxy[j] (float64 array), elevation at the ring's centre
    angle. The intensity carries ring + j / 10000 so that every point of a cloud is distinct and a mix-up of points shows."""
    az = az0 + sweep * np.arange(cnt) / cnt
    el = math.radians(ring_centre_deg(r, n_scans))
    p = np.column_stack([dxy * np.cos(az), dxy * np.sin(az), dxy * math.tan(el), r + np.arange(cnt) / 10000.0])
    return p.astype(F)


def room_profile(cnt, half_width, seed, noise=0.01, pole_every=47):
    """horizontal distance of a square room seen from its middle (corners at 45 deg), float32-sized noise, and poles of 1..4 returns
    that stand 0.5 m in front of the wall every `pole_every` returns or so"""
    rng = np.random.default_rng(seed)
    az = 2.0 * math.pi * np.arange(cnt) / cnt
    d = half_width / np.maximum(np.abs(np.cos(az)), np.abs(np.sin(az))) + rng.normal(0.0, noise, cnt)
    j = 11 + int(rng.integers(0, 20))
    while j < cnt - 8:
        d[j:j + 1 + int(rng.integers(0, 4))] -= 0.5
        j += pole_every + int(rng.integers(-9, 10))
    return d


def interleave(rings_pts, extra=None):
    """one cloud out of per-ring point lists: the rings' points shuffled into each other, each ring's own order kept"""
    key = np.concatenate([np.arange(len(p)) / len(p) + 1e-7 * i for i, p in enumerate(rings_pts)])
    allp = np.concatenate(rings_pts)
    if extra is not None:
        key = np.concatenate([key, np.linspace(0.0, 1.0, len(extra), endpoint=False)]); allp = np.concatenate([allp, extra])
    return np.ascontiguousarray(allp[np.argsort(key, kind="stable")])


# ring -> returns, 16 rings. C = cnt - 10, len = C / 6, m = len - 1 (sectors 0..4), m5 = C - 1 - 5 len:
#   131 -> m 19, m5 20 | 130 skipped | 1548 -> 255, 257 | 1553 -> 256, 257 | 3084 -> 511, 513 | 3088 -> 512, 512 | 6154 -> 1023, 1023 | 6160 -> 1024 x 6
SECTOR_RINGS = {1: 131, 2: 130, 4: 1548, 5: 1553, 7: 3084, 8: 3088, 10: 6154, 15: 6160}
SECTOR_M_WANTED = (19, 20, 255, 256, 257, 511, 512, 513, 1023, 1024)


def sector_m(cnt):
    c = cnt - 10
    return [c // 6 - 1] * 5 + [c - 1 - 5 * (c // 6)]


@functools.lru_cache(maxsize=None)
def sector_cloud(big=6160):
    """the 16-ring cloud of SECTOR_RINGS (ring 15 with `big` returns; 6161 puts 1025 elements into its last sector), ring 0 and
    rings 3, 6, 9, 11..14 empty, plus returns that no ring takes"""
    rings = []
    for r, cnt in SECTOR_RINGS.items():
        cnt = big if r == 15 else cnt
        hw = 3.7 if cnt <= 131 else 5.0 + 0.4 * r                       # the sparse rings close by (but beyond the 3 m gate): neighbours around sqrt(0.05) m apart
        rings.append(make_ring(r, 16, cnt, room_profile(cnt, hw, 100 + r)))
    rej = np.array([(1.0, 1.0, 0.0, -1.0), (np.nan, 1.0, 0.0, -2.0), (10.0, 0.0, 9.0, -3.0), (300.0, 0.0, 0.0, -4.0), (10.0, 0.0, -9.0, -5.0)] * 40, dtype=F)
    return interleave(rings, rej)


@functools.lru_cache(maxsize=None)
def rejected_cloud():
    """n > 0 and no point in any ring: below the minimum range, above the top ring, NaN"""
    rng = np.random.default_rng(7)
    a = np.column_stack([rng.uniform(-2, 2, 600), rng.uniform(-2, 2, 600), rng.uniform(-1, 1, 600), np.ones(600)]).astype(F)
    a[::3] = (20.0, 0.0, 15.0, 2.0); a[1::7, 1] = np.nan
    return a


@functools.lru_cache(maxsize=None)
def one_ring_cloud():
    return make_ring(7, 16, 701, room_profile(701, 6.0, 3))


@functools.lru_cache(maxsize=None)
def tie_ring_cloud():
    """a table of 64 float32 points repeated 49 times exactly (3136 returns, sectors of 520 and 525): every curvature repeats exactly"""
    rng = np.random.default_rng(11)
    d = 10.0 + rng.normal(0.0, 0.03, 64)
    d[20:23] -= 0.4
    table = make_ring(8, 16, 64, d, sweep=0.128)
    p = np.tile(table, (49, 1))
    p[:, 3] = 8.0                                                        # equal intensities: a tie is then a tie of whole points too
    return p


@functools.lru_cache(maxsize=None)
def identical_ring_cloud():
    """400 times the same point, all coordinates exact in float32 sums: curvature exactly 0, six sectors of 64"""
    p = np.tile(np.array([(6.0, 8.0, 0.25, 0.0)], dtype=F), (400, 1))
    p[:, 3] = np.arange(400)
    return p


CORNER_AT = (103, 204, 301, 407)          # ring of 610: sector s is 5 + 100 s .. 103 + 100 s, element 104 + 100 s is dropped


@functools.lru_cache(maxsize=None)
def corner_ring_cloud():
    """a smooth circle of 610 returns (sectors of 99) with four returns 0.08 m off it: on the last kept element of sector 0, on the
    dropped element behind sector 1, two before the last kept element of sector 2 and two behind the first element of sector 4"""
    d = np.full(610, 10.0)
    d[list(CORNER_AT)] += 0.08
    return make_ring(8, 16, 610, d)


@functools.lru_cache(maxsize=None)
def gap_ring_cloud():
    """the circle of 610 with one plateau of six returns 0.5 m off it in every sector (a gap above sqrt(0.05) m on both ends); return k
    of sector k's plateau is another 0.05 m out, so it is picked first and suppresses 5 - k returns after it and k before it"""
    d = np.full(610, 10.0)
    for k in range(6):
        d[35 + 100 * k: 41 + 100 * k] += 0.5
        d[35 + 100 * k + k] += 0.05
    return make_ring(8, 16, 610, d)


# --------------------------------------------------------------------------------------------------------------------- depth
def _patch(rng, n, cx, depth, half=0.05, slope=0.0, side=0):
    """n camera-frame points around the ray (cx, 0, 1): offsets within +-half of the ray in x / z and y / z, on the plane
    z = depth + slope * (x - cx depth). side = +1 / -1 keeps the x offsets on one side of the ray."""
    ox = rng.uniform(-half, half, n); oy = rng.uniform(-half, half, n)
    if side:
        ox = side * (0.2 * half + 0.8 * np.abs(ox))
    x = cx * depth + ox * depth
    z = depth + slope * (x - cx * depth)
    return np.column_stack([x, oy * depth, z, np.ones(n)])


@functools.lru_cache(maxsize=None)
def depth_sized(n):
    """n points on a noisy wall 10 m ahead within +-3 deg of the axis, 40 features inside"""
    rng = np.random.default_rng(1000 + n)
    cloud = _patch(rng, n, 0.0, 10.0)
    cloud[:, 2] += rng.normal(0.0, 0.05, n)
    feats = np.column_stack([rng.uniform(-0.04, 0.04, 40), rng.uniform(-0.04, 0.04, 40), np.ones(40)])
    return cloud.astype(F), feats.astype(F)


@functools.lru_cache(maxsize=None)
def depth_usable(k):
    """12 points of which only k have a distance: the others have zero range or a NaN coordinate"""
    cloud, feats = depth_sized(12)
    cloud = cloud.copy()
    bad = np.setdiff1d(np.arange(12), [2, 5, 9][:k])
    cloud[bad[::2], :3] = 0.0
    cloud[bad[1::2], 1] = np.nan
    return cloud, feats


@functools.lru_cache(maxsize=None)
def depth_ties():
    """feature (0, 0, 1); the 3rd and 4th nearest points are mirror images in x (exactly equal distances, another plane) in the first
    cloud and exact duplicates in the second"""
    far = _patch(np.random.default_rng(5), 12, 0.0, 10.0, half=0.04)
    far[:, 0] += 0.6
    base = [(0.05, 0.1, 10.0, 1.0), (0.03, -0.1, 10.2, 1.0)]
    mirror = np.array(base + [(0.2, 0.05, 10.5, 1.0), (-0.2, 0.05, 10.5, 1.0)] + far.tolist(), dtype=F)
    mirror2 = np.array(base + [(-0.2, 0.05, 10.5, 1.0), (0.2, 0.05, 10.5, 1.0)] + far.tolist(), dtype=F)
    dup = np.array(base + [(0.2, 0.05, 10.5, 1.0), (0.2, 0.05, 10.5, 1.0)] + far.tolist(), dtype=F)
    feats = np.array([(0.0, 0.0, 1.0), (0.0, 0.0, 2.0), (0.0, 0.001, 1.0)], dtype=F)
    return [mirror, mirror2, dup], feats


DEPTH_EXIT_PLAN = (("ok", -0.8), ("spread", -0.5), ("s_small", -0.2), ("low", 0.1), ("clamp_max", 0.4), ("clamp_min", 0.7), ("threshold", 1.0))


@functools.lru_cache(maxsize=None)
def depth_exits():
    """one patch per exit of getFeatureDepth, each around its own ray (x / z = DEPTH_EXIT_PLAN), 10 features per patch"""
    rng = np.random.default_rng(42)
    cl, ft = [], []
    for name, cx in DEPTH_EXIT_PLAN:
        if name == "ok":
            cl.append(_patch(rng, 150, cx, 10.0))
        elif name == "spread":
            p = _patch(rng, 150, cx, 10.0); p[::2, :3] *= 1.3; cl.append(p)
        elif name == "s_small":
            cl.append(_patch(rng, 150, cx, 0.4))
        elif name == "low":
            cl.append(_patch(rng, 150, cx, 1.5))
        elif name == "clamp_max":
            cl.append(_patch(rng, 150, cx, 10.0, half=0.02, slope=20.0, side=-1))
        elif name == "clamp_min":
            cl.append(_patch(rng, 150, cx, 10.0, half=0.02, slope=20.0, side=+1))
        if name == "threshold":
            ft.append(np.column_stack([cx + rng.uniform(-0.01, 0.01, 10), rng.uniform(-0.01, 0.01, 10), np.ones(10)]))       # nothing within 2.5 deg
        elif name.startswith("clamp"):
            ft.append(np.column_stack([np.full(10, cx), rng.uniform(-0.01, 0.01, 10), np.ones(10)]))
        else:
            ft.append(np.column_stack([cx + rng.uniform(-0.03, 0.03, 10), rng.uniform(-0.03, 0.03, 10), np.ones(10)]))
    cloud = np.concatenate(cl)
    return np.ascontiguousarray(cloud[rng.permutation(len(cloud))].astype(F)), np.concatenate(ft).astype(F)


@functools.lru_cache(maxsize=None)
def exact_gap():
    """float32 offsets (a, b, c) with fl(fl(a a + b b) + c c) == 0.05 exactly in double; a is a multiple of 2^-20 so that 8 + a is a float"""
    a = math.floor(math.sqrt(0.05) * 2 ** 20) / 2 ** 20
    b = float(F(math.sqrt(0.05 - a * a)))
    while a * a + b * b > 0.05:
        b = float(np.nextafter(F(b), F(0)))
    c = float(F(math.sqrt(0.05 - (a * a + b * b))))
    assert (a * a + b * b) + c * c == 0.05 and float(F(a)) == a
    return a, b, c


EXACT_GAP_AT = 256


@functools.lru_cache(maxsize=None)
def exact_gap_ring_cloud():
    """610 returns along a line, 1 / 64 m apart (every curvature away from the step is exactly 0), with one step between returns 256
    and 257 whose squared length is exactly the double 0.05: the suppression's `> 0.05` must walk across it"""
    a, b, c = exact_gap()
    j = np.arange(610)
    p = np.zeros((610, 4))
    p[:, 0] = 4.0 + j / 64.0
    after = j > EXACT_GAP_AT
    p[after, 0] = 8.0 + a + (j[after] - EXACT_GAP_AT - 1) / 64.0
    p[after, 1] = b; p[after, 2] = c
    p[:, 3] = j
    q = p.astype(F)
    assert np.array_equal(q.astype(np.float64), p)                         # every coordinate is a float32 exactly
    return q
