"""Scan Context on the device (csrc/vilf_sc.hip) at the edges tests/test_scancontext.py does not reach: candidates beyond one pass of the waves' stride, exact ties at
every minimum (ring-key top-k, alignment, shift, candidate), every parameter away from its default, descriptor bins on exact boundaries, empty descriptors, refused
creation, and the distance against its definition at 60 digits (tests/sc_exact.py).

Every case is built by a cached function that runs the restatement (tests/sc_reference.py) and asserts the case's preconditions on it: the plant wins, the tie is a
tie to the bit, the gap to the next DISTINCT distance exceeds 1e-9. The CPU tests call those functions, so a machine without a GPU checks every precondition; the
GPU tests hand the same case to the device and compare as tests/test_scancontext.py does: integers equal, min_dist to 1e-12, yaw_diff_rad as float32.
Builder clouds (tests/sc_cases.py) hold multiples of 1/8: their ring keys, and so the float ring-key distances both sides compute with the same operations, are the
same bits on the device and in the restatement (asserted in test_snapshot_schedules), so candidate lists need no gap. No number here was tuned on a device result.
"""
import ctypes as C
import functools
import math
import numpy as np
import pytest
from vil_fusion_amd import abi
import sc_cases as K
import sc_exact as X
import sc_reference as R

U = 2.0 ** -53
# DESIGN.md §3f derives both: 44 u on a cosine (20 u for the 20-term dot against |a||b|, 23 u for the product of two norms or 24 u for two normalised columns, 1 u for
# the quotient where there is one), 30.5 u for the ordered sum of n <= 60 terms of magnitude <= 1 divided by n, 1 u for that division, 2 u for the subtraction
# (a distance is at most 2): 77.5 u to first order, asserted as 80 u. An argmin is only compared where the exact gap exceeds twice the bound (both values move).
BOUND_RESTATEMENT = 80 * U
BOUND_KERNEL = 80 * U
EXH = dict(num_exclude_recent=1, tree_making_period=1, num_candidates=0, search_ratio=1.0)        # query k sees [0, k), every candidate, every shift
ROW_BYTES = abi.ScResult.candidates.offset + 16 * 4                                               # vilf_sc_result without its tail padding


@functools.lru_cache(maxsize=None)
def _cloud_of(key):
    return K.cloud_from_heights(np.frombuffer(key).reshape(K.RINGS, K.SECTORS))


def _clouds(maps):
    return [_cloud_of(np.ascontiguousarray(h, dtype=np.float64).tobytes()) for h in maps]


def _ref(maps, memo=None, **over):
    m = R.SCManager(R.Params(**over), memo)
    for h in maps:
        m.add_descriptor(h)
    return m


def _pre(records, thres):
    """what must hold on the restatement before the device is looked at; exact ties are allowed, near ties are not"""
    for o in records:
        assert o["distinct_gap"] > 1e-9, o
        assert abs(o["min_dist"] - thres) > 1e-9, o


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------------------------
STRIDE_SIZES = (255, 256, 257, 258, 511, 512, 513, 519)
STRIDE_PLACES = (0, 255, 256, 257, 511, 512)
TIE_PAIRS = ((0, 256), (255, 256), (1, 2), (3, 4), (40, 300), (64, 128), (64, 256), (128, 320))     # (64, 256): slot 0 holds the HIGHER place, read by the same lane first
TIE_TRIPLES = ((0, 256, 512), (255, 256, 257), (2, 64, 300))
_MEMO = {}                                   # distances of the shared query against the shared base, computed once for all strided and tied cases


@functools.lru_cache(maxsize=None)
def _base():
    base = K.database(520, seed=11)
    q = K.random_heights(np.random.default_rng(12))
    return base, q, K.variant(q, rot=17, thin=0.2, seed=1), K.variant(q, rot=17, thin=0.45, seed=2)


def _planted(S, plants):
    """the base's first S maps with `plants` {index: map} put in, the query as key frame S; -> (maps, the restatement's record of the query)"""
    base, q, _, _ = _base()
    maps = list(base[:S]) + [q]
    for i, h in plants.items():
        maps[i] = h
    return maps, _ref(maps, _MEMO, dist_thres=0.5, **EXH).detect_at(S)


@functools.lru_cache(maxsize=None)
def _stride_cases(S):
    _, _, plant, _ = _base()
    out = []
    for place in sorted({p for p in STRIDE_PLACES if p < S} | {S - 1}):
        maps, ref = _planted(S, {place: plant})
        assert ref["nearest"] == place and ref["loop_id"] == place and ref["n_candidates"] == S and ref["candidates"] == list(range(16)), (S, place, ref)
        _pre([ref], 0.5)
        out.append((place, maps, ref))
    return out


@functools.lru_cache(maxsize=None)
def _tie_cases():
    _, _, plant, worse = _base()
    out = []
    for places in TIE_PAIRS + TIE_TRIPLES:
        lo, hi = min(places), max(places)
        thirds = [hi + 5, lo - 1 if lo > 0 else lo + 1]
        assert not set(thirds) & set(places)
        for third in thirds:                                  # the worse plant after the tied ones, then before (or between) them
            maps, ref = _planted(519, {**{p: plant for p in places}, third: worse})
            assert ref["nearest"] == lo and ref["runner_up_gap"] == 0.0, (places, third, ref)
            _pre([ref], 0.5)
            out.append((places, third, maps, ref))
    return out


@functools.lru_cache(maxsize=None)
def _mixed_case():
    maps = K.database(261, seed=13, plants={70: (5, 3, 0.2), 150: (100, 50, 0.25), 256: (64, 9, 0.2), 258: (30, 7, 0.2), 259: (257, 58, 0.15), 260: (256, 31, 0.1)})
    m = _ref(maps, dist_thres=0.5, **EXH)
    at = (60, 64, 65, 128, 256, 257, 260)
    ref = {k: m.detect_at(k) for k in at}
    _pre(ref.values(), 0.5)
    assert ref[256]["nearest"] == 64 and ref[260]["nearest"] == 256
    return maps, ref


PLACE = dict(num_exclude_recent=1, tree_making_period=1, num_candidates=16, search_ratio=1.0, dist_thres=0.5)


@functools.lru_cache(maxsize=None)
def _place_cases():
    """entry `plain` holds A (the query's place seen again), entry `scaled` holds 2 A: the same distances to the bit, a ring key further from the query's, so A is
    searched first wherever it stands"""
    out = []
    for plain, scaled in ((5, 2), (2, 5)):
        maps = K.database(13, seed=21)
        a = K.variant(maps[12], rot=9, thin=0.15, seed=3)
        maps[plain], maps[scaled] = a, 2.0 * a
        m = _ref(maps, **PLACE)
        ref = m.detect_at(12)
        c = ref["candidates"]
        assert ref["n_candidates"] == 12 and c.index(plain) < c.index(scaled)
        assert R.distance(maps[12], a, m.p) == R.distance(maps[12], 2.0 * a, m.p) and ref["runner_up_gap"] == 0.0
        assert ref["nearest"] == plain and ref["loop_id"] == plain
        _pre([ref], 0.5)
        out.append((plain, scaled, maps, ref))
    return out


TOPK_PAIRS = ((10, 11), (20, 84), (63, 64), (127, 128))
TOPK_CLOSER_AT = tuple(150 + 3 * i for i in range(15))


@functools.lru_cache(maxsize=None)
def _topk_cases(k):
    """snapshot of 200, the query as key frame 200. Two entries with bit-equal ring keys (a variant of the query and a same_rings() copy of it) stand at ranks
    (k - 1, k) of the ring-key order (the cut at k between them) or (k - 2, k - 1); the ranks before them are nested, less thinned variants of the query"""
    out = []
    for e1, e2 in TOPK_PAIRS:
        for straddle in (True, False):
            closer = k - 1 if straddle else k - 2
            if closer < 0:
                continue
            maps = K.database(201, seed=61)
            q = maps[200]
            for i in range(closer):
                maps[TOPK_CLOSER_AT[i]] = K.variant(q, rot=i + 1, seed=9, drop=2 * (i + 1))
            maps[e1] = K.variant(q, rot=3, seed=9, drop=40)
            maps[e2] = K.same_rings(maps[e1], rot=11, moves=6, seed=e2)
            m = _ref(maps, num_exclude_recent=1, tree_making_period=1, num_candidates=k, dist_thres=0.5)
            ref = m.detect_at(200)
            assert np.array_equal(m.rkeys[e1], m.rkeys[e2]) and not np.array_equal(maps[e1], np.roll(maps[e2], -11, axis=1))
            c = ref["candidates"]
            assert len(c) == k and sorted(c[:closer]) == sorted(TOPK_CLOSER_AT[:closer]), (k, e1, e2, straddle, c)
            assert (c[-1] == e1 and e2 not in c) if straddle else c[-2:] == [e1, e2], (k, e1, e2, straddle, c)
            _pre([ref], 0.5)
            out.append((e1, e2, straddle, maps, ref))
    return out


SAME_KEY_QUERIES = (1, 2, 15, 16, 17, 63, 64, 65, 200)


@functools.lru_cache(maxsize=None)
def _same_key_case(k):
    """every entry has the same ring key: all ring-key distances are equal and the candidates must be the first min(k, S) entries"""
    base = K.random_heights(np.random.default_rng(71))
    maps = [K.same_rings(base, rot=i % 60, moves=30, seed=1000 + i) for i in range(201)]
    m = _ref(maps, num_exclude_recent=1, tree_making_period=1, num_candidates=k, dist_thres=0.5)
    assert all(np.array_equal(m.rkeys[0], r) for r in m.rkeys)
    ref = {q: m.detect_at(q) for q in SAME_KEY_QUERIES}
    assert all(o["candidates"] == list(range(min(k, q))) for q, o in ref.items())
    _pre(ref.values(), 0.5)
    return maps, ref


SHIFT_ROTATIONS = (0, 1, 2, 3, 30, 57, 58, 59)
SHIFT_RATIOS = ((0.0, 0), (0.05, 2), (0.1, 3), (0.15, 5), (0.95, 29), (1.0, 30))


@functools.lru_cache(maxsize=None)
def _shift_case(ratio, radius):
    """key frames 2 i and 2 i + 1 = (a place rotated by SHIFT_ROTATIONS[i] columns and thinned, the place): query 2 i + 1 finds 2 i"""
    rng = np.random.default_rng(81)
    maps = []
    for i, rot in enumerate(SHIFT_ROTATIONS):
        q = K.random_heights(rng)
        maps += [K.variant(q, rot=rot, thin=0.1, seed=i), q]
    over = dict(num_exclude_recent=1, tree_making_period=1, num_candidates=0, search_ratio=ratio, dist_thres=0.5)
    m = _ref(maps, **over)
    ref = m.detect_range(0, len(maps))
    wraps = 0
    for i, rot in enumerate(SHIFT_ROTATIONS):
        o = ref[2 * i + 1]
        al = R.align(R.sector_key(maps[2 * i + 1]), R.sector_key(maps[2 * i]))
        searched = R.search_shifts(al, m.p)
        assert al == (60 - rot) % 60 and len(searched) == min(2 * radius + 1, 60), (ratio, rot, al, searched)
        assert (o["nearest"], o["shift"]) == (2 * i, al), (ratio, rot, o)
        if radius == 0:
            assert searched == [al]                                            # only the aligned shift is read
        if 0 < radius < 30 and (al < radius or al > 59 - radius):
            assert 0 in searched and 59 in searched and searched != list(range(searched[0], searched[0] + len(searched)))
            wraps += 1
    assert wraps >= (0 if radius in (0, 30) else 4)
    _pre(ref[1:], 0.5)
    return maps, over, ref


@functools.lru_cache(maxsize=None)
def _symmetric_cases():
    """a candidate that is the same under a rotation by 30 columns: the alignment norms and the distances tie at s and s + 30, the lower shift wins"""
    out = []
    rng = np.random.default_rng(91)
    for rot in (0, 4, 29, 31, 47):
        q = K.random_heights(rng)
        cand = K.symmetric(K.variant(q, rot=rot, thin=0.1, seed=rot))
        d = R.shift_distances(q, cand, range(60))
        n = X.align_norms(q, cand)
        assert np.array_equal(d[:30], d[30:]) and all(n[s] == n[s + 30] for s in range(30))
        for mode in (dict(num_candidates=0, search_ratio=1.0), dict(num_candidates=3, search_ratio=0.1)):
            over = dict(num_exclude_recent=1, tree_making_period=1, dist_thres=0.9, **mode)
            ref = _ref([cand, q], **over).detect_at(1)
            assert ref["nearest"] == 0 and ref["shift"] < 30 and d[ref["shift"]] == ref["min_dist"]
            if mode["search_ratio"] == 1.0:
                assert ref["min_dist"] == d.min() and ref["runner_up_gap"] == 0.0
            else:
                assert ref["shift"] in R.search_shifts(R.align(R.sector_key(q), R.sector_key(cand)), R.Params(**over))
            _pre([ref], 0.9)
            out.append((rot, [cand, q], over, ref))
    return out


SCHEDULES = tuple((e, t) for e in (1, 2, 45) for t in (1, 7, 64))


@functools.lru_cache(maxsize=None)
def _schedule_maps():
    return K.database(140, seed=31, plants={i: (i - 70, (7 * i) % 60, 0.05) for i in range(75, 140, 5)})


@functools.lru_cache(maxsize=None)
def _schedule_case(exclude, period):
    over = dict(num_exclude_recent=exclude, tree_making_period=period, dist_thres=0.3)
    _, ref = R.replay(_clouds(_schedule_maps()), R.Params(**over))
    searched = [o for o in ref if o["n_candidates"] > 0]
    assert len(searched) == 140 - exclude and [o["snapshot"] for o in searched] == [period * (c // period) + 1 for c in range(140 - exclude)]
    assert any(o["loop_id"] >= 0 for o in searched) and any(o["loop_id"] < 0 for o in searched)
    _pre(searched, 0.3)
    return over, ref


IRREGULAR = dict(num_exclude_recent=5, tree_making_period=7, dist_thres=0.3)


@functools.lru_cache(maxsize=None)
def _irregular_case():
    """detects[i] calls of detect after key frame i: none, one or two, and some while fewer than num_exclude_recent + 1 key frames exist"""
    maps = _schedule_maps()[:90]
    detects = [int(v) for v in np.random.default_rng(5).integers(0, 3, len(maps))]
    assert sum(detects[:5]) > 0 and 0 in detects[5:] and 2 in detects[5:]
    m = R.SCManager(R.Params(**IRREGULAR))
    ref, differs = [], 0
    for k, c in enumerate(_clouds(maps)):
        m.add(c)
        for _ in range(detects[k]):
            o = m.detect()
            differs += o["n_candidates"] > 0 and o["snapshot"] != m.detect_at(k)["snapshot"]
            ref.append(o)
    assert differs >= 1, differs                        # otherwise the host's call counter and the replay's formula could not be told apart
    _pre([o for o in ref if o["n_candidates"] > 0], 0.3)
    return maps, detects, ref


@functools.lru_cache(maxsize=None)
def _empty_cases():
    q = _cloud_of(K.random_heights(np.random.default_rng(95)).tobytes())
    none = np.zeros((0, 4), dtype=np.float32)
    out = []
    for name, clouds, over, at in (
            ("empty query, exhaustive", _clouds(K.database(5, seed=96)) + [none], dict(EXH), 5),
            ("empty query, reference mode", _clouds(K.database(5, seed=96)) + [none], dict(num_exclude_recent=1, tree_making_period=1), 5),
            ("300 empty candidates", [none] * 300 + [q], dict(EXH), 300),
            ("300 empty candidates, dist_thres = inf", [none] * 300 + [q], dict(EXH, dist_thres=math.inf), 300)):
        m = R.SCManager(R.Params(**over))
        for c in clouds:
            m.add(c)
        ref = m.detect_at(at)
        want_loop = 0 if over.get("dist_thres") == math.inf else -1          # 10000000 < inf: nn_idx's initial value is reported as a loop (include/vilfusion.h)
        assert (ref["loop_id"], ref["nearest"], ref["shift"], ref["min_dist"]) == (want_loop, 0, 0, R.NO_DIST), (name, ref)
        out.append((name, clouds, over, at, ref))
    return out


def _pt(ring, sector, z):
    """a point at the centre of bin (ring, sector), both from 0"""
    a = math.radians((sector + 0.5) * 6.0)
    return [(ring + 0.5) * 4.0 * math.cos(a), (ring + 0.5) * 4.0 * math.sin(a), z, 0.0]


def _scatter(n, seed):
    """n points anywhere within 85 m (ring boundaries and the radius are not avoided), at least 0.3 degrees inside their sector: the sector is the one thing that
    goes through an atan"""
    rng = np.random.default_rng(seed)
    ang = np.deg2rad((rng.integers(0, 60, n) + rng.uniform(0.05, 0.95, n)) * 6.0)
    rad = rng.uniform(0.01, 85.0, n)
    return np.column_stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-3.0, 6.0, n), np.zeros(n)]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _descriptor_edge_clouds():
    p = R.Params()
    f32 = np.float32
    up = lambda v: np.nextafter(f32(v), f32(np.inf) if v > 0 else f32(-np.inf))          # away from zero
    down = lambda v: np.nextafter(f32(v), f32(0))
    cases = {}
    # exact ranges 20, 40, 60, 80 in the four quadrants and 4 k on the +x axis; every point has its own height, rising with the index
    exact = [(sx * bx * m, sy * by * m) for m in (1, 2, 3, 4) for bx, by in ((12, 16), (16, 12)) for sx, sy in ((1, 1), (-1, 1), (-1, -1), (1, -1))]
    axis = [(4.0 * k, 0.0) for k in range(1, 21)]
    for name, move in (("exact", lambda v: f32(v)), ("up", up), ("down", down)):
        pts = [[f32(x), f32(y)] for x, y in exact + axis]
        if name != "exact":
            pts = [[move(x), f32(y)] for x, y in exact + axis] + [[f32(x), move(y)] for x, y in exact]
        z = 0.125 * (1 + np.arange(len(pts)))
        cases["ranges " + name] = np.column_stack([np.array(pts, dtype=np.float32), z, np.zeros(len(pts))]).astype(np.float32)
    ok, ring, _, _, rng_, _ = R.point_bins(cases["ranges exact"], p)
    assert ok.all() and np.array_equal(rng_[:32], np.repeat([20, 40, 60, 80], 8).astype(np.float32)) and np.array_equal(ring[:32], np.repeat([4, 9, 14, 19], 8))
    assert np.array_equal(rng_[32:], 4.0 * np.arange(1, 21)) and rng_[-1] == 80.0 and ring[-1] == 19        # range 80 lands in ring 20; 4 k / 80 * 20 is not k for every k
    ok, ring, _, _, rng_, _ = R.point_bins(cases["ranges up"], p)
    assert not ok[51] and rng_[51] > 80.0 and ring[32] == 1                       # the next float above 80 on the axis is skipped, the one above 4 is in ring 2
    ok, ring, *_ = R.point_bins(cases["ranges down"], p)
    assert ok.all() and np.array_equal(ring[32:52], np.arange(20))
    # z + height around NO_POINT = -1000, each alone in its bin; z = -2 stores 0.0; a bin of negative heights only
    lo = f32(-1002.0)
    cases["heights"] = np.array([_pt(3, 7, lo), _pt(4, 8, np.nextafter(lo, f32(0))), _pt(5, 9, np.nextafter(lo, f32(-np.inf))), _pt(6, 10, -2.0),
                                 _pt(7, 11, -3.0), _pt(7, 11, -2.5), _pt(7, 11, -4.0), _pt(8, 12, 1.0)], dtype=np.float32)
    d = R.make_descriptor(cases["heights"], p)
    assert d[3, 7] == 0 and d[4, 8] == float(np.nextafter(f32(-1000.0), f32(0))) and d[5, 9] == 0 and d[6, 10] == 0 and d[7, 11] == -0.5 and np.count_nonzero(d) == 3
    rng = np.random.default_rng(7)
    z = rng.uniform(-1.0, 5.0, 5000)
    for name, zz in (("5000 in a bin, maximum last", np.append(z, 5.5)), ("5000 in a bin, maximum first", np.append(5.5, z))):
        cases[name] = np.array([_pt(9, 33, v) for v in zz], dtype=np.float32)
        assert R.make_descriptor(cases[name], p)[9, 33] == 7.5 and len(cases[name]) == 5001
    for n in (255, 256, 257, 100000):
        cases[f"{n} points"] = _scatter(n, n)
    return cases


@functools.lru_cache(maxsize=None)
def _zero_height_case():
    """columns 7 and 40 of key frame 1 hold nothing but points that store 0.0 (z = -2) or never enter (z + 2 = -1000): their norm is zero and they are not counted"""
    maps = K.database(3, seed=97, plants={2: (1, 5, 0.1)})
    for h in maps[1:]:
        h[:, [7, 40]] = 0.0
    clouds = _clouds(maps)
    clouds[1] = np.concatenate([clouds[1], np.array([_pt(2, 7, -2.0), _pt(9, 7, -2.0), _pt(15, 7, -2.0), _pt(4, 40, -1002.0)], dtype=np.float32)])
    m = R.SCManager(R.Params(dist_thres=0.5, **EXH))
    for c in clouds:
        m.add(c)
    assert np.array_equal(m.descs[1], maps[1]) and (R.col_norms(m.descs[1]) == 0).sum() == 2
    ref = m.detect_range(0, 3)
    _pre(ref[1:], 0.5)
    return clouds, ref


@functools.lru_cache(maxsize=None)
def _exact_set():
    """ten key frames, five from the builders and five of the route that revisits itself (69 and 70 see the places of 0 and 1 again), and for the 45 pairs (k, j < k)
    the exact alignment norms and per-shift distances"""
    rng = np.random.default_rng(51)
    q, other = K.random_heights(rng), K.random_heights(rng)
    maps = [q, K.variant(q, rot=13, thin=0.2, seed=1), other, K.variant(q, rot=41, thin=0.35, seed=2, scale=2.0), K.variant(other, rot=59, thin=0.1, seed=3)]
    route, _ = R.revisit_route(n_frames=72)
    clouds = _clouds(maps) + [route[i] for i in (0, 1, 35, 69, 70)]
    descs = [R.make_descriptor(c, R.Params()) for c in clouds]
    assert all(np.array_equal(d, h) for d, h in zip(descs, maps))
    pairs = [(k, j) for k in range(len(descs)) for j in range(k)]
    exact = {(k, j): (X.align_norms(descs[k], descs[j]), X.shift_distances(descs[k], descs[j])) for k, j in pairs}
    return clouds, descs, pairs, exact


def _argmin_gap(values, order):
    """(first minimum's place, gap to the runner-up as a float) of exact values"""
    best, arg = X.first_min(values, order, X.NO_DIST)
    return arg, float(X.gap_to_runner_up(values, order))


# ---- CPU: the builders -------------------------------------------------------------------------------------------------------------------------------------------
def test_builder_cloud_has_the_descriptor_it_was_built_from():
    p = R.Params()
    rng = np.random.default_rng(1)
    for _ in range(5):
        h = K.random_heights(rng)
        assert 300 < np.count_nonzero(h) < 420
        for m in (h, 2.0 * h, K.variant(h, rot=23, thin=0.3, seed=4), K.symmetric(h), K.same_rings(h, 7, 20, 5)):
            assert np.array_equal(R.make_descriptor(K.cloud_from_heights(m), p), m)
    assert np.array_equal(R.make_descriptor(K.cloud_from_heights(np.zeros((20, 60))), p), np.zeros((20, 60)))


def test_builder_rotation_keeps_the_ring_key_bits_and_scaling_keeps_the_distances():
    rng = np.random.default_rng(2)
    h, q = K.random_heights(rng), K.random_heights(rng)
    for k in (1, 17, 30, 59):
        assert np.array_equal(R.ring_key(np.roll(h, k, axis=1)), R.ring_key(h))
    s = K.same_rings(h, 11, 25, 3)
    assert np.array_equal(R.ring_key(s), R.ring_key(h)) and 30 < np.count_nonzero(s != np.roll(h, 11, axis=1)) <= 50
    assert np.array_equal(R.shift_distances(q, 2.0 * h, range(60)), R.shift_distances(q, h, range(60))) and not np.array_equal(R.ring_key(2.0 * h), R.ring_key(h))
    assert np.array_equal(R.col_norms(2.0 * h), 2.0 * R.col_norms(h))


def test_builder_symmetric_candidate_ties_at_s_and_s_plus_30():
    rng = np.random.default_rng(3)
    h, q = K.symmetric(K.random_heights(rng)), K.random_heights(rng)
    d = R.shift_distances(q, h, range(60))
    assert np.array_equal(d[:30], d[30:])
    d = R.shift_distances(h, q, range(60))            # a symmetric QUERY sums the same terms in another order: no tie to the bit
    assert not np.array_equal(d[:30], d[30:]) and np.allclose(d[:30], d[30:], rtol=0, atol=1e-14)


def test_builder_variants_of_one_seed_are_nested_and_database_plants():
    h = K.random_heights(np.random.default_rng(4))
    a, b = K.variant(h, seed=9, drop=10), K.variant(h, seed=9, drop=30)
    assert np.count_nonzero(h) - np.count_nonzero(a) == 10 and np.all((b == 0) | (b == a)) and np.all((a == 0) | (a == h))
    maps = K.database(8, seed=5, plants={3: (1, 7, 0.25), 6: (3, 2, 0.0), 7: h})
    assert np.array_equal(maps[6], np.roll(maps[3], 2, axis=1)) and np.array_equal(maps[7], h)
    p = R.Params(num_candidates=0, search_ratio=1.0)
    d_plant, d_other = R.distance(maps[3], maps[1], p)[0], [R.distance(maps[i], maps[j], p)[0] for i in (0, 2, 4) for j in (1, 5)]
    assert d_plant < 0.3 and 0.5 < min(d_other) and max(d_other) < 0.8


@pytest.mark.parametrize("over", [dict(), dict(num_exclude_recent=2, tree_making_period=7), dict(num_exclude_recent=45, tree_making_period=64, num_candidates=16)])
def test_reference_detect_at_is_the_replay(over):
    maps = _schedule_maps()[:100]
    m, ref = R.replay(_clouds(maps), R.Params(**over))
    calls = m.calls
    assert m.detect_range(0, len(maps)) == ref and m.calls == calls
    assert _ref(maps[:60], **over).detect_at(59) == ref[59]                   # needs key frames 0..k only; add_descriptor() is add() for a builder cloud


# ---- CPU: the restatement against the definition at 60 digits ---------------------------------------------------------------------------------------------------
def test_restatement_distances_within_the_derived_bound_of_exact():
    _, descs, pairs, exact = _exact_set()
    worst, n = 0.0, 0
    for k, j in pairs:
        got = R.shift_distances(descs[k], descs[j], range(60))
        for s in range(60):
            want = exact[k, j][1][s]
            assert (want is None) == bool(np.isnan(got[s]))
            if want is not None:
                worst = max(worst, abs(float(X.MP.mpf(float(got[s])) - want)))
                n += 1
    print(f"restatement against exact: {len(pairs)} pairs, {n} distances, worst error {worst / U:.2f} u, bound {BOUND_RESTATEMENT / U:.0f} u")
    assert n == 60 * len(pairs) and worst <= BOUND_RESTATEMENT
    for k in range(1, len(descs)):                   # the device test compares every query's argmin: none may be too close to call
        every = sorted(v for j in range(k) for v in exact[k, j][1] if v is not None)
        assert float(every[1] - every[0]) > 2 * BOUND_KERNEL, k


def test_restatement_alignment_and_shift_equal_exact():
    """the alignment norm of a pair is bounded by 280 u max|sector key|; decisions whose exact gap is below twice the bound are skipped, at most 5 %"""
    _, descs, pairs, exact = _exact_set()
    assert min(d.min() for d in descs) >= 0                       # the bound takes |difference of two keys| <= max |key|: keys of one sign
    decisions = skipped = 0
    for k, j in pairs:
        norms, dists = exact[k, j]
        bound_n = 280 * U * max(float(abs(v)) for d in (descs[k], descs[j]) for v in X.sector_key(d))
        al, gap = _argmin_gap(norms, range(60))
        decisions += 1
        if gap <= 2 * bound_n:
            skipped += 1
            continue
        assert R.align(R.sector_key(descs[k]), R.sector_key(descs[j])) == al, (k, j)
        for ratio, radius in ((0.1, 3), (1.0, 30)):
            window = X.search_window(al, radius)
            arg, gap = _argmin_gap(dists, window)
            decisions += 1
            if gap <= 2 * BOUND_RESTATEMENT:
                skipped += 1
                continue
            d, s = R.distance(descs[k], descs[j], R.Params(search_ratio=ratio))
            want, want_s, _ = X.distance(descs[k], descs[j], radius, norms, dists)
            assert s == arg == want_s and abs(float(X.MP.mpf(d) - want)) <= BOUND_RESTATEMENT, (k, j, ratio)
    print(f"alignment and shift: {decisions} decisions, {skipped} skipped for an exact gap below twice the bound")
    assert skipped <= 0.05 * decisions


def test_exact_reference_on_a_pair_known_by_construction():
    h = K.random_heights(np.random.default_rng(6))
    h[:, 5] = 0.0
    r = np.roll(h, 7, axis=1)
    d, n = X.shift_distances(r, h), X.align_norms(r, h)
    assert abs(d[7]) < 1e-55 and n[7] == 0 and min(v for s, v in enumerate(d) if s != 7) > 0.3 and X.distance(r, h, 3)[1:] == (7, 7)
    assert X.sector_key(h)[5] == 0 and abs(X.sector_key(h)[6] - X.MP.mpf(float(h[:, 6].sum())) / 20) < 1e-55
    empty = np.zeros((20, 60))
    assert X.shift_distances(h, empty) == [None] * 60 and X.distance(h, empty, 30)[:2] == (X.NO_DIST, 0)
    one = np.zeros((20, 60)); one[3, 0] = 2.0; two = np.zeros((20, 60)); two[3, 10] = 1.0; two[4, 10] = 1.0
    d = X.shift_distances(one, two)                                           # one column each: they meet at shift 50 only, at cos 45 degrees
    assert [s for s in range(60) if d[s] is not None] == [50] and abs(d[50] - (1 - 1 / X.MP.sqrt(2))) < 1e-55


# ---- CPU: every precondition of the device tests ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", STRIDE_SIZES)
def test_preconditions_strided_candidates(S):
    assert len(_stride_cases(S)) == len({p for p in STRIDE_PLACES if p < S} | {S - 1})


def test_preconditions_ties_place_and_mixed_sizes():
    assert len(_tie_cases()) == 2 * (len(TIE_PAIRS) + len(TIE_TRIPLES)) and len(_place_cases()) == 2 and len(_mixed_case()[1]) == 7


@pytest.mark.parametrize("k", [1, 2, 3, 16])
def test_preconditions_ring_key_top_k(k):
    assert len(_topk_cases(k)) == (4 if k == 1 else 8) and len(_same_key_case(k)[1]) == len(SAME_KEY_QUERIES)


def test_preconditions_shifts():
    for ratio, radius in SHIFT_RATIOS:
        assert int(math.floor(0.5 * ratio * 60 + 0.5)) == radius
        _shift_case(ratio, radius)
    assert len(_symmetric_cases()) == 10


def test_preconditions_schedules_descriptors_and_empty():
    for e, t in SCHEDULES:
        _schedule_case(e, t)
    _irregular_case()
    assert len(_descriptor_edge_clouds()) == 10 and len(_empty_cases()) == 4 and len(_zero_height_case()[1]) == 3


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver():
    from vil_fusion_amd.estimator import BackendSolver
    s = BackendSolver()
    yield s
    s.close()


def _sc(solver, clouds, capacity=None, **over):
    from vil_fusion_amd.estimator import ScanContext
    sc = ScanContext(solver, capacity=capacity or len(clouds), **over)
    assert sc.add_many(clouds) == 0 and len(sc) == len(clouds)
    return sc


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _compare(got, ref, what):
    assert len(got) == len(ref)
    worst = 0.0
    for k, (g, r) in enumerate(zip(got, ref)):
        for f in ("loop_id", "nearest", "shift", "n_candidates", "candidates"):
            assert g[f] == r[f], (what, k, f, g, {f: r[f] for f in g})
        assert abs(g["min_dist"] - r["min_dist"]) <= 1e-12, (what, k, g["min_dist"], r["min_dist"])
        assert np.float32(g["yaw_diff_rad"]) == np.float32(r["yaw_diff_rad"]), (what, k)
        worst = max(worst, abs(g["min_dist"] - r["min_dist"]))
    return worst


def _raw_rows(solver, first, n):
    """vilf_sc_detect_range as bytes per row, the struct's tail padding left out"""
    arr = (abi.ScResult * n)()
    solver._check(solver._L.vilf_sc_detect_range(solver._h, int(first), int(n), arr), "vilf_sc_detect_range")
    return [bytes(arr[i])[:ROW_BYTES] for i in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("S", STRIDE_SIZES)
def test_strided_candidates_planted_winner(solver, S):
    """exhaustive mode beyond the 256 slots of a query: a wave meets a second and a third candidate, sc_reduce goes round its lane loop four times"""
    for place, maps, ref in _stride_cases(S):
        sc = _sc(solver, _clouds(maps), dist_thres=0.5, **EXH)
        _compare(sc.detect_range(S, 1), [ref], f"snapshot {S}, plant at {place}")


@pytest.mark.gpu
def test_mixed_snapshot_sizes_in_one_launch(solver):
    """one launch for queries that see 60 to 260 entries (gridDim.y and the slot count follow the last) against one launch per query (they follow that query)"""
    maps, ref = _mixed_case()
    sc = _sc(solver, _clouds(maps), dist_thres=0.5, **EXH)
    rows = _raw_rows(solver, 60, 201)
    for k in range(60, 261):
        assert _raw_rows(solver, k, 1)[0] == rows[k - 60], k
    got = sc.detect_range(60, 201)
    assert [o["n_candidates"] for o in got] == list(range(60, 261))
    _compare([got[k - 60] for k in ref], list(ref.values()), "mixed sizes")


@pytest.mark.gpu
def test_candidate_ties_go_to_the_lower_place(solver):
    for places, third, maps, ref in _tie_cases():
        sc = _sc(solver, _clouds(maps), dist_thres=0.5, **EXH)
        _compare(sc.detect_range(519, 1), [ref], f"plants at {places}, a worse one at {third}")


@pytest.mark.gpu
def test_reference_mode_tie_goes_to_the_place_not_the_index(solver):
    for plain, scaled, maps, ref in _place_cases():
        sc = _sc(solver, _clouds(maps), **PLACE)
        got = sc.detect_range(12, 1)
        _compare(got, [ref], f"A at {plain}, 2 A at {scaled}")
        assert got[0]["nearest"] == plain


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 3, 16])
def test_ring_key_top_k_ties_and_sizes(solver, k):
    for e1, e2, straddle, maps, ref in _topk_cases(k):
        sc = _sc(solver, _clouds(maps), num_exclude_recent=1, tree_making_period=1, num_candidates=k, dist_thres=0.5)
        _compare(sc.detect_range(200, 1), [ref], f"k {k}, equal keys at {e1} and {e2}, {'across' if straddle else 'inside'} the cut")
    maps, ref = _same_key_case(k)
    sc = _sc(solver, _clouds(maps), num_exclude_recent=1, tree_making_period=1, num_candidates=k, dist_thres=0.5)
    assert all(_same_bits(sc.get(i)[1], R.ring_key(maps[i])) for i in (0, 1, 64, 200))
    got = sc.detect_range()
    _compare([got[q] for q in ref], list(ref.values()), f"k {k}, one ring key for all")
    _compare(sc.detect_range(65, 1) + sc.detect_range(200, 1), [ref[65], ref[200]], f"k {k}, one ring key for all, single queries")


@pytest.mark.gpu
@pytest.mark.parametrize("ratio,radius", SHIFT_RATIOS)
def test_shift_windows(solver, ratio, radius):
    maps, over, ref = _shift_case(ratio, radius)
    sc = _sc(solver, _clouds(maps), **over)
    _compare(sc.detect_range(), ref, f"search_ratio {ratio}")


@pytest.mark.gpu
def test_symmetric_candidate_takes_the_lower_shift(solver):
    for rot, maps, over, ref in _symmetric_cases():
        sc = _sc(solver, _clouds(maps), **over)
        got = sc.detect_range(1, 1)
        _compare(got, [ref], f"symmetric candidate, rotation {rot}, {over}")
        assert got[0]["shift"] < 30


@pytest.mark.gpu
@pytest.mark.parametrize("exclude,period", SCHEDULES)
def test_snapshot_schedules(solver, exclude, period):
    over, ref = _schedule_case(exclude, period)
    maps = _schedule_maps()
    sc = _sc(solver, _clouds(maps), **over)
    for i in range(0, 140, 9):                                    # builder clouds: the same descriptor and ring-key bits on both sides
        d, rk, _ = sc.get(i)
        assert _same_bits(d, maps[i]) and _same_bits(rk, R.ring_key(maps[i])), i
    _compare(sc.detect_range(), ref, f"num_exclude_recent {exclude}, tree_making_period {period}")


@pytest.mark.gpu
def test_irregular_detect_schedule(solver):
    from vil_fusion_amd.estimator import ScanContext
    maps, detects, ref = _irregular_case()
    sc = ScanContext(solver, capacity=len(maps), **IRREGULAR)
    got = []
    for k, c in enumerate(_clouds(maps)):
        assert sc.makeAndSaveScancontextAndKeys(c) == k
        for _ in range(detects[k]):
            sc.detectLoopClosureID()
            got.append(sc.last)
    _compare(got, ref, "irregular schedule of vilf_sc_detect")


@pytest.mark.gpu
def test_descriptor_edges_unfiltered(solver):
    p = R.Params()
    cases = _descriptor_edge_clouds()
    sc = _sc(solver, list(cases.values()))
    for i, (name, cloud) in enumerate(cases.items()):
        want = R.make_descriptor(cloud, p)
        d, rk, sk = sc.get(i)
        diff = np.argwhere(d != want)
        print(f"{name}: {len(cloud)} points, {np.count_nonzero(want)} bins, {len(diff)} bins differ")
        assert _same_bits(d, want), (name, diff[:5], d[tuple(diff[0])], want[tuple(diff[0])])
        rw, sw = R.ring_key(want), R.sector_key(want)
        assert rk.dtype == np.float32 and np.all(np.abs(rk.astype(np.float64) - rw.astype(np.float64)) <= np.spacing(np.abs(rw)).astype(np.float64)), name
        assert np.all(np.abs(sk - sw) <= 1e-15 * np.abs(sw)), name
    clouds, ref = _zero_height_case()
    sc = _sc(solver, clouds, dist_thres=0.5, **EXH)
    assert _same_bits(sc.get(1)[0], R.make_descriptor(clouds[1], p))
    _compare(sc.detect_range(), ref, "columns that hold only heights of 0.0")


@pytest.mark.gpu
def test_empty_descriptors(solver):
    for name, clouds, over, at, ref in _empty_cases():
        sc = _sc(solver, clouds, **over)
        _compare(sc.detect_range(at, 1), [ref], name)


def _bad_creations():
    bad = [("capacity", 0, abi.VILF_ERR_INVALID_ARGUMENT), ("num_rings", 16, abi.VILF_ERR_UNSUPPORTED)]
    bad += [(f, v, abi.VILF_ERR_INVALID_ARGUMENT) for f, vs in (("max_radius", (0.0, math.nan, math.inf)), ("lidar_height", (math.nan,)), ("num_exclude_recent", (0,)),
                                                                 ("num_candidates", (-1, 17)), ("search_ratio", (-0.1, 1.1, math.nan)), ("dist_thres", (math.nan,)),
                                                                 ("tree_making_period", (0,))) for v in vs]
    return bad


@pytest.mark.gpu
def test_refused_creation_leaves_the_database_alone(solver):
    from vil_fusion_amd.estimator import ScanContext, sc_default_params
    over = dict(num_exclude_recent=2, tree_making_period=5, num_candidates=0, search_ratio=1.0, dist_thres=0.5)
    clouds = _clouds(K.database(8, seed=41, plants={6: (1, 9, 0.2)}))
    sc = ScanContext(solver, capacity=8, **over)
    m = R.SCManager(R.Params(**over))
    got, ref = [], []
    for c in clouds[:6]:
        sc.makeAndSaveScancontextAndKeys(c); m.add(c)
        sc.detectLoopClosureID(); got.append(sc.last); ref.append(m.detect())
    assert m.calls == 4                                           # not a multiple of the period: the next detect keeps the snapshot of the first
    before = sc.get(3)
    assert len(_bad_creations()) == 14
    for field, value, code in _bad_creations():
        p = sc_default_params(**over)
        capacity = 8
        if field == "capacity":
            capacity = value
        else:
            setattr(p, field, value)
        assert solver._L.vilf_sc_create(solver._h, C.byref(p), capacity) == code, (field, value)
        assert len(sc) == 6, (field, value)
    assert all(_same_bits(a, b) for a, b in zip(before, sc.get(3)))
    sc.makeAndSaveScancontextAndKeys(clouds[6]); m.add(clouds[6])
    sc.detectLoopClosureID(); got.append(sc.last); ref.append(m.detect())
    assert ref[-1]["snapshot"] == 1 and ref[-1]["n_candidates"] == 1 and len(m.descs) - 2 == 5          # a counter back at 0 would have rebuilt it: 5 entries
    _pre(ref[2:], 0.5)
    _compare(got, ref, "detect around refused creations")
    assert solver._L.vilf_sc_create(solver._h, C.byref(sc_default_params(dist_thres=math.inf)), 1) == abi.VILF_OK and len(sc) == 0      # +inf is accepted


@pytest.mark.gpu
def test_device_min_dist_within_the_derived_bound_of_exact(solver):
    """query k of the exhaustive replay against the exact minimum over every (candidate j < k, shift); each device distance is within BOUND_KERNEL of the exact one, so
    the minima are too"""
    clouds, descs, pairs, exact = _exact_set()
    sc = _sc(solver, clouds, dist_thres=0.5, **EXH)
    assert all(_same_bits(sc.get(i)[0], descs[i]) for i in range(len(descs)))
    got = sc.detect_range()
    worst = 0.0
    skipped = 0
    for k in range(1, len(descs)):
        every = sorted((exact[k, j][1][s], j, s) for j in range(k) for s in range(60) if exact[k, j][1][s] is not None)
        err = abs(float(X.MP.mpf(got[k]["min_dist"]) - every[0][0]))
        worst = max(worst, err)
        print(f"query {k}: device min_dist {got[k]['min_dist']:.17g}, error {err / U:.2f} u")
        assert err <= BOUND_KERNEL, (k, err / U)
        if float(every[1][0] - every[0][0]) > 2 * BOUND_KERNEL:
            assert (got[k]["nearest"], got[k]["shift"]) == every[0][1:], (k, got[k], every[0])
        else:
            skipped += 1
    print(f"device against exact: {len(descs) - 1} queries over {len(pairs)} pairs, worst error {worst / U:.2f} u, bound {BOUND_KERNEL / U:.0f} u, "
          f"{skipped} argmin comparisons skipped")
    assert skipped == 0
