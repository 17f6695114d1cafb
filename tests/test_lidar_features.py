"""LOAM feature extraction (featureExtraction.hpp:54-232) — oracle pins on CPU, HIP-vs-oracle parity on the GPU."""
import numpy as np
import pytest
from vil_fusion_amd import synth


def _raw_scan(seed, rings=64, n_poles=80):
    scene = synth.LidarScene(seed, n_poles=n_poles, rings=rings)
    R = synth.euler_R(np.array(0.1 * seed), np.array(0.0), np.array(0.0)); t = np.array([-20.0 + seed, 3.0, scene.h])
    return scene, R, t, scene.scan_raw(R, t)


def test_oracle_feature_extraction_invariants(oracle):
    scene, R, t, raw = _raw_scan(5)
    e, s = oracle.extract_features(raw)
    assert len(e) > 100 and len(s) > 1000
    # every output point is an input point, edge and surf are disjoint, at most 20 edges per (ring, sector)
    key = lambda a: {tuple(p) for p in a.view(np.uint32).reshape(-1, 4)[:, :3].tolist()}
    ke, ks, kr = key(e), key(s), key(raw)
    assert ke <= kr and ks <= kr and not (ke & ks)
    assert len(e) <= 64 * 6 * 20
    # a flat wall-less ground patch (smooth rings) must yield no edges at a generous threshold: curvature of noise-free rings is tiny
    scene2 = synth.LidarScene(1, n_poles=0, noise=0.0)
    raw2 = scene2.scan_raw(np.eye(3), np.array([0.0, 0.0, scene2.h]))
    ground = raw2[np.abs(raw2[:, 2] + scene2.h) < 1e-3]                 # ground returns only (sensor at height h)
    rad = np.linalg.norm(ground[:, :2], axis=1)
    near = ground[(rad > 5.0) & (rad < 30.0)]        # (the lowest beam sits exactly on the -24.33 deg cut of the ring model: skip it)
    e2, s2 = oracle.extract_features(near, edge_threshold=1.0)
    assert len(e2) == 0 and len(s2) > 0
    # empty and tiny inputs
    e3, s3 = oracle.extract_features(np.zeros((0, 4), dtype=np.float32))
    assert len(e3) == 0 and len(s3) == 0
    e4, s4 = oracle.extract_features(raw[:100])
    assert len(e4) == 0 and len(s4) == 0                                  # every ring has fewer than 131 points


@pytest.mark.gpu
@pytest.mark.parametrize("seed,rings", [(5, 64), (7, 64), (3, 32), (4, 16)])
def test_hip_feature_extraction_matches_oracle(oracle, opts, seed, rings):
    """Ring assignment, curvature, per-sector sort and picks on the device: the edge and surf clouds must be bit-identical to the
    oracle's, in the same order. Includes NaN returns and out-of-range points."""
    from vil_fusion_amd.estimator import BackendSolver, FeatureExtraction
    _, _, _, raw = _raw_scan(seed, rings=rings)
    raw = raw.copy()
    raw[::997, 0] = np.nan                                                # pcl::removeNaNFromPointCloud only indexes: NaNs fall out by the range / ring tests
    raw[5::1013, :2] *= 100.0                                             # beyond lidarMaxRange
    s = BackendSolver(opts)
    fe = FeatureExtraction(s, n_scans=rings)
    ge, gs = fe.extractFeature(raw)
    re_, rs = oracle.extract_features(raw, n_scans=rings)
    assert ge.shape == re_.shape and gs.shape == rs.shape
    assert np.array_equal(ge.view(np.uint32), re_.view(np.uint32)) and np.array_equal(gs.view(np.uint32), rs.view(np.uint32))
    # a second, different scan through the same handle (workspace re-use) and an empty scan
    _, _, _, raw2 = _raw_scan(seed + 20, rings=rings)
    ge2, gs2 = fe.extractFeature(raw2[: len(raw2) // 2])
    re2, rs2 = oracle.extract_features(raw2[: len(raw2) // 2], n_scans=rings)
    assert np.array_equal(ge2.view(np.uint32), re2.view(np.uint32)) and np.array_equal(gs2.view(np.uint32), rs2.view(np.uint32))
    ge3, gs3 = fe.extractFeature(np.zeros((0, 4), dtype=np.float32))
    assert len(ge3) == 0 and len(gs3) == 0
    s.close()


def _depth_case(seed, opts):
    """camera-frame depth cloud from a raw scan (points in front of the camera, inside its field of view) + normalised features"""
    _, _, _, raw = _raw_scan(seed)
    RCL = np.array(opts.RCL[:]).reshape(3, 3); TCL = np.array(opts.TCL[:])
    pc = raw[:, :3].astype(np.float64) @ RCL.T + TCL                          # camera <- LiDAR
    front = (pc[:, 2] > 1.0) & (np.abs(pc[:, 0] / pc[:, 2]) < 0.9) & (np.abs(pc[:, 1] / pc[:, 2]) < 0.3)
    cloud = np.column_stack([pc[front], np.ones(front.sum())]).astype(np.float32)
    rng = np.random.default_rng(seed)
    feats = np.column_stack([rng.uniform(-0.85, 0.85, 200), rng.uniform(-0.25, 0.25, 200), np.ones(200)]).astype(np.float32)
    return cloud, feats


def test_oracle_feature_depth(oracle, opts):
    cloud, feats = _depth_case(5, opts)
    assert len(cloud) > 1000
    d = oracle.feature_depth(cloud, feats)
    ok = d > 0
    assert 20 < ok.sum() < 200 and np.all(d[ok] > 2.0) and np.all(d[~ok] == -1.0)
    # a fronto-parallel wall at z = 10: every feature that gets a depth gets ~10
    gx, gy = np.meshgrid(np.linspace(-9, 9, 300), np.linspace(-3, 3, 100))
    wall = np.column_stack([gx.ravel(), gy.ravel(), np.full(gx.size, 10.0), np.ones(gx.size)]).astype(np.float32)
    dw = oracle.feature_depth(wall, feats)
    assert (dw > 0).sum() > 150 and np.allclose(dw[dw > 0], 10.0, atol=1e-3)
    assert np.all(oracle.feature_depth(wall[:9], feats) == -1.0)           # fewer than 10 points: no depth at all


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [5, 8])
def test_hip_feature_depth_matches_oracle(oracle, opts, seed):
    from vil_fusion_amd.estimator import BackendSolver, FeatureExtraction
    cloud, feats = _depth_case(seed, opts)
    s = BackendSolver(opts); fe = FeatureExtraction(s)
    got = fe.getFeatureDepth(cloud, feats)
    ref = oracle.feature_depth(cloud, feats)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), "depths must be bit-identical"
    assert np.all(fe.getFeatureDepth(cloud[:9], feats) == -1.0)
    dup = np.concatenate([cloud[:50], cloud[:50], cloud])                   # exact duplicates: ties resolved by index
    assert np.array_equal(fe.getFeatureDepth(dup, feats).view(np.uint32), oracle.feature_depth(dup, feats).view(np.uint32))
    s.close()


# ====================================================================================================================================
# The stage against an independent statement of it (tests/feat_reference.py, written from the reference's text) on designed inputs
# (tests/feat_cases.py). CPU: the oracle is held to the restatement bit for bit, and the restatement's own report proves that each
# input hits what it was built for. GPU: the device is held to both. DESIGN.md 3k has the figures and the mutations these catch.
# ====================================================================================================================================
import collections
import ctypes as C

import feat_cases as cases
import feat_reference as fref
from vil_fusion_amd import abi

_FP = C.POINTER(C.c_float)
UNSUPPORTED_MESSAGE = "feature extraction: a sector holds more than 1024 points (ring with more than ~6150 returns)"


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _scan_case(seed, rings):
    raw = _raw_scan(seed, rings=rings)[3].copy()
    raw[::997, 0] = np.nan
    raw[5::1013, :2] *= 100.0
    return raw


# name -> (cloud, keyword arguments of extract): the four synthetic scans of the parity test and every designed input
EXTRACT_CASES = {
    "scan5_64": (lambda: _scan_case(5, 64), dict(n_scans=64)),
    "scan7_64": (lambda: _scan_case(7, 64), dict(n_scans=64)),
    "scan3_32": (lambda: _scan_case(3, 32), dict(n_scans=32)),
    "scan4_16": (lambda: _scan_case(4, 16), dict(n_scans=16)),
    "sectors": (cases.sector_cloud, dict(n_scans=16)),
    "sectors_all_candidates": (cases.sector_cloud, dict(n_scans=16, edge_thr=-1.0)),
    "sectors_no_candidate": (cases.sector_cloud, dict(n_scans=16, edge_thr=1e300)),
    "sectors_as_32": (cases.sector_cloud, dict(n_scans=32)),
    "all_rejected": (cases.rejected_cloud, dict(n_scans=16)),
    "one_ring": (cases.one_ring_cloud, dict(n_scans=16)),
    "ties": (cases.tie_ring_cloud, dict(n_scans=16)),
    "ties_all_candidates": (cases.tie_ring_cloud, dict(n_scans=16, edge_thr=-1.0)),
    "identical": (cases.identical_ring_cloud, dict(n_scans=16)),
    "identical_all_candidates": (cases.identical_ring_cloud, dict(n_scans=16, edge_thr=-1.0)),
    "corners": (cases.corner_ring_cloud, dict(n_scans=16)),
    "gaps": (cases.gap_ring_cloud, dict(n_scans=16)),
    "gap_of_exactly_0.05": (cases.exact_gap_ring_cloud, dict(n_scans=16)),
    "ring_of_130": (lambda: cases.one_ring_cloud()[:130], dict(n_scans=16)),
    "ring_of_131": (lambda: cases.one_ring_cloud()[:131], dict(n_scans=16, edge_thr=-1.0)),
}
_restated = {}


def _restatement(name):
    """the restatement's result for a case, computed once and shared"""
    if name not in _restated:
        make, kw = EXTRACT_CASES[name]
        _restated[name] = (make(), fref.extract(make(), **kw))
    return _restated[name]


def _oracle_kw(kw):
    return {{"edge_thr": "edge_threshold"}.get(k, k): v for k, v in kw.items()}


@pytest.mark.parametrize("name", list(EXTRACT_CASES))
def test_oracle_extraction_is_the_restatement(oracle, name):
    """edge cloud, surf cloud and their order: the oracle and the numpy restatement of featureExtraction.hpp agree bit for bit"""
    cloud, ref = _restatement(name)
    e, s = oracle.extract_features(cloud, **_oracle_kw(EXTRACT_CASES[name][1]))
    print(f"{name}: {len(cloud)} points -> edge {len(e)} / {len(ref['edge'])}, surf {len(s)} / {len(ref['surf'])}")
    assert _bits_equal(e, ref["edge"]), "edge cloud"
    assert _bits_equal(s, ref["surf"]), "surf cloud"


def test_designed_clouds_hit_what_they_were_built_for():
    """the restatement's report on the designed inputs: sector sizes, ties, the 21st pick, thresholds, halo, gaps"""
    # sector sizes: every m at which fe_sector changes its path occurs, 1024 in all six sectors of the big ring
    cloud, ref = _restatement("sectors")
    assert len(cloud) <= 25000
    cnt = collections.Counter(ref["rings"].tolist())
    assert {r: cnt.get(r, 0) for r in range(16)} == {r: cases.SECTOR_RINGS.get(r, 0) for r in range(16)}
    assert cnt[-1] == 200 and cnt[0] == 0 and cnt[15] == 6160 and cnt[2] == 130
    ms = collections.defaultdict(list)
    for sec in ref["sectors"]:
        ms[sec["ring"]].append(sec["m"])
    assert dict(ms) == {r: cases.sector_m(c) for r, c in cases.SECTOR_RINGS.items() if c >= 131}        # the ring of 130 is skipped
    assert {m for v in ms.values() for m in v} == set(cases.SECTOR_M_WANTED) and ms[15] == [1024] * 6 and ms[1] == [19] * 5 + [20]
    assert sum(sec["lost"] is not None for sec in ref["sectors"]) >= 10                       # the 21st pick happens on ordinary data too
    assert cases.sector_m(6161)[5] == 1025
    # every point a candidate: 20 edges wherever 21 picks fit, the 21st in neither cloud; no candidate: everything is surf
    _, allc = _restatement("sectors_all_candidates")
    big = [sec for sec in allc["sectors"] if sec["m"] >= 255]
    assert len(big) == 36 and all(len(sec["edges"]) == 20 and sec["lost"] is not None and not sec["by_threshold"] for sec in big)
    assert all(sec["lost"] not in sec["edges"] and sec["lost"] not in sec["surf"] for sec in big)
    assert len(allc["edge"]) + len(allc["surf"]) < sum(sec["m"] for sec in allc["sectors"])
    _, none = _restatement("sectors_no_candidate")
    assert len(none["edge"]) == 0 and len(none["surf"]) == sum(sec["m"] for sec in none["sectors"])
    assert all(sec["by_threshold"] and sec["surf"] == sorted(sec["surf"], key=lambda j: (none["curv"][sec["ring"]][j - 5], j)) for sec in none["sectors"])
    _, rej = _restatement("all_rejected")
    assert set(rej["rings"].tolist()) == {-1} and not rej["sectors"]
    _, one = _restatement("one_ring")
    assert set(one["rings"].tolist()) == {7} and len(one["sectors"]) == 6 and len(one["edge"]) > 0
    assert not _restatement("ring_of_130")[1]["sectors"]
    r131 = _restatement("ring_of_131")[1]
    assert [sec["m"] for sec in r131["sectors"]] == [19] * 5 + [20]
    # ties: hundreds of exactly equal curvatures in sectors above 512, also among the picks
    _, tie = _restatement("ties")
    assert all(sec["m"] > 512 and sec["ties"] >= 100 for sec in tie["sectors"]) and len(tie["sectors"]) == 6
    cv = tie["curv"][8]
    assert any(cv[a - 5] == cv[b - 5] for sec in tie["sectors"] for a, b in zip(sec["edges"], sec["edges"][1:]))        # a tie decides the pick order
    # identical points: curvature exactly 0, no edge, surf in index order; with every point a candidate the picks walk down from the
    # last kept element and the suppression leaves the sector on both sides
    _, ident = _restatement("identical")
    assert all(np.all(v == 0.0) for v in ident["curv"].values()) and len(ident["edge"]) == 0
    assert all(sec["m"] == 64 and sec["surf"] == list(range(sec["first"], sec["last"] + 1)) for sec in ident["sectors"])
    _, ida = _restatement("identical_all_candidates")
    for sec in ida["sectors"]:
        assert sec["edges"][0] == sec["last"] and sec["edges"][:3] == [sec["last"], sec["last"] - 6, sec["last"] - 12] and sec["lost"] is None
        assert max(sec["picked"]) == sec["last"] + 5 and min(sec["picked"]) < sec["first"] and not sec["surf"]
    # corners at the sector ends: picked where kept, invisible where dropped, suppression reaches into the halo and stays local
    _, cor = _restatement("corners")
    by = {sec["sector"]: sec for sec in cor["sectors"]}
    last0, dropped1, near2, near4 = cases.CORNER_AT
    assert by[0]["edges"] == [last0] and by[0]["last"] == last0 and by[1]["dropped"] == dropped1 and by[1]["edges"] == [] and by[3]["edges"] == [] and by[5]["edges"] == []
    assert by[2]["edges"] == [near2] and by[2]["last"] == near2 + 2 and by[4]["edges"] == [near4] and by[4]["first"] == near4 - 2
    assert all(j in by[0]["picked"] and j in by[1]["surf"] for j in range(by[1]["first"], by[1]["first"] + 4))       # picked in sector 0's list, surf of sector 1
    assert all(j in by[2]["picked"] and j in by[3]["surf"] for j in (by[3]["first"], by[3]["first"] + 1))
    assert all(j in by[4]["picked"] and j in by[3]["surf"] for j in (by[3]["last"] - 1, by[3]["last"]))
    assert all(dropped1 not in sec["surf"] and dropped1 not in sec["edges"] for sec in cor["sectors"])
    assert len(cor["edge"]) == 3
    # gaps: the first pick of sector k suppresses 5 - k returns after it and k before it
    _, gap = _restatement("gaps")
    assert [(sec["fwd"][0], sec["bwd"][0]) for sec in gap["sectors"]] == [(5 - k, k) for k in range(6)]
    assert {n for sec in gap["sectors"] for n in sec["fwd"]} >= set(range(6)) and {n for sec in gap["sectors"] for n in sec["bwd"]} >= set(range(6))
    # a step whose squared length is exactly the double 0.05 is no gap: the suppression walks across it
    cloud, exact = _restatement("gap_of_exactly_0.05")
    g = cases.EXACT_GAP_AT
    assert set(exact["rings"].tolist()) == {8} and fref._gap2(cloud, g + 1, g) == np.float64(0.05)
    sec = exact["sectors"][2]
    assert sec["first"] < g < sec["last"] and sec["edges"][0] in (g, g + 1) and g in sec["picked"] and g + 1 in sec["picked"]
    assert sec["fwd"][0] == 5 and sec["bwd"][0] == 5


# ---- ring assignment ---------------------------------------------------------------------------------------------------------------
RING_MARGIN_FACTOR = 64          # the probes must be decided by 64 x the double evaluation's own deviation from the exact t (the device's atan is looser than glibc's)
_probe_truth = {}


def _ring_probe_truth(n_scans):
    if n_scans not in _probe_truth:
        pts, labels = cases.ring_probes(n_scans)
        _probe_truth[n_scans] = (pts, labels) + fref.ring_exact(pts, n_scans)
    return _probe_truth[n_scans]


def _ring_margin():
    return RING_MARGIN_FACTOR * max(_ring_probe_truth(ns)[4].max() for ns in (16, 32, 64))


@pytest.mark.parametrize("n_scans", [16, 32, 64])
def test_ring_probes_are_decided_and_oracle_is_exact(oracle, n_scans):
    """every probe around every decision of the ring model lies further from it than the margin (so the exact ring is the only right
    answer for any evaluation that accurate); the numpy ring_of and the oracle's vilo_lidar_rings give the exact ring on all of them"""
    pts, labels, ring, dist, terr = _ring_probe_truth(n_scans)
    margin = _ring_margin()
    worst = int(dist.argmin())
    print(f"n_scans {n_scans}: {len(pts)} probes at {len(set(labels))} decisions; max |t_double - t_exact| {terr.max():.3e}; margin {margin:.3e}; "
          f"smallest distance to a decision {dist[worst]:.3e} ({labels[worst]}, point {pts[worst, :3].tolist()})")
    assert len(pts) == 17 * len(cases.PROBE_XY) * len(cases.ring_boundaries(n_scans))
    assert dist.min() > margin, (labels[worst], pts[worst], dist[worst], margin)
    at_decision = np.array([l != "upper t=33 behind the seam" for l in labels])
    assert dist[at_decision].max() < 1e-4                                 # and they are probes: all within a few float32 steps of a decision
    for label in set(labels):                                             # each decision is seen from both sides
        sides = {int(r) for r, l in zip(ring, labels) if l == label}
        if label == "t=0":
            assert sides == {0}, sides                                    # truncation toward zero: t in (-1, 0) is ring 0 as well
        elif n_scans == 64 and label in ("upper t=-1", "upper t=0", "lower t=32"):
            assert sides == {-1}, (label, sides)                          # beyond the cuts at 2 and -24.33: rejected on both sides
        elif n_scans == 64 and label in ("seam -8.83", "upper t=33 behind the seam"):
            assert sides == {32}, (label, sides)                          # both formulas give ring 32 at the seam; the upper one's next step lies behind it
        else:
            assert len(sides) == 2, (label, sides)
    assert set(ring.tolist()) == set(range(-1, n_scans))                  # every ring and the rejection occur
    assert np.array_equal(fref.ring_of(pts, n_scans), ring)
    assert np.array_equal(oracle.lidar_rings(pts, n_scans), ring)


def test_oracle_range_gate_and_non_finite_points(oracle):
    seen = set()
    for pts, lo, hi in cases.gate_probes():
        want = fref.ring_of(pts, 16, lo, hi)
        assert np.array_equal(oracle.lidar_rings(pts, 16, lo, hi), want)
        seen |= set(want.tolist())
    pts, lo, hi = cases.gate_probes()[0]
    want = fref.ring_of(pts, 16, lo, hi)
    assert want[0] == 8 and want[3] == -1 and want[6] == 8               # dxy == min_range is accepted, its lower neighbour is not
    assert want[9] == 8                                                   # dxy == max_range (60, 80) is accepted
    assert want[30] == -1 and want[24] == 8                               # the upper neighbour of 100 is rejected
    assert np.all(want[39:45] == -1)                                      # z = NaN, x = +-inf, x = NaN, y = NaN
    assert len(seen) > 3


# ---- depth -------------------------------------------------------------------------------------------------------------------------
def _depth_cases():
    out = {f"n{n}": cases.depth_sized(n) for n in (9, 10, 11, 255, 256, 257, 1000)}
    out.update({f"usable{k}": cases.depth_usable(k) for k in range(4)})
    clouds, feats = cases.depth_ties()
    out.update({"mirror_3rd_4th": (clouds[0], feats), "mirror_4th_3rd": (clouds[1], feats), "duplicate_3rd_4th": (clouds[2], feats)})
    out["exits"] = cases.depth_exits()
    cloud, feats = cases.depth_sized(1000)
    out["m0"] = (cloud, feats[:0]); out["m1"] = (cloud, feats[:1]); out["m1000"] = (cloud, np.tile(feats, (25, 1)) * np.linspace(0.5, 2.0, 1000, dtype=np.float32)[:, None])
    zf = feats.copy(); zf[::4] = 0.0; zf[1::4, 0] = np.nan
    out["zero_feature"] = (cloud, zf)
    return out


DEPTH_CASES = ["n9", "n10", "n11", "n255", "n256", "n257", "n1000", "usable0", "usable1", "usable2", "usable3", "mirror_3rd_4th", "mirror_4th_3rd", "duplicate_3rd_4th",
               "exits", "m0", "m1", "m1000", "zero_feature"]
_depth_restated = {}


def _depth_restatement(name):
    if not _depth_restated:
        for k, (cloud, feats) in _depth_cases().items():
            _depth_restated[k] = (cloud, feats) + fref.feature_depth(cloud, feats)
        assert list(_depth_restated) == DEPTH_CASES
    return _depth_restated[name]


@pytest.mark.parametrize("name", DEPTH_CASES)
def test_oracle_depth_is_the_restatement(oracle, name):
    cloud, feats, depth, exits, clamps = _depth_restatement(name)
    got = oracle.feature_depth(cloud, feats)
    print(f"{name}: n {len(cloud)}, m {len(feats)}, exits {dict(collections.Counter(exits))}, clamps {dict(collections.Counter(clamps))}")
    assert _bits_equal(got, depth)


def test_designed_depth_clouds_hit_what_they_were_built_for():
    ex = lambda name: collections.Counter(_depth_restatement(name)[3])
    assert ex("n9") == {"few": 40} and "few" not in ex("n10") and ex("n10")["ok"] >= 20 and ex("n11")["ok"] >= 20
    for n in (255, 256, 257, 1000):
        assert ex(f"n{n}")["ok"] >= 35
    for k in range(3):
        assert ex(f"usable{k}") == {"no3": 40}                           # 0, 1, 2 points with a distance: every feature returns -1
        assert np.all(_depth_restatement(f"usable{k}")[2] == -1.0)
    assert "no3" not in ex("usable3") and ex("usable3")["ok"] >= 1
    a, b, d = (_depth_restatement(k)[2] for k in ("mirror_3rd_4th", "mirror_4th_3rd", "duplicate_3rd_4th"))
    assert np.all(a > 2) and np.all(b > 2) and np.all(a[:2] != b[:2])     # which of two equally distant points is third changes the depth ...
    assert _bits_equal(a, d)                                              # ... unless they are the same point
    cloud, feats = cases.depth_ties()[0][0], cases.depth_ties()[1]
    with np.errstate(all="ignore"):
        u = cloud[:, :3] / np.sqrt(cloud[:, 0] ** 2 + cloud[:, 1] ** 2 + cloud[:, 2] ** 2)[:, None]
        dd = ((u - np.array([0, 0, 1], dtype=np.float32)) ** 2).sum(axis=1)
    assert dd[2] == dd[3] and np.all(dd[4:] > dd[3]) and np.all(dd[:2] < dd[2])
    assert ex("m0") == {} and len(ex("m1")) == 1 and sum(ex("m1000").values()) == 1000
    zexits = _depth_restatement("zero_feature")[3]
    assert all(e == "no3" for e in zexits[::4]) and all(e == "no3" for e in zexits[1::4]) and "ok" in zexits
    _, _, _, exits, clamps = _depth_restatement("exits")
    cnt, ccnt = collections.Counter(exits), collections.Counter(clamps)
    print("exits", dict(cnt), "clamps", dict(ccnt))
    for e in ("threshold", "spread", "s_small", "low", "ok"):
        assert cnt[e] >= 5, (e, cnt)
    assert ccnt["max"] >= 5 and ccnt["min"] >= 5
    assert sum(1 for e, c in zip(exits, clamps) if e == "ok" and c is None) >= 5


# ---- calls -------------------------------------------------------------------------------------------------------------------------
def test_oracle_capacities(oracle):
    """counts in full, only `cap` points written, a negative capacity refused"""
    L = oracle.lib()
    L.vilo_extract_features.argtypes = [_FP, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, _FP, C.c_int, C.POINTER(C.c_int), _FP, C.c_int, C.POINTER(C.c_int)]
    cloud, ref = _restatement("one_ring")
    for ce, cs in ((7, 100), (0, 0), (len(ref["edge"]), len(ref["surf"]))):
        e = np.full((len(cloud), 4), -7.0, dtype=np.float32); s = np.full((len(cloud), 4), -7.0, dtype=np.float32)
        ne, ns = C.c_int(-1), C.c_int(-1)
        assert L.vilo_extract_features(cloud.ctypes.data_as(_FP), len(cloud), 16, 3.0, 100.0, 0.1, e.ctypes.data_as(_FP), ce, C.byref(ne), s.ctypes.data_as(_FP), cs, C.byref(ns)) == 0
        assert (ne.value, ns.value) == (len(ref["edge"]), len(ref["surf"]))
        assert _bits_equal(e[:ce], ref["edge"][:ce]) and _bits_equal(s[:cs], ref["surf"][:cs]) and np.all(e[ce:] == -7.0) and np.all(s[cs:] == -7.0)
    for ce, cs in ((-1, 10), (10, -1), (-2 ** 31, -2 ** 31)):
        ne, ns = C.c_int(0), C.c_int(0)
        assert L.vilo_extract_features(cloud.ctypes.data_as(_FP), len(cloud), 16, 3.0, 100.0, 0.1, e.ctypes.data_as(_FP), ce, C.byref(ne), s.ctypes.data_as(_FP), cs, C.byref(ns)) == abi.VILF_ERR_INVALID_ARGUMENT


# ---- the device --------------------------------------------------------------------------------------------------------------------
class _Device:
    """a handle and the raw entry points, with explicit capacities"""

    def __init__(self, opts):
        from vil_fusion_amd.estimator import BackendSolver, FeatureExtraction
        self.s = BackendSolver(opts)
        self.fe = FeatureExtraction(self.s)
        self.L = self.s._L
        self.L.vilf_debug_lidar_rings.argtypes = [C.c_void_p, _FP, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_int)]

    def rings(self, pts, n_scans, lo=3.0, hi=100.0):
        a = np.ascontiguousarray(pts, dtype=np.float32)
        out = np.full(len(a), -99, dtype=np.int32)
        rc = self.L.vilf_debug_lidar_rings(self.s._h, a.ctypes.data_as(_FP), len(a), n_scans, lo, hi, out.ctypes.data_as(C.POINTER(C.c_int)))
        assert rc == 0, (rc, self.error())
        return out

    def extract_raw(self, cloud, n_scans=16, edge_thr=0.1, cap_edge=None, cap_surf=None, rows=None):
        """(rc, n_edge, n_surf, edge buffer, surf buffer): buffers of `rows` points pre-filled with a guard pattern"""
        a = np.ascontiguousarray(cloud, dtype=np.float32)
        n = len(a)
        rows = max(n, 1) if rows is None else rows
        e = np.full((rows, 4), -7.0, dtype=np.float32); s = np.full((rows, 4), -7.0, dtype=np.float32)
        ne, ns = C.c_int(-1), C.c_int(-1)
        rc = self.L.vilf_lidar_extract_features(self.s._h, a.ctypes.data_as(_FP), n, n_scans, 3.0, 100.0, edge_thr, e.ctypes.data_as(_FP), n if cap_edge is None else cap_edge,
                                                C.byref(ne), s.ctypes.data_as(_FP), n if cap_surf is None else cap_surf, C.byref(ns))
        return rc, ne.value, ns.value, e, s

    def extract(self, cloud, n_scans=16, edge_thr=0.1):
        rc, ne, ns, e, s = self.extract_raw(cloud, n_scans, edge_thr)
        assert rc == 0, (rc, self.error())
        return e[:ne].copy(), s[:ns].copy()

    def error(self):
        return self.L.vilf_last_error(self.s._h).decode()

    def close(self):
        self.s.close()


@pytest.fixture
def device(opts):
    d = _Device(opts)
    yield d
    d.close()


def _same_as_oracle_and_restatement(oracle, name, e, s):
    cloud, ref = _restatement(name)
    oe, os_ = oracle.extract_features(cloud, **_oracle_kw(EXTRACT_CASES[name][1]))
    assert _bits_equal(e, oe) and _bits_equal(s, os_), f"{name}: device against the oracle"
    assert _bits_equal(e, ref["edge"]) and _bits_equal(s, ref["surf"]), f"{name}: device against the restatement"


@pytest.mark.gpu
@pytest.mark.parametrize("n_scans", [16, 32, 64])
def test_hip_ring_probes_match_exact_ring(device, n_scans):
    """fe_ring through vilf_debug_lidar_rings: around every integer value of t, the accept / reject ends, the seam and the cuts of the
    64-ring model, the device's ring is the ring of 40-digit arithmetic. Every probe is decided by more than the margin (see
    test_ring_probes_are_decided_and_oracle_is_exact), so a wrong ring here is a wrong evaluation, not a coin toss."""
    pts, labels, ring, dist, terr = _ring_probe_truth(n_scans)
    assert dist.min() > _ring_margin()
    got = device.rings(pts, n_scans)
    bad = np.flatnonzero(got != ring)
    assert len(bad) == 0, [(labels[i], pts[i, :3].tolist(), int(got[i]), int(ring[i]), dist[i]) for i in bad[:10]]


@pytest.mark.gpu
def test_hip_range_gate_and_non_finite_points(device):
    for pts, lo, hi in cases.gate_probes():
        want = fref.ring_of(pts, 16, lo, hi)
        got = device.rings(pts, 16, lo, hi)
        assert np.array_equal(got, want), (got.tolist(), want.tolist())
    pts, lo, hi = cases.gate_probes()[0]
    for n_scans in (32, 64):
        assert np.array_equal(device.rings(pts, n_scans, lo, hi), fref.ring_of(pts, n_scans, lo, hi))


@pytest.mark.gpu
def test_hip_sector_sizes_and_refusal_above_1024(oracle, opts, device):
    """fe_sector at m = 19, 20, 255 .. 257, 511 .. 513, 1023 and 1024 (bitonic sort of 32, 256, 512 and 1024, one to four trips of the
    surf compaction), empty rings, a skipped ring of 130. Then m = 1025: refused with the documented message, and the handle goes on
    to give what a fresh handle gives."""
    e, s = device.extract(cases.sector_cloud(), 16)
    _same_as_oracle_and_restatement(oracle, "sectors", e, s)
    rc, ne, ns, eb, sb = device.extract_raw(cases.sector_cloud(6161), 16)
    assert rc == abi.VILF_ERR_UNSUPPORTED and device.error() == UNSUPPORTED_MESSAGE and (ne, ns) == (0, 0)
    assert np.all(eb == -7.0) and np.all(sb == -7.0)
    e2, s2 = device.extract(cases.sector_cloud(), 16)
    fresh = _Device(opts)
    e3, s3 = fresh.extract(cases.sector_cloud(), 16)
    fresh.close()
    assert _bits_equal(e2, e3) and _bits_equal(s2, s3) and _bits_equal(e2, e) and _bits_equal(s2, s)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [k for k in EXTRACT_CASES if not k.startswith("scan") and k != "sectors"])
def test_hip_designed_extraction(oracle, device, name):
    """ties, identical points, thresholds that every point or none passes, the 21st pick, corners at the sector ends, gaps, a cloud
    with no ring and one with a single ring: bit-identical to the oracle and to the restatement, in content and order"""
    cloud, _ = _restatement(name)
    kw = EXTRACT_CASES[name][1]
    e, s = device.extract(cloud, kw["n_scans"], kw.get("edge_thr", 0.1))
    _same_as_oracle_and_restatement(oracle, name, e, s)


@pytest.mark.gpu
def test_hip_capacities_and_guard(device):
    """capacities below the totals: counts in full, `cap` points written, the guard pattern behind them untouched; a negative
    capacity is refused before any device work"""
    cloud, ref = _restatement("one_ring")
    te, ts = len(ref["edge"]), len(ref["surf"])
    assert te > 7 and ts > 100
    for ce, cs in ((7, 100), (0, 0), (te, ts), (te - 1, ts + 5), (1, ts - 1)):
        rc, ne, ns, e, s = device.extract_raw(cloud, 16, cap_edge=ce, cap_surf=cs)
        assert rc == 0 and (ne, ns) == (te, ts)
        we, ws = min(ce, te), min(cs, ts)
        assert _bits_equal(e[:we], ref["edge"][:we]) and _bits_equal(s[:ws], ref["surf"][:ws])
        assert np.all(e[we:] == -7.0) and np.all(s[ws:] == -7.0)
    for ce, cs in ((-1, 10), (10, -1), (-2 ** 31, -2 ** 31)):
        rc, ne, ns, e, s = device.extract_raw(cloud, 16, cap_edge=ce, cap_surf=cs)
        assert rc == abi.VILF_ERR_INVALID_ARGUMENT and "negative" in device.error()
        assert np.all(e == -7.0) and np.all(s == -7.0)
    rc, ne, ns, e, s = device.extract_raw(cloud, 16)
    assert rc == 0 and _bits_equal(e[:ne], ref["edge"]) and _bits_equal(s[:ns], ref["surf"])


@pytest.mark.gpu
def test_hip_one_handle_changes_n_scans_and_runs_depth_between(oracle, device):
    """64 -> 16 -> 64 rings on one handle with n growing and shrinking (the workspace is re-allocated by the ring count), and
    vilf_feature_depth between the extractions"""
    scan64, scan64b = _scan_case(5, 64), _scan_case(7, 64)
    dc, df, dd = _depth_restatement("exits")[:3]
    steps = [(scan64[:20000], 64), (cases.sector_cloud(), 16), (scan64b, 64), (cases.one_ring_cloud(), 16), (scan64[:30000], 64), (cases.sector_cloud(), 32)]
    for cloud, n_scans in steps:
        e, s = device.extract(cloud, n_scans)
        oe, os_ = oracle.extract_features(cloud, n_scans=n_scans)
        assert _bits_equal(e, oe) and _bits_equal(s, os_), (len(cloud), n_scans)
        assert _bits_equal(device.fe.getFeatureDepth(dc, df), dd)


@pytest.mark.gpu
@pytest.mark.parametrize("name", DEPTH_CASES)
def test_hip_designed_depth(oracle, device, name):
    """fd_unit / fd_depth with lanes that hold zero, one or two candidates (n = 10 .. 257), fewer than three usable points, equal
    distances at the 3rd / 4th place, m = 0 / 1 / 1000, zero and NaN features, and every exit: bit-identical to oracle and restatement"""
    cloud, feats, depth, exits, clamps = _depth_restatement(name)
    got = device.fe.getFeatureDepth(cloud, feats)
    assert _bits_equal(got, oracle.feature_depth(cloud, feats)), "device against the oracle"
    assert _bits_equal(got, depth), "device against the restatement"
