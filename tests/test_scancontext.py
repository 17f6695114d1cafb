"""Scan Context loop detection on the device (vilf_sc_*, ≙ SCManager of global_fusion/include/Scancontext/Scancontext.h) against tests/sc_reference.py, the numpy
restatement of the semantics include/vilfusion.h states. CPU: the ABI surface, the struct layouts, and properties that pin the restatement itself. GPU: descriptors
bit-identical, the replay of a route that revisits itself (reference mode at two thresholds, exhaustive mode), the add paths, the pose-graph hook."""
import ctypes as C
import math
import os
import re
import subprocess
import numpy as np
import pytest
from vil_fusion_amd import abi, lib, posegraph, synth
import sc_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vilfusion.h")
SC_FUNCTIONS = ["vilf_sc_default_params", "vilf_sc_create", "vilf_sc_add_keyframe", "vilf_sc_add_keyframes", "vilf_sc_detect", "vilf_sc_detect_range", "vilf_sc_get",
                "vilf_sc_size"]


# ---- CPU: the boundary ---------------------------------------------------------------------------------------------------------
def test_header_library_and_loader_have_the_sc_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(vilf_[a-z0-9_]+)\s*\(", src))
    assert set(SC_FUNCTIONS) <= declared, sorted(set(SC_FUNCTIONS) - declared)
    assert set(SC_FUNCTIONS) <= set(lib.EXPORTED)
    if not os.path.exists(lib.SO_PATH):
        lib.build()
    L = C.CDLL(lib.SO_PATH)                          # loads without a GPU
    assert not [n for n in SC_FUNCTIONS if not hasattr(L, n)]
    p = abi.ScParams()
    L.vilf_sc_default_params(C.byref(p))             # host code only
    assert (p.num_rings, p.num_sectors, p.max_radius, p.lidar_height) == (20, 60, 80.0, 2.0)
    assert (p.num_exclude_recent, p.num_candidates, p.search_ratio, p.dist_thres, p.tree_making_period) == (30, 3, 0.1, 0.2, 30)
    q = R.Params()
    assert (q.max_radius, q.lidar_height, q.num_exclude_recent, q.num_candidates, q.search_ratio, q.dist_thres, q.tree_making_period) == (80.0, 2.0, 30, 3, 0.1, 0.2, 30)


def test_sc_struct_layouts_match_the_c_header(tmp_path):
    structs = {"vilf_sc_params": abi.ScParams, "vilf_sc_result": abi.ScResult}
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "vilfusion.h"', "int main(void) {"]
    checks = []
    for cname, ct in structs.items():
        prog.append(f'  printf("%zu\\n", sizeof({cname}));')
        checks.append((cname, "sizeof", C.sizeof(ct)))
        for fname, _ in ct._fields_:
            prog.append(f'  printf("%zu\\n", offsetof({cname}, {fname}));')
            checks.append((cname, fname, getattr(ct, fname).offset))
    prog += ["  return 0;", "}"]
    src = tmp_path / "layout.c"; exe = tmp_path / "layout"
    src.write_text("\n".join(prog))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert len(out) == len(checks)
    bad = [(c, f, int(o), e) for (c, f, e), o in zip(checks, out) if int(o) != e]
    assert not bad, bad


# ---- CPU: the restatement, pinned by what it must do by construction ----------------------------------------------------------------------
def _bin_centre_cloud(seed, n=400):
    """points on exact bin centres (ring r + 0.5, sector s + 0.5), distinct bins, random heights: a rotation by a multiple of 6 degrees in float moves them by ~1e-5 of
    a bin, never across one"""
    rng = np.random.default_rng(seed)
    bins = rng.permutation(R.RINGS * R.SECTORS)[:n]
    ring, sec = bins // R.SECTORS, bins % R.SECTORS
    rad, ang = (ring + 0.5) * 4.0, np.deg2rad((sec + 0.5) * 6.0)
    z = rng.uniform(-1.5, 6.0, n)
    return np.column_stack([rad * np.cos(ang), rad * np.sin(ang), z, np.ones(n)]).astype(np.float32), ring, sec, z.astype(np.float32)


def _rot_z(cloud, deg):
    a = np.deg2rad(deg)
    Rz = np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]], dtype=np.float32)
    out = cloud.copy()
    out[:, :2] = (cloud[:, :2] @ Rz.T).astype(np.float32)
    return out


def test_reference_descriptor_of_known_bins():
    p = R.Params()
    cloud, ring, sec, z = _bin_centre_cloud(0)
    d = R.make_descriptor(cloud, p)
    want = np.zeros((20, 60))
    want[ring, sec] = (z.astype(np.float64) + 2.0).astype(np.float32)
    assert np.array_equal(d, want)
    # two points in one bin: the higher one; a point at z + 2 <= -1000 never enters; beyond the radius, NaN and the origin are skipped
    extra = np.array([[10.0, 1.0, 1.0, 0], [10.0, 1.0, 3.0, 0], [10.0, 1.0, 2.0, 0], [30.0, -2.0, -1500.0, 0], [80.5, 0.0, 9.0, 0], [np.nan, 1.0, 9.0, 0], [1.0, 1.0, np.inf, 0],
                      [0.0, 0.0, 9.0, 0], [-0.0, 0.0, 9.0, 0]], dtype=np.float32)
    d2 = R.make_descriptor(extra, p)
    assert d2[2, 0] == 5.0 and np.count_nonzero(d2) == 1
    # x = +-0: the quotient is +-inf, atan +-pi/2: sectors 15 / 1 (clamped from -15) / 45 / 60 (clamped from 75)
    ok, ring0, sec0, *_ = R.point_bins(np.array([[0.0, 5.0, 1, 0], [-0.0, 5.0, 1, 0], [0.0, -5.0, 1, 0], [-0.0, -5.0, 1, 0]], dtype=np.float32), p)
    assert ok.all() and list(sec0 + 1) == [15, 1, 45, 60] and list(ring0 + 1) == [2, 2, 2, 2]
    assert np.array_equal(R.make_descriptor(np.zeros((0, 4), dtype=np.float32), p), np.zeros((20, 60)))


@pytest.mark.parametrize("k", [1, 7, 29, 46, 59])
def test_reference_rotation_by_k_sectors_shifts_columns(k):
    p = R.Params(num_candidates=0, search_ratio=1.0)            # exhaustive: every shift
    cloud, *_ = _bin_centre_cloud(1)
    d0, dk = R.make_descriptor(cloud, p), R.make_descriptor(_rot_z(cloud, 6.0 * k), p)
    assert np.array_equal(dk, np.roll(d0, k, axis=1))            # column c of the rotated cloud = column c - k of the original
    assert np.array_equal(R.ring_key(dk), R.ring_key(d0))        # a row holds a few floats of similar size: their fp64 sum is exact in any order
    assert np.allclose(np.roll(R.sector_key(d0), k), R.sector_key(dk), rtol=0, atol=0)
    dist, shift = R.distance(dk, d0, p)                          # circshift(d0, k) == dk
    assert shift == k and abs(dist) < 1e-15
    dist, shift = R.distance(d0, dk, p)
    assert shift == (60 - k) % 60 and abs(dist) < 1e-15
    # the reference's shortcut finds it too (the sector keys align exactly)
    assert R.distance(dk, d0, R.Params())[1] == k


def test_reference_ring_key_is_rotation_invariant_only_up_to_summation_order():
    """the ring key sums a row in column order, so a column shift may change its last bit: what is invariant is the multiset of the row. Documented, not asserted away:
    the bin-centre cloud above has few entries per row and exact float sums; a dense row differs by at most one ulp of the float key."""
    rng = np.random.default_rng(5)
    d = rng.uniform(0, 8, (20, 60)).astype(np.float32).astype(np.float64)
    a, b = R.ring_key(d), R.ring_key(np.roll(d, 17, axis=1))
    assert np.all(np.abs(a - b) <= np.spacing(np.maximum(np.abs(a), np.abs(b))))


def test_reference_empty_cloud_never_wins():
    p = R.Params()
    cloud, *_ = _bin_centre_cloud(2)
    empty = R.make_descriptor(np.zeros((0, 4), dtype=np.float32), p)
    full = R.make_descriptor(cloud, p)
    assert np.isnan(R.shift_distances(full, empty, range(60))).all() and np.isnan(R.shift_distances(empty, empty, [0])).all()
    assert R.distance(full, empty, p) == (R.NO_DIST, 0)
    m = R.SCManager(p)
    for _ in range(31):
        m.add(np.zeros((0, 4), dtype=np.float32))
    m.add(cloud)
    r = m.detect()                                               # every candidate is empty: nothing wins, nn_idx stays 0, no loop
    assert (r["loop_id"], r["nearest"], r["shift"], r["min_dist"]) == (-1, 0, 0, R.NO_DIST)


def test_reference_snapshot_schedule():
    """the searchable set is rebuilt every 30th counted call and stale in between: a query at call 29 after a rebuild cannot return an entry at or beyond the bound of that
    rebuild, although 29 newer entries are old enough by then"""
    p = R.Params(dist_thres=0.5)
    base, *_ = _bin_centre_cloud(3, n=600)
    other = [_bin_centre_cloud(100 + i, n=600)[0] for i in range(80)]
    m = R.SCManager(p)
    out = []
    for k in range(80):
        # key frames 20 (inside the first snapshot's reach only after a rebuild) and 59 hold the same place as the last query
        m.add(base if k in (20, 59) else other[k])
        out.append(m.detect())
    assert all(o["nearest"] == -1 and o["n_candidates"] == 0 for o in out[:30])       # fewer than 31 descriptors: early return, not counted
    assert [o["snapshot"] for o in out[30:]] == [30 * ((k - 30) // 30) + 1 for k in range(30, 80)]
    # query 59 (call 29, snapshot [0, 1)) cannot see key frame 20; query 60 (call 30: rebuild, snapshot [0, 31)) can
    assert out[59]["snapshot"] == 1 and out[59]["candidates"] == [0] and out[59]["loop_id"] != 20
    # the same place at key frames 20 and 60
    m3 = R.SCManager(p)
    res = []
    for k in range(61):
        m3.add(base if k in (20, 60) else other[k])
        res.append(m3.detect())
    assert res[60]["snapshot"] == 31 and res[60]["loop_id"] == 20 and res[60]["min_dist"] < 1e-12 and res[60]["shift"] == 0
    assert all(max(o["candidates"], default=-1) < o["snapshot"] for o in out[30:] + res[30:])


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver():
    from vil_fusion_amd.estimator import BackendSolver
    s = BackendSolver()
    yield s
    s.close()


@pytest.fixture(scope="module")
def route():
    clouds, poses = R.revisit_route()
    return clouds, poses


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _descriptor_cases():
    p = R.Params()
    cases = []
    specials = np.array([[0.0, 5.0, 1.0, 0], [-0.0, 5.0, 1.5, 0], [0.0, -5.0, 0.5, 0], [-0.0, -5.0, 0.25, 0], [0.0, 0.0, 9.0, 0], [-0.0, 0.0, 9.0, 0],
                         [np.nan, 1.0, 9.0, 0], [1.0, np.nan, 9.0, 0], [1.0, 1.0, np.nan, 0], [np.inf, 1.0, 9.0, 0], [3.0, 4.0, np.inf, 0], [3.0, 4.0, -np.inf, 0],
                         [85.0, 3.0, 7.0, 0], [-60.0, 60.0, 7.0, 0], [3e20, 1.0, 7.0, 0], [30.0, -2.0, -1500.0, 0], [12.0, -7.0, -2.0, 0]], dtype=np.float32)
    for rings, az, seed in ((16, 720, 11), (64, 1800, 12)):
        scene = synth.LidarScene(seed, n_poles=60, rings=rings, azimuths=az)          # max_range 90: returns beyond the 80 m radius are in every scan
        for i in range(2):
            yaw = 0.3 + 1.1 * i
            raw = R.mount(scene.scan_raw(synth.euler_R(np.array(yaw), np.array(0.0), np.array(0.0)), np.array([5.0 * i, -3.0, scene.h])))
            kept, removed = R.drop_boundary_points(raw, p)
            assert removed <= 1e-3 * len(raw), (removed, len(raw))                    # the filter cannot empty a test
            assert (np.hypot(kept[:, 0], kept[:, 1]) > 80.0).any()
            # the special points come after the filter: x = +-0 sits exactly on a sector boundary by construction (atan(+-inf) is exact) and must stay in
            cases.append(np.ascontiguousarray(np.concatenate([kept[: len(kept) // 2], specials, kept[len(kept) // 2:]])))
    cases.append(np.zeros((0, 4), dtype=np.float32))                                  # an empty cloud
    cases.append(np.array([[7.0, -2.0, 0.5, 1.0]], dtype=np.float32))                 # one point
    cases.append(specials)
    return p, cases


@pytest.mark.gpu
def test_descriptors_bit_identical(solver):
    from vil_fusion_amd.estimator import ScanContext
    p, cases = _descriptor_cases()
    sc = ScanContext(solver, capacity=len(cases))
    assert sc.add_many(cases) == 0 and len(sc) == len(cases)
    for i, cloud in enumerate(cases):
        want = R.make_descriptor(cloud, p)
        d, rk, sk = sc.get(i)
        diff = np.argwhere(d != want)
        print(f"cloud {i}: {len(cloud)} points, {np.count_nonzero(want)} bins, {len(diff)} bins differ")
        assert _same_bits(d, want), (i, diff[:5], d[tuple(diff[0])], want[tuple(diff[0])])
        rw, sw = R.ring_key(want), R.sector_key(want)
        assert rk.dtype == np.float32 and np.all(np.abs(rk.astype(np.float64) - rw.astype(np.float64)) <= np.spacing(np.abs(rw)).astype(np.float64)), i
        assert np.all(np.abs(sk - sw) <= 1e-15 * np.abs(sw)), i


def _check_preconditions(ref, thres, first=30):
    """asserted on the restatement before the device is looked at, so that a flip cannot be blamed on rounding"""
    q = ref[first:]
    assert min(o["ring_gap_rel"] for o in q) > 1e-5
    assert min(o["runner_up_gap"] for o in q) > 1e-9
    assert min(abs(o["min_dist"] - thres) for o in q) > 1e-9


def _compare(got, ref, what):
    assert len(got) == len(ref)
    worst = 0.0
    for k, (g, r) in enumerate(zip(got, ref)):                # every query, the early returns included
        for f in ("loop_id", "nearest", "shift", "n_candidates", "candidates"):
            assert g[f] == r[f], (what, k, f, g, r)
        assert abs(g["min_dist"] - r["min_dist"]) <= 1e-12, (what, k, g["min_dist"], r["min_dist"])
        assert np.float32(g["yaw_diff_rad"]) == np.float32(r["yaw_diff_rad"]), (what, k)
        worst = max(worst, abs(g["min_dist"] - r["min_dist"]))
    print(f"{what}: {len(got)} queries, max |min_dist - restatement| {worst:.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("thres", [0.2, 0.4])
def test_replay_parity(solver, route, thres):
    from vil_fusion_amd.estimator import ScanContext
    clouds, _ = route
    _, ref = R.replay(clouds, R.Params(dist_thres=thres))
    _check_preconditions(ref, thres)
    loops = sum(o["loop_id"] >= 0 for o in ref)
    print(f"thres {thres}: restatement reports {loops} loops in {len(ref) - 30} searched queries")
    assert (loops >= 1) and (loops < len(ref) - 30) and (thres < 0.3 or loops >= 20)      # both outcomes occur
    sc = ScanContext(solver, capacity=len(clouds), dist_thres=thres)
    sc.add_many(clouds)
    _compare(sc.detect_range(), ref, "detect_range")
    _compare(sc.detect_range(50, 40), ref[50:90], "detect_range(50, 40)")
    sc = ScanContext(solver, capacity=len(clouds), dist_thres=thres)                       # a second create on the handle starts clean
    assert len(sc) == 0
    step = []
    for k, c in enumerate(clouds):
        assert sc.makeAndSaveScancontextAndKeys(c) == k
        loop_id, yaw = sc.detectLoopClosureID()
        assert (loop_id, np.float32(yaw)) == (sc.last["loop_id"], np.float32(sc.last["yaw_diff_rad"]))
        step.append(sc.last)
    _compare(step, ref, "detect, frame by frame")


@pytest.mark.gpu
def test_exhaustive_mode(solver, route):
    from vil_fusion_amd.estimator import ScanContext
    clouds, _ = route
    _, ref = R.replay(clouds, R.Params(num_candidates=0, search_ratio=1.0))
    assert min(o["runner_up_gap"] for o in ref[30:]) > 1e-9 and min(abs(o["min_dist"] - 0.2) for o in ref[30:]) > 1e-9
    sc = ScanContext(solver, capacity=len(clouds), num_candidates=0, search_ratio=1.0)
    sc.add_many(clouds)
    exh = sc.detect_range()
    _compare(exh, ref, "exhaustive detect_range")
    assert [o["n_candidates"] for o in exh[30:]] == [30 * ((k - 30) // 30) + 1 for k in range(30, len(clouds))]
    sc = ScanContext(solver, capacity=len(clouds))
    sc.add_many(clouds)
    fast = sc.detect_range()
    assert all(e["min_dist"] <= f["min_dist"] for e, f in zip(exh, fast))                  # the shortcuts search a subset of the same distances
    print("exhaustive below the reference mode in", sum(e["min_dist"] < f["min_dist"] for e, f in zip(exh, fast)), "of", len(exh) - 30, "queries")


@pytest.mark.gpu
def test_add_paths_agree_and_overflow_is_an_error(solver, route):
    from vil_fusion_amd.estimator import ScanContext
    from vil_fusion_amd.lib import VilfError
    clouds = route[0][:45] + [np.zeros((0, 4), dtype=np.float32)] + route[0][45:60]
    sc = ScanContext(solver, capacity=len(clouds))
    assert sc.add_many(clouds[:20]) == 0 and sc.add_many(clouds[20:]) == 20
    batched = [sc.get(i) for i in range(len(clouds))]
    res_b = sc.detect_range()
    sc = ScanContext(solver, capacity=len(clouds))
    assert len(sc) == 0
    for k, c in enumerate(clouds):
        assert sc.makeAndSaveScancontextAndKeys(c) == k
    for i in range(len(clouds)):
        assert all(_same_bits(a, b) for a, b in zip(batched[i], sc.get(i))), i
    assert res_b == sc.detect_range()                            # the normalised copies, norms and masks behind the search are the same too
    # overflow: an error, nothing added, the database still usable
    sc = ScanContext(solver, capacity=5)
    sc.add_many(clouds[:4])
    with pytest.raises(VilfError, match="capacity"):
        sc.add_many(clouds[4:7])
    assert len(sc) == 4
    assert sc.makeAndSaveScancontextAndKeys(clouds[4]) == 4
    with pytest.raises(VilfError, match="capacity"):
        sc.makeAndSaveScancontextAndKeys(clouds[5])
    assert len(sc) == 5 and all(_same_bits(a, b) for a, b in zip(batched[4], sc.get(4)))
    with pytest.raises(VilfError):
        sc.detect_range(3, 5)
    solver._check(solver._L.vilf_reset(solver._h), "vilf_reset")          # clearState() of the estimator: another node, the database stays
    assert len(sc) == 5 and _same_bits(batched[2][0], sc.get(2)[0])


class _ReferenceDetector:
    """the restatement behind the detector interface PoseGraph drives"""
    def __init__(self, params):
        self.m = R.SCManager(params)

    def makeAndSaveScancontextAndKeys(self, cloud):
        return self.m.add(cloud)

    def detectLoopClosureID(self):
        r = self.m.detect()
        return r["loop_id"], r["yaw_diff_rad"]


def _drive(pg, clouds, poses):
    pairs, keys = [], 0
    for k, (c, (x, y, yaw)) in enumerate(zip(clouds, poses)):
        q = synth.R_to_q(synth.euler_R(np.array(yaw), np.array(0.0), np.array(0.0)))
        keys += pg.add_odometry(0.1 * k, np.concatenate([q, [x, y, 0.0]]), cloud=c)
        hit = pg.detect_loop()
        if hit is not None:
            pairs.append(hit)
    return pairs, keys


@pytest.mark.gpu
def test_pose_graph_hook(solver):
    from vil_fusion_amd.estimator import ScanContext
    clouds, poses = R.revisit_route(step=2.1, n_frames=135)      # 2.1 m: the chord exceeds the 2 m gate, every message is a key frame
    want, keys_ref = _drive(posegraph.PoseGraph(None, detector=_ReferenceDetector(R.Params(dist_thres=0.4))), clouds, poses)
    assert keys_ref == len(clouds) and len(want) >= 10
    pg = posegraph.PoseGraph(None, detector=ScanContext(solver, capacity=len(clouds), dist_thres=0.4))
    got, keys = _drive(pg, clouds, poses)
    assert keys == keys_ref and len(pg.detector) == keys
    assert [(a, b) for a, b, _ in got] == [(a, b) for a, b, _ in want]
    assert [np.float32(y) for _, _, y in got] == [np.float32(y) for _, _, y in want]
    assert all(prev < curr - 30 for prev, curr, _ in got)
    print(f"pose-graph hook: {keys} key frames, {len(got)} pairs queued for ICP, first {got[0]}")


def test_pose_graph_without_a_detector_is_unchanged():
    """no detector: clouds are ignored, detect_loop() has nothing to ask; with one, a key frame without its cloud is an error"""
    pg = posegraph.PoseGraph(None)
    q = np.array([0, 0, 0, 1.0])
    assert pg.add_odometry(0.0, np.concatenate([q, [0, 0, 0]])) and not pg.add_odometry(0.1, np.concatenate([q, [0.5, 0, 0]]), cloud=np.zeros((3, 4)))
    assert pg.add_odometry(0.2, np.concatenate([q, [2.6, 0, 0]])) and len(pg.nodes) == 2 and len(pg.edges) == 1 and pg.detect_loop() is None
    pg = posegraph.PoseGraph(None, detector=_ReferenceDetector(R.Params()))
    with pytest.raises(ValueError):
        pg.add_odometry(0.0, np.concatenate([q, [0, 0, 0]]))
    assert len(pg.nodes) == 0
