"""Scan-to-local-map (EstimationMapping) — oracle pins (CPU) and HIP-vs-oracle parity (GPU)."""
import ctypes as C
import numpy as np
import pytest
from vil_fusion_amd import abi, synth


def test_oracle_voxel_grid_vs_numpy(oracle):
    rng = np.random.default_rng(0)
    pts = np.column_stack([rng.uniform(-20, 20, 5000), rng.uniform(-20, 20, 5000), rng.uniform(-2, 3, 5000), rng.uniform(0, 1, 5000)]).astype(np.float32)
    out = np.zeros((5000, 4), dtype=np.float32); n = C.c_int(0)
    L = oracle.lib()
    L.vilo_voxel_grid.argtypes = [C.POINTER(C.c_float), C.c_int, C.c_float, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int)]
    leaf = np.float32(0.8)
    L.vilo_voxel_grid(pts.ctypes.data_as(C.POINTER(C.c_float)), 5000, leaf, out.ctypes.data_as(C.POINTER(C.c_float)), 5000, C.byref(n))
    out = out[:n.value]
    inv = np.float32(1.0) / leaf
    ijk = np.floor(pts[:, :3] * inv).astype(np.int64)
    ijk -= ijk.min(0)
    div = ijk.max(0) + 1
    key = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
    uk = np.unique(key)
    assert len(uk) == n.value
    ref = np.stack([pts[key == k].astype(np.float64).mean(0) for k in uk])     # ascending leaf index, like PCL's output order
    assert np.abs(out - ref).max() < 1e-4


def test_oracle_knn5_and_plane_line_fits(oracle, opts):
    rng = np.random.default_rng(1)
    L = oracle.lib()
    mp = np.column_stack([rng.uniform(-10, 10, 4000), rng.uniform(-10, 10, 4000), np.zeros(4000) + rng.normal(0, 0.01, 4000), np.ones(4000)]).astype(np.float32)
    q = rng.uniform(-9, 9, (200, 3)).astype(np.float32); q[:, 2] = rng.uniform(-0.3, 0.3, 200)
    idx = np.zeros((200, 5), dtype=np.int32); d5 = np.zeros((200, 5), dtype=np.float32)
    L.vilo_knn5_bruteforce.argtypes = [C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_float)]
    L.vilo_knn5_bruteforce(mp.ctypes.data_as(C.POINTER(C.c_float)), 4000, q.ctypes.data_as(C.POINTER(C.c_float)), 200, idx.ctypes.data_as(C.POINTER(C.c_int)), d5.ctypes.data_as(C.POINTER(C.c_float)))
    D = ((mp[None, :, :3].astype(np.float64) - q[:, None, :].astype(np.float64)) ** 2).sum(-1)
    ref = np.argsort(D, axis=1, kind="stable")[:, :5]
    assert (np.sort(idx, 1) == np.sort(ref, 1)).mean() > 0.999        # float vs double ordering of near ties
    assert np.allclose(d5, np.take_along_axis(D, idx.astype(np.int64), 1), rtol=1e-5, atol=1e-6)
    # plane association on a z = 0 ground: normal ~ +-z, d ~ 0, all points valid
    pose = np.array([0, 0, 0, 1, 0, 0, 0.0])
    pts = np.column_stack([q, np.ones(200)]).astype(np.float32)
    valid = np.zeros(200, dtype=np.uint8); nrm = np.zeros((200, 3)); d = np.zeros(200)
    L.vilo_s2m_associate_surf.argtypes = [C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_float), C.c_int, abi.c_double_p, C.POINTER(C.c_uint8), abi.c_double_p, abi.c_double_p]
    L.vilo_s2m_associate_surf(mp.ctypes.data_as(C.POINTER(C.c_float)), 4000, pts.ctypes.data_as(C.POINTER(C.c_float)), 200, abi.dptr(pose), valid.ctypes.data_as(C.POINTER(C.c_uint8)), abi.dptr(nrm), abi.dptr(d))
    ok = valid == 1
    assert ok.mean() > 0.5
    assert np.all(np.isfinite(nrm[ok]))
    # ... and against the independent restatement of the reference's text (tests/s2m_reference.py): the same five indices and float distances bit for bit, the same
    # verdict wherever it is not inside its own rounding error, and the plane within the derived tolerance. (The fit A n = -1 on a ground through the origin is
    # ill-conditioned by construction — d = 1/|n| is tiny — which the tolerance's condition number accounts for.)
    import s2m_reference as R
    ref = R.associate(mp, pts, pose, True)
    assert np.array_equal(idx, ref["idx"]) and d5.tobytes() == ref["d2"].tobytes()
    rb = ref["robust"] & (ref["d2"][:, 4] < 1)
    assert rb.sum() > 100 and np.array_equal(valid[rb] * 2, ref["kind"][rb])
    checked = 0
    for i in np.nonzero(rb & (ref["kind"] == 2))[0]:
        tol, _ = R.rule_tolerances(mp[ref["idx"][i], :3].astype(np.float64), True)
        if np.isfinite(tol):
            assert R.record_error(2, np.array([*nrm[i], d[i]]), ref["rec"][i]) <= tol
            checked += 1
    assert checked > 50


def test_oracle_scan2map_tracks_the_truth(oracle, opts):
    scans, poses = synth.make_lidar_sequence(3, 6, rings=32, azimuths=900)
    m = oracle.OracleS2M(opts)
    m.init(*scans[0])
    R0, t0 = poses[0]
    for k in range(1, 6):
        r = m.step(*scans[k])
        t_true = R0.T @ (poses[k][1] - t0)
        assert np.linalg.norm(np.array(r.pose_qt[4:]) - t_true) < 0.25
        assert r.n_edge_factors[1] > 10 and r.n_surf_factors[1] > 50 and r.iterations[0] >= 1


@pytest.mark.gpu
def test_scan2map_matches_oracle(oracle, opts):
    """configs[2] LiDAR stage: voxel down-sampling, radix-hashed voxel 5-NN, line / plane fits, edge / plane factors, LM solve,
    local-map maintenance — the HIP path against the CPU restatement, frame by frame. Integer results (point counts, accepted
    factor counts, iterations) must be identical; poses to 1e-9; the maintained local maps bit-identical."""
    from vil_fusion_amd.estimator import BackendSolver, Scan2Map
    scans, poses = synth.make_lidar_sequence(5, 7, rings=32, azimuths=900)
    ref = oracle.OracleS2M(opts); ref.init(*scans[0])
    s = BackendSolver(opts); dev = Scan2Map(s); dev.localMapInited(*scans[0])
    for k in range(1, 7):
        r = ref.step(*scans[k]); g = dev.optimation_processing(*scans[k])
        assert (r.n_edge_ds, r.n_surf_ds) == (g.n_edge_ds, g.n_surf_ds)
        assert list(r.n_edge_factors) == list(g.n_edge_factors) and list(r.n_surf_factors) == list(g.n_surf_factors)
        assert list(r.iterations) == list(g.iterations)
        assert (r.map_edge_size, r.map_surf_size) == (g.map_edge_size, g.map_surf_size)
        assert np.abs(np.array(r.pose_qt[:]) - np.array(g.pose_qt[:])).max() < 1e-9
        assert np.abs(np.array(r.rel_t[:]) - np.array(g.rel_t[:])).max() < 1e-9 and np.abs(np.array(r.rel_q[:]) - np.array(g.rel_q[:])).max() < 1e-9
        assert np.allclose(list(r.final_cost), list(g.final_cost), rtol=1e-9)
    for which in (0, 1):
        a, b = ref.get_map(which), dev.getMapCloud(which)
        assert a.shape == b.shape and np.array_equal(a, b), "local map must be bit-identical"
    s.close()


@pytest.mark.gpu
def test_scan2map_edge_cases(oracle, opts):
    from vil_fusion_amd.estimator import BackendSolver, Scan2Map
    s = BackendSolver(opts); dev = Scan2Map(s)
    ref = oracle.OracleS2M(opts)
    # tiny local map (< 10 edge / < 50 surf points): no association, pose only predicted, map still maintained
    rng = np.random.default_rng(0)
    e0 = np.column_stack([rng.uniform(5, 10, (5, 3)), np.ones(5)]).astype(np.float32)
    s0 = np.column_stack([rng.uniform(5, 10, (20, 3)), np.ones(20)]).astype(np.float32)
    dev.localMapInited(e0, s0); ref.init(e0, s0)
    g = dev.optimation_processing(e0, s0); r = ref.step(e0, s0)
    assert list(g.iterations) == [0, 0] == list(r.iterations)
    assert (g.map_edge_size, g.map_surf_size) == (r.map_edge_size, r.map_surf_size)
    # empty edge cloud
    empty = np.zeros((0, 4), dtype=np.float32)
    g = dev.optimation_processing(empty, s0); r = ref.step(empty, s0)
    assert (g.n_edge_ds, g.n_surf_ds) == (r.n_edge_ds, r.n_surf_ds) == (0, r.n_surf_ds)
    s.close()


@pytest.mark.gpu
def test_scan2map_batch_matches_single_stream_and_oracle(oracle, opts):
    """S independent LiDAR streams stepped together: every stream must reproduce the single-stream result (which is checked
    against the oracle above) bit for bit — same counts, same poses, same maps — including after a snapshot / rewind."""
    from vil_fusion_amd.estimator import BackendSolver, Scan2Map, Scan2MapBatch
    seqs = [synth.make_lidar_sequence(20 + k, 5, rings=32, azimuths=900)[0] for k in range(3)]
    S = 7                                                    # stream i replays sequence i % 3
    s = BackendSolver(opts)
    b = Scan2MapBatch(s, S, 2048, 8192, 8192, 32768)
    for i in range(S):
        b.localMapInited(i, *seqs[i % 3][0])
    singles = []
    for k in range(3):
        hs = BackendSolver(opts); m = Scan2Map(hs); m.localMapInited(*seqs[k][0]); singles.append((hs, m))
    refs = [oracle.OracleS2M(opts) for _ in range(3)]
    for k in range(3):
        refs[k].init(*seqs[k][0])
    for f in range(1, 5):
        for i in range(S):
            b.set_scan(i, *seqs[i % 3][f])
        if f == 3:
            b.snapshot()
        b.step()
        got = b.results()
        if f == 3:                                           # rewind + redo must give the same step again
            b.rewind(); b.step()
            again = b.results()
            for i in range(S):
                assert bytes(again[i]) == bytes(got[i])
        one = [m.optimation_processing(*seqs[k][f]) for k, (_, m) in enumerate(singles)]
        ora = [refs[k].step(*seqs[k][f]) for k in range(3)]
        for i in range(S):
            g, r, o = got[i], one[i % 3], ora[i % 3]
            assert bytes(g) == bytes(r), f"stream {i} frame {f} differs from the single-stream path"
            assert (g.n_edge_ds, g.n_surf_ds) == (o.n_edge_ds, o.n_surf_ds) and list(g.n_edge_factors) == list(o.n_edge_factors)
            assert list(g.n_surf_factors) == list(o.n_surf_factors) and list(g.iterations) == list(o.iterations)
            assert np.abs(np.array(g.pose_qt[:]) - np.array(o.pose_qt[:])).max() < 1e-9
    for i in range(S):
        for which in (0, 1):
            assert np.array_equal(b.getMapCloud(i, which), singles[i % 3][1].getMapCloud(which))
            assert np.array_equal(b.getMapCloud(i, which), refs[i % 3].get_map(which))
    for hs, _ in singles:
        hs.close()
    s.close()


def _lattice_scene():
    """A ground and a few poles on a dyadic lattice (every coordinate a multiple of 1/64 m: the sums, centroids and squared distances below are exact in float), with a
    checkerboard ripple of 1/32 m on both — the neighbours of a query still come in rings of exactly equal distance, but WHICH of them enter a fit changes the plane /
    line. Map = the lattice; scan = the same lattice lifted by 1/16 m."""
    g = np.arange(-8.0, 8.0, 0.5, dtype=np.float32)
    I, J = np.meshgrid(np.arange(len(g)), np.arange(len(g)), indexing="ij")
    surf = np.column_stack([g[I.ravel()] + 20.0, g[J.ravel()], -2.0 + ((I.ravel() + J.ravel()) % 2) / 32.0, np.ones(I.size)]).astype(np.float32)
    zz = np.arange(-1.5, 2.5, 0.25, dtype=np.float32)
    poles = [(16.0, -6.0), (18.0, -2.0), (22.0, 1.5), (25.0, 5.0), (19.0, 6.5)]
    edge = np.concatenate([np.column_stack([px + (np.arange(len(zz)) % 2) / 32.0, np.full(len(zz), py), zz, np.ones(len(zz))]) for px, py in poles]).astype(np.float32)
    lift = np.array([0.0, 0.0, 0.0625, 0.0], dtype=np.float32)
    return edge, surf, edge + lift, surf + lift


@pytest.mark.gpu
@pytest.mark.parametrize("grid_first", [False, True])
def test_scan2map_lattice_scene_equal_distances_everywhere(oracle, opts, grid_first):
    """Every down-sampled query of this scene sits at a centre of symmetry of the map lattice: its neighbours come in rings of EXACTLY equal float distances, so which five
    points the search keeps — and with the ripple, which plane / line the fit returns — is decided by the reference's rule for equal distances alone (ascending map
    index: what a linear scan keeps; b_associate_ties redoes such queries in that order). Counts, iterations, poses and maps must still equal the oracle's.
    grid_first: a step with empty scans first — no factors, the pose stays the identity to the bit, and the map update turns the raw map into a voxel grid in the
    library's cell-major order, where the reference's index order has to be recovered from the leaf keys. The last frame starts from an optimised (no longer dyadic)
    pose: the ordinary path on the same scene."""
    from vil_fusion_amd.estimator import BackendSolver, Scan2Map
    e0, s0, e1, s1 = _lattice_scene()
    empty = np.zeros((0, 4), dtype=np.float32)
    ref = oracle.OracleS2M(opts); ref.init(e0, s0)
    s = BackendSolver(opts); dev = Scan2Map(s); dev.localMapInited(e0, s0)
    frames = ([(empty, empty)] if grid_first else []) + [(e1, s1), (e0, s0)]
    for k, (e, sc) in enumerate(frames):
        r = ref.step(e, sc); g = dev.optimation_processing(e, sc)
        assert (g.n_edge_ds, g.n_surf_ds) == (r.n_edge_ds, r.n_surf_ds)
        assert list(g.n_edge_factors) == list(r.n_edge_factors) and list(g.n_surf_factors) == list(r.n_surf_factors), f"frame {k}"
        assert list(g.iterations) == list(r.iterations)
        assert np.abs(np.array(g.pose_qt[:]) - np.array(r.pose_qt[:])).max() < 1e-9, f"frame {k}"
        assert (g.map_edge_size, g.map_surf_size) == (r.map_edge_size, r.map_surf_size)
        if len(e) == 0:
            assert list(r.iterations) == [0, 0] and np.array_equal(np.array(g.pose_qt[:]), np.array([0, 0, 0, 1, 0, 0, 0.0]))
        elif k == len(frames) - 2:
            assert r.n_surf_factors[0] > 50 and r.n_edge_factors[0] > 5           # the scene does produce factors of both kinds
    for which in (0, 1):
        assert np.allclose(dev.getMapCloud(which), ref.get_map(which), rtol=0, atol=1e-5)
    s.close()


def test_oracle_grid_knn_equals_bruteforce_inside_the_gate(oracle):
    """The oracle's 1 m cell grid (what its scan-to-map step uses, like the reference's kd-tree) must return exactly the brute-force
    neighbours — indices, order and squared distances — for every query whose 5th neighbour is closer than 1 m, and agree that
    the others fail the gate."""
    rng = np.random.default_rng(7)
    mp = np.column_stack([rng.uniform(-15, 15, 6000), rng.uniform(-15, 15, 6000), rng.uniform(-1, 2, 6000), np.ones(6000)]).astype(np.float32)
    mp[100:140, :3] = mp[100, :3]                                         # exact duplicates: ties resolved by index
    q = np.concatenate([rng.uniform(-16, 16, (500, 3)), mp[90:150, :3] + 1e-3]).astype(np.float32)
    L = oracle.lib()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    outs = []
    for fn in (L.vilo_knn5_bruteforce, L.vilo_knn5_grid):
        fn.argtypes = [fp, C.c_int, fp, C.c_int, ip, fp]
        idx = np.zeros((len(q), 5), dtype=np.int32); d5 = np.zeros((len(q), 5), dtype=np.float32)
        fn(mp.ctypes.data_as(fp), len(mp), q.ctypes.data_as(fp), len(q), idx.ctypes.data_as(ip), d5.ctypes.data_as(fp))
        outs.append((idx, d5))
    (ib, db), (ig, dg) = outs
    inside = db[:, 4] < 1.0
    assert inside.sum() > 100 and (~inside).sum() > 10
    assert np.array_equal(ib[inside], ig[inside]) and np.array_equal(db[inside], dg[inside])
    assert np.all(dg[~inside, 4] >= 1.0)


@pytest.mark.gpu
def test_scan2map_bench_size_parity_and_invariants(oracle, opts):
    """BASELINE configs[2] LiDAR stage at its full size (≈ 1.2 k edge + ≈ 2.8 k surf queries against a ≈ 30 k + ≈ 59 k point local map):
    HIP == oracle on the warm-up frame and on the measured frame, plus size-independent properties of the maintained maps:
    ascending leaf order, one point per leaf (a voxel grid is idempotent), every point inside the crop box."""
    from vil_fusion_amd.estimator import BackendSolver, Scan2MapBatch
    me, ms, scans, pl = synth.make_lidar_bench_case(7000)
    ident = np.array([0, 0, 0, 1, 0, 0, 0.0])
    ref = oracle.OracleS2M(opts); ref.init(me, ms); ref.set_pose(ident, pl)
    s = BackendSolver(opts)
    S = 3
    b = Scan2MapBatch(s, S, len(scans[0][0]) + len(scans[1][0]) + 64, len(scans[0][1]) + len(scans[1][1]) + 64, len(me) + len(scans[0][0]) + 64, len(ms) + len(scans[0][1]) + 64)
    for i in range(S):
        b.localMapInited(i, me, ms, None, pl)
    for f in range(2):
        for i in range(S):
            b.set_scan(i, *scans[f])
        b.step()
        r = ref.step(*scans[f])
        for g in b.results():
            assert (g.n_edge_ds, g.n_surf_ds, list(g.n_edge_factors), list(g.n_surf_factors), list(g.iterations), g.map_edge_size, g.map_surf_size) == \
                   (r.n_edge_ds, r.n_surf_ds, list(r.n_edge_factors), list(r.n_surf_factors), list(r.iterations), r.map_edge_size, r.map_surf_size)
            assert np.abs(np.array(g.pose_qt[:]) - np.array(r.pose_qt[:])).max() < 1e-9
    assert r.n_edge_ds > 900 and r.n_surf_ds > 2000 and r.map_edge_size > 25000 and r.map_surf_size > 50000
    pose_t = np.array(r.pose_qt[4:])
    for which, leaf in ((0, np.float32(opts.edge_leaf_size)), (1, np.float32(opts.surf_leaf_size))):
        m = b.getMapCloud(1, which)
        assert np.array_equal(m, ref.get_map(which))
        inv = np.float32(1.0) / leaf
        ijk = np.floor(m[:, :3] * inv).astype(np.int64)
        key = ijk[:, 2] * (1 << 42) + ijk[:, 1] * (1 << 21) + ijk[:, 0]            # lexicographic (z, y, x) = PCL's leaf order for any min corner
        assert np.all(np.diff(key) > 0), "ascending leaf order, one point per leaf"
        assert np.all(np.abs(m[:, :3] - pose_t.astype(np.float32)) <= np.float32(opts.s2m_crop_half) + 1e-3)
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_scan,leaf", [(3000, 0.8), (24000, 0.25), (22150, 0.25), (20500, 0.25), (20500, 0.02), (3000, 0.02)])
def test_map_update_crop_duplicates_and_large_tails(oracle, n_scan, leaf):
    """createSubMap (EstimationMapping.hpp:298-352) in isolation: with <= 10 edge points in the map the reference skips the optimisation
    (:250) and still updates the maps, so the pose is the constant-velocity prediction on both sides and the surf map sees: a crop box
    (half 6 m) that moves 1.5 m per frame across the cloud (old leaves leave, leaves straddle the boundary), scan points falling into
    existing leaves, between them and beyond both ends, exact duplicates, and — second case — more than 8192 new leaves per frame
    (the fused update's global-memory variant). Maps must stay bit-identical to the oracle over 5 frames; the first frame also
    exercises the unsorted-map path. The scan sizes / leaf sizes also walk the scan voxel grid through its variants: 32-bit keys in LDS
    (3000 points; leaf 0.02 m: 30 key bits = 4 radix passes), the 24-bit layout (20500 points; leaf 0.02 m: top key byte recomputed from
    the points), the global-sort path (24000 points) and a batch whose streams split between the two (22150, 22050 and 21950 points: the in-LDS grid holds 22112)."""
    from vil_fusion_amd.estimator import BackendSolver, Scan2MapBatch
    o = oracle.default_options()
    o.s2m_crop_half = 6.0
    o.surf_leaf_size = leaf
    rng = np.random.default_rng(n_scan)
    S = 3
    cloud = lambda n, c, h: np.concatenate([rng.uniform(-h, h, (n, 3)) + c, rng.uniform(0, 1, (n, 1))], 1).astype(np.float32)
    s = BackendSolver(o)
    b = Scan2MapBatch(s, S, 64, n_scan + 64, 256, 200000)
    refs = [oracle.OracleS2M(o) for _ in range(S)]
    ident = np.array([0, 0, 0, 1, 0, 0, 0.0]); last = np.array([0, 0, 0, 1, -1.5, 0.3, 0.0])
    for i in range(S):
        me, ms = cloud(5, np.zeros(3), 1.0), cloud(4000 + 500 * i, np.zeros(3), 8.0)
        b.localMapInited(i, me, ms, ident, last)
        refs[i].init(me, ms); refs[i].set_pose(ident, last)
    for f in range(5):
        for i in range(S):
            sc = cloud(n_scan - 100 * i, np.zeros(3), 7.0)
            sc[:50] = sc[50:100]                                       # exact duplicates
            e = cloud(1, np.zeros(3), 1.0)
            b.set_scan(i, e, sc)
            r = refs[i].step(e, sc)
        b.step()
        got = b.results()
        for i in range(S):
            assert list(got[i].iterations) == [0, 0]
            m, mr = b.getMapCloud(i, 1), refs[i].get_map(1)
            assert m.shape == mr.shape, (f, i, m.shape, mr.shape)
            assert np.array_equal(m, mr), (f, i)
            assert np.array_equal(b.getMapCloud(i, 0), refs[i].get_map(0))
    assert got[0].map_surf_size > (8192 if n_scan > 20000 and leaf > 0.1 else 500)
    s.close()


@pytest.mark.gpu
def test_scan_voxel_grid_from_runs_and_handed_back_streams_in_one_batch(oracle):
    """The scan voxel grid sorts RUNS of consecutive points with one leaf (b_scan_voxel_runs) and hands clouds without scan order back to the point-sorting grid
    (b_scan_voxel): one batch holds a ring-ordered cloud (long runs, leaves of many runs, runs across the 64-lane strips and the 2048-point tiles), a random cloud
    with more runs than the run grid holds (handed back) and a small random one (every point its own run). Down-sampled counts identical, maps bit-identical
    to the oracle over 3 frames (the map is the voxel grid of map + scan: every centroid is a serial float sum in index order)."""
    from vil_fusion_amd.estimator import BackendSolver, Scan2MapBatch
    o = oracle.default_options()
    o.s2m_crop_half = 30.0
    rng = np.random.default_rng(5)
    def rings(n_ring, n_az, jitter):
        az = np.linspace(0, 2 * np.pi, n_az, endpoint=False)
        pts = []
        for r in range(n_ring):
            rad = 4.0 + 1.3 * r + 0.5 * np.sin(3 * az + r)
            pts.append(np.stack([rad * np.cos(az), rad * np.sin(az), -1.5 + 0.02 * r * np.cos(az), np.full_like(az, r)], 1))
        c = np.concatenate(pts).astype(np.float32)
        c[:, :3] += rng.normal(0, jitter, (len(c), 3)).astype(np.float32)
        return c
    cloud = lambda n, h: np.concatenate([rng.uniform(-h, h, (n, 3)), rng.uniform(0, 1, (n, 1))], 1).astype(np.float32)
    S = 3
    s = BackendSolver(o)
    b = Scan2MapBatch(s, S, 64, 21000, 256, 120000)
    refs = [oracle.OracleS2M(o) for _ in range(S)]
    ident = np.array([0, 0, 0, 1, 0, 0, 0.0])
    for i in range(S):
        me, ms = cloud(5, 1.0), cloud(3000, 20.0)
        b.localMapInited(i, me, ms, ident, ident)
        refs[i].init(me, ms); refs[i].set_pose(ident, ident)
    for f in range(3):
        scans = [rings(16, 1250, 0.002 * (f + 1)), cloud(12000, 20.0), cloud(3000, 20.0)]
        e = cloud(1, 1.0)
        want = []
        for i in range(S):
            b.set_scan(i, e, scans[i])
            want.append(refs[i].step(e, scans[i]))
        b.step()
        got = b.results()
        for i in range(S):
            assert (got[i].n_edge_ds, got[i].n_surf_ds) == (want[i].n_edge_ds, want[i].n_surf_ds), (f, i)
            assert np.array_equal(b.getMapCloud(i, 1), refs[i].get_map(1)), (f, i)
    assert want[0].n_surf_ds < 20000 // 3 and want[1].n_surf_ds > 7168           # long runs in the ring cloud; more leaves than the run grid holds runs in the random one
    s.close()


@pytest.mark.gpu
def test_scan_voxel_grid_sizes_around_every_boundary(oracle):
    """Scan sizes around the 64-run strips, the 2048-point tiles, the run capacity (7168) and the layouts of the point-sorting grid, random / ring-ordered / duplicated
    clouds, two leaf sizes, no optimisation (empty edge scans: the pose stays the identity, so every map is the voxel grid of map + scan to the bit). A batch whose
    largest scan has 15.1 k .. 16.4 k points used to ask for more LDS than a CU has (launch failed with "invalid argument"): 16000 is among the sizes."""
    from vil_fusion_amd.estimator import BackendSolver, Scan2MapBatch
    rng = np.random.default_rng(11)
    def rings(n, n_ring, jitter, scale):
        n_az = max(1, n // n_ring)
        az = np.linspace(0, 2 * np.pi, n_az, endpoint=False)
        pts = [np.stack([scale * (4.0 + 1.3 * r + 0.5 * np.sin(3 * az + r)) * np.cos(az), scale * (4.0 + 1.3 * r + 0.5 * np.sin(3 * az + r)) * np.sin(az),
                         -1.5 + 0.02 * r * np.cos(az), np.full_like(az, r)], 1) for r in range(n_ring)]
        c = np.concatenate(pts)[:n].astype(np.float32)
        c[:, :3] += rng.normal(0, jitter, (len(c), 3)).astype(np.float32)
        return c
    cloud = lambda n, h: np.concatenate([rng.uniform(-h, h, (n, 3)), rng.uniform(0, 1, (n, 1))], 1).astype(np.float32)
    sizes = [1, 2, 63, 64, 65, 512, 513, 2047, 2048, 2049, 4096, 7167, 7168, 7169, 8192, 15200, 16000, 16383, 16384, 20000, 21999]
    S = 4
    empty = np.zeros((0, 4), dtype=np.float32)
    for leaf in (0.4, 0.8):
        o = oracle.default_options(); o.s2m_crop_half = 60.0; o.surf_leaf_size = leaf
        s = BackendSolver(o)
        b = Scan2MapBatch(s, S, 64, 22064, 256, 160000)
        refs = [oracle.OracleS2M(o) for _ in range(S)]
        ident = np.array([0, 0, 0, 1, 0, 0, 0.0])
        for i in range(S):
            me, ms = cloud(5, 1.0), cloud(200, 20.0)
            b.localMapInited(i, me, ms, ident, ident); refs[i].init(me, ms); refs[i].set_pose(ident, ident)
        for rnd in range(6):
            want = []
            for i in range(S):
                n = sizes[(4 * rnd + i + (7 if leaf > 0.5 else 0)) % len(sizes)]
                kind = (rnd + i) % 4
                sc = cloud(n, 20.0) if kind == 0 else rings(n, [1, 4, 16, 64][(rnd + i) % 4], 0.002 * i, 0.5 + 0.6 * i) if kind == 1 else \
                    np.repeat(cloud(max(1, n // 7), 20.0), 7, axis=0)[:n] if kind == 2 else np.concatenate([rings(n // 2 + 1, 8, 0.002, 1.0), cloud(n - n // 2, 20.0)])[:max(n, 1)]
                b.set_scan(i, empty, sc); want.append(refs[i].step(empty, sc))
            b.step()
            got = b.results()
            for i in range(S):
                assert got[i].n_surf_ds == want[i].n_surf_ds, (leaf, rnd, i)
                assert np.array_equal(b.getMapCloud(i, 1), refs[i].get_map(1)), (leaf, rnd, i)
        s.close()


@pytest.mark.gpu
def test_voxel_index_overflow_fails_loudly(oracle):
    """a leaf so small that the scan's voxel index needs more than 32 bits (17 bits per axis here) must be reported, not silently mis-binned"""
    from vil_fusion_amd.estimator import BackendSolver, Scan2MapBatch
    from vil_fusion_amd.lib import VilfError
    o = oracle.default_options()
    o.surf_leaf_size = 0.001
    rng = np.random.default_rng(0)
    cloud = lambda n, h: np.concatenate([rng.uniform(-h, h, (n, 3)), rng.uniform(0, 1, (n, 1))], 1).astype(np.float32)
    s = BackendSolver(o)
    b = Scan2MapBatch(s, 1, 64, 4096, 256, 20000)
    b.localMapInited(0, cloud(5, 1.0), cloud(2000, 50.0), None, None)
    b.set_scan(0, cloud(1, 1.0), cloud(3000, 60.0))
    with pytest.raises(VilfError, match="voxel index"):
        b.step()
        b.results()
    s.close()


@pytest.mark.gpu
def test_local_map_orders_uploads_and_stream_copies(oracle, opts):
    """The device keeps a local map in cell-major leaf order (its own neighbour index); the outside sees pcl::VoxelGrid's order. (i) a raw cloud handed to
    localMapInited comes back from getMapCloud as given; (ii) a map that getMapCloud handed out (a voxel grid in PCL order) can be uploaded again — it is stored in
    cell-major order, comes back unchanged, and the next steps of that stream equal the steps of the stream it was taken from, bit for bit, and the oracle;
    (iii) a stream copied on the device is a replica; (iv) every maintained map is in ascending PCL leaf order with one point per leaf."""
    from vil_fusion_amd.estimator import BackendSolver, Scan2MapBatch
    scans, _ = synth.make_lidar_sequence(31, 6, rings=32, azimuths=900)
    s = BackendSolver(opts)
    b = Scan2MapBatch(s, 3, 2048, 8192, 8192, 32768)
    b.localMapInited(0, *scans[0])
    for which in (0, 1):
        assert np.array_equal(b.getMapCloud(0, which), scans[0][which]), "a raw cloud is not re-ordered"
    ref = oracle.OracleS2M(opts); ref.init(*scans[0])
    poses = []
    for f in (1, 2):
        b.set_scan(0, *scans[f]); b.step(); ref.step(*scans[f])
        poses.append(np.array(b.results(0, 1)[0].pose_qt[:]))
    maps = [b.getMapCloud(0, which) for which in (0, 1)]
    for which, leaf in ((0, np.float32(opts.edge_leaf_size)), (1, np.float32(opts.surf_leaf_size))):
        assert np.array_equal(maps[which], ref.get_map(which))
        ijk = np.floor(maps[which][:, :3] * (np.float32(1.0) / leaf)).astype(np.int64)
        assert np.all(np.diff(ijk[:, 2] * (1 << 42) + ijk[:, 1] * (1 << 21) + ijk[:, 0]) > 0), "ascending PCL leaf order, one point per leaf"
    b.localMapInited(1, maps[0], maps[1], poses[1], poses[0])     # globalOdom = the pose after frame 2, globalOdom_last = after frame 1
    b.copy_stream(0, 2)
    for which in (0, 1):
        assert np.array_equal(b.getMapCloud(1, which), maps[which]) and np.array_equal(b.getMapCloud(2, which), maps[which])
    for f in (3, 4, 5):
        for i in range(3):
            b.set_scan(i, *scans[f])
        b.step()
        got = b.results(); o = ref.step(*scans[f])
        assert bytes(got[0]) == bytes(got[2]), "a device copy of a stream is a replica"
        assert bytes(got[0]) == bytes(got[1]), "an uploaded voxel grid behaves like the map it was downloaded from"
        assert list(got[0].n_edge_factors) == list(o.n_edge_factors) and list(got[0].n_surf_factors) == list(o.n_surf_factors) and list(got[0].iterations) == list(o.iterations)
        assert np.abs(np.array(got[0].pose_qt[:]) - np.array(o.pose_qt[:])).max() < 1e-9
    for which in (0, 1):
        assert np.array_equal(b.getMapCloud(2, which), ref.get_map(which)) and np.array_equal(b.getMapCloud(1, which), ref.get_map(which))
    s.close()


@pytest.mark.gpu
def test_lidar_sequences_soak_frame_by_frame(oracle):
    """Promoted from tools/dev_soak_s2m_seq.py (round 4: 440 frames, 0 mismatches): LiDAR sequences of varied geometry (16 / 32 / 64 rings, 450 / 900 / 1800 azimuths,
    4 .. 8 frames) through the HIP scan-to-map path and the oracle frame by frame, the local maps evolving through voxel grid, association, LM solve, append, crop and map
    update: down-sampled counts, factor counts, LM iterations and map sizes identical in every frame, poses to 1e-9, map shapes equal at the end (a map row may differ in
    a last bit where an optimised pose differs in its last bits)."""
    from vil_fusion_amd.estimator import BackendSolver, Scan2Map
    rng = np.random.default_rng(5)
    o = oracle.default_options()
    frames = 0
    worst = 0.0
    for case in range(10):
        rings = int(rng.choice([16, 32, 64])); az = int(rng.choice([450, 900, 1800])); n = int(rng.integers(4, 9)); seed = int(rng.integers(1, 10000))
        scans, _poses = synth.make_lidar_sequence(seed, n, rings=rings, azimuths=az)
        ref = oracle.OracleS2M(o); ref.init(*scans[0])
        s = BackendSolver(o)
        try:
            dev = Scan2Map(s); dev.localMapInited(*scans[0])
            for k in range(1, n):
                r = ref.step(*scans[k]); g = dev.optimation_processing(*scans[k]); frames += 1
                assert (r.n_edge_ds, r.n_surf_ds, list(r.n_edge_factors), list(r.n_surf_factors), list(r.iterations), r.map_edge_size, r.map_surf_size) == \
                       (g.n_edge_ds, g.n_surf_ds, list(g.n_edge_factors), list(g.n_surf_factors), list(g.iterations), g.map_edge_size, g.map_surf_size), (case, rings, az, k)
                dp = float(np.abs(np.array(r.pose_qt[:]) - np.array(g.pose_qt[:])).max()); worst = max(worst, dp)
                assert dp <= 1e-9, (case, rings, az, k, dp)
            for which in (0, 1):
                assert ref.get_map(which).shape == dev.getMapCloud(which).shape, (case, which)
        finally:
            s.close()
    print(f"{frames} frames, worst |dpose| {worst:.2e}")


@pytest.mark.gpu
def test_library_radix_sort_is_a_stable_sort():
    """vilf_sort.hip (the library's own LSD radix sort of (key, value) pairs in global memory: tile histograms, one scan, stable scatter — it replaced the vendor sort on
    the unordered-map / oversized-scan / feature-extraction paths) against numpy's stable argsort: 32- and 64-bit keys, bit counts that are not multiples of eight,
    sizes around the tile (2048) and scan-chunk boundaries, many duplicates (stability: the values are the input positions), bits above `bits` ignored."""
    from vil_fusion_amd.estimator import BackendSolver
    solver = BackendSolver()
    L = solver._L
    L.vilf_debug_sort_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    rng = np.random.default_rng(9)
    for key64, bits in ((0, 7), (0, 19), (0, 32), (1, 33), (1, 45), (1, 64)):
        for n in (1, 255, 2047, 2048, 2049, 40000, 300001):
            dt = np.uint64 if key64 else np.uint32
            hi = min(bits, 12) if n > 1000 else bits                       # few distinct digits in the long arrays: long runs of equal keys
            keys = rng.integers(0, 2 ** min(hi, 62), size=n, dtype=np.uint64)
            if bits > 12 and n > 1000:
                keys |= rng.integers(0, 2 ** 6, size=n, dtype=np.uint64) << np.uint64(bits - 6)       # and the top digit in play
            junk = rng.integers(0, 16, size=n, dtype=np.uint64) << np.uint64(bits) if bits < (64 if key64 else 32) - 4 else np.zeros(n, dtype=np.uint64)
            full = (keys | junk).astype(dt)
            vals = np.arange(n, dtype=np.int32)
            ko = np.zeros(n, dtype=dt); vo = np.zeros(n, dtype=np.int32)
            rc = L.vilf_debug_sort_pairs(solver._h, full.ctypes.data, vals.ctypes.data, n, bits, key64, ko.ctypes.data, vo.ctypes.data)
            assert rc == 0
            order = np.argsort(keys, kind="stable")
            assert np.array_equal(vo, order.astype(np.int32)), (key64, bits, n)
            assert np.array_equal(ko, full[order]), (key64, bits, n)
    solver.close()
