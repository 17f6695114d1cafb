"""Every stage of a handle is registered for tear-down (vilf_destroy) and for the profile switch (vilf_set_profiling): one smallest call of each stage on one handle.
A stage missing from the handle's table keeps its times after the switch (the first test) or its memory after the destroy (the third)."""
import ctypes as C
import numpy as np
import pytest
import torch          # before the first handle: torch brings a HIP runtime of its own, and the one loaded first serves the process
import exrot_cases as ec
import feat_cases as fc
import kf_reference as kr
import s2m_scene
import sfm_cases as sc
import startup_reference as su_ref
import track_reference as tr
import tri_cases as tc

pytestmark = pytest.mark.gpu

# every profile getter that vilf_set_profiling resets, with its number of slots. vilf_get_profile_large_window is not among them: the general path times with a wait
# of its own per group and accumulates over the switch (bench.py reads differences); it is read in test_getters_before_any_stage_exists only
GETTERS = {"vilf_get_profile": 4, "vilf_get_profile_marginalize": 4, "vilf_get_profile_scan2map": 8, "vilf_get_profile_sc": 4, "vilf_get_profile_icp": 8,
           "vilf_get_profile_icp_map": 4, "vilf_track_profile": 5, "vilf_track_profile_frontend": 2, "vilf_track_profile_mask": 2, "vilf_startup_profile": 4,
           "vilf_startup_sfm_profile": 2, "vilf_startup_ba_profile": 1, "vilf_features_profile": 1, "vilf_exrot_profile": 3, "vilf_kf_profile": 5}
W, H = 64, 48
CAM = (61.6, 60.3, 31.0, 24.1, 0.0, 0.0, 0.0, 0.0)
SU_PARAMS = dict(n_hypotheses=64, seed=5)


def read(solver, name, n=None):
    n = GETTERS[name] if n is None else n
    ms, cnt = (C.c_double * n)(), (C.c_long * n)()
    f = getattr(solver._L, name)
    f.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_long)]
    assert f(solver._h, ms, cnt) == 0, name
    return list(ms), list(cnt)


@pytest.fixture(scope="module")
def inputs():
    from vil_fusion_amd import synth
    from vil_fusion_amd.estimator import default_options
    rng = np.random.default_rng(7)
    scene = sc.chain_scene(5700, n_frames=6, n=40, n_full=30)
    tex = tr.texture(13, min_period=5.0, max_period=40.0)
    me, ms = s2m_scene.scene(1)
    push = ec.make_pushes(11, 1, m=40)[0]
    mask = np.full((H, W), 255, dtype=np.uint8)
    mask[10:20, 10:20] = 0
    win, prior, _ = synth.make_window(123, default_options(), synth.SynthConfig(n_features=60))
    return dict(win=win, prior=prior, su_win=scene["win"], rel=dict(l=scene["l"], R=scene["rel_R"], T=scene["rel_T"]),
                pnp=dict(pts3=scene["X"][:20], pts2=scene["X"][:20, :2] / scene["X"][:20, 2:3], R=np.eye(3), t=np.zeros(3), min_count=6),
                tri=dict(tc.cases())["three windows"], push=(push["a"], push["b"], push["dq"]),
                imgs=[tr.render(tex, W, H, shift=(float(k), 0.0)) for k in range(3)], mask=mask, pattern=kr.read_pattern(),
                window_uv=rng.uniform(12, 36, (5, 2)).astype(np.float32), clouds=[rng.uniform(-20, 20, (300, 3)).astype(np.float32) * (1.0, 1.0, 0.05) for _ in range(4)],
                room=(me, ms), scan=s2m_scene.scans(me, ms, 1)[0], ring=fc.one_ring_cloud())


def run_stages(solver, inp):
    """one smallest call of every stage -> (getter -> what it reads right after its stage's call, the relative-pose rows). The tracker's record holds the last frame only,
    so its three getters are read after the frame that books into them"""
    from vil_fusion_amd.estimator import (ExRotation, FeatureExtraction, FeatureTracker, KeyFrameStore, LoopICP, Scan2Map, ScanContext, construct, frame_pnp,
                                          posegraph_optimize, relative_pose, triangulate_features)
    seen = {}
    solver.batch_upload([inp["win"]], [inp["prior"]]); solver.batch_solve(); solver.batch_marginalize()
    seen["vilf_get_profile"] = read(solver, "vilf_get_profile"); seen["vilf_get_profile_marginalize"] = read(solver, "vilf_get_profile_marginalize")
    lidar = Scan2Map(solver)
    lidar.localMapInited(*inp["room"]); lidar.optimation_processing(*inp["scan"])
    seen["vilf_get_profile_scan2map"] = read(solver, "vilf_get_profile_scan2map")
    FeatureExtraction(solver, n_scans=16).extractFeature(inp["ring"])
    ident = np.array([[0, 0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 1.0, 0, 0]], dtype=np.float64)
    posegraph_optimize(solver, ident, np.full(6, 1e-2), [(0, 1, [0, 0, 0, 1], [1.0, 0, 0], [0.1] * 6, 0)], max_iterations=2)
    db = ScanContext(solver, capacity=8, num_exclude_recent=1, tree_making_period=1)
    db.add_many(inp["clouds"]); db.detectLoopClosureID()
    seen["vilf_get_profile_sc"] = read(solver, "vilf_get_profile_sc")
    icp = LoopICP(solver, cap_keyframes=4, cap_points=4096)
    icp.add_many(inp["clouds"][:2])
    poses6 = np.zeros((2, 6)); poses6[1, 0] = 0.1
    icp.align(0, 1, poses6); icp.global_map(poses6)
    seen["vilf_get_profile_icp"] = read(solver, "vilf_get_profile_icp"); seen["vilf_get_profile_icp_map"] = read(solver, "vilf_get_profile_icp_map")
    trk = FeatureTracker(solver, W, H, CAM, max_cnt=30, min_dist=5, equalize=True, f_threshold=1.0, n_hypotheses=64)
    trk.readImage(inp["imgs"][0], 0.0); trk.readImage(inp["imgs"][1], 0.1)
    seen["vilf_track_profile"] = read(solver, "vilf_track_profile"); seen["vilf_track_profile_frontend"] = read(solver, "vilf_track_profile_frontend")
    trk.readImage_mask(inp["imgs"][2], inp["mask"], 0.2)
    seen["vilf_track_profile_mask"] = read(solver, "vilf_track_profile_mask")
    rows = relative_pose(solver, [inp["su_win"]], **SU_PARAMS)
    seen["vilf_startup_profile"] = read(solver, "vilf_startup_profile")
    construct(solver, [inp["su_win"]], rel=[inp["rel"]]); frame_pnp(solver, [inp["pnp"]])
    seen["vilf_startup_sfm_profile"] = read(solver, "vilf_startup_sfm_profile"); seen["vilf_startup_ba_profile"] = read(solver, "vilf_startup_ba_profile")
    triangulate_features(solver, inp["tri"])
    seen["vilf_features_profile"] = read(solver, "vilf_features_profile")
    ExRotation(solver, 1, n_hypotheses=64).push([inp["push"]])
    seen["vilf_exrot_profile"] = read(solver, "vilf_exrot_profile")
    kf = KeyFrameStore(solver, W, H, CAM, inp["pattern"], cap_keyframes=4, cap_keypoints=4096)
    kf.add_keyframe(inp["imgs"][0], inp["window_uv"]); kf.add_keyframe(inp["imgs"][1], inp["window_uv"]); kf.searchByBRIEFDes(1, [0])
    seen["vilf_kf_profile"] = read(solver, "vilf_kf_profile")
    return seen, rows


# the slots the calls of run_stages book into: all of a getter's, except slot 7 of the ICP (no launch books into it) and the scan-to-map groups, of which one step
# surely has the association (3) and the solve (4)
def booked(name, cnt):
    if name == "vilf_get_profile_icp":
        return range(7)
    if name == "vilf_get_profile_scan2map":
        return sorted({3, 4} | {i for i, c in enumerate(cnt) if c})
    return range(GETTERS[name])


def same_rows(a, b):
    for ra, rb in zip(a, b):
        assert ra["l"] == rb["l"] and ra["inlier_cnt"] == rb["inlier_cnt"] and len(ra["pairs"]) == len(rb["pairs"])
        for k in ("R", "T"):
            assert np.array_equal(np.ascontiguousarray(ra[k]).view(np.uint64), np.ascontiguousarray(rb[k]).view(np.uint64)), k
        for pa, pb in zip(ra["pairs"], rb["pairs"]):
            for k in ("count", "flags", "best_k", "score", "cheirality", "chosen", "inlier_cnt"):
                assert pa[k] == pb[k], k
            for k in ("parallax", "F", "R", "T"):
                assert np.array_equal(np.ascontiguousarray(pa[k], dtype=np.float64).view(np.uint64), np.ascontiguousarray(pb[k], dtype=np.float64).view(np.uint64)), k


def test_every_stage_resets_with_the_switch(inputs):
    from vil_fusion_amd.estimator import BackendSolver
    solver = BackendSolver()
    try:
        solver.set_profiling(True)
        seen, _ = run_stages(solver, inputs)
        assert sorted(seen) == sorted(GETTERS)
        for name, (ms, cnt) in seen.items():
            print(name, [round(v, 4) for v in ms], cnt)
            for i in booked(name, cnt):
                assert cnt[i] >= 1 and ms[i] > 0.0, (name, i, ms, cnt)
        solver.set_profiling(True)
        for name, n in GETTERS.items():
            assert read(solver, name) == ([0.0] * n, [0] * n), name
    finally:
        solver.close()


def test_getters_before_any_stage_exists():
    from vil_fusion_amd.estimator import BackendSolver
    solver = BackendSolver()
    try:
        solver.set_profiling(True)
        for name, n in dict(GETTERS, vilf_get_profile_large_window=4).items():
            assert read(solver, name, n) == ([0.0] * n, [0] * n), name
    finally:
        solver.close()


# the smallest device buffer any call of run_stages allocates: a DBuf asks for bytes + bytes / 8 + 256, so none is smaller than 256 bytes. A stage that vilf_destroy
# misses keeps at least that; the caches of the runtime are warm after the first handle
SMALLEST_BUFFER = 256


def test_destroy_and_recreate(inputs):
    from vil_fusion_amd.estimator import BackendSolver, relative_pose
    first, free = None, []
    for k in range(3):
        solver = BackendSolver()
        try:
            _, rows = run_stages(solver, inputs)
        finally:
            solver.close()
        first = rows if first is None else first
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    print("free bytes after destroy 1, 2, 3:", free)
    assert free[0] - free[2] <= SMALLEST_BUFFER, free
    solver = BackendSolver()
    try:
        fourth = relative_pose(solver, [inputs["su_win"]], **SU_PARAMS)
    finally:
        solver.close()
    same_rows(fourth, first)
    want = su_ref.relative_pose(inputs["su_win"], **SU_PARAMS)          # the exact reference of the stage's own tests
    assert fourth[0]["l"] == want["l"] and np.array_equal(np.asarray(fourth[0]["R"]).view(np.uint64), np.asarray(want["R"]).view(np.uint64))
