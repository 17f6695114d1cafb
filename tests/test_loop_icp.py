"""ICP verification of loop candidates (vilf_icp_*, vilf_icp.hip; ≙ icpCalculation of global_fusion): the boundary and the numpy restatement on the CPU, the device
against the restatement on the GPU. The semantics are the text in include/vilfusion.h; parity with PCL itself is unpinned."""
import ctypes as C
import math
import os
import re
import subprocess
import numpy as np
import pytest
from vil_fusion_amd import abi, lib, posegraph, synth
import icp_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vilfusion.h")
ICP_FUNCTIONS = ["vilf_icp_default_params", "vilf_icp_create", "vilf_icp_add_cloud", "vilf_icp_add_clouds", "vilf_icp_size", "vilf_icp_submap", "vilf_icp_align",
                 "vilf_icp_align_pairs", "vilf_icp_get_history", "vilf_icp_get_search", "vilf_get_profile_icp"]


# ---- CPU: the boundary ---------------------------------------------------------------------------------------------------------
def test_header_library_and_loader_have_the_icp_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(vilf_[a-z0-9_]+)\s*\(", src))
    assert set(ICP_FUNCTIONS) <= declared, sorted(set(ICP_FUNCTIONS) - declared)
    assert set(ICP_FUNCTIONS) <= set(lib.EXPORTED)
    if not os.path.exists(lib.SO_PATH):
        lib.build()
    L = C.CDLL(lib.SO_PATH)                          # loads without a GPU
    assert not [n for n in ICP_FUNCTIONS if not hasattr(L, n)]
    p = abi.IcpParams()
    L.vilf_icp_default_params(C.byref(p))            # host code only
    assert (p.max_correspondence_distance, p.max_iterations, p.history_keyframes, p.transformation_epsilon, p.euclidean_fitness_epsilon) == (100.0, 100, 25, 1e-6, 1e-6)
    assert (p.rotation_threshold, p.mse_relative, p.fitness_threshold, p.leaf_size, p.own_pose) == (0.99999, 1e-5, 0.3, 0.4, 0)
    q = R.Params()
    for name, _ in abi.IcpParams._fields_:
        if name != "pad_":
            assert getattr(q, name) == getattr(p, name), name


def test_icp_struct_layouts_match_the_c_header(tmp_path):
    structs = {"vilf_icp_params": abi.IcpParams, "vilf_icp_result": abi.IcpResult, "vilf_icp_iter": abi.IcpIter}
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
def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _scene_cloud(seed, n=6000):
    """a well-conditioned cloud: a ground patch, two walls and scattered points"""
    rng = np.random.default_rng(seed)
    g = np.column_stack([rng.uniform(-15, 15, n // 2), rng.uniform(-15, 15, n // 2), 0.02 * rng.standard_normal(n // 2)])
    w1 = np.column_stack([np.full(n // 6, 12.0), rng.uniform(-15, 15, n // 6), rng.uniform(0, 4, n // 6)])
    w2 = np.column_stack([rng.uniform(-15, 15, n // 6), np.full(n // 6, -9.0), rng.uniform(0, 4, n // 6)])
    s = np.column_stack([rng.uniform(-15, 15, n // 6), rng.uniform(-15, 15, n // 6), rng.uniform(0, 5, n // 6)])
    xyz = np.concatenate([g, w1, w2, s])
    return np.column_stack([xyz, rng.uniform(0, 1, len(xyz))]).astype(np.float32)


def test_reference_submap_of_one_cloud_is_the_oracle_voxel_grid(oracle):
    """identity pose: the sub-map of one cloud = pcl::VoxelGrid of it as the oracle restates it. The oracle sorts (leaf, input index) pairs with std::stable_sort and
    sums a leaf in float in that order: input order, the order the header pins."""
    cloud = _scene_cloud(1)
    L = oracle.lib()
    L.vilo_voxel_grid.argtypes = [C.POINTER(C.c_float), C.c_int, C.c_float, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int)]
    out = np.zeros((len(cloud), 4), dtype=np.float32); n = C.c_int(0)
    L.vilo_voxel_grid(cloud.ctypes.data_as(C.POINTER(C.c_float)), len(cloud), np.float32(0.4), out.ctypes.data_as(C.POINTER(C.c_float)), len(cloud), C.byref(n))
    got = R.submap([cloud], np.zeros((1, 6)), 0, 0, 0)
    assert 100 < n.value < len(cloud) and len(got) == n.value
    assert _same_bits(got, out[:n.value])


def _moved(cloud, rpy, t):
    Rm = synth.euler_R(np.array(rpy[2]), np.array(rpy[1]), np.array(rpy[0]))
    out = cloud.copy()
    out[:, :3] = (cloud[:, :3].astype(np.float64) @ Rm.T + np.asarray(t)).astype(np.float32)
    return out, Rm


@pytest.mark.parametrize("rpy,t", [((0.0, 0.0, 0.0), (0.003, -0.002, 0.001)), ((0.01, -0.02, 0.05), (0.12, -0.08, 0.03)), ((0.0, 0.0, -0.04), (-0.2, 0.15, 0.0))])
def test_reference_recovers_a_rigid_motion(rpy, t):
    """source = a rigidly moved copy of the target (the same points, so every nearest neighbour is the right one once it is close): recovered to float accuracy, accepted"""
    tgt = R.voxel_grid(_scene_cloud(2), 0.4)
    src, Rm = _moved(tgt, rpy, t)                       # ICP must find the inverse motion
    r = R.align(src, tgt)
    Rt = Rm.T
    assert r["converged"] and r["accepted"] and r["criterion"] in (R.TRANSFORM, R.ABS_MSE, R.REL_MSE) and r["n_correspondences"] == len(src)
    assert np.abs(r["transform"][:3, :3] - Rt).max() < 2e-6
    assert np.abs(r["transform"][:3, 3] - (-Rt @ np.asarray(t))).max() < 2e-4 and r["fitness"] < 1e-6
    assert abs(np.linalg.norm(r["pose_qt"][:4]) - 1) < 1e-12 and np.allclose(posegraph.rpy_from_q(r["pose_qt"][:4]), r["pose6"][3:], atol=1e-9)


def test_reference_too_few_correspondences_and_empty_source():
    tgt = R.voxel_grid(_scene_cloud(3), 0.4)
    far = np.array([[500.0, 0, 0, 0], [0, 600.0, 0, 0], [tgt[0, 0], tgt[0, 1], tgt[0, 2], 0], [tgt[1, 0], tgt[1, 1], tgt[1, 2], 0]], dtype=np.float32)
    r = R.align(far, tgt)                               # two points in range
    assert not r["converged"] and not r["accepted"] and r["criterion"] == R.NO_CORRESPONDENCES and r["iterations"] == 0 and r["n_correspondences"] == 2
    assert np.array_equal(r["transform"], np.eye(4, dtype=np.float32)) and r["fitness"] > 1e4          # no range limit in the fitness
    e = R.align(np.zeros((0, 4), dtype=np.float32), tgt)
    assert e["fitness"] == R.DBL_MAX and not e["accepted"] and e["n_source"] == 0


def test_reference_ties_go_to_the_lower_index():
    tg = R.Target(np.array([[0, 0, 0], [1.25, 0, 0], [2.25, 0, 0], [2.25, 0, 0]], dtype=np.float32))
    idx, d2 = tg.nearest(np.array([[1.75, 0, 0], [2.25, 0.5, 0]], dtype=np.float32))
    assert list(idx) == [1, 2] and list(d2) == [0.25, 0.25]


def test_reference_root_pose_quirk():
    """(prev, history, root = prev) puts every cloud under prev's pose (:206), not under its own (:205): the two targets differ, the single-cloud sub-map of prev does not"""
    clouds = [_scene_cloud(10 + k, 1500) for k in range(5)]
    poses = np.array([[2.0 * k, 0.3 * k, 0.0, 0.0, 0.0, 0.1 * k] for k in range(5)])
    a, b = R.submap(clouds, poses, 2, 2, 2), R.submap(clouds, poses, 2, 2, 2, R.Params(own_pose=1))
    assert len(a) and len(b) and not (len(a) == len(b) and np.array_equal(a, b))
    assert _same_bits(R.submap(clouds, poses, 2, 0, 2), R.submap(clouds, poses, 2, 0, 2, R.Params(own_pose=1)))
    one = R.voxel_grid(np.concatenate([R.transform(R.pose_matrix(poses[2]), c) for c in clouds]), 0.4)
    assert _same_bits(a, one)


# ---- CPU: PoseGraph with a stub verifier ----------------------------------------------------------------------------------------
class _StubVerifier:
    def __init__(self, accepted, pose_qt):
        self.accepted, self.pose_qt, self.clouds, self.calls = accepted, np.asarray(pose_qt, dtype=np.float64), [], []

    def add_cloud(self, cloud):
        self.clouds.append(cloud)

    def align(self, prev, curr, poses6):
        self.calls.append((prev, curr, np.array(poses6)))
        return dict(accepted=self.accepted, converged=True, pose_qt=self.pose_qt, fitness=0.1 if self.accepted else 1.0)


def _three_keyframes(pg):
    q = np.array([0, 0, 0, 1.0])
    for k in range(3):
        assert pg.add_odometry(0.1 * k, np.concatenate([q, [2.5 * k, 0, 0]]), cloud=np.full((4, 4), float(k), dtype=np.float32))


def test_pose_graph_with_a_stub_verifier():
    icp_qt = np.concatenate([synth.R_to_q(synth.euler_R(np.array(0.2), np.array(0.0), np.array(0.0))), [0.3, -0.1, 0.05]])
    pg = posegraph.PoseGraph(None, verifier=_StubVerifier(True, icp_qt))
    _three_keyframes(pg)
    assert len(pg.verifier.clouds) == 3 and pg.verifier.clouds[2][0, 0] == 2.0
    res = pg.verify_loop(0, 2)
    want = posegraph.PoseGraph(None)
    _three_keyframes(want)
    want.add_loop(0, 2, icp_qt)
    assert res["accepted"] and len(pg.edges) == len(want.edges) == 3
    for a, b in zip(pg.edges[-1], want.edges[-1]):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    prev, curr, poses6 = pg.verifier.calls[0]
    assert (prev, curr) == (0, 2) and poses6.shape == (3, 6) and np.array_equal(poses6, np.array([n["updated"] for n in pg.nodes]))
    rej = posegraph.PoseGraph(None, verifier=_StubVerifier(False, icp_qt))
    _three_keyframes(rej)
    assert not rej.verify_loop(0, 2)["accepted"] and len(rej.edges) == 2
    assert rej.close_loops() is None                   # no detector: nothing is queued
    with pytest.raises(ValueError):
        rej.add_odometry(1.0, np.concatenate([[0, 0, 0, 1.0], [50.0, 0, 0]]))      # a key frame without its cloud


def test_pose_graph_without_a_verifier_is_unchanged():
    pg = posegraph.PoseGraph(None)
    q = np.array([0, 0, 0, 1.0])
    assert pg.add_odometry(0.0, np.concatenate([q, [0, 0, 0]])) and pg.add_odometry(0.2, np.concatenate([q, [2.6, 0, 0]]))
    assert pg.verifier is None and len(pg.nodes) == 2 and len(pg.edges) == 1 and pg.close_loops() is None
    with pytest.raises(ValueError):
        pg.verify_loop(0, 1)


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver():
    from vil_fusion_amd.estimator import BackendSolver
    s = BackendSolver()
    yield s
    s.close()


@pytest.fixture(scope="module")
def route():
    """the route of the alignment tests and the restatement's answer for each of its candidates, checked before the device is looked at"""
    clouds, poses, pairs = R.loop_route()
    ref = [R.align_pair(clouds, poses, prev, curr) for prev, curr, _ in pairs]
    assert sum(r["accepted"] for r in ref) >= 2 and sum(not r["accepted"] for r in ref) >= 2, [r["accepted"] for r in ref]
    keep = [i for i, r in enumerate(ref) if r["margin"] > 1e-3 and r["fitness_margin"] > 1e-3 and r["stable"]]
    assert len(ref) - len(keep) <= len(ref) // 8 and len(keep) >= 8, (len(ref), len(keep))
    return clouds, poses, pairs, ref, keep


def _store(solver, clouds, **over):
    from vil_fusion_amd.estimator import LoopICP
    icp = LoopICP(solver, cap_keyframes=len(clouds) + 2, cap_points=sum(len(c) for c in clouds) + 16, **over)
    assert icp.add_many(clouds) == 0 and len(icp) == len(clouds)
    return icp


@pytest.mark.gpu
def test_submaps_bit_identical(solver):
    rng = np.random.default_rng(4)
    clouds = [_scene_cloud(20 + k, 1200 + 37 * k) for k in range(9)] + [np.zeros((0, 4), dtype=np.float32)]      # key frame 9 has no points
    poses = np.column_stack([rng.uniform(-30, 30, (10, 2)), rng.uniform(-1, 1, 10), rng.uniform(-0.05, 0.05, (10, 2)), rng.uniform(-3, 3, 10)])
    for own in (0, 1):
        icp = _store(solver, clouds, own_pose=own)
        p = R.Params(own_pose=own)
        for key, half, root in [(4, 0, 2), (4, 3, 4), (1, 3, 1), (0, 25, 0), (8, 2, 8), (8, 25, 3), (9, 0, 9), (9, 0, 2)]:
            got, want = icp.submap(key, half, root, poses), R.submap(clouds, poses, key, half, root, p)
            assert _same_bits(got, want), (own, key, half, root, len(got), len(want))
        assert len(icp.submap(9, 0, 9, poses)) == 0


@pytest.mark.gpu
def test_search_indices_and_d2_identical(solver):
    """first round and fitness pass against the restatement for every source point of a dense scene, with source points more than 50 m from every target point (the
    fallback scan). Exact ties have a test of their own below: the voxel filter leaves none in a scene like this."""
    rng = np.random.default_rng(6)
    tgt = _scene_cloud(30, 9000)
    tgt[:4, :3] = [[0, 0, 0], [1.25, 0, 0], [2.25, 0, 0], [-40.0, -40.0, -3.0]]
    src = _scene_cloud(31, 3000)
    src[:, :3] += np.float32(0.07)
    src[:6, :3] = [[1.75, 0, 0], [90.0, 5.0, 1.0], [-120.0, 80.0, 2.0], [0.0, 0.0, 70.0], [1.75, 0.0, 0.0], [60.0, -70.0, 0.0]]
    poses = np.zeros((2, 6))
    icp = _store(solver, [tgt, src], history_keyframes=0, max_iterations=3)
    S, T = R.submap([tgt, src], poses, 1, 0, 0), R.submap([tgt, src], poses, 0, 0, 0)
    assert _same_bits(icp.submap(1, 0, 0, poses), S) and _same_bits(icp.submap(0, 0, 0, poses), T)
    res = icp.align(0, 1, poses)
    ref = R.align(S, T, R.Params(history_keyframes=0, max_iterations=3))
    far = np.sqrt(ref["first_search"][1]) > 50.0
    assert far.sum() >= 3 and res["n_source"] == len(S) and res["n_target"] == len(T)
    for which, (ri, rd) in ((0, ref["first_search"]), (1, ref["fitness_search"])):
        gi, gd = icp.search(0, which)
        assert np.array_equal(gi, ri), (which, np.flatnonzero(gi != ri)[:10])
        assert _same_bits(gd, rd.astype(np.float32)), which
    assert res["iterations"] == ref["iterations"] and res["criterion"] == ref["criterion"]


def _tie_clouds():
    """targets that survive the 0.4 m voxel filter as they are (one point per leaf, binary-exact coordinates) and queries at exact float midpoints.
    Block A: the integer lattice [0, 12]^2 x [0, 2] (1 m apart; search cells are 1.6 m, the box starts at 0): queries at the midpoints of x edges, y edges, z edges
    (2 tied points), of xy faces (4) and of cubes (8). The midpoint 3.5 of 3 and 4 lies in the cell of 4, so the lower index sits in the neighbouring cell; 1.5 lies in
    the cell of 1. Block B: a sparse lattice 4 m apart at y >= 40: ties at d2 = 4 and 8, found in the second shell and beyond."""
    g = np.arange(13, dtype=np.float32)
    A = np.array([[x, y, z] for z in (0.0, 1.0, 2.0) for y in g for x in g], dtype=np.float32)
    B = np.array([[4.0 * i, 40.0 + 4.0 * j, 0.0] for j in range(4) for i in range(4)], dtype=np.float32)
    tgt = np.concatenate([A, B])
    q = []
    for z in (0.0, 1.0):
        for y in g[:-1]:
            for x in g[:-1]:
                q += [[x + 0.5, y, z], [x, y + 0.5, z], [x, y, z + 0.5], [x + 0.5, y + 0.5, z], [x + 0.5, y + 0.5, z + 0.5]]
    for j in range(3):
        for i in range(3):
            q += [[4.0 * i + 2.0, 40.0 + 4.0 * j, 0.0], [4.0 * i, 42.0 + 4.0 * j, 0.0], [4.0 * i + 2.0, 42.0 + 4.0 * j, 0.0]]
    rng = np.random.default_rng(9)
    src = np.array(q, dtype=np.float32)[rng.permutation(len(q))]
    pad = lambda c: np.column_stack([c, np.zeros(len(c), dtype=np.float32)]).astype(np.float32)
    return pad(tgt[rng.permutation(len(tgt))]), pad(src)


@pytest.mark.gpu
def test_search_exact_ties_go_to_the_lower_index(solver):
    tgt, src = _tie_clouds()
    poses = np.zeros((2, 6))
    S, T = R.submap([tgt, src], poses, 1, 0, 0), R.submap([tgt, src], poses, 0, 0, 0)
    # the restatement first: both clouds pass the filter unchanged (as sets), and the ties are there, by brute force over every pair
    assert len(S) == len(src) and len(T) == len(tgt)
    assert {tuple(v) for v in T[:, :3]} == {tuple(v) for v in tgt[:, :3]} and {tuple(v) for v in S[:, :3]} == {tuple(v) for v in src[:, :3]}
    d2 = R.d2_float(S[:, None, :3], T[None, :, :3])
    best = d2.min(1)
    tied = (d2 == best[:, None]).sum(1)
    want = np.argmax(d2 == best[:, None], axis=1)                      # the lowest index among the tied
    cell = lambda c: np.floor(c[:, :3] / np.float32(1.6)).astype(np.int64)      # the device's search cells: 4 leaves, the target's box starts at 0
    other_cell = (cell(T[want]) != cell(S)).any(1)
    own_cell_has_a_tied_point = np.array([(cell(T[d2[i] == best[i]]) == cell(S[i:i + 1])).all(1).any() for i in range(len(S))])
    assert (tied >= 2).sum() >= 1000 and (tied == 4).sum() >= 200 and (tied == 8).sum() >= 200, np.bincount(tied)
    assert ((tied >= 2) & other_cell & own_cell_has_a_tied_point).sum() >= 100       # the winner lies outside the query's cell although a tied point lies inside
    assert ((tied >= 2) & (best >= 4.0)).sum() >= 20                                 # ties beyond the first shell
    ri, rd = R.Target(T).nearest(S)
    assert np.array_equal(ri, want) and np.array_equal(rd, best)
    # the device
    icp = _store(solver, [tgt, src], history_keyframes=0, max_iterations=1)
    assert _same_bits(icp.submap(1, 0, 0, poses), S) and _same_bits(icp.submap(0, 0, 0, poses), T)
    icp.align(0, 1, poses)
    gi, gd = icp.search(0, 0)
    assert np.array_equal(gi, want), np.flatnonzero(gi != want)[:10]
    assert _same_bits(gd, best.astype(np.float32))


def _tolerances(ref, clouds):
    extent = max(float(np.abs(c[:, :3]).max()) for c in clouds if len(c)) * 2.0
    floor = 4.0 * float(np.spacing(np.float32(extent)))
    return {k: max(10.0 * v, floor) for k, v in ref["order_diff"].items()}, floor


@pytest.mark.gpu
def test_alignment_matches_the_restatement(solver, route):
    """Tolerance per quantity = max(10 x the restatement's own two-order difference, 4 float ulps of the cloud extent). Measured on one MI355X: see DESIGN.md section 3g."""
    clouds, poses, pairs, ref, keep = route
    icp = _store(solver, clouds)
    batch = icp.align_pairs([(a, b) for a, b, _ in pairs], poses)
    hist = [icp.history(i) for i in range(len(pairs))]
    worst = dict(translation=0.0, angle=0.0, fitness=0.0, mse=0.0)
    for i in keep:
        g, r = batch[i], ref[i]
        tol, floor = _tolerances(r, clouds)
        assert (g["converged"], g["accepted"], g["criterion"], g["iterations"]) == (r["converged"], r["accepted"], r["criterion"], r["iterations"]), (pairs[i], g, r["fitness"])
        assert (g["n_source"], g["n_target"]) == (r["n_source"], r["n_target"])
        assert [h["n_correspondences"] for h in hist[i]] == [h["n_correspondences"] for h in r["rounds"]]
        assert [h["criterion"] for h in hist[i]] == [h["criterion"] for h in r["rounds"]]
        d = dict(translation=float(np.abs(g["transform"][:3, 3].astype(np.float64) - r["transform"][:3, 3]).max()),
                 angle=abs(R.rotation_angle(g["transform"]) - R.rotation_angle(r["transform"])), fitness=abs(g["fitness"] - r["fitness"]),
                 mse=max(abs(a["mse"] - b["mse"]) for a, b in zip(hist[i], r["rounds"])))
        print(f"pair {pairs[i]}: iterations {g['iterations']} criterion {g['criterion']} accepted {g['accepted']} fitness {g['fitness']:.6f}; differences " +
              ", ".join(f"{k} {v:.3e} (tol {tol[k]:.3e})" for k, v in d.items()))
        for k in d:
            worst[k] = max(worst[k], d[k])
            assert d[k] <= tol[k], (pairs[i], k, d[k], tol[k])
        want6, wantq = R.result_pose(g["transform"])
        assert np.array_equal(g["pose6"], want6) and np.abs(g["pose_qt"] - wantq).max() < 1e-12
    print(f"worst differences over {len(keep)} candidates: {worst}; floor {floor:.3e}")
    # the batch equals the single calls bit for bit, and a second run equals the first
    again = icp.align_pairs([(a, b) for a, b, _ in pairs], poses)
    for i, (a, b, _) in enumerate(pairs):
        one = icp.align(a, b, poses)
        h1 = icp.history(0)
        for other in (one, again[i]):
            for k, v in batch[i].items():
                assert _same_bits(np.asarray(v), np.asarray(other[k])), (pairs[i], k)
        assert h1 == hist[i]


@pytest.mark.gpu
def test_a_true_guess_turns_a_rejected_candidate_into_an_accepted_one(solver, route):
    clouds, poses, pairs, ref, keep = route
    i = next(i for i in keep if pairs[i][2] == "large" and not ref[i]["accepted"])
    prev, curr, _ = pairs[i]
    P = lambda p: np.vstack([np.column_stack([synth.euler_R(np.array(p[5]), np.array(p[4]), np.array(p[3])), p[:3]]), [0, 0, 0, 1.0]])
    G = P(poses[curr]) @ np.linalg.inv(P(poses[prev]))       # the source sits under prev's pose: this moves it to where curr really was
    guess = np.concatenate([synth.R_to_q(G[:3, :3]), G[:3, 3]])
    r = R.align_pair(clouds, poses, prev, curr, guess_qt=guess)
    assert r["accepted"] and r["stable"] and r["margin"] > 1e-3 and r["fitness_margin"] > 1e-3          # the restatement's claim first
    icp = _store(solver, clouds)
    g0, g1 = icp.align(prev, curr, poses), icp.align(prev, curr, poses, guess_qt=guess)
    assert not g0["accepted"] and g1["accepted"]
    assert (g1["iterations"], g1["criterion"]) == (r["iterations"], r["criterion"])
    tol, _ = _tolerances(r, clouds)
    assert abs(g1["fitness"] - r["fitness"]) <= tol["fitness"] and np.abs(g1["transform"][:3, 3].astype(np.float64) - r["transform"][:3, 3]).max() <= tol["translation"]


@pytest.mark.gpu
def test_overflow_and_bad_indices_are_errors_and_leave_the_store(solver):
    from vil_fusion_amd.estimator import LoopICP
    clouds = [_scene_cloud(40 + k, 600) for k in range(3)]
    icp = LoopICP(solver, cap_keyframes=3, cap_points=2000)
    assert icp.add_cloud(clouds[0]) == 0 and icp.add_many(clouds[1:2]) == 1
    poses = np.zeros((3, 6))
    before, first = icp.submap(1, 1, 0, poses), icp.submap(0, 0, 0, poses)
    with pytest.raises(RuntimeError):
        icp.add_cloud(_scene_cloud(50, 1200))          # 1200 + 1200 points > 2000
    with pytest.raises(RuntimeError):
        icp.add_many(clouds[:2])                       # 2 + 2 key frames > 3
    assert len(icp) == 2
    for bad in [(-1, 1), (0, 2), (2, 0)]:
        with pytest.raises(RuntimeError):
            icp.align(bad[0], bad[1], poses)
    with pytest.raises(RuntimeError):
        icp.submap(2, 0, 0, poses)
    with pytest.raises(RuntimeError):
        icp.submap(0, 0, 5, poses)
    assert _same_bits(icp.submap(1, 1, 0, poses), before)
    assert icp.add_cloud(clouds[2][:100]) == 2 and len(icp) == 3
    solver._check(solver._L.vilf_reset(solver._h), "vilf_reset")
    assert len(icp) == 3 and len(first) > 100 and _same_bits(icp.submap(0, 0, 0, poses), first)       # vilf_reset leaves the store alone


@pytest.mark.gpu
def test_values_that_are_not_finite_are_rejected_by_the_host(solver):
    """a LiDAR no-return as inf / NaN, a pose or a guess that is not a number: invalid argument before anything is enqueued, the store as it was"""
    from vil_fusion_amd.estimator import LoopICP
    clouds = [_scene_cloud(60 + k, 600) for k in range(2)]
    icp = LoopICP(solver, cap_keyframes=4, cap_points=4000)
    assert icp.add_many(clouds) == 0
    poses = np.zeros((2, 6))
    before = icp.submap(1, 1, 0, poses)
    for bad_value in (np.inf, -np.inf, np.nan):
        bad = clouds[0].copy()
        bad[17, 1] = bad_value
        with pytest.raises(RuntimeError, match="not finite"):
            icp.add_cloud(bad)
        with pytest.raises(RuntimeError, match="not finite"):
            icp.add_many([clouds[1], bad])
        bad_poses = poses.copy()
        bad_poses[1, 5] = bad_value
        with pytest.raises(RuntimeError, match="not finite"):
            icp.align(0, 1, bad_poses)
        with pytest.raises(RuntimeError, match="not finite"):
            icp.submap(0, 0, 0, bad_poses)
        with pytest.raises(RuntimeError, match="not finite"):
            icp.align(0, 1, poses, guess_qt=[0, 0, 0, 1, bad_value, 0, 0])
    with pytest.raises(RuntimeError, match="zero quaternion"):
        icp.align(0, 1, poses, guess_qt=[0, 0, 0, 0, 0, 0, 0])
    assert len(icp) == 2 and _same_bits(icp.submap(1, 1, 0, poses), before)
    assert icp.align(0, 1, poses)["n_source"] > 0


@pytest.mark.gpu
def test_pose_graph_closes_a_loop_from_clouds_and_odometry_alone(solver):
    """ScanContext names the pair, LoopICP verifies it, posegraph_optimize takes the edge: no transform is handed in"""
    import sc_reference
    from vil_fusion_amd.estimator import LoopICP, ScanContext, posegraph_optimize
    clouds, poses = sc_reference.revisit_route(step=2.1, n_frames=100, yaw2=0.02, offset2=0.2)
    truth = np.array([np.concatenate([synth.R_to_q(synth.euler_R(np.array(yaw), np.array(0.0), np.array(0.0))), [x, y, 0.0]]) for x, y, yaw in poses])
    rng = np.random.default_rng(8)
    odo = [truth[0]]
    for k in range(1, len(truth)):                      # dead reckoning with a heading bias: metres of drift at the revisit
        rel = posegraph.between(truth[k - 1], truth[k])
        noise = np.concatenate([synth.q_exp(np.array([0.0, 0.0, 0.002]) + rng.normal(0, 0.0005, 3)), rng.normal(0, 0.01, 3)])
        odo.append(posegraph.compose(odo[-1], posegraph.compose(rel, noise)))
    backend = lambda x0, ps, e: posegraph_optimize(solver, x0, ps, e, max_iterations=30, tol=1e-9)[0]

    def run(with_loops):
        pg = posegraph.PoseGraph(backend, detector=ScanContext(solver, capacity=len(clouds), dist_thres=0.4),
                                 verifier=LoopICP(solver, cap_keyframes=len(clouds), cap_points=sum(len(c) for c in clouds)))
        closed = []
        for k, (c, o) in enumerate(zip(clouds, odo)):
            assert pg.add_odometry(0.1 * k, o, cloud=c)
            if with_loops:
                hit = pg.close_loops()
                if hit is not None and hit[2]["accepted"]:
                    closed.append(hit[:2])
        x = pg.update()
        return closed, float(np.linalg.norm(x[-1, 4:] - truth[-1, 4:])), pg

    none, err0, _ = run(False)
    closed, err1, pg = run(True)
    print(f"end to end: {len(closed)} loops closed (first {closed[:1]}), end-point error {err0:.3f} m without loops, {err1:.3f} m with")
    assert not none and len(closed) >= 1 and len(pg.edges) == len(clouds) - 1 + len(closed)
    assert err1 < err0
