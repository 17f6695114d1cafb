#!/usr/bin/env python3
"""Global-map build timing (vilf_icp_global_map): the new path against the only route the library offered before it, vilf_icp_submap(key = 0,
submap_size = size, root = 0) on an own_pose = 1 store, over the same clouds and poses in the same process, the two alternating.
  clouds   seeded synth.LidarScene scans (16 rings x --azimuths azimuths, about 2000 returns each) from key frames 2 m apart on a slowly widening spiral
  sizes    --keyframes 64 2000 (default): a short run and a route-scale one
  kernel   HIP events under vilf_set_profiling: vilf_get_profile_icp_map (4 stages) / slots 0-3 of vilf_get_profile_icp (icp_bbox, icp_leaf_keys, sorts, icp_voxel),
           per build; wall = the whole call (host table, uploads, the one wait), from runs without the events
One warm-up build of each path, then --repeats alternating builds; median and [min, max] are reported. The two maps are compared bit for bit first.

  python tools/dev_global_map.py [--keyframes 64 2000] [--repeats 7] [--out FILE.json]"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)
import numpy as np

MAP_STAGES = ("gmap_xf_bbox+gmap_box", "gmap_leaf_keys", "radix_sort", "gmap_count+gmap_scan+gmap_centroids")
SUB_STAGES = ("icp_bbox", "icp_leaf_keys", "radix_sort", "icp_voxel")


def route(n_kf, azimuths, seed=3):
    from vil_fusion_amd import synth
    scene = synth.LidarScene(seed, n_poles=20, rings=16, azimuths=azimuths)
    clouds, poses = [], []
    a, r = 0.0, 30.0
    for k in range(n_kf):
        x, y, yaw = r * math.cos(a), r * math.sin(a), a + math.pi / 2
        Rm = synth.euler_R(np.array(yaw), np.array(0.0), np.array(0.0))
        clouds.append(np.ascontiguousarray(scene.scan_raw(Rm, np.array([x, y, scene.h]))[:, :4], dtype=np.float32))
        poses.append([x, y, scene.h, 0.0, 0.0, math.atan2(math.sin(yaw), math.cos(yaw))])
        a += 2.0 / r
        r = min(r + 0.02, 80.0)
    return clouds, np.array(poses)


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def measure(s, n_kf, azimuths, repeats):
    from vil_fusion_amd import abi
    from vil_fusion_amd.estimator import LoopICP
    L, h = s._L, s._h
    clouds, poses = route(n_kf, azimuths)
    icp = LoopICP(s, cap_keyframes=n_kf, cap_points=sum(len(c) for c in clouds), own_pose=1)
    icp.add_many(clouds)
    p = np.ascontiguousarray(poses)
    n_map, n_sub = C.c_long(0), C.c_int(0)

    def build_map():
        s._check(L.vilf_icp_global_map(h, 0, n_kf, 1, abi.dptr(p), C.byref(n_map)), "vilf_icp_global_map")

    def build_sub():
        s._check(L.vilf_icp_submap(h, 0, n_kf, 0, abi.dptr(p), None, 0, C.byref(n_sub)), "vilf_icp_submap")

    def profiles():
        ms8, c8, ms4, c4 = (C.c_double * 8)(), (C.c_long * 8)(), (C.c_double * 4)(), (C.c_long * 4)()
        s._check(L.vilf_get_profile_icp(h, ms8, c8), "vilf_get_profile_icp")
        s._check(L.vilf_get_profile_icp_map(h, ms4, c4), "vilf_get_profile_icp_map")
        return np.array(ms8[:4]), np.array(ms4[:])

    s._check(L.vilf_set_profiling(h, 0), "vilf_set_profiling")
    same = icp.global_map(poses).tobytes() == icp.submap(0, n_kf, 0, poses).tobytes()          # warm-up of both paths, and the check that they build the same map
    wall_map, wall_sub = [], []
    for _ in range(repeats):
        t0 = time.perf_counter(); build_sub(); wall_sub.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter(); build_map(); wall_map.append((time.perf_counter() - t0) * 1e3)
    s._check(L.vilf_set_profiling(h, 1), "vilf_set_profiling")
    build_sub(); build_map()
    ker_map, ker_sub = [], []
    for _ in range(repeats):
        a8, a4 = profiles()
        build_sub()
        b8, b4 = profiles()
        build_map()
        c8, c4 = profiles()
        ker_sub.append(b8 - a8); ker_map.append(c4 - b4)
    s._check(L.vilf_set_profiling(h, 0), "vilf_set_profiling")
    ker_map, ker_sub = np.array(ker_map), np.array(ker_sub)
    out = dict(keyframes=n_kf, points=int(sum(len(c) for c in clouds)), map_points=int(n_map.value), submap_points=int(n_sub.value), identical=bool(same),
               kernel_ms_map=stats(ker_map.sum(1)), kernel_ms_submap=stats(ker_sub.sum(1)),
               stages_ms_map={k: stats(ker_map[:, i]) for i, k in enumerate(MAP_STAGES)}, stages_ms_submap={k: stats(ker_sub[:, i]) for i, k in enumerate(SUB_STAGES)},
               wall_ms_map=stats(wall_map), wall_ms_submap=stats(wall_sub))
    out["kernel_ratio_submap_over_map"] = out["kernel_ms_submap"]["median"] / out["kernel_ms_map"]["median"]
    out["wall_ratio_submap_over_map"] = out["wall_ms_submap"]["median"] / out["wall_ms_map"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, nargs="+", default=[64, 2000])
    ap.add_argument("--azimuths", type=int, default=160)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from vil_fusion_amd.estimator import BackendSolver
    s = BackendSolver()
    result = dict(tool="tools/dev_global_map.py", repeats=a.repeats, runs=[])
    for n_kf in a.keyframes:
        r = measure(s, n_kf, a.azimuths, a.repeats)
        result["runs"].append(r)
        print(json.dumps(r), flush=True)
    s.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
