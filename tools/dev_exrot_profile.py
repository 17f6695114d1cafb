#!/usr/bin/env python3
"""Camera-IMU rotation calibration: what vilf_exrot_profile reports for ONE push at 1 and at VILF_EXROT_MAX_SLOTS slots, m = 150 correspondences,
K = 512 hypotheses, as the 10th entry of every slot's history and as the last one it can hold. The histories are filled with m = 0 pushes first (not measured);
the measured push is repeated on freshly filled slots and the median is kept. Run by hand on a machine with the GPU:

    python3 tools/dev_exrot_profile.py [--repeats 5] [--out profiles/exrot_profile.json]
"""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--m", type=int, default=150)
    ap.add_argument("--k", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import exrot_cases as ec
    from vil_fusion_amd import abi
    from vil_fusion_amd.estimator import BackendSolver, ExRotation
    solver = BackendSolver()
    empty = np.zeros((0, 2))
    rows = []
    for slots in (1, abi.VILF_EXROT_MAX_SLOTS):
        for hist in (10, abi.VILF_EXROT_MAX_HISTORY):
            rng = np.random.default_rng(slots * 1000 + hist)
            fill = [ec.quat_xyzw(*ec.imu_rotation(rng)) for _ in range(hist - 1)]
            pairs = [(pr["a"], pr["b"], pr["dq"]) for pr in ec.make_pushes(7, slots, m=a.m)]      # a pair of its own per slot
            ms, wall = [], []
            dev = ExRotation(solver, slots, n_hypotheses=a.k)
            for _ in range(a.repeats + 1):                                                        # the first repeat warms up
                dev.reset()
                solver.set_profiling(False)
                for dq in fill:
                    dev.push([(empty, empty, dq)] * slots)
                solver.set_profiling(True)
                t0 = time.perf_counter()
                out = dev.push(pairs)
                wall.append((time.perf_counter() - t0) * 1e3)
                ms.append(dev.profile()[0])
                assert all(r["frame_count"] == hist and r["flags"] == abi.VILF_EXROT_SOLVED for r in out)
            ms, wall = np.array(ms[1:]), np.array(wall[1:])
            row = dict(slots=slots, history=hist, m=a.m, K=a.k, repeats=a.repeats,
                       ms_median=dict(zip(("ex_hypotheses", "ex_score", "ex_solve"), [float(v) for v in np.median(ms, axis=0)])),
                       ms_min=dict(zip(("ex_hypotheses", "ex_score", "ex_solve"), [float(v) for v in ms.min(axis=0)])),
                       kernels_ms_median=float(np.median(ms.sum(axis=1))), wall_ms_median=float(np.median(wall)))
            rows.append(row)
            print(json.dumps(row))
    solver.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(what="vilf_exrot_profile per push (HIP events), wall = the whole vilf_exrot_push call through ctypes", rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
