#!/usr/bin/env python3
"""Scan Context replay timing: a database of N synthetic key frames (default 4096, the size of a KITTI-08 run), then
  add      vilf_sc_add_keyframes of all clouds (one upload, one sc_descriptor launch)
  ref      vilf_sc_detect_range over all key frames in the reference's mode (3 candidates, 7 shifts)
  exh      the same in exhaustive mode (every snapshot entry, 60 shifts: the mode sc_distance's matrix-core product exists for)
  host     tests/sc_reference.py (numpy) on a sample of the same queries, scaled to the replay by its (candidate, shift) count: context only
Kernel times are HIP events under vilf_set_profiling (vilf_get_profile_sc); wall times include the copies and the host side of the call.

  python tools/dev_sc_replay.py [--n 4096] [--out FILE.json]       # runs the steps as child processes, each GPU step under its own `timeout`, stops at the first that fails
  python tools/dev_sc_replay.py --step add|ref|exh|host            # one step in this process; prints one JSON line

The clouds are synthetic descriptors turned back into points (one point per occupied bin, on the bin centre): 40 "places" with their own skyline, every key frame
one of them seen under a random yaw with noise on the heights, so the search has revisits to find. No ray casting."""
import argparse
import json
import math
import os
import subprocess
import sys
import time

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)
sys.path.insert(0, os.path.join(_R, "tests"))
import numpy as np

PEAK_FP64_MFMA = 78.6e12
FLOP_PER_PAIR = 16 * 5 * 2 * 16 * 16 * 4      # 16 tiles x 5 k-steps of v_mfma_f64_16x16x4_f64 (issued, the 64 x 64 padding included)
STEP_TIMEOUT = {"add": 240, "ref": 240, "exh": 420, "host": 900}


def make_clouds(n, seed=7, places=40, fill=0.45):
    rng = np.random.default_rng(seed)
    sky = rng.uniform(0.3, 9.0, (places, 20, 60)) * (rng.random((places, 20, 60)) < fill)
    clouds = []
    for k in range(n):
        d = np.roll(sky[rng.integers(places)], rng.integers(60), axis=1)
        ring, sec = np.nonzero(d)
        z = d[ring, sec] + rng.normal(0, 0.05, ring.size) - 2.0
        rad, ang = (ring + 0.5) * 4.0, np.deg2rad((sec + 0.5) * 6.0)
        clouds.append(np.column_stack([rad * np.cos(ang), rad * np.sin(ang), z, np.ones(ring.size)]).astype(np.float32))
    return clouds


def pair_counts(n, exhaustive, exclude=30, period=30, k=3):
    """(candidate pairs, searched (pair, shift) distances) of a replay over key frames 0 .. n - 1"""
    pairs = 0
    for q in range(exclude, n):
        snap = period * ((q - exclude) // period) + 1
        pairs += snap if exhaustive else min(k, snap)
    return pairs, pairs * (60 if exhaustive else 7)


def gpu_step(step, n):
    from vil_fusion_amd.estimator import BackendSolver, ScanContext
    clouds = make_clouds(n)
    s = BackendSolver()
    over = dict(num_candidates=0, search_ratio=1.0) if step == "exh" else {}
    sc = ScanContext(s, capacity=n, **over)
    sc.add_many(clouds)                                  # warm-up: allocations, code object load
    if step != "add":
        sc.detect_range(0, 64)
    out = dict(step=step, n=n, points=int(sum(len(c) for c in clouds)))
    reps = []
    for _ in range(3):
        if step == "add":
            sc = ScanContext(s, capacity=n, **over)
        s._check(s._L.vilf_set_profiling(s._h, 1), "vilf_set_profiling")
        t = time.perf_counter()
        if step == "add":
            sc.add_many(clouds)                          # wall time includes the host-side concatenation of the clouds
        else:
            res = sc.detect_range()
        wall = time.perf_counter() - t
        prof = sc.profile()
        s._check(s._L.vilf_set_profiling(s._h, 0), "vilf_set_profiling")
        reps.append(dict(wall_ms=1e3 * wall, **{k: v[0] for k, v in prof.items() if v[1]}))
    out["runs"] = reps
    if step != "add":
        pairs, dists = pair_counts(n, step == "exh")
        out.update(pairs=pairs, distances=dists, loops=sum(r["loop_id"] >= 0 for r in res), below_0p4=sum(r["min_dist"] < 0.4 for r in res))
        ms = min(r["sc_distance"] for r in reps)
        out.update(sc_distance_ms=ms, issued_mfma_flop=pairs * FLOP_PER_PAIR, mfma_tflops=pairs * FLOP_PER_PAIR / (ms * 1e-3) / 1e12,
                   mfma_peak_fraction=pairs * FLOP_PER_PAIR / (ms * 1e-3) / PEAK_FP64_MFMA)
    s.close()
    return out


def host_step(n, sample=24):
    import sc_reference as R
    clouds = make_clouds(n)
    out = dict(step="host", n=n)
    descs = [R.make_descriptor(c, R.Params()) for c in clouds]
    for mode, over in (("ref", {}), ("exh", dict(num_candidates=0, search_ratio=1.0))):
        p = R.Params(**over)
        m = R.SCManager(p)
        m.descs, m.rkeys = descs, [R.ring_key(d) for d in descs]
        qs = np.linspace(30, n - 1, sample if mode == "exh" else 8 * sample).astype(int)
        done = 0
        t = time.perf_counter()
        for q in qs:                                  # detect() of key frame q with the snapshot the replay gives it
            mq = R.SCManager(p)
            mq.descs, mq.rkeys = descs[:q + 1], m.rkeys[:q + 1]
            mq.calls, mq.snapshot = 1, 30 * ((q - 30) // 30) + 1
            done += mq.detect()["n_candidates"]
        dt = time.perf_counter() - t
        pairs, _ = pair_counts(n, mode == "exh")
        out[mode] = dict(sampled_queries=len(qs), sampled_pairs=done, sampled_s=dt, replay_pairs=pairs, replay_s_scaled=dt * pairs / max(done, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--step", choices=["add", "ref", "exh", "host"])
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.step:
        print(json.dumps(host_step(a.n) if a.step == "host" else gpu_step(a.step, a.n)))
        return 0
    lines = []
    for step in ("add", "ref", "exh", "host"):
        r = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--n", str(a.n)],
                           stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            print(f"step {step} ended with status {r.returncode}: nothing more is started", file=sys.stderr)
            return r.returncode
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        lines.append(json.loads(line))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(lines, fh, indent=1)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
