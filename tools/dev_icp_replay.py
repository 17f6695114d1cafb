#!/usr/bin/env python3
"""Loop-candidate ICP replay timing: the candidates of tests/icp_reference.loop_route (12 pairs: 8 revisits with a small heading change, 4 with a
large one; sources of ~3.4 k points against targets of ~12 k points after the voxel filter), replicated --copies times for the batched run.
  single   vilf_icp_align per candidate: latency per candidate (wall, the whole call: sub-maps, grid, rounds, fitness, one wait)
  batch    vilf_icp_align_pairs over all copies in one chain of launches: candidates per second
  host     tests/icp_reference.py on the same candidates: numpy + scipy cKDTree on the host CPU, NOT PCL: context only
Kernel times are HIP events under vilf_set_profiling (vilf_get_profile_icp), taken in runs of their own: the events serialise the chain, the wall times come from
runs without them. Bytes of the search: every (query, target point) distance evaluated would read 16 B; the figure reported is the lower bound rounds x
(source read + write, 32 B per point) + the target once per round, against the HBM figure of DESIGN.md.

  python tools/dev_icp_replay.py [--copies 16] [--out FILE.json]   # runs the steps as child processes, each GPU step under its own `timeout`, stops at the first that fails
  python tools/dev_icp_replay.py --step single|batch|host          # one step in this process; prints one JSON line
  python tools/dev_icp_replay.py --gaps KERNEL_TRACE.csv [--out FILE.json]   # no GPU: the idle time between consecutive icp_search / icp_step launches in the kernel trace of
                                                                    # `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/dev_icp_replay.py --step single`
                                                                    # (does the host wait between rounds?) and the per-kernel totals of that trace"""
import argparse
import json
import os
import subprocess
import sys
import time

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)
sys.path.insert(0, os.path.join(_R, "tests"))
import numpy as np

HBM_BYTES_PER_S = 8.0e12            # MI355X HBM3E peak, the figure DESIGN.md measures against
STEP_TIMEOUT = {"single": 240, "batch": 240, "host": 600}
REPEATS = 5


def gpu_step(step, copies):
    import icp_reference as R
    from vil_fusion_amd.estimator import BackendSolver, LoopICP
    clouds, poses, pairs = R.loop_route()
    pr = [(a, b) for a, b, _ in pairs]
    s = BackendSolver()
    icp = LoopICP(s, cap_keyframes=len(clouds), cap_points=sum(len(c) for c in clouds))
    icp.add_many(clouds)
    out = dict(step=step, candidates=len(pr))
    if step == "single":
        for a, b in pr:                                  # warm-up: allocations, code object load
            icp.align(a, b, poses)
        lat = []
        for _ in range(REPEATS):
            row = []
            for a, b in pr:
                t0 = time.perf_counter(); res = icp.align(a, b, poses); row.append((time.perf_counter() - t0) * 1e3)
            lat.append(row)
        lat = np.array(lat)
        results = [icp.align(a, b, poses) for a, b in pr]
        out.update(latency_ms_best=lat.min(0).tolist(), latency_ms_median=np.median(lat, 0).tolist(), mean_latency_ms=float(np.median(lat, 0).mean()),
                   rounds=[r["iterations"] for r in results], mean_rounds=float(np.mean([r["iterations"] for r in results])),
                   accepted=[bool(r["accepted"]) for r in results], n_source=[r["n_source"] for r in results], n_target=[r["n_target"] for r in results])
        s._check(s._L.vilf_set_profiling(s._h, 1), "vilf_set_profiling")
        for a, b in pr:
            icp.align(a, b, poses)
        prof = icp.profile()
        out["kernel_ms_per_candidate"] = {k: v[0] / len(pr) for k, v in prof.items()}
        out["kernel_launches_per_candidate"] = {k: v[1] / len(pr) for k, v in prof.items()}
        # lower bound of the search traffic: per round the source read and written (32 B per point) and the target read once (16 B per point); + the fitness pass
        byt = sum((r["iterations"] + 1) * (32 * r["n_source"] + 16 * r["n_target"]) for r in results)
        live = sum(r["iterations"] + 1 for r in results)
        srch = prof["icp_search"]
        out.update(search_bytes_lower_bound=byt, search_live_launches=live, search_ms_total=srch[0],
                   search_bytes_per_s=byt / (srch[0] * 1e-3) if srch[0] > 0 else None, hbm_fraction=byt / (srch[0] * 1e-3) / HBM_BYTES_PER_S if srch[0] > 0 else None)
    else:
        big = pr * copies
        icp.align_pairs(big, poses)
        wall = []
        for _ in range(REPEATS):
            t0 = time.perf_counter(); res = icp.align_pairs(big, poses); wall.append((time.perf_counter() - t0) * 1e3)
        out.update(pairs=len(big), wall_ms=wall, wall_ms_best=min(wall), candidates_per_s=len(big) / (np.median(wall) * 1e-3),
                   identical_to_first_copy=all(res[i]["transform"].tobytes() == res[i % len(pr)]["transform"].tobytes() and res[i]["fitness"] == res[i % len(pr)]["fitness"] for i in range(len(big))))
        s._check(s._L.vilf_set_profiling(s._h, 1), "vilf_set_profiling")
        icp.align_pairs(big, poses)
        out["kernel_ms"] = {k: v[0] for k, v in icp.profile().items()}
    s.close()
    return out


def host_step():
    import icp_reference as R
    clouds, poses, pairs = R.loop_route()
    t0 = time.perf_counter()
    res = [R.align_pair(clouds, poses, a, b, both=False) for a, b, _ in pairs]
    dt = time.perf_counter() - t0
    return dict(step="host", what="numpy + scipy cKDTree restatement on the host CPU (not PCL)", candidates=len(pairs), seconds=dt, ms_per_candidate=dt * 1e3 / len(pairs),
                rounds=[r["iterations"] for r in res])


def trace_gaps(path):
    import csv
    rows = list(csv.DictReader(open(path)))
    total = {}
    for r in rows:
        name = r["Kernel_Name"].replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0].split("<")[0]
        c = total.setdefault(name, [0, 0])
        c[0] += 1; c[1] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    rounds = sorted((r for r in rows if r["Kernel_Name"].startswith(("icp_search", "icp_step"))), key=lambda r: int(r["Start_Timestamp"]))
    gaps = np.array([int(b["Start_Timestamp"]) - int(a["End_Timestamp"]) for a, b in zip(rounds, rounds[1:])])
    calls = sum(1 for r in rows if r["Kernel_Name"].startswith("icp_voxel"))
    return dict(what="idle ns between consecutive icp_search / icp_step launches of one process (tools/dev_icp_replay.py --step single under rocprofv3 --kernel-trace); "
                     "a host wait between rounds would show as one long gap per round, the boundaries between align calls do show",
                launches=len(rounds), align_calls=calls, gap_ns_median=float(np.median(gaps)), gap_ns_p90=float(np.percentile(gaps, 90)), gap_ns_p99=float(np.percentile(gaps, 99)),
                gaps_above_50us=int((gaps > 50000).sum()), kernels={k: dict(calls=v[0], total_ms=v[1] * 1e-6) for k, v in sorted(total.items(), key=lambda kv: -kv[1][1])})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=["single", "batch", "host"])
    ap.add_argument("--gaps", default=None)
    a = ap.parse_args()
    if a.gaps:
        out = trace_gaps(a.gaps)
        print(json.dumps(out))
        if a.out:
            with open(a.out, "w") as fh:
                json.dump(out, fh, indent=1)
                fh.write("\n")
        return
    if a.step:
        print(json.dumps(host_step() if a.step == "host" else gpu_step(a.step, a.copies)))
        return
    result = dict(tool="tools/dev_icp_replay.py", copies=a.copies, repeats=REPEATS, note="one run on one MI355X; wall times include the copies and the Python side")
    for step in ("single", "batch", "host"):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--copies", str(a.copies)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            print(f"step {step} failed with status {p.returncode}; nothing more is started\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            sys.exit(1)
        result[step] = json.loads(p.stdout.strip().splitlines()[-1])
        print(step, json.dumps(result[step])[:400])
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
