#!/usr/bin/env python3
"""bench.py — sliding-window solve iterations/s on MI355X (BASELINE.json metric), one process per GPU.

A "step" = one pass of the hot path over one batch of synthetic input. The unit is a FRAME of BASELINE.json configs[2]:
  * the LiDAR stage: one scan-to-map step (EstimationMapping::optimation_processing) — voxel down-sampling, radix-hashed
    voxel 5-NN, ~1.2 k edge + ~2.8 k plane queries -> ~3-4 k edge/plane factors, 2 x <= 4 LM iterations, local-map update
    against a ~30 k + ~78 k point local map;
  * the back-end: the full Estimator::optimization() solve of the 11-frame window (~1.5 k visual factors, 10 IMU, 10 LiDAR
    between-factors, prior; Ceres-configured dogleg, max 8 iterations, time limit off).
Every rank re-arms its B HBM-resident frames (window snapshots + LiDAR streams), runs both stages on all of them, then gathers
the newest-frame poses over RCCL (the global_fusion input). Frames are independent units, sharded over ranks with no data-path
collective => weak scaling. `value` counts the window solver's iterations only; the LiDAR stage is inside the timed region.

  python bench.py --gpus 1 --steps 10 --warmup 2
  python bench.py --gpus 1 --steps 10 --warmup 2 --full        # + the side legs: CPU baseline, overlapped stages, ragged / converging / PCIe-inclusive /
                                                                #   estimate_td batches, single-frame latency, the compact configs[4] leg
  python bench.py --gpus 1 --steps 10 --warmup 2 --dump-outputs DIR   # + what the last timed step computed, as DIR/<name>.npy
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

A plain run sets up, warms up, times the steps (with the per-kernel spans that the roofline is read from) and prints the line; everything
else it measures runs only with --full. Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def algorithmic_bytes_per_iteration(win, prior, part="all"):
    """fused-minimum bytes of one solver iteration (inputs read once, reduced system written once).
    part: "all" (the §8d figure, charged to the linearisation kernel), "reduced" (the reduced system + per-feature terms the
    solve kernel consumes), "inputs" (factor inputs + prior + state the step kernel re-reads for the candidate cost)."""
    n_vis = win.n_factors
    n_imu = win.n_frames - 1
    n_lid = win.n_frames - 1 if win.lidar is not None else 0
    n_p = prior.n if (prior is not None and prior.valid) else 0
    k_p = prior.n_blocks if (prior is not None and prior.valid) else 0
    F = win.n_features
    P = 15 * win.n_frames
    inputs = 60 * n_vis + 2296 * n_imu + 56 * n_lid + 8 * (n_p * n_p + n_p + 7 * k_p) + 8 * (16 * win.n_frames + 8 + F)
    reduced = 16 * F + 8 * (P * P + P)
    return {"all": inputs + reduced, "reduced": reduced + 8 * (n_p * n_p + n_p), "inputs": inputs}[part]


def cpu_baseline(opts_unused, wins, priors, lidar_cases, marginalize, seconds_target=12.0):
    """The CPU restatement (oracle/, 'port') timed on this box's host cores on a bounded sample of the same frames."""
    import numpy as np
    from concurrent.futures import ThreadPoolExecutor
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib
    oracle_lib.build()
    o = oracle_lib.default_options()
    cores = max(1, min(16, os.cpu_count() or 1))
    ident = np.array([0, 0, 0, 1, 0, 0, 0.0])
    prepared = []                                  # per distinct scene: the oracle after the same warm-up frame (untimed)
    for c in lidar_cases:
        me, ms, scans, pl = c[4]
        m = oracle_lib.OracleS2M(o); m.init(me, ms); m.set_pose(ident, pl); m.step(*scans[0])
        prepared.append((m, scans[1]))

    def frame(i):
        if prepared:
            m, (se, ss) = prepared[i % len(prepared)]
            m.clone().step(se, ss)
        res = oracle_lib.window_solve(o, wins[i % len(wins)], priors[i % len(priors)])
        if marginalize:
            oracle_lib.window_marginalize(o, wins[i % len(wins)], res, priors[i % len(priors)])
        return res.summary["num_iterations"]
    t0 = time.perf_counter()
    frame(0)                                   # calibrate on one frame
    t1 = time.perf_counter() - t0
    n = int(max(cores, min(32768, seconds_target * cores / max(t1, 1e-4))))
    t0 = time.perf_counter()
    with ThreadPoolExecutor(cores) as ex:
        its = sum(ex.map(frame, range(n)))
    dt = time.perf_counter() - t0
    # second leg at the reference's own thread count (num_threads = 4, NUM_THREADS = 4: estimator.cpp:841, marginalization_factor.h:13), ~5 s
    n4 = int(max(4, min(n, 5.0 * 4 / max(t1, 1e-4))))
    t0 = time.perf_counter()
    with ThreadPoolExecutor(4) as ex:
        its4 = sum(ex.map(frame, range(n4)))
    dt4 = time.perf_counter() - t0
    what = ("scan-to-map step (1 m grid 5-NN) + " if lidar_cases else "") + "window solve" + (" + marginalization" if marginalize else "")
    # one frame alone on one thread (the oracle has no threads inside a frame; Ceres in the reference uses 4 inside its solve): the latency reference
    tl = time.perf_counter(); r1 = oracle_lib.window_solve(o, wins[0], priors[0]); tl1 = time.perf_counter()
    oracle_lib.window_marginalize(o, wins[0], r1, priors[0]); tl2 = time.perf_counter()
    lat = {"window_solve_ms": 1e3 * (tl1 - tl), "marginalize_ms": 1e3 * (tl2 - tl1)}
    if prepared:
        m, (se, ss) = prepared[0]
        mc = m.clone(); tl3 = time.perf_counter(); mc.step(se, ss); lat["scan_to_map_frame_ms"] = 1e3 * (time.perf_counter() - tl3)
    return dict(single_frame_latency_1_thread=lat, value=its / dt, unit="iterations/s", cores=cores, kind="port",
                sample=f"{n} frames ({its} window iterations; per frame: {what}) of the same synthetic input by oracle/ "
                       f"(C++ -O3, one frame per thread, {cores} threads), {dt:.1f} s; at the reference's 4 threads: {n4} frames in {dt4:.1f} s",
                value_4_threads=its4 / dt4)


def lidar_search_statistics(cases, opts):
    """What the 5-NN of the LiDAR stage touches, counted on the host from the steady-state maps: cells are 0.8 m x 0.8 m (two edge leaves, one surf leaf), a query visits the
    rows / columns of cells that [q - 1.001, q + 1.001] m covers. The raw scan points, moved by the pose after the warm-up frame, stand in for the down-sampled queries.
    Returns averages per query (weighted by the edge / surf query counts of the scene) and the occupied cells per frame (both maps)."""
    import numpy as np
    from vil_fusion_amd import synth
    tot_c = tot_r = tot_q = 0.0; cells = []
    for me, ms, (se, ss), pose, _ in cases:
        R = synth.q_to_R(np.asarray(pose[:4])); t = np.asarray(pose[4:])
        ncell = 0
        for m, sc, leaf in ((me, se, float(opts.edge_leaf_size)), (ms, ss, float(opts.surf_leaf_size))):
            k = 1
            while leaf * k < 0.5:
                k *= 2
            c = leaf * k
            ij = np.floor(np.asarray(m)[:, :2] / c).astype(np.int64)
            lo = ij.min(0) - 4; ext = ij.max(0) - lo + 5
            grid = np.zeros((ext[1] + 1, ext[0] + 1)); np.add.at(grid, (ij[:, 1] - lo[1] + 1, ij[:, 0] - lo[0] + 1), 1.0)
            ncell += int((grid > 0).sum())
            sat = grid.cumsum(0).cumsum(1)
            q = (np.asarray(sc)[::7, :3] @ R.T + t)[:, :2]
            a = np.clip(np.floor((q - 1.001) / c).astype(np.int64) - lo, 0, ext - 1); b_ = np.clip(np.floor((q + 1.001) / c).astype(np.int64) - lo, 0, ext - 1)
            cnt = sat[b_[:, 1] + 1, b_[:, 0] + 1] - sat[a[:, 1], b_[:, 0] + 1] - sat[b_[:, 1] + 1, a[:, 0]] + sat[a[:, 1], a[:, 0]]
            tot_c += float(cnt.sum()); tot_r += float((b_[:, 1] - a[:, 1] + 1).sum()); tot_q += len(q)
        cells.append(ncell)
    return dict(candidates_per_query=tot_c / max(tot_q, 1), rows_per_query=tot_r / max(tot_q, 1), map_cells=float(np.mean(cells)))


def host_cpus():
    """CPUs this process may use: its affinity mask, capped by a cgroup CPU quota and by OMP_NUM_THREADS where either is set (os.cpu_count() counts the whole machine)"""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(quota) // int(period)))
    except (OSError, ValueError):
        pass
    omp = os.environ.get("OMP_NUM_THREADS", "")
    if omp.isdigit() and int(omp) > 0:
        n = min(n, int(omp))
    return max(1, n)


DUMP_MAX_WINDOWS = 4096          # --dump-outputs: per-window arrays of at most this many windows (a seeded sample beyond it)
DUMP_PRIORS = 64                 # new priors of a seeded sample of this many windows (one prior is up to 75 x 75 doubles)
DUMP_MAPS = 4                    # local maps (edge + surf, ~0.1 M points each) of a seeded sample of this many LiDAR streams
DUMP_MAX_BYTES = 64 << 20


def dump_outputs(path, solver, s2m, B, marginalized, table=None, seed=2024):
    """--dump-outputs DIR: what the timed path handed its caller in the LAST timed step, one DIR/<name>.npy each (float64; the local maps float32, as the library
    returns them). Windows are slots of the batch, in slot order (window_index: which slots, when B exceeds DUMP_MAX_WINDOWS):
      window_para_pose (S, 11, 7), window_para_speed_bias (S, 11, 9), window_para_feature (S, Fmax; zero past window_n_features), window_Ps / Rs / Vs / Bas / Bgs,
      window_summary (S, 7): num_iterations, num_successful_steps, num_linear_solves, termination, initial_cost, final_cost, final_radius (no timings);
      prior_index / prior_valid / prior_n / prior_residuals (P, nmax) / prior_jacobians (P, nmax, nmax): the marginalization's new priors of a seeded sample of slots;
      lidar_pose_qt (S, 7), lidar_rel_q (S, 4), lidar_rel_t (S, 3), lidar_final_cost (S, 2), lidar_counts (S, 10): n_edge_ds, n_surf_ds, n_edge_factors[2],
      n_surf_factors[2], iterations[2], map_edge_size, map_surf_size; lidar_map_index, lidar_map_{edge,surf}_<slot> (n, 4) of a seeded sample of streams;
      gathered_poses (world * B, 8): the pose table of the gather (N > 1).
    Returns the bytes written."""
    import numpy as np
    rng = np.random.default_rng(seed)
    idx = np.arange(B) if B <= DUMP_MAX_WINDOWS else np.sort(rng.choice(B, DUMP_MAX_WINDOWS, replace=False))
    out = {"window_index": idx.astype(np.float64)}
    res = solver.batch_download()
    sm = solver.batch_summaries()
    nf = np.array([len(res[i].para_feature) for i in idx])
    feat = np.zeros((len(idx), max(int(nf.max()), 1)))
    for r, i in enumerate(idx):
        feat[r, :nf[r]] = res[i].para_feature
    out.update(window_para_pose=np.stack([res[i].para_pose for i in idx]), window_para_speed_bias=np.stack([res[i].para_speed_bias for i in idx]),
               window_para_feature=feat, window_n_features=nf.astype(np.float64))
    for k in ("Ps", "Rs", "Vs", "Bas", "Bgs"):
        out["window_" + k] = np.stack([getattr(res[i], k) for i in idx])
    out["window_summary"] = np.array([[sm[i].num_iterations, sm[i].num_successful_steps, sm[i].num_linear_solves, sm[i].termination,
                                       sm[i].initial_cost, sm[i].final_cost, sm[i].final_radius] for i in idx], dtype=np.float64)
    if marginalized:
        pidx = np.sort(rng.choice(B, min(B, DUMP_PRIORS), replace=False))
        pri = [solver.get_prior(int(i)) for i in pidx]
        pn = np.array([p.n if p.valid else 0 for p in pri])
        nmax = max(int(pn.max()), 1)
        pr = np.zeros((len(pidx), nmax)); pj = np.zeros((len(pidx), nmax, nmax))
        for r, p in enumerate(pri):
            n = int(pn[r])
            pr[r, :n] = np.frombuffer(p.linearized_residuals, dtype=np.float64, count=n)
            pj[r, :n, :n] = np.frombuffer(p.linearized_jacobians, dtype=np.float64, count=n * n).reshape(n, n)
        out.update(prior_index=pidx.astype(np.float64), prior_valid=np.array([p.valid for p in pri], dtype=np.float64), prior_n=pn.astype(np.float64),
                   prior_residuals=pr, prior_jacobians=pj)
    if s2m is not None:
        rs = s2m.results()
        out.update(lidar_pose_qt=np.array([rs[i].pose_qt[:] for i in idx]), lidar_rel_q=np.array([rs[i].rel_q[:] for i in idx]),
                   lidar_rel_t=np.array([rs[i].rel_t[:] for i in idx]), lidar_final_cost=np.array([rs[i].final_cost[:] for i in idx]),
                   lidar_counts=np.array([[rs[i].n_edge_ds, rs[i].n_surf_ds, *rs[i].n_edge_factors, *rs[i].n_surf_factors, *rs[i].iterations,
                                           rs[i].map_edge_size, rs[i].map_surf_size] for i in idx], dtype=np.float64))
        midx = np.sort(rng.choice(B, min(B, DUMP_MAPS), replace=False))
        out["lidar_map_index"] = midx.astype(np.float64)
        for i in midx:
            out[f"lidar_map_edge_{i}"] = s2m.getMapCloud(int(i), 0)
            out[f"lidar_map_surf_{i}"] = s2m.getMapCloud(int(i), 1)
    if table is not None:
        out["gathered_poses"] = np.asarray(table, dtype=np.float64)
    return write_dump(path, out)


def write_dump(path, arrays):
    """DIR/<name>.npy for every array (at most DUMP_MAX_BYTES in all); returns the bytes written"""
    import numpy as np
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_MAX_BYTES:
        raise SystemExit(f"--dump-outputs: {total / 2**20:.1f} MB of outputs exceed the {DUMP_MAX_BYTES >> 20} MB budget")
    os.makedirs(path, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(path, k + ".npy"), a)
    return total


def _profile_order(path):
    """profiles/rNN_vMM_*: round, then version, numerically (r01_v10 after r01_v9)"""
    import re
    m = re.search(r"r(\d+)_v(\d+)", os.path.basename(path))
    return (int(m.group(1)), int(m.group(2))) if m else (0, 0)


def stress_leg(local_rank, n_windows=8, steps=3):
    """BASELINE configs[4] inside the default run, so that the driver times it: ONE group of `n_windows` independent 51-frame / ~46 k-factor windows
    (vilf_window_solve_group), `steps` solves after one warm-up; aggregate iterations/s + the general path's launch groups. Never `value`."""
    import torch
    from vil_fusion_amd import synth
    from vil_fusion_amd.estimator import BackendSolver
    from vil_fusion_amd.lib import default_options
    o = default_options(); o.window_size = 50
    distinct = [synth.make_window(900 + 7 * k, o, synth.SynthConfig(n_frames=51, n_features=2500, with_prior=False))[0] for k in range(min(n_windows, 2))]
    wl = [distinct[k % len(distinct)] for k in range(n_windows)]
    s = BackendSolver(o, device=local_rank)
    grp = s.prepare_group(wl)                      # the caller's structs, built once (a C++ caller holds them anyway)
    s.solve_group(grp)                             # warm-up: arena allocated
    torch.cuda.synchronize(); t0 = time.perf_counter(); its = 0
    for _ in range(steps):
        its += sum(o.summary.num_iterations for o in s.solve_group(grp, finish=False))
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    s.set_profiling(True)                          # launch groups of ONE more solve (profiling waits per group: outside the timed loop)
    s.solve_group(grp, finish=False)
    prof = s.get_profile_large_window()
    s.close()
    w = distinct[0]
    P, F = 15 * 51, w.n_features
    alg_schur, issued_schur, _ = schur_flops(w)              # 2 sum_f (6 k_f)^2, and what the span-aware MFMA reduce issues for it
    nsol = max(prof["lw_cholesky"]["launches"], 1)
    syrk_s = max(prof["lw_schur_syrk"]["ms"] * 1e-3, 1e-12)
    return {"value": its / dt, "unit": "iterations/s", "windows": n_windows, "steps": steps, "ms_per_group_solve": 1e3 * dt / steps, "iterations": its,
            "frames": 51, "features": int(F), "visual_factors": int(len(w.obs_point) - F), "reduced_system": P,
            "kernels_ms_per_group_solve": {k: v["ms"] for k, v in prof.items()},
            "schur_algorithmic_flop_per_window_iteration": alg_schur, "schur_issued_flop_per_window_iteration": issued_schur,
            "schur_reduce": {"launches": nsol, "ms_per_launch": prof["lw_schur_syrk"]["ms"] / nsol, "TFLOPs_algorithmic": alg_schur * n_windows * nsol / syrk_s / 1e12,
                             "TFLOPs_issued": issued_schur * n_windows * nsol / syrk_s / 1e12, "frac_of_fp64_mfma_peak_issued": issued_schur * n_windows * nsol / syrk_s / 1e12 / 78.6,
                             "frac_of_fp64_mfma_peak_algorithmic": alg_schur * n_windows * nsol / syrk_s / 1e12 / 78.6},
            "cholesky_flop_per_window_iteration": P ** 3 / 3.0 + 2.0 * P * P,
            "cholesky": {"launches": nsol, "ms_per_factorisation_of_all_windows": prof["lw_cholesky"]["ms"] / nsol,
                         "TFLOPs": (P ** 3 / 3.0 + 2.0 * P * P) * n_windows * nsol / max(prof["lw_cholesky"]["ms"] * 1e-3, 1e-12) / 1e12,
                         "frac_of_fp64_mfma_peak": (P ** 3 / 3.0 + 2.0 * P * P) * n_windows * nsol / max(prof["lw_cholesky"]["ms"] * 1e-3, 1e-12) / 1e12 / 78.6},
            "distinct_windows": len(distinct),
            "what": "configs[4]: vilf_window_solve_group of %d independent 51-frame windows (%d distinct synthetic windows, replicated: ~40 s of host ray casting each), host buffers in / out, pack + upload inside, general path (vilf_lw.hip)" % (n_windows, len(distinct))}


def schur_flops(w, kb=32):
    """SURVEY 8(d)'s algorithmic flops of the Schur reduce of one window, 2 sum_f (6 k_f)^2 over the non-constant features (k_f = frames that see feature f), and what
    lw_syrk_mfma issues for it: 64 x 64 tiles of the lower triangle over the compact pose columns x chunks of `kb` features in (start frame, track length) order whose
    frame span reaches the tile's rows and columns — 2 * kb * 64 * 64 flop each (the kernel's own skip rule, restated on the host)."""
    import numpy as np
    st = np.asarray(w.feature_start_frame); nobs = np.diff(w.feature_obs_offset); cst = np.asarray(w.feature_const)
    alg = 2.0 * float(np.sum((6.0 * nobs[(cst == 0) & (nobs >= 2)]) ** 2))
    order = np.lexsort((np.minimum(nobs, w.n_frames), st))
    nt = (6 * w.n_frames + 63) // 64
    tiles = 0
    for q in range((len(st) + kb - 1) // kb):
        fs = order[kb * q: kb * q + kb]; fs = fs[(cst[fs] == 0) & (nobs[fs] >= 2)]
        if len(fs) == 0:
            continue
        lo = int((6 * st[fs]).min()); hi = int((6 * (st[fs] + nobs[fs] - 1) + 5).max())
        t0, t1 = lo // 64, min(nt - 1, hi // 64)
        tiles += (t1 - t0 + 1) * (t1 - t0 + 2) // 2
    return alg, tiles * 2.0 * kb * 64 * 64, tiles


def np_diff_nonconst(w):
    import numpy as np
    return np.diff(w.feature_obs_offset)[np.asarray(w.feature_const) == 0].astype(np.float64)


def stress_main(args):
    """BASELINE configs[4]: the 51-frame stress window through vilf_window_solve's general path; a step = one window solve per GPU (independent
    windows per rank, no collective). Reports solver iterations/s and the fp64 MFMA roofline of the Schur SYRK (2 F P^2 flop per linear solve)."""
    import numpy as np
    import torch
    rank = int(os.environ.get("RANK", "0")); local_rank = int(os.environ.get("LOCAL_RANK", "0")); world = int(os.environ.get("WORLD_SIZE", "1"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the solve path has no CPU fallback")
    rehearse = os.environ.get("VILF_BENCH_REHEARSAL") == "1"
    if rehearse:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if rehearse:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
    from vil_fusion_amd import synth
    from vil_fusion_amd.estimator import BackendSolver
    from vil_fusion_amd.lib import default_options
    opts = default_options(); opts.window_size = 50
    win, _, _ = synth.make_window(900 + rank, opts, synth.SynthConfig(n_frames=51, n_features=2500, with_prior=False))
    solver = BackendSolver(opts, device=local_rank)
    for _ in range(max(args.warmup, 1)):
        res = solver.optimization(win)

    # ---- S independent stress windows at once. A single window's solve is a chain of ~32 small launches per iteration on a handful of workgroups (12 sequential panel
    # steps per factorisation), so the chip is filled by solving windows side by side. "group" (default): vilf_window_solve_group — ONE chain of launches, every kernel
    # finds its window in blockIdx.z. "streams": one handle (= HIP stream, workspace) and one host thread per window — the runtime multiplexes its streams onto four
    # hardware queues, so that tops out near 3 k iterations/s; kept for comparison. Aggregate iterations/s; no per-kernel profiling here.
    sweep = []
    if world == 1:
        import threading
        Pn = 15 * 51
        for S_ in [int(x) for x in args.stress_windows.split(",") if x.strip()]:
            wins_ = [win] + [synth.make_window(900 + 7 * k, opts, synth.SynthConfig(n_frames=51, n_features=2500, with_prior=False))[0] for k in range(1, min(S_, 4))]
            wl = [wins_[k % len(wins_)] for k in range(S_)]
            if args.stress_mode == "group":
                grp = solver.prepare_group(wl)                                  # the caller's structs, built once
                solver.solve_group(grp)                                         # warm-up: arena allocated
                torch.cuda.synchronize(); t0 = time.perf_counter()
                nits = 0
                for _ in range(args.steps):
                    nits += sum(o.summary.num_iterations for o in solver.solve_group(grp, finish=False))
                torch.cuda.synchronize(); dts = time.perf_counter() - t0
            else:
                hs = [solver] + [BackendSolver(opts, device=local_rank) for _ in range(S_ - 1)]
                for k, h_ in enumerate(hs):
                    h_.optimization(wl[k])                                      # warm-up: workspaces allocated
                its_ = [0] * S_

                def work(k):
                    for _ in range(args.steps):
                        its_[k] += hs[k].optimization(wl[k]).summary["num_iterations"]
                torch.cuda.synchronize(); t0 = time.perf_counter()
                th = [threading.Thread(target=work, args=(k,)) for k in range(S_)]
                for t_ in th:
                    t_.start()
                for t_ in th:
                    t_.join()
                torch.cuda.synchronize(); dts = time.perf_counter() - t0
                nits = sum(its_)
                for h_ in hs[1:]:
                    h_.close()
            row = {"windows": S_, "mode": args.stress_mode, "value": nits / dts, "unit": "iterations/s", "ms_per_solve_of_all_windows": 1e3 * dts / args.steps}
            if args.stress_mode == "group":      # the launch groups of ONE more group solve with per-group waits (outside the timed loop), Schur reduce priced on SURVEY 8(d)'s flops and on the issued ones
                solver.set_profiling(True); p0 = solver.get_profile_large_window()
                solver.solve_group(grp, finish=False)
                p1 = solver.get_profile_large_window(); solver.set_profiling(False)
                dms = {k: p1[k]["ms"] - p0[k]["ms"] for k in p1}; nl = max(p1["lw_schur_syrk"]["launches"] - p0["lw_schur_syrk"]["launches"], 1)
                fl = [schur_flops(w_) for w_ in wl]
                alg_f, iss_f = sum(f_[0] for f_ in fl), sum(f_[1] for f_ in fl)
                ssec = max(dms["lw_schur_syrk"] * 1e-3, 1e-12); csec = max(dms["lw_cholesky"] * 1e-3, 1e-12)
                row.update({"kernels_ms_per_group_solve": dms, "linear_solves": nl,
                            "schur_reduce": {"ms_per_launch": dms["lw_schur_syrk"] / nl, "algorithmic_flop_per_launch": alg_f, "issued_flop_per_launch": iss_f,
                                             "TFLOPs_algorithmic": alg_f * nl / ssec / 1e12, "TFLOPs_issued": iss_f * nl / ssec / 1e12,
                                             "frac_of_fp64_mfma_peak_algorithmic": alg_f * nl / ssec / 1e12 / 78.6, "frac_of_fp64_mfma_peak_issued": iss_f * nl / ssec / 1e12 / 78.6},
                            "cholesky": {"ms_per_factorisation_of_all_windows": dms["lw_cholesky"] / nl, "TFLOPs": (Pn ** 3 / 3.0 + 2.0 * Pn * Pn) * S_ * nl / csec / 1e12,
                                         "frac_of_fp64_mfma_peak": (Pn ** 3 / 3.0 + 2.0 * Pn * Pn) * S_ * nl / csec / 1e12 / 78.6}})
            sweep.append(row)
    solver.set_profiling(True)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
    barrier()
    t0 = time.perf_counter(); its = 0
    for _ in range(args.steps):
        res = solver.optimization(win); its += res.summary["num_iterations"]
    barrier()
    dt = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:               # the last timed solve of this rank's stress window, as vilf_window_solve returned it
        sm = res.summary
        write_dump(args.dump_outputs, {"window_para_pose": res.para_pose, "window_para_speed_bias": res.para_speed_bias, "window_para_feature": res.para_feature,
                                       "window_Ps": res.Ps, "window_Rs": res.Rs, "window_Vs": res.Vs, "window_Bas": res.Bas, "window_Bgs": res.Bgs,
                                       "window_summary": np.array([sm[k] for k in ("num_iterations", "num_successful_steps", "num_linear_solves", "termination",
                                                                                   "initial_cost", "final_cost", "final_radius")], dtype=np.float64)})
    prof = solver.get_profile_large_window()
    t = torch.tensor([dt, float(its)], dtype=torch.float64, device="cpu" if rehearse else "cuda")
    if world > 1:
        tmax = t.clone(); dist.all_reduce(tmax, op=dist.ReduceOp.MAX); tsum = t.clone(); dist.all_reduce(tsum, op=dist.ReduceOp.SUM)
        dt, its = float(tmax[0]), float(tsum[1])
    if rank == 0:
        P, F = 15 * 51, win.n_features
        nfac = len(win.obs_point) - win.n_features
        # fp64 MFMA roofline of the DOMINANT launch group of the dense reduce (the group with the most time): Schur SYRK F P (P + 1) flop per linear solve (the lower
        # triangle only: earlier rounds priced it as a full GEMM, 2 F P^2, twice the work the kernel is asked to do), Cholesky (+ the triangular solves) P^3 / 3 + 2 P^2
        flops = {"lw_schur_syrk": schur_flops(win)[1], "lw_cholesky": P ** 3 / 3.0 + 2.0 * P * P}        # the Schur reduce on the flops it issues (span-aware tiles); SURVEY 8(d)'s 2 sum (6 k_f)^2 beside it below
        names = {"lw_schur_syrk": "lw_syrk_mfma: Schur reduce Wn^T Wn over the pose columns, span-aware (hand-written fp64 MFMA 16x16x4 SYRK)",
                 "lw_cholesky": "lw_chol_panel + lw_chol_update + lw_chol_back: blocked Cholesky of the 765 x 765 reduced system, rhs as row P (hand-written fp64 MFMA, 2 launches per 64-column block)"}
        dom = max(flops, key=lambda k: prof[k]["ms"])
        rl = {}
        for k in flops:
            a = flops[k] * prof[k]["launches"] / max(prof[k]["ms"] * 1e-3, 1e-12) / 1e12 if prof[k]["launches"] else 0.0
            rl[k] = {"achieved": a, "frac": a / 78.6, "flop_per_launch": flops[k], "avg_launch_ms": prof[k]["ms"] / max(prof[k]["launches"], 1)}
        rl["lw_schur_syrk"]["algorithmic_flop_per_launch"] = schur_flops(win)[0]
        rl["lw_schur_syrk"]["frac_algorithmic"] = rl["lw_schur_syrk"]["frac"] * schur_flops(win)[0] / max(flops["lw_schur_syrk"], 1.0)
        out = {"metric": "sliding-window solve iters/sec (10 KF, ~5.5k factors) @1/2/4/8 GPU vs CPU", "value": its / dt, "unit": "iterations/s", "n_gpus": world, "steps": args.steps,
               "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
               "config": {"workload": "configs[4]: synthetic stress window, 51 frames (reduced system 765 x 765), one independent window per GPU and step; host buffers in -> host buffers out (pack + upload inside the step)", "frames": 51, "features": int(F),
                          "visual_factors": int(nfac), "imu_factors": 50, "lidar_between_factors": 50, "max_iterations": int(opts.max_num_iterations), "parallelism": f"{world} x independent windows"},
               "roofline": {"bound": "mfma", "kernel": names[dom], "achieved": rl[dom]["achieved"], "peak": 78.6, "unit": "TFLOP/s", "frac": rl[dom]["frac"], "traffic": None,
                            "flop_per_launch": rl[dom]["flop_per_launch"], "avg_launch_ms": rl[dom]["avg_launch_ms"], "groups": rl,
                            "kernels_ms_per_solve": {k: v["ms"] / args.steps for k, v in prof.items()}},
               "cpu_baseline": None}
        if sweep:
            out["concurrent_windows"] = sweep
            out["single_window"] = {"value": out["value"], "ms_per_solve": out["ms_per_step"]}
            best = max(sweep, key=lambda r: r["value"])
            if best["value"] > out["value"]:          # the aggregate over independent windows on one GPU is the throughput figure; the single-window line stays beside it
                out["value"] = best["value"]; out["ms_per_step"] = best["ms_per_solve_of_all_windows"]
                out["config"]["parallelism"] = f"{world} GPU x {best['windows']} independent windows at once (" + ("vilf_window_solve_group: one chain of launches" if best["mode"] == "group" else "one handle / HIP stream / host thread each") + ")"
                # the roofline of the line describes the configuration `value` is quoted on: the GROUP's flops over the group's launches (round 4 divided ONE window's
                # flops by a 32-window launch and printed 0.0044 for what is 0.088); the single window's figures stay under roofline.single_window
                if "cholesky" in best and "schur_reduce" in best:
                    rf = out["roofline"]
                    rf["single_window"] = {"kernel": rf["kernel"], "achieved": rf["achieved"], "frac": rf["frac"], "avg_launch_ms": rf["avg_launch_ms"], "groups": rf.pop("groups")}
                    dm = best["kernels_ms_per_group_solve"]
                    use_chol = dm["lw_cholesky"] >= dm["lw_schur_syrk"]
                    a = best["cholesky"]["TFLOPs"] if use_chol else best["schur_reduce"]["TFLOPs_issued"]
                    rf.update({"kernel": names["lw_cholesky" if use_chol else "lw_schur_syrk"] + f" — group of {best['windows']} windows", "achieved": a, "frac": a / 78.6,
                               "flop_per_launch": ((P ** 3 / 3.0 + 2.0 * P * P) * best["windows"]) if use_chol else best["schur_reduce"]["issued_flop_per_launch"],
                               "avg_launch_ms": (best["cholesky"]["ms_per_factorisation_of_all_windows"] if use_chol else best["schur_reduce"]["ms_per_launch"]),
                               "windows_per_launch": best["windows"]})
        if not args.no_cpu_baseline and world == 1:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import oracle_lib
            tc = time.perf_counter(); ref = oracle_lib.window_solve(opts, win, None); tc = time.perf_counter() - tc
            out["cpu_baseline"] = {"value": ref.summary["num_iterations"] / tc, "unit": "iterations/s", "cores": 1, "kind": "port", "sample": "one stress window (%d iterations) through oracle/ (C++ -O3, one thread), %.2f s" % (ref.summary["num_iterations"], tc)}
        print(json.dumps(out))
    if world > 1:
        dist.barrier(); dist.destroy_process_group()
    return 0


def launch_ranks(n):
    """`python bench.py --gpus N` without a launcher around it (WORLD_SIZE unset): start N rank processes of this script — one per GPU, RANK / LOCAL_RANK /
    WORLD_SIZE / MASTER_* in their environment, exactly what `python -m torch.distributed.run --nproc-per-node N` would give them — wait for them and pass rank 0's
    JSON line through. The parent imports neither torch nor the library and never initialises the GPU (a process that has must not exec / fork GPU children on this
    pool); it only counts devices through the sysfs-free, HIP-free route below when it can. With fewer than N devices visible it refuses, unless
    VILF_BENCH_REHEARSAL=1 (every rank on cuda:0, gloo collectives: the code path, never a measurement)."""
    import socket
    import subprocess
    rehearse = os.environ.get("VILF_BENCH_REHEARSAL") == "1"
    if not rehearse:
        try:
            import torch                                  # device_count() reads the driver's device list without creating a context on this image
            ndev = torch.cuda.device_count()
        except Exception:                                 # noqa: BLE001
            ndev = None
        if ndev is not None and ndev < n:
            raise SystemExit(f"bench.py --gpus {n}: only {ndev} GPU(s) visible (VILF_BENCH_REHEARSAL=1 rehearses the {n}-rank path on one GPU)")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, text=(r == 0)))
    out0, _ = procs[0].communicate()
    rc = procs[0].returncode
    for p_ in procs[1:]:
        try:
            rc = max(rc, abs(p_.wait(timeout=120 if procs[0].returncode else None)))
        except subprocess.TimeoutExpired:                 # rank 0 failed: the others wait in a collective — end exactly the children started here
            p_.kill(); p_.wait(); rc = max(rc, 1)
    sys.stdout.write(out0); sys.stdout.flush()
    return rc


def dryrun_main(args):
    """VILF_BENCH_DRYRUN=1 (tests only, never a measurement, nothing of the product runs): the rank plumbing of `--gpus N` without a GPU — every rank joins a gloo
    group, contributes its rows [global unit index, ...] to the pose gather (vil_fusion_amd.dist.gather_poses, the function the rehearsal mode uses), the barrier /
    max-over-ranks timing runs as in the real line, and rank 0 prints ONE JSON line that says which ranks arrived."""
    import numpy as np
    import torch
    import torch.distributed as dist
    from vil_fusion_amd import dist as vdist
    rank = int(os.environ.get("RANK", "0")); world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    B = 4
    rows = torch.zeros((B, 8), dtype=torch.float64); rows[:, 0] = torch.arange(rank * B, (rank + 1) * B, dtype=torch.float64); rows[:, 7] = 1.0
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    tab = rows
    for _ in range(args.steps):
        tab = vdist.gather_poses(rows) if world > 1 else rows
    if world > 1:
        dist.barrier()
    t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    col = tab[:, 0].numpy()
    if rank == 0:
        print(json.dumps({"dryrun": True, "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": float(t[0]) / max(args.steps, 1) * 1e3,
                          "gather": {"through": "gloo (dry run: no GPU, no product code)", "rccl_ranks": None, "rows": int(len(col)),
                                     "ranks_in_table": int(len(set((col // B).astype(np.int64).tolist()))),
                                     "global_unit_order": bool(np.array_equal(col, np.arange(world * B, dtype=np.float64)))}}))
    if world > 1:
        dist.barrier(); dist.destroy_process_group()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--windows", type=int, default=4096, help="frames (window snapshot + LiDAR stream) resident per GPU")
    ap.add_argument("--distinct", type=int, default=64, help="distinct synthetic windows (tiled to --windows)")
    ap.add_argument("--distinct-lidar", type=int, default=64, help="distinct synthetic LiDAR scenes (tiled to --windows; generated on the host cores before the GPU is touched)")
    ap.add_argument("--converging-windows", type=int, default=32, help="distinct windows of the converging-batch line (half of them start at their own fixed point and stop by tolerance); 0 skips it")
    ap.add_argument("--no-lidar-stage", action="store_true", help="configs[1]-style run: back-end window solve only")
    ap.add_argument("--no-marginalize", action="store_true", help="leave lines 863-1046 of Estimator::optimization() (marginalization) out of the frame")
    ap.add_argument("--overlap", action="store_true", help="run the LiDAR stage on its own handle / HIP stream / host thread, concurrently with the "
                    "window solve (like the reference's separate nodes); ~7 %% more frames/s, but per-kernel timings then include contention")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-pcie", action="store_true", help="skip the PCIe-inclusive leg (profile runs: its 2048-window solves would mix into the per-kernel averages)")
    ap.add_argument("--ragged-windows", type=int, default=1024, help="distinct windows of the ragged-batch line (features U(120, 320), mixed prior / no prior, mixed marginalization flags), tiled to --windows; 0 skips it")
    ap.add_argument("--no-latency", dest="latency", action="store_false", help="skip the single-frame latency line")
    ap.add_argument("--td-windows", type=int, default=64, help="windows of the estimate_td batch line (general path as one group of launches vs the plain batch); 0 skips it")
    ap.add_argument("--stress-mode", default="group", choices=["group", "streams"], help="--stress: how the independent windows run side by side (one grouped chain of launches / one handle and stream each)")
    ap.add_argument("--stress-windows", default="1,8,32", help="--stress: numbers of independent stress windows solved side by side (one handle / stream / host thread each)")
    ap.add_argument("--no-stress-leg", dest="stress_leg", action="store_false", help="skip the compact configs[4] leg (one group of 8 stress windows, 3 solves) of the default run")
    ap.add_argument("--stress", action="store_true", help="BASELINE configs[4] instead of the headline workload: one synthetic 51-frame / ~46 k-factor window per step and GPU")
    ap.add_argument("--full", action="store_true", help="also run everything beside the headline (CPU baseline, overlapped stages, ragged / converging / PCIe-inclusive / "
                    "estimate_td batches, single-frame latency, the compact configs[4] leg; the --no-* options and the window counts above select among them). "
                    "Without it a run only sets up, warms up, times the steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write what the last one computed (solved windows, new priors, scan-to-map results, "
                    "gathered poses; a seeded sample where larger than 64 MB) as DIR/<name>.npy")
    args = ap.parse_args()
    if not args.full:                                  # a plain run: the headline alone
        args.no_cpu_baseline = args.no_pcie = True
        args.latency = args.stress_leg = False
        args.ragged_windows = args.converging_windows = args.td_windows = 0
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return launch_ranks(args.gpus)                # `python bench.py --gpus N`: this process only starts the N ranks and relays rank 0's line (it never touches the GPU)
    if os.environ.get("VILF_BENCH_DRYRUN") == "1":
        return dryrun_main(args)
    if args.stress:
        return stress_main(args)

    import numpy as np
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    raw_lidar = []
    if not args.no_lidar_stage:                    # the distinct synthetic scenes (ray casting in numpy, ~6 s each): on the host cores, in child processes forked BEFORE
        from vil_fusion_amd import synth as _synth  # anything initialises the GPU
        seeds = [7000 + 31 * rank + k for k in range(args.distinct_lidar)]
        nproc = max(1, min(len(seeds), host_cpus() // max(1, min(world, 8))))
        try:
            if len(seeds) <= 4:                    # few scenes (profile runs: a counter-collecting profiler has initialised the GPU before python starts — no fork then)
                raise RuntimeError("serial")
            import multiprocessing as mp
            with mp.get_context("fork").Pool(nproc) as pool:
                raw_lidar = pool.map(_synth.make_lidar_bench_case, seeds)
        except Exception:
            raw_lidar = [_synth.make_lidar_bench_case(sd) for sd in seeds]
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the solve path has no CPU fallback")
    # VILF_BENCH_REHEARSAL=1: every rank on cuda:0 with gloo collectives — rehearses the N > 1 code path on a one-GPU box (never a measurement)
    rehearse = os.environ.get("VILF_BENCH_REHEARSAL") == "1"
    if rehearse:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if rehearse:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))

    from vil_fusion_amd import synth
    from vil_fusion_amd import dist as vdist
    from vil_fusion_amd.estimator import BackendSolver, Scan2MapBatch
    stream = torch.cuda.current_stream().cuda_stream
    solver = BackendSolver(device=local_rank, stream=stream)
    opts = solver.options
    B = args.windows
    cfg = synth.SynthConfig(n_features=230)        # ~1.5 k visual factors + 10 IMU + 10 LiDAR between-factors + prior (n = 75)
    wins, priors = synth.make_batch(1000 + rank, B, opts, cfg, distinct=args.distinct)
    solver.batch_upload(wins, priors)              # inputs resident in HBM before the timed region
    lidar_cases, s2m = [], None
    if not args.no_lidar_stage:                    # one LiDAR stream per frame, resident in HBM
        raw = raw_lidar
        # --overlap: the LiDAR stage gets its own handle = its own HIP stream and host thread, like the reference's separate
        # feature-tracker node (feature_tracker_node.cpp:384,524); default: both stages back to back on one stream
        lidar_handle = BackendSolver(device=local_rank)            # its own handle = its own HIP stream, always; whether the two stages run back to back or concurrently is step()'s choice
        # warm-up frame on the distinct scenes only: raw local map + scan 1 -> the steady-state (voxelised, leaf-ordered) local map
        # and the two poses of the constant-velocity model; the measured frames then start from that state with scan 2
        D = len(raw)
        warm = Scan2MapBatch(lidar_handle, D, max(len(c[2][0][0]) for c in raw) + 64, max(len(c[2][0][1]) for c in raw) + 64,
                             max(len(c[0]) + len(c[2][0][0]) for c in raw) + 64, max(len(c[1]) + len(c[2][0][1]) for c in raw) + 64)
        for k, (me, ms, scans, pl) in enumerate(raw):
            warm.localMapInited(k, me, ms, None, pl)
            warm.set_scan(k, *scans[0])
        warm.step()
        wres = warm.results()
        ident = np.array([0, 0, 0, 1, 0, 0, 0.0])
        # (steady-state edge map, surf map, measured scan, pose after the warm-up frame)
        lidar_cases = [(warm.getMapCloud(k, 0), warm.getMapCloud(k, 1), raw[k][2][1], np.array(wres[k].pose_qt[:]), raw[k]) for k in range(D)]
        s2m = Scan2MapBatch(lidar_handle, B, max(len(c[2][0]) for c in lidar_cases) + 64, max(len(c[2][1]) for c in lidar_cases) + 64,
                            max(len(c[0]) + len(c[2][0]) for c in lidar_cases) + 64, max(len(c[1]) + len(c[2][1]) for c in lidar_cases) + 64)
        for i in range(min(B, D)):
            me, ms, (se, ss), pose1, _ = lidar_cases[i]
            s2m.localMapInited(i, me, ms, pose1, ident)    # globalOdom = pose after frame 1, globalOdom_last = pose 0
            s2m.set_scan(i, se, ss)
        for i in range(D, B):
            s2m.copy_stream(i % D, i)                      # replicas of the distinct streams, copied on the device
        s2m.snapshot()
    poses = torch.zeros((B, 8), dtype=torch.float64, device="cuda")
    stamps = rank * B + np.arange(B, dtype=np.float64)     # global unit index: the gathered table must come out as 0 .. world * B - 1 (checked after the timed region)
    # N > 1: the newest-frame poses go through the library's own collective (vilf_comm_create / vilf_gather_poses = ncclCommInitRank / ncclAllGather over RCCL — what a
    # C++ / ROS estimator process per GPU would call), enqueued on the solver's stream behind the kernel that writes the rows. torch.distributed only
    # hands rank 0's communicator id to the other ranks and provides the barrier / the max-over-ranks of the timing. The one-GPU rehearsal keeps gloo (two ranks may not
    # share a device in one RCCL communicator).
    gather = None
    gathered = None
    gather_note = None
    gather_state = {"table": None}
    if world > 1 and not rehearse:
        # every rank first checks, without any collective, that the library's own RCCL binding loads (vilf_comm_unique_id dlopens librccl); only when all do is the
        # communicator created (a collective: a rank that failed before it would leave the others waiting). Otherwise torch.distributed carries the gather and says so.
        ok = torch.ones(1, dtype=torch.int32, device="cuda")
        try:
            my_id = vdist.RcclPoseGather.unique_id()
        except Exception as e:                                            # noqa: BLE001 — reported in the JSON line
            ok.zero_(); gather_note = f"C-ABI RCCL binding unavailable on rank {rank}: {e}"
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        if int(ok.item()) == 1:
            idt = torch.zeros(128, dtype=torch.uint8, device="cuda")
            if rank == 0:
                idt.copy_(torch.frombuffer(bytearray(my_id), dtype=torch.uint8))
            dist.broadcast(idt, src=0)
            gather = vdist.RcclPoseGather(world, rank, device=local_rank, unique_id=bytes(idt.cpu().numpy().tobytes()))
            gathered = torch.zeros((world * B, 8), dtype=torch.float64, device="cuda")
        elif gather_note is None:
            gather_note = "C-ABI RCCL binding unavailable on another rank"
    torch.cuda.synchronize()          # `poses` / `gathered` were zero-filled on torch's stream; the library's streams are non-blocking and do not wait for it by themselves

    def gather_step():
        solver.newest_poses_to_device(stamps, poses.data_ptr())              # a kernel on the solver's stream, no host wait
        if gather is not None:
            gather.gather_handle(solver, poses.data_ptr(), B, gathered.data_ptr())   # ncclAllGather on the SOLVER's stream: behind the kernel that wrote the rows
        else:
            solver.synchronize()                                                  # torch.distributed works on torch's stream: wait for the rows first
            gather_state["table"] = vdist.gather_poses(poses.cpu() if rehearse else poses)

    import threading

    def lidar_stage():
        s2m.rewind()
        s2m.step(sync=True)

    def step(overlap=args.overlap):
        th = None
        if s2m is not None and overlap:
            th = threading.Thread(target=lidar_stage)   # ctypes releases the GIL: both stages enqueue and run concurrently
            th.start()
        elif s2m is not None:
            # the LiDAR stage, then the window solve: nothing overlaps on the device (the per-kernel times are clean), but the host does not wait in between —
            # the solver's stream takes a device-side dependency on the LiDAR stage's stream (vilf_wait_for) and the whole frame is enqueued at once
            s2m.rewind()
            s2m.step(sync=False)
            if lidar_handle is not solver:
                solver.wait_for(lidar_handle)
        solver.batch_rewind()                           # state AND priors back to the uploaded snapshot
        solver.batch_solve(sync=False)
        if not args.no_marginalize:
            solver.batch_marginalize(sync=False)        # estimator.cpp:863-1046: the new priors stay on the device
        if th is not None:
            th.join()
        solver.synchronize()                            # end of the frame: the one host wait (the LiDAR stage finished before the solve started)
        if s2m is not None and lidar_handle is not solver:
            lidar_handle.synchronize()                  # (already idle: reads its pending profile spans, so its event pool is reused)
        if world > 1:
            gather_step()                               # RCCL all_gather: 64 B per solved window (rank 0 feeds global_fusion)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    solver.set_profiling(True)
    if s2m is not None and lidar_handle is not solver:
        lidar_handle.set_profiling(True)
    barrier()
    t0 = time.perf_counter()
    its_local = 0
    # Back-to-back mode: frame k + 1's LiDAR stage is enqueued (behind a device-side dependency on frame k's marginalization) BEFORE the host reads frame k's
    # summaries, so the device does not idle while the host counts iterations. Exactly `steps` LiDAR stages and `steps` back-end stages run inside the timed region.
    pipelined = s2m is not None and not args.overlap and lidar_handle is not solver
    if pipelined:
        s2m.rewind(); s2m.step(sync=False)
    for k in range(args.steps):
        if pipelined:
            solver.wait_for(lidar_handle)
            solver.batch_rewind()
            solver.batch_solve(sync=False)
            if not args.no_marginalize:
                solver.batch_marginalize(sync=False)
            if k + 1 < args.steps:
                lidar_handle.wait_for(solver)
                s2m.rewind(); s2m.step(sync=False)
            if world > 1:
                gather_step()
        else:
            step()
        its_local += sum(s.num_iterations for s in solver.batch_summaries())     # waits for the solver's stream (frame k done)
    barrier()
    dt = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:               # before anything else runs on these handles: the state is the last timed step's
        solver.synchronize()
        tab = None
        if world > 1:
            tab = (gathered if gather is not None else gather_state["table"]).cpu().numpy()
        dump_outputs(args.dump_outputs, solver, s2m, B, not args.no_marginalize, tab)
    prof = solver.get_profile()
    if not args.no_marginalize:
        prof.update(solver.get_profile_marginalize())
    lid = None
    if s2m is not None:
        prof.update(lidar_handle.get_profile_scan2map())
        rs = s2m.results()
        nq = float(np.mean([r.n_edge_ds + r.n_surf_ds for r in rs]))
        lid = dict(queries=nq, factors=float(np.mean([r.n_edge_factors[1] + r.n_surf_factors[1] for r in rs])),
                   lm_iterations=float(np.mean([r.iterations[0] + r.iterations[1] for r in rs])),
                   map_points=float(np.mean([len(c[0]) + len(c[1]) for c in lidar_cases])), scan_points=float(np.mean([len(c[2][0]) + len(c[2][1]) for c in lidar_cases])),
                   map_edge_points=float(np.mean([len(c[0]) for c in lidar_cases])), map_surf_points=float(np.mean([len(c[1]) for c in lidar_cases])))
        # scan clouds beyond the in-LDS voxel grid's capacity (22 112 points, SV_MAXPTS24 in vilf_s2m.hip) take the global-sort path (b_voxel_keys + a radix sort of
        # (key, index) + heads + reduce) in EVERY step: that is what the s2m_radix_sort group of the timed region is
        lid["scan_surf_points_max"] = int(max(len(c[2][1]) for c in lidar_cases)); lid["scan_edge_points_max"] = int(max(len(c[2][0]) for c in lidar_cases))
        lid["oversized_scan_clouds"] = int(sum(1 for c in lidar_cases for k in (0, 1) if len(c[2][k]) > 22112)); lid["distinct_scenes"] = len(lidar_cases)
        lid.update(lidar_search_statistics(lidar_cases[:8], opts))
    # N > 1: what the gather delivered — the table of the last step must hold every rank's rows in global unit order; the rank count comes from the communicator itself
    gather_info = None
    if world > 1:
        solver.synchronize()
        tab = gathered if gather is not None else gather_state["table"]
        col = tab[:, 0].cpu().numpy()
        gather_info = {"through": "vilf_gather_poses_handle (ncclAllGather on the solver's stream)" if gather is not None else ("gloo (one-GPU rehearsal)" if rehearse else "torch.distributed: " + str(gather_note)),
                       "rccl_ranks": gather.ranks()[0] if gather is not None else None,
                       "ranks_in_table": int(len(set((col // B).astype(np.int64).tolist()))), "rows": int(len(col)),
                       "global_unit_order": bool(np.array_equal(col, np.arange(world * B, dtype=np.float64)))}
    t = torch.tensor([dt, float(its_local)], dtype=torch.float64, device="cpu" if rehearse else "cuda")
    if world > 1:
        tmax = t.clone(); dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        tsum = t.clone(); dist.all_reduce(tsum, op=dist.ReduceOp.SUM)
        dt_max, its_total = float(tmax[0]), float(tsum[1])
    else:
        dt_max, its_total = dt, float(its_local)

    # ---- the two stages concurrently: the LiDAR stage on its own HIP stream and host thread next to the window solve — how the reference runs them (separate nodes,
    # feature_tracker_node.cpp:384,524) and how a deployment would. Reported beside the headline, never as `value`: `value` and the roofline come from the back-to-back
    # region above, whose per-kernel times are not inflated by the other stage's kernels.
    overlapped = None
    if s2m is not None and world == 1 and not args.overlap and not args.no_pcie:
        solver.set_profiling(False); lidar_handle.set_profiling(False)
        step(True)
        torch.cuda.synchronize()
        t1 = time.perf_counter(); oits = 0
        for _ in range(args.steps):
            step(True)
            oits += sum(s_.num_iterations for s_ in solver.batch_summaries())
        torch.cuda.synchronize()
        t1 = time.perf_counter() - t1
        overlapped = {"value": oits / t1, "unit": "iterations/s", "ms_per_step": t1 / args.steps * 1e3,
                      "what": "same frames, the LiDAR stage on its own HIP stream / host thread concurrently with the window solve + marginalization"}

    # ---- ragged-batch line: the headline replicates 64 windows of one shape; here every window differs (feature count, prior, marginalization flag).
    # Solve + marginalization only (the LiDAR streams are the same), after the timed region, reported beside the headline — never as `value`.
    ragged = None
    if args.ragged_windows > 0 and world == 1:
        rng = np.random.default_rng(4242)
        nr = min(args.ragged_windows, B)
        rw, rp = [], []
        for i in range(nr):
            c = synth.SynthConfig(n_features=int(rng.integers(120, 321)), with_prior=bool(rng.random() < 0.8),
                                  marginalization_flag=(0 if rng.random() < 0.7 else 1))      # VILF_MARGIN_OLD / VILF_MARGIN_SECOND_NEW
            wnd, pr, _ = synth.make_window(500000 + i, opts, c)
            rw.append(wnd); rp.append(pr)
        rsolver = BackendSolver(device=local_rank)
        rsolver.batch_upload([rw[i % nr] for i in range(B)], [rp[i % nr] for i in range(B)])

        def rstep():
            rsolver.batch_rewind(); rsolver.batch_solve(sync=True)
            if not args.no_marginalize:
                rsolver.batch_marginalize(sync=True)
        rstep()
        torch.cuda.synchronize(); tr0 = time.perf_counter(); rits = 0
        for _ in range(3):
            rstep(); rits += sum(s_.num_iterations for s_ in rsolver.batch_summaries())
        torch.cuda.synchronize(); trd = time.perf_counter() - tr0
        # the same three steps of the regular (64 distinct) batch without the LiDAR stage, for a like-for-like ratio
        tq0 = time.perf_counter(); qits = 0
        for _ in range(3):
            solver.batch_rewind(); solver.batch_solve(sync=True)
            if not args.no_marginalize:
                solver.batch_marginalize(sync=True)
            qits += sum(s_.num_iterations for s_ in solver.batch_summaries())
        torch.cuda.synchronize(); tqd = time.perf_counter() - tq0
        ragged = {"value": rits / trd, "unit": "iterations/s", "what": "window solve" + ("" if args.no_marginalize else " + marginalization") + ", no LiDAR stage",
                  "distinct_windows": nr, "features": "U(120, 320)", "prior_fraction": 0.8, "margin_old_fraction": 0.7, "mean_iterations": rits / (3.0 * B),
                  "ms_per_step": trd / 3 * 1e3, "regular_batch_same_stages": {"value": qits / tqd, "ms_per_step": tqd / 3 * 1e3}}
        rsolver.close()

    # ---- converging-batch line: with Ceres' default tolerances none of the synthetic windows stops before the iteration budget (the cost still falls by ~3e-4 per iteration
    # after eight of them; function_tolerance is 1e-6). Here half of the distinct windows START at their own fixed point (pre-solved on the device with a budget of 1000
    # iterations: FUNCTION_TOLERANCE after ~120) and stop in their first iteration, the other half are the regular windows. A finished window's workgroup leaves every
    # later launch at once (VbState::done), so the step costs what the unfinished windows cost; the launches themselves are still enqueued (no host round trip inside a solve).
    converging = None
    if args.converging_windows > 1 and world == 1:
        import copy
        nc = min(args.converging_windows, args.distinct, B); half = nc // 2
        o2 = type(opts).from_buffer_copy(opts); o2.max_num_iterations = 1000
        pre = BackendSolver(o2, device=local_rank)
        pre.batch_upload(wins[:half], priors[:half]); pre.batch_solve(sync=True)
        pres = pre.batch_download(); psum = pre.batch_summaries(); pre.close()
        cw = []
        for i in range(nc):
            if i < half:
                w2 = copy.deepcopy(wins[i]); r_ = pres[i]
                w2.para_pose = np.ascontiguousarray(np.asarray(r_.para_pose).reshape(-1, 7)); w2.para_speed_bias = np.ascontiguousarray(np.asarray(r_.para_speed_bias).reshape(-1, 9))
                w2.para_feature = np.ascontiguousarray(r_.para_feature)
                cw.append(w2)
            else:
                cw.append(wins[i])
        order = [int(k) for k in np.random.default_rng(77).integers(0, nc, B)]      # which window sits in which slot is random, as in a real batch: a periodic arrangement of
                                                                                    # short and long workgroups can fall on the same CUs launch after launch (tools/dev_converge.py)
        csolver = BackendSolver(device=local_rank)
        csolver.batch_upload([cw[k] for k in order], [priors[k] for k in order])

        def cstep():
            csolver.batch_rewind(); csolver.batch_solve(sync=True)
            if not args.no_marginalize:
                csolver.batch_marginalize(sync=True)
        cstep()
        torch.cuda.synchronize(); tc0 = time.perf_counter(); cits = 0; cterm = 0
        for _ in range(3):
            cstep(); sm = csolver.batch_summaries(); cits += sum(s_.num_iterations for s_ in sm); cterm += sum(1 for s_ in sm if s_.termination != 0)
        torch.cuda.synchronize(); tcd = time.perf_counter() - tc0
        tq0 = time.perf_counter(); qits = 0
        for _ in range(3):
            solver.batch_rewind(); solver.batch_solve(sync=True)
            if not args.no_marginalize:
                solver.batch_marginalize(sync=True)
            qits += sum(s_.num_iterations for s_ in solver.batch_summaries())
        torch.cuda.synchronize(); tqd = time.perf_counter() - tq0
        converging = {"value": cits / tcd, "unit": "iterations/s", "windows_per_s": 3.0 * B / tcd, "ms_per_step": tcd / 3 * 1e3, "mean_iterations": cits / (3.0 * B),
                      "stopped_by_tolerance_fraction": cterm / (3.0 * B), "distinct_windows": nc,
                      "presolve_iterations": [int(s_.num_iterations) for s_ in psum][:8],
                      "what": "window solve" + ("" if args.no_marginalize else " + marginalization") + ", no LiDAR stage; half of the windows start at their fixed point (FUNCTION_TOLERANCE in iteration 1), half are the regular 8-iteration windows",
                      "regular_batch_same_stages": {"value": qits / tqd, "windows_per_s": 3.0 * B / tqd, "ms_per_step": tqd / 3 * 1e3, "mean_iterations": qits / (3.0 * B)}}
        csolver.close()

    # ---- PCIe-inclusive figure: host buffers in (vilf_batch_upload: pack on the host threads + H2D from pinned staging) -> solve -> host buffers out
    # (vilf_batch_download_states), 2048 windows through ONE handle, priors resident (they are produced on the device in the running system). Never `value`.
    pcie = None
    if world == 1 and not args.no_pcie:
        from vil_fusion_amd import abi as vabi
        nb = min(2048, B)
        psolver = BackendSolver(device=local_rank)
        psolver.batch_upload(wins[:nb], priors[:nb])
        parr = (vabi.WindowIn * nb)()
        for i in range(nb):
            parr[i] = wins[i].as_struct()
        pout = psolver.batch_download_states()
        best = None
        for _ in range(4):
            tp0 = time.perf_counter()
            psolver._check(psolver._L.vilf_batch_upload(psolver._h, nb, parr), "vilf_batch_upload")
            tp1 = time.perf_counter(); psolver.batch_solve(sync=True); tp2 = time.perf_counter()
            psolver.batch_download_states(out=pout); tp3 = time.perf_counter()
            pits = sum(x.num_iterations for x in pout["summaries"])
            cur = {"value": pits / (tp3 - tp0), "unit": "iterations/s", "windows": nb, "upload_ms": 1e3 * (tp1 - tp0), "solve_ms": 1e3 * (tp2 - tp1), "download_ms": 1e3 * (tp3 - tp2),
                   "what": "window solve only, one handle: vilf_batch_upload (pack + H2D) + vilf_batch_solve + vilf_batch_download_states"}
            if best is None or cur["value"] > best["value"]:
                best = cur
        pcie = best
        # the same host-buffers-in / host-buffers-out path as a STREAM of batches over TWO handles (each its own HIP stream, staging and device buffers — the reference's
        # several estimator processes are several handles): while one handle's solve runs on the device (vilf_batch_solve with sync = 0), the host packs and uploads the
        # other handle's next batch. No library change: this is how the ABI is meant to be driven when batches keep arriving.
        try:
            half = nb // 2
            parr2 = []
            for k in range(2):
                arr_k = (vabi.WindowIn * half)()
                for i in range(half):
                    arr_k[i] = wins[k * half + i].as_struct()
                parr2.append(arr_k)

            def stream_of_batches(hl, rounds):
                """rounds x len(hl) batches; the clock covers the uploads + solves + downloads of rounds 1 .. rounds - 1 (round 0 warms up; its downloads fall inside, uncounted)"""
                pouts = [hl[k].batch_download_states(first=0, n=half) for k in range(len(hl))]
                inflight = [False] * len(hl)
                t_a = None
                for r in range(rounds):
                    if r == 1:
                        torch.cuda.synchronize(); t_a = time.perf_counter()
                    for k in range(len(hl)):
                        if inflight[k]:
                            hl[k].batch_download_states(first=0, n=half, out=pouts[k])
                        hl[k]._check(hl[k]._L.vilf_batch_upload(hl[k]._h, half, parr2[k % 2]), "vilf_batch_upload")
                        hl[k].batch_solve(sync=False); inflight[k] = True
                for k in range(len(hl)):
                    hl[k].batch_download_states(first=0, n=half, out=pouts[k])
                t_b = time.perf_counter()
                return (t_b - t_a) / (len(hl) * (rounds - 1)), sum(sum(x.num_iterations for x in po["summaries"]) for po in pouts) / len(hl)
            psolver._check(psolver._L.vilf_batch_upload(psolver._h, half, parr2[0]), "vilf_batch_upload"); psolver._n = half
            psolver.set_async_upload(True)                                       # vilf_set_async_upload: the upload returns once its copies are enqueued
            # the runtime multiplexes its streams onto a few hardware queues, and two streams on one queue run one after the other (this process holds several
            # more handles by now): handles are added one at a time and kept only if the stream gets faster with them — up to three, from up to five candidates
            chosen, cands, best_per = [psolver], [], 1e-3 * (pcie["upload_ms"] + pcie["solve_ms"] + pcie["download_ms"]) / 2
            tried_per = []                                                       # every configuration tried, kept or not (ms per batch): the figure below is a selection
            for _ in range(5):
                hc = BackendSolver(device=local_rank)
                hc.batch_upload(wins[half:nb] if len(chosen) % 2 else wins[:half], priors[half:nb] if len(chosen) % 2 else priors[:half])
                hc.set_async_upload(True)
                cands.append(hc)
                per, _its = stream_of_batches(chosen + [hc], 3)
                tried_per.append({"handles": len(chosen) + 1, "ms_per_batch": 1e3 * per, "kept": bool(per < 0.97 * best_per)})
                if per < 0.97 * best_per:
                    chosen.append(hc); best_per = per
                if len(chosen) == 3:
                    break
            if len(chosen) >= 2:
                per, its_batch = stream_of_batches(chosen, 7)
                pcie["stream_of_batches"] = {"value": its_batch / per, "unit": "iterations/s", "windows_per_batch": half, "handles": len(chosen), "batches": 6 * len(chosen), "ms_per_batch": 1e3 * per,
                                       "selection": {"rule": "handles added one at a time, one kept only if the stream gets >= 3 % faster with it (two streams on one hardware queue run one after the other)", "tried": tried_per},
                                       "what": "the same path as a stream of 1024-window batches alternating over two or three handles with vilf_set_async_upload: the host packs one handle's batch while the others' copies and solves (sync = 0) are on the device; download of a handle's results before its next upload"}
            else:
                pcie["stream_of_batches"] = {"error": "no second handle whose stream ran beside the first"}
            for hc in cands:
                hc.close()
        except Exception as e_:              # a side figure: never takes the bench line down
            pcie["stream_of_batches"] = {"error": repr(e_)}
        psolver.close()

    # ---- single-frame latency: the reference's only mode is ONE window per frame (estimator_node.cpp:243-396) — through the single-window / single-stream entry
    # points, host buffers in, host buffers out, median of 20 (one workgroup per kernel: a chain of dependent fp64 operations at 36 cycles each)
    latency = None
    if world == 1 and args.latency:
        from vil_fusion_amd.estimator import Scan2Map
        ls = BackendSolver(device=local_rank)
        lw_, lp_ = wins[0], priors[0]

        def med(fn, n=20):
            ts = []
            for _ in range(n):
                t_ = time.perf_counter(); fn(); ts.append(time.perf_counter() - t_)
            return 1e3 * float(np.median(ts))

        def f_solve():
            ls.set_prior(lp_); return ls.optimization(lw_)

        def f_solve_marg():
            ls.set_prior(lp_); ls.optimization(lw_); ls.marginalize()
        f_solve()

        def f_solve_resident():                     # the running system: the prior is on the device (written by the last marginalization), nothing to import
            return ls.optimization(lw_)
        latency = {"window_solve_ms": med(f_solve), "window_solve_device_usec": f_solve().summary["usec_solve"], "window_solve_resident_prior_ms": med(f_solve_resident),
                   "window_solve_marginalize_ms": med(f_solve_marg),
                   "what": "vilf_window_solve (upload + <= 8 dogleg iterations + download) of ONE 11-frame window — with the prior imported by the call (vilf_prior_import: repeatable) and with the prior already resident on the device (the running system) — and + vilf_window_marginalize; vilf_scan2map_step of ONE LiDAR stream (steady-state local map)"}
        if raw_lidar:
            me_, ms_, scans_, pl_ = raw_lidar[0]
            m1 = Scan2Map(ls); m1.localMapInited(me_, ms_)
            m1.optimation_processing(*scans_[0])
            t_ = time.perf_counter(); m1.optimation_processing(*scans_[1]); latency["scan_to_map_frame_ms"] = 1e3 * (time.perf_counter() - t_)
            # One frame the way the reference runs it — the LiDAR node and the estimator node are separate processes (feature_tracker_node.cpp:384,524 /
            # estimator_node.cpp:243-396): the scan-to-map step of ONE stream on its own handle (= its own HIP stream) and host thread beside the window solve +
            # marginalization of ONE window; the stream is rewound to the same steady-state map before every frame.
            import threading

            def f_est():
                ls.optimization(lw_); ls.marginalize()
            f_est()
            # (The runtime maps a process's streams onto a few hardware queues, and two streams that land on one queue run one after the other: with the handles this
            #  run has open that is the case for every other new stream. Two LiDAR handles are tried and the better one reported — a deployment has two streams, or two
            #  processes, and no such collision.)
            best = None
            tried_ = []
            tried_ms = []
            for _try in range(2):
                lh = BackendSolver(device=local_rank)
                sb1 = Scan2MapBatch(lh, 1, len(scans_[0][0]) + len(scans_[1][0]) + 64, len(scans_[0][1]) + len(scans_[1][1]) + 64, len(me_) + len(scans_[0][0]) + 64, len(ms_) + len(scans_[0][1]) + 64)
                sb1.localMapInited(0, me_, ms_, None, pl_)
                sb1.set_scan(0, *scans_[0]); sb1.step()
                sb1.set_scan(0, *scans_[1]); sb1.snapshot()

                def f_s2m():
                    sb1.rewind(); sb1.step(sync=True)
                f_s2m()
                alone = med(f_s2m)
                # both loops side by side, 40 frames each (a thread started per frame would measure Python's thread start-up, not the device): wall time per frame
                nfr = 40
                ths = [threading.Thread(target=lambda f=f: [f() for _ in range(nfr)]) for f in (f_est, f_s2m)]
                t_ = time.perf_counter(); [x.start() for x in ths]; [x.join() for x in ths]
                both = 1e3 * (time.perf_counter() - t_) / nfr
                if best is None or both < best[0]:
                    best = (both, alone)
                tried_ms.append({"frame_overlapped_ms": both, "scan_to_map_alone_ms": alone})
                tried_.append(lh)                                 # the first handle stays open while the second is tried (its stream keeps its queue)
            for lh in tried_:
                lh.close()
            latency["scan_to_map_frame_median_ms"] = best[1]
            latency["frame_overlapped_ms"] = best[0]
            latency["frame_overlapped_selection"] = {"rule": "the better of two LiDAR handles (the other one's stream shares a hardware queue with the estimator's)", "tried": tried_ms}
            latency["what"] += "; frame_overlapped_ms: 40 frames of window solve (resident prior) + marginalization on one handle / host thread while 40 scan-to-map steps of one stream run on another handle / thread — the reference's separate nodes; wall time per frame"
        ls.close()

    # ---- estimate_td batch (ProjectionTdFactor, td a variable: estimator.cpp:713-717,772-777; off in the KITTI configuration): such batches go through the general path,
    # all slots as ONE group of launches (vilf_lw.hip), not through the LDS kernels. 64 windows, solve only, against the plain batch of the same windows.
    td_batch = None
    if world == 1 and args.td_windows > 0:
        nb = args.td_windows
        tdw = [synth.with_td_inputs(wins[i % args.distinct], 10 + i) for i in range(min(nb, 16))]
        tdw = [tdw[i % len(tdw)] for i in range(nb)]
        tdp = [priors[i % min(nb, 16) % args.distinct] for i in range(nb)]
        tms = {}
        for flag in (0, 1):
            from vil_fusion_amd.lib import default_options as _defopts
            o2 = _defopts(); o2.estimate_td = flag
            ts = BackendSolver(o2, device=local_rank)
            ts.batch_upload(tdw, tdp)
            for _ in range(2):
                ts.batch_rewind(); ts.batch_solve()
            torch.cuda.synchronize(); tq0 = time.perf_counter()
            for _ in range(5):
                ts.batch_rewind(); ts.batch_solve()
            torch.cuda.synchronize(); tms[flag] = (time.perf_counter() - tq0) / 5 * 1e3
            tms[(flag, "it")] = sum(x.num_iterations for x in ts.batch_summaries())
            ts.close()
        td_batch = {"windows": nb, "plain_batch_ms": tms[0], "estimate_td_batch_ms": tms[1], "ratio": tms[1] / tms[0], "iterations": [tms[(0, "it")], tms[(1, "it")]],
                    "what": "vilf_batch_solve of the same 64 windows (with priors): estimate_td = 0 (LDS kernels) vs estimate_td = 1 (general path, one group of launches; the slots ran one by one until round 3: ~80 ms)"}

    # ---- configs[4] in brief (the full sweep: --stress)
    stress = None
    if world == 1 and args.stress_leg:
        stress = stress_leg(local_rank)

    if rank == 0:
        abytes = float(np.mean([algorithmic_bytes_per_iteration(w, p) for w, p in zip(wins[:args.distinct], priors[:args.distinct])]))
        # algorithmic bytes per STEP (all B frames) per kernel / launch group; for the window kernels
        # every launch is one solver iteration of all B windows, so bytes-per-step / ms-per-step == bytes-per-launch / ms-per-launch
        lps = {k: v["launches"] / args.steps for k, v in prof.items()}
        part = lambda what: float(np.mean([algorithmic_bytes_per_iteration(w, p, what) for w, p in zip(wins[:args.distinct], priors[:args.distinct])]))
        alg = {"k_linearize": abytes * B * lps["k_linearize"], "k_solve": part("reduced") * B * lps["k_solve"], "k_step": part("inputs") * B * lps["k_step"]}
        if not args.no_marginalize:           # per frame: re-evaluate the dropped factors once, n_p^2 prior in, n x n prior out
            mbytes = part("inputs") + 8.0 * 75 * 76
            alg.update({"k_marg_prepare": part("inputs") * B, "k_marg_schur": 8.0 * (96 * 97 + 117 * 118) * B, "k_marg_finish": 8.0 * 75 * 76 * 2 * B, "k_prior_prep": 8.0 * 75 * 76 * 2 * B})
        if lid is not None:
            nm, ns, nq = lid["map_points"], lid["scan_points"], lid["queries"]
            alg.update({
                # 2 passes over all queries: the query point in (16 B), its factor record out (64 B), per row of cells two directory slots (8 B), and the candidates the
                # rows' spans hold (16 B each; counted on the host from the maps: lid["candidates_per_query"]) — the bytes this design moves, not SURVEY's 27-cell estimate
                "s2m_associate": B * 2 * nq * (16 + 64 + lid["rows_per_query"] * 8 + lid["candidates_per_query"] * 16),
                "s2m_neighbour_index": B * (nm * 4 + lid["map_cells"] * 4),  # directory: one 4-byte slot id in per map point, one 4-byte slot out per occupied cell
                "s2m_radix_sort": B * ns * 12 * 2,                       # only when a scan cloud exceeds the in-LDS grid (22 k points): ONE pass over (key, index)
                "s2m_voxel_grid": B * (ns + nq) * 16,                    # the two scan grids: raw scan points in, centroids out
                "s2m_map_update": B * (nm * 32 + nq * 16),               # the two map updates: old map + registered scan in, new map out (+ 4 B per occupied cell: the directory)
                "s2m_lm_solve": B * nq * 64.0 * 2 * 5,                   # factor records (one 64-byte sector each), 2 passes x 5 evaluations
                "s2m_submap": B * nq * 16 * 2})                         # transform + append of the registered scan (crop and grid are in s2m_voxel_grid)
        survey_knn = None
        if lid is not None:
            # SURVEY 8(d)'s own price of the association, beside the design's: N_q (12 + 27 c 16) per pass with c = 2 points per 1 m cell, 2 passes, + the map hash
            # build N_map 16 2 (this design builds no hash: the map is its own index) — printed so that the s2m_associate fraction can be read against either
            sb = B * (2 * nq * (12 + 27 * 2.0 * 16) + nm * 16 * 2)
            t_as = prof["s2m_associate"]["ms"] / args.steps * 1e-3
            survey_knn = {"formula": "2 passes x N_q (12 + 27 x 2 x 16) + N_map x 16 x 2 (SURVEY.md 8(d))", "bytes_per_step": sb,
                          "achieved_GBps_on_survey_bytes": sb / max(t_as, 1e-12) / 1e9, "frac_of_hbm_peak_on_survey_bytes": sb / max(t_as, 1e-12) / 1e9 / 8000.0,
                          "design_bytes_per_step": alg["s2m_associate"], "note": "the design's bytes (rows of cells actually walked, candidates actually read, counted on the host from the maps) are what the kernels_achieved_GBps entry is priced on"}
        workload_tag = ("lidar+" if lid is not None else "") + "solve" + ("" if args.no_marginalize else "+marginalize")
        dom = max(alg, key=lambda k: prof[k]["ms"])
        avg_ms = prof[dom]["ms"] / max(prof[dom]["launches"], 1)
        achieved = alg[dom] / max(lps[dom], 1e-9) / (avg_ms * 1e-3) / 1e9
        # HBM traffic per launch of the dominant kernel from the committed PMC passes (separate rocprofv3 --pmc runs of this
        # same command; gfx950-corrected as MI355X_MICROARCH.md prescribes) — only when they were taken on this configuration
        traffic = None
        traffic_raw = None
        try:
            import glob
            pmc = json.load(open(sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic.json")), key=_profile_order)[-1]))
            if pmc.get("config", {}).get("frames_per_gpu") == B and pmc["config"].get("workload_tag") == workload_tag:
                traffic = pmc["groups"][dom]["hbm_bytes_per_launch_corrected"]
                traffic_raw = pmc["groups"][dom].get("hbm_bytes_per_launch_raw")
        except Exception:
            traffic = None
        # the dense reduce (k_solve_sb) against the fp64 MFMA roofline, counted analytically per window-iteration (no PMC file: a counter pass of an older kernel
        # version must not be combined with current timings). "algorithmic" = SURVEY §8(d): P^3/3 + 2 P^2 + 2 sum_f (6 k_f)^2; "issued" = the v_mfma_f64_16x16x4_f64
        # instructions the kernel executes (2048 flop each: 80-wide padded feature reduce, Y recurrence + Y^T Y, rank-4 panel updates of the dense Cholesky).
        mfma = None
        try:
            F_mean = float(np.mean([w.n_features for w in wins[:args.distinct]]))
            nsteps = (int(F_mean) + 3) // 4
            issued = 15 * nsteps + 10 * (9 * 4 + 3 * 15) - 9 * 4 + sum(sum(1 for (ta, tb) in [(a_, b_) for a_ in range(5) for b_ in range(a_ + 1)] if 16 * tb + 15 >= 4 * bj + 4) for bj in range(19))
            kf = [np.diff(w.feature_obs_offset)[np.asarray(w.feature_const) == 0] for w in wins[:args.distinct]]
            alg_flop = float(np.mean([165.0 ** 3 / 3 + 2 * 165.0 ** 2 + 2 * float(np.sum((6.0 * k) ** 2)) for k in kf]))
            ms = prof["k_solve"]["ms"] / max(prof["k_solve"]["launches"], 1)
            mfma = {"k_solve": {"bound": "mfma", "peak": 78.6, "unit": "TFLOP/s", "avg_launch_ms": ms, "mfma_instructions_per_window": issued,
                                "issued_flop_per_launch": issued * 2048.0 * B, "achieved_issued": issued * 2048.0 * B / (ms * 1e-3) / 1e12, "frac_issued": issued * 2048.0 * B / (ms * 1e-3) / 1e12 / 78.6,
                                "algorithmic_flop_per_launch": alg_flop * B, "achieved": alg_flop * B / (ms * 1e-3) / 1e12, "frac": alg_flop * B / (ms * 1e-3) / 1e12 / 78.6,
                                "source": "analytic instruction count of the current kernel (see DESIGN.md)"}}
            # PMC cross-check (profiles/r*_pmc_mfma.json, a separate rocprofv3 --pmc pass of the solve-only bench): used only when it was taken at this batch size AND
            # its per-window MFMA count of k_solve_sb agrees with the count above (= the same kernel version); anything else is refused as stale and said so
            try:
                import glob
                cand = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_mfma.json")), key=_profile_order)
                pm = json.load(open(cand[-1]))
                ke = pm["kernels"].get("k_solve_sb")
                if ke is None or pm.get("config", {}).get("frames_per_gpu") != B:
                    mfma["k_solve"]["pmc"] = "refused: " + os.path.basename(cand[-1]) + " was taken on another kernel / batch size"
                elif abs(ke["mfma_instructions_per_window"] - issued) > 0.03 * issued:
                    mfma["k_solve"]["pmc"] = "refused: " + os.path.basename(cand[-1]) + f" counts {ke['mfma_instructions_per_window']:.0f} MFMA instructions per window, the current kernel issues {issued}"
                else:
                    mfma["k_solve"]["pmc"] = {"file": os.path.basename(cand[-1]), "mfma_instructions_per_window": ke["mfma_instructions_per_window"], "MfmaUtil_percent": ke.get("MfmaUtil_percent")}
            except Exception:
                mfma["k_solve"]["pmc"] = None
        except Exception:
            mfma = None
        # launch groups whose bytes are not HBM traffic of the timed launches (pricing them gave "bandwidths" above the 8 TB/s peak): the radix-sort group only runs for
        # oversized scans (none in this workload: the launches counted are set-up), k_prior_prep skips every window whose prior is unchanged, and the LM solve re-reads
        # its factor records from L2 (PMC: 3.96 GB per launch at the HBM interface against 5 x the record bytes priced)
        n_over = lid["oversized_scan_clouds"] if lid is not None else 0
        not_priced = {"s2m_radix_sort": (f"inside the timed region: {n_over} of {2 * lid['distinct_scenes']} scan clouds of the distinct scenes exceed the in-LDS voxel grid (22 112 points) and take "
                                         "the global-sort path every step (b_voxel_keys, the vendor radix sort, heads + reduce); priced per launch it is a set-up-sized group, not a stream of the map's bytes"
                                         if n_over else "no launch in the timed region (no scan cloud exceeds the in-LDS voxel grid)"), "k_prior_prep": "skips windows whose prior is unchanged: no fixed byte count per launch",
                      "s2m_lm_solve": "factor records are re-read from L2 across the 5 evaluations: algorithmic bytes are not HBM bytes here"}
        window_kernels = None
        try:                                   # registers / spills / LDS of the two window kernels, from the code objects of the shipped library (tools/kernel_resources.py at build time)
            kr = json.load(open(os.path.join(ROOT, "vil_fusion_amd", "csrc", "kernel_resources.json")))
            import ctypes as _C
            _l3 = (_C.c_int * 3)()
            solver._L.vilf_debug_lds_bytes.argtypes = [_C.c_void_p, _C.POINTER(_C.c_int)]
            solver._L.vilf_debug_lds_bytes(solver._h, _l3)
            dyn = {"k_linearize": int(_l3[0]), "k_solve_sb": int(_l3[1]), "k_solve": None}          # the launch's dynamic LDS, from the library (k_linearize's LDS is all dynamic since round 5)
            window_kernels = {k: {"vgpr": kr[k]["vgpr"], "vgpr_spills": kr[k]["vgpr_spills"], "scratch_bytes_per_lane": kr[k]["scratch_bytes_per_lane"],
                                  "static_lds_bytes": kr[k]["static_lds_bytes"], "dynamic_lds_bytes": dyn.get(k), "waves_per_simd_by_registers": kr[k]["waves_per_simd_by_registers"]} for k in ("k_linearize", "k_solve_sb", "k_solve")}
        except Exception:
            window_kernels = None
        it_ms = sum(prof[k]["ms"] for k in ("k_linearize", "k_solve", "k_step")) / max(prof["k_solve"]["launches"], 1)
        whole_it = abytes * B / (it_ms * 1e-3) / 1e9
        out = {
            "metric": "sliding-window solve iters/sec (10 KF, ~5.5k factors) @1/2/4/8 GPU vs CPU",
            "value": its_total / dt_max, "unit": "iterations/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt_max / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": ("configs[2]: per frame one scan-to-map step (voxel-kNN, edge/plane factors, 2 x <=4 LM iterations, map update) + "
                                    "the 10-keyframe window solve (11 frames, visual+IMU+LiDAR between-factors+prior, <=8 dogleg iterations); "
                                    "batched independent frames") if lid is not None else
                                   "configs[1]-style: 10-keyframe window solve only (visual+IMU+LiDAR between-factors+prior), batched independent windows",
                       "frames_per_gpu": B, "workload_tag": workload_tag, "lidar_stage": lid,
                       "windows_per_gpu": B, "distinct_windows": args.distinct, "visual_factors_per_window": float(np.mean([w.n_factors for w in wins[:args.distinct]])),
                       "features_per_window": float(np.mean([w.n_features for w in wins[:args.distinct]])), "max_iterations": int(opts.max_num_iterations),
                       "parallelism": f"{world} x independent window shards (no data-path collective; " + ("one-GPU rehearsal: gloo all_gather of 64 B poses" if rehearse else "RCCL all_gather of 64 B poses" + (" through vilf_gather_poses" if gather is not None else (" through torch.distributed: " + gather_note if gather_note else ""))) + ")"},
            "roofline": {"bound": "hbm", "kernel": dom, "achieved": achieved, "peak": 8000.0, "unit": "GB/s", "frac": achieved / 8000.0,
                         "traffic": traffic, "traffic_raw": traffic_raw, "traffic_note": "PMC FETCH_SIZE doubled (gfx950: wide coalesced reads are under-counted 2x) + WRITE_SIZE; `traffic_raw` without the doubling — this kernel reads mostly 8-byte operands, the truth lies between",
                         "avg_launch_ms": avg_ms, "launches_per_step": lps[dom], "algorithmic_bytes_per_launch": alg[dom] / max(lps[dom], 1e-9),
                         "algorithmic_bytes_per_window_iteration": abytes,
                         "whole_iteration": {"ms": it_ms, "achieved": whole_it, "frac": whole_it / 8000.0, "what": "388 KB x windows over the launches of one iteration (k_solve_sb + k_linearize; k_step = the step-only launch that ends a solve, spread over the iterations)"},
                         "kernels_ms": {k: v["ms"] / max(v["launches"], 1) for k, v in prof.items()},
                         "kernels_ms_per_step": {k: v["ms"] / args.steps for k, v in prof.items()},
                         "kernels_achieved_GBps": {k: alg[k] / (prof[k]["ms"] / args.steps) / 1e6 for k in alg
                                                   if prof[k]["launches"] > 0 and prof[k]["ms"] > 0 and k not in not_priced},
                         "kernels_not_priced": not_priced, "s2m_associate_on_survey_8d_bytes": survey_knn,
                         "binding": "fp64 issue + dependent latency, not HBM: one iteration is ~9 MFLOP per 388 KB (23 flop/B against a machine balance of 9.8), every dependent fp64 "
                                    "operation costs 36 cycles and the kernels run two waves per SIMD (DESIGN.md 3c); `bound: hbm` is SURVEY 8(d)'s convention for this row",
                         "window_kernels": window_kernels},
        }
        if gather_info is not None:
            out["gather"] = gather_info
            out["rccl_ranks"] = gather_info["rccl_ranks"]
        if mfma is not None:
            out["roofline_mfma"] = mfma
        if overlapped is not None:
            out["stages_overlapped"] = overlapped
        if ragged is not None:
            out["ragged_batch"] = ragged
        if converging is not None:
            out["converging_batch"] = converging
        if pcie is not None:
            out["pcie_inclusive"] = pcie
        if td_batch is not None:
            out["estimate_td_batch"] = td_batch
        if latency is not None:
            out["single_frame_latency"] = latency
        if stress is not None:
            out["stress"] = stress
        out["cpu_baseline"] = None                      # (N > 1, --no-cpu-baseline: the key stays, empty)
        if not args.no_cpu_baseline and world == 1:     # the CPU port is timed on rank 0 at N = 1 only
            out["cpu_baseline"] = cpu_baseline(opts, wins[:args.distinct], priors[:args.distinct], lidar_cases, not args.no_marginalize)
        print(json.dumps(out))
    if gather is not None:
        gather.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if s2m is not None and lidar_handle is not solver:
        lidar_handle.close()
    solver.close()


if __name__ == "__main__":
    main()
