"""Host-side mirror of the reference's operator surface for the hot path.

`BackendSolver.optimization(window)` ≙ Estimator::optimization() (vins_estimator/estimator.cpp:689-1050): solve on the
MI355X through the C ABI, gauge fix, then (optionally) marginalization; the prior lives on the device between calls like
`last_marginalization_info` (estimator.h:123-124). `BackendSolver.batch_*` drive many independent window snapshots.
Errors: the C ABI returns status ints; this wrapper raises VilfError for status < 0 (invalid argument / device error /
unsupported) and returns the summary for status >= 0, mirroring the reference where solver failures are not checked
(estimator.cpp:852-855).
"""
import ctypes as C
import numpy as np
from . import abi
from .lib import lib, VilfError, default_options


class BackendSolver:
    def __init__(self, options=None, device=0, stream=None):
        self._L = lib()
        self.options = options if options is not None else default_options()
        h = C.c_void_p()
        rc = self._L.vilf_create(C.byref(self.options), int(device), C.c_void_p(stream) if stream else None, C.byref(h))
        if rc != 0:
            raise VilfError(f"vilf_create failed with status {rc}" + (" (no GPU visible: the solve path has no CPU fallback)" if rc == abi.VILF_ERR_NO_GPU else ""))
        self._h = h
        self._keep = None
        self._n = 0
        self._device = int(device)
        self._tri = None

    def close(self):
        if getattr(self, "_tri", None) is not None:
            self._tri.close()
            self._tri = None
        if getattr(self, "_h", None):
            self._L.vilf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc < 0:
            raise VilfError(f"{what}: status {rc}: {self._L.vilf_last_error(self._h).decode()}")
        return rc

    # ---- single window (drop-in for Estimator::optimization) -----------------------------------------------------
    def set_prior(self, prior, slot=0):
        """≙ last_marginalization_info / last_marginalization_parameter_blocks"""
        if prior is None:
            prior = abi.Prior()
        self._check(self._L.vilf_prior_import(self._h, slot, C.byref(prior)), "vilf_prior_import")

    def get_prior(self, slot=0):
        p = abi.Prior()
        self._check(self._L.vilf_prior_export(self._h, slot, C.byref(p)), "vilf_prior_export")
        return p

    def optimization(self, window):
        res = abi.WindowResult(window.n_frames, window.n_features)
        s = window.as_struct()
        self._check(self._L.vilf_window_solve(self._h, C.byref(s), C.byref(res.struct)), "vilf_window_solve")
        return res.finish()

    def prepare_group(self, windows):
        """the ctypes views of a group of windows (input structs + result buffers), built once: a caller that solves the same group repeatedly (bench) or keeps
        its windows in C structs anyway does not pay the per-call conversion"""
        n = len(windows)
        res = [abi.WindowResult(w.n_frames, w.n_features) for w in windows]
        ins = (abi.WindowIn * n)(); outs = (abi.WindowOut * n)()
        for i, w in enumerate(windows):
            ins[i] = w.as_struct(); outs[i] = res[i].struct
        return dict(n=n, ins=ins, outs=outs, res=res, windows=windows)

    def solve_group(self, group, finish=True):
        """vilf_window_solve_group on a prepared group; finish=False skips the numpy unpacking of the results (the summaries are in group["outs"][i].summary)"""
        self._check(self._L.vilf_window_solve_group(self._h, group["n"], group["ins"], group["outs"]), "vilf_window_solve_group")
        if not finish:
            return group["outs"]
        for i, r in enumerate(group["res"]):
            r.struct = group["outs"][i]          # the summaries were written into the array's copies (the buffers they point to are the results' own)
        return [r.finish() for r in group["res"]]

    def optimization_group(self, windows):
        """several windows of sizes other than 11 frames (the general path) side by side in one chain of launches ≙ one optimization() each"""
        return self.solve_group(self.prepare_group(windows))

    def marginalize(self):
        self._check(self._L.vilf_window_marginalize(self._h), "vilf_window_marginalize")

    def reset(self):
        """≙ Estimator::clearState() for the prior (estimator.cpp:72-77)"""
        self._check(self._L.vilf_reset(self._h), "vilf_reset")

    # ---- batch of independent window snapshots -------------------------------------------------------------------
    def batch_upload(self, windows, priors=None):
        n = len(windows)
        arr = (abi.WindowIn * n)()
        for i, w in enumerate(windows):
            arr[i] = w.as_struct()
        if priors is not None:
            for i, p in enumerate(priors):
                self.set_prior(p, i)
        self._keep = (windows, arr)
        self._check(self._L.vilf_batch_upload(self._h, n, arr), "vilf_batch_upload")
        self._n = n
        self._shapes = [(w.n_frames, w.n_features) for w in windows]

    def set_async_upload(self, on=True):
        """vilf_set_async_upload: batch_upload returns once its copies are enqueued (streams of batches over two handles)"""
        self._check(self._L.vilf_set_async_upload(self._h, 1 if on else 0), "vilf_set_async_upload")

    def batch_solve(self, sync=True):
        self._check(self._L.vilf_batch_solve(self._h, 1 if sync else 0), "vilf_batch_solve")

    def batch_rewind(self):
        self._check(self._L.vilf_batch_rewind(self._h), "vilf_batch_rewind")

    def synchronize(self):
        self._check(self._L.vilf_synchronize(self._h), "vilf_synchronize")

    def wait_for(self, other):
        """work enqueued on this handle from now on starts after everything enqueued on `other` so far has finished (device-side dependency, no host wait)"""
        self._check(self._L.vilf_wait_for(self._h, other._h), "vilf_wait_for")

    def set_profiling(self, on=True):
        self._check(self._L.vilf_set_profiling(self._h, 1 if on else 0), "vilf_set_profiling")

    def get_profile(self):
        ms = (C.c_double * 4)(); n = (C.c_long * 4)()
        self._check(self._L.vilf_get_profile(self._h, ms, n), "vilf_get_profile")
        names = ["k_linearize", "k_solve", "k_step", "other"]
        return {names[i]: dict(ms=ms[i], launches=n[i]) for i in range(4)}

    S2M_GROUPS = ("s2m_voxel_grid", "s2m_radix_sort", "s2m_neighbour_index", "s2m_associate", "s2m_lm_solve", "s2m_submap", "s2m_other", "s2m_map_update")

    def get_profile_scan2map(self):
        ms = (C.c_double * 8)(); n = (C.c_long * 8)()
        self._check(self._L.vilf_get_profile_scan2map(self._h, ms, n), "vilf_get_profile_scan2map")
        return {k: dict(ms=ms[i], launches=n[i]) for i, k in enumerate(self.S2M_GROUPS)}

    def get_profile_marginalize(self):
        ms = (C.c_double * 4)(); n = (C.c_long * 4)()
        self._check(self._L.vilf_get_profile_marginalize(self._h, ms, n), "vilf_get_profile_marginalize")
        return {k: dict(ms=ms[i], launches=n[i]) for i, k in enumerate(("k_marg_prepare", "k_marg_schur", "k_marg_finish", "k_prior_prep"))}

    def get_profile_large_window(self):
        ms = (C.c_double * 4)(); n = (C.c_long * 4)()
        self._check(self._L.vilf_get_profile_large_window(self._h, ms, n), "vilf_get_profile_large_window")
        return {k: dict(ms=ms[i], launches=n[i]) for i, k in enumerate(("lw_factor_scatter", "lw_schur_syrk", "lw_cholesky", "lw_other"))}

    def marginalize_stats(self):
        """paths of the last marginalization: windows with a new prior, of those Amm by Cholesky, of those the kept block by Cholesky, windows left unchanged"""
        c = (C.c_int * 4)()
        self._check(self._L.vilf_batch_marginalize_stats(self._h, c), "vilf_batch_marginalize_stats")
        return dict(new_prior=c[0], amm_cholesky=c[1], kept_cholesky=c[2], unchanged=c[3])

    def batch_marginalize(self, sync=True):
        self._check(self._L.vilf_batch_marginalize(self._h, 1 if sync else 0), "vilf_batch_marginalize")

    def batch_summaries(self, first=0, n=None):
        n = self._n - first if n is None else n
        arr = (abi.Summary * n)()
        self._check(self._L.vilf_batch_summaries(self._h, first, n, arr), "vilf_batch_summaries")
        return arr

    def batch_download(self, first=0, n=None):
        n = self._n - first if n is None else n
        results = [abi.WindowResult(*self._shapes[first + i]) for i in range(n)]
        arr = (abi.WindowOut * n)()
        for i, r in enumerate(results):
            arr[i] = r.struct
        self._check(self._L.vilf_batch_download(self._h, first, n, arr), "vilf_batch_download")
        for i, r in enumerate(results):
            r.struct = arr[i]
            r.finish()
        return results

    def batch_download_states(self, first=0, n=None, out=None):
        """Ps / Rs / Vs / Bas / Bgs + summaries of n windows into contiguous numpy arrays (re-used when `out` is given): the per-frame download"""
        n = self._n - first if n is None else n
        if out is None:
            out = dict(Ps=np.empty((n, 11, 3)), Rs=np.empty((n, 11, 3, 3)), Vs=np.empty((n, 11, 3)), Bas=np.empty((n, 11, 3)), Bgs=np.empty((n, 11, 3)), summaries=(abi.Summary * n)())
        self._L.vilf_batch_download_states.argtypes = [C.c_void_p, C.c_int, C.c_int, abi.c_double_p, abi.c_double_p, abi.c_double_p, abi.c_double_p, abi.c_double_p, C.POINTER(abi.Summary)]
        self._check(self._L.vilf_batch_download_states(self._h, first, n, abi.dptr(out["Ps"]), abi.dptr(out["Rs"]), abi.dptr(out["Vs"]), abi.dptr(out["Bas"]), abi.dptr(out["Bgs"]), out["summaries"]),
                    "vilf_batch_download_states")
        return out

    def newest_poses_to_device(self, stamps, device_ptr):
        st = np.ascontiguousarray(stamps, dtype=np.float64)
        self._check(self._L.vilf_batch_newest_poses_device(self._h, abi.dptr(st), C.c_void_p(device_ptr)), "vilf_batch_newest_poses_device")

    # ---- Ceres-layout hooks (same signatures as the reference's Evaluate) ----------------------------------------
    def _params(self, arrs):
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in arrs]
        return arrs, (abi.c_double_p * len(arrs))(*[abi.dptr(a) for a in arrs])

    def eval_projection(self, params, pts_i, pts_j, want_ex_jacobian=True):
        arrs, p = self._params(params)
        r = np.zeros(2)
        jacs = [np.zeros((2, 7)), np.zeros((2, 7)), np.zeros((2, 7)), np.zeros((2, 1))]
        ptrs = [abi.dptr(jacs[0]), abi.dptr(jacs[1]), abi.dptr(jacs[2]) if want_ex_jacobian else abi.c_double_p(), abi.dptr(jacs[3])]
        jp = (abi.c_double_p * 4)(*ptrs)
        self._check(self._L.vilf_eval_projection(self._h, p, abi.dptr(np.ascontiguousarray(pts_i, dtype=np.float64)),
                                                 abi.dptr(np.ascontiguousarray(pts_j, dtype=np.float64)), abi.dptr(r), jp), "vilf_eval_projection")
        return r, jacs

    def eval_imu(self, params, pre):
        arrs, p = self._params(params)
        r = np.zeros(15)
        jacs = [np.zeros((15, 7)), np.zeros((15, 9)), np.zeros((15, 7)), np.zeros((15, 9))]
        jp = (abi.c_double_p * 4)(*[abi.dptr(j) for j in jacs])
        self._check(self._L.vilf_eval_imu(self._h, p, C.byref(pre), abi.dptr(r), jp), "vilf_eval_imu")
        return r, jacs

    def eval_imu_raw(self, params, pre):
        """residual / jacobians before the multiplication by sqrt_info, and the device's sqrt_info [15, 15]"""
        arrs, p = self._params(params)
        r = np.zeros(15); S = np.zeros((15, 15))
        jacs = [np.zeros((15, 7)), np.zeros((15, 9)), np.zeros((15, 7)), np.zeros((15, 9))]
        jp = (abi.c_double_p * 4)(*[abi.dptr(j) for j in jacs])
        self._check(self._L.vilf_eval_imu_raw(self._h, p, C.byref(pre), abi.dptr(r), jp, abi.dptr(S)), "vilf_eval_imu_raw")
        return r, jacs, S

    def eval_lidar_between(self, params, c):
        arrs, p = self._params(params)
        r = np.zeros(6)
        jacs = [np.zeros((6, 7)), np.zeros((6, 7))]
        jp = (abi.c_double_p * 2)(*[abi.dptr(j) for j in jacs])
        self._check(self._L.vilf_eval_lidar_between(self._h, p, C.byref(c), abi.dptr(r), jp), "vilf_eval_lidar_between")
        return r, jacs

    def eval_projection_td(self, params, pts_i, pts_j, vel_i, vel_j, td_i, td_j, row_i, row_j):
        """ProjectionTdFactor::Evaluate on the device: params = [Pose_i, Pose_j, Ex_Pose, [inv depth], [td]]"""
        arrs, p = self._params(params)
        r = np.zeros(2)
        jacs = [np.zeros((2, 7)), np.zeros((2, 7)), np.zeros((2, 7)), np.zeros((2, 1)), np.zeros((2, 1))]
        jp = (abi.c_double_p * 5)(*[abi.dptr(j) for j in jacs])
        f = lambda v: abi.dptr(np.ascontiguousarray(v, dtype=np.float64))
        self._L.vilf_eval_projection_td.argtypes = [C.c_void_p, C.c_void_p, abi.c_double_p, abi.c_double_p, abi.c_double_p, abi.c_double_p,
                                                    C.c_double, C.c_double, C.c_double, C.c_double, abi.c_double_p, C.c_void_p]
        self._check(self._L.vilf_eval_projection_td(self._h, p, f(pts_i), f(pts_j), f(vel_i), f(vel_j), float(td_i), float(td_j), float(row_i), float(row_j),
                                                    abi.dptr(r), jp), "vilf_eval_projection_td")
        return r, jacs

    def eval_prior(self, prior, params):
        """MarginalizationFactor::Evaluate (marginalization_factor.cpp:333-381) on the device: residuals [n], jacobians [n x size_i]"""
        arrs, p = self._params(params)
        sizes = [prior.block_size[i] for i in range(prior.n_blocks)]
        r = np.zeros(prior.n)
        jacs = [np.zeros((prior.n, s)) for s in sizes]
        jp = (abi.c_double_p * len(sizes))(*[abi.dptr(j) for j in jacs])
        self._check(self._L.vilf_eval_prior(self._h, C.byref(prior), p, abi.dptr(r), jp), "vilf_eval_prior")
        return r, jacs

    def eval_edge(self, pose, cp, a, b):
        r = np.zeros(3); J = np.zeros((3, 7))
        f = lambda x: abi.dptr(np.ascontiguousarray(x, dtype=np.float64))
        self._check(self._L.vilf_eval_edge(self._h, f(pose), f(cp), f(a), f(b), abi.dptr(r), abi.dptr(J)), "vilf_eval_edge")
        return r, J

    def eval_surf(self, pose, cp, n, d):
        r = np.zeros(1); J = np.zeros((1, 7))
        f = lambda x: abi.dptr(np.ascontiguousarray(x, dtype=np.float64))
        self._check(self._L.vilf_eval_surf(self._h, f(pose), f(cp), f(n), float(d), abi.dptr(r), abi.dptr(J)), "vilf_eval_surf")
        return r, J

    def pose_plus(self, x, d, se3=False):
        out = np.zeros(7)
        f = lambda v: abi.dptr(np.ascontiguousarray(v, dtype=np.float64))
        fn = self._L.vilf_se3_plus if se3 else self._L.vilf_pose_plus
        self._check(fn(self._h, f(x), f(d), abi.dptr(out)), "vilf_pose_plus")
        return out

    # ---- feature manager ------------------------------------------------------------------------------------------
    def triangulate_features(self, tables):
        """≙ f_manager.triangulate + getDepthVector for every table at once (triangulate_features below), on a handle of its own with these options: its stream
        and its buffers are not those of the window solve. This is what SlidingWindowEstimator and run_sequences_lockstep take as `triangulate`."""
        if self._tri is None:
            self._tri = BackendSolver(self.options, self._device)
        return triangulate_features(self._tri, tables)

    def features_profile(self):
        """ms and kernel launches of triangulate_features since set_profiling_features"""
        return features_profile(self._tri) if self._tri is not None else ([0.0], [0])

    def set_profiling_features(self, on=True):
        if self._tri is None:
            self._tri = BackendSolver(self.options, self._device)
        self._tri.set_profiling(on)

    # ---- visual loop closure, third stage -------------------------------------------------------------------------
    def optimize4dof(self, vio_R, vio_T, sequence, fixed, loops, params=None):
        """≙ PoseGraph::optimize4DoF (pose_graph.cpp:406-582) on the device (vilf_pg4_optimize; the contract is in include/vilfusion.h). vio_R (n, 3, 3), vio_T (n, 3),
        sequence and fixed (n,), loops: iterable of (from, to, rel_t[3], rel_yaw); params: a dict of vilf_pg4_params fields that replace the defaults.
        Returns dict(t (n, 3), ypr (n, 3), R (n, 3, 3), result: dict of vilf_pg4_result, history (iterations, 5))."""
        R = np.ascontiguousarray(vio_R, dtype=np.float64).reshape(-1, 9)
        T = np.ascontiguousarray(vio_T, dtype=np.float64).reshape(-1, 3)
        seq = np.ascontiguousarray(sequence, dtype=np.int32).reshape(-1)
        fx = np.ascontiguousarray(np.asarray(fixed) != 0, dtype=np.int32).reshape(-1)
        n = len(T)
        if not (len(R) == n and len(seq) == n and len(fx) == n):
            raise ValueError("optimize4dof: vio_R, vio_T, sequence and fixed differ in length")
        p = pg4_default_params(**(params or {}))
        loops = list(loops)
        arr = (abi.Pg4Loop * max(len(loops), 1))()
        for k, (a, b, rel_t, rel_yaw) in enumerate(loops):
            arr[k].from_, arr[k].to, arr[k].rel_yaw = int(a), int(b), float(rel_yaw)
            arr[k].rel_t[:] = [float(v) for v in rel_t]
        t_out, ypr_out, R_out = np.zeros((max(n, 1), 3)), np.zeros((max(n, 1), 3)), np.zeros((max(n, 1), 9))
        hist = np.zeros((max(p.max_iterations, 1), 5))
        res = abi.Pg4Result()
        ip = C.POINTER(C.c_int)
        self._check(self._L.vilf_pg4_optimize(self._h, C.byref(p), n, abi.dptr(R), abi.dptr(T), seq.ctypes.data_as(ip), fx.ctypes.data_as(ip), len(loops), arr,
                                              abi.dptr(t_out), abi.dptr(ypr_out), abi.dptr(R_out), C.byref(res), abi.dptr(hist)), "vilf_pg4_optimize")
        result = dict(iterations=res.iterations, accepted=res.accepted, pivot_rejections=res.pivot_rejections, flags=res.flags, cost0=res.cost0, cost1=res.cost1,
                      radius=res.radius, yaw_drift=res.yaw_drift, r_drift=np.array(res.r_drift).reshape(3, 3), t_drift=np.array(res.t_drift))
        return dict(t=t_out[:n], ypr=ypr_out[:n], R=R_out[:n].reshape(-1, 3, 3), result=result, history=hist[:res.iterations].copy())

    def pg4_profile(self):
        """ms and spans of upload + first linearisation, chain, capacitance + dense solve, step + decision, download of the optimize4dof calls since set_profiling"""
        ms, cnt = (C.c_double * 5)(), (C.c_long * 5)()
        self._check(self._L.vilf_pg4_profile(self._h, ms, cnt), "vilf_pg4_profile")
        return dict(zip(PG4_STAGES, ((ms[i], cnt[i]) for i in range(5))))


PG4_STAGES = ("upload_linearize", "chain", "capacitance_solve", "step_decide", "download")


def pg4_default_params(**over):
    """vilf_pg4_params with the reference's constants (max_num_iterations = 5, HuberLoss(0.1), the / 10 of FourDOFWeightError) and Ceres's defaults for the
    trust region; keyword arguments replace fields"""
    p = abi.Pg4Params()
    lib().vilf_pg4_default_params(C.byref(p))
    for k, v in over.items():
        if not hasattr(p, k):
            raise AttributeError(f"vilf_pg4_params has no field {k}")
        setattr(p, k, v)
    return p


def imu_preintegrate(noise, acc_0, gyr_0, ba, bg, dt, acc, gyr):
    """≙ IntegrationBase (host): returns an abi.ImuPreint."""
    out = abi.ImuPreint()
    f = lambda v: abi.dptr(np.ascontiguousarray(v, dtype=np.float64))
    dt = np.ascontiguousarray(dt, dtype=np.float64)
    rc = lib().vilf_imu_preintegrate(C.byref(noise), f(acc_0), f(gyr_0), f(ba), f(bg), len(dt), abi.dptr(dt), f(acc), f(gyr), C.byref(out))
    if rc != 0:
        raise VilfError(f"vilf_imu_preintegrate: status {rc}")
    return out


def imu_preintegrate_batch(solver, noise, acc_0, gyr_0, ba, bg, n_samples, dt, acc, gyr):
    """≙ IntegrationBase for many intervals at once on the device (vilf_imu_preintegrate_batch). acc_0 / gyr_0 / ba / bg: (n, 3);
    n_samples: (n,); dt: (n, max); acc / gyr: (n, max, 3). Returns an (n, 467) array of vilf_imu_preint rows."""
    f64 = lambda v: np.ascontiguousarray(v, dtype=np.float64)
    acc_0, gyr_0, ba, bg, dt, acc, gyr = [f64(v) for v in (acc_0, gyr_0, ba, bg, dt, acc, gyr)]
    ns = np.ascontiguousarray(n_samples, dtype=np.int32)
    n, mx = len(ns), dt.shape[1] if dt.ndim == 2 else 0
    out = np.zeros((max(n, 1), abi.IMU_DOUBLES))
    L = solver._L
    L.vilf_imu_preintegrate_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(abi.ImuNoise), abi.c_double_p, abi.c_double_p, abi.c_double_p, abi.c_double_p,
                                              C.POINTER(C.c_int), C.c_int, abi.c_double_p, abi.c_double_p, abi.c_double_p, C.c_void_p]
    solver._check(L.vilf_imu_preintegrate_batch(solver._h, n, C.byref(noise), abi.dptr(acc_0), abi.dptr(gyr_0), abi.dptr(ba), abi.dptr(bg),
                                                ns.ctypes.data_as(C.POINTER(C.c_int)), mx, abi.dptr(dt), abi.dptr(acc), abi.dptr(gyr), out.ctypes.data), "vilf_imu_preintegrate_batch")
    return out[:n]


def visual_imu_alignment(solver, noise, frame_R, frame_T, acc_0, gyr_0, lin_ba, lin_bg, n_samples, dt, acc, gyr, bgs0):
    """≙ VisualIMUAlignment(all_image_frame, Bgs, g, x) (initial/initial_aligment.cpp:199) on the device (vilf_visual_imu_alignment).
    frame_R (n, 3, 3) = c0_R_bk, frame_T (n, 3) = c0_T_ck up to scale, the n - 1 raw IMU intervals as in imu_preintegrate_batch.
    Returns dict(ok, delta_bg, g, x, pre): the reference's bool, the gyro-bias correction, refined gravity in c0, x = [body velocities,
    2 tangent coefficients, scale] and the intervals re-integrated at (0, bgs0 + delta_bg) as (n - 1, 467) vilf_imu_preint rows."""
    f64 = lambda v: np.ascontiguousarray(v, dtype=np.float64)
    frame_R, frame_T, acc_0, gyr_0, lin_ba, lin_bg, dt, acc, gyr, bgs0 = [f64(v) for v in (frame_R, frame_T, acc_0, gyr_0, lin_ba, lin_bg, dt, acc, gyr, bgs0)]
    ns = np.ascontiguousarray(n_samples, dtype=np.int32)
    n = len(frame_R)
    assert frame_R.size == 9 * n and frame_T.size == 3 * n and len(ns) == n - 1
    dbg, g, x = np.zeros(3), np.zeros(3), np.zeros(3 * n + 4)
    pre = np.zeros((max(n - 1, 1), abi.IMU_DOUBLES))
    nx, ok = C.c_int(0), C.c_int(0)
    L = solver._L
    dp = abi.c_double_p
    L.vilf_visual_imu_alignment.argtypes = [C.c_void_p, C.c_int, dp, dp, C.POINTER(abi.ImuNoise), dp, dp, dp, dp, C.POINTER(C.c_int), C.c_int, dp, dp, dp,
                                            dp, dp, dp, dp, C.POINTER(C.c_int), C.c_void_p, C.POINTER(C.c_int)]
    solver._check(L.vilf_visual_imu_alignment(solver._h, n, abi.dptr(frame_R), abi.dptr(frame_T), C.byref(noise), abi.dptr(acc_0), abi.dptr(gyr_0), abi.dptr(lin_ba),
                                              abi.dptr(lin_bg), ns.ctypes.data_as(C.POINTER(C.c_int)), dt.shape[1] if dt.ndim == 2 else 0, abi.dptr(dt), abi.dptr(acc),
                                              abi.dptr(gyr), abi.dptr(bgs0), abi.dptr(dbg), abi.dptr(g), abi.dptr(x), C.byref(nx), pre.ctypes.data, C.byref(ok)),
                  "vilf_visual_imu_alignment")
    return dict(ok=bool(ok.value), delta_bg=dbg, g=g, x=x[:nx.value].copy(), pre=pre[:n - 1])


def startup_default_params(**over):
    """vilf_startup_params with the reference's constants (estimator.cpp:468-481, solve_5pts.cpp:195-221); keyword arguments replace fields (n_hypotheses=64, seed=3, ...)"""
    p = abi.StartupParams()
    lib().vilf_startup_default_params(C.byref(p))
    for k, v in over.items():
        if not hasattr(p, k):
            raise TypeError(f"vilf_startup_params has no field {k}")
        setattr(p, k, v)
    return p


def _startup_windows(windows):
    """-> (the ctypes array of vilf_startup_window, the numpy arrays it points into)"""
    W = (abi.StartupWindow * max(len(windows), 1))()
    keep = []
    for k, w in enumerate(windows):
        start = np.ascontiguousarray(w["start_frame"], dtype=np.int32)
        first = np.ascontiguousarray(w["first_obs"], dtype=np.int32)
        pts = np.ascontiguousarray(w["pts"], dtype=np.float64).reshape(-1, 2)
        keep.append((start, first, pts))
        W[k].n_frames, W[k].n_features = int(w["n_frames"]), len(start)
        W[k].start_frame = start.ctypes.data_as(C.POINTER(C.c_int32))
        W[k].first_obs = first.ctypes.data_as(C.POINTER(C.c_int32))
        W[k].pts = abi.dptr(pts)
    return W, keep


def relative_pose(solver, windows, correspondences=False, **params):
    """≙ Estimator::relativePose (estimator.cpp:461-490) for every window at once on the device (vilf_startup_relative_pose). windows: an iterable of
    dict(n_frames, start_frame [n], first_obs [n + 1], pts [total][2]): the feature table in feature order, normalised image points. params: fields of
    vilf_startup_params. Returns a list of dict(ok, l, R, T, inlier_cnt, pairs) per window; pairs = the rows of the pairs (i, newest), i = 0 .. n_frames - 2, as
    dicts. correspondences=True adds to every row feature [count], mask [count] (bit 0 RANSAC inlier, bit 1 good under the chosen candidate), points [count][3]."""
    L = lib()
    p = startup_default_params(**params)
    windows = list(windows)
    n = len(windows)
    W, keep = _startup_windows(windows)
    NP, NF = abi.VILF_MAX_FRAMES - 1, abi.VILF_MAX_FEATURES
    out = (abi.StartupResult * max(n, 1))()
    rows = (abi.StartupPair * (max(n, 1) * NP))()
    solver._check(L.vilf_startup_relative_pose(solver._h, C.byref(p), n, W, out, rows), "vilf_startup_relative_pose")
    if correspondences:
        feat = np.zeros((n, NP, NF), dtype=np.int32); mask = np.zeros((n, NP, NF), dtype=np.uint8); points = np.zeros((n, NP, NF, 3))
        solver._check(L.vilf_startup_get_correspondences(solver._h, n, feat.ctypes.data_as(C.POINTER(C.c_int)), mask.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                         abi.dptr(points)), "vilf_startup_get_correspondences")
    res = []
    for k, w in enumerate(windows):
        pairs = []
        for i in range(int(w["n_frames"]) - 1):
            r = rows[k * NP + i]
            row = dict(count=r.count, flags=r.flags, best_k=r.best_k, score=r.score, cheirality=[int(v) for v in r.cheirality], chosen=r.chosen,
                       inlier_cnt=r.inlier_cnt, parallax=float(r.parallax), F=np.array(r.F), R=np.array(r.R).reshape(3, 3), T=np.array(r.T),
                       ok=r.flags == abi.VILF_SU_PASS)
            if correspondences:
                row.update(feature=feat[k, i, :r.count].copy(), mask=mask[k, i, :r.count].copy(), points=points[k, i, :r.count].copy())
            pairs.append(row)
        o = out[k]
        res.append(dict(ok=o.l >= 0, l=o.l, R=np.array(o.R).reshape(3, 3), T=np.array(o.T), inlier_cnt=o.inlier_cnt, pairs=pairs))
    return res


def startup_profile(solver):
    """ms and launches of su_gather, su_hypotheses, su_score, su_pose since vilf_set_profiling"""
    ms, cnt = (C.c_double * 4)(), (C.c_long * 4)()
    solver._check(lib().vilf_startup_profile(solver._h, ms, cnt), "vilf_startup_profile")
    return list(ms), list(cnt)


def startup_default_sfm_params(**over):
    """vilf_startup_sfm_params with the reference's constants (initial_sfm.cpp:45-48); keyword arguments replace fields (pnp_iterations=1, ...)"""
    p = abi.StartupSfmParams()
    lib().vilf_startup_default_sfm_params(C.byref(p))
    for k, v in over.items():
        if not hasattr(p, k):
            raise TypeError(f"vilf_startup_sfm_params has no field {k}")
        setattr(p, k, v)
    return p


def _startup_frame(r):
    return dict(count=r.count, flags=r.flags, accepted=r.accepted, cost0=float(r.cost0), cost1=float(r.cost1), R=np.array(r.R).reshape(3, 3), t=np.array(r.t),
                Q=np.array(r.Q).reshape(3, 3), T=np.array(r.T))


def global_sfm(solver, windows, rel=None, structure=False, **params):
    """≙ the frame chain of GlobalSFM::construct (initial/initial_sfm.cpp:117-217) for every window at once on the device (vilf_startup_sfm). windows as in
    relative_pose; rel: per window a dict with l, R, T (what relative_pose returns) or None, which runs relative_pose first with the fields of vilf_startup_params
    among params and feeds its results through; the other params are fields of vilf_startup_sfm_params. Returns a list of dict(ok, fail_frame, n_triangulated,
    l, frames) per window, frames = the rows of the frames 0 .. n_frames - 1 as dicts (count, flags, accepted, cost0, cost1, R, t, Q, T). structure=True adds
    state [n_features] and positions [n_features][3], in the camera of frame l."""
    L = lib()
    windows = list(windows)
    n = len(windows)
    stage1 = {k: params.pop(k) for k in list(params) if hasattr(abi.StartupParams, k) and not hasattr(abi.StartupSfmParams, k)}
    p = startup_default_sfm_params(**params)
    if rel is None:
        rel = relative_pose(solver, windows, **stage1)
    elif stage1:
        raise TypeError(f"parameters of relative_pose given together with rel: {sorted(stage1)}")
    W, keep = _startup_windows(windows)
    rl = (abi.StartupResult * max(n, 1))()
    for k, r in enumerate(rel):
        rl[k].l = int(r["l"])
        rl[k].R[:] = [float(v) for v in np.asarray(r["R"], dtype=np.float64).reshape(9)]
        rl[k].T[:] = [float(v) for v in np.asarray(r["T"], dtype=np.float64).reshape(3)]
    NF, NX = abi.VILF_MAX_FRAMES, abi.VILF_MAX_FEATURES
    out = (abi.StartupStructure * max(n, 1))()
    rows = (abi.StartupFrame * (max(n, 1) * NF))()
    solver._check(L.vilf_startup_sfm(solver._h, C.byref(p), n, W, rl, out, rows), "vilf_startup_sfm")
    if structure:
        state = np.zeros((n, NX), dtype=np.uint8); pos = np.zeros((n, NX, 3))
        solver._check(L.vilf_startup_get_structure(solver._h, n, state.ctypes.data_as(C.POINTER(C.c_uint8)), abi.dptr(pos)), "vilf_startup_get_structure")
    res = []
    for k, w in enumerate(windows):
        o = out[k]
        r = dict(ok=bool(o.ok), fail_frame=o.fail_frame, n_triangulated=o.n_triangulated, l=o.l, frames=[_startup_frame(rows[k * NF + i]) for i in range(int(w["n_frames"]))])
        if structure:
            nx = len(keep[k][0])
            r.update(state=state[k, :nx].copy(), positions=pos[k, :nx].copy())
        res.append(r)
    return res


def frame_pnp(solver, problems, **params):
    """≙ solveFrameByPnP (initial_sfm.cpp:22-72) alone for a batch of independent problems on the device (vilf_startup_pnp). problems: an iterable of
    dict(pts3 [n][3], pts2 [n][2], R [3][3], t [3], min_count): the members in their order, the guess and the problem's minimum count (estimator.cpp:352 uses 6).
    params: fields of vilf_startup_sfm_params. Returns the rows as dicts, as the frames of global_sfm."""
    L = lib()
    p = startup_default_sfm_params(**params)
    problems = list(problems)
    n = len(problems)
    arr = (abi.StartupPnpProblem * max(n, 1))()
    keep = []
    for k, q in enumerate(problems):
        p3 = np.ascontiguousarray(q["pts3"], dtype=np.float64).reshape(-1, 3)
        p2 = np.ascontiguousarray(q["pts2"], dtype=np.float64).reshape(-1, 2)
        assert len(p3) == len(p2)
        keep.append((p3, p2))
        arr[k].n, arr[k].min_count = len(p3), int(q["min_count"])
        arr[k].pts3, arr[k].pts2 = abi.dptr(p3), abi.dptr(p2)
        arr[k].R[:] = [float(v) for v in np.asarray(q["R"], dtype=np.float64).reshape(9)]
        arr[k].t[:] = [float(v) for v in np.asarray(q["t"], dtype=np.float64).reshape(3)]
    out = (abi.StartupFrame * max(n, 1))()
    solver._check(L.vilf_startup_pnp(solver._h, C.byref(p), n, arr, out), "vilf_startup_pnp")
    return [_startup_frame(out[k]) for k in range(n)]


def startup_sfm_profile(solver):
    """ms and launches of su_sfm_chain and su_pnp_batch since vilf_set_profiling"""
    ms, cnt = (C.c_double * 2)(), (C.c_long * 2)()
    solver._check(lib().vilf_startup_sfm_profile(solver._h, ms, cnt), "vilf_startup_sfm_profile")
    return list(ms), list(cnt)


def startup_default_ba_params(**over):
    """vilf_startup_ba_params with the reference's constants (initial_sfm.cpp:277-289, Ceres's function tolerance); keyword arguments replace fields (ba_iterations=1, ...)"""
    p = abi.StartupBaParams()
    lib().vilf_startup_default_ba_params(C.byref(p))
    for k, v in over.items():
        if not hasattr(p, k):
            raise TypeError(f"vilf_startup_ba_params has no field {k}")
        setattr(p, k, v)
    return p


def _startup_ba_results(solver, windows, keep, out, rows):
    """the BA's rows and its structure (vilf_startup_get_ba_structure) as dicts per window"""
    n = len(windows)
    NF, NX = abi.VILF_MAX_FRAMES, abi.VILF_MAX_FEATURES
    state = np.zeros((n, NX), dtype=np.uint8); pos = np.zeros((n, NX, 3))
    solver._check(lib().vilf_startup_get_ba_structure(solver._h, n, state.ctypes.data_as(C.POINTER(C.c_uint8)), abi.dptr(pos)), "vilf_startup_get_ba_structure")
    res = []
    for k, w in enumerate(windows):
        o, nx = out[k], len(keep[k][0])
        frames = [dict(R=np.array(r.R).reshape(3, 3), t=np.array(r.t), Q=np.array(r.Q).reshape(3, 3), T=np.array(r.T)) for r in rows[k * NF:k * NF + int(w["n_frames"])]]
        res.append(dict(ok=bool(o.ok), flags=o.flags, iterations=o.iterations, accepted=o.accepted, n_camera=o.n_camera, n_members=o.n_members, n_residuals=o.n_residuals,
                        l=o.l, cost0=float(o.cost0), cost1=float(o.cost1), lam=float(o.lambda_), frames=frames, state=state[k, :nx].copy(), positions=pos[k, :nx].copy()))
    return res


def bundle_adjust(solver, windows, starts, **params):
    """≙ the full bundle adjustment of GlobalSFM::construct (initial/initial_sfm.cpp:232-310) alone, for every window at once on the device (vilf_startup_ba). windows
    as in relative_pose; starts: per window a dict(l, R [n_frames][3][3], t [n_frames][3], state [n_features], positions [n_features][3]) and optionally chain_ok
    (default True), the poses in the chain's convention. params: fields of vilf_startup_ba_params. Returns a list of dict(ok, flags, iterations, accepted, n_camera,
    n_members, n_residuals, l, cost0, cost1, lam, frames (dicts of R, t, Q, T), state, positions) per window."""
    L = lib()
    p = startup_default_ba_params(**params)
    windows = list(windows)
    n = len(windows)
    W, keep = _startup_windows(windows)
    st = (abi.StartupBaStart * max(n, 1))()
    hold = []
    for k, s in enumerate(starts):
        st[k].l, st[k].chain_ok = int(s["l"]), int(bool(s.get("chain_ok", True)))
        R = np.ascontiguousarray(s["R"], dtype=np.float64).reshape(-1, 9)
        t = np.ascontiguousarray(s["t"], dtype=np.float64).reshape(-1, 3)
        state = np.ascontiguousarray(s["state"], dtype=np.uint8)
        pos = np.ascontiguousarray(s["positions"], dtype=np.float64).reshape(-1, 3)
        assert len(R) >= int(windows[k]["n_frames"]) and len(t) >= int(windows[k]["n_frames"]) and len(state) >= len(keep[k][0]) and len(pos) >= len(keep[k][0])
        hold.append((R, t, state, pos))
        st[k].R, st[k].t, st[k].state, st[k].positions = abi.dptr(R), abi.dptr(t), state.ctypes.data_as(C.POINTER(C.c_uint8)), abi.dptr(pos)
    out = (abi.StartupBaResult * max(n, 1))()
    rows = (abi.StartupBaFrame * (max(n, 1) * abi.VILF_MAX_FRAMES))()
    solver._check(L.vilf_startup_ba(solver._h, C.byref(p), n, W, st, out, rows), "vilf_startup_ba")
    return _startup_ba_results(solver, windows, keep, out, rows)


def construct(solver, windows, rel=None, **params):
    """≙ GlobalSFM::construct (initial/initial_sfm.cpp:117-310): the frame chain, then the full bundle adjustment from its poses and structure, for every window at
    once and without a host round trip in between (vilf_startup_construct). windows and rel as in global_sfm (rel=None runs relative_pose first); params: fields of
    vilf_startup_params (only with rel=None), vilf_startup_sfm_params and vilf_startup_ba_params (lambda0 sets both, sfm_lambda0 / ba_lambda0 one of them). Returns
    the BA's dicts as bundle_adjust does, each with chain = dict(ok, fail_frame, n_triangulated, l, frames) as global_sfm returns it."""
    L = lib()
    windows = list(windows)
    n = len(windows)
    stage1 = {k: params.pop(k) for k in list(params) if hasattr(abi.StartupParams, k) and not hasattr(abi.StartupSfmParams, k) and not hasattr(abi.StartupBaParams, k)}
    sfm = {k: params[k] for k in params if hasattr(abi.StartupSfmParams, k)}
    ba = {k: params[k] for k in params if hasattr(abi.StartupBaParams, k)}
    if "sfm_lambda0" in params:
        sfm["lambda0"] = params.pop("sfm_lambda0")
    if "ba_lambda0" in params:
        ba["lambda0"] = params.pop("ba_lambda0")
    unknown = [k for k in params if k not in sfm and k not in ba]
    if unknown:
        raise TypeError(f"no start-up parameter is called {sorted(unknown)}")
    sp, bp = startup_default_sfm_params(**sfm), startup_default_ba_params(**ba)
    if rel is None:
        rel = relative_pose(solver, windows, **stage1)
    elif stage1:
        raise TypeError(f"parameters of relative_pose given together with rel: {sorted(stage1)}")
    W, keep = _startup_windows(windows)
    rl = (abi.StartupResult * max(n, 1))()
    for k, r in enumerate(rel):
        rl[k].l = int(r["l"])
        rl[k].R[:] = [float(v) for v in np.asarray(r["R"], dtype=np.float64).reshape(9)]
        rl[k].T[:] = [float(v) for v in np.asarray(r["T"], dtype=np.float64).reshape(3)]
    NF = abi.VILF_MAX_FRAMES
    out = (abi.StartupBaResult * max(n, 1))()
    rows = (abi.StartupBaFrame * (max(n, 1) * NF))()
    chain = (abi.StartupStructure * max(n, 1))()
    crow = (abi.StartupFrame * (max(n, 1) * NF))()
    solver._check(L.vilf_startup_construct(solver._h, C.byref(sp), C.byref(bp), n, W, rl, out, rows, chain, crow), "vilf_startup_construct")
    res = _startup_ba_results(solver, windows, keep, out, rows)
    for k, w in enumerate(windows):
        o = chain[k]
        res[k]["chain"] = dict(ok=bool(o.ok), fail_frame=o.fail_frame, n_triangulated=o.n_triangulated, l=o.l,
                               frames=[_startup_frame(crow[k * NF + i]) for i in range(int(w["n_frames"]))])
    return res


def startup_ba_profile(solver):
    """ms and launches of su_sfm_ba since vilf_set_profiling"""
    ms, cnt = (C.c_double * 1)(), (C.c_long * 1)()
    solver._check(lib().vilf_startup_ba_profile(solver._h, ms, cnt), "vilf_startup_ba_profile")
    return list(ms), list(cnt)


def triangulate_features(solver, tables):
    """≙ FeatureManager::triangulate (feature_manager.cpp:218-274) and getDepthVector (:194-216) for every window at once on the device
    (vilf_features_triangulate). tables: an iterable of dict(n_frames, Ps [n_frames][3], Rs [n_frames][3][3], tic [3], ric [3][3], start_frame [n], first_obs [n + 1],
    points [total][3], depth [n]): ALL features of the feature manager in list order (FeatureManager.triangulation_table). Returns per table a dict(depth [n]: the
    depths after triangulation, inv_depth [n_used]: getDepthVector, flags [n]: VILF_TRI_*, sweeps [n], result: dict(n_used, n_candidates, n_reset, n_nonfinite))."""
    L = lib()
    tables = list(tables)
    n = len(tables)
    W = (abi.TriWindow * max(n, 1))()
    keep = []
    i32p, u8p = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    for k, t in enumerate(tables):
        nf = int(t["n_frames"])
        Ps = np.ascontiguousarray(t["Ps"], dtype=np.float64).reshape(-1)[:3 * nf].copy()
        Rs = np.ascontiguousarray(t["Rs"], dtype=np.float64).reshape(-1)[:9 * nf].copy()
        start = np.ascontiguousarray(t["start_frame"], dtype=np.int32)
        first = np.ascontiguousarray(t["first_obs"], dtype=np.int32)
        pts = np.ascontiguousarray(t["points"], dtype=np.float64).reshape(-1, 3)
        din = np.ascontiguousarray(t["depth"], dtype=np.float64)
        m = len(start)
        dout, inv, flags, sweeps = np.zeros(max(m, 1)), np.zeros(max(m, 1)), np.zeros(max(m, 1), dtype=np.uint8), np.zeros(max(m, 1), dtype=np.uint8)
        keep.append((Ps, Rs, start, first, pts, din, dout, inv, flags, sweeps))
        w = W[k]
        w.n_frames, w.n_features = nf, m
        w.Ps, w.Rs = abi.dptr(Ps), abi.dptr(Rs)
        w.tic[:] = [float(v) for v in np.asarray(t["tic"], dtype=np.float64).reshape(3)]
        w.ric[:] = [float(v) for v in np.asarray(t["ric"], dtype=np.float64).reshape(9)]
        w.start_frame, w.first_obs = start.ctypes.data_as(i32p), first.ctypes.data_as(i32p)
        w.points, w.depth_in = abi.dptr(pts), abi.dptr(din)
        w.depth_out, w.inv_depth_out = abi.dptr(dout), abi.dptr(inv)
        w.flags_out, w.sweeps_out = flags.ctypes.data_as(u8p), sweeps.ctypes.data_as(u8p)
    out = (abi.TriResult * max(n, 1))()
    solver._check(L.vilf_features_triangulate(solver._h, n, W, out), "vilf_features_triangulate")
    res = []
    for k in range(n):
        m = len(keep[k][2])
        o = out[k]
        res.append(dict(depth=keep[k][6][:m], inv_depth=keep[k][7][:o.n_used], flags=keep[k][8][:m], sweeps=keep[k][9][:m],
                        result=dict(n_used=o.n_used, n_candidates=o.n_candidates, n_reset=o.n_reset, n_nonfinite=o.n_nonfinite)))
    return res


def features_profile(solver):
    """ms and kernel launches (tri_cameras + tri_solve: two per call that has a candidate) of vilf_features_triangulate since vilf_set_profiling"""
    ms, cnt = (C.c_double * 1)(), (C.c_long * 1)()
    solver._check(lib().vilf_features_profile(solver._h, ms, cnt), "vilf_features_profile")
    return list(ms), list(cnt)


def exrot_default_params(**over):
    """vilf_exrot_params with the reference's constants (initial_ex_rotation.cpp:30, :60, :71); keyword arguments replace fields (n_hypotheses=64, seed=3, ...)"""
    p = abi.ExrotParams()
    lib().vilf_exrot_default_params(C.byref(p))
    for k, v in over.items():
        if not hasattr(p, k):
            raise TypeError(f"vilf_exrot_params has no field {k}")
        setattr(p, k, v)
    return p


def exrot_result_dict(r):
    return dict(frame_count=r.frame_count, flags=r.flags, count=r.count, best_k=r.best_k, score=r.score, front=[int(v) for v in r.front], chosen=r.chosen,
                ok=bool(r.ok), Rc=np.array(r.Rc).reshape(3, 3), angle=np.float64(r.angle), weight=np.float64(r.weight), sigma=np.array(r.sigma), x=np.array(r.x),
                ric=np.array(r.ric).reshape(3, 3))


class ExRotation:
    """≙ InitialEXRotation (initial/initial_ex_rotation.cpp) for n_slots independent calibrators whose state lives on the device, in the handle of a BackendSolver
    (vilf_exrot_*). params: fields of vilf_exrot_params. A handle holds one set of calibrators: creating a second ExRotation on the same solver resets the first."""

    def __init__(self, solver, n_slots=1, **params):
        self.s, self.n_slots = solver, int(n_slots)
        self.params = exrot_default_params(**params)
        self.reset()

    def reset(self):
        """frame_count 0, ric = I and an empty history in every slot"""
        self.s._check(lib().vilf_exrot_reset(self.s._h, self.n_slots), "vilf_exrot_reset")

    def push(self, pairs):
        """pairs: per slot (a [m][2], b [m][2], delta_q [4] xyzw), the normalised points of the older and of the newer frame, or None to skip the slot.
        Returns per slot a dict of the fields of vilf_exrot_result (ok: the calibration succeeded and ric is calib_ric)."""
        pairs = list(pairs)
        n = len(pairs)
        arr = (abi.ExrotPair * max(n, 1))()
        keep = []
        for k, pr in enumerate(pairs):
            if pr is None:
                arr[k].n = -1
                continue
            a = np.ascontiguousarray(np.asarray(pr[0], dtype=np.float64).reshape(-1, 2))
            b = np.ascontiguousarray(np.asarray(pr[1], dtype=np.float64).reshape(-1, 2))
            if len(a) != len(b):
                raise ValueError("a and b of a pair differ in length")
            keep.append((a, b))
            arr[k].n, arr[k].a, arr[k].b = len(a), abi.dptr(a), abi.dptr(b)
            arr[k].delta_q[:] = [float(v) for v in np.asarray(pr[2], dtype=np.float64).reshape(4)]
        out = (abi.ExrotResult * max(n, 1))()
        self.s._check(lib().vilf_exrot_push(self.s._h, C.byref(self.params), n, arr, out), "vilf_exrot_push")
        return [exrot_result_dict(out[k]) for k in range(n)]

    def history(self, slot=0):
        """dict(count, Rc, Rimu, Rcg [count][3][3], angle, weight [count]: of the slot's last push)"""
        H = abi.VILF_EXROT_MAX_HISTORY
        Rc, Rimu, Rcg, ang, wgt = np.zeros((H, 3, 3)), np.zeros((H, 3, 3)), np.zeros((H, 3, 3)), np.zeros(H), np.zeros(H)
        cnt = C.c_int(0)
        self.s._check(lib().vilf_exrot_get_history(self.s._h, int(slot), C.byref(cnt), abi.dptr(Rc), abi.dptr(Rimu), abi.dptr(Rcg), abi.dptr(ang), abi.dptr(wgt)),
                      "vilf_exrot_get_history")
        c = cnt.value
        return dict(count=c, Rc=Rc[:c].copy(), Rimu=Rimu[:c].copy(), Rcg=Rcg[:c].copy(), angle=ang[:c].copy(), weight=wgt[:c].copy())

    def profile(self):
        """ms and launches of ex_hypotheses, ex_score, ex_solve since vilf_set_profiling"""
        ms, cnt = (C.c_double * 3)(), (C.c_long * 3)()
        self.s._check(lib().vilf_exrot_profile(self.s._h, ms, cnt), "vilf_exrot_profile")
        return list(ms), list(cnt)


def posegraph_optimize(solver, poses_qt, prior_sigma, edges, max_iterations=30, tol=1e-9):
    """≙ the gtsam graph + isam update of global_fusion (poseGraphOptimization.cpp:349-374, :560-587, :433-436) on the device
    (vilf_posegraph_optimize). poses_qt (n, 7) [qx qy qz qw tx ty tz]; edges: iterable of (i, j, q[4], t[3], sigma[6], robust).
    Returns (poses (n, 7), iterations, cost)."""
    x = np.ascontiguousarray(poses_qt, dtype=np.float64).copy()
    ps = np.ascontiguousarray(prior_sigma, dtype=np.float64)
    arr = (abi.PgEdge * max(len(edges), 1))()
    for k, (i, j, q, t, sg, rb) in enumerate(edges):
        arr[k].i, arr[k].j, arr[k].robust = int(i), int(j), int(rb)
        arr[k].q[:] = [float(v) for v in q]; arr[k].t[:] = [float(v) for v in t]; arr[k].sigma[:] = [float(v) for v in sg]
    it, cost = C.c_int(0), np.zeros(1)
    L = solver._L
    L.vilf_posegraph_optimize.argtypes = [C.c_void_p, C.c_int, abi.c_double_p, abi.c_double_p, C.c_int, C.POINTER(abi.PgEdge), C.c_int, C.c_double, C.POINTER(C.c_int), abi.c_double_p]
    solver._check(L.vilf_posegraph_optimize(solver._h, len(x), abi.dptr(x), abi.dptr(ps), len(edges), arr, max_iterations, tol, C.byref(it), abi.dptr(cost)), "vilf_posegraph_optimize")
    return x, it.value, cost[0]


def sc_default_params(**over):
    """vilf_sc_params with SCManager's constants (Scancontext.h:304-327); keyword arguments replace fields (dist_thres=0.4, num_candidates=0, ...)"""
    p = abi.ScParams()
    lib().vilf_sc_default_params(C.byref(p))
    for k, v in over.items():
        if not hasattr(p, k):
            raise AttributeError(f"vilf_sc_params has no field {k}")
        setattr(p, k, v)
    return p


def sc_result_dict(r):
    return dict(loop_id=r.loop_id, nearest=r.nearest, shift=r.shift, n_candidates=r.n_candidates, min_dist=r.min_dist, yaw_diff_rad=float(r.yaw_diff_rad),
                candidates=[int(v) for v in r.candidates[:min(max(r.n_candidates, 0), 16)]])


class ScanContext:
    """Host mirror of SCManager (global_fusion/include/Scancontext/Scancontext.h) over the device database of a BackendSolver handle (vilf_sc_*).
    Clouds are (n, 3) or (n, 4) arrays (xyz or xyzi). `last` holds the full record of the latest detectLoopClosureID."""

    def __init__(self, solver, capacity=4096, params=None, **over):
        self.s = solver
        self._L = solver._L
        self.params = params if params is not None else sc_default_params(**over)
        self.last = None
        self.s._check(self._L.vilf_sc_create(self.s._h, C.byref(self.params), int(capacity)), "vilf_sc_create")

    @staticmethod
    def _xyzi(cloud):
        a = np.asarray(cloud, dtype=np.float32)
        if a.size == 0:
            return np.zeros((0, 4), dtype=np.float32)
        assert a.ndim == 2 and a.shape[1] in (3, 4), a.shape
        if a.shape[1] == 3:
            a = np.concatenate([a, np.zeros((len(a), 1), dtype=np.float32)], axis=1)
        return np.ascontiguousarray(a)

    def __len__(self):
        n = C.c_int(0)
        self.s._check(self._L.vilf_sc_size(self.s._h, C.byref(n)), "vilf_sc_size")
        return n.value

    def makeAndSaveScancontextAndKeys(self, cloud):
        """:193-204. Returns the index of the new key frame."""
        a = self._xyzi(cloud)
        idx = C.c_int(-1)
        self.s._check(self._L.vilf_sc_add_keyframe(self.s._h, a.ctypes.data_as(C.POINTER(C.c_float)), len(a), C.byref(idx)), "vilf_sc_add_keyframe")
        return idx.value

    def add_many(self, clouds):
        """all clouds in one upload and one launch (vilf_sc_add_keyframes). Returns the index of the first."""
        cl = [self._xyzi(c) for c in clouds]
        off = np.zeros(len(cl) + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(c) for c in cl])
        pts = np.ascontiguousarray(np.concatenate(cl, axis=0)) if cl else np.zeros((0, 4), dtype=np.float32)
        first = C.c_int(-1)
        self.s._check(self._L.vilf_sc_add_keyframes(self.s._h, len(cl), pts.ctypes.data_as(C.POINTER(C.c_float)), off.ctypes.data_as(C.POINTER(C.c_int)), C.byref(first)),
                      "vilf_sc_add_keyframes")
        return first.value

    def detectLoopClosureID(self):
        """:210-300 for the newest key frame -> (loop_id, yaw_diff_rad)"""
        r = abi.ScResult()
        self.s._check(self._L.vilf_sc_detect(self.s._h, C.byref(r)), "vilf_sc_detect")
        self.last = sc_result_dict(r)
        return r.loop_id, float(r.yaw_diff_rad)

    def detect_range(self, first=0, n=None):
        """the replay (vilf_sc_detect_range): one record per key frame first .. first + n - 1, as a list of dicts"""
        n = len(self) - first if n is None else n
        arr = (abi.ScResult * max(n, 1))()
        self.s._check(self._L.vilf_sc_detect_range(self.s._h, int(first), int(n), arr), "vilf_sc_detect_range")
        return [sc_result_dict(arr[i]) for i in range(n)]

    def get(self, index):
        """(descriptor (20, 60) float64, ring key (20,) float32, sector key (60,) float64) of a key frame"""
        d, rk, sk = np.zeros((20, 60)), np.zeros(20, dtype=np.float32), np.zeros(60)
        self.s._check(self._L.vilf_sc_get(self.s._h, int(index), abi.dptr(d), rk.ctypes.data_as(C.POINTER(C.c_float)), abi.dptr(sk)), "vilf_sc_get")
        return d, rk, sk

    def profile(self):
        """ms and launches of sc_descriptor, sc_ringkey_topk, sc_distance, sc_reduce since vilf_set_profiling was switched on"""
        ms, cnt = (C.c_double * 4)(), (C.c_long * 4)()
        self.s._check(self._L.vilf_get_profile_sc(self.s._h, ms, cnt), "vilf_get_profile_sc")
        return dict(zip(("sc_descriptor", "sc_ringkey_topk", "sc_distance", "sc_reduce"), ((ms[i], cnt[i]) for i in range(4))))


KF_STAGES = ("upload_blur", "fast", "brief_lift", "match", "download")
KFL_STAGES = ("gather", "hypotheses", "score", "refine", "download")


def kf_default_loop_params(qic=None, tic=None, **over):
    """vilf_kf_loop_params with the reference's constants (keyframe.cpp:226-232, 406, 480); qic (3, 3) and tic (3,) are the camera-IMU extrinsic (identity and 0
    if not given); keyword arguments replace fields (n_hypotheses=256, seed=0, hyp_iterations=5, refine_iterations=10, min_loop_num=25, ...)"""
    p = abi.KfLoopParams()
    lib().vilf_kf_default_loop_params(C.byref(p))
    if qic is not None:
        p.qic = (C.c_double * 9)(*np.asarray(qic, dtype=np.float64).reshape(9))
    if tic is not None:
        p.tic = (C.c_double * 3)(*np.asarray(tic, dtype=np.float64).reshape(3))
    for k, v in over.items():
        if not hasattr(p, k):
            raise AttributeError(f"vilf_kf_loop_params has no field {k}")
        setattr(p, k, v)
    return p


def kf_loop_row_dict(r):
    return dict(n_matched=r.n_matched, n_inliers=r.n_inliers, best_k=r.best_k, flags=r.flags, has_loop=bool(r.has_loop), accepted=r.accepted,
                R=np.array(r.R).reshape(3, 3), t=np.array(r.t), PnP_R_old=np.array(r.PnP_R_old).reshape(3, 3), PnP_T_old=np.array(r.PnP_T_old),
                relative_t=np.array(r.relative_t), relative_q=np.array(r.relative_q), relative_yaw=r.relative_yaw, cost0=r.cost0, cost1=r.cost1)


BOW_STAGES = ("transform", "sort_compact", "score", "select", "download")


def load_vocabulary(path):
    """the VINS binary vocabulary (ThirdParty/VocabularyBinary.hpp; the reference's brief_k10L6.bin) -> dict of k, L, scoringType, weightingType, nodes (structured
    array abi.BOW_NODE_DTYPE: nodeId, parentId, weight, descriptor[4]) and words (abi.BOW_WORD_DTYPE: nodeId, wordId). The layout: six int32, then nNodes records
    of 48 bytes, then nWords records of 8 bytes. A file that ends early, or a negative count, raises ValueError."""
    with open(path, "rb") as f:
        raw = f.read()
    if len(raw) < 24:
        raise ValueError(f"{path}: {len(raw)} bytes, the header has 24")
    k, L, scoring, weighting, n_nodes, n_words = (int(v) for v in np.frombuffer(raw, dtype="<i4", count=6))
    if n_nodes < 0 or n_words < 0:
        raise ValueError(f"{path}: nNodes {n_nodes}, nWords {n_words}")
    need = 24 + n_nodes * abi.BOW_NODE_DTYPE.itemsize + n_words * abi.BOW_WORD_DTYPE.itemsize
    if len(raw) < need:
        raise ValueError(f"{path}: {len(raw)} bytes, {n_nodes} nodes and {n_words} words need {need}")
    nodes = np.frombuffer(raw, dtype=abi.BOW_NODE_DTYPE, count=n_nodes, offset=24).copy()
    words = np.frombuffer(raw, dtype=abi.BOW_WORD_DTYPE, count=n_words, offset=24 + n_nodes * abi.BOW_NODE_DTYPE.itemsize).copy()
    return dict(k=k, L=L, scoringType=scoring, weightingType=weighting, nodes=nodes, words=words)


def bow_default_params(**over):
    """vilf_bow_params with detectLoop's constants; keyword arguments replace fields (max_results=4, min_gap=50, neighbour_score=0.05, loop_score=0.015)"""
    p = abi.BowParams()
    lib().vilf_kf_bow_default_params(C.byref(p))
    for k, v in over.items():
        if not hasattr(p, k):
            raise AttributeError(f"vilf_bow_params has no field {k}")
        setattr(p, k, v)
    return p


def bow_result_dict(r):
    n = r.n_results
    return dict(loop_index=r.loop_index, find_loop=bool(r.find_loop), n_results=n, n_words=r.n_words, id=np.array(r.id[:], dtype=np.int32), score=np.array(r.score[:], dtype=np.float64),
                ret=[(r.id[i], r.score[i]) for i in range(min(max(n, 0), abi.VILF_BOW_MAX_RESULTS))])


def kf_default_params(width, height, camera, pattern, **over):
    """vilf_kf_params: camera = (fx, fy, cx, cy, k1, k2, p1, p2); pattern = (x1, y1, x2, y2), 256 integers each (the reference reads them from
    config/brief_pattern.yml); keyword arguments replace fields (fast_threshold=20, match_max_dist=128, match_accept_dist=80)"""
    p = abi.KfParams()
    lib().vilf_kf_default_params(C.byref(p))
    p.width, p.height = int(width), int(height)
    assert len(camera) == 8, "camera = (fx, fy, cx, cy, k1, k2, p1, p2)"
    p.fx, p.fy, p.cx, p.cy, p.k1, p.k2, p.p1, p.p2 = (float(v) for v in camera)
    assert len(pattern) == 4 and all(len(a) == abi.VILF_KF_BITS for a in pattern), "pattern = (x1, y1, x2, y2), 256 entries each"
    for name, a in zip(("x1", "y1", "x2", "y2"), pattern):
        setattr(p, name, (C.c_int * abi.VILF_KF_BITS)(*(int(v) for v in a)))
    for k, v in over.items():
        if not hasattr(p, k):
            raise AttributeError(f"vilf_kf_params has no field {k}")
        setattr(p, k, v)
    return p


class KeyFrameStore:
    """Host mirror of what pose_graph's KeyFrame computes from an image (keyframe.cpp:75-118) and of searchByBRIEFDes (:121-171), over the device store of a
    BackendSolver handle (vilf_kf_*). Images are (height, width) uint8 arrays, points (n, 2) float32 pixels, descriptors (n, 4) uint64 (bit i in word i // 64 at
    position i % 64). With a geometry (set_geometry) findConnection adds PnPRANSAC and the loop decision (:200-256, 401-520). The arithmetic is the contract in
    include/vilfusion.h. With a vocabulary (set_vocabulary; load_vocabulary reads the file) detectLoop names the old key frame: the DBoW2 query of
    pose_graph.cpp:307-389 over the stored key-point descriptors."""

    def __init__(self, solver, width, height, camera, pattern, cap_keyframes=1024, cap_keypoints=1 << 20, params=None, **over):
        self.s, self._L = solver, solver._L
        self.params = params if params is not None else kf_default_params(width, height, camera, pattern, **over)
        self.width, self.height = self.params.width, self.params.height
        self.s._check(self._L.vilf_kf_create(self.s._h, C.byref(self.params), int(cap_keyframes), int(cap_keypoints)), "vilf_kf_create")
        self.has_vocabulary = False

    def _img(self, img):
        a = np.asarray(img)
        assert a.dtype == np.uint8 and a.ndim == 2 and a.shape == (self.height, self.width) and a.strides[1] == 1 and a.strides[0] >= self.width, (a.dtype, a.shape, a.strides)
        return a

    @staticmethod
    def _u8(a):
        return a.ctypes.data_as(C.POINTER(C.c_uint8))

    @staticmethod
    def _fp(a):
        return a.ctypes.data_as(C.POINTER(C.c_float))

    @staticmethod
    def _ip(a):
        return a.ctypes.data_as(C.POINTER(C.c_int))

    @staticmethod
    def _u64(a):
        return a.ctypes.data_as(C.POINTER(C.c_uint64))

    @staticmethod
    def _pts(p):
        return np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 2)

    @staticmethod
    def _desc(d):
        return np.ascontiguousarray(d, dtype=np.uint64).reshape(-1, abi.VILF_KF_WORDS)

    def __len__(self):
        n = C.c_int(0)
        self.s._check(self._L.vilf_kf_size(self.s._h, C.byref(n)), "vilf_kf_size")
        return n.value

    def add_keyframe(self, img, window_uv):
        """computeWindowBRIEFPoint and computeBRIEFPoint for one image and its window points (point_2d_uv) -> (index, number of FAST key points)"""
        a, w = self._img(img), self._pts(window_uv)
        idx, nkp = C.c_int(-1), C.c_int(0)
        self.s._check(self._L.vilf_kf_add_keyframe(self.s._h, self._u8(a), int(a.strides[0]), self._fp(w), len(w), C.byref(idx), C.byref(nkp)), "vilf_kf_add_keyframe")
        return idx.value, nkp.value

    def add_loaded(self, keypoints, keypoints_norm, descriptors, window_uv, window_descriptors):
        """the "load previous keyframe" constructor (keyframe.cpp:44-72): a key frame from stored data -> index"""
        kp, kn, d, w, wd = self._pts(keypoints), self._pts(keypoints_norm), self._desc(descriptors), self._pts(window_uv), self._desc(window_descriptors)
        assert len(kp) == len(kn) == len(d) and len(w) == len(wd)
        idx = C.c_int(-1)
        self.s._check(self._L.vilf_kf_add_loaded(self.s._h, len(kp), self._fp(kp), self._fp(kn), self._u64(d), len(w), self._fp(w), self._u64(wd), C.byref(idx)), "vilf_kf_add_loaded")
        return idx.value

    def get(self, index):
        """a stored key frame as a dict: keypoints, keypoints_norm (n, 2) float32, descriptors (n, 4) uint64, window_uv (m, 2) float32, window_descriptors (m, 4) uint64"""
        nk, nw = C.c_int(0), C.c_int(0)
        self.s._check(self._L.vilf_kf_get(self.s._h, int(index), 0, None, None, None, C.byref(nk), 0, None, None, C.byref(nw)), "vilf_kf_get")
        k, m = nk.value, nw.value
        kp, kn, w = (np.zeros((max(n, 1), 2), dtype=np.float32) for n in (k, k, m))
        d, wd = (np.zeros((max(n, 1), abi.VILF_KF_WORDS), dtype=np.uint64) for n in (k, m))
        self.s._check(self._L.vilf_kf_get(self.s._h, int(index), k, self._fp(kp), self._fp(kn), self._u64(d), None, m, self._fp(w), self._u64(wd), None), "vilf_kf_get")
        return dict(keypoints=kp[:k], keypoints_norm=kn[:k], descriptors=d[:k], window_uv=w[:m], window_descriptors=wd[:m])

    def searchByBRIEFDes(self, cur, olds):
        """:152-171 for key frame cur against every old key frame of `olds`, in one launch -> dict of status (n_old, n) uint8, pt_old, pt_old_norm (n_old, n, 2)
        float32, best_index, best_dist (n_old, n) int32, n_matched (n_old,) int32, with n the window points of cur"""
        old = np.ascontiguousarray(olds, dtype=np.int32).reshape(-1)
        nw = C.c_int(0)
        self.s._check(self._L.vilf_kf_get(self.s._h, int(cur), 0, None, None, None, None, 0, None, None, C.byref(nw)), "vilf_kf_get")
        n, k = nw.value, len(old)
        rows = max(n * k, 1)
        st = np.zeros(rows, dtype=np.uint8)
        pt, ptn = np.zeros((rows, 2), dtype=np.float32), np.zeros((rows, 2), dtype=np.float32)
        bi, bd, nm = np.zeros(rows, dtype=np.int32), np.zeros(rows, dtype=np.int32), np.zeros(max(k, 1), dtype=np.int32)
        self.s._check(self._L.vilf_kf_match(self.s._h, int(cur), k, self._ip(old), self._u8(st), self._fp(pt), self._fp(ptn), self._ip(bi), self._ip(bd), self._ip(nm)), "vilf_kf_match")
        return dict(status=st[:n * k].reshape(k, n), pt_old=pt[:n * k].reshape(k, n, 2), pt_old_norm=ptn[:n * k].reshape(k, n, 2), best_index=bi[:n * k].reshape(k, n),
                    best_dist=bd[:n * k].reshape(k, n), n_matched=nm[:k])

    def set_geometry(self, index, point_3d, vio_R, vio_T):
        """the geometry of a stored key frame: point_3d (n_window, 3) float32 (the world points of its window features), origin_vio_R (3, 3), origin_vio_T (3,).
        A second call replaces it."""
        X = np.ascontiguousarray(point_3d, dtype=np.float32).reshape(-1, 3)
        R, T = np.ascontiguousarray(vio_R, dtype=np.float64).reshape(9), np.ascontiguousarray(vio_T, dtype=np.float64).reshape(3)
        nw = C.c_int(0)
        self.s._check(self._L.vilf_kf_get(self.s._h, int(index), 0, None, None, None, None, 0, None, None, C.byref(nw)), "vilf_kf_get")
        if len(X) != nw.value:
            raise ValueError(f"{len(X)} world points for {nw.value} window points")
        self.s._check(self._L.vilf_kf_set_geometry(self.s._h, int(index), self._fp(X), abi.dptr(R), abi.dptr(T)), "vilf_kf_set_geometry")

    def findConnection(self, cur, olds, qic, tic, point_id=None, params=None, **over):
        """PnPRANSAC and the loop decision of findConnection (:401-520) for key frame cur against every old key frame of `olds`, in one chain of launches -> one
        dict per old key frame: the fields of vilf_kf_loop_result, loop_info (the 8-vector relative_t, relative_q (w, x, y, z), relative_yaw of :485-487, or None
        without a loop), status (n,) uint8 (the inlier mask over the window points of cur) and, with point_id (n,) given, match_points (k, 3) float32: the
        (x, y, id) rows of the fast-relocalisation message (:492-499) for the inliers (the reference publishes them only with a loop)."""
        old = np.ascontiguousarray(olds, dtype=np.int32).reshape(-1)
        p = params if params is not None else kf_default_loop_params(qic, tic, **over)
        nw = C.c_int(0)
        self.s._check(self._L.vilf_kf_get(self.s._h, int(cur), 0, None, None, None, None, 0, None, None, C.byref(nw)), "vilf_kf_get")
        n, k = nw.value, len(old)
        rows = (abi.KfLoopResult * max(k, 1))()
        st, ptn = np.zeros(max(n * k, 1), dtype=np.uint8), np.zeros((max(n * k, 1), 2), dtype=np.float32)
        self.s._check(self._L.vilf_kf_find_connection(self.s._h, C.byref(p), int(cur), k, self._ip(old), rows, self._u8(st), self._fp(ptn)), "vilf_kf_find_connection")
        st, ptn = st[:n * k].reshape(k, n), ptn[:n * k].reshape(k, n, 2)
        ids = None if point_id is None else np.asarray(point_id).reshape(n)
        out = []
        for i in range(k):
            r = kf_loop_row_dict(rows[i])
            r["loop_info"] = np.concatenate([r["relative_t"], r["relative_q"], [r["relative_yaw"]]]) if r["has_loop"] else None
            r["status"] = st[i].copy()
            if ids is not None:
                on = st[i] != 0
                r["match_points"] = np.concatenate([ptn[i][on], ids[on].astype(np.float32).reshape(-1, 1)], axis=1).astype(np.float32).reshape(-1, 3)
            out.append(r)
        return out

    def loop_profile(self):
        """ms and spans of gather, hypotheses, score, refine, download of the findConnection calls since vilf_set_profiling was switched on"""
        ms, cnt = (C.c_double * 5)(), (C.c_long * 5)()
        self.s._check(self._L.vilf_kf_loop_profile(self.s._h, ms, cnt), "vilf_kf_loop_profile")
        return dict(zip(KFL_STAGES, ((ms[i], cnt[i]) for i in range(5))))

    # ---- candidate retrieval (vilf_kf_bow_*): detectLoop's DBoW2 query over the stored key-point descriptors ----
    def set_vocabulary(self, voc):
        """voc: what load_vocabulary returns (k, L, scoringType, weightingType, nodes, words). Validated, renumbered breadth-first and uploaded; drops the database."""
        nodes = np.ascontiguousarray(voc["nodes"], dtype=abi.BOW_NODE_DTYPE).reshape(-1)
        words = np.ascontiguousarray(voc["words"], dtype=abi.BOW_WORD_DTYPE).reshape(-1)
        v = abi.BowVocabulary(int(voc["k"]), int(voc["L"]), int(voc["scoringType"]), int(voc["weightingType"]), len(nodes), len(words),
                              nodes.ctypes.data_as(C.POINTER(abi.BowNode)), words.ctypes.data_as(C.POINTER(abi.BowWord)))
        self.s._check(self._L.vilf_kf_bow_set_vocabulary(self.s._h, C.byref(v)), "vilf_kf_bow_set_vocabulary")
        self.has_vocabulary = True

    def bow_size(self):
        n = C.c_int(0)
        self.s._check(self._L.vilf_kf_bow_size(self.s._h, C.byref(n)), "vilf_kf_bow_size")
        return n.value

    def bow_add(self, index):
        """addKeyFrameIntoVoc (pose_graph.cpp:391-404): key frame `index` (= the database's size) becomes an entry"""
        self.s._check(self._L.vilf_kf_bow_add(self.s._h, int(index)), "vilf_kf_bow_add")

    def bow_add_range(self, first, n):
        """the same for n key frames in one chain of launches"""
        self.s._check(self._L.vilf_kf_bow_add_range(self.s._h, int(first), int(n)), "vilf_kf_bow_add_range")

    def detect_loop(self, index, params=None, **over):
        """detectLoop (:307-389) for key frame `index` (= the database's size): query, add, decision -> dict of loop_index, find_loop, n_results, n_words, id, score
        (16 each, the rest -1 / 0) and ret, the (Id, Score) pairs"""
        p = params if params is not None else bow_default_params(**over)
        r = abi.BowResult()
        self.s._check(self._L.vilf_kf_bow_detect(self.s._h, C.byref(p), int(index), C.byref(r)), "vilf_kf_bow_detect")
        return bow_result_dict(r)

    def detectLoop(self, index, params=None, **over):
        """the reference's signature: the loop index or -1"""
        return self.detect_loop(index, params, **over)["loop_index"]

    def detect_loop_range(self, first, n, params=None, **over):
        """the replay: what detect_loop returned, or would have returned, for key frames first .. first + n - 1 on their arrival, over a database that holds them
        already; one chain of launches, the database is not touched -> list of dicts"""
        p = params if params is not None else bow_default_params(**over)
        rows = (abi.BowResult * max(int(n), 1))()
        self.s._check(self._L.vilf_kf_bow_detect_range(self.s._h, C.byref(p), int(first), int(n), rows), "vilf_kf_bow_detect_range")
        return [bow_result_dict(rows[i]) for i in range(int(n))]

    def bow_vector(self, index):
        """the stored vector of entry `index` -> (word ids (n,) int32 ascending, values (n,) float64)"""
        n = C.c_int(0)
        self.s._check(self._L.vilf_kf_bow_get(self.s._h, int(index), 0, None, None, C.byref(n)), "vilf_kf_bow_get")
        w, v = np.zeros(max(n.value, 1), dtype=np.int32), np.zeros(max(n.value, 1), dtype=np.float64)
        self.s._check(self._L.vilf_kf_bow_get(self.s._h, int(index), n.value, self._ip(w), abi.dptr(v), None), "vilf_kf_bow_get")
        return w[:n.value], v[:n.value]

    def bow_transform(self, desc):
        """(word id, weight) of each descriptor (n, 4) uint64 (stateless) -> ((n,) int32, (n,) float64)"""
        d = self._desc(desc)
        w, wt = np.zeros(max(len(d), 1), dtype=np.int32), np.zeros(max(len(d), 1), dtype=np.float64)
        self.s._check(self._L.vilf_kf_bow_transform(self.s._h, self._u64(d), len(d), self._ip(w), abi.dptr(wt)), "vilf_kf_bow_transform")
        return w[:len(d)], wt[:len(d)]

    def bow_profile(self):
        """ms and spans of transform, sort + compact, score, select, download since vilf_set_profiling was switched on"""
        ms, cnt = (C.c_double * 5)(), (C.c_long * 5)()
        self.s._check(self._L.vilf_kf_bow_profile(self.s._h, ms, cnt), "vilf_kf_bow_profile")
        return dict(zip(BOW_STAGES, ((ms[i], cnt[i]) for i in range(5))))

    def blur(self, img):
        """the blurred image BRIEF reads (stateless)"""
        a = self._img(img)
        out = np.zeros((self.height, self.width), dtype=np.uint8)
        self.s._check(self._L.vilf_kf_blur(self.s._h, self._u8(a), int(a.strides[0]), self._u8(out)), "vilf_kf_blur")
        return out

    def fast(self, img, cap=None):
        """the FAST key points of an image (stateless) -> (points (n, 2) float32 in row-major order, scores (n,) uint8); more than cap points raise"""
        a = self._img(img)
        cap = self.width * self.height if cap is None else int(cap)
        pts, sc = np.zeros((max(cap, 1), 2), dtype=np.float32), np.zeros(max(cap, 1), dtype=np.uint8)
        n = C.c_int(0)
        self.s._check(self._L.vilf_kf_fast(self.s._h, self._u8(a), int(a.strides[0]), cap, self._fp(pts), self._u8(sc), C.byref(n)), "vilf_kf_fast")
        return pts[:n.value].copy(), sc[:n.value].copy()

    def brief(self, img, pts):
        """the descriptors of points on the blur of an image (stateless) -> (n, 4) uint64"""
        a, p = self._img(img), self._pts(pts)
        out = np.zeros((max(len(p), 1), abi.VILF_KF_WORDS), dtype=np.uint64)
        self.s._check(self._L.vilf_kf_brief(self.s._h, self._u8(a), int(a.strides[0]), self._fp(p), len(p), self._u64(out)), "vilf_kf_brief")
        return out[:len(p)]

    def profile(self):
        """ms and spans of upload + blur, FAST, descriptors + lift, match, download since vilf_set_profiling was switched on"""
        ms, cnt = (C.c_double * 5)(), (C.c_long * 5)()
        self.s._check(self._L.vilf_kf_profile(self.s._h, ms, cnt), "vilf_kf_profile")
        return dict(zip(KF_STAGES, ((ms[i], cnt[i]) for i in range(5))))


ICP_MAP_KERNELS = ("gmap_xf_bbox", "gmap_leaf_keys", "radix_sort", "gmap_centroids")
ICP_KERNELS = ("icp_bbox", "icp_leaf_keys", "radix_sort", "icp_voxel", "icp_cell_table", "icp_search", "icp_step", "unused")


def icp_default_params(**over):
    """vilf_icp_params with the reference's constants (poseGraphOptimization.cpp:394-414); keyword arguments replace fields (own_pose=1, max_iterations=30, ...)"""
    p = abi.IcpParams()
    lib().vilf_icp_default_params(C.byref(p))
    for k, v in over.items():
        if not hasattr(p, k):
            raise AttributeError(f"vilf_icp_params has no field {k}")
        setattr(p, k, v)
    return p


def icp_result_dict(r):
    return dict(converged=bool(r.converged), accepted=bool(r.accepted), criterion=r.criterion, iterations=r.iterations, n_source=r.n_source, n_target=r.n_target,
                n_correspondences=r.n_correspondences, fitness=r.fitness, final_mse=r.final_mse, transform=np.array(r.transform, dtype=np.float32).reshape(4, 4),
                pose6=np.array(r.pose6), pose_qt=np.array(r.pose_qt))


class LoopICP:
    """Host mirror of icpCalculation (global_fusion/poseGraphOptimization.cpp:376-443) over the key-frame cloud store of a BackendSolver handle (vilf_icp_*).
    Clouds are (n, 3) or (n, 4) arrays; poses6 is (size, 6) [x y z roll pitch yaw], the KeyFramePosesUpdated of every stored key frame."""

    def __init__(self, solver, cap_keyframes=4096, cap_points=1 << 24, params=None, **over):
        self.s = solver
        self._L = solver._L
        self.params = params if params is not None else icp_default_params(**over)
        self.s._check(self._L.vilf_icp_create(self.s._h, C.byref(self.params), int(cap_keyframes), int(cap_points)), "vilf_icp_create")

    def __len__(self):
        n = C.c_int(0)
        self.s._check(self._L.vilf_icp_size(self.s._h, C.byref(n)), "vilf_icp_size")
        return n.value

    def add_cloud(self, cloud):
        """the cloud of the next key frame (thisKeyFrameDS). Returns its index."""
        a = ScanContext._xyzi(cloud)
        idx = C.c_int(-1)
        self.s._check(self._L.vilf_icp_add_cloud(self.s._h, a.ctypes.data_as(C.POINTER(C.c_float)), len(a), C.byref(idx)), "vilf_icp_add_cloud")
        return idx.value

    def add_many(self, clouds):
        """all clouds in one upload (vilf_icp_add_clouds). Returns the index of the first."""
        cl = [ScanContext._xyzi(c) for c in clouds]
        off = np.zeros(len(cl) + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(c) for c in cl])
        pts = np.ascontiguousarray(np.concatenate(cl, axis=0)) if cl else np.zeros((0, 4), dtype=np.float32)
        first = C.c_int(-1)
        self.s._check(self._L.vilf_icp_add_clouds(self.s._h, len(cl), pts.ctypes.data_as(C.POINTER(C.c_float)), off.ctypes.data_as(C.POINTER(C.c_int)), C.byref(first)),
                      "vilf_icp_add_clouds")
        return first.value

    def _poses(self, poses6):
        p = np.ascontiguousarray(np.asarray(poses6, dtype=np.float64).reshape(-1, 6))
        if len(p) < len(self):
            raise ValueError(f"{len(p)} poses for {len(self)} stored key frames")
        return p

    def submap(self, key, submap_size, root, poses6):
        """loopFindNearKeyframeCLoud(key, submap_size, root) :194-219 -> (n, 4) float32"""
        p = self._poses(poses6)
        n = C.c_int(0)
        self.s._check(self._L.vilf_icp_submap(self.s._h, int(key), int(submap_size), int(root), abi.dptr(p), None, 0, C.byref(n)), "vilf_icp_submap")
        out = np.zeros((max(n.value, 1), 4), dtype=np.float32)
        self.s._check(self._L.vilf_icp_submap(self.s._h, int(key), int(submap_size), int(root), abi.dptr(p), out.ctypes.data_as(C.POINTER(C.c_float)), n.value, C.byref(n)), "vilf_icp_submap")
        return out[:n.value]

    def align(self, prev, curr, poses6, guess_qt=None):
        """the ICP of the pair (prev, curr) -> result dict (pose_qt is what PoseGraph.add_loop takes)"""
        p = self._poses(poses6)
        g = None if guess_qt is None else np.ascontiguousarray(np.asarray(guess_qt, dtype=np.float64).reshape(7))
        r = abi.IcpResult()
        self.s._check(self._L.vilf_icp_align(self.s._h, int(prev), int(curr), abi.dptr(p), abi.dptr(g), C.byref(r)), "vilf_icp_align")
        return icp_result_dict(r)

    def align_pairs(self, pairs, poses6, guesses_qt=None):
        """all (prev, curr) pairs in one chain of launches -> list of result dicts, each identical to the single call"""
        p = self._poses(poses6)
        pr = np.ascontiguousarray(np.array([a for a, _ in pairs], dtype=np.int32))
        cu = np.ascontiguousarray(np.array([b for _, b in pairs], dtype=np.int32))
        g = None if guesses_qt is None else np.ascontiguousarray(np.asarray(guesses_qt, dtype=np.float64).reshape(len(pairs), 7))
        arr = (abi.IcpResult * max(len(pairs), 1))()
        ipt = C.POINTER(C.c_int)
        self.s._check(self._L.vilf_icp_align_pairs(self.s._h, len(pairs), pr.ctypes.data_as(ipt), cu.ctypes.data_as(ipt), abi.dptr(p), abi.dptr(g), arr), "vilf_icp_align_pairs")
        return [icp_result_dict(arr[i]) for i in range(len(pairs))]

    def history(self, pair=0):
        """the rounds of pair `pair` of the last align call, as a list of dicts"""
        n = C.c_int(0)
        arr = (abi.IcpIter * self.params.max_iterations)()
        self.s._check(self._L.vilf_icp_get_history(self.s._h, int(pair), arr, self.params.max_iterations, C.byref(n)), "vilf_icp_get_history")
        return [dict(n_correspondences=arr[i].n_correspondences, criterion=arr[i].criterion, mse=arr[i].mse, cos_angle=arr[i].cos_angle, translation_sqr=arr[i].translation_sqr)
                for i in range(min(n.value, self.params.max_iterations))]

    def search(self, pair=0, which=0):
        """(nearest target index, d2) of every source point of pair `pair` of the last align call: which = 0 the first round, 1 the fitness pass"""
        n = C.c_int(0)
        self.s._check(self._L.vilf_icp_get_search(self.s._h, int(pair), int(which), None, None, 0, C.byref(n)), "vilf_icp_get_search")
        idx, d2 = np.zeros(max(n.value, 1), dtype=np.int32), np.zeros(max(n.value, 1), dtype=np.float32)
        self.s._check(self._L.vilf_icp_get_search(self.s._h, int(pair), int(which), idx.ctypes.data_as(C.POINTER(C.c_int)), d2.ctypes.data_as(C.POINTER(C.c_float)), n.value, C.byref(n)),
                      "vilf_icp_get_search")
        return idx[:n.value], d2[:n.value]

    def profile(self):
        """ms and launches of the ICP kernels since vilf_set_profiling was switched on"""
        ms, cnt = (C.c_double * 8)(), (C.c_long * 8)()
        self.s._check(self._L.vilf_get_profile_icp(self.s._h, ms, cnt), "vilf_get_profile_icp")
        return dict(zip(ICP_KERNELS[:7], ((ms[i], cnt[i]) for i in range(7))))

    def global_map(self, poses6, first=0, count=None, skip=1):
        """publishGlobalMap :310-336: the clouds first, first + skip, ... (< first + count; count=None: to the end of the store), each under its own pose,
        concatenated and voxel-filtered -> (n, 4) float32. The map stays on the device until the next build (global_map_size, global_map_part)."""
        p = self._poses(poses6)
        n = C.c_long(0)
        cnt = len(self) - int(first) if count is None else int(count)
        self.s._check(self._L.vilf_icp_global_map(self.s._h, int(first), cnt, int(skip), abi.dptr(p), C.byref(n)), "vilf_icp_global_map")
        return self.global_map_part(0, n.value)

    def global_map_size(self):
        n = C.c_long(0)
        self.s._check(self._L.vilf_icp_global_map_size(self.s._h, C.byref(n)), "vilf_icp_global_map_size")
        return n.value

    def global_map_part(self, offset, count):
        """points [offset, offset + count) of the map built last -> (count, 4) float32"""
        out = np.zeros((max(int(count), 1), 4), dtype=np.float32)
        self.s._check(self._L.vilf_icp_global_map_get(self.s._h, int(offset), int(count), out.ctypes.data_as(C.POINTER(C.c_float))), "vilf_icp_global_map_get")
        return out[:max(int(count), 0)]

    def map_profile(self):
        """ms and launches of the global-map stages since vilf_set_profiling was switched on"""
        ms, cnt = (C.c_double * 4)(), (C.c_long * 4)()
        self.s._check(self._L.vilf_get_profile_icp_map(self.s._h, ms, cnt), "vilf_get_profile_icp_map")
        return dict(zip(ICP_MAP_KERNELS, ((ms[i], cnt[i]) for i in range(4))))


class Scan2Map:
    """Host mirror of EstimationMapping (feature_tracker/include/EstimationMapping.hpp): localMapInited / optimation_processing /
    getMapCloud over the device path. One LiDAR stream per BackendSolver handle."""

    def __init__(self, solver):
        self.s = solver
        self._L = solver._L

    @staticmethod
    def _fp(a):
        a = np.ascontiguousarray(a, dtype=np.float32)
        assert a.ndim == 2 and a.shape[1] == 4
        return a, a.ctypes.data_as(C.POINTER(C.c_float))

    def localMapInited(self, edge_xyzi, surf_xyzi):
        e, ep = self._fp(edge_xyzi); s, sp = self._fp(surf_xyzi)
        self.s._check(self._L.vilf_scan2map_init(self.s._h, ep, len(e), sp, len(s)), "vilf_scan2map_init")

    def optimation_processing(self, edge_xyzi, surf_xyzi):
        e, ep = self._fp(edge_xyzi); s, sp = self._fp(surf_xyzi)
        res = abi.Scan2MapResult()
        self.s._check(self._L.vilf_scan2map_step(self.s._h, ep, len(e), sp, len(s), C.byref(res)), "vilf_scan2map_step")
        return res

    def getMapCloud(self, which):
        n = C.c_int(0)
        self.s._check(self._L.vilf_scan2map_get_map(self.s._h, which, None, 0, C.byref(n)), "vilf_scan2map_get_map")
        out = np.zeros((max(n.value, 1), 4), dtype=np.float32)
        self.s._check(self._L.vilf_scan2map_get_map(self.s._h, which, out.ctypes.data_as(C.POINTER(C.c_float)), n.value, C.byref(n)), "vilf_scan2map_get_map")
        return out[:n.value]

    def set_pose(self, pose_qt, pose_last_qt):
        f = lambda v: abi.dptr(np.ascontiguousarray(v, dtype=np.float64))
        self.s._check(self._L.vilf_scan2map_set_pose(self.s._h, f(pose_qt), f(pose_last_qt)), "vilf_scan2map_set_pose")


class Scan2MapBatch:
    """n_streams independent EstimationMapping objects (one per LiDAR stream / replayed segment) stepped together on the
    device: fixed per-stream capacities, device-side counters, no host round trip inside a step."""

    def __init__(self, solver, n_streams, cap_scan_edge, cap_scan_surf, cap_map_edge, cap_map_surf):
        self.s = solver
        self._L = solver._L
        self.n = int(n_streams)
        self.s._check(self._L.vilf_scan2map_batch_create(self.s._h, self.n, int(cap_scan_edge), int(cap_scan_surf), int(cap_map_edge), int(cap_map_surf)),
                      "vilf_scan2map_batch_create")

    def localMapInited(self, stream, edge_xyzi, surf_xyzi, pose_qt=None, pose_last_qt=None):
        e, ep = Scan2Map._fp(edge_xyzi); s, sp = Scan2Map._fp(surf_xyzi)
        keep = [None if v is None else np.ascontiguousarray(v, dtype=np.float64) for v in (pose_qt, pose_last_qt)]
        pp, pl = [None if v is None else abi.dptr(v) for v in keep]
        self.s._check(self._L.vilf_scan2map_batch_init(self.s._h, stream, ep, len(e), sp, len(s), pp, pl), "vilf_scan2map_batch_init")

    def set_scan(self, stream, edge_xyzi, surf_xyzi):
        e, ep = Scan2Map._fp(edge_xyzi); s, sp = Scan2Map._fp(surf_xyzi)
        self.s._check(self._L.vilf_scan2map_batch_set_scan(self.s._h, stream, ep, len(e), sp, len(s)), "vilf_scan2map_batch_set_scan")

    def step(self, sync=True):
        self.s._check(self._L.vilf_scan2map_batch_step(self.s._h, 1 if sync else 0), "vilf_scan2map_batch_step")

    def snapshot(self):
        self.s._check(self._L.vilf_scan2map_batch_snapshot(self.s._h), "vilf_scan2map_batch_snapshot")

    def rewind(self):
        self.s._check(self._L.vilf_scan2map_batch_rewind(self.s._h), "vilf_scan2map_batch_rewind")

    def copy_stream(self, src, dst):
        """stream dst := stream src (maps, poses, resident scan), on the device"""
        self.s._check(self._L.vilf_scan2map_batch_copy_stream(self.s._h, src, dst), "vilf_scan2map_batch_copy_stream")

    def results(self, first=0, n=None):
        n = self.n - first if n is None else n
        arr = (abi.Scan2MapResult * n)()
        self.s._check(self._L.vilf_scan2map_batch_results(self.s._h, first, n, arr), "vilf_scan2map_batch_results")
        return list(arr)

    def getMapCloud(self, stream, which):
        n = C.c_int(0)
        self.s._check(self._L.vilf_scan2map_batch_get_map(self.s._h, stream, which, None, 0, C.byref(n)), "vilf_scan2map_batch_get_map")
        out = np.zeros((max(n.value, 1), 4), dtype=np.float32)
        self.s._check(self._L.vilf_scan2map_batch_get_map(self.s._h, stream, which, out.ctypes.data_as(C.POINTER(C.c_float)), n.value, C.byref(n)), "vilf_scan2map_batch_get_map")
        return out[:n.value]


class FeatureExtraction:
    """Host mirror of featureExtraction (feature_tracker/include/featureExtraction.hpp): extractFeature(raw scan) -> (edge, surf)
    over the device path. Parameters ≙ initParam (:43-52; velodyne_param_64.yaml)."""

    def __init__(self, solver, n_scans=64, min_range=3.0, max_range=100.0, edge_threshold=0.1):
        self.s, self._L = solver, solver._L
        self.n_scans, self.min_range, self.max_range, self.edge_threshold = int(n_scans), float(min_range), float(max_range), float(edge_threshold)
        fp = C.POINTER(C.c_float)
        self._L.vilf_lidar_extract_features.argtypes = [C.c_void_p, fp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, fp, C.c_int, C.POINTER(C.c_int),
                                                        fp, C.c_int, C.POINTER(C.c_int)]

    def extractFeature(self, cloud_xyzi):
        a = np.ascontiguousarray(cloud_xyzi, dtype=np.float32)
        assert a.ndim == 2 and a.shape[1] == 4
        n = len(a)
        fp = C.POINTER(C.c_float)
        e = np.zeros((max(n, 1), 4), dtype=np.float32); s = np.zeros((max(n, 1), 4), dtype=np.float32)
        ne, ns = C.c_int(0), C.c_int(0)
        self.s._check(self._L.vilf_lidar_extract_features(self.s._h, a.ctypes.data_as(fp), n, self.n_scans, self.min_range, self.max_range, self.edge_threshold,
                                                          e.ctypes.data_as(fp), n, C.byref(ne), s.ctypes.data_as(fp), n, C.byref(ns)), "vilf_lidar_extract_features")
        return e[:ne.value].copy(), s[:ns.value].copy()

    def getFeatureDepth(self, depth_cloud_xyzi, features_xyz):
        """≙ getFeatureDepth (feature_tracker_node.cpp:54-163): LiDAR depth per visual feature, -1 = none"""
        c = np.ascontiguousarray(depth_cloud_xyzi, dtype=np.float32); f = np.ascontiguousarray(features_xyz, dtype=np.float32)
        assert c.ndim == 2 and c.shape[1] == 4 and f.ndim == 2 and f.shape[1] == 3
        fp = C.POINTER(C.c_float)
        self._L.vilf_feature_depth.argtypes = [C.c_void_p, fp, C.c_int, fp, C.c_int, fp]
        out = np.zeros(max(len(f), 1), dtype=np.float32)
        self.s._check(self._L.vilf_feature_depth(self.s._h, c.ctypes.data_as(fp), len(c), f.ctypes.data_as(fp), len(f), out.ctypes.data_as(fp)), "vilf_feature_depth")
        return out[:len(f)].copy()


TRACK_STAGES = ("pyramid", "lk", "set_mask", "detect", "undistort")


class FeatureTracker:
    """Host mirror of FeatureTracker (feature_tracker/feature_tracker.cpp) over the device tracker of a BackendSolver handle (vilf_track_*): the camera half of the
    feature-tracker node. Images are (height, width) uint8 arrays; camera = (fx, fy, cx, cy, k1, k2, p1, p2). The arithmetic is the contract in include/vilfusion.h.
    equalize = True puts CLAHE (clahe = (clip, tiles_x, tiles_y)) in front of everything; f_threshold = a number of pixels turns rejectWithF on (focal_length,
    n_hypotheses, seed). With both at their defaults the tracker is never configured and runs as it did before these steps existed.
    readImage_mask is the front-end of the second node (feature_tracker_node_mask.cpp): a mask image marks dynamic objects (0 = dynamic); configure_mask sets its
    parameters, set_fisheye_mask the fixed image that setMask and the detection of both readImage variants start from."""

    def __init__(self, solver, width, height, camera, max_cnt=200, min_dist=20, equalize=False, f_threshold=None, focal_length=460.0, clahe=(3.0, 8, 8),
                 n_hypotheses=512, seed=0):
        self.s, self._L = solver, solver._L
        self.width, self.height, self.max_cnt, self.min_dist = int(width), int(height), int(max_cnt), int(min_dist)
        self.camera = tuple(float(v) for v in camera)
        assert len(self.camera) == 8, "camera = (fx, fy, cx, cy, k1, k2, p1, p2)"
        self.params = abi.TrackParams(self.width, self.height, self.max_cnt, self.min_dist, *self.camera)
        self.s._check(self._L.vilf_track_init(self.s._h, C.byref(self.params)), "vilf_track_init")
        self.frontend = abi.TrackFrontend(int(bool(equalize)), float(clahe[0]), int(clahe[1]), int(clahe[2]), int(f_threshold is not None),
                                          1.0 if f_threshold is None else float(f_threshold), float(focal_length), int(n_hypotheses), int(seed))
        if (bool(equalize), f_threshold, float(focal_length), tuple(clahe), int(n_hypotheses), int(seed)) != (False, None, 460.0, (3.0, 8, 8), 512, 0):
            self.s._check(self._L.vilf_track_configure(self.s._h, C.byref(self.frontend)), "vilf_track_configure")
        self.mask_params = abi.TrackMaskParams(5, 5, 1, 0.1, 1.0)          # the defaults of vilf_track_init
        self._clear()

    def _clear(self):
        self.ids, self.track_cnt = np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
        self.cur_pts, self.cur_un_pts, self.pts_velocity = (np.zeros((0, 2), dtype=np.float32) for _ in range(3))

    def _img(self, img):
        a = np.asarray(img)
        assert a.dtype == np.uint8 and a.ndim == 2 and a.shape == (self.height, self.width) and a.strides[1] == 1 and a.strides[0] >= self.width, (a.dtype, a.shape, a.strides)
        return a

    @staticmethod
    def _u8(a):
        return a.ctypes.data_as(C.POINTER(C.c_uint8))

    @staticmethod
    def _fp(a):
        return a.ctypes.data_as(C.POINTER(C.c_float))

    def reset(self):
        """a fresh FeatureTracker: no points, no previous image, n_id = 0"""
        self.s._check(self._L.vilf_track_reset(self.s._h), "vilf_track_reset")
        self._clear()

    def readImage(self, img, stamp):
        """:119-209 and the updateID loop (feature_tracker_node.cpp:285-292). A row stride larger than the width is passed on as it is. Returns the number of points."""
        a = self._img(img)
        n = C.c_int(0)
        self.s._check(self._L.vilf_track_read_image(self.s._h, self._u8(a), int(a.strides[0]), float(stamp), C.byref(n)), "vilf_track_read_image")
        return self._fetch(n)

    def readImage_mask(self, img, mask, stamp):
        """:212-381: readImage under a mask image of dynamic objects (0 = dynamic, anything else = static). Returns the number of points."""
        a, m = self._img(img), self._img(mask)
        n = C.c_int(0)
        self.s._check(self._L.vilf_track_read_image_mask(self.s._h, self._u8(a), int(a.strides[0]), self._u8(m), int(m.strides[0]), float(stamp), C.byref(n)), "vilf_track_read_image_mask")
        return self._fetch(n)

    def _fetch(self, n):
        m = max(n.value, 1)
        ids, cnt = np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int32)
        pts, un, vel = (np.zeros((m, 2), dtype=np.float32) for _ in range(3))
        ip = C.POINTER(C.c_int)
        self.s._check(self._L.vilf_track_get(self.s._h, m, ids.ctypes.data_as(ip), cnt.ctypes.data_as(ip), self._fp(pts), self._fp(un), self._fp(vel), C.byref(n)), "vilf_track_get")
        k = n.value
        self.ids, self.track_cnt, self.cur_pts, self.cur_un_pts, self.pts_velocity = ids[:k], cnt[:k], pts[:k], un[:k], vel[:k]
        return k

    def pyramid(self, img, level):
        """level `level` (0 .. Lmax) of the image's pyramid"""
        a = self._img(img)
        w, h = self.width, self.height
        for _ in range(int(level)):
            w, h = (w + 1) // 2, (h + 1) // 2
        out = np.zeros((h, w), dtype=np.uint8)
        self.s._check(self._L.vilf_track_pyramid(self.s._h, self._u8(a), int(a.strides[0]), int(level), self._u8(out)), "vilf_track_pyramid")
        return out

    def lk(self, img_prev, img_next, pts):
        """calcOpticalFlowPyrLK between two images -> (points (n, 2) float32, status (n,) uint8), without inBorder"""
        a, b = np.ascontiguousarray(self._img(img_prev)), np.ascontiguousarray(self._img(img_next))
        p = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 2)
        out, st = np.zeros((max(len(p), 1), 2), dtype=np.float32), np.zeros(max(len(p), 1), dtype=np.uint8)
        self.s._check(self._L.vilf_track_lk(self.s._h, self._u8(a), self._u8(b), self._fp(p), len(p), self._fp(out), self._u8(st)), "vilf_track_lk")
        return out[:len(p)], st[:len(p)]

    def detect(self, img, kept_pts, n_max):
        """goodFeaturesToTrack under the mask of the kept points -> new corners (n, 2) float32 in acceptance order"""
        a = np.ascontiguousarray(self._img(img))
        kp = np.ascontiguousarray(kept_pts, dtype=np.float32).reshape(-1, 2)
        out = np.zeros((max(int(n_max), 1), 2), dtype=np.float32)
        n = C.c_int(0)
        self.s._check(self._L.vilf_track_detect(self.s._h, self._u8(a), self._fp(kp), len(kp), int(n_max), self._fp(out), C.byref(n)), "vilf_track_detect")
        return out[:n.value].copy()

    def clahe(self, img):
        """CLAHE of an image with the configured clip and tiles (stateless)"""
        a = self._img(img)
        out = np.zeros((self.height, self.width), dtype=np.uint8)
        self.s._check(self._L.vilf_track_clahe(self.s._h, self._u8(a), int(a.strides[0]), self._u8(out)), "vilf_track_clahe")
        return out

    def reject_f(self, cur_pts, forw_pts):
        """rejectWithF on point pairs (stateless) -> (status (n,) uint8, best, n_inliers, F (9,) float64); best = -1: nothing rejected"""
        a, b = (np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 2) for p in (cur_pts, forw_pts))
        assert len(a) == len(b)
        st, F = np.zeros(max(len(a), 1), dtype=np.uint8), np.zeros(9)
        best, n_in = C.c_int(0), C.c_int(0)
        self.s._check(self._L.vilf_track_reject_f(self.s._h, self._fp(a), self._fp(b), len(a), self._u8(st), abi.dptr(F), C.byref(best), C.byref(n_in)), "vilf_track_reject_f")
        return st[:len(a)], best.value, n_in.value, F

    def configure_mask(self, erode_radius=5, probe=5, reject=True, f_threshold=0.1, epi_threshold=1.0):
        """the parameters of readImage_mask: the erosion radius, the probe distance, rejectWithF_mask on / off and its two thresholds"""
        mp = abi.TrackMaskParams(int(erode_radius), int(probe), int(bool(reject)), float(f_threshold), float(epi_threshold))
        self.s._check(self._L.vilf_track_configure_mask(self.s._h, C.byref(mp)), "vilf_track_configure_mask")
        self.mask_params = mp

    def set_fisheye_mask(self, mask):
        """the fisheye mask (None: none): setMask keeps a point only where it is 255, the detection finds corners only where it is not 0"""
        if mask is None:
            self.s._check(self._L.vilf_track_set_fisheye_mask(self.s._h, None, 0), "vilf_track_set_fisheye_mask")
            return
        m = self._img(mask)
        self.s._check(self._L.vilf_track_set_fisheye_mask(self.s._h, self._u8(m), int(m.strides[0])), "vilf_track_set_fisheye_mask")

    def erode(self, mask):
        """the erosion of a mask image with the configured radius (stateless) -> (height, width) uint8, 255 or 0"""
        m = self._img(mask)
        out = np.zeros((self.height, self.width), dtype=np.uint8)
        self.s._check(self._L.vilf_track_erode(self.s._h, self._u8(m), int(m.strides[0]), self._u8(out)), "vilf_track_erode")
        return out

    def probe(self, eroded, pts):
        """the probe of points in an eroded mask with the configured distance (stateless) -> (n,) uint8, 1 = static"""
        e = np.ascontiguousarray(self._img(eroded))
        p = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 2)
        st = np.zeros(max(len(p), 1), dtype=np.uint8)
        self.s._check(self._L.vilf_track_probe(self.s._h, self._u8(e), self._fp(p), len(p), self._u8(st)), "vilf_track_probe")
        return st[:len(p)]

    def reject_f_mask(self, cur_pts, forw_pts, is_static):
        """rejectWithF_mask on point pairs (stateless) -> (status (n,) uint8, best, n_static_inliers, F (9,) float64); best = -1: nothing rejected"""
        a, b = (np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 2) for p in (cur_pts, forw_pts))
        s = np.ascontiguousarray(np.asarray(is_static) != 0, dtype=np.uint8).reshape(-1)
        assert len(a) == len(b) == len(s)
        if len(s) == 0:
            s = np.zeros(1, dtype=np.uint8)
        st, F = np.zeros(max(len(a), 1), dtype=np.uint8), np.zeros(9)
        best, n_in = C.c_int(0), C.c_int(0)
        self.s._check(self._L.vilf_track_reject_f_mask(self.s._h, self._fp(a), self._fp(b), self._u8(s), len(a), self._u8(st), abi.dptr(F), C.byref(best), C.byref(n_in)),
                      "vilf_track_reject_f_mask")
        return st[:len(a)], best.value, n_in.value, F

    def detect_masked(self, img, eroded, kept_pts, n_max):
        """detect() under an eroded mask as well: corners only where it is not 0"""
        a, e = np.ascontiguousarray(self._img(img)), np.ascontiguousarray(self._img(eroded))
        kp = np.ascontiguousarray(kept_pts, dtype=np.float32).reshape(-1, 2)
        out = np.zeros((max(int(n_max), 1), 2), dtype=np.float32)
        n = C.c_int(0)
        self.s._check(self._L.vilf_track_detect_masked(self.s._h, self._u8(a), self._u8(e), self._fp(kp), len(kp), int(n_max), self._fp(out), C.byref(n)), "vilf_track_detect_masked")
        return out[:n.value].copy()

    def profile_mask(self):
        """ms and launches of the erosion and of the probe with rejectWithF_mask in the last readImage_mask (vilf_set_profiling)"""
        ms, cnt = (C.c_double * 2)(), (C.c_long * 2)()
        self.s._check(self._L.vilf_track_profile_mask(self.s._h, ms, cnt), "vilf_track_profile_mask")
        return {"erode": (ms[0], cnt[0]), "probe_reject": (ms[1], cnt[1])}

    def profile_frontend(self):
        """ms and launches of CLAHE and rejectWithF in the last readImage (vilf_set_profiling)"""
        ms, cnt = (C.c_double * 2)(), (C.c_long * 2)()
        self.s._check(self._L.vilf_track_profile_frontend(self.s._h, ms, cnt), "vilf_track_profile_frontend")
        return {"clahe": (ms[0], cnt[0]), "reject_f": (ms[1], cnt[1])}

    def feature_message(self, depths=None):
        """the rows with track_cnt > 1 as {id: (x, y, 1, u, v, vx, vy, depth)} (feature_tracker_node.cpp:311-336): what SlidingWindowEstimator.process_image takes.
        depths: one value per such row, as FeatureExtraction.getFeatureDepth returns for message_points(); None = no LiDAR depth (-1)"""
        rows = np.flatnonzero(self.track_cnt > 1)
        assert depths is None or len(depths) == len(rows)
        return {int(self.ids[i]): (float(self.cur_un_pts[i, 0]), float(self.cur_un_pts[i, 1]), 1.0, float(self.cur_pts[i, 0]), float(self.cur_pts[i, 1]),
                                   float(self.pts_velocity[i, 0]), float(self.pts_velocity[i, 1]), -1.0 if depths is None else float(depths[k]))
                for k, i in enumerate(rows)}

    def message_points(self):
        """(x, y, 1) of the rows feature_message() publishes, (m, 3) float32: the features_xyz of FeatureExtraction.getFeatureDepth"""
        rows = np.flatnonzero(self.track_cnt > 1)
        return np.concatenate([self.cur_un_pts[rows], np.ones((len(rows), 1), dtype=np.float32)], axis=1)

    def profile(self):
        """ms and launches of the stages of the last readImage (vilf_set_profiling)"""
        ms, cnt = (C.c_double * 5)(), (C.c_long * 5)()
        self.s._check(self._L.vilf_track_profile(self.s._h, ms, cnt), "vilf_track_profile")
        return dict(zip(TRACK_STAGES, ((ms[i], cnt[i]) for i in range(5))))
