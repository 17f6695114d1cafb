/*
 * vilfusion.h — C ABI of the MI355X-native sliding-window back-end for VIL_Fusion.
 *
 * Drop-in boundary for ONE hot path of RichExplor/VIL_Fusion (reference paths are relative to
 * src/visual_inertial_lidar/):
 *   - Estimator::optimization()            vins_estimator/estimator.cpp:689-1050
 *   - MarginalizationInfo                  vins_estimator/factor/marginalization_factor.{h,cpp}
 *   - EstimationMapping::optimation_processing   feature_tracker/include/EstimationMapping.hpp:235-296
 *
 * Plain C: POD structs, caller-owned host buffers, library-owned device state, int status codes,
 * never throws / never aborts (reference error convention: Evaluate() always returns true, solver
 * failures are not checked — estimator.cpp:852-855).
 *
 * Memory-layout conventions are the reference's:
 *   pose block   [tx ty tz qx qy qz qw]            (estimator.cpp:509-516)
 *   speed-bias   [vx vy vz bax bay baz bgx bgy bgz] (estimator.cpp:518-528)
 *   quaternions in structs: x y z w   (Eigen coeffs order)
 *   matrices: row-major
 *   scan-to-map pose [qx qy qz qw tx ty tz]        (EstimationMapping.hpp:383-385)
 *
 * Parameter-block ids replace the reference's address keys (marginalization_factor.h:59-62):
 *   Pose[i] -> i,  SpeedBias[i] -> NF+i,  Ex_Pose -> 2NF,  Td -> 2NF+1,  Feature[k] -> 2NF+2+k
 * with NF = window_size+1 frames.
 */
#ifndef VILFUSION_H
#define VILFUSION_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VILF_MAX_FRAMES 11         /* WINDOW_SIZE + 1, vins_estimator/parameters.h:24 */
#define VILF_MAX_FEATURES 1000     /* NUM_OF_F, parameters.h:26 */
#define VILF_PRIOR_MAX_DIM 160     /* 10 poses*6 + 10 speedbias*9 + ex 6 + td 1 = 157 */
#define VILF_PRIOR_MAX_BLOCKS 24

/* status codes */
#define VILF_OK 0
#define VILF_ERR_INVALID_ARGUMENT (-1)
#define VILF_ERR_DEVICE (-2)
#define VILF_ERR_UNSUPPORTED (-3)
#define VILF_ERR_NO_GPU (-4)
#define VILF_SOLVER_ABNORMAL 1     /* >0: solver terminated abnormally (summary tells why) */

/* marginalization_flag, estimator.h:63-67 */
#define VILF_MARGIN_OLD 0
#define VILF_MARGIN_SECOND_NEW 1

/* termination types (mirrors ceres::TerminationType semantics for the configured minimizer) */
#define VILF_TERM_NO_CONVERGENCE 0    /* max_num_iterations reached */
#define VILF_TERM_CONVERGENCE_FUNCTION 1
#define VILF_TERM_CONVERGENCE_PARAMETER 2
#define VILF_TERM_CONVERGENCE_GRADIENT 3
#define VILF_TERM_FAILURE 4           /* too many invalid steps / min radius */

typedef struct vilf_handle vilf_handle;

/* Options ≙ the globals read by readParameters() (vins_estimator/parameters.cpp:45-155) plus the
 * solver options set in estimator.cpp:838-850. */
typedef struct vilf_options {
    int window_size;          /* WINDOW_SIZE = 10 */
    int max_num_iterations;   /* NUM_ITERATIONS = 8 (kitti_config.yaml:74) */
    double max_solver_time;   /* SOLVER_TIME seconds (estimator.cpp:847-850); <= 0 disables the wall-clock limit (parity runs). When > 0 the
                               * solve tests the host clock at the top of every iteration, as Ceres does; windows whose marginalization_flag is
                               * VILF_MARGIN_OLD get 4/5 of it (the factor the reference applies). A stopped window reports VILF_TERM_NO_CONVERGENCE
                               * and keeps its last accepted state. The batched solve then waits for the stream once per iteration. */
    double focal_length;      /* FOCAL_LENGTH = 460; sqrt_info = focal/1.5 * I2 (estimator.cpp:17) */
    double cauchy_a;          /* CauchyLoss(1.0) (estimator.cpp:694) */
    double G[3];              /* global G (parameters.cpp:14,77) */
    int estimate_extrinsic;   /* ESTIMATE_EXTRINSIC */
    int estimate_td;          /* ESTIMATE_TD */
    int use_lidar_const;      /* #define USE_LIDAR_CONST (parameters.h:56) */
    double RIC[9], TIC[3];    /* imu^R_cam, imu^T_cam   (globals used by lidarFactor) */
    double RCL[9], TCL[3];    /* cam^R_lidar, cam^T_lidar */
    double TR, ROW;           /* rolling shutter read-out time, image rows */
    double init_depth;        /* INIT_DEPTH = 5.0 (parameters.cpp:132), feature_manager.cpp:205-208 */
    /* scan-to-map (velodyne_param_64.yaml:22-23, EstimationMapping.hpp:263,277,327) */
    double edge_leaf_size;    /* 0.4 */
    double surf_leaf_size;    /* 0.8 */
    double huber_a;           /* 0.1 */
    int s2m_outer_iterations; /* 2 */
    int s2m_max_iterations;   /* 4 */
    double s2m_crop_half;     /* 100.0 */
} vilf_options;

/* IntegrationBase state consumed by IMUFactor (factor/integration_base.h:188-207) */
typedef struct vilf_imu_preint {
    double sum_dt;
    double delta_p[3];
    double delta_q[4];        /* x y z w */
    double delta_v[3];
    double linearized_ba[3];
    double linearized_bg[3];
    double jacobian[225];     /* 15x15 row-major */
    double covariance[225];   /* 15x15 row-major */
} vilf_imu_preint;

/* lidarConstraintsBase (factor/lidarConstraint_base.h:24-25) */
typedef struct vilf_lidar_constraint {
    double q[4];              /* x y z w */
    double t[3];
} vilf_lidar_constraint;

/* One window ≙ the members optimization() reads (estimator.h:70-146). */
typedef struct vilf_window_in {
    int n_frames;                         /* options.window_size + 1. 11 = the reference's WINDOW_SIZE: batched LDS kernels; any other size: the general
                                             path (vilf_window_solve, or several at once: vilf_window_solve_group; no prior, no marginalization) —
                                             BASELINE configs[4].
                                             options.estimate_extrinsic / estimate_td (para_ex_pose / para_td become variables; obs_velocity,
                                             obs_cur_td, obs_row required for td): solved through the same general path at any window size, by
                                             vilf_window_solve and by vilf_batch_solve (all slots side by side as one group); an 11-frame window keeps its device
                                             prior, and vilf_window_marginalize() / vilf_batch_marginalize() carry Ex_Pose and Td as kept blocks
                                             of it (ProjectionTdFactor rows when estimate_td is set). */
    const double *para_pose;              /* [n_frames][7] */
    const double *para_speed_bias;        /* [n_frames][9] */
    double para_ex_pose[7];
    double para_td;
    int n_features;                       /* f_manager.getFeatureCount() */
    const double *para_feature;           /* [n_features] inverse depth (feature_manager.cpp:194-216) */
    const uint8_t *feature_const;         /* [n_features] lidar_depth_flag (estimator.cpp:780,789) */
    const int32_t *feature_start_frame;   /* [n_features] */
    const int32_t *feature_obs_offset;    /* [n_features+1] CSR into obs_*; obs k of a feature is in frame start+k */
    int n_obs;
    const double *obs_point;              /* [n_obs][3] feature_per_frame[k].point */
    const double *obs_velocity;           /* [n_obs][2] or NULL (td factor only) */
    const double *obs_cur_td;             /* [n_obs]    or NULL */
    const double *obs_row;                /* [n_obs] uv.y() or NULL */
    const vilf_imu_preint *imu;           /* [n_frames]; entry j = pre_integrations[j], j >= 1 used */
    const vilf_lidar_constraint *lidar;   /* [n_frames]; entry j = lidarConstraints[j], j >= 1 used; may be NULL if !use_lidar_const */
    int marginalization_flag;
    const double *gauge_R0;               /* optional Rs[0] (9, row-major) override for double2vector (failure_occur path); NULL: from para_pose[0] */
    const double *gauge_P0;               /* optional Ps[0] override; NULL: from para_pose[0] */
} vilf_window_in;

typedef struct vilf_summary {
    int num_iterations;        /* trust-region iterations executed (excluding iteration 0) */
    int num_successful_steps;
    int num_linear_solves;     /* dense Schur solves (rejected steps re-use the previous one) */
    int termination;           /* VILF_TERM_* */
    double initial_cost;
    double final_cost;
    double final_radius;
    double usec_solve;         /* wall time spent in the solve, microseconds */
} vilf_summary;

/* State after Solve + double2vector() (estimator.cpp:549-638). Caller-owned buffers. */
typedef struct vilf_window_out {
    double *para_pose;         /* [n_frames][7]   raw solver output (before gauge fix); may be NULL */
    double *para_speed_bias;   /* [n_frames][9]   may be NULL */
    double *para_feature;      /* [n_features]    may be NULL */
    double *Ps;                /* [n_frames][3] */
    double *Rs;                /* [n_frames][9] */
    double *Vs;                /* [n_frames][3] */
    double *Bas;               /* [n_frames][3] */
    double *Bgs;               /* [n_frames][3] */
    double tic[3], ric[9];
    double td;
    vilf_summary summary;
} vilf_window_out;

/* Marginalization prior ≙ MarginalizationInfo after marginalize()+getParameterBlocks()
 * (marginalization_factor.h:58-70). Block ids are already shifted (estimator.cpp:960-971). */
typedef struct vilf_prior {
    int valid;
    int n;                                       /* rows = kept local dimension */
    int m;                                       /* marginalized local dimension (informative) */
    int n_blocks;
    int block_id[VILF_PRIOR_MAX_BLOCKS];
    int block_size[VILF_PRIOR_MAX_BLOCKS];       /* global size (7 / 9 / 1) */
    int block_idx[VILF_PRIOR_MAX_BLOCKS];        /* local column offset = keep_block_idx - m */
    double block_x0[VILF_PRIOR_MAX_BLOCKS][9];   /* keep_block_data */
    double linearized_residuals[VILF_PRIOR_MAX_DIM];
    double linearized_jacobians[VILF_PRIOR_MAX_DIM * VILF_PRIOR_MAX_DIM]; /* n x n row-major, leading dim n */
} vilf_prior;

/* ---- lifecycle ------------------------------------------------------------------------- */
void vilf_default_options(vilf_options *opts);                 /* KITTI config values */
/* hip_stream: a hipStream_t (as void*) all work is enqueued on, or NULL for the library's own stream. */
int vilf_create(const vilf_options *opts, int device, void *hip_stream, vilf_handle **out);
void vilf_destroy(vilf_handle *h);
int vilf_reset(vilf_handle *h);                                /* drop priors ≙ clearState(), estimator.cpp:72-77 */
const char *vilf_last_error(const vilf_handle *h);
const char *vilf_version(void);

/* ---- single-window drop-in (≙ Estimator::optimization()) ------------------------------- */
/* estimator.cpp:689-860: build problem, Solve, double2vector. Uses/keeps the prior of slot 0. */
int vilf_window_solve(vilf_handle *h, const vilf_window_in *in, vilf_window_out *out);
/* n independent windows of sizes other than 11 frames (the general path), solved side by side in ONE chain of launches: a window's chain is ~32 small dependent
 * launches per iteration, so a group fills the chip where a single window (or one handle / stream per window) cannot. in / out: arrays of n; every out[i] needs
 * Ps / Rs / Vs / Bas / Bgs. Same results as n calls of vilf_window_solve, bit for bit (no reduction on this path depends on the order in which workgroups finish; with
 * options.estimate_extrinsic / estimate_td: to the rounding of the remaining atomics). 11-frame windows:
 * VILF_ERR_UNSUPPORTED (use vilf_batch_*). Returns VILF_SOLVER_ABNORMAL if any window terminated abnormally (its summary tells). */
int vilf_window_solve_group(vilf_handle *h, int n, const vilf_window_in *in, vilf_window_out *out);
/* estimator.cpp:863-1046: marginalization of the just-solved window (slot 0); new prior stays on device. */
int vilf_window_marginalize(vilf_handle *h);

/* ---- batched windows (independent window snapshots resident in HBM) -------------------- */
/* Pack + upload n windows into slots 0..n-1 (inputs stay resident until the next upload). */
int vilf_batch_upload(vilf_handle *h, int n_windows, const vilf_window_in *wins);
/* Solve every resident window from its resident state (all kernels enqueued on the handle's stream). sync!=0 waits; with sync == 0 the usec_solve of the summaries
 * is filled by the next call that waits for the stream (vilf_batch_summaries / vilf_batch_download_states). Returns VILF_OK also when single windows terminated
 * abnormally: their summaries tell (termination = VILF_TERM_FAILURE). options.estimate_extrinsic / estimate_td: all slots run through the general path as ONE group
 * of launches (vilf_window_solve_group's machinery, each slot with its device-resident prior); that path reads its results back, so the call is always synchronous.
 * options.max_solver_time > 0: ONE host clock for the whole batch, started by this call (the windows of a batch run in lockstep), and a stream wait per iteration. */
int vilf_batch_solve(vilf_handle *h, int sync);
/* Re-arm the resident windows with their uploaded initial state (bench loop: repeated identical steps). */
int vilf_batch_rewind(vilf_handle *h);
int vilf_batch_marginalize(vilf_handle *h, int sync);
int vilf_batch_download(vilf_handle *h, int first, int n_windows, vilf_window_out *outs);
int vilf_batch_summaries(vilf_handle *h, int first, int n_windows, vilf_summary *sums);
/* the estimator's outputs only (double2vector(): Ps [n][33], Rs [n][99] row-major, Vs, Bas, Bgs [n][33]) and the summaries into contiguous caller arrays;
 * any pointer may be NULL. The per-frame caller's download: the parameter arrays stay on the device for the marginalization. */
int vilf_batch_download_states(vilf_handle *h, int first, int n_windows, double *Ps, double *Rs, double *Vs, double *Bas, double *Bgs, vilf_summary *sums);
int vilf_synchronize(vilf_handle *h);
/* Work enqueued on h's stream after this call starts once everything enqueued on other's stream so far has finished — a dependency on the device
 * (hipEventRecord + hipStreamWaitEvent), the host does not wait. The reference runs the LiDAR node and the estimator node side by side and hands
 * lidarConstraints across (feature_tracker_node.cpp:384,524 -> estimator.cpp:689-860); with one handle per stage this orders a frame's two stages
 * without a host round trip between them. Both handles must be on the same device. */
int vilf_wait_for(vilf_handle *h, vilf_handle *other);
/* on != 0: vilf_batch_upload returns as soon as its copies and set-up launches are enqueued instead of waiting for them (the caller's window structs are
 * consumed while the call packs them, as before; the library's pinned staging is protected by a wait at the start of the handle's NEXT upload). Everything
 * that follows on the handle is ordered behind the copies on its stream. For streams of batches over two handles: while one handle's copies and solve
 * (vilf_batch_solve with sync == 0) are on the device, the host packs the other handle's next batch — bench.py: pcie_inclusive.stream_of_batches. Default: off. */
int vilf_set_async_upload(vilf_handle *h, int on);
/* per-kernel timing by HIP events on the handle's stream (kind 0 linearize incl. the trust-region step, 1 reduce+solve, 2 the step-only launch that ends a solve, 3 other).
 * With sync == 0 calls the spans stay pending and are read by the next call that waits for the stream (a sync call, vilf_batch_summaries, vilf_get_profile*). */
int vilf_set_profiling(vilf_handle *h, int on);
int vilf_get_profile(vilf_handle *h, double ms_out[4], long launches_out[4]);
/* same switch, scan-to-map launches by group: 0 voxel grid of the scan clouds, 1 radix sort, 2 neighbour index, 3 associate (5-NN + fits),
 * 4 LM solve, 5 sub-map maintenance, 6 other, 7 fused local-map update (crop + merge + voxel grid + directory) */
int vilf_get_profile_scan2map(vilf_handle *h, double ms_out[8], long launches_out[8]);
/* same switch, marginalization kernels: 0 prepare (factor re-evaluation at the linearisation point), 1 Schur complement, 2 eigen + prior, 3 prior H/g */
int vilf_get_profile_marginalize(vilf_handle *h, double ms_out[4], long launches_out[4]);
/* Which form the last vilf_batch_marginalize() / vilf_window_marginalize() took per window. marginalization_factor.cpp:267-291 eigen-decomposes the dropped
 * block Amm and the kept block with a 1e-8 truncation; where that truncation provably removes nothing (positive Cholesky pivots and trace(A^-1) < 1e8, i.e.
 * lambda_min > 1e-8) the library uses Cholesky factors instead — same J0^T J0, J0^T r0, |r0|^2 — and falls back to the eigen-decompositions otherwise.
 * counts[0] windows that produced a new prior; [1] of those: Amm by the arrow Cholesky; [2] of those: kept block by Cholesky (J0 = L^T, r0 = L^-1 b);
 * [3] windows whose prior was left as it was. */
int vilf_batch_marginalize_stats(vilf_handle *h, int counts[4]);
/* the general (window_size != 10) path of vilf_window_solve: factor scatter (linearisations), Schur SYRK, Cholesky, unused */
int vilf_get_profile_large_window(vilf_handle *h, double ms_out[4], long launches_out[4]);
/* newest-frame pose per resident window: [stamp x y z qx qy qz qw] (8 doubles each) into a DEVICE buffer
 * (feeds the RCCL gather for global_fusion, poseGraphOptimization.cpp:116-121). Enqueued on the handle's stream; the call does NOT wait for it (stamps_host is
 * copied to a pinned staging buffer of the handle before the call returns): order a consumer behind it by using the same stream (vilf_gather_poses takes one) or
 * vilf_synchronize(). */
int vilf_batch_newest_poses_device(vilf_handle *h, const double *stamps_host, void *device_out8);

/* ---- multi-GPU: the pose gather over RCCL (SURVEY.md §8(b),(e)) --------------------------- */
/* Independent windows / sequence segments shard over the GPUs of a node, one process and one vilf_handle per GPU, no intra-solve
 * communication. The only exchange is an all-gather of the newest-frame pose rows above — what global_fusion subscribes to as
 * nav_msgs/Odometry (src/global_fusion/poseGraphOptimization.cpp:116-121: position, quaternion, stamp). The communicator is RCCL
 * (ncclCommInitRank / ncclAllGather over xGMI); the launcher distributes rank 0's id (MPI, a file, a ROS parameter ...). */
#define VILF_COMM_ID_BYTES 128
typedef struct vilf_comm vilf_comm;
int vilf_comm_unique_id(unsigned char id[VILF_COMM_ID_BYTES]);                       /* rank 0: ncclGetUniqueId */
int vilf_comm_create(const unsigned char id[VILF_COMM_ID_BYTES], int world_size, int rank, int device, vilf_comm **out);
int vilf_comm_destroy(vilf_comm *comm);
/* local_dev8: n_local rows of 8 doubles on this rank's device; out_dev8: world_size * n_local rows, rank-major (= the global unit order
 * under contiguous sharding). Enqueued on hip_stream (NULL: default stream); the caller synchronises. Every rank passes the same n_local. */
int vilf_gather_poses(vilf_comm *comm, void *hip_stream, const double *local_dev8, int n_local, double *out_dev8);
/* The same gather enqueued on the stream h works on — whichever that is: the one handed to vilf_create, or the library's own. The library's own stream is
 * NON-BLOCKING: it does not synchronise with the default (NULL) stream, so a gather enqueued on NULL is NOT ordered behind vilf_batch_newest_poses_device /
 * an asynchronous vilf_batch_solve of such a handle. This entry point is: it runs behind everything enqueued on h so far. local_dev8 / out_dev8 must be
 * ready (allocated and, for local_dev8, written by work on h's stream or synchronised) when the call is made. */
int vilf_gather_poses_handle(vilf_comm *comm, vilf_handle *h, const double *local_dev8, int n_local, double *out_dev8);
/* ranks of the communicator as RCCL reports them (ncclCommCount) and this process's rank in it (ncclCommUserRank) */
int vilf_comm_ranks(vilf_comm *comm, int *world_size_out, int *rank_out);
/* the hipStream_t (as void*) h enqueues its work on */
int vilf_get_stream(vilf_handle *h, void **hip_stream_out);
const char *vilf_comm_last_error(void);

/* ---- prior import / export (tests, snapshots) ------------------------------------------ */
int vilf_prior_export(vilf_handle *h, int slot, vilf_prior *out);
int vilf_prior_import(vilf_handle *h, int slot, const vilf_prior *prior);

/* ---- fine-grained hooks in the reference's Ceres layout -------------------------------- */
/* bool Evaluate(double const *const *parameters, double *residuals, double **jacobians): row-major
 * jacobians in GLOBAL size (pose: 7 columns, last = 0); jacobians / jacobians[i] may be NULL. All run on
 * the device through the same device functions the solve kernels use. */
int vilf_eval_projection(vilf_handle *h, const double *const *parameters, const double pts_i[3],
                         const double pts_j[3], double *residuals, double **jacobians);   /* projection_factor.cpp:21 */
/* ProjectionTdFactor (5 blocks: Pose_i, Pose_j, Ex_Pose, inverse depth, td); row_* = uv.y of the two observations, TR / ROW from the options.
 * In the solve: options.estimate_td = 1 makes vilf_window_solve use this factor for every visual observation and td a variable
 * (estimator.cpp:713-717, 765-777); see vilf_window_solve. */
int vilf_eval_projection_td(vilf_handle *h, const double *const *parameters, const double pts_i[3], const double pts_j[3],
                            const double velocity_i[2], const double velocity_j[2], double td_i, double td_j, double row_i, double row_j,
                            double *residuals, double **jacobians);                          /* projection_td_factor.cpp:34 */
/* IMUFactor::Evaluate. Contract of the inputs, for vilf_eval_imu, vilf_eval_imu_raw and the IMU factors of a window alike: the quaternions of the
 * two poses are unit to within rounding, as Ceres delivers them after the local parameterization (a quaternion is inverted as the reference inverts
 * it, conjugate / squaredNorm, and rotates as Eigen's does; nothing is re-normalised and no sign is flipped: q and -q give residuals of opposite
 * sign in the rotation rows, a residual rotation past 180 degrees is taken as it comes). pre->covariance must have an inverse. It has none for an
 * interval of no samples or with zero noise (the covariance is exactly zero) and for an interval of ONE sample (integration_base.h:109-118: the position
 * rows of V are dt / 2 times its velocity rows, rank 12). sqrt_info of such a covariance is not defined: no error is returned, the 15 fixed elimination
 * steps run, and the entries are not finite or not meaningful (an all-zero covariance gives NaN in the whole upper triangle), as are the whitened
 * residual and Jacobians; the parts before sqrt_info (vilf_eval_imu_raw's residuals and jacobians) do not depend on it. */
int vilf_eval_imu(vilf_handle *h, const double *const *parameters, const vilf_imu_preint *pre,
                  double *residuals, double **jacobians);                                   /* imu_factor.h:19 */
/* the two parts of that product on their own (test hook): residuals / jacobians BEFORE the multiplication by sqrt_info (imu_factor.h:60-62, 86-173 without the
 * sqrt_info * ... lines), same layouts, and sqrt_info = LLT(covariance^-1).matrixL()^T (:64) as the device computes it once per upload; any output may be NULL. */
int vilf_eval_imu_raw(vilf_handle *h, const double *const *parameters, const vilf_imu_preint *pre,
                      double *residuals, double **jacobians, double *sqrt_info225);
int vilf_eval_lidar_between(vilf_handle *h, const double *const *parameters,
                            const vilf_lidar_constraint *c, double *residuals, double **jacobians); /* lidar_factor.h:19 */
/* prior must be valid with 1 <= n <= VILF_PRIOR_MAX_DIM and 1 <= n_blocks <= VILF_PRIOR_MAX_BLOCKS, and its block table is checked as vilf_prior_import checks
 * it: every block_size 7, 9 or 1, block_id >= 0, block_idx >= 0 and block_idx + local size (6 for a pose) <= n. Anything else returns
 * VILF_ERR_INVALID_ARGUMENT before anything is copied or launched. */
int vilf_eval_prior(vilf_handle *h, const vilf_prior *prior, const double *const *parameters,
                    double *residuals, double **jacobians);                                 /* marginalization_factor.cpp:333 */
int vilf_eval_edge(vilf_handle *h, const double pose_qt[7], const double curr_point[3], const double point_a[3],
                   const double point_b[3], double residuals[3], double *jacobian /*3x7 or NULL*/);   /* lidarFactor.hpp:21 */
int vilf_eval_surf(vilf_handle *h, const double pose_qt[7], const double curr_point[3], const double norm[3],
                   double negative_OA_dot_norm, double residuals[1], double *jacobian /*1x7 or NULL*/); /* lidarFactor.hpp:79 */
int vilf_pose_plus(vilf_handle *h, const double x[7], const double delta[6], double x_plus_delta[7]); /* pose_local_parameterization.cpp:3 */
int vilf_se3_plus(vilf_handle *h, const double x[7], const double delta[6], double x_plus_delta[7]);  /* EstimationMapping.hpp:34 */

/* ---- IMU pre-integration (host; ≙ IntegrationBase, integration_base.h:30-158) ---------- */
typedef struct vilf_imu_noise { double acc_n, gyr_n, acc_w, gyr_w; } vilf_imu_noise;
int vilf_imu_preintegrate(const vilf_imu_noise *noise, const double acc_0[3], const double gyr_0[3],
                          const double linearized_ba[3], const double linearized_bg[3], int n_samples,
                          const double *dt, const double *acc /*[n][3]*/, const double *gyr /*[n][3]*/,
                          vilf_imu_preint *out);

/* the same integration for n intervals at once on the device (one lane per interval): all inputs are [n][...] host arrays with
 * max_samples slots per interval (n_samples[i] of them used); out[n] */
int vilf_imu_preintegrate_batch(vilf_handle *h, int n, const vilf_imu_noise *noise, const double *acc_0 /*[n][3]*/, const double *gyr_0,
                                const double *linearized_ba, const double *linearized_bg, const int *n_samples, int max_samples,
                                const double *dt /*[n][max]*/, const double *acc /*[n][max][3]*/, const double *gyr, vilf_imu_preint *out);
/* ---- visual-inertial alignment before the first window solve (≙ VisualIMUAlignment, initial/initial_aligment.cpp:199-207; device) ----
 * n_frames frames of all_image_frame in time order: frame_R[k] = c0_R_bk (ImageFrame::R), frame_T[k] = c0_T_ck up to scale (ImageFrame::T),
 * and the n_frames - 1 raw IMU intervals between them (interval k joins frames k and k + 1 = frame k + 1's pre_integration; arrays as in
 * vilf_imu_preintegrate_batch), first integrated at lin_ba / lin_bg. TIC and G come from the handle's options.
 *   solveGyroscopeBias (:3)  -> delta_bg (the caller adds it to every Bgs[i]); every interval is re-integrated at (0, bgs0 + delta_bg) -> pre_out[n-1]
 *   LinearAlignment (:125) + RefineGravity (:55) -> g (c0 frame), x = [v_0 .. v_{n-1} in the body frames, 2 tangent coefficients, s], *n_x = 3 n + 3
 *   (3 n + 4 = [v.., g, 100 s] when the |g| / s gate at :184 fails), *ok = the reference's bool result. */
int vilf_visual_imu_alignment(vilf_handle *h, int n_frames, const double *frame_R /*[n][9]*/, const double *frame_T /*[n][3]*/,
                              const vilf_imu_noise *noise, const double *acc_0 /*[n-1][3]*/, const double *gyr_0, const double *lin_ba, const double *lin_bg,
                              const int *n_samples /*[n-1]*/, int max_samples, const double *dt /*[n-1][max]*/, const double *acc /*[n-1][max][3]*/, const double *gyr,
                              const double bgs0[3], double delta_bg[3], double g[3], double *x /*[3 n + 4]*/, int *n_x, vilf_imu_preint *pre_out /*[n-1] or NULL*/,
                              int *ok);

/* ---- pose-graph back-end of global_fusion (≙ poseGraphOptimization.cpp: the gtsam graph + isam update, :349-374, :560-587, :433-436; device) ----
 * Nodes = key-frame poses [qx qy qz qw tx ty tz] (gtsam::Pose3), node 0 carries the PriorFactor (its pose as handed in, sigma = prior_sigma).
 * Edges = BetweenFactor<Pose3>(i, j, measured = T_i^-1 T_j) with a Diagonal noise model given as sigmas in gtsam's tangent order
 * [rot x y z, trans x y z] (the reference: odometry variances 1e-6 / 1e-4, loop variances 0.5) and robust = 1 for
 * noiseModel::Robust(Cauchy(1), ...) (the ICP loop edges). Every consecutive pair (k, k + 1) needs at least one edge (the odometry
 * chain); all other edges are loop closures. ISAM2's incremental Gauss-Newton is run as batch Gauss-Newton to convergence:
 * at most max_iterations steps, stop when max |delta| < tol. poses_qt is updated in place. */
typedef struct vilf_pg_edge {
    int i, j;
    double q[4], t[3];        /* measured relative pose, x y z w */
    double sigma[6];
    int robust;
    int pad_;
} vilf_pg_edge;
/* Limit: at most 2048 loop edges (edges between non-consecutive key frames): their 6 L x 6 L capacitance block is solved by the library's own dense Cholesky, whose
 * back substitution keeps the solution in LDS. More loop edges: VILF_ERR_UNSUPPORTED, before any work is enqueued. */
int vilf_posegraph_optimize(vilf_handle *h, int n_nodes, double *poses_qt /*[n][7] in/out*/, const double prior_sigma[6], int n_edges, const vilf_pg_edge *edges,
                            int max_iterations, double tol, int *iterations_out, double *final_cost);

/* ---- Scan Context loop detection of global_fusion (≙ SCManager, global_fusion/include/Scancontext/Scancontext.h; device) ----
 * A database of key-frame descriptors that lives on the device (sized at creation, one per handle) and the search over it:
 *   descriptor   makeScancontext :42-86 + xy2theta common.h:79-92: 20 rings x 60 sectors, bin = max(z + lidar_height) as float, stored as double, empty bin 0.
 *                Point arithmetic is float like the reference's (range = sqrtf of separately rounded products; the angle from a correctly rounded
 *                atanf = fp64 atan of the float quotient rounded to float, scaled in double, rounded to float; ceil in double, clamped to [1, 20] / [1, 60]).
 *                Points with a non-finite x, y or z, and points with x == 0 && y == 0, are undefined behaviour in the reference (int(ceil(NaN))): they are skipped.
 *   keys         ring key :89-103 = row means (summed in column order, fp64, / 60, cast to float like eig2stdvec); sector key :105-119 = column means (fp64)
 *   detection    detectLoopClosureID :210-300: nothing while fewer than num_exclude_recent + 1 descriptors exist; the searchable set is a snapshot
 *                [0, n - num_exclude_recent) taken when the call counter is a multiple of tree_making_period and reused for the following calls; the
 *                num_candidates snapshot entries nearest to the query's ring key (float squared L2, dimensions summed in order; nanoflann's search is exact, so
 *                the brute-force set is the same; exact ties go to the lower index, where nanoflann's order would depend on its tree), fewer if the snapshot is smaller
 *   distance     distanceBtnScanContext :153-190: first shift = argmin over 60 shifts of |sector-key difference| (first minimum wins), searched shifts = that one
 *                +- round(0.5 * search_ratio * 60) in ascending order, first minimum wins; distance at a shift (distDirectSC :127-151) = 1 - mean over the columns
 *                where both norms are non-zero of the cosine; no such column: NaN, which never wins. circshift moves column c to (c + s) % 60.
 * Exhaustive mode (not in the reference; equation 6 of the Scan Context paper): num_candidates = 0 takes every snapshot entry (candidate order = index order),
 * search_ratio = 1 every shift. vilf_reset leaves the database alone; vilf_sc_create resets it. */
typedef struct vilf_sc_params {
    int num_rings, num_sectors;      /* PC_NUM_RING 20, PC_NUM_SECTOR 60 (:308-309): the only shape the kernels are built for, anything else is VILF_ERR_UNSUPPORTED */
    double max_radius;               /* PC_MAX_RADIUS 80 (:311, setMaximumRadius :301) */
    double lidar_height;             /* LIDAR_HEIGHT 2.0 (:306) */
    int num_exclude_recent;          /* NUM_EXCLUDE_RECENT 30 (:316) */
    int num_candidates;              /* NUM_CANDIDATES_FROM_TREE 3 (:317), at most 16; 0 = every snapshot entry */
    double search_ratio;             /* SEARCH_RATIO 0.1 (:320); 1 = all shifts */
    double dist_thres;               /* SC_DIST_THRES 0.2 (:322, setSCdistThres :296). +inf is accepted and accepts everything, also a search in which no candidate had
                                      * a distance: min_dist stays 10000000 < inf, so loop_id = nearest = 0, nn_idx's initial value, as in the reference */
    int tree_making_period;          /* TREE_MAKING_PERIOD_ 30 (:325) */
    int pad_;
} vilf_sc_params;
void vilf_sc_default_params(vilf_sc_params *p);
typedef struct vilf_sc_result {
    int loop_id;                     /* nearest if min_dist < dist_thres, else -1 (:275-285) */
    int nearest;                     /* nn_idx (what the reference prints); -1 for a query that returned early (:221-225) */
    int shift;                       /* nn_align */
    int n_candidates;                /* candidates searched (exhaustive mode: the snapshot size) */
    double min_dist;                 /* 10000000 (the reference's initial value) when no candidate had a distance */
    float yaw_diff_rad;              /* float(deg2rad(shift * 6.0)) :288 */
    int candidates[16];              /* the first min(n_candidates, 16) candidate indices in search order, the rest -1 */
} vilf_sc_result;
/* a database for `capacity` key frames (an existing one of the handle is dropped, the call counter and the snapshot with it) */
int vilf_sc_create(vilf_handle *h, const vilf_sc_params *p, int capacity);
/* makeAndSaveScancontextAndKeys (:193-204; poseGraphOptimization.cpp:553): xyzi [n_points][4] -> descriptor + keys of key frame *index_out.
 * A full database is VILF_ERR_UNSUPPORTED and leaves it as it was. */
int vilf_sc_add_keyframe(vilf_handle *h, const float *xyzi, int n_points, int *index_out);
/* the same for n clouds in one upload and one launch: cloud i = points [offsets[i], offsets[i + 1]) of xyzi */
int vilf_sc_add_keyframes(vilf_handle *h, int n, const float *xyzi, const int *offsets /*[n + 1]*/, int *first_index_out);
/* detectLoopClosureID (:210-300; performSCLoopDetection, poseGraphOptimization.cpp:598-614) for the newest key frame; counts the calls that get past the early return */
int vilf_sc_detect(vilf_handle *h, vilf_sc_result *out);
/* replay: out[i] = what vilf_sc_detect returned, or would have, right after key frame first + i was added, had it been called once per key frame from an empty
 * database (query k >= num_exclude_recent is call c = k - num_exclude_recent, its snapshot [0, period * (c / period) + 1)). One chain of launches for all queries;
 * does not touch the call counter of vilf_sc_detect. */
int vilf_sc_detect_range(vilf_handle *h, int first, int n, vilf_sc_result *out);
int vilf_sc_get(vilf_handle *h, int index, double desc[1200] /*[20][60]*/, float ring_key[20], double sector_key[60]);
int vilf_sc_size(vilf_handle *h, int *n_out);
/* vilf_set_profiling: sc_descriptor, sc_ringkey_topk, sc_distance, sc_reduce */
int vilf_get_profile_sc(vilf_handle *h, double ms_out[4], long launches_out[4]);

/* ---- ICP verification of a loop candidate (≙ icpCalculation, global_fusion/poseGraphOptimization.cpp:376-443; device) ----
 * PCL 1.7.2 is not available, so this is a restatement from PCL's documented behaviour: parity unpinned. Every choice PCL leaves to Eigen or FLANN internals is
 * pinned here; tests/icp_reference.py restates the same text in numpy.
 *   store        key-frame clouds (thisKeyFrameDS :541-551, float xyzi, finite) resident on the device, one store per handle, sized at creation (key frames and
 *                total points). Poses (KeyFramePosesUpdated, x y z roll pitch yaw as doubles) come with every call: they change after every graph update.
 *   sub-map      loopFindNearKeyframeCLoud(key, submap_size, root) :194-219: the clouds key - submap_size .. key + submap_size that exist, concatenated in that
 *                order, every one transformed with the pose of key frame `root` (the own-pose line is commented out at :205; own_pose = 1 uses each cloud's own
 *                pose instead). The transform is pcl::getTransformation as a float affine: the six values rounded to float, sine and cosine of an angle = the fp64
 *                function of the float angle rounded to float, A, B = cos, sin yaw, C, D = cos, sin pitch, E, F = cos, sin roll, DE = D*E, DF = D*F,
 *                rows [A*C, A*DF - B*E, B*F + A*DE | x], [B*C, A*E + B*DF, B*DE - A*F | y], [-D, C*F, C*E | z], every product and sum rounded on its own.
 *                Applied as local2global :171-192: per component ((m0*x + m1*y) + m2*z) + m3 in float, no contraction; intensity copied.
 *                Then pcl::VoxelGrid with leaf `leaf_size`: inv = 1.0f / leaf; leaf coordinates floor(p * inv) in float relative to floor(min * inv) of the
 *                cloud's own bounding box; leaf index ix + iy * dx + iz * dx * dy; leaves in ascending leaf index; centroid of x, y, z, intensity: the points of
 *                a leaf summed in float in concatenation order, then divided by the float count (PCL's std::sort leaves the order open; this is the order of
 *                the oracle's voxel_grid). An empty sub-map stays empty (:210-211). A bounding box of 2^40 leaves or more is VILF_ERR_UNSUPPORTED.
 *                Source = (curr, 0, root = prev), target = (prev, history, root = prev) :394-398.
 *   ICP          pcl::IterativeClosestPoint as configured at :401-412. final = guess (identity in the reference) as a float 4 x 4, the source moved by it.
 *                Each round: for every source point its nearest target point, d2 = ((dx*dx) + (dy*dy)) + (dz*dz) in float without contraction (FLANN L2_Simple),
 *                exact ties to the lower target index; accepted if d2 <= max_correspondence_distance^2 (compared in double). No reciprocal test, no rejectors,
 *                no RANSAC. Fewer than 3 accepted: not converged, stop (criterion 5). Step = rigid Umeyama without scale (TransformationEstimationSVD) in fp64:
 *                n, sum s, sum t, sum s t^T over the accepted pairs accumulated in fp64 in a fixed tree (xor butterfly 32, 16, .. 1 within 64 consecutive source
 *                points, then the 4 groups of 64 of a block of 256 in order, then the blocks in order), H = sum t s^T / n - mean_t mean_s^T, H = U D V^T by
 *                one-sided Jacobi, R = U diag(1, 1, det U det V) V^T, t = mean_t - R mean_s; the 4 x 4 rounded to float = T_k. Below rank two (collinear
 *                correspondences, or a single target point) R is a proper rotation that maps mean_s to mean_t (with t) and the source's principal direction
 *                onto the target's, and nothing more is pinned. source <- T_k source (float,
 *                as above, on the already moved source: incrementally, as PCL does), final <- T_k final (float, entry = ((a0*b0 + a1*b1) + a2*b2) + a3*b3).
 *                DefaultConvergenceCriteria after every step, in this order: 1 iterations reached max_iterations; 2 cos = 0.5 (trace R_k - 1) >=
 *                rotation_threshold and |t_k|^2 <= transformation_epsilon (fp64 of the float entries); with mse = mean of the accepted d2 of this round (fp64):
 *                3 |mse - mse_prev| < euclidean_fitness_epsilon; 4 |mse - mse_prev| / mse_prev < mse_relative (mse_prev starts at DBL_MAX).
 *   fitness      getFitnessScore(): one more search over the final source, mean of the nearest d2 (float each, summed in fp64 in the same tree) over all source
 *                points, no range limit; no source or no target point: DBL_MAX. accepted = converged && fitness <= fitness_threshold (:414-423).
 *   result       pcl::getTranslationAndEulerAngles(final): roll = atan2(m21, m22), pitch = asin(-m20), yaw = atan2(m10, m00), each the fp64 function of the float
 *                entries rounded to float -> pose6 [x y z roll pitch yaw]; pose_qt = [qx qy qz qw tx ty tz] of Rot3::RzRyRx(roll, pitch, yaw) in fp64, qw >= 0
 *                (:428-432). The loop edge measures its inverse (:433-436), which PoseGraph.add_loop takes.
 *   global map   publishGlobalMap :310-336 (driven by loopMap :338-347, topic /Map_graph): the clouds first, first + skip, ... (< first + count), each under its OWN
 *                pose whatever own_pose says (:320), concatenated in key-frame order, then pcl::VoxelGrid with leaf `leaf_size` (:326-327): transform, voxel-filter
 *                arithmetic and summation order are the sub-map's, above, so the map of an own_pose = 1 store equals the sub-map over the same clouds bit for bit.
 *                Rebuilt from scratch by every call, as the reference does every 5 s: a loop closure moves every pose. The map lives in a buffer of its own until
 *                the next build or vilf_icp_create; no align or sub-map call writes it. An empty selection is an empty map. More than 2^30 selected points, or a
 *                bounding box of 2^40 leaves or more, is VILF_ERR_UNSUPPORTED: the store stays as it was and the previous map is dropped (size 0). This
 *                deliberately does not mirror PCL's int32 guard, which warns and returns the input unfiltered.
 * vilf_reset leaves the store alone; vilf_icp_create resets it. */
typedef struct vilf_icp_params {
    double max_correspondence_distance;  /* 100 (:402) */
    int max_iterations;                  /* 100 (:403); at most 1000 */
    int history_keyframes;               /* historyKeyframesSearchNum 25 (:394) */
    double transformation_epsilon;       /* 1e-6 (:404) */
    double euclidean_fitness_epsilon;    /* 1e-6 (:405) */
    double rotation_threshold;           /* DefaultConvergenceCriteria: 0.99999 */
    double mse_relative;                 /* DefaultConvergenceCriteria: 1e-5 */
    double fitness_threshold;            /* loopFitnessScoreThreshold 0.3 (:414) */
    double leaf_size;                    /* MapLeafSize 0.4 (:646-647) */
    int own_pose;                        /* 0 (:206); 1: every cloud of a sub-map under its own pose (:205) */
    int pad_;
} vilf_icp_params;
void vilf_icp_default_params(vilf_icp_params *p);
enum { VILF_ICP_NONE = 0, VILF_ICP_ITERATIONS = 1, VILF_ICP_TRANSFORM = 2, VILF_ICP_ABS_MSE = 3, VILF_ICP_REL_MSE = 4, VILF_ICP_NO_CORRESPONDENCES = 5 };
typedef struct vilf_icp_result {
    int converged, accepted, criterion /* VILF_ICP_*: the rule that ended the rounds */, iterations;
    int n_source, n_target, n_correspondences /* of the last round */, pad_;
    double fitness, final_mse;
    float transform[16];             /* final, row-major */
    double pose6[6], pose_qt[7];
} vilf_icp_result;
typedef struct vilf_icp_iter {
    int n_correspondences, criterion /* VILF_ICP_NONE while the rounds go on */;
    double mse, cos_angle, translation_sqr;
} vilf_icp_iter;
/* a store for cap_keyframes clouds of cap_points points in all (an existing one of the handle is dropped) */
int vilf_icp_create(vilf_handle *h, const vilf_icp_params *p, int cap_keyframes, long cap_points);
/* cloud of the next key frame (xyzi [n][4]). A full store is VILF_ERR_UNSUPPORTED, a value that is not finite invalid-argument; both leave the store as it was.
 * Poses and guesses that are not finite are invalid-argument too, before any work is enqueued. */
int vilf_icp_add_cloud(vilf_handle *h, const float *xyzi, int n, int *index_out);
int vilf_icp_add_clouds(vilf_handle *h, int n, const float *xyzi, const int *offsets /*[n + 1]*/, int *first_index_out);
int vilf_icp_size(vilf_handle *h, int *n_out);
/* the sub-map as ICP sees it; poses6 = [size][6]. n_out is always complete, xyzi_out truncated to cap points. A key or root outside the store: invalid argument. */
int vilf_icp_submap(vilf_handle *h, int key, int submap_size, int root, const double *poses6, float *xyzi_out, int cap, int *n_out);
/* icpCalculation for the pair (prev, curr); guess_qt = [qx qy qz qw tx ty tz] or NULL for identity */
int vilf_icp_align(vilf_handle *h, int prev, int curr, const double *poses6, const double *guess_qt, vilf_icp_result *out);
/* n pairs in one chain of launches (grid dimension = pair); out[i] is bit-identical to the single call. guess_qt = [n][7] or NULL */
int vilf_icp_align_pairs(vilf_handle *h, int n, const int *prev, const int *curr, const double *poses6, const double *guess_qt, vilf_icp_result *out);
/* the rounds of pair `pair` of the last align call */
int vilf_icp_get_history(vilf_handle *h, int pair, vilf_icp_iter *out, int cap, int *n_out);
/* diagnostic (what lets a test compare the search point by point): nearest target index (into the target sub-map, -1: none) and d2 of every source point of pair `pair` of the last align call: which = 0 the first round, 1 the fitness pass */
int vilf_icp_get_search(vilf_handle *h, int pair, int which, int *index_out, float *d2_out, int cap, int *n_out);
/* vilf_set_profiling: icp_bbox, icp_leaf_keys, radix sorts, icp_voxel, icp_cell_keys + icp_cell_table, icp_search, icp_step, (unused) */
int vilf_get_profile_icp(vilf_handle *h, double ms_out[8], long launches_out[8]);
/* publishGlobalMap: clouds first, first+skip, ... (< first+count) each under its OWN pose (whatever own_pose says), concatenated in key-frame order, VoxelGrid(leaf_size).
 * One chain of launches over the whole grid, one wait. Invalid argument, nothing enqueued, the previous map kept: first < 0, count < 0, skip < 1, first + count > size,
 * a null poses6 or n_out, a pose that is not finite. count = 0 is a valid empty map. Like vilf_icp_submap, a build invalidates vilf_icp_get_history / get_search. */
int vilf_icp_global_map(vilf_handle *h, int first, int count, int skip, const double *poses6 /*[size][6]*/, long *n_out);
/* points of the current map (0: none built, or the last build failed) */
int vilf_icp_global_map_size(vilf_handle *h, long *n_out);
/* points [offset, offset + count) of the map, ascending leaf index. Outside [0, n), or before any build: invalid argument */
int vilf_icp_global_map_get(vilf_handle *h, long offset, long count, float *xyzi_out /*[count][4]*/);
/* vilf_set_profiling: gmap_xf_bbox + gmap_box, gmap_leaf_keys, radix sort, gmap_count + gmap_scan + gmap_centroids */
int vilf_get_profile_icp_map(vilf_handle *h, double ms_out[4], long launches_out[4]);

/* ---- scan-to-map (≙ EstimationMapping) -------------------------------------------------- */
/* points are float xyzi (pcl::PointXYZI without padding): [n][4] */
int vilf_scan2map_init(vilf_handle *h, const float *edge_xyzi, int n_edge, const float *surf_xyzi, int n_surf);   /* localMapInited, :105 */
/* optimation_processing(:235): in/out pose_qt = parameter_opti [qx qy qz qw tx ty tz] is kept in the handle
 * (globalOdom / globalOdom_last); returns the new global pose and the frame-to-frame relative pose T_ij. */
typedef struct vilf_scan2map_result {
    double pose_qt[7];          /* globalOdom after the step */
    double rel_q[4], rel_t[3];  /* globalOdom_last^-1 * globalOdom: the /Odometry message (feature_tracker_node.cpp:400-415) */
    int n_edge_ds, n_surf_ds;   /* after voxel down-sampling */
    int n_edge_factors[2];      /* accepted edge factors in association pass 0/1 */
    int n_surf_factors[2];
    int iterations[2];          /* solver iterations per pass */
    double final_cost[2];
    int map_edge_size, map_surf_size;
} vilf_scan2map_result;
int vilf_scan2map_step(vilf_handle *h, const float *edge_xyzi, int n_edge, const float *surf_xyzi, int n_surf,
                       vilf_scan2map_result *res);
int vilf_scan2map_get_map(vilf_handle *h, int which /*0 edge, 1 surf*/, float *xyzi_out, int capacity, int *n_out);
int vilf_scan2map_set_pose(vilf_handle *h, const double pose_qt[7], const double pose_last_qt[7]);

/* ---- batched scan-to-map: n_streams independent EstimationMapping objects (one per LiDAR stream / replayed segment)
 * stepped together with no host round trip. Capacities are per stream and fixed (a step that would overflow a local map
 * reports VILF_ERR_UNSUPPORTED through vilf_scan2map_batch_results). Stream i's result equals what a single-stream
 * handle fed with the same clouds returns. */
int vilf_scan2map_batch_create(vilf_handle *h, int n_streams, int cap_scan_edge, int cap_scan_surf, int cap_map_edge, int cap_map_surf);
/* localMapInited (:105) of one stream: its local map := the clouds; pose_qt (NULL = identity) -> globalOdom,
 * pose_last_qt (NULL = pose_qt) -> globalOdom_last (the constant-velocity prediction of the first step, :238-243) */
int vilf_scan2map_batch_init(vilf_handle *h, int stream, const float *edge_xyzi, int n_edge, const float *surf_xyzi, int n_surf,
                             const double *pose_qt, const double *pose_last_qt);
/* the scan the next vilf_scan2map_batch_step consumes for this stream (stays resident in HBM until replaced) */
int vilf_scan2map_batch_set_scan(vilf_handle *h, int stream, const float *edge_xyzi, int n_edge, const float *surf_xyzi, int n_surf);
/* stream dst := stream src (local maps, poses, resident scan) by device copies: replicas of a few distinct streams without one upload per stream */
int vilf_scan2map_batch_copy_stream(vilf_handle *h, int src, int dst);
int vilf_scan2map_batch_step(vilf_handle *h, int sync);                 /* optimation_processing (:235) for every stream */
/* A snapshot holds until the next one. A call that writes a stream's map outside a step (vilf_scan2map_batch_init,
 * vilf_scan2map_batch_copy_stream) drops it: vilf_scan2map_batch_rewind then fails with VILF_ERR_INVALID_ARGUMENT
 * ("no snapshot") until a new snapshot is taken. */
int vilf_scan2map_batch_snapshot(vilf_handle *h);                       /* remember maps + poses ... */
int vilf_scan2map_batch_rewind(vilf_handle *h);                         /* ... and restore them (bench loop: repeated identical steps) */
int vilf_scan2map_batch_results(vilf_handle *h, int first, int n, vilf_scan2map_result *res);
int vilf_scan2map_batch_get_map(vilf_handle *h, int stream, int which, float *xyzi_out, int capacity, int *n_out);

/* ---- LiDAR feature extraction (≙ featureExtraction::extractFeature, feature_tracker/include/featureExtraction.hpp:54-232) ----
 * raw scan (xyzi, firing order) -> edge / surf feature clouds, the inputs of vilf_scan2map_*: ring assignment from the vertical
 * angle (n_scans 16 / 32 / 64), per-ring 10-neighbour curvature, six sectors per ring, <= 20 edge picks per sector with +-5
 * neighbour suppression, the remaining points as surf. Outputs are truncated to the capacities; the counts are always complete.
 * A negative capacity is VILF_ERR_INVALID_ARGUMENT, before any device work. A sector of more than 1024 elements (a ring of more than
 * 6160 accepted returns) is VILF_ERR_UNSUPPORTED with both counts 0; the handle stays usable. */
int vilf_lidar_extract_features(vilf_handle *h, const float *xyzi, int n_points, int n_scans, double min_range, double max_range,
                                double edge_threshold, float *edge_xyzi_out, int cap_edge, int *n_edge,
                                float *surf_xyzi_out, int cap_surf, int *n_surf);
/* LiDAR depth of the tracked visual features ≙ getFeatureDepth (feature_tracker/feature_tracker_node.cpp:54-163): depth cloud in the
 * camera frame (xyzi), features as normalised image points (x, y, z = 1); depth_out[i] = depth of feature i (what the estimator
 * receives as point(7), estimator_node.cpp) or -1 when the 3 nearest returns do not support one. */
int vilf_feature_depth(vilf_handle *h, const float *depth_cloud_xyzi, int n_points, const float *features_xyz, int n_features, float *depth_out);

/* ---- Image feature tracker (≙ FeatureTracker::readImage and readImage_mask, feature_tracker/feature_tracker.cpp:119-209, :212-381; device) ----
 * OpenCV is not available, so this text fixes the arithmetic itself; tests/track_reference.py restates it in numpy (frontend_reference.py and mask_reference.py the optional steps) and the kernels agree with that to the bit.
 * It is modelled on what the reference calls: cv::calcOpticalFlowPyrLK(.., Size(21,21), 3) (:151: window, levels, 30 iterations / 0.01 px, the 1e-4 minimum
 * eigenvalue, 14-bit fixed-point patches, unnormalised Scharr gradients), cv::goodFeaturesToTrack(.., 0.01, MIN_DIST, mask) (:190), setMask (:36-71), inBorder
 * (:5-11), undistortedPoints (:556-604), updateID. One deliberate difference makes bit identity possible: sums over a window are exact integer sums, where OpenCV
 * adds floats in an unspecified SIMD order. Agreement with OpenCV itself is not measured and not claimed.
 *   conventions  images are 8-bit, row-major, W x H. R(i, n) = reflect-101 of an index, applied periodically with period 2 (n - 1), so it is defined for any
 *                offset. Points are float32 (x, y) pixel coordinates. "fp64 / float32, each operation rounded": every + - * / sqrt is its own IEEE operation
 *                (no contraction). rint is round-half-to-even.
 *   pyramid      level 0 is the image; level L + 1 has size ((W_L + 1) / 2, (H_L + 1) / 2) and value (sum_{i,j = -2..2} k_i k_j I_L(R(2x + i), R(2y + j)) + 128) >> 8,
 *                k = [1 4 6 4 1]. Levels used: 0 .. Lmax, Lmax <= 3 the largest level whose two sides are both > 21.
 *                Gradients (int): Gx(x, y) = 3 (I(x+1, y-1) - I(x-1, y-1)) + 10 (I(x+1, y) - I(x-1, y)) + 3 (I(x+1, y+1) - I(x-1, y+1)), Gy its transpose, image reads
 *                through R; Gx = Gy = 0 at positions outside the image.
 *   LK           per point, from level Lmax down to 0. p_L = float32(prev * 2^-L); q = p_L at Lmax, else 2 * the previous level's q.
 *                corner: c = p_L - 10 in float32, (ix, iy) = floor(c), (a, b) = c - floor(c). Bounds: ix < -21, ix >= W_L, iy < -21 or iy >= H_L (or a coordinate
 *                that is not a number): at level 0 status <- 0; at any level the level is skipped and q carried on unchanged.
 *                weights (int, the products in float32, each operation rounded): w00 = rint((1-a)(1-b) 16384), w01 = rint(a (1-b) 16384), w10 = rint((1-a) b 16384),
 *                w11 = 16384 - w00 - w01 - w10.
 *                template, for the 21 x 21 offsets (u, v), bilinear over (ix+u, iy+v) and its right, lower and lower-right neighbours with w00, w01, w10, w11:
 *                T = (sum w I + 256) >> 9, Tx = (sum w Gx + 8192) >> 14, Ty likewise (>> is arithmetic); image reads through R.
 *                normal matrix: A11 = sum Tx^2, A12 = sum Tx Ty, A22 = sum Ty^2 as exact integers, a_ij = A_ij 2^-20 in fp64; in fp64, each operation rounded:
 *                D = a11 a22 - a12 a12, e = ((a11 + a22) - sqrt((a11 - a22)^2 + (4 a12) a12)) / 882. If e < 1e-4 or D < 1.1920929e-7: at level 0 status <- 0; the
 *                level is skipped.
 *                iterations, at most 30: corner and weights from q - 10 as above with the same bounds rule (out of bounds ends the level, at level 0 status <- 0);
 *                J = the same bilinear form on the next image; b1 = sum (J - T) Tx, b2 = sum (J - T) Ty as exact integers, each scaled by 2^-20;
 *                delta = ((a12 b2 - a22 b1) (1 / D), (a12 b1 - a11 b2) (1 / D)); q <- float32(q + delta); stop if delta . delta <= 1e-4; from the second iteration
 *                on: if |dx + dx_prev| < 0.01 and |dy + dy_prev| < 0.01 then q <- float32(q - delta / 2) and stop.
 *                Result: q at level 0, status 1 unless cleared. vilf_track_lk returns exactly this; vilf_track_read_image then clears the status of the points
 *                whose pixel (rint x, rint y) is not in [1, W-2] x [1, H-2] (inBorder) and drops every point with status 0.
 *   setMask      the survivors get track_cnt + 1 and are ordered by track_cnt descending, ties by lower index; a point is kept iff its pixel (rint x, rint y) lies
 *                in no disc dx^2 + dy^2 <= MIN_DIST^2 around the pixel of an already kept point. (cv::circle's raster may differ from this disc at rim pixels and
 *                std::sort is not stable: deviations, DESIGN.md.)
 *   detection    n_max = MAX_CNT - kept, skipped if <= 0. Sobel 3 x 3 Sx, Sy (int, reads through R): Sx = (I(x+1, y-1) + 2 I(x+1, y) + I(x+1, y+1)) - (the same at
 *                x-1), Sy its transpose. P = sum Sx^2, Q = sum Sx Sy, S = sum Sy^2 over the 3 x 3 neighbourhood, the neighbour's coordinates taken through R.
 *                lambda = (P + S) - sqrt((P - S)^2 + (4 Q) Q) in fp64, each operation rounded. A pixel is allowed iff it lies in none of the kept points' discs;
 *                lambda_max = the maximum over the allowed pixels. Candidates: allowed, 1 <= x <= W-2, 1 <= y <= H-2, lambda > 0.01 lambda_max, lambda >= lambda of
 *                every 3 x 3 neighbour; ordered by lambda descending, ties by lower y W + x; accepted greedily while fewer than n_max are accepted: iff
 *                dx^2 + dy^2 >= MIN_DIST^2 to every accepted corner. New points are appended behind the kept ones with id -1, track_cnt 1; the ids -1 then
 *                become n_id++ in list order (updateID).
 *   undistortion (PinholeCamera::liftProjective, PinholeCamera.cc:450-510) fp64, each operation rounded: m = ((1 / fx) u + (-cx / fx), (1 / fy) v + (-cy / fy)).
 *                If any of k1, k2, p1, p2 is non-zero: 8 rounds of m_u = m - distortion(m_u), starting from m_u = m, with (PinholeCamera::distortion, :646-662)
 *                rho2 = x x + y y, rad = k1 rho2 + (k2 rho2) rho2, dx = (x rad + (2 p1) (x y)) + p2 (rho2 + 2 (x x)), dy = (y rad + (2 p2) (x y)) + p1 (rho2 + 2 (y y)).
 *                The result is rounded to float32. velocity = (un_cur - un_prev of the same id) / (t_cur - t_prev) in fp64 from the float32 values, rounded to
 *                float32; 0 for a new id and on the first frame.
 *   CLAHE        optional (vilf_track_configure, equalize), in front of everything else: the pyramid, LK and the detection see the equalised image. Modelled on
 *                cv::createCLAHE(3.0, Size(8, 8))->apply (:127); clip c and the tiles tx x ty are parameters. Agreement with OpenCV is neither measured nor claimed.
 *                padding: if W % tx == 0 and H % ty == 0 there is none, W' = W, H' = H. Otherwise W' = W + (tx - W % tx) and H' = H + (ty - H % ty), the new columns
 *                and rows read through R: I'(x, y) = I(R(x, W), R(y, H)). A direction that does divide is then padded by a whole tx or ty. That is what the
 *                model does, and it is kept. Tile (tw, th) = (W' / tx, H' / ty), area = tw th; tile (i, j) covers x in [i tw, (i + 1) tw), y in [j th, (j + 1) th).
 *                limit (int): 0 (no clipping) if c <= 0, else max(1, (int)((c * (double)area) / 256.0)), the product and the quotient in fp64, each rounded.
 *                per tile: hist[256] = counts of I' over the tile (int). If limit > 0: excess = sum max(hist - limit, 0), hist = min(hist, limit),
 *                batch = excess / 256, residual = excess - 256 batch (int); every bin + batch; if residual > 0, with step = max(256 / residual, 1) (int) the bins
 *                0, step, 2 step, .. < 256 get + 1 each while residual lasts (bin b iff b % step == 0 and b / step < residual).
 *                lut[b] = sat_u8(rint(float32(sum_{a <= b} hist[a]) * (255.f / float32(area)))): an int sum, a float32 quotient, a float32 product, each rounded.
 *                remap, per pixel (x, y) of the unpadded image with value v, float32, each operation rounded: txf = float32(x) * (1.f / float32(tw)) - 0.5f,
 *                x1 = floor(txf), xa = txf - x1, x2 = x1 + 1, then x1 and x2 clamped to [0, tx - 1]; y1, ya, y2 likewise from y and th;
 *                out = sat_u8(rint((lut[y1, x1][v] * (1 - xa) + lut[y1, x2][v] * xa) * (1 - ya) + (lut[y2, x1][v] * (1 - xa) + lut[y2, x2][v] * xa) * ya)).
 *   rejectWithF  optional (vilf_track_configure, reject_f), after the inBorder drop and before setMask, on the surviving points in list order (n of them;
 *                x = the point in the current image, x' = where LK found it in the new one). Skipped when n < 8 (:385). Modelled on :383-420, but
 *                cv::findFundamentalMat(FM_RANSAC) draws random samples, so the search itself is a design of this project (deviations: DESIGN.md §3i).
 *                lift: both points through the undistortion text above in fp64 (before its rounding to float32), then u = FOCAL_LENGTH x + W / 2.0,
 *                v = FOCAL_LENGTH y + H / 2.0 in fp64, each operation rounded, and (u, v) rounded to float32 (cv::Point2f). All that follows is fp64 on these values.
 *                hypotheses: a fixed number K (1 .. 2048, default 512), no adaptive stopping. With 8-point samples and an inlier share w the chance that no
 *                sample is all inliers is (1 - w^8)^K: about e^-30 at w = 0.7 and 0.13 at w = 0.5 for K = 512.
 *                sample of hypothesis k: mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 (uint32, wrapping).
 *                g(k, d) = mix(mix(mix(seed + 0x9e3779b9) + k) + d). Slot j = 0 .. 7 takes i = (uint64(g(k, j)) * n) >> 32; while i equals the index of an earlier
 *                slot, i <- (i + 1) mod n (at most j steps; no second draw, so the loop is bounded). No state: hypothesis k is the same wherever it is computed.
 *                8-point solve, each side of the sample on its own: c = (sum_j p_j) / 8, the sums from 0 in slot order; mean = (sum_j sqrt(dx dx + dy dy)) / 8 with
 *                (dx, dy) = p_j - c; s = sqrt(2.0) / mean; p^_j = (p_j - c) s. Row j of A: (x^' x^, x^' y^, x^', y^' x^, y^' y^, y^', x^, y^, 1). M = A^T A, each of
 *                the 45 upper entries a sum from 0 over j in slot order, a product and an addition per term. Jacobi(M, 9): V = I; 10 sweeps; in each, the pairs
 *                (p, q), p < q, in row-major order; a pair with a_pq == 0 exactly is skipped; theta = (a_qq - a_pp) / (2 a_pq);
 *                t = (theta < 0 ? -1 : 1) / (|theta| + sqrt(theta theta + 1)); c = 1 / sqrt(t t + 1); s = t c; for r != p, q:
 *                a_rp' = c a_rp - s a_rq, a_rq' = s a_rp + c a_rq (and their mirror images); a_pp' = a_pp - t a_pq; a_qq' = a_qq + t a_pq; a_pq = 0; for every r:
 *                v_rp' = c v_rp - s v_rq, v_rq' = s v_rp + c v_rq. f = the column of V under the smallest a_ii (compared with <, so ties and NaNs leave the lower
 *                index); F^ = f as a row-major 3 x 3. Rank 2: G = F^^T F^ (g_pq = sum_r F^_rp F^_rq from 0), Jacobi(G, 3) as above, v = the column under the
 *                smallest g_ii, w_r = (F^_r0 v_0 + F^_r1 v_1) + F^_r2 v_2, F^_rc <- F^_rc - w_r v_c. Denormalise with (tx, ty) = (s c_x, s c_y) of each side:
 *                B_r0 = F^_r0 s, B_r1 = F^_r1 s, B_r2 = (F^_r2 - F^_r0 tx) - F^_r1 ty; F_0c = s' B_0c, F_1c = s' B_1c, F_2c = (B_2c - tx' B_0c) - ty' B_1c.
 *                The hypothesis is invalid (score -1) unless s, s' and the nine F_rc are finite. (FM_RANSAC uses 7-point samples: one solution, no cubic here.)
 *                score: for every point l' = F x (l'_r = (F_r0 x + F_r1 y) + F_r2), l = F^T x' (l_c = (F_0c x' + F_1c y') + F_2c), d = (x' l'_0 + y' l'_1) + l'_2;
 *                inlier iff d d / (l'_0 l'_0 + l'_1 l'_1) <= F_THRESHOLD^2 and d d / (l_0 l_0 + l_1 l_1) <= F_THRESHOLD^2 (the larger of the two errors; a NaN
 *                compares false: an outlier). Score = the number of inliers. The winner is the valid hypothesis of the highest score, ties to the lower k; the
 *                status is its inlier mask, there is no refit. No valid hypothesis: nothing is rejected (every status 1, best = -1).
 *   mask image   (readImage_mask, :212-381, the front-end of feature_tracker_node_mask.cpp) an 8-bit W x H image that marks dynamic objects: a pixel means "static /
 *                allowed" iff it is != 0 and "dynamic" iff it is 0, which is what the node's copyTo (feature_tracker_node_mask.cpp:276-278) makes of the message.
 *   erode        (the node's cv::erode with an 11 x 11 MORPH_ELLIPSE, :283-290) radius r is a parameter, default 5, 0 .. VILF_TRACK_MAX_ERODE. The element is the
 *                offsets (dx, dy) with |dy| <= r and |dx| <= hw(|dy|), hw(d) = rint(sqrt((double)(r r - d d))); for r = 5 the half-widths are 5, 5, 5, 4, 3, 0.
 *                E(x, y) = 255 iff mask(x + dx, y + dy) != 0 for every offset whose pixel lies inside the image, else 0: pixels outside the image do not erode
 *                (OpenCV's default border for erode). r = 0 only binarises. The element's shape is this text's, not OpenCV's raster (deviations: DESIGN.md §3i).
 *   probe        (:256-290) for each point that survived LK and inBorder, with (x, y) its pixel (rint x, rint y) in the new image and d the probe distance
 *                (parameter, default 5, 1 .. 64): if x > d, y > d, x < W - d and y < H - d, the point is static iff E(x, y - d), E(x, y + d), E(x - d, y) and
 *                E(x + d, y) are all != 0; if the guard does not hold, the point is static. (The reference reads mask_img.at<uchar>(col, row -+ 5), transposed,
 *                and guards with col < ROW - 5: deviations)
 *   rejectWithF_mask (:423-500) after the probe and before setMask, only if the mask parameters' reject is on, on a frame that has a previous one. S = the static
 *                survivors in list order, m = |S|; if m < 8 nothing is rejected. Otherwise all survivors are lifted exactly as in rejectWithF; the hypotheses
 *                are drawn exactly as there, with the configured K, seed and focal length and with S in place of the list (sample indices address S); scored
 *                over S with the mask parameters' f_threshold (default 0.1, :449); winner = highest score, ties to the lower k, no refit. Then for every
 *                survivor, static or not, with (x, y) its lifted point in the current image and (x', y') in the new one: A = (F00 x + F01 y) + F02,
 *                B = (F10 x + F11 y) + F12, C = (F20 x + F21 y) + F22, dd = |(A x' + B y') + C| / sqrt(A A + B B) in fp64, each operation rounded; the point
 *                is dropped iff dd > epi_threshold (default 1.0, :485); a NaN compares false, so the point is kept. No valid hypothesis: nothing is rejected.
 *                The inlier mask of the search itself is not used and the test on all points is one-sided, both as in the reference.
 *   fisheye mask (:38-39) an optional W x H image held by the tracker, for both readImage variants. With it setMask keeps a point only if the fisheye mask at its
 *                pixel is == 255 (:61) and the pixel lies in no disc, and the detection allows a pixel only if the fisheye mask there is != 0
 *                (goodFeaturesToTrack's mask rule) and the pixel lies in no disc. The two rules differ for the values 1 .. 254: there a tracked point is dropped
 *                while a new corner may be found; the difference is the reference's and is kept. Without the image everything is as above.
 *   detection under the dynamic mask (:356-360) a pixel is allowed iff E != 0 there, the fisheye rule holds there and it lies in no disc; lambda_max is the
 *                maximum over the allowed pixels, as before, and nothing else of the detection paragraph changes.
 *   frame order of readImage_mask: CLAHE if on, LK, inBorder, probe, rejectWithF_mask, setMask, detection under E, undistortion; on the first frame there is no LK,
 *                probe or rejection. The reject_f switch of vilf_track_configure does not act here (the reference calls only rejectWithF_mask, :318-319). Plain
 *                and masked calls may alternate on one tracker; they share all state, as the reference's two methods do. */
typedef struct vilf_track_params {
    int width, height;               /* COL, ROW */
    int max_cnt;                     /* MAX_CNT, 1 .. VILF_MAX_FEATURES */
    int min_dist;                    /* MIN_DIST, >= 1 */
    double fx, fy, cx, cy;           /* PinholeCamera::Parameters */
    double k1, k2, p1, p2;
} vilf_track_params;
/* workspace of the tracker, hung off the handle and sized here: four pyramids (current, next, two for the stateless calls), the feature list, the detection
 * buffers (one candidate slot per pixel). Invalid argument, the handle and an existing tracker untouched: a side <= 21, max_cnt < 1 or > VILF_MAX_FEATURES,
 * min_dist < 1, a focal length that is not positive, a camera parameter that is not finite. A second call drops the tracker and its state and sizes a new one. */
int vilf_track_init(vilf_handle *h, const vilf_track_params *p);
/* a fresh FeatureTracker (feature_tracker.cpp:32-34): no points, no previous image, n_id = 0 */
int vilf_track_reset(vilf_handle *h);
/* readImage (:119-209) and the updateID loop (feature_tracker_node.cpp:285-292) for one image (rows row_stride bytes apart): one chain of launches; the host
 * uploads the image and downloads the list. *n_out = rows of the list. */
int vilf_track_read_image(vilf_handle *h, const unsigned char *img, int row_stride, double stamp, int *n_out);
/* the list of the last vilf_track_read_image in list order: ids [n], track_cnt [n], cur_pts / un_pts / velocity [n][2] (any may be NULL). cap < n: invalid
 * argument, nothing written. */
int vilf_track_get(vilf_handle *h, int cap, int *ids, int *track_cnt, float *cur_pts, float *un_pts, float *velocity, int *n_out);
/* stateless pieces (they leave the tracker's state alone): level `level` (0 .. Lmax) of the pyramid of an image, rows tight; */
int vilf_track_pyramid(vilf_handle *h, const unsigned char *img, int row_stride, int level, unsigned char *out);
/* calcOpticalFlowPyrLK (:151) between two images (rows tight) for n points [n][2] -> pts_out [n][2], status_out [n]; without inBorder; */
int vilf_track_lk(vilf_handle *h, const unsigned char *img_prev, const unsigned char *img_next, const float *pts, int n, float *pts_out, unsigned char *status_out);
/* goodFeaturesToTrack (:190) under the mask of n_kept kept points (finite, within 1e6 pixels; at most VILF_MAX_FEATURES): at most n_max <= VILF_MAX_FEATURES
 * new corners -> pts_out [n_max][2] in acceptance order, *n_out of them */
int vilf_track_detect(vilf_handle *h, const unsigned char *img, const float *kept_pts, int n_kept, int n_max, float *pts_out, int *n_out);
/* vilf_set_profiling: the stages of the last vilf_track_read_image: upload + pyramid, LK, setMask, detection (mask, response, candidates, sorts, acceptance),
 * ids + undistortion + velocity */
int vilf_track_profile(vilf_handle *h, double ms_out[5], long launches_out[5]);
/* The two optional steps of readImage (the paragraphs CLAHE and rejectWithF above). Both are off after vilf_track_init, and a tracker that is never configured
 * computes what it computed before they existed. */
typedef struct vilf_track_frontend {
    int equalize; double clahe_clip; int clahe_tiles_x, clahe_tiles_y;                  /* 0/1, 3.0, 8, 8 */
    int reject_f; double f_threshold, focal_length; int n_hypotheses; unsigned seed;    /* 0/1, 1.0, 460, 512 */
} vilf_track_frontend;
#define VILF_TRACK_MAX_TILES 1024        /* tiles_x * tiles_y: the LUT storage sized by vilf_track_init */
#define VILF_TRACK_MAX_HYPOTHESES 2048
/* after vilf_track_init; a later vilf_track_init returns to "both off" with the defaults in the comments above. Every field is checked whether its step is on or
 * not. Invalid argument, the handle and the tracker untouched: no tracker, tiles < 1 or tiles_x * tiles_y > VILF_TRACK_MAX_TILES, a clip that is negative or not
 * finite, a threshold or focal length that is not positive and finite, n_hypotheses outside 1 .. VILF_TRACK_MAX_HYPOTHESES. The tracked state is kept. */
int vilf_track_configure(vilf_handle *h, const vilf_track_frontend *fe);
/* stateless: CLAHE of an image (rows row_stride bytes apart) with the configured clip and tiles (the defaults if never configured) -> out, rows tight */
int vilf_track_clahe(vilf_handle *h, const unsigned char *img, int row_stride, unsigned char *out);
/* stateless: rejectWithF on n point pairs [n][2] with the tracker's camera and the configured threshold, focal length, K and seed -> status_out [n], F_out (row-major),
 * *best_out = the winning k, *n_inliers_out. n < 8 or no valid hypothesis: every status 1, best -1, n_inliers n, F 0; that is no error. Invalid argument, nothing
 * written: a null pointer, n < 0, n > VILF_MAX_FEATURES, a coordinate that is not finite. */
int vilf_track_reject_f(vilf_handle *h, const float *cur_pts, const float *forw_pts, int n, unsigned char *status_out, double F_out[9], int *best_out, int *n_inliers_out);
/* vilf_set_profiling: CLAHE (both kernels) and rejectWithF (lift, hypotheses, score, apply) of the last vilf_track_read_image; 0 for a step that is off. The
 * five stages of vilf_track_profile are as before: CLAHE falls into the first of them, rejectWithF into the second. */
int vilf_track_profile_frontend(vilf_handle *h, double ms_out[2], long launches_out[2]);
/* The dynamic-object mask and the fisheye mask (the paragraphs mask image .. frame order above). A tracker that never sets a fisheye mask and never calls the
 * masked entry point computes what it computed before they existed, with the same launches. */
#define VILF_TRACK_MAX_ERODE 16
typedef struct vilf_track_mask_params {
    int erode_radius, probe, reject;          /* 5, 5, 1 */
    double f_threshold, epi_threshold;        /* 0.1, 1.0 */
} vilf_track_mask_params;
/* after vilf_track_init; a later vilf_track_init returns to the defaults in the comments above and drops the fisheye mask, vilf_track_reset keeps both (the node
 * loads the fisheye mask once, after construction). Invalid argument, the handle and the tracker untouched: no tracker, null parameters, a radius outside
 * 0 .. VILF_TRACK_MAX_ERODE, a probe outside 1 .. 64, reject other than 0 or 1, a threshold that is not positive and finite. */
int vilf_track_configure_mask(vilf_handle *h, const vilf_track_mask_params *mp);
/* the fisheye mask, W x H, rows row_stride bytes apart (copied); NULL: none. It applies to both readImage variants and to both detection calls. */
int vilf_track_set_fisheye_mask(vilf_handle *h, const unsigned char *mask, int row_stride);
/* readImage_mask (:212-381) and the updateID loop for one image and its mask image: one chain of launches; the host uploads the image and the mask and downloads
 * the list, which vilf_track_get returns. Invalid argument, nothing changed: a null pointer, a stride below the width. */
int vilf_track_read_image_mask(vilf_handle *h, const unsigned char *img, int row_stride, const unsigned char *mask, int mask_row_stride, double stamp, int *n_out);
/* stateless pieces (they leave the tracked state alone): the erosion of a mask image with the configured radius -> out, rows tight; */
int vilf_track_erode(vilf_handle *h, const unsigned char *mask, int row_stride, unsigned char *out);
/* the probe of n points [n][2] (finite; at most VILF_MAX_FEATURES) in an eroded mask (rows tight) with the configured distance -> static_out [n], 1 = static; */
int vilf_track_probe(vilf_handle *h, const unsigned char *eroded, const float *pts, int n, unsigned char *static_out);
/* rejectWithF_mask on n point pairs, all of them survivors, those with is_static[i] != 0 static -> status_out [n], F_out (row-major), *best_out = the winning k,
 * *n_static_inliers_out = its score over the static pairs. Fewer than 8 static pairs or no valid hypothesis: every status 1, best -1, F 0,
 * n_static_inliers = the number of static pairs; that is no error. Invalid argument, nothing written: as vilf_track_reject_f; */
int vilf_track_reject_f_mask(vilf_handle *h, const float *cur_pts, const float *forw_pts, const unsigned char *is_static, int n, unsigned char *status_out, double F_out[9], int *best_out,
                             int *n_static_inliers_out);
/* vilf_track_detect under an eroded mask (rows tight) as well: "detection under the dynamic mask". Both calls honour the fisheye mask when one is set. */
int vilf_track_detect_masked(vilf_handle *h, const unsigned char *img, const unsigned char *eroded, const float *kept_pts, int n_kept, int n_max, float *pts_out, int *n_out);
/* vilf_set_profiling: the erosion, and the probe with rejectWithF_mask (probe, lift, hypotheses, score, apply), of the last vilf_track_read_image_mask; 0 for a
 * plain frame. In the five stages of vilf_track_profile the mask's upload and the erosion fall into the first, the probe and the rejection into the second. */
int vilf_track_profile_mask(vilf_handle *h, double ms_out[2], long launches_out[2]);

/* ---- Visual start-up: relativePose (≙ Estimator::relativePose, estimator.cpp:461-490, with FeatureManager::getCorresponding, feature_manager.cpp:129-148, and
 *      MotionEstimator::solveRelativeRT, initial/solve_5pts.cpp:193-227; device) ----
 * The first stage of initialStructure: the frame l of the window whose correspondences with the newest frame carry enough parallax, and the relative pose of the
 * two. The reference calls cv::findFundamentalMat(FM_RANSAC, 0.3 / 460, 0.99) on normalised coordinates and cv::recoverPose; OpenCV is not available, so this text
 * fixes the arithmetic itself (deviations: DESIGN.md §3n), tests/startup_reference.py restates it in numpy and the kernels agree with that to the bit. GlobalSFM and
 * the per-frame PnP are not part of it. "fp64, each operation rounded" is as in the tracker's text; a NaN compares false everywhere.
 *   window       n_frames frames 0 .. newest = n_frames - 1 and n_features features in feature order; feature f was first seen in frame start_frame[f] and has
 *                n_obs(f) = first_obs[f + 1] - first_obs[f] observations in consecutive frames, observation o at row first_obs[f] + o of pts: the normalised image
 *                point (x, y) of frame start_frame[f] + o, fp64.
 *   correspondences of the pair (i, newest), i = 0 .. n_frames - 2: feature f belongs to it iff start_frame[f] <= i and start_frame[f] + n_obs(f) - 1 >= newest.
 *                The members are taken in feature order, j = 0 .. m - 1; a_j = the point of frame i, b_j = the point of frame newest, both coordinates rounded
 *                to float32 (the reference goes through cv::Point2f). Everything below is fp64 on these float32 values.
 *   gates        count: m > min_count (20, estimator.cpp:468). parallax: d_j = sqrt(dx dx + dy dy), (dx, dy) = a_j - b_j, fp64, each operation rounded. The sum:
 *                64 partial sums, p_t = the sum from 0.0 of d_j over j = t, t + 64, t + 128, .. < m in ascending order, t = 0 .. 63; then for o = 32, 16, 8, 4, 2, 1:
 *                every p_t <- p_t + p_(t xor o), all t at once (addition commutes, so all 64 end equal). parallax = (p_0 / m) * focal_length (460); 0 if m = 0;
 *                the gate is parallax > min_parallax (30, :481). solve count: m >= min_solve_count (15, solve_5pts.cpp:195; dead behind the count gate with the
 *                defaults, kept because both are parameters) and m >= 8. A pair that fails a gate is not searched: best_k = chosen = -1 and score, F, R, T and the counts of its row are 0.
 *   search       the tracker's rejectWithF paragraphs "sample", "8-point solve" and "score" word for word, with n = m, x = a_j, x' = b_j, K = n_hypotheses
 *                (1 .. VILF_TRACK_MAX_HYPOTHESES, default 512), the seed of pair i = seed + i (uint32, wrapping) and F_THRESHOLD = ransac_threshold (0.3 / 460.0); the
 *                squared threshold is the fp64 product ransac_threshold * ransac_threshold. Winner = the valid hypothesis of the highest score, ties to the lower
 *                k; its inlier mask is the RANSAC mask; no refit (FM_RANSAC has none). No valid hypothesis: the pair fails, best_k = -1.
 *   recoverPose  E = the winner's F as it is (the coordinates are normalised: x'^T E x = 0 with x in frame i, x' in frame newest). G = E^T E, g_pq = sum_r E_rp E_rq
 *                from 0 over r = 0, 1, 2; Jacobi(G, 3) of the tracker's text -> eigenvalues g_ii, eigenvectors the columns of V. i3 = the index of the smallest
 *                g_ii (compared with <, ties and NaNs leave the lower index); r0 < r1 the two other indices; i1 = r1 if g_r1r1 > g_r0r0, else r0; i2 = the other.
 *                v1, v2 = columns i1, i2 of V; v3 = v1 x v2 (c_0 = p_1 q_2 - p_2 q_1, c_1 = p_2 q_0 - p_0 q_2, c_2 = p_0 q_1 - p_1 q_0 for c = p x q, two products
 *                and a subtraction each). For j = 1, 2: w_r = (E_r0 v_j0 + E_r1 v_j1) + E_r2 v_j2, u_j = w / sqrt((w_0 w_0 + w_1 w_1) + w_2 w_2); u3 = u1 x u2.
 *                With U = [u1 u2 u3], V = [v1 v2 v3] both determinants are +1 by construction. R1 = U W V^T: R1_rc = (u2_r v1_c - u1_r v2_c) + u3_r v3_c;
 *                R2 = U W^T V^T: R2_rc = (u1_r v2_c - u2_r v1_c) + u3_r v3_c; t = u3. If any entry of R1, R2 or t is not finite the pair fails (counts 0,
 *                chosen -1, R and T 0). The four candidates in OpenCV's order: 0 (R1, t), 1 (R2, t), 2 (R1, -t), 3 (R2, -t).
 *   cheirality   for candidate (R, t) and pair j, with a = a_j, b = b_j: r_k = (R_k0 a_x + R_k1 a_y) + R_k2; rr = (r_0 r_0 + r_1 r_1) + r_2 r_2;
 *                xx = (b_x b_x + b_y b_y) + 1.0; rx = (r_0 b_x + r_1 b_y) + r_2; rt = (r_0 t_0 + r_1 t_1) + r_2 t_2; xt = (b_x t_0 + b_y t_1) + t_2;
 *                det = rr xx - rx rx; z1 = (rx xt - xx rt) / det; z2 = (rr xt - rx rt) / det: the depths along the two rays that minimise
 *                |z1 R (a, 1) + t - z2 (b, 1)|, in closed form (this replaces OpenCV's 4 x 4 DLT triangulation: a deviation). The pair is good iff
 *                0 < z1 < distance_threshold and 0 < z2 < distance_threshold (50, OpenCV's default in this overload). count_c = the number of good pairs among
 *                the RANSAC inliers. chosen = the first c in the order above with the largest count (OpenCV's >= chain). inlier_cnt = count_chosen; the pair
 *                passes iff inlier_cnt > min_inliers (12, solve_5pts.cpp:221).
 *   output       with (R, t) the chosen candidate, the reference's convention (solve_5pts.cpp:219-220): Rotation = R^T, Translation_r = -((R_0r t_0 + R_1r t_1) + R_2r t_2).
 *                Point of pair j: (z1 a_x, z1 a_y, z1) in the camera of frame i if j is a RANSAC inlier and good under the chosen candidate, else (0, 0, 0).
 *   l            the lowest i whose pair passes every gate, -1 if none does. The reference stops at the first passing i; the pairs do not depend on each other,
 *                so all of them are evaluated and the table of pairs comes with the answer. */
#define VILF_SU_COUNT 1          /* flags of a pair: m > min_count */
#define VILF_SU_PARALLAX 2       /* parallax > min_parallax */
#define VILF_SU_SOLVE_COUNT 4    /* m >= min_solve_count and m >= 8 */
#define VILF_SU_HYPOTHESIS 8     /* a valid hypothesis exists */
#define VILF_SU_FINITE 16        /* the decomposition is finite */
#define VILF_SU_INLIERS 32       /* inlier_cnt > min_inliers */
#define VILF_SU_PASS 63
#define VILF_STARTUP_MAX_WINDOWS 256
typedef struct vilf_startup_params {
    int n_hypotheses; unsigned seed;                                              /* 512, 0 */
    int min_count, min_solve_count, min_inliers, pad_;                            /* 20, 15, 12 */
    double ransac_threshold, focal_length, min_parallax, distance_threshold;      /* 0.3 / 460.0, 460, 30, 50 */
} vilf_startup_params;
void vilf_startup_default_params(vilf_startup_params *p);
typedef struct vilf_startup_window {
    int n_frames, n_features;        /* 2 .. VILF_MAX_FRAMES, 0 .. VILF_MAX_FEATURES */
    const int *start_frame;          /* [n_features] */
    const int *first_obs;            /* [n_features + 1], first_obs[0] = 0, non-decreasing */
    const double *pts;               /* [first_obs[n_features]][2] */
} vilf_startup_window;
typedef struct vilf_startup_result {
    int l, inlier_cnt;               /* l = -1: no pair passes, everything else 0 */
    double R[9], T[3];               /* relative_R (row-major), relative_T of pair l */
} vilf_startup_result;
typedef struct vilf_startup_pair {
    int count, flags, best_k, score; /* m, VILF_SU_*, the winning k or -1, its inliers */
    int cheirality[4];               /* the four candidates' counts */
    int chosen, inlier_cnt;          /* the chosen candidate or -1, its count */
    double parallax;                 /* the number the parallax gate compares */
    double F[9], R[9], T[3];         /* the winner (row-major), Rotation, Translation */
} vilf_startup_pair;
/* relativePose for n_windows independent windows: one chain of launches on the handle's stream (gather, hypotheses, score, pose), the host waits once, one download.
 * out [n_windows]; pairs_out [n_windows][VILF_MAX_FRAMES - 1] or NULL (rows of pairs the window does not have are 0 with best_k = chosen = -1). Invalid argument,
 * nothing written: a null pointer, n_windows < 1 or > VILF_STARTUP_MAX_WINDOWS, n_frames < 2 or > VILF_MAX_FRAMES, n_features < 0 or > VILF_MAX_FEATURES, first_obs
 * that does not start at 0 or decreases, start_frame < 0, start_frame + n_obs > n_frames, a coordinate that is not finite, n_hypotheses outside
 * 1 .. VILF_TRACK_MAX_HYPOTHESES, a threshold, focal length or distance that is not positive and finite, a min_parallax that is not finite, a negative count gate. */
int vilf_startup_relative_pose(vilf_handle *h, const vilf_startup_params *p, int n_windows, const vilf_startup_window *windows, vilf_startup_result *out,
                               vilf_startup_pair *pairs_out);
/* the per-correspondence outputs of the last vilf_startup_relative_pose, each [n_windows][VILF_MAX_FRAMES - 1][VILF_MAX_FEATURES] in correspondence order, 0 behind
 * the pair's count (any may be NULL): the feature index, the mask (bit 0: RANSAC inlier, bit 1: good under the chosen candidate), the points [..][3].
 * n_windows other than the last call's, or no call yet: invalid argument, nothing written. */
int vilf_startup_get_correspondences(vilf_handle *h, int n_windows, int *feature_out, unsigned char *mask_out, double *points_out);
/* vilf_set_profiling: su_gather, su_hypotheses, su_score, su_pose of the calls since the switch was set */
int vilf_startup_profile(vilf_handle *h, double ms_out[4], long launches_out[4]);

/* ---- Visual start-up: GlobalSFM frame chain (≙ GlobalSFM::construct, initial/initial_sfm.cpp:117-217, with triangulatePoint :5-19, solveFrameByPnP :22-72 and
 *      triangulateTwoFrames :74-110; device) ----
 * The second stage of initialStructure: from l, relative_R and relative_T of the first stage, the poses of all frames of the window and the positions of its
 * features in the camera of frame l, the starting value of the full bundle adjustment (:232-310), which is not part of it, as the PnP of the non-key frames
 * (estimator.cpp:305-372) is not. The reference calls Eigen's jacobiSvd and cv::solvePnP; neither is available, so this text fixes the arithmetic (deviations:
 * DESIGN.md §3o), tests/sfm_reference.py restates it in numpy and the kernels agree with that to the bit. Everything is fp64, each operation rounded; a NaN
 * compares false everywhere; "-(x)" negates the rounded x. The window is vilf_startup_window; feature f is seen in frame k iff
 * start_frame[f] <= k < start_frame[f] + n_obs(f), and its point there, p(f, k), is row first_obs[f] + k - start_frame[f] of pts.
 *   poses        (:125-153) c_R[k] (row-major 3 x 3) and c_t[k] are the camera-from-world pose of frame k, world = the camera of frame l; P[k] = [c_R[k] | c_t[k]],
 *                3 x 4. c_R[l] = I, c_t[l] = 0. With R = relative_R and T = relative_T: c_R[newest]_rc = R_cr, c_t[newest]_r = -((R_0r T_0 + R_1r T_1) + R_2r T_2).
 *                (With l = newest - 1 .. 0 < newest the two frames always differ.)
 *   triangulatePoint (:5-19) of the poses P, P' and the points (x, y), (x', y'), fp64 as they are in pts (the reference uses Vector2d): the 4 x 4 matrix A,
 *                A_0c = x P_2c - P_0c, A_1c = y P_2c - P_1c, A_2c = x' P'_2c - P'_0c, A_3c = y' P'_2c - P'_1c (a product and a subtraction each); G = A^T A,
 *                g_pq = the sum from 0.0 of A_rp A_rq over r = 0, 1, 2, 3 in this order, p <= q; Jacobi(G, 4) of the tracker's text; at = the index of the smallest
 *                g_ii (compared with <, ties and NaNs leave the lower index); v = column at of V; the position is (v_0 / v_3, v_1 / v_3, v_2 / v_3). If one of the
 *                three is not finite the feature stays untriangulated at this step (state 0, position 0); a later step may triangulate it. There is no test of
 *                the depth's sign, as in the reference.
 *   triangulateTwoFrames(a, b) (:74-110) for every feature that is not yet triangulated and is seen in both frames: triangulatePoint(P[a], P[b], p(f, a), p(f, b)).
 *   solveFrameByPnP(i, R0, t0) (:22-72) the members are the triangulated features seen in frame i, in feature order, j = 0 .. m - 1; X_j = the position, u_j = p(f, i),
 *                every coordinate of both rounded to float32 and back (the reference goes through cv::Point3f / cv::Point2f). m < warn_pnp_count (15, :45) only
 *                sets a flag; m < min_pnp_count (10, :48) fails the frame, nothing is solved. Otherwise a Levenberg-Marquardt of pnp_iterations (default 10,
 *                1 .. 64) iterations from (R, t) = (R0, t0), lambda = lambda0 (1e-3):
 *     residual   of member j under (R, t): q_r = (R_r0 X_0 + R_r1 X_1) + R_r2 X_2; p_r = q_r + t_r; iz = 1.0 / p_2; xn = p_0 iz; yn = p_1 iz; e_0 = xn - u_x; e_1 = yn - u_y.
 *     Jacobian   for the left perturbation R <- exp(w) R, t <- t + d, the unknowns ordered (w_0, w_1, w_2, d_0, d_1, d_2): c_0 = xn iz, c_1 = yn iz,
 *                J_0 = (-(c_0 q_1), iz q_2 + c_0 q_0, -(iz q_1), iz, 0.0, -c_0), J_1 = (-(iz q_2 + c_1 q_1), c_1 q_0, iz q_0, 0.0, iz, -c_1).
 *     terms      of member j, 28 of them: h_ab = J_0a J_0b + J_1a J_1b for a <= b (a = 0 .. 5, b = a .. 5, in this order: 21), g_a = J_0a e_0 + J_1a e_1 (6),
 *                c = e_0 e_0 + e_1 e_1; two products and an addition each, the structural zeros multiplied like any other number.
 *     sums       each of the 28 separately: 256 partial sums, s_t = the sum from 0.0 of the terms of the members j = t, t + 256, .. < m in ascending order; then
 *                within every group of 64 consecutive t, for o = 32, 16, 8, 4, 2, 1: every s_t <- s_t + s_(t xor o), all at once; then the sum is
 *                ((s_0 + s_64) + s_128) + s_192. H, g and cost are these sums.
 *     solve      Hd = H with every diagonal entry replaced by H_aa + lambda H_aa; b_a = -g_a. LDL^T without pivoting: for j = 0 .. 5: d_j = Hd_jj minus
 *                u_jk L_jk for k = 0 .. j - 1 in ascending order (one subtraction of a rounded product at a time); the step is rejected iff not d_j > 0 for some j
 *                (the candidate is then not evaluated); for i = j + 1 .. 5: u_ij = Hd_ji minus u_ik L_jk for k = 0 .. j - 1 in the same way, L_ij = u_ij / d_j.
 *                y_i = b_i minus L_ik y_k for k = 0 .. i - 1 ascending, i = 0 .. 5; z_i = y_i / d_i; x_i = z_i minus L_ki x_k for k = i + 1 .. 5 ascending,
 *                i = 5 .. 0. (w, d) = (x_0 .. x_2, x_3 .. x_5).
 *     candidate  a_i = 0.5 w_i; n = sqrt(((1.0 + a_0 a_0) + a_1 a_1) + a_2 a_2); the quaternion (s, x, y, z) = (1.0 / n, a_0 / n, a_1 / n, a_2 / n); Q = R(q):
 *                Q_00 = 1.0 - 2.0 (y y + z z), Q_01 = 2.0 (x y - s z), Q_02 = 2.0 (x z + s y), Q_10 = 2.0 (x y + s z), Q_11 = 1.0 - 2.0 (x x + z z),
 *                Q_12 = 2.0 (y z - s x), Q_20 = 2.0 (x z - s y), Q_21 = 2.0 (y z + s x), Q_22 = 1.0 - 2.0 (x x + y y); R'_rc = (Q_r0 R_0c + Q_r1 R_1c) + Q_r2 R_2c;
 *                t'_r = t_r + d_r. Only + - * / sqrt: no sin / cos, so that the restatement and the device can agree to the bit.
 *     accept     cost' = the sum c of the candidate in the order above. The step is accepted iff it was not rejected by a pivot and cost' < cost (a NaN rejects):
 *                (R, t, cost) <- (R', t', cost'), lambda <- lambda / 10.0, accepted + 1. Otherwise lambda <- lambda * 10.0. Every iteration linearises anew at
 *                the current (R, t); there is no convergence test.
 *     result     cost0 = the cost of the first iteration, cost1 = the cost after the last. The frame fails iff an entry of (R, t) or cost1 is not finite
 *                (a cost that is not a number accepts no step, so the pose would be the guess).
 *     row        count = m; flags = VILF_SFM_PNP, with VILF_SFM_FEW iff m < warn_pnp_count, and one of VILF_SFM_FAIL_COUNT (accepted, cost0, cost1 = 0),
 *                VILF_SFM_FAIL_FINITE (accepted, cost0, cost1 as they came out) or VILF_SFM_POSE; the pose in both conventions, 0 unless VILF_SFM_POSE. The rows
 *                of l and newest: count 0, VILF_SFM_FIXED | VILF_SFM_POSE, costs 0, the given pose.
 *   chain        (:156-217) 1. triangulateTwoFrames(l, newest). 2. for i = l + 1 .. newest - 1: solveFrameByPnP(i, P[i - 1]), then triangulateTwoFrames(i, newest).
 *                3. for i = l + 1 .. newest - 1: triangulateTwoFrames(l, i). 4. for i = l - 1 .. 0: solveFrameByPnP(i, P[i + 1]), then triangulateTwoFrames(i, l).
 *                5. every feature that is still untriangulated and has n_obs >= 2: triangulatePoint of its first and last frame and its points there.
 *                The first failing PnP ends the chain (the reference's return false): fail_frame = its frame, ok = 0, the frames not reached and the failing
 *                one keep a pose of 0, step 5 is not run; what was triangulated until then is reported.
 *   output       (:290-303 without the BA in between) Q[k]_rc = c_R[k]_cr, T[k]_r = -((Q_r0 c_t_0 + Q_r1 c_t_1) + Q_r2 c_t_2); per feature state (0 / 1) and the
 *                position in the camera of frame l (what sfm_tracked_points and the BA start from), 0 where state is 0. */
#define VILF_SFM_FIXED 1         /* flags of a frame: l or newest, the pose is given */
#define VILF_SFM_PNP 2           /* solveFrameByPnP was run for this frame */
#define VILF_SFM_FEW 4           /* m < warn_pnp_count ("unstable features tracking", :45) */
#define VILF_SFM_FAIL_COUNT 8    /* m < min_pnp_count: the frame fails */
#define VILF_SFM_FAIL_FINITE 16  /* the pose or cost1 is not finite: the frame fails */
#define VILF_SFM_POSE 32         /* R, t, Q, T hold a pose */
#define VILF_STARTUP_MAX_PROBLEMS 4096
typedef struct vilf_startup_sfm_params {
    int min_pnp_count, warn_pnp_count, pnp_iterations, pad_;       /* 10, 15, 10 */
    double lambda0;                                                /* 1e-3 */
} vilf_startup_sfm_params;
void vilf_startup_default_sfm_params(vilf_startup_sfm_params *p);
typedef struct vilf_startup_frame {
    int count, flags, accepted, pad_;  /* m, VILF_SFM_*, accepted steps */
    double cost0, cost1;
    double R[9], t[3];                 /* c_R, c_t */
    double Q[9], T[3];                 /* the output convention */
} vilf_startup_frame;
typedef struct vilf_startup_structure {
    int ok, fail_frame, n_triangulated, l;   /* fail_frame = -1 unless a PnP failed; l as given */
} vilf_startup_structure;
/* GlobalSFM's chain for n_windows independent windows, rel [n_windows] as vilf_startup_relative_pose returned it: one launch on the handle's stream (a workgroup
 * per window), the host waits once, one download. out [n_windows]; frames_out [n_windows][VILF_MAX_FRAMES] or NULL (rows of frames the window does not have or
 * did not reach are 0). A window with rel.l = -1 is skipped: ok = 0, fail_frame = -1, everything else 0; that is no error. Invalid argument, nothing written:
 * what vilf_startup_relative_pose refuses in the windows, and rel.l < -1 or > n_frames - 2, an entry of rel.R or rel.T that is not finite (with l >= 0),
 * pnp_iterations outside 1 .. 64, a negative count, a lambda0 that is not positive and finite. */
int vilf_startup_sfm(vilf_handle *h, const vilf_startup_sfm_params *p, int n_windows, const vilf_startup_window *windows, const vilf_startup_result *rel,
                     vilf_startup_structure *out, vilf_startup_frame *frames_out);
/* the per-feature outputs of the last vilf_startup_sfm: state [n_windows][VILF_MAX_FEATURES], positions [n_windows][VILF_MAX_FEATURES][3], 0 behind n_features (either
 * may be NULL). n_windows other than the last call's, or no call yet: invalid argument, nothing written. */
int vilf_startup_get_structure(vilf_handle *h, int n_windows, unsigned char *state_out, double *positions_out);
/* solveFrameByPnP alone for n_problems independent problems (1 .. VILF_STARTUP_MAX_PROBLEMS), for the PnP of the non-key frames (estimator.cpp:352 uses a minimum of
 * 6, hence min_count per problem; the parameters' min_pnp_count is not read): the members are the n points in their order, pts3 [n][3] and pts2 [n][2] fp64 and
 * rounded to float32 by the call, (R, t) the guess. out [n_problems]: count = n, flags, accepted, cost0, cost1 and the pose in both conventions (0 for a problem that
 * fails). One launch, a workgroup per problem. Invalid argument, nothing written: a null pointer, n < 0 or > VILF_MAX_FEATURES, min_count < 0, a coordinate or an
 * entry of the guess that is not finite, the parameters as above. */
typedef struct vilf_startup_pnp_problem {
    int n, min_count;
    const double *pts3, *pts2;
    double R[9], t[3];
} vilf_startup_pnp_problem;
int vilf_startup_pnp(vilf_handle *h, const vilf_startup_sfm_params *p, int n_problems, const vilf_startup_pnp_problem *problems, vilf_startup_frame *out);
/* vilf_set_profiling: the chain kernel (vilf_startup_sfm) and the PnP kernel (vilf_startup_pnp) of the calls since the switch was set */
int vilf_startup_sfm_profile(vilf_handle *h, double ms_out[2], long launches_out[2]);

/* ---- Visual start-up: GlobalSFM full BA (≙ initial_sfm.cpp:232-310, ReprojectionError3D initial_sfm.h:25-54; device) ----
 * The third stage of initialStructure: the bundle adjustment over the poses and the positions the frame chain left. The reference hands the problem to Ceres
 * (DENSE_SCHUR, 0.2 s); Ceres is not available, so this text fixes the arithmetic (deviations: DESIGN.md §3p), tests/ba_reference.py restates it in numpy and the
 * kernel agrees with that to the bit. The PnP of the non-key frames (estimator.cpp:305-372) is not part of it. Everything is fp64, each operation rounded; a NaN
 * compares false everywhere; "-(x)" negates the rounded x. Window, "seen" and p(f, k) as in the chain's text; observations and positions are fp64 as they are (the
 * reference passes Vector2d and double position[3]: no float32 rounding, unlike the PnP).
 *   problem      the unknowns are c_R[k], c_t[k] (camera-from-world, world = the camera of l, the chain's convention) and the positions X_f of the features with
 *                state 1, the members. Constant (:248-255): c_R[l], c_t[l], c_t[newest]; c_R[newest] is free. Frame k has n_k free unknowns in the order
 *                (w_0, w_1, w_2, d_0, d_1, d_2): n_l = 0, n_newest = 3 (the rotation), n_k = 6 otherwise; its first has the index o_k = the sum of n_j over j < k;
 *                nc = the sum of all n_k = 6 n_frames - 9 (57 at 11 frames, 3 at 2). Every observation of a member is a residual (:258-273), those in l and newest too.
 *   residual     of member f in frame k, with (R, t) = (c_R[k], c_t[k]), X = X_f, u = p(f, k): the PnP's paragraph "residual" -> q, p, iz, xn, yn, e_0, e_1.
 *   Jacobian     the PnP's c_0, c_1 and J_0, J_1 for the left perturbation R <- exp(w) R, t <- t + d; only the first n_k entries of J_0, J_1 exist for frame k (the
 *                columns of a constant rotation or translation are left out, not multiplied as zeros; frame l has none). The point's: P_0c = iz R_0c - c_0 R_2c,
 *                P_1c = iz R_1c - c_1 R_2c, c = 0, 1, 2 (two products and a subtraction each).
 *   sums over features  "the total over the members (seen in ..)" of a term: 256 partial sums, s_t = the sum from 0.0 of the term over the features f = t, t + 256, .. <
 *                n_features that are members (and seen in ..), ascending; then the butterfly within every 64 consecutive t and ((s_0 + s_64) + s_128) + s_192 as in
 *                the PnP's paragraph "sums". (The stride runs over the feature index, not over a compacted member list: a deviation from the PnP that saves the ranking.)
 *   cost         c_k = the total over the members seen in k of e_0 e_0 + e_1 e_1, k = 0 .. n_frames - 1; cost = the sum from 0.0 of c_k in ascending k.
 *   camera terms of frame k with n_k > 0: U_k,ab = the total over the members seen in k of J_0a J_0b + J_1a J_1b, a <= b < n_k; g_k,a = the total of J_0a e_0 + J_1a e_1.
 *   point terms  of member f, its own sums over the frames k that see it in ascending k, from 0.0: v_cd = the sum of P_0c P_0d + P_1c P_1d, c <= d; gp_c = the sum of
 *                P_0c e_0 + P_1c e_1. Damped: Vd_cc = v_cc + lambda v_cc, Vd_cd = v_cd. LDL^T without pivoting: d_0 = Vd_00; L_10 = Vd_01 / d_0; L_20 = Vd_02 / d_0;
 *                d_1 = Vd_11 - Vd_01 L_10; u = Vd_12 - Vd_02 L_10; L_21 = u / d_1; d_2 = (Vd_22 - Vd_02 L_20) - u L_21. The whole step is rejected iff not d_j > 0 for
 *                some j of some member. The inverse: i_j = 1.0 / d_j; m_10 = -(L_10); m_21 = -(L_21); m_20 = L_21 L_10 - L_20; Vi_22 = i_2; Vi_12 = m_21 i_2;
 *                Vi_02 = m_20 i_2; Vi_11 = i_1 + m_21 Vi_12; Vi_01 = m_10 i_1 + m_21 Vi_02; Vi_00 = (i_0 + m_10 (m_10 i_1)) + m_20 Vi_02; Vi is symmetric.
 *   coupling     of member f and a frame k that sees it: W_ac = J_0a P_0c + J_1a P_1c, a < n_k; Y_ac = (W_a0 Vi_0c + W_a1 Vi_1c) + W_a2 Vi_2c.
 *   reduced system (dense Schur) for frames j <= k with n_j, n_k > 0, a < n_j, b < n_k (and a <= b if j = k): T = the total over the members seen in both of
 *                (Y_a0 W'_b0 + Y_a1 W'_b1) + Y_a2 W'_b2, Y of frame j, W' of frame k. S_(o_j + a)(o_k + b) = Ud - T if j = k, with Ud_ab = U_k,ab + lambda U_k,ab
 *                if a = b, else U_k,ab; -(T) if j < k. r_(o_k + a) = g_k,a minus the total over the members seen in k of (Y_a0 gp_0 + Y_a1 gp_1) + Y_a2 gp_2;
 *                the right-hand side is b_i = -(r_i).
 *   solve        the LDL^T without pivoting of the PnP's paragraph "solve" at the size nc, S read in its upper triangle, the same pivot rule (the step is rejected
 *                iff not d_j > 0 for some j), y and z as there; x_i = z_i minus L_ki x_k for k = nc - 1 .. i + 1 in descending order, i = nc - 1 .. 0 (descending, so
 *                that a finished x_k can be taken out of every row at once; the PnP's text has ascending).
 *   back-substitution of member f: s_c = gp_c, then for every frame k that sees f in ascending k and a = 0 .. n_k - 1 ascending: s_c <- s_c + W_ac x_(o_k + a);
 *                dX_c = -((Vi_c0 s_0 + Vi_c1 s_1) + Vi_c2 s_2).
 *   candidate    frame k with n_k > 0: (w, d) = (x_(o_k) .. x_(o_k + 2), x_(o_k + 3) .. x_(o_k + 5)), d = 0 if n_k = 3; the PnP's paragraph "candidate" gives R'
 *                (and t' = t + d if n_k = 6, t' = t as it is if n_k = 3). X'_f = X_f + dX. Only + - * / sqrt.
 *   iteration    lambda = lambda0 (1e-3). Each of at most ba_iterations (default 20, 1 .. 64) iterations linearises at the current values (cost, camera and point
 *                terms), solves and evaluates cost' of the candidate. The step is accepted iff no pivot rejected it and cost' < cost: the values become the
 *                candidate's, lambda <- lambda / 10.0, accepted + 1; else lambda <- lambda * 10.0. After an accepted step with
 *                cost - cost' <= function_tolerance * cost (1e-6, Ceres's default; cost the one before the step) the loop ends and VILF_BA_CONVERGED is set.
 *   verdict      (replaces :277-289; there is no wall-clock limit where the reference gives Ceres 0.2 s: a deviation.) cost0 = the cost of the first iteration,
 *                cost1 = the cost of the values reached; final_cost = 0.5 cost1 (Ceres's convention); VILF_BA_COST iff final_cost < cost_threshold (5e-3);
 *                VILF_BA_FINITE iff every entry of every c_R[k], c_t[k], every member's position and cost1 are finite. ok iff VILF_BA_FINITE and (VILF_BA_CONVERGED
 *                or VILF_BA_COST); otherwise the window fails (the reference's return false) and still reports what it reached.
 *   output       per frame the pose in both conventions, Q and T by the chain's paragraph "output" (:290-303), 0 for the frames the window does not have; per
 *                feature the state as given and the position, 0 where state is 0. A window with l = -1 or a failed chain (chain_ok = 0) is skipped: everything 0
 *                but l; that is no error. */
#define VILF_BA_CONVERGED 1      /* flags of a window: the function tolerance ended the loop */
#define VILF_BA_COST 2           /* final_cost < cost_threshold */
#define VILF_BA_FINITE 4         /* poses, positions and cost1 are finite */
typedef struct vilf_startup_ba_params {
    int ba_iterations, pad_;                                       /* 20 */
    double lambda0, function_tolerance, cost_threshold;            /* 1e-3, 1e-6, 5e-3 */
} vilf_startup_ba_params;
void vilf_startup_default_ba_params(vilf_startup_ba_params *p);
typedef struct vilf_startup_ba_start {
    int l, chain_ok;                 /* l = -1 or chain_ok = 0: the window is skipped */
    const double *R, *t;             /* [n_frames][9] c_R row-major, [n_frames][3] c_t */
    const unsigned char *state;      /* [n_features], 0 / 1 */
    const double *positions;         /* [n_features][3], read where state is 1 */
} vilf_startup_ba_start;
typedef struct vilf_startup_ba_result {
    int ok, flags, iterations, accepted;        /* VILF_BA_*, iterations run, steps accepted */
    int n_camera, n_members, n_residuals, l;    /* nc, the members, their observations (two residuals each); l as given */
    double cost0, cost1, lambda;                /* lambda as the last iteration left it */
} vilf_startup_ba_result;
typedef struct vilf_startup_ba_frame {
    double R[9], t[3];                 /* c_R, c_t */
    double Q[9], T[3];                 /* the output convention */
} vilf_startup_ba_frame;
/* The BA alone for n_windows independent windows from a given start: one launch on the handle's stream (a workgroup per window), the host waits once, one download.
 * out [n_windows]; frames_out [n_windows][VILF_MAX_FRAMES] or NULL. Invalid argument, nothing written: what vilf_startup_relative_pose refuses in the windows, a null
 * pointer (in a start too, unless the window is skipped or has no features), l < -1 or > n_frames - 2, a state other than 0 / 1, a member with fewer than two
 * observations, an entry of R or t or a member's position that is not finite (in a window that is not skipped), ba_iterations outside 1 .. 64, a lambda0,
 * function_tolerance or cost_threshold that is not positive and finite. */
int vilf_startup_ba(vilf_handle *h, const vilf_startup_ba_params *p, int n_windows, const vilf_startup_window *windows, const vilf_startup_ba_start *start,
                    vilf_startup_ba_result *out, vilf_startup_ba_frame *frames_out);
/* GlobalSFM::construct: the chain, then the BA from its poses and structure, on the handle's stream with no host round trip in between (two launches, the host waits
 * once, one download). out, frames_out as vilf_startup_ba; chain_out [n_windows] and chain_frames_out [n_windows][VILF_MAX_FRAMES] (either may be NULL) as
 * vilf_startup_sfm returns them, so that a caller sees where a failure came from. Invalid argument, nothing written: what vilf_startup_sfm and vilf_startup_ba refuse
 * in their parameters, the windows and rel. */
int vilf_startup_construct(vilf_handle *h, const vilf_startup_sfm_params *sp, const vilf_startup_ba_params *bp, int n_windows, const vilf_startup_window *windows,
                           const vilf_startup_result *rel, vilf_startup_ba_result *out, vilf_startup_ba_frame *frames_out, vilf_startup_structure *chain_out,
                           vilf_startup_frame *chain_frames_out);
/* the per-feature outputs of the last vilf_startup_ba or vilf_startup_construct, as vilf_startup_get_structure */
int vilf_startup_get_ba_structure(vilf_handle *h, int n_windows, unsigned char *state_out, double *positions_out);
/* vilf_set_profiling: su_sfm_ba of the calls since the switch was set (the chain of a vilf_startup_construct counts in vilf_startup_sfm_profile) */
int vilf_startup_ba_profile(vilf_handle *h, double ms_out[1], long launches_out[1]);

/* ---- Feature manager: triangulate (≙ FeatureManager::triangulate, feature_manager.cpp:218-274, with getDepthVector :194-216; device) ----
 * The first half of solveOdometry (estimator.cpp:492-503): the depth of every feature of the window that has none yet, from all its observations. The reference
 * takes the right singular vector of the smallest singular value from Eigen::JacobiSVD; Eigen is not available, so this text fixes the arithmetic as the CPU oracle
 * has it (oracle/sequence.cpp, a one-sided Hestenes Jacobi: the one deliberate deviation; agreement with Eigen is neither measured nor claimed),
 * tests/tri_reference.py restates it and the kernel agrees with that to the bit. Everything is fp64, each operation rounded (no fused multiply-add); a NaN compares
 * false everywhere; "-(x)" negates the rounded x; "the sum from 0.0 of" terms starts at +0.0 and adds the terms in the stated order, the first one too (so that a
 * lone -0.0 becomes +0.0). Matrices are row-major, M_rc = M[3 r + c].
 *   window       n_frames frames with the body positions Ps[k] and rotations Rs[k], the extrinsics tic, ric, and ALL features of f_manager.feature in list order:
 *                feature f was first seen in frame start_frame[f] and has n_obs(f) = first_obs[f + 1] - first_obs[f] observations in consecutive frames,
 *                observation o at row first_obs[f] + o of points: feature_per_frame[o].point = (x, y, z) of frame start_frame[f] + o. z need not be 1.
 *   used         n_obs(f) >= 2 and start_frame[f] < options.window_size - 2 (:223). Only used features are ever touched.
 *   candidate    used and not depth_in[f] > 0 (:226): a depth of 0, a negative one and a NaN are all candidates. Every other feature keeps depth_in, bit for bit.
 *   camera       of frame k: tc_k = Ps[k] + Rs[k] tic, Rc_k = Rs[k] ric, with M v: (M v)_r = (M_r0 v_0 + M_r1 v_1) + M_r2 v_2; u + v by component;
 *                (M N)_rc = the sum from 0.0 of M_rk N_kc over k = 0, 1, 2. The same numbers for every feature of the window.
 *   design matrix of candidate f with i = start_frame[f] (:229-258): for o = 0 .. n_obs(f) - 1, j = i + o (observation 0 goes through the same products; it is not
 *                replaced by the identity): d = tc_j - tc_i; t_r = (Rc_i,0r d_0 + Rc_i,1r d_1) + Rc_i,2r d_2 (= Rc_i^T d); R_rc = the sum from 0.0 of
 *                Rc_i,kr Rc_j,kc over k = 0, 1, 2 (= Rc_i^T Rc_j); P_rc = R_cr for c < 3, P_r3 = -((R_0r t_0 + R_1r t_1) + R_2r t_2) (= [R^T | -(R^T t)]).
 *                n = sqrt((x x + y y) + z z); (f_0, f_1, f_2) = (x / n, y / n, z / n). Rows 2 o and 2 o + 1 of A (2 n_obs(f) x 4, at most 22 x 4):
 *                A_(2o)c = f_0 P_2c - f_2 P_0c, A_(2o+1)c = f_1 P_2c - f_2 P_1c, c = 0 .. 3 (two products and a subtraction each).
 *   right singular vector  V = the 4 x 4 identity. At most 60 sweeps; a sweep visits the pairs (p, q) in the order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3). A pair:
 *                alpha, beta, gamma = the sums from 0.0 of A_rp A_rp, A_rq A_rq, A_rp A_rq over the rows r in ascending order. The pair is skipped iff
 *                |gamma| <= 1e-17 sqrt(alpha beta) or gamma == 0.0. Else zeta = (beta - alpha) / (2.0 gamma); t = sg / (|zeta| + sqrt(1.0 + zeta zeta)) with
 *                sg = 1.0 if zeta >= 0, else -1.0 (a NaN gives -1.0); c = 1.0 / sqrt(1.0 + t t); s = c t; then every row r in ascending order:
 *                (A_rp, A_rq) <- (c A_rp - s A_rq, s A_rp + c A_rq) from the old pair, and the four rows of V the same way. The loop stops after the first sweep
 *                that rotated nothing; sweeps = the sweeps run, that one included (1 .. 60). Winner: n_c = the sum from 0.0 of A_rc A_rc over the rows in ascending
 *                order, c = 0 .. 3; best = 0, bound = +inf; for c = 0 .. 3: if n_c < bound then bound = n_c, best = c (strict: the first wins a tie, a NaN never wins).
 *   result       depth = V_2,best / V_3,best. If depth < 0.1 the depth becomes options.init_depth (:268-271) and VILF_TRI_RESET is set; an inf or a NaN stays as
 *                it is, as in the reference, and VILF_TRI_NONFINITE is set.
 *   getDepthVector  for the used features in feature order, compacted: 1.0 / depth if depth > 0, else 1.0 / options.init_depth, over the depths after triangulation. */
#define VILF_TRI_MAX_WINDOWS 4096
#define VILF_TRI_USED 1          /* flags of a feature: the used rule holds */
#define VILF_TRI_DONE 2          /* it was a candidate: depth_out is the triangulation's */
#define VILF_TRI_RESET 4         /* its depth was < 0.1 and became init_depth */
#define VILF_TRI_NONFINITE 8     /* its depth is inf or NaN and was kept */
typedef struct vilf_tri_window {
    int n_frames, n_features;        /* 2 .. VILF_MAX_FRAMES, 0 .. VILF_MAX_FEATURES */
    const double *Ps, *Rs;           /* [n_frames][3], [n_frames][9] row-major */
    double tic[3], ric[9];
    const int *start_frame;          /* [n_features] */
    const int *first_obs;            /* [n_features + 1], first_obs[0] = 0, non-decreasing */
    const double *points;            /* [first_obs[n_features]][3] */
    const double *depth_in;          /* [n_features] estimated_depth */
    double *depth_out;               /* [n_features]; a feature that is no candidate gets depth_in back, bit for bit */
    double *inv_depth_out;           /* [n_used] getDepthVector, or NULL */
    unsigned char *flags_out;        /* [n_features] VILF_TRI_*, or NULL */
    unsigned char *sweeps_out;       /* [n_features] the sweeps run (1 .. 60), 0 for a feature that is no candidate, or NULL */
} vilf_tri_window;
typedef struct vilf_tri_result { int n_used, n_candidates, n_reset, n_nonfinite; } vilf_tri_result;
/* triangulate + getDepthVector for n_windows independent windows: the host applies the used and the candidate rule while it packs and hands the device ONE dense list
 * of the candidates of all windows; one upload, one chain of two launches on the handle's stream (tri_cameras: the cameras of every window once; tri_solve: a lane
 * per candidate), the host waits once, one download; a call without any candidate launches nothing. out [n_windows]. A feature's result does not depend on the batch it is in or on its place in it, to the bit.
 * Invalid argument, nothing written: a null handle, windows or out, n_windows < 1 or > VILF_TRI_MAX_WINDOWS, n_frames < 2 or > VILF_MAX_FRAMES, n_features < 0 or
 * > VILF_MAX_FEATURES, a null Ps, Rs or first_obs, a null start_frame, depth_in or depth_out with n_features > 0, a first_obs that does not start at 0 or decreases,
 * a used feature with start_frame < 0 or start_frame + n_obs > n_frames, a null points with first_obs[n_features] > 0, an entry of Ps, Rs, tic or ric
 * that is not finite. The points are not screened: what a point that is not finite gives is what the text gives. */
int vilf_features_triangulate(vilf_handle *h, int n_windows, const vilf_tri_window *windows, vilf_tri_result *out);
/* vilf_set_profiling: the time and the number of the kernel launches (two per call that has a candidate) since the switch was set */
int vilf_features_profile(vilf_handle *h, double ms_out[1], long launches_out[1]);

/* ---- Camera-IMU rotation calibration (≙ InitialEXRotation::CalibrationExRotation, initial/initial_ex_rotation.cpp:11-67, with solveRelativeR :69-99,
 *      testTriangulation :101-125 and decomposeE :127-142; called from estimator.cpp:159-175 while ESTIMATE_EXTRINSIC is 2; device) ----
 * The on-line calibration of the camera-IMU rotation ric before any structure exists: every new frame hands in the correspondences of the last two frames and the
 * pre-integrated rotation between them; the calibrator keeps the history of all frames and solves q_c (x) q_ic = q_ic (x) q_imu for q_ic over the whole history.
 * The reference calls cv::findFundamentalMat, cv::SVD, cv::triangulatePoints and Eigen's JacobiSVD; none is available, so this text fixes the arithmetic
 * (deviations: DESIGN.md §3r), tests/exrot_reference.py restates it in numpy and the kernels agree with that to the bit. Everything is fp64, each operation
 * rounded on its own; a NaN compares false everywhere; "-(x)" negates the rounded x. Matrices are row-major; quaternion coefficients are ordered (x, y, z, w).
 * A slot is one calibrator (one sequence, for example): its frame_count (the pushes so far), its ric (I after a reset) and the three histories Rc, Rimu, Rc_g, entry
 * i = 1 .. frame_count. (The reference's entry 0, three identities, is never read.) A push into slot s with the correspondences (a_j, b_j), j = 0 .. m - 1, of the
 * frames (frame_count - 1, frame_count) of the estimator, a_j in the older one, and delta_q:
 *   solveRelativeR (:69-99) every coordinate of a_j and b_j is rounded to float32 (the reference goes through cv::Point2f); all that follows is fp64 on these values.
 *                m < min_corres (9, :71) or m < 8: Rc = I, nothing is searched (VILF_EXROT_COUNT is not set). Otherwise the tracker's rejectWithF paragraphs
 *                "sample", "8-point solve" and "score" word for word, as relativePose does, with n = m, x = a_j, x' = b_j, K = n_hypotheses (1 ..
 *                VILF_TRACK_MAX_HYPOTHESES, default 512), the seed of the push = seed + (the slot's frame_count before the push) (uint32, wrapping) and
 *                F_THRESHOLD = ransac_threshold, its square the fp64 product ransac_threshold * ransac_threshold. Winner = the valid hypothesis of the highest score,
 *                ties to the lower k. The default ransac_threshold is 3.0: the reference calls cv::findFundamentalMat(ll, rr) with its default arguments (FM_RANSAC,
 *                3.0, 0.99) on NORMALISED coordinates, where 3.0 is larger than any epipolar distance. Nearly every valid hypothesis then scores m and the lowest
 *                valid k wins, which is what OpenCV's RANSAC does there too: the first valid sample has every point as an inlier and the iteration stops. A
 *                caller who wants a search that rejects outliers passes something like 0.3 / 460. No valid hypothesis: Rc = I (VILF_EXROT_HYPOTHESIS is not set).
 *                decomposition: E = the winner's F as it is; the recoverPose paragraph of relativePose up to R1, R2 and t = u3. Both determinants are +1 by
 *                construction, so the reference's branch determinant(R1) + 1 < 1e-9 (E <- -E, :83-87) is dead here. An entry of R1, R2 or t that is not finite:
 *                Rc = I (VILF_EXROT_FINITE is not set).
 *   testTriangulation (:101-125) for (R, t') and pair j the depths z1, z2 of relativePose's cheirality paragraph (they replace cv::triangulatePoints on float
 *                matrices: the same deviation as there). The pair is in front iff z1 > 0 and z2 > 0; there is no distance bound. The count runs over ALL m
 *                correspondences, not over the inliers of the search (the reference passes ll, rr whole). front = (c(R1, t), c(R1, -t), c(R2, t), c(R2, -t));
 *                under -t both depths are those under t, negated exactly. ans = R1 (chosen 0) iff max(front_0, front_1) > max(front_2, front_3), else R2
 *                (chosen 1): the reference compares the ratios count / m, which share the denominator. Rc = ans^T (:92-95).
 *   history      Rimu = R(delta_q) by the Q = R(q) formula of the PnP's paragraph "candidate" with (x, y, z, s) = delta_q; no normalisation, as in Eigen's
 *                toRotationMatrix. Rc_g = ric^T Rimu ric with the slot's ric BEFORE this push, two products in this order: T_rc = (ric_0r Rimu_0c + ric_1r Rimu_1c)
 *                + ric_2r Rimu_2c; Rc_g_rc = (T_r0 ric_0c + T_r1 ric_1c) + T_r2 ric_2c. (The reference writes ric.inverse(); ric is R(x)^T of a quaternion that is
 *                unit to rounding, so the transpose is its inverse to rounding: a deviation.) frame_count + 1; (Rc, Rimu, Rc_g) become entry frame_count. Rc_g of
 *                earlier pushes is never recomputed, as in the reference.
 *   quat(M)      Eigen's matrix-to-quaternion (Quaterniond(Matrix3d)): tr = (M_00 + M_11) + M_22. If tr > 0: s = sqrt(tr + 1.0); w = 0.5 s; u = 0.5 / s;
 *                x = (M_21 - M_12) u; y = (M_02 - M_20) u; z = (M_10 - M_01) u. Else i = 0; if M_11 > M_00: i = 1; if M_22 > M_ii: i = 2; j = (i + 1) mod 3,
 *                k = (j + 1) mod 3; s = sqrt(((M_ii - M_jj) - M_kk) + 1.0); q_i = 0.5 s; u = 0.5 / s; w = (M_kj - M_jk) u; q_j = (M_ji + M_ij) u; q_k = (M_ki + M_ik) u,
 *                with (q_0, q_1, q_2) = (x, y, z).
 *   atan2p(y, x) for y, x >= 0, in + - * / sqrt only (see the PnP's "no sin / cos"): swapped = y > x; lo = swapped ? x : y, hi = swapped ? y : x; q = lo / hi, or 0.0
 *                if hi == 0; three times q <- q / (1.0 + sqrt(1.0 + q q)); z = q q; s = c_15; then for n = 13, 11, 9, 7, 5, 3: s <- c_n - z s, with c_n the
 *                fp64 quotient 1.0 / n; s <- 1.0 - z s; r = (q s) 8.0; the result is swapped ? 1.5707963267948966 - r : r.
 *   weights      (:21-31) for EVERY entry i = 1 .. frame_count, every push: r1 = quat(Rc_i), r2 = quat(Rc_g_i), c = conj(r2) = (-x2, -y2, -z2, w2),
 *                d = r1 * c: d_w = ((w1 w_c - x1 x_c) - y1 y_c) - z1 z_c; d_x = ((w1 x_c + x1 w_c) + y1 z_c) - z1 y_c; d_y = ((w1 y_c + y1 w_c) + z1 x_c) - x1 z_c;
 *                d_z = ((w1 z_c + z1 w_c) + x1 y_c) - y1 x_c. angle_i = 57.29577951308232 (2.0 atan2p(sqrt((d_x d_x + d_y d_y) + d_z d_z), |d_w|)), Eigen 3.3's
 *                angularDistance in degrees. weight_i = angle_i > huber_deg (5.0) ? huber_deg / angle_i : 1.0.
 *   system       (:32-59) with (x, y, z, w) = quat(Rc_i): L = [w -z y x; z w -x y; -y x w z; -x -y -z w]; with (x, y, z, w) = quat(Rimu_i):
 *                R = [w z -y x; -z w x y; y -x w z; -x -y -z w]; B_i = weight_i (L - R), a subtraction then a product per entry. G = A^T A of the 4 frame_count x 4
 *                matrix A of the blocks B_i: g_pq, p <= q, is the sum from 0.0 over i ascending and within i over the rows r = 0 .. 3 of B_rp B_rq, a product and
 *                an addition per term. Jacobi(G, 4) of the tracker's text. sigma_k = sqrt(g_kk) if g_kk > 0, else 0.0; they are reported sorted in descending
 *                order. x = the column of V under the smallest g_kk (compared with <, ties and NaNs leave the lower index): the reference's svd.matrixV().col(3).
 *                ric <- R(x)^T, ric_rc = Q_cr of the "candidate" formula with (x, y, z, s) = x, not normalised.
 *   success      ok iff frame_count >= min_frames (10 = WINDOW_SIZE) and the third of the sorted sigmas > min_sigma (0.25): ric_cov(1) of :58-60. The slot keeps
 *                its ric either way; calib_ric is the result's ric where ok is set.
 *   bounds       at most VILF_EXROT_MAX_SLOTS slots; a slot's history holds at most VILF_EXROT_MAX_HISTORY entries. The reference's history grows without bound;
 *                here a push into a full slot is an invalid argument and nothing is written: the caller resets. */
#define VILF_EXROT_COUNT 1        /* flags of a push: m >= min_corres and m >= 8, the pair was searched */
#define VILF_EXROT_HYPOTHESIS 2   /* a valid hypothesis exists */
#define VILF_EXROT_FINITE 4       /* the decomposition is finite: Rc is solveRelativeR's, not the identity */
#define VILF_EXROT_SOLVED 7
#define VILF_EXROT_SKIPPED 8      /* the slot's pair had n = -1: nothing was pushed, the row only reports the slot's frame_count and ric */
#define VILF_EXROT_MAX_SLOTS 256
#define VILF_EXROT_MAX_HISTORY 256
typedef struct vilf_exrot_params {
    int n_hypotheses; unsigned seed;                          /* 512, 0 */
    int min_corres, min_frames;                               /* 9, 10 */
    double ransac_threshold, huber_deg, min_sigma;            /* 3.0, 5.0, 0.25 */
} vilf_exrot_params;
void vilf_exrot_default_params(vilf_exrot_params *p);
typedef struct vilf_exrot_pair {
    int n, pad_;                     /* the correspondences, 0 .. VILF_MAX_FEATURES; -1 skips the slot */
    const double *a, *b;             /* [n][2] normalised image points of the older and of the newer frame (may be NULL with n <= 0) */
    double delta_q[4];               /* the pre-integrated rotation between the two frames (x, y, z, w) */
} vilf_exrot_pair;
typedef struct vilf_exrot_result {
    int frame_count, flags, count, best_k, score;   /* the slot's pushes after this one, VILF_EXROT_*, m (-1 skipped), the winning k or -1, its inliers */
    int front[4];                    /* c(R1, t), c(R1, -t), c(R2, t), c(R2, -t) over all m */
    int chosen, ok, pad_;            /* 0 = R1, 1 = R2, -1 = Rc is the identity; the success rule */
    double Rc[9];                    /* what solveRelativeR returns */
    double angle, weight;            /* of the newest entry, degrees */
    double sigma[4], x[4], ric[9];   /* sorted in descending order; (x, y, z, w); the slot's ric after the push */
} vilf_exrot_result;
/* (re)creates n_slots calibrators on the handle: frame_count 0, ric = I, empty histories. Invalid argument, the existing calibrators kept: n_slots outside
 * 1 .. VILF_EXROT_MAX_SLOTS. */
int vilf_exrot_reset(vilf_handle *h, int n_slots);
/* one push into every slot whose pair has n >= 0: one upload, one chain of three launches on the handle's stream (ex_hypotheses, ex_score, ex_solve: a workgroup
 * per slot), the host waits once, one download. out [n_slots]. A slot's result does not depend on the other slots of the call, to the bit. Invalid argument, nothing
 * written and no state changed: a null pointer (a or b with n > 0 included), n_slots outside 1 .. VILF_EXROT_MAX_SLOTS or other than the last vilf_exrot_reset's
 * (or no reset yet), n < -1 or > VILF_MAX_FEATURES, a coordinate or a delta_q entry that is not finite, a pushed slot that already holds VILF_EXROT_MAX_HISTORY
 * entries, n_hypotheses outside 1 .. VILF_TRACK_MAX_HYPOTHESES, a threshold, huber_deg or min_sigma that is not positive and finite, min_corres or min_frames < 0. */
int vilf_exrot_push(vilf_handle *h, const vilf_exrot_params *p, int n_slots, const vilf_exrot_pair *pairs, vilf_exrot_result *out);
/* the history of a slot: *count_out = frame_count, Rc, Rimu, Rc_g [count][9] and the angles and weights [count] of the slot's last push, entry i at row i - 1.
 * Every array holds VILF_EXROT_MAX_HISTORY rows at the caller's and may be NULL. Invalid argument, nothing written: a null handle or count_out, no reset yet, a slot
 * outside 0 .. n_slots - 1. */
int vilf_exrot_get_history(vilf_handle *h, int slot, int *count_out, double *Rc_out, double *Rimu_out, double *Rcg_out, double *angle_out, double *weight_out);
/* vilf_set_profiling: ex_hypotheses, ex_score, ex_solve of the pushes since the switch was set */
int vilf_exrot_profile(vilf_handle *h, double ms_out[3], long launches_out[3]);

/* ---- Visual loop closure, first stage: key-frame BRIEF and matching (≙ KeyFrame::computeWindowBRIEFPoint, computeBRIEFPoint, searchByBRIEFDes and searchInAera,
 * pose_graph/keyframe.cpp:75-171, with BRIEF::compute, pose_graph/ThirdParty/DVision/BRIEF.cpp:39-106; device) ----
 * What a KeyFrame computes from its image, and the brute-force descriptor search between key frames, over a store of key frames that stays on the device. OpenCV is
 * not available, so this text fixes the arithmetic itself, as the tracker's text does; tests/kf_reference.py restates it in numpy and the kernels agree with that
 * on every integer and every float bit. Agreement with OpenCV's own rasters (GaussianBlur's fixed-point rounding, FAST's pixel order) is neither measured nor
 * claimed. Candidate retrieval (detectLoop's DBoW2 query), PnP-RANSAC, the 4-DoF graph and the relocalisation factors are not part of this stage:
 * the caller names the old key frames, or asks vilf_kf_bow_detect for one (the paragraph "Visual loop closure, candidate retrieval" below).
 *   conventions  images are 8-bit, row-major, W x H, both sides > 21. R(i, n) is the tracker's reflect-101. Points are float32 (x, y) pixel coordinates, finite and
 *                within 1e6 pixels of the origin (anything else is an invalid argument). >> is arithmetic. No floating point in blur, FAST or the search.
 *   pattern      VILF_KF_BITS = 256 tests (x1_i, y1_i, x2_i, y2_i), int, given by the caller in the parameters (the reference reads config/brief_pattern.yml
 *                through BriefExtractor). An entry with |v| > 64 is an invalid argument.
 *   blur         stands for cv::GaussianBlur(9 x 9, sigma = 2) on 8-bit (BRIEF.cpp:60): integer and separable. Taps q = {7, 17, 32, 46, 52, 46, 32, 17, 7}
 *                = rint(256 g_i) of the normalised Gaussian; they sum to 256. h(x, y) = sum_i q_i I(R(x + i - 4, W), y) (at most 65280: 16 bits);
 *                v(x, y) = sum_i q_i h(x, R(y + i - 4, H)); blur(x, y) = (v + 32768) >> 16.
 *   FAST         stands for cv::FAST(image, keypoints, 20, true) (keyframe.cpp:92), type 9-16, on the unblurred image; the threshold t is a parameter, 1 .. 254,
 *                default 20. Circle c_k, k = 0 .. 15: (0,3) (1,3) (2,2) (3,1) (3,0) (3,-1) (2,-2) (1,-3) (0,-3) (-1,-3) (-2,-2) (-3,-1) (-3,0) (-3,1) (-2,2) (-1,3).
 *                Tested pixels p: 3 <= x < W - 3, 3 <= y < H - 3. d_k = I(p) - I(p + c_k). A = the maximum over the 16 cyclic arcs of 9 consecutive k of the
 *                minimum of d_k on the arc; B the same with -d_k. p is a corner iff max(A, B) > t; its score is max(A, B) - 1, the largest threshold at which it
 *                is still a corner (1 .. 254). Every other pixel scores 0. A corner is kept iff its score is strictly greater than the scores of all eight
 *                neighbours: two equal adjacent maxima both go. Key points are emitted in row-major order (y, then x), pt = (x, y) as float32.
 *   descriptor   (BRIEF::compute) for a float32 point (px, py), on the blurred image. For test i: X1 = (int)(px + (float)x1_i), the addition in float32, the
 *                conversion truncating toward zero (so -0.5 gives 0 and passes the range check, as in the reference); Y1, X2, Y2 likewise. Bit i is set iff
 *                0 <= X1, X2 < W and 0 <= Y1, Y2 < H and blur(X1, Y1) < blur(X2, Y2). Layout: four uint64 words per descriptor, bit i in word i / 64 at
 *                position i % 64. The window descriptors are those of the caller's point_2d_uv (sub-pixel points, any position); the key-point descriptors
 *                are those of the FAST points.
 *   lift         (keyframe.cpp:105-112) each FAST point through the tracker's undistortion text with the store's camera, rounded to float32: keypoints_norm.
 *   match        (searchInAera, keyframe.cpp:121-150) for a window descriptor w of the current key frame and an old key frame with descriptors D_0 .. D_(m-1):
 *                (dist, j) = the lexicographic minimum of (popcount(w ^ D_j), j) over the j with popcount(w ^ D_j) < match_max_dist (128: the reference's loop
 *                with bestDist = 128 and a strict <). No such j (m = 0 included): index -1, distance match_max_dist, status 0. Otherwise status = 1 iff
 *                dist < match_accept_dist (80). Outputs per (old key frame, window point): status, the old key point's pt and its lifted point ((0, 0) when
 *                status is 0), j, dist; per old key frame the number of status 1. */
#define VILF_KF_BITS 256
#define VILF_KF_WORDS 4              /* uint64 words of a descriptor */
#define VILF_KF_MAX_OFFSET 64        /* largest |v| of a pattern entry */
#define VILF_KF_MATCH_CHUNK 256      /* kf_match: old descriptors per pass through LDS, 64 for each of the four waves (tests place their edge cases by it) */
#define VILF_KF_MAX_CANDIDATES 256   /* old key frames of one vilf_kf_match */
typedef struct vilf_kf_params {
    int width, height;               /* COL, ROW */
    int fast_threshold;              /* 1 .. 254; 20 (keyframe.cpp:90) */
    int match_max_dist;              /* 0 .. 257; 128 (bestDist, keyframe.cpp:129) */
    int match_accept_dist;           /* 0 .. 257; 80 (keyframe.cpp:142) */
    int pad_;
    double fx, fy, cx, cy;           /* PinholeCamera::Parameters, as vilf_track_params */
    double k1, k2, p1, p2;
    int x1[VILF_KF_BITS], y1[VILF_KF_BITS], x2[VILF_KF_BITS], y2[VILF_KF_BITS];
} vilf_kf_params;
/* the three thresholds at their defaults, everything else 0: the image size, the camera and the pattern are the caller's */
void vilf_kf_default_params(vilf_kf_params *p);
/* the store, hung off the handle and sized here: cap_keyframes key frames, cap_keypoints FAST points over all of them; every key frame has room for
 * VILF_MAX_FEATURES window points. Invalid argument, the handle and an existing store untouched: a null pointer, a side <= 21, a capacity < 1, cap_keypoints > 2^30,
 * a threshold outside its range, a pattern entry with |v| > VILF_KF_MAX_OFFSET, a focal length that is not positive, a camera parameter that is not finite.
 * A second call drops the store and sizes a new one. */
int vilf_kf_create(vilf_handle *h, const vilf_kf_params *p, int cap_keyframes, long cap_keypoints);
/* a key frame from its image (rows row_stride bytes apart) and its window points window_uv [n_window][2] (point_2d_uv), 0 <= n_window <= VILF_MAX_FEATURES: blur,
 * FAST, both sets of descriptors and the lift, all kept on the device. The host reads the number of FAST points once. *index_out = its index,
 * *n_keypoints_out = its FAST points (either may be NULL). Invalid argument, the store as it was: no store, a null image, row_stride < width, n_window out of
 * range, a null window_uv with n_window > 0, a window point outside the conventions, no free key frame, more FAST points than the free key points (never truncated). */
int vilf_kf_add_keyframe(vilf_handle *h, const unsigned char *img, int row_stride, const float *window_uv, int n_window, int *index_out, int *n_keypoints_out);
/* the "load previous keyframe" constructor (keyframe.cpp:44-72): a key frame from stored data, no image. keypoints, keypoints_norm [n_kp][2], descriptors
 * [n_kp][4], window_uv [n_window][2], window_descriptors [n_window][4]; the values are stored as they are. Invalid argument, the store as it was: as above, n_kp < 0,
 * a null array whose count is > 0. */
int vilf_kf_add_loaded(vilf_handle *h, int n_kp, const float *keypoints, const float *keypoints_norm, const unsigned long long *descriptors,
                       int n_window, const float *window_uv, const unsigned long long *window_descriptors, int *index_out);
/* a stored key frame: *n_kp_out, *n_window_out and the arrays in the layouts above (any output may be NULL). cap_kp < its key points with a key-point array asked
 * for, or cap_window < its window points with a window array asked for: invalid argument, nothing written. */
int vilf_kf_get(vilf_handle *h, int index, int cap_kp, float *keypoints, float *keypoints_norm, unsigned long long *descriptors, int *n_kp_out,
                int cap_window, float *window_uv, unsigned long long *window_descriptors, int *n_window_out);
int vilf_kf_size(vilf_handle *h, int *n_out);
/* searchByBRIEFDes (keyframe.cpp:152-171) of key frame cur's window descriptors in the key-point descriptors of n_old key frames (1 .. VILF_KF_MAX_CANDIDATES; an
 * index may repeat and may be cur), all in one launch. With n = the window points of cur: status [n_old][n], pt_old, pt_old_norm [n_old][n][2], best_index,
 * best_dist [n_old][n], n_matched [n_old] (any output may be NULL). Invalid argument, nothing written: no store, cur or an old index out of range, n_old out of
 * range, a null old_index. */
int vilf_kf_match(vilf_handle *h, int cur, int n_old, const int *old_index, unsigned char *status, float *pt_old, float *pt_old_norm, int *best_index,
                  int *best_dist, int *n_matched);
/* stateless pieces (they need the store's parameters and leave its key frames alone): the blurred image, rows tight; */
int vilf_kf_blur(vilf_handle *h, const unsigned char *img, int row_stride, unsigned char *out);
/* the FAST key points of an image in their order, pts_out [cap][2], score_out [cap] (the score byte of each; may be NULL), *n_out of them; more than cap points:
 * invalid argument, nothing written (*n_out included); */
int vilf_kf_fast(vilf_handle *h, const unsigned char *img, int row_stride, int cap, float *pts_out, unsigned char *score_out, int *n_out);
/* the descriptors of n points [n][2] (0 .. 2^20) on the blur of an image -> desc_out [n][4] */
int vilf_kf_brief(vilf_handle *h, const unsigned char *img, int row_stride, const float *pts, int n, unsigned long long *desc_out);
/* vilf_set_profiling: upload + blur, FAST (score, row counts, scan, placement), descriptors + lift, match, download, summed over the calls since the switch was set */
int vilf_kf_profile(vilf_handle *h, double ms_out[5], long launches_out[5]);

/* ---- Visual loop closure, second stage: PnP-RANSAC and the loop decision (≙ KeyFrame::PnPRANSAC and the end of KeyFrame::findConnection,
 * pose_graph/keyframe.cpp:200-256, 401-520; device, the decision on the host) ----
 * What findConnection does after searchByBRIEFDes: the pose of the old key frame from the current key frame's world points and the old key frame's matched lifted
 * points, and the decision whether the two close a loop. cv::solvePnPRansac draws random samples and OpenCV is not available, so the search is a design of this
 * project, as rejectWithF's is; tests/kfloop_reference.py restates this text in numpy and the kernels agree with it on every integer and every float bit up to the
 * pose out (deviations from OpenCV: DESIGN.md §3t). Candidate retrieval (vilf_kf_bow_*, below), optimize4DoF and the relocalisation factors are not part of this
 * stage.
 *   geometry     of a key frame: point_3d [n_window][3], the world points of its window features rounded to float32 (cv::Point3f), and origin_vio_R [9] (row-major),
 *                origin_vio_T [3] in fp64; all finite. The extrinsic qic [9], tic [3] is a parameter of the call. Only the current key frame needs a geometry.
 *   gate         for an old key frame: S = the window points of cur with match status 1 (first stage, paragraph match), in window order, m = |S|. m <= min_loop_num
 *                (25, keyframe.h:16; :406): no PnP, no loop. Member j of S: X_j = point_3d of cur, u_j = the matched old key point's keypoints_norm, both float32.
 *   guess        of cur, fp64, every product and sum rounded on its own, three-term sums left to right: R_w_c = origin_vio_R qic (entry (r, c) =
 *                (R_r0 q_0c + R_r1 q_1c) + R_r2 q_2c); T_w_c_r = origin_vio_T_r + ((R_r0 tic_0 + R_r1 tic_1) + R_r2 tic_2); R0 = R_w_c^T;
 *                t0_r = -((R0_r0 T_w_c_0 + R0_r1 T_w_c_1) + R0_r2 T_w_c_2) (:212-216).
 *   hypotheses   K = n_hypotheses (1 .. VILF_TRACK_MAX_HYPOTHESES, default 256), no adaptive stopping. The sample of hypothesis k is the tracker's rejectWithF
 *                paragraph "sample" with 5 slots in place of 8 and n = m; the seed of an old key frame is seed + (its key-frame index) (uint32, wrapping): the
 *                index, not the position in the call, so a candidate's result does not depend on its neighbours in the call. Each hypothesis solves the start-up's
 *                paragraph solveFrameByPnP ("residual", "Jacobian", "terms", "solve", "candidate", "accept") on its 5 members in slot order, from (R0, t0), with
 *                lambda0 and hyp_iterations iterations (default 5, 1 .. 64), with one difference: each of the 28 sums, and the candidate's cost, is a plain sum
 *                from 0.0 in slot order (no 256 partial sums, no butterfly). There is no count gate and a hypothesis is invalid (score -1) unless the nine R and
 *                three t it ends with are finite. This is OpenCV 2.4's solvePnPRansac (iterative solvePnP on 5-point samples from the extrinsic guess), which the
 *                reference's CV_MAJOR_VERSION < 3 branch calls; OpenCV 3.x runs EPnP on the sample instead.
 *   score        with (p_2, e_0, e_1) of the paragraph "residual" (p_2 = q_2 + t_2): member j is an inlier of (R, t) iff p_2 > 0 and e_0 e_0 + e_1 e_1 <= thr2,
 *                thr2 = reproj_threshold * reproj_threshold in fp64 (default 10.0 / 460.0, :232); a NaN compares false. (OpenCV has no p_2 > 0 test: it is added
 *                on purpose.) Score = the number of inliers over S. The winner is the valid hypothesis of the highest score, ties to the lower k. No valid
 *                hypothesis: best_k = -1, every status 0, no loop.
 *   refit        the status mask is the winner's (OpenCV 3.x reports the model's inliers and refits; so does this). The refit is solveFrameByPnP word for word, 256
 *                partial sums and butterfly included, with no count gate, on the inliers in S order, from the winner's pose, with lambda0 and refine_iterations (10,
 *                1 .. 64). If it ends not finite (its cost, R or t), the pose is the winner's and VILF_KFL_REFIT_DROPPED says so; cost0, cost1 and accepted are the
 *                refit's either way.
 *   pose out     (:245-254) R_w_c_old = R^T; T_w_c_old_r = -((R_0r t_0 + R_1r t_1) + R_2r t_2); PnP_R_old = R_w_c_old qic^T (entry (r, c) =
 *                (W_r0 q_c0 + W_r1 q_c1) + W_r2 q_c2); PnP_T_old_r = T_w_c_old_r - ((P_r0 tic_0 + P_r1 tic_1) + P_r2 tic_2), P = PnP_R_old. On the device, fp64,
 *                each operation rounded.
 *   decision     (:472-487) on the host in fp64 after the download, only if the inlier count is > min_loop_num. relative_t = PnP_R_old^T (origin_vio_T - PnP_T_old);
 *                relative_q = the quaternion of PnP_R_old^T origin_vio_R by Eigen's rule (trace > 0: from sqrt(trace + 1); else around the largest diagonal
 *                entry), as (w, x, y, z); relative_yaw = normalizeAngle(yaw(origin_vio_R) - yaw(PnP_R_old)) in degrees, yaw(R) = atan2(R_10, R_00) * 180 / pi
 *                (Utility::R2ypr), normalizeAngle(a) = a - 360 floor((a + 180) / 360) for a > 0, else a + 360 floor((-a + 180) / 360). Loop iff
 *                |relative_yaw| < max_yaw (30.0) and |relative_t| < max_dist (20.0). atan2 is the host's libm: bit agreement with numpy is not claimed here. */
#define VILF_KFL_GATE 1              /* m <= min_loop_num: no PnP; the row is 0 apart from n_matched and this flag */
#define VILF_KFL_NO_HYPOTHESIS 2     /* no valid hypothesis */
#define VILF_KFL_REFIT 4             /* the pose is the refit's */
#define VILF_KFL_REFIT_DROPPED 8     /* the refit ended not finite: the pose is the winner's */
#define VILF_KFL_LOOP 16             /* has_loop */
typedef struct vilf_kf_loop_params {
    int n_hypotheses;                /* 1 .. VILF_TRACK_MAX_HYPOTHESES; 256 */
    unsigned seed;
    int hyp_iterations;              /* 1 .. 64; 5 */
    int refine_iterations;           /* 1 .. 64; 10 */
    int min_loop_num;                /* >= 5; 25 (MIN_LOOP_NUM) */
    int pad_;
    double lambda0;                  /* 1e-3 */
    double reproj_threshold;         /* 10.0 / 460.0 */
    double max_yaw, max_dist;        /* 30.0 degrees, 20.0 */
    double qic[9], tic[3];           /* the camera-IMU extrinsic; identity and 0 by default */
} vilf_kf_loop_params;
typedef struct vilf_kf_loop_result {
    int n_matched, n_inliers, best_k, flags, has_loop, accepted;
    double R[9], t[3];               /* the camera pose of the old key frame (world to camera) */
    double PnP_R_old[9], PnP_T_old[3];
    double relative_t[3], relative_q[4], relative_yaw;      /* with more than min_loop_num inliers, else 0; q as (w, x, y, z) */
    double cost0, cost1;             /* the refit's first and last cost */
} vilf_kf_loop_result;
void vilf_kf_default_loop_params(vilf_kf_loop_params *p);
/* the geometry of stored key frame `index` (from vilf_kf_add_keyframe or vilf_kf_add_loaded): point_3d [n_window][3] of its window points, origin_vio_R [9],
 * origin_vio_T [3]. A second call replaces the geometry. Invalid argument, the store as it was: no store, index out of range, a null point_3d with n_window > 0, a
 * null vio_R or vio_T, a value that is not finite. */
int vilf_kf_set_geometry(vilf_handle *h, int index, const float *point_3d, const double vio_R[9], const double vio_T[3]);
/* findConnection of key frame cur against n_old old key frames (as vilf_kf_match: an index may repeat): one upload, one chain of launches on the handle's stream
 * (match, gather, hypotheses, score, refine), one wait, one download, then the decision on the host. out [n_old]; with n = the window points of cur, status_out
 * [n_old][n] (the inlier mask, over the window points) and pt_old_norm_out [n_old][n][2] (the first stage's matched lifted points) may be NULL. Old key frames need
 * no geometry. Invalid argument, nothing written: anything vilf_kf_match refuses, a null p or out, cur without geometry, a parameter outside its range or not finite,
 * a threshold, lambda0, max_yaw or max_dist that is not positive, min_loop_num < 5 (the sample needs m > min_loop_num >= 5). */
int vilf_kf_find_connection(vilf_handle *h, const vilf_kf_loop_params *p, int cur, int n_old, const int *old_index, vilf_kf_loop_result *out,
                            unsigned char *status_out, float *pt_old_norm_out);
/* vilf_set_profiling: gather, hypotheses, score, refine, download of the vilf_kf_find_connection calls since the switch was set (their match is booked in
 * vilf_kf_profile's slot) */
int vilf_kf_loop_profile(vilf_handle *h, double ms_out[5], long launches_out[5]);

/* ---- Visual loop closure, third stage: the 4-DoF pose graph (≙ PoseGraph::optimize4DoF, pose_graph/pose_graph.cpp:406-582, with FourDOFError, FourDOFWeightError
 * and AngleLocalParameterization, pose_graph/pose_graph.h:101-250; device, the drift on the host) ----
 * What consumes the second stage's loop_info: yaw and translation of the key frames between the earliest looped key frame and the newest one are re-estimated from
 * the VIO's own relative motion (sequential edges) and the verified loops. A pure function of its arguments: it is not tied to the key-frame store. The reference
 * hands the problem to Ceres, which cannot be built here, so this text fixes the arithmetic itself: the residuals and the graph are the reference's, the minimiser is
 * Ceres's Levenberg-Marquardt as its documentation states it. tests/pg4_reference.py restates this text in numpy; tests/pg4_exact.py is the 40-digit yardstick both
 * are measured against. Agreement with Ceres itself is neither measured nor claimed. The relocalisation factors, candidate retrieval (vilf_kf_bow_*,
 * below) and saving the graph are not part of this stage.
 *   nodes        n key frames in order (the reference's local_index). Unknowns of node k: yaw_k in degrees and t_k [3], starting at yaw(vio_R_k) and vio_T_k. pitch_k
 *                and roll_k come from R2ypr(vio_R_k) (Utility::R2ypr, degrees, on the device) and stay constant. fixed[k] != 0 stands for SetParameterBlockConstant
 *                (:476-480: the first node and every node of sequence 0); fixed[0] must be set. Columns of fixed nodes carry no unknowns.
 *   angles       NormalizeAngle(a) = a - 360 for a > 180, a + 360 for a < -180, else a (pose_graph.h:88-99: one turn at the most).
 *                R(y, p, r) = ypr2R(y, p, r) = Rz(y) Ry(p) Rx(r), degrees (YawPitchRollToRotationMatrix).
 *   sequential   (:483-498) for node i and j = 1 .. VILF_PG4_BAND, if i - j >= 0 and sequence[i] == sequence[i - j]: an edge (from, to) = (i - j, i) with
 *                rel_t = vio_R_(i-j)^T (vio_T_i - vio_T_(i-j)) (the matrix as given, not rebuilt from its angles), rel_yaw = yaw_i - yaw_(i-j) at the start, not
 *                normalised, weight w = 1, no loss.
 *   loops        (:502-517) loops[l] = {from, to, rel_t, rel_yaw}, 0 <= from < to < n; several may share an endpoint or repeat, and a loop may lie inside the band.
 *                w = loop_yaw_scale (0.1: the / T(10.0) of FourDOFWeightError), loss Huber(a = huber).
 *   residual     of an edge (i, j) = (from, to), pitch and roll those of i: r[0..2] = R(yaw_i, pitch_i, roll_i)^T (t_j - t_i) - rel_t,
 *                r[3] = w NormalizeAngle(yaw_j - yaw_i - rel_yaw).
 *   Jacobian     analytic. d r[0..2] / d yaw_i = (pi / 180) (d R / d y)^T (t_j - t_i) (the yaw is in degrees), d r[0..2] / d t_i = -R^T, d r[0..2] / d t_j = R^T,
 *                d r[3] / d yaw_i = -w, d r[3] / d yaw_j = w (NormalizeAngle has derivative 1). Columns of fixed nodes are zero.
 *   loss         s = |r|^2 of the block. No loss: rho = s. Huber: rho = s, rho' = 1 for s <= a^2, else rho = 2 a sqrt(s) - a^2, rho' = a / sqrt(s); the block's residual
 *                and Jacobian rows are scaled by sqrt(rho'), with no second-order correction (Ceres applies none when rho'' <= 0). cost = 1/2 sum rho.
 *   step         with J, r the robustified rows over the free columns: H = J^T J, g = J^T r; (H + diag(H) / mu) delta = -g. Ceres's Jacobi scaling and its clamp of the
 *                scaled diagonal to 1e-6 are left out; the two coincide where no column norm is below about 1e-3, which holds whenever a free node has an edge (the
 *                yaw row alone gives a column norm of 1 for a sequential edge and loop_yaw_scale for a loop). Candidate: yaw <- NormalizeAngle(yaw + delta),
 *                t <- t + delta. model = -(delta^T g + 1/2 |J delta|^2), rho = (cost - cost') / model.
 *   rule         mu = initial_radius, factor = 2. At the start: max |g| <= gradient_tolerance ends the run before any attempt (VILF_PG4_GRADIENT). Otherwise, while no
 *                flag is set: if iterations == max_iterations, VILF_PG4_MAX_ITERATIONS; else one attempt (every attempt counts as an iteration). A non-positive
 *                pivot anywhere in the solve, or a candidate cost that is not finite, rejects the attempt (pivot_rejections; history: cost' = cost, rho = 0,
 *                accepted = -1). Otherwise the step is accepted iff rho > min_relative_decrease. Accepted: mu = min(mu / max(1/3, 1 - (2 rho - 1)^3), max_radius),
 *                factor = 2, the candidate becomes the state, and the run ends on any of cost - cost' <= function_tolerance cost (VILF_PG4_FUNCTION), max |g| of the
 *                new state <= gradient_tolerance (VILF_PG4_GRADIENT), |delta| <= parameter_tolerance (|x| + parameter_tolerance) (VILF_PG4_PARAMETER; |x| the 2-norm
 *                of the free unknowns before the step, yaw in degrees). Rejected: mu /= factor, factor *= 2, and mu < min_radius ends the run (VILF_PG4_RADIUS).
 *   result       iterations, accepted, pivot_rejections, flags (the rules that ended the run, and VILF_PG4_FINITE iff every output is finite), cost0, cost1, the last
 *                radius. ypr_out = (yaw, pitch, roll), R_out = ypr2R of it, on the device. The drift of the last node (:552-560), on the host in fp64 after the
 *                download: yaw_drift = yaw(R_out[n-1]) - yaw(vio_R[n-1]) with yaw(R) = atan2(R_10, R_00) 180 / pi, r_drift = ypr2R(yaw_drift, 0, 0),
 *                t_drift = t_out[n-1] - r_drift vio_T[n-1]. history_out [max_iterations][5], row it = {cost, cost', rho, mu before the attempt, accepted} of attempt
 *                it; rows from `iterations` on are not written.
 *   solver       nodes in groups of four: with VILF_PG4_BAND = 4 the sequential part of H is block tridiagonal in 16 x 16 blocks. The chain (sequential edges, and
 *                diag(H) / mu with the loops' share of the diagonal) is factorised block by block; the loop edges enter as a rank 4 n_loops update (Woodbury) whose
 *                4 n_loops x 4 n_loops capacitance block goes through the dense Cholesky of the large-window path. Sums run in a fixed order: no float atomics, a
 *                result does not depend on the schedule. The host waits once per attempt. */
#define VILF_PG4_BAND 4
#define VILF_PG4_MAX_ITERATIONS_LIMIT 64
#define VILF_PG4_MAX_ITERATIONS 1    /* flags: iterations reached max_iterations */
#define VILF_PG4_FUNCTION 2
#define VILF_PG4_GRADIENT 4
#define VILF_PG4_PARAMETER 8
#define VILF_PG4_RADIUS 16
#define VILF_PG4_FINITE 32
typedef struct vilf_pg4_params {
    int max_iterations;              /* 0 .. 64; 5 (options.max_num_iterations). 0 evaluates the cost and returns the start */
    int pad_;
    double initial_radius;           /* 1e4 */
    double max_radius, min_radius;   /* 1e16, 1e-32 */
    double min_relative_decrease;    /* 1e-3 */
    double function_tolerance, gradient_tolerance, parameter_tolerance;   /* 1e-6, 1e-10, 1e-8 */
    double huber;                    /* 0.1 (ceres::HuberLoss(0.1)) */
    double loop_yaw_scale;           /* 0.1 */
} vilf_pg4_params;
typedef struct vilf_pg4_loop {
    int from, to;                    /* 0 <= from < to < n: the old key frame and the one that found it */
    double rel_t[3], rel_yaw;        /* loop_info's relative_t and relative_yaw (degrees) */
} vilf_pg4_loop;
typedef struct vilf_pg4_result {
    int iterations, accepted, pivot_rejections, flags;
    double cost0, cost1, radius;
    double yaw_drift, r_drift[9], t_drift[3];
} vilf_pg4_result;
void vilf_pg4_default_params(vilf_pg4_params *p);
/* vio_R [n][9] (row-major), vio_T [n][3], sequence [n], fixed [n], loops [n_loops] (may be NULL with n_loops == 0) -> t_out [n][3], ypr_out [n][3], R_out [n][9],
 * *result; history_out [max_iterations][5] may be NULL. Invalid argument, nothing written and the handle good for the next call: a null pointer among the required
 * arguments, n < 1, fixed[0] == 0, n_loops < 0, an input that is not finite, a loop with from >= to or an index out of range, max_iterations outside 0 .. 64, a
 * radius, huber or loop_yaw_scale that is not positive and finite, a tolerance or min_relative_decrease that is negative or not finite. Unsupported, before anything
 * is enqueued: 4 n_loops above what the dense Cholesky takes (12288). */
int vilf_pg4_optimize(vilf_handle *h, const vilf_pg4_params *p, int n, const double *vio_R, const double *vio_T, const int *sequence, const int *fixed,
                      int n_loops, const vilf_pg4_loop *loops, double *t_out, double *ypr_out, double *R_out, vilf_pg4_result *result, double *history_out);
/* vilf_set_profiling: upload + first linearisation, chain factor + chain solve, capacitance + dense solve, step + candidate linearisation + decision, download,
 * summed over the calls since the switch was set */
int vilf_pg4_profile(vilf_handle *h, double ms_out[5], long launches_out[5]);

/* ---- Visual loop closure, candidate retrieval: the DBoW2 query of detectLoop (≙ PoseGraph::detectLoop and addKeyFrameIntoVoc, pose_graph/pose_graph.cpp:307-404,
 * with TemplatedVocabulary::transform, ThirdParty/DBoW/TemplatedVocabulary.h:1065-1121 and :1217-1258, BowVector::addWeight, addIfNotExist and normalize,
 * BowVector.cpp:34-84, and TemplatedDatabase::queryL1, TemplatedDatabase.h:656-723; device, the decision on the host) ----
 * The stage that names the old key frame which the other three verify and use. It reads the key-point descriptors of the key-frame store, which lie on the device in
 * the layout DBoW2 uses (boost::dynamic_bitset from the four blocks, TemplatedVocabulary.h:1541). Everything is integer Hamming distances and fp64 additions,
 * subtractions and one division in a fixed order; tests/bow_reference.py restates this text in plain Python and the kernels agree with it on every integer and every
 * float bit.
 *   vocabulary   the caller's file (estimator.load_vocabulary reads the VINS binary layout): k, L, scoringType, weightingType, nNodes node records (nodeId, parentId,
 *                weight, descriptor[4]) and nWords word records (nodeId, wordId), as VINSLoop::Vocabulary holds them (ThirdParty/VocabularyBinary.hpp). The root is
 *                node 0 and has no record. A node's children are ordered by their position in the node array (loadBin, TemplatedVocabulary.h:1529-1538:
 *                children.push_back in file order); this order decides ties. A leaf is a node without children (isLeaf); the tree may be unbalanced, and a node may
 *                have any number of children >= 1: k and L are not used. Invalid argument, the store untouched: nNodes or nWords < 1, node ids that are not a
 *                permutation of 1 .. nNodes, a parent that does not exist (or is the node itself), a node that the root does not reach, a leaf without a word, a
 *                word on an inner node, a word id outside 0 .. nWords - 1 or used twice, a leaf named by two words, a weight that is negative or not finite, a
 *                leaf deeper than VILF_BOW_MAX_DEPTH (the root's children have depth 1), a weightingType outside 0 .. 3 or a scoringType outside 0 .. 5.
 *                scoringType other than L1_NORM (0) is VILF_ERR_UNSUPPORTED. The four weightings TF_IDF (0), TF (1), IDF (2), BINARY (3) are served; the weights
 *                are the file's, as loadBin leaves them. On upload the host renumbers the nodes breadth-first: the children of a node lie side by side on the
 *                device in their order, with descriptors, word id and weight in arrays of their own. The caller's ids never reach a kernel.
 *   transform    of one descriptor f (:1217-1258): start at the root; among the node's children c_0 .. c_(m-1) in their order take the lexicographic minimum of
 *                (popcount(f ^ D_(c_j)), j): the reference's strict < with the first child as the start. Repeat from that child until it is a leaf: the result is
 *                (word_id, weight) of the leaf.
 *   vector       of a key frame (:1065-1121), over its key-point descriptors in their order. TF_IDF and TF: every descriptor whose weight is > 0 adds its weight to
 *                its word's value (addWeight): a word seen c times holds ((w + w) + w) ..., c - 1 rounded additions, not c w. IDF and BINARY: the value is w once
 *                (addIfNotExist). The vector is sorted by word id. norm = the sum of |value| in ascending word order from 0.0, one rounding per addition; if
 *                norm > 0 every value is divided by norm (normalize, BowVector.cpp:62-84). A key frame without key points, or with stopped words only (weight 0),
 *                has an empty vector and is an entry all the same.
 *   database     entry e is key frame e of the store; entries are added in key-frame order: adding or detecting key frame cur while the database holds a number of
 *                entries other than cur is an invalid argument (the reference's EntryId is its own counter; tying it to the key-frame index is this project's
 *                constraint). The vector of key frame e occupies rows kp_off .. kp_off + n_bow - 1 of two store-sized arrays (word id, value), n_bow <= n_kp.
 *                use_di is false in the reference (pose_graph.cpp:41): no direct index, no feature vectors.
 *   query        (queryL1) of vector v against n_entries entries with max_id: entry e is eligible iff e < max_id or max_id == -1 or e == n_entries - 1 (:679: the
 *                strict < despite the header's comment, the all-pass value -1 which frame_index - 50 takes at frame 49, and the newest entry always, which is why
 *                ret[0] is "the neighbour" in detectLoop). For an eligible entry s_e = the sum over the words common to v and the entry, in ascending word id, from
 *                the first term, of (fabs(q - d) - fabs(q)) - fabs(d). An entry without a common word is no result. The results are ordered by (s_e ascending, e
 *                ascending): std::sort leaves equal scores in no defined order, sending them to the lower id is this project's choice. The list is cut to
 *                max_results, then Score = -s_e / 2.0.
 *   decision     (pose_graph.cpp:351-387) on the host after the download. max_id = frame_index - min_gap. find_loop iff ret[0].Score > neighbour_score and some
 *                ret[i].Score > loop_score with i >= 1. If find_loop and frame_index > min_gap: min_index = -1; for i = 0 ..: if min_index == -1 or (ret[i].Id <
 *                min_index and ret[i].Score > loop_score) then min_index = ret[i].Id; the loop index is min_index (ret[0] seeds it whatever its score). Otherwise -1. */
#define VILF_BOW_MAX_DEPTH 16        /* deepest leaf of a vocabulary */
#define VILF_BOW_MAX_RESULTS 16      /* largest max_results */
#define VILF_BOW_LDS_WORDS 2048      /* bow_score: a query vector of up to this many words is kept in LDS (24 KB), a longer one is read from global memory */
#define VILF_BOW_L1_NORM 0
#define VILF_BOW_TF_IDF 0
#define VILF_BOW_TF 1
#define VILF_BOW_IDF 2
#define VILF_BOW_BINARY 3
typedef struct vilf_bow_node { int nodeId, parentId; double weight; unsigned long long descriptor[4]; } vilf_bow_node;     /* VINSLoop::Node, 48 bytes */
typedef struct vilf_bow_word { int nodeId, wordId; } vilf_bow_word;                                                        /* VINSLoop::Word */
typedef struct vilf_bow_vocabulary {
    int k, L, scoringType, weightingType, nNodes, nWords;
    const vilf_bow_node *nodes;      /* [nNodes], in file order */
    const vilf_bow_word *words;      /* [nWords] */
} vilf_bow_vocabulary;
typedef struct vilf_bow_params {
    int max_results;                 /* 1 .. VILF_BOW_MAX_RESULTS; 4 (pose_graph.cpp:322) */
    int min_gap;                     /* >= 0; 50 (:322, :376) */
    double neighbour_score;          /* 0.05 (:351); not NaN */
    double loop_score;               /* 0.015 (:355, :381); not NaN */
} vilf_bow_params;
typedef struct vilf_bow_result {
    int loop_index;                  /* detectLoop's return value */
    int find_loop;
    int n_results;                   /* ret.size() */
    int n_words;                     /* size of the query vector */
    int id[VILF_BOW_MAX_RESULTS];    /* ret[i].Id, the rest -1 */
    double score[VILF_BOW_MAX_RESULTS];      /* ret[i].Score, the rest 0 */
} vilf_bow_result;
void vilf_kf_bow_default_params(vilf_bow_params *p);
/* the vocabulary of the store's database: validated on the host, renumbered and uploaded. It needs a store, drops an existing database (size 0) and replaces an
 * existing vocabulary; vilf_kf_create drops both with the store, vilf_reset leaves both alone. Every call below is an invalid argument with nothing written without
 * a store or without a vocabulary. */
int vilf_kf_bow_set_vocabulary(vilf_handle *h, const vilf_bow_vocabulary *v);
/* addKeyFrameIntoVoc (:391-404): the vector of stored key frame `index`, which must be the database's size, becomes its entry */
int vilf_kf_bow_add(vilf_handle *h, int index);
/* the same for key frames first .. first + n - 1 (first = the database's size, n >= 0, all in the store): ONE chain of launches over all their descriptors
 * (transform, sort, compact), one wait. Entry for entry equal to n single adds, to the bit. */
int vilf_kf_bow_add_range(vilf_handle *h, int first, int n);
/* detectLoop (:307-389) of stored key frame cur = the database's size: its vector, the query against the cur entries before it, the entry added, then the decision.
 * Invalid argument, nothing written, the database as it was: a null p or out, cur other than the size or outside the store, a parameter outside its range. */
int vilf_kf_bow_detect(vilf_handle *h, const vilf_bow_params *p, int cur, vilf_bow_result *out);
/* the replay over a database that holds key frames 0 .. first + n - 1 already: out[i] is what vilf_kf_bow_detect returned, or would have returned, for key frame
 * first + i on its arrival (n_entries = first + i). All queries go in one chain of launches; the database is not touched. */
int vilf_kf_bow_detect_range(vilf_handle *h, const vilf_bow_params *p, int first, int n, vilf_bow_result *out);
/* the stored vector of entry `index`: *n_out words, word_out and value_out [cap] (either may be NULL). cap < its words with an array asked for: invalid argument. */
int vilf_kf_bow_get(vilf_handle *h, int index, int cap, int *word_out, double *value_out, int *n_out);
/* stateless: (word_id, weight) of n descriptors [n][4] (0 .. 2^24); it needs the vocabulary and leaves the database alone */
int vilf_kf_bow_transform(vilf_handle *h, const unsigned long long *desc, int n, int *word_out, double *weight_out);
int vilf_kf_bow_size(vilf_handle *h, int *n_out);
/* vilf_set_profiling: transform, sort + compact, score, select, download, summed over the calls since the switch was set */
int vilf_kf_bow_profile(vilf_handle *h, double ms_out[5], long launches_out[5]);
#ifdef __cplusplus
}
#endif
#endif /* VILFUSION_H */
