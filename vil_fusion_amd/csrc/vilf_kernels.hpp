// vilf_kernels.hpp — the launch contract of every kernel that is defined in one translation unit and launched from another (vilf_kernels.hip, vilf_marg.hip and
// vilf_host.hip define; vilf_api.hip, vilf_lw.hip and vilf_init.hip launch). Per kernel: its declaration (the definers include this header too, so the compiler compares
// declaration with definition — the extern "C" ones would link whatever their arguments), its workgroup size (__launch_bounds__ and the launch read the same name) and,
// where it takes dynamic LDS, the layout as offsets in doubles plus the total. The kernel carves s_dyn with the offsets, the host passes the total.
// The asserts on the totals see the dynamic part only: static __shared__ arrays come on top (kernel_resources.json, written by the build, has them per kernel).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/vilfusion.h"
#include "vilf_batch.hpp"

#define VILF_MAX_FEATURES_DEV 1000      // per-feature LDS arrays of k_solve and k_marg_schur
static_assert(VILF_MAX_FEATURES_DEV == VILF_MAX_FEATURES, "the kernels' per-feature LDS arrays hold what the ABI admits");
#define VILF_LDS_CU_BYTES (160 * 1024)  // LDS of a CU (gfx950): a kernel declared __launch_bounds__(NT, k) for k workgroups per CU may take 1/k of it

// ---- workgroup sizes -------------------------------------------------------------------------------------------------
// VB_NT (vilf_batch.hpp): the window kernels, the marginalization kernels, k_prior_prep, k_reset
#define SNT 512             // k_solve
#define SBT 256             // k_solve_sb, k_sb_table (one table column per thread of k_solve_sb)
#define IMU_PREP_NT 64      // k_imu_prep: four factors of 16 lanes
#define WIN1_NT 64          // k_finalize (a lane per frame), k_time_limit (one lane)
#define QL_NT 64            // k_mf_ql: one wave, QL_LPW lanes of it at work
#define HOOK_NT 64          // the single-thread residual hooks
#define HOOK_PRIOR_NT 256   // k_hook_prior
#define PREINT_NT 64        // k_preintegrate: a lane per interval

// ---- k_linearize*: VB_LIN_LDS_BYTES (vilf_batch.hpp; sizeof(LinShared) is asserted beside the struct) -------------------------
static_assert(VB_LIN_LDS_DOUBLES >= 10 * 512, "the IMU staging area precedes the chunk loop in the same region");
static_assert(VB_LIN_LDS_BYTES <= VILF_LDS_CU_BYTES / 2, "k_linearize: two workgroups per CU");

// ---- k_solve (dense fallback; owns its CU) -------------------------------------------------------------------------------
#define SOLVE_OFF_T 0                                         // 66 lower tiles of 16 x 16
#define SOLVE_OFF_G (SOLVE_OFF_T + 66 * 256)                  // g~ (permuted, padded to VB_NPAD)
#define SOLVE_OFF_DIAG (SOLVE_OFF_G + VB_NPAD)
#define SOLVE_OFF_SCALE (SOLVE_OFF_DIAG + VB_NPAD)
#define SOLVE_OFF_Y (SOLVE_OFF_SCALE + VB_NPAD)               // rhs -> solution
#define SOLVE_OFF_INVD (SOLVE_OFF_Y + VB_NPAD)                // 1 / L_jj
#define SOLVE_OFF_V (SOLVE_OFF_INVD + VB_NPAD)                // v = g~ ./ diagonal_^2
#define SOLVE_OFF_RED (SOLVE_OFF_V + VB_NPAD)                 // block-sum scratch [SNT]; row 67 of schur_mfma's reduce between the sums
#define SOLVE_OFF_CF (SOLVE_OFF_RED + SNT)                    // per feature: s_f / sqrt(h~')
#define SOLVE_OFF_RNG (SOLVE_OFF_CF + VILF_MAX_FEATURES_DEV)  // per feature, int: 6*start | (6*(start+nobs)) << 16
#define SOLVE_LDS_BYTES (SOLVE_OFF_RNG * 8 + VILF_MAX_FEATURES_DEV * 4)
static_assert(SOLVE_LDS_BYTES <= VILF_LDS_CU_BYTES, "k_solve");

// ---- k_solve_sb: SB_OFF_* / SB_LDS_DOUBLES (vilf_batch.hpp) ----------------------------------------------------------------
#define SB_LDS_BYTES (SB_LDS_DOUBLES * 8)
#define SB_TAB_ROWS 23      // k_sb_table: int4 rows per thread of k_solve_sb
static_assert(SB_LDS_BYTES <= VILF_LDS_CU_BYTES / 2, "k_solve_sb: two workgroups per CU");

// ---- k_prior_prep: the n x n prior Jacobian, odd row stride (n <= MG_NK: 73.5 KB, two workgroups per CU) ------------------------------
#define PRIOR_PREP_LDS_BYTES ((MG_NK + 1) * (MG_NK + 1) * 8)
static_assert(MG_NK * (MG_NK | 1) * 8 <= PRIOR_PREP_LDS_BYTES && PRIOR_PREP_LDS_BYTES <= VILF_LDS_CU_BYTES / 2, "k_prior_prep");

// ---- k_marg_schur: the arrow fast path (exact == 0, three workgroups per CU) and the Jacobi path (exact == 1, a CU for itself) ---------------------
#define MGS_OFF_S 0                                           // [md][md]
#define MGS_OFF_Y (MGS_OFF_S + MG_MD * MG_MD)                 // [md][n + 1]
#define MGS_OFF_IH (MGS_OFF_Y + MG_MD * (MG_NK + 1))          // [mf] 1 / h_f
#define MGS_OFF_RED (MGS_OFF_IH + VILF_MAX_FEATURES_DEV)      // [VB_NT]
#define MGS_OFF_W (MGS_OFF_RED + VB_NT)                       // [MG_FCH][MG_RWP] staged arrow rows
#define MGS_FAST_LDS_BYTES ((MGS_OFF_W + MG_FCH * MG_RWP) * 8)
#define MGS_EXACT_LDS_DOUBLES (MG_MLDS * MG_MLDS)             // Amm while M <= MG_MLDS, then X while it fits
#define MGS_EXACT_LDS_BYTES (MGS_EXACT_LDS_DOUBLES * 8)
static_assert(MGS_FAST_LDS_BYTES <= VILF_LDS_CU_BYTES / 3, "k_marg_schur, fast path: three workgroups per CU");
static_assert(MGS_EXACT_LDS_BYTES <= VILF_LDS_CU_BYTES && MGS_FAST_LDS_BYTES <= MGS_EXACT_LDS_BYTES, "k_marg_schur, exact path (its total is the kernel's attribute)");

// ---- k_mf_chol_tiles (__launch_bounds__(VB_NT, 2); ~34 KB) -------------------------------------------------------------------------
#define MFT_ROWS 160                                          // 80 (A, b, padding) + 80 (identity rows, padding)
#define MFT_OFF_P 0                                           // packed lower rows 0..75
#define MFT_OFF_PAN (MFT_OFF_P + SB_NR * (SB_NR + 1) / 2)     // the panel's columns [row][4]
#define MFT_OFF_LP (MFT_OFF_PAN + 4 * MFT_ROWS)               // the panel's factor rows [row][4]
#define MFT_LDS_DOUBLES (MFT_OFF_LP + 4 * MFT_ROWS + 16)
#define MFT_LDS_BYTES (MFT_LDS_DOUBLES * 8)
static_assert(MFT_LDS_BYTES <= VILF_LDS_CU_BYTES / 2, "k_mf_chol_tiles");

// ---- k_mf_ql: d then e, element i of lane l at [QL_LPW * i + l] -----------------------------------------------------------------
#define QL_OFF_D 0
#define QL_OFF_E (QL_OFF_D + (MG_NK + 2) * QL_LPW)
#define QL_LDS_BYTES ((QL_OFF_E + (MG_NK + 2) * QL_LPW) * 8)
static_assert(QL_LPW <= QL_NT && QL_LDS_BYTES <= VILF_LDS_CU_BYTES, "k_mf_ql");

// ---- k_mf_chol, k_mf_tridiag, k_mf_apply, k_marg_finish: V = n rows of stride n | 1 at s_dyn, in two dimension classes -------------------------
// A large batch launches each kernel once per class (n_lo <= n < n_hi): the small class takes three workgroups per CU.
#define MGF_SMALL_N 78                                                  // the small class: n < MGF_SMALL_N
#define MGF_SMALL_LDS_BYTES ((MGF_SMALL_N - 1) * (MGF_SMALL_N - 1) * 8)
#define MGF_LDS_BYTES ((MG_NK + 2) * (MG_NK + 2) * 8)                   // every n <= MG_NK
#define MFA_CH 64                                                       // rotations per staged chunk of k_mf_apply
#define MFA_LDS_EXTRA_BYTES (4 * MFA_CH * 8 + QL_ICAP * 2)              // k_mf_apply behind V: two chunks of (c, s) pairs + the 16-bit QL iteration table
static_assert((MGF_SMALL_N - 1) * ((MGF_SMALL_N - 1) | 1) * 8 <= MGF_SMALL_LDS_BYTES && MG_NK * (MG_NK | 1) * 8 <= MGF_LDS_BYTES, "V fits its class");
static_assert(MGF_SMALL_LDS_BYTES + MFA_LDS_EXTRA_BYTES <= VILF_LDS_CU_BYTES / 3 && MGF_LDS_BYTES + MFA_LDS_EXTRA_BYTES <= VILF_LDS_CU_BYTES, "kept-block kernels");

// ---- declarations ----------------------------------------------------------------------------------------------------
extern "C" {
// vilf_kernels.hip
__global__ __launch_bounds__(IMU_PREP_NT) void k_imu_prep(int n, const double *cov, double *work, double *imu_rec);
__global__ __launch_bounds__(VB_NT) void k_prior_prep(VbBatch b, double *prior_H, double *prior_g, unsigned lds_bytes, const int *done4);
__global__ __launch_bounds__(VB_NT) void k_linearize(VbBatch b, int iteration_zero);
__global__ __launch_bounds__(VB_NT) void k_linearize_last(VbBatch b);
__global__ __launch_bounds__(VB_NT) void k_linearize_split(VbBatch b, int iteration_zero);
__global__ __launch_bounds__(SNT) void k_solve(VbBatch b);
__global__ __launch_bounds__(SBT) void k_sb_table(int *tab);
__global__ __launch_bounds__(SBT, 2) void k_solve_sb(VbBatch b);
__global__ void k_finalize(VbBatch b);
__global__ void k_time_limit(VbBatch b, const int *mflag, int only_margin_old);
__global__ void k_reset(VbBatch b, int rewind_state);
__global__ void k_hook_projection(const double *p0, const double *p1, const double *p2, double lam, const double *pi, const double *pj, double sqrt_info, double *out);
__global__ void k_hook_projection_td(const double *in, double *out);
__global__ void k_hook_imu(const double *p0, const double *p1, const double *p2, const double *p3, const double *rec, const double *G, double *out, double *scratch);
__global__ void k_hook_lidar(const double *p0, const double *p1, const double *qil, const double *til, const double *lc, double *out);
__global__ void k_hook_prior(const int *hdr, const double *x0, const double *x, const double *J0, const double *r0, double *out);
__global__ void k_hook_edge(const double *pose, const double *cp, const double *pa, const double *pb, double *out);
__global__ void k_hook_surf(const double *pose, const double *cp, const double *n, double d, double *out);
__global__ void k_hook_plus(const double *x, const double *d, int kind, double *out);
// vilf_marg.hip
__global__ __launch_bounds__(VB_NT, 2) void k_marg_prepare(VbBatch b, VbMarg g);
__global__ __launch_bounds__(VB_NT) void k_marg_prepare_td(VbBatch b, VbMarg g);
__global__ __launch_bounds__(VB_NT, 3) void k_marg_schur(VbBatch b, VbMarg g, int exact);
__global__ __launch_bounds__(VB_NT) void k_mf_chol(VbBatch b, VbMarg g, int n_lo, int n_hi, int disable);
__global__ __launch_bounds__(VB_NT, 2) void k_mf_chol_tiles(VbBatch b, VbMarg g, int disable);
__global__ __launch_bounds__(VB_NT) void k_mf_tridiag(VbBatch b, VbMarg g, int n_lo, int n_hi);
__global__ __launch_bounds__(QL_NT) void k_mf_ql(VbBatch b, VbMarg g, int force_overflow);
__global__ __launch_bounds__(VB_NT) void k_mf_apply(VbBatch b, VbMarg g, int n_lo, int n_hi);
__global__ __launch_bounds__(VB_NT) void k_marg_finish(VbBatch b, VbMarg g, int n_lo, int n_hi, int only_flagged);
__global__ __launch_bounds__(VB_NT) void k_prior_keep(VbBatch b, VbMarg g);
}
// vilf_host.hip
__global__ void k_preintegrate(int n, vilf_imu_noise nz, const double *acc0, const double *gyr0, const double *ba, const double *bg, const int *n_samples, int max_samples,
                               const double *dt, const double *acc, const double *gyr, vilf_imu_preint *out);
