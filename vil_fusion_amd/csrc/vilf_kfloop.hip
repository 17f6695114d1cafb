// vilf_kfloop.hip — the second stage of the visual loop closure on the device (≙ KeyFrame::PnPRANSAC and the end of KeyFrame::findConnection,
//   pose_graph/keyframe.cpp:200-256, 401-520). The arithmetic is stated once, in include/vilfusion.h ("Visual loop closure, second stage"); the Levenberg-Marquardt
//   is the start-up's (vilf_pnp.hpp), the sampler the tracker's (vilf_fmat.hpp), the match the first stage's (vilf_kf.hpp). One call = one chain on the handle's stream:
//   kf_match            the first stage's launch; its results stay on the device
//   kf_loop_gather      a workgroup per candidate: the status-1 window points compacted in window order by ballot rank and a running offset (no atomics), and the
//                       guess (R0, t0) of cur by thread 0
//   kf_loop_hypotheses  grid (ceil(K / 64), candidates), a lane per hypothesis: the sample, then the 5-point LM entirely in the lane's registers
//   kf_loop_score       grid (ceil(K / 64), candidates), a lane per hypothesis with its pose in registers: the members pass through LDS in chunks and every lane reads
//                       the same member (a broadcast); the score is a register count, so no lane ever meets another and the schedule cannot show
//   kf_loop_refine      a workgroup of 256 per candidate: the winner by (max score, min k), its mask, the inliers compacted into LDS, sf_pnp, the pose out, the row
// Candidates that fail the gate leave every kernel at once; kf_loop_refine writes their row.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include "vilf_internal.hpp"
#include "vilf_device.hpp"
#include "vilf_fmat.hpp"
#include "vilf_pnp.hpp"
#include "vilf_kf.hpp"

#define KFL_SLOTS 5                     // members of a sample
#define KFL_CHUNK 256                   // kf_loop_score: members per pass through LDS (20 bytes each)
static_assert(KF_NT == SF_NT, "kf_loop_refine runs sf_pnp");

// one call's device arrays, indexed by candidate; n = the window points of cur, K = the hypotheses
struct KflDev {
    const unsigned char *status; const float2 *ptn;      // kf_match's, [cand][n]
    const float *geo_X; const double *geo_pose;          // of cur: [n][3], [12]
    const int *old;                                      // [cand] key-frame indices
    float *X; float2 *u; int *widx; int *m;              // gather: [cand][n][3], [cand][n], [cand][n], [cand]
    double *guess;                                       // [cand][12]
    double *pose; int *score;                            // [cand][K][12], [cand][K]
    vilf_kf_loop_result *rows; unsigned char *mask;      // [cand], [cand][n]
};
struct KflPar { int K, hyp_iters, refine_iters, min_loop_num; unsigned seed; double lambda0, thr2, qic[9], tic[3]; };

// ---- launch contract -----------------------------------------------------------------------------------------------------
__global__ void kf_loop_gather(KflDev d, KflPar p, int n);             // grid = candidates, block KF_NT
__global__ void kf_loop_hypotheses(KflDev d, KflPar p, int n);         // grid (ceil(K / 64), candidates), block 64
__global__ void kf_loop_score(KflDev d, KflPar p, int n);              // grid (ceil(K / 64), candidates), block 64
__global__ void kf_loop_refine(KflDev d, KflPar p, int n);             // grid = candidates, block KF_NT

namespace {
// the rank of every flagged thread of the workgroup among the flagged ones, in thread order, and their number; wc [KF_WAVES] is LDS. Two barriers.
VD int kfl_rank(bool flag, int tid, int *wc, int &count) {
    const int wave = tid >> 6, lane = tid & 63;
    const unsigned long long b = __ballot(flag);
    if (lane == 0) wc[wave] = __popcll(b);
    __syncthreads();
    int off = 0, all = 0;
#pragma unroll
    for (int w = 0; w < KF_WAVES; w++) { const int c = wc[w]; off += w < wave ? c : 0; all += c; }
    __syncthreads();
    count = all;
    return off + __popcll(b & ((1ull << lane) - 1ull));
}
// the score's rule for one member
VD bool kfl_inlier(const double *R, const double *t, const float *X, float2 u, double thr2) {
    double q[3], iz, xn, yn, e0, e1;
    sf_residual(R, t, X, u, q, iz, xn, yn, e0, e1);
    const double p2 = __dadd_rn(q[2], t[2]);
    return p2 > 0.0 && __dadd_rn(__dmul_rn(e0, e0), __dmul_rn(e1, e1)) <= thr2;
}
VD bool kfl_finite(const double *R, const double *t) {
    bool fin = true;
#pragma unroll
    for (int e = 0; e < 9; e++) fin = fin && isfinite(R[e]);
#pragma unroll
    for (int r = 0; r < 3; r++) fin = fin && isfinite(t[r]);
    return fin;
}
}  // namespace

// ---- kf_loop_gather ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KF_NT) void kf_loop_gather(KflDev d, KflPar p, int n) {
    __shared__ int wc[KF_WAVES];
    const int tid = threadIdx.x, cand = blockIdx.x;
    const size_t row = (size_t)cand * n;
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += KF_NT) {                  // the trip count is the workgroup's
        const int i = c0 + tid;
        const bool st = i < n && d.status[row + i] != 0;
        int cnt;
        const int r = base + kfl_rank(st, tid, wc, cnt);
        if (st) {                                            // r < the number of status-1 points <= n: inside the candidate's rows
            const float2 un = d.ptn[row + i];
            d.X[3 * (row + r)] = d.geo_X[3 * i]; d.X[3 * (row + r) + 1] = d.geo_X[3 * i + 1]; d.X[3 * (row + r) + 2] = d.geo_X[3 * i + 2];
            d.u[row + r] = un;
            d.widx[row + r] = i;
        }
        base += cnt;
    }
    if (tid != 0) return;
    d.m[cand] = base;
    // the guess, of cur
    const double *Rv = d.geo_pose, *Tv = d.geo_pose + 9;
    double Rwc[9], Twc[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) Rwc[r * 3 + c] = vilf_dot3(Rv[r * 3], p.qic[c], Rv[r * 3 + 1], p.qic[3 + c], Rv[r * 3 + 2], p.qic[6 + c]);
        Twc[r] = __dadd_rn(Tv[r], vilf_dot3(Rv[r * 3], p.tic[0], Rv[r * 3 + 1], p.tic[1], Rv[r * 3 + 2], p.tic[2]));
    }
    double *g = d.guess + (size_t)cand * 12;
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) g[r * 3 + c] = Rwc[c * 3 + r];
        g[9 + r] = -vilf_dot3(Rwc[r], Twc[0], Rwc[3 + r], Twc[1], Rwc[6 + r], Twc[2]);
    }
}

// ---- kf_loop_hypotheses: a lane per hypothesis --------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void kf_loop_hypotheses(KflDev d, KflPar p, int n) {
    const int cand = blockIdx.y, k = blockIdx.x * 64 + threadIdx.x;
    const int m = d.m[cand];
    if (m <= p.min_loop_num || k >= p.K) return;             // m > min_loop_num >= 5: the sample has its five distinct members
    const size_t row = (size_t)cand * n;
    // sample: slot j in registers (every loop over the slots is unrolled)
    int S[KFL_SLOTS];
    const unsigned base = tk_mix(tk_mix(p.seed + (unsigned)d.old[cand] + 0x9e3779b9u) + (unsigned)k);
#pragma unroll
    for (int j = 0; j < KFL_SLOTS; j++) {
        int i = (int)(((unsigned long long)tk_mix(base + (unsigned)j) * (unsigned long long)m) >> 32);
#pragma unroll
        for (int step = 0; step < j; step++) {
            bool dup = false;
#pragma unroll
            for (int e = 0; e < j; e++) dup |= S[e] == i;
            i = dup ? (i + 1 == m ? 0 : i + 1) : i;
        }
        S[j] = i;
    }
    float X[KFL_SLOTS][3];
    float2 u[KFL_SLOTS];
#pragma unroll
    for (int j = 0; j < KFL_SLOTS; j++) {                    // S[j] < m <= n
        const float *x = d.X + 3 * (row + S[j]);
        X[j][0] = x[0]; X[j][1] = x[1]; X[j][2] = x[2];
        u[j] = d.u[row + S[j]];
    }
    double R[9], t[3];
    const double *g = d.guess + (size_t)cand * 12;
#pragma unroll
    for (int e = 0; e < 9; e++) R[e] = g[e];
#pragma unroll
    for (int r = 0; r < 3; r++) t[r] = g[9 + r];
    double lam = p.lambda0;
    for (int it = 0; it < p.hyp_iters; it++) {
        double s[SF_TERMS];
#pragma unroll
        for (int e = 0; e < SF_TERMS; e++) s[e] = 0.0;
#pragma unroll
        for (int j = 0; j < KFL_SLOTS; j++) sf_add_terms(R, t, X[j], u[j], s);
        double x[6], Rn[9], tn[3];
        const bool pos = sf_solve(s, lam, x);
        sf_candidate(R, t, x, Rn, tn);
        double cn = 0.0;
#pragma unroll
        for (int j = 0; j < KFL_SLOTS; j++) {
            double q[3], iz, xn, yn, e0, e1;
            sf_residual(Rn, tn, X[j], u[j], q, iz, xn, yn, e0, e1);
            cn = __dadd_rn(cn, __dadd_rn(__dmul_rn(e0, e0), __dmul_rn(e1, e1)));
        }
        if (pos && cn < s[27]) {
#pragma unroll
            for (int e = 0; e < 9; e++) R[e] = Rn[e];
#pragma unroll
            for (int r = 0; r < 3; r++) t[r] = tn[r];
            lam = __ddiv_rn(lam, 10.0);
        } else {
            lam = __dmul_rn(lam, 10.0);
        }
    }
    double *o = d.pose + ((size_t)cand * p.K + k) * 12;
#pragma unroll
    for (int e = 0; e < 9; e++) o[e] = R[e];
#pragma unroll
    for (int r = 0; r < 3; r++) o[9 + r] = t[r];
}

// ---- kf_loop_score: a lane per hypothesis, the members broadcast from LDS ----------------------------------------------------------
__global__ __launch_bounds__(64) void kf_loop_score(KflDev d, KflPar p, int n) {
    __shared__ float sX[3 * KFL_CHUNK];
    __shared__ float2 su[KFL_CHUNK];
    const int cand = blockIdx.y, lane = threadIdx.x, k = blockIdx.x * 64 + lane;
    const int m = d.m[cand];
    if (m <= p.min_loop_num) return;                         // the whole workgroup
    const size_t row = (size_t)cand * n;
    const bool live = k < p.K;
    double R[9], t[3];
    const double *g = d.pose + ((size_t)cand * p.K + (live ? k : 0)) * 12;
#pragma unroll
    for (int e = 0; e < 9; e++) R[e] = g[e];
#pragma unroll
    for (int r = 0; r < 3; r++) t[r] = g[9 + r];
    const bool valid = kfl_finite(R, t);
    int cnt = 0;
    for (int c0 = 0; c0 < m; c0 += KFL_CHUNK) {              // the trip count is the workgroup's
        const int cn = min(KFL_CHUNK, m - c0);
        for (int i = lane; i < 3 * cn; i += 64) sX[i] = d.X[3 * (row + c0) + i];
        for (int i = lane; i < cn; i += 64) su[i] = d.u[row + c0 + i];
        __syncthreads();
        for (int j = 0; j < cn; j++) cnt += kfl_inlier(R, t, sX + 3 * j, su[j], p.thr2) ? 1 : 0;
        __syncthreads();
    }
    if (live) d.score[(size_t)cand * p.K + k] = valid ? cnt : -1;
}

// ---- kf_loop_refine: a workgroup per candidate -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(KF_NT) void kf_loop_refine(KflDev d, KflPar p, int n) {
    __shared__ float sX[3 * KF_WIN_CAP];
    __shared__ float2 su[KF_WIN_CAP];
    __shared__ unsigned char smask[KF_WIN_CAP];
    __shared__ double s_red[4 * SF_TERMS], s_red2[4];
    __shared__ int s_bs[KF_NT], s_bk[KF_NT], wc[KF_WAVES];
    const int tid = threadIdx.x, cand = blockIdx.x;
    const size_t row = (size_t)cand * n;
    const int m = d.m[cand];
    vilf_kf_loop_result *out = d.rows + cand;
    // the row starts at 0 (as doubles: 8-byte rows of a hipMalloc'ed array), the mask too
    static_assert(sizeof(vilf_kf_loop_result) % 8 == 0, "the row is cleared as doubles");
    for (int e = tid; e < (int)(sizeof(vilf_kf_loop_result) / 8); e += KF_NT) ((double *)out)[e] = 0.0;
    for (int i = tid; i < n; i += KF_NT) smask[i] = 0;       // n <= KF_WIN_CAP
    __syncthreads();
    int flags = 0, best_k = 0, ninl = 0, accepted = 0;
    double R[9], t[3], cost0 = 0.0, cost1 = 0.0;
    bool pose = false;
    if (m <= p.min_loop_num) {
        flags = VILF_KFL_GATE;
    } else {
        // the winner: (max score, min k) of every thread's hypotheses, then of the 256 threads, read by all
        int bs = -1, bk = -1;
        for (int k = tid; k < p.K; k += KF_NT) { const int s = d.score[(size_t)cand * p.K + k]; if (s > bs) { bs = s; bk = k; } }      // k ascends: the first of equal scores stays
        s_bs[tid] = bs; s_bk[tid] = bk;
        __syncthreads();
        bs = -1; bk = -1;
        for (int i = 0; i < KF_NT; i++) { const int s = s_bs[i], k = s_bk[i]; if (s > bs || (s == bs && s >= 0 && k < bk)) { bs = s; bk = k; } }
        if (bs < 0) {
            flags = VILF_KFL_NO_HYPOTHESIS; best_k = -1;
        } else {
            best_k = bk;
            const double *g = d.pose + ((size_t)cand * p.K + bk) * 12;
            double Rw[9], tw[3];
#pragma unroll
            for (int e = 0; e < 9; e++) { Rw[e] = g[e]; R[e] = Rw[e]; }
#pragma unroll
            for (int r = 0; r < 3; r++) { tw[r] = g[9 + r]; t[r] = tw[r]; }
            // the winner's mask; its inliers into LDS in S order
            for (int c0 = 0; c0 < m; c0 += KF_NT) {          // the trip count is the workgroup's
                const int j = c0 + tid;
                bool in = false;
                float x[3] = {0.f, 0.f, 0.f};
                float2 un = make_float2(0.f, 0.f);
                if (j < m) {
                    x[0] = d.X[3 * (row + j)]; x[1] = d.X[3 * (row + j) + 1]; x[2] = d.X[3 * (row + j) + 2];
                    un = d.u[row + j];
                    in = kfl_inlier(Rw, tw, x, un, p.thr2);
                }
                int cnt;
                const int r = ninl + kfl_rank(in, tid, wc, cnt);
                if (in) {                                    // r < m <= n <= KF_WIN_CAP; widx < n
                    sX[3 * r] = x[0]; sX[3 * r + 1] = x[1]; sX[3 * r + 2] = x[2];
                    su[r] = un;
                    smask[d.widx[row + j]] = 1;
                }
                ninl += cnt;
            }
            __syncthreads();
            SfPar sp;
            sp.min_count = 0; sp.warn_count = 0; sp.iters = p.refine_iters; sp.lambda0 = p.lambda0;
            SfRow sr;
            const bool ok = sf_pnp(sX, su, ninl, 0, sp, R, t, s_red, s_red2, tid, sr);
            cost0 = sr.cost0; cost1 = sr.cost1; accepted = sr.accepted;
            if (ok) {
                flags = VILF_KFL_REFIT;
            } else {
                flags = VILF_KFL_REFIT_DROPPED;
#pragma unroll
                for (int e = 0; e < 9; e++) R[e] = Rw[e];
#pragma unroll
                for (int r = 0; r < 3; r++) t[r] = tw[r];
            }
            pose = true;
        }
    }
    __syncthreads();
    for (int i = tid; i < n; i += KF_NT) d.mask[row + i] = smask[i];
    if (tid != 0) return;
    out->n_matched = m; out->n_inliers = ninl; out->best_k = best_k; out->flags = flags; out->accepted = accepted;
    if (!pose) return;
    out->cost0 = cost0; out->cost1 = cost1;
    double W[9], Tw[3], P[9];
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) W[r * 3 + c] = R[c * 3 + r];
        Tw[r] = -vilf_dot3(R[r], t[0], R[3 + r], t[1], R[6 + r], t[2]);
    }
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) P[r * 3 + c] = vilf_dot3(W[r * 3], p.qic[c * 3], W[r * 3 + 1], p.qic[c * 3 + 1], W[r * 3 + 2], p.qic[c * 3 + 2]);
#pragma unroll
    for (int e = 0; e < 9; e++) { out->R[e] = R[e]; out->PnP_R_old[e] = P[e]; }
#pragma unroll
    for (int r = 0; r < 3; r++) {
        out->t[r] = t[r];
        out->PnP_T_old[r] = __dsub_rn(Tw[r], vilf_dot3(P[r * 3], p.tic[0], P[r * 3 + 1], p.tic[1], P[r * 3 + 2], p.tic[2]));
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
namespace {
bool kfl_all_finite(const double *v, int n) {
    for (int i = 0; i < n; i++) if (!std::isfinite(v[i])) return false;
    return true;
}
bool kfl_params_ok(const vilf_kf_loop_params *p) {
    return p->n_hypotheses >= 1 && p->n_hypotheses <= VILF_TRACK_MAX_HYPOTHESES && p->hyp_iterations >= 1 && p->hyp_iterations <= 64 && p->refine_iterations >= 1 &&
           p->refine_iterations <= 64 && p->min_loop_num >= KFL_SLOTS && std::isfinite(p->lambda0) && p->lambda0 > 0 &&
           std::isfinite(p->reproj_threshold) && p->reproj_threshold > 0 && std::isfinite(p->max_yaw) && p->max_yaw > 0 && std::isfinite(p->max_dist) && p->max_dist > 0 &&
           kfl_all_finite(p->qic, 9) && kfl_all_finite(p->tic, 3);
}
double kfl_yaw_deg(const double *R) { return std::atan2(R[3], R[0]) / M_PI * 180.0; }
double kfl_normalize_angle(double a) {
    return a > 0 ? a - 360.0 * std::floor((a + 180.0) / 360.0) : a + 360.0 * std::floor((-a + 180.0) / 360.0);
}
// Eigen's matrix-to-quaternion rule -> (w, x, y, z)
void kfl_quaternion(const double *M, double *q) {
    const double tr = M[0] + M[4] + M[8];
    if (tr > 0.0) {
        double s = std::sqrt(tr + 1.0);
        q[0] = 0.5 * s;
        s = 0.5 / s;
        q[1] = (M[7] - M[5]) * s; q[2] = (M[2] - M[6]) * s; q[3] = (M[3] - M[1]) * s;
    } else {
        int i = 0;
        if (M[4] > M[0]) i = 1;
        if (M[8] > M[i * 4]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        double s = std::sqrt(M[i * 4] - M[j * 4] - M[k * 4] + 1.0);
        q[1 + i] = 0.5 * s;
        s = 0.5 / s;
        q[0] = (M[k * 3 + j] - M[j * 3 + k]) * s;
        q[1 + j] = (M[j * 3 + i] + M[i * 3 + j]) * s;
        q[1 + k] = (M[k * 3 + i] + M[i * 3 + k]) * s;
    }
}
// the paragraph "decision" for one row with more than min_loop_num inliers
void kfl_decide(const vilf_kf_loop_params *p, const double *vio, vilf_kf_loop_result *r) {
    const double *P = r->PnP_R_old, *Rv = vio, *Tv = vio + 9;
    double dT[3], M[9];
    for (int e = 0; e < 3; e++) dT[e] = Tv[e] - r->PnP_T_old[e];
    for (int a = 0; a < 3; a++) {
        r->relative_t[a] = P[a] * dT[0] + P[3 + a] * dT[1] + P[6 + a] * dT[2];
        for (int b = 0; b < 3; b++) M[a * 3 + b] = P[a] * Rv[b] + P[3 + a] * Rv[3 + b] + P[6 + a] * Rv[6 + b];
    }
    kfl_quaternion(M, r->relative_q);
    r->relative_yaw = kfl_normalize_angle(kfl_yaw_deg(Rv) - kfl_yaw_deg(P));
    const double dist = std::sqrt(r->relative_t[0] * r->relative_t[0] + r->relative_t[1] * r->relative_t[1] + r->relative_t[2] * r->relative_t[2]);
    if (std::fabs(r->relative_yaw) < p->max_yaw && dist < p->max_dist) { r->has_loop = 1; r->flags |= VILF_KFL_LOOP; }
}
}  // namespace

extern "C" void vilf_kf_default_loop_params(vilf_kf_loop_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->n_hypotheses = 256; p->hyp_iterations = 5; p->refine_iterations = 10; p->min_loop_num = 25; p->lambda0 = 1e-3; p->reproj_threshold = 10.0 / 460.0;
    p->max_yaw = 30.0; p->max_dist = 20.0;
    p->qic[0] = p->qic[4] = p->qic[8] = 1.0;
}

extern "C" int vilf_kf_set_geometry(vilf_handle *h, int index, const float *point_3d, const double vio_R[9], const double vio_T[3]) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    KfCtx *c = vilf_kf_ctx(h, "vilf_kf_set_geometry");
    if (!c) return VILF_ERR_INVALID_ARGUMENT;
    if (index < 0 || index >= c->size) { h->err = "vilf_kf_set_geometry: index out of range"; return VILF_ERR_INVALID_ARGUMENT; }
    const int nw = c->meta[index].n_win;
    if ((nw > 0 && !point_3d) || !vio_R || !vio_T) { h->err = "vilf_kf_set_geometry: null pointer"; return VILF_ERR_INVALID_ARGUMENT; }
    bool fin = kfl_all_finite(vio_R, 9) && kfl_all_finite(vio_T, 3);
    for (int i = 0; i < 3 * nw; i++) fin = fin && std::isfinite(point_3d[i]);
    if (!fin) { h->err = "vilf_kf_set_geometry: a value that is not finite"; return VILF_ERR_INVALID_ARGUMENT; }
    HIPCHECK(h, hipSetDevice(h->device));
    const size_t K = (size_t)c->capK, k = (size_t)index;
    if (c->has_geo.empty()) {
        if (!c->geo_X.ensure(K * KF_WIN_CAP * 12) || !c->geo_pose.ensure(K * 96)) { h->err = "hipMalloc failed (key-frame geometry)"; return VILF_ERR_DEVICE; }
        c->has_geo.assign(K, 0);
        c->geo_pose_h.assign(K * 12, 0.0);
    }
    double pose[12];
    std::memcpy(pose, vio_R, 72); std::memcpy(pose + 9, vio_T, 24);
    if (nw > 0) HIPCHECK(h, hipMemcpyAsync(c->geo_X.as<float>() + k * KF_WIN_CAP * 3, point_3d, (size_t)nw * 12, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(h, hipMemcpyAsync(c->geo_pose.as<double>() + k * 12, pose, 96, hipMemcpyHostToDevice, h->stream));
    { const int rc = vilf_kf_finish(h); if (rc != VILF_OK) return rc; }      // the caller's arrays are free again
    std::memcpy(c->geo_pose_h.data() + k * 12, pose, 96);
    c->has_geo[k] = 1;
    return VILF_OK;
}

extern "C" int vilf_kf_find_connection(vilf_handle *h, const vilf_kf_loop_params *p, int cur, int n_old, const int *old_index, vilf_kf_loop_result *out,
                                       unsigned char *status_out, float *pt_old_norm_out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    KfCtx *c = vilf_kf_ctx(h, "vilf_kf_find_connection");
    if (!c) return VILF_ERR_INVALID_ARGUMENT;
    if (!p || !out) { h->err = "vilf_kf_find_connection: null pointer"; return VILF_ERR_INVALID_ARGUMENT; }
    { const int rc = vilf_kf_match_check(h, c, "vilf_kf_find_connection", cur, n_old, old_index); if (rc != VILF_OK) return rc; }
    if (c->has_geo.empty() || !c->has_geo[cur]) { h->err = "vilf_kf_find_connection: the current key frame has no geometry (vilf_kf_set_geometry)"; return VILF_ERR_INVALID_ARGUMENT; }
    if (!kfl_params_ok(p)) {
        h->err = "vilf_kf_find_connection: 1 <= n_hypotheses <= VILF_TRACK_MAX_HYPOTHESES, 1 <= iterations <= 64, min_loop_num >= 5, positive finite lambda0, "
                 "reproj_threshold, max_yaw and max_dist, a finite extrinsic";
        return VILF_ERR_INVALID_ARGUMENT;
    }
    HIPCHECK(h, hipSetDevice(h->device));
    const int n = c->meta[cur].n_win, K = p->n_hypotheses;
    const size_t C = (size_t)n_old, rows = C * n;
    // one block: what comes back first (the rows, the lifted points, the masks), then what stays on the device
    Layout l;
    const size_t o_rows = l.take(C * sizeof(vilf_kf_loop_result), 8), o_ptn = l.take(rows * 8, 8), o_mask = l.take(rows, 1), down_bytes = l.at;
    const size_t o_pt = l.take(rows * 8, 8), o_idx = l.take(rows * 4, 4), o_dist = l.take(rows * 4, 4), o_cnt = l.take(C * 4, 4), o_st = l.take(rows, 1);
    const size_t o_X = l.take(rows * 12, 8), o_u = l.take(rows * 8, 8), o_widx = l.take(rows * 4, 4), o_m = l.take(C * 4, 4), o_guess = l.take(C * 96, 8);
    const size_t o_pose = l.take(C * K * 96, 8), o_score = l.take(C * K * 4, 4), bytes = l.at;
    if (!c->loop_d.ensure(bytes) || !c->loop_down.ensure(down_bytes)) { h->err = "allocation failed (vilf_kf_find_connection)"; return VILF_ERR_DEVICE; }
    char *b = c->loop_d.as<char>();
    const KfMatchOut mo{(unsigned char *)(b + o_st), (float2 *)(b + o_pt), (float2 *)(b + o_ptn), (int *)(b + o_idx), (int *)(b + o_dist), (int *)(b + o_cnt)};
    KflDev d;
    d.status = mo.status; d.ptn = mo.ptn; d.geo_X = c->geo_X.as<float>() + (size_t)cur * KF_WIN_CAP * 3; d.geo_pose = c->geo_pose.as<double>() + (size_t)cur * 12;
    d.old = c->old_d.as<int>();
    d.X = (float *)(b + o_X); d.u = (float2 *)(b + o_u); d.widx = (int *)(b + o_widx); d.m = (int *)(b + o_m); d.guess = (double *)(b + o_guess);
    d.pose = (double *)(b + o_pose); d.score = (int *)(b + o_score); d.rows = (vilf_kf_loop_result *)(b + o_rows); d.mask = (unsigned char *)(b + o_mask);
    KflPar kp;
    kp.K = K; kp.hyp_iters = p->hyp_iterations; kp.refine_iters = p->refine_iterations; kp.min_loop_num = p->min_loop_num; kp.seed = p->seed; kp.lambda0 = p->lambda0;
    kp.thr2 = p->reproj_threshold * p->reproj_threshold;
    std::memcpy(kp.qic, p->qic, 72); std::memcpy(kp.tic, p->tic, 24);
    const dim3 gk((K + 63) / 64, n_old);
    ProfMarks first(h, c->prof);
    { const int rc = vilf_kf_match_enqueue(h, c, cur, n_old, old_index, mo); if (rc != VILF_OK) return rc; }
    first.mark(3);
    ProfMarks prof(h, c->loop_prof);
    hipLaunchKernelGGL(kf_loop_gather, dim3(n_old), dim3(KF_NT), 0, h->stream, d, kp, n);
    prof.mark(0);
    hipLaunchKernelGGL(kf_loop_hypotheses, gk, dim3(64), 0, h->stream, d, kp, n);
    prof.mark(1);
    hipLaunchKernelGGL(kf_loop_score, gk, dim3(64), 0, h->stream, d, kp, n);
    prof.mark(2);
    hipLaunchKernelGGL(kf_loop_refine, dim3(n_old), dim3(KF_NT), 0, h->stream, d, kp, n);
    prof.mark(3);
    HIPCHECK(h, hipGetLastError());
    HIPCHECK(h, hipMemcpyAsync(c->loop_down.p, b, down_bytes, hipMemcpyDeviceToHost, h->stream));
    prof.mark(4);
    { const int rc = vilf_kf_finish(h); if (rc != VILF_OK) return rc; }
    const char *hb = (const char *)c->loop_down.p;
    std::memcpy(out, hb + o_rows, C * sizeof(vilf_kf_loop_result));
    if (rows && status_out) std::memcpy(status_out, hb + o_mask, rows);
    if (rows && pt_old_norm_out) std::memcpy(pt_old_norm_out, hb + o_ptn, rows * 8);
    for (int i = 0; i < n_old; i++)
        if (out[i].n_inliers > p->min_loop_num) kfl_decide(p, c->geo_pose_h.data() + (size_t)cur * 12, &out[i]);
    return VILF_OK;
}

extern "C" int vilf_kf_loop_profile(vilf_handle *h, double ms_out[5], long launches_out[5]) { return vilf_stage_profile(h, ST_KF, &KfCtx::loop_prof, ms_out, launches_out); }
