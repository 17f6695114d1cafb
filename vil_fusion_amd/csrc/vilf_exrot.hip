// vilf_exrot.hip — the on-line camera-IMU rotation calibration on the device (≙ InitialEXRotation::CalibrationExRotation, initial/initial_ex_rotation.cpp:11-67, with
//   solveRelativeR, testTriangulation and decomposeE). The arithmetic is stated once, in include/vilfusion.h ("Camera-IMU rotation calibration"); the search is the
//   tracker's (vilf_fmat.hpp), the decomposition and the depths are the start-up's (vilf_pose.hpp).
// The state lives on the device, in the handle: per slot frame_count, ric and the three histories, plus the angles and weights of the slot's last push. One push of
// all slots = one upload, one chain of three launches on the handle's stream; the host waits once, at the one download:
//   ex_hypotheses  grid (ceil(K / 64), slots), a lane per hypothesis: tk_f_hypothesis on the slot's points; a slot that is skipped or has too few points leaves at once
//   ex_score       grid (ceil(K / 4), slots), a wave per hypothesis: ballot + popcount, one packed 64-bit atomicMax per hypothesis
//   ex_solve       a workgroup per slot: wave 0 decomposes the winner (every lane the same numbers in its own LDS column), counts the four fronts by ballot and
//                  chooses; thread 0 appends (Rc, Rimu, Rc_g); a thread per history entry computes its weight and its block B into LDS; ten threads sum G in the
//                  text's order; thread 0 runs the Jacobi and writes the result row, the new ric and frame_count
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "vilf_internal.hpp"
#include "vilf_device.hpp"
#include "vilf_fmat.hpp"
#include "vilf_pose.hpp"

#define EX_MAXN VILF_MAX_FEATURES            // correspondences of a push
#define EX_MAXK VILF_TRACK_MAX_HYPOTHESES
#define EX_H VILF_EXROT_MAX_HISTORY
#define EX_STAGES 3
enum { EH_N = 0, EH_FIRST = 1, EH_INTS = 2 };      // a slot's integers in the upload: n (-1: skipped), the first row of its points

// the device arrays of one call, indexed by slot
struct ExDev {
    const int *hdr; const double *dq; const float2 *ua, *ub;                 // the upload: [slot][EH_INTS], [slot][4], the points of all slots
    int *fc; double *ric, *hist, *ang, *wgt;                                 // the state: [slot], [slot][9], [slot][3][EX_H][9] (Rc, Rimu, Rc_g), [slot][EX_H] twice
    double *F; int *valid; unsigned long long *best;                         // [slot][K][9], [slot][K], [slot]: (score + 1) << 32 | (K - 1 - k); 0 = no valid hypothesis
    vilf_exrot_result *rows;                                                 // the download
};
struct ExPar { int K; unsigned seed; int min_corres, min_frames; double thr2, huber, min_sigma; };

// ---- launch contract -----------------------------------------------------------------------------------------------------
#define EX_NT 256                           // ex_solve: grid (slots), one workgroup per slot, a thread per history entry: EX_H <= EX_NT
#define EX_SCORE_WAVES 4                    // ex_score: block 256, grid (ceil(K / 4), slots), a wave per hypothesis; no workgroup barrier
                                            // ex_hypotheses: block TK_F_LANES (one wave), grid (ceil(K / 64), slots)
static_assert(EX_H <= EX_NT, "ex_solve gives every history entry a thread of its own");
__global__ void ex_hypotheses(ExDev d, ExPar p);
__global__ void ex_score(ExDev d, ExPar p);
__global__ void ex_solve(ExDev d, ExPar p);

struct ExrotCtx : VilfStage {
    StageIO io;
    DBuf state, work;
    int n_slots = 0;
    std::vector<int> fc;                     // host mirror of the slots' frame_count (the full-slot check needs no download)
    StageProf<EX_STAGES> prof;
    void profile_reset() override { prof.reset(); }
};

namespace {
VD bool ex_searched(int n, int min_corres) { return n >= min_corres && n >= 8; }
// Q = R(q) of the PnP's paragraph "candidate", (x, y, z, s) = q
VD void ex_q_to_R(const double *q, double *Q) {
    const double x = q[0], y = q[1], z = q[2], s = q[3];
    const double xx = __dmul_rn(x, x), yy = __dmul_rn(y, y), zz = __dmul_rn(z, z), xy = __dmul_rn(x, y), xz = __dmul_rn(x, z), yz = __dmul_rn(y, z);
    const double sx = __dmul_rn(s, x), sy = __dmul_rn(s, y), sz = __dmul_rn(s, z);
    Q[0] = __dsub_rn(1.0, __dmul_rn(2.0, __dadd_rn(yy, zz))); Q[1] = __dmul_rn(2.0, __dsub_rn(xy, sz)); Q[2] = __dmul_rn(2.0, __dadd_rn(xz, sy));
    Q[3] = __dmul_rn(2.0, __dadd_rn(xy, sz)); Q[4] = __dsub_rn(1.0, __dmul_rn(2.0, __dadd_rn(xx, zz))); Q[5] = __dmul_rn(2.0, __dsub_rn(yz, sx));
    Q[6] = __dmul_rn(2.0, __dsub_rn(xz, sy)); Q[7] = __dmul_rn(2.0, __dadd_rn(yz, sx)); Q[8] = __dsub_rn(1.0, __dmul_rn(2.0, __dadd_rn(xx, yy)));
}
// quat(M) -> (x, y, z, w); M is read from memory, so the run-time indices of the second branch cost nothing
VD void ex_quat(const double *M, double &qx, double &qy, double &qz, double &qw) {
    const double m00 = M[0], m11 = M[4], m22 = M[8];
    const double tr = __dadd_rn(__dadd_rn(m00, m11), m22);
    if (tr > 0.0) {
        const double s = __dsqrt_rn(__dadd_rn(tr, 1.0)), u = __ddiv_rn(0.5, s);
        qw = __dmul_rn(0.5, s);
        qx = __dmul_rn(__dsub_rn(M[7], M[5]), u); qy = __dmul_rn(__dsub_rn(M[2], M[6]), u); qz = __dmul_rn(__dsub_rn(M[3], M[1]), u);
    } else {
        int i = 0;
        if (m11 > m00) i = 1;
        if (m22 > M[i * 4]) i = 2;
        const int j = i == 2 ? 0 : i + 1, k = j == 2 ? 0 : j + 1;
        const double s = __dsqrt_rn(__dadd_rn(__dsub_rn(__dsub_rn(M[i * 4], M[j * 4]), M[k * 4]), 1.0)), u = __ddiv_rn(0.5, s);
        const double qi = __dmul_rn(0.5, s), qj = __dmul_rn(__dadd_rn(M[j * 3 + i], M[i * 3 + j]), u), qk = __dmul_rn(__dadd_rn(M[k * 3 + i], M[i * 3 + k]), u);
        qw = __dmul_rn(__dsub_rn(M[k * 3 + j], M[j * 3 + k]), u);
        qx = i == 0 ? qi : (j == 0 ? qj : qk); qy = i == 1 ? qi : (j == 1 ? qj : qk); qz = i == 2 ? qi : (j == 2 ? qj : qk);
    }
}
// atan2p of the text: y, x >= 0
VD double ex_atan2p(double y, double x) {
    const bool swapped = y > x;
    const double lo = swapped ? x : y, hi = swapped ? y : x;
    double q = hi == 0.0 ? 0.0 : __ddiv_rn(lo, hi);
#pragma unroll
    for (int it = 0; it < 3; it++) q = __ddiv_rn(q, __dadd_rn(1.0, __dsqrt_rn(__dadd_rn(1.0, __dmul_rn(q, q)))));
    const double z = __dmul_rn(q, q);
    double s = __ddiv_rn(1.0, 15.0);
    s = __dsub_rn(__ddiv_rn(1.0, 13.0), __dmul_rn(z, s)); s = __dsub_rn(__ddiv_rn(1.0, 11.0), __dmul_rn(z, s)); s = __dsub_rn(__ddiv_rn(1.0, 9.0), __dmul_rn(z, s));
    s = __dsub_rn(__ddiv_rn(1.0, 7.0), __dmul_rn(z, s)); s = __dsub_rn(__ddiv_rn(1.0, 5.0), __dmul_rn(z, s)); s = __dsub_rn(__ddiv_rn(1.0, 3.0), __dmul_rn(z, s));
    s = __dsub_rn(1.0, __dmul_rn(z, s));
    const double r = __dmul_rn(__dmul_rn(q, s), 8.0);
    return swapped ? __dsub_rn(1.5707963267948966, r) : r;
}
// C_rc = (A_r0 B_0c + A_r1 B_1c) + A_r2 B_2c, A read transposed if ta
VD void ex_mat3(const double *A, bool ta, const double *B, double *Cm) {
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++)
            Cm[r * 3 + c] = ta ? vilf_dot3(A[r], B[c], A[3 + r], B[3 + c], A[6 + r], B[6 + c]) : vilf_dot3(A[r * 3], B[c], A[r * 3 + 1], B[3 + c], A[r * 3 + 2], B[6 + c]);
}
}  // namespace

// ---- ex_hypotheses: a lane per hypothesis ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TK_F_LANES) void ex_hypotheses(ExDev d, ExPar p) {
    __shared__ double s_M[45][TK_F_LANES], s_V[81][TK_F_LANES];          // 64 512 bytes: a column per lane
    const int lane = threadIdx.x, k = blockIdx.x * TK_F_LANES + lane, slot = blockIdx.y;
    const int n = min(d.hdr[slot * EH_INTS + EH_N], EX_MAXN);
    if (blockIdx.x == 0 && lane == 0) d.best[slot] = 0ull;               // ex_score runs in a later launch
    if (!ex_searched(n, p.min_corres) || k >= p.K) return;
    const size_t first = (size_t)d.hdr[slot * EH_INTS + EH_FIRST];
    double F[9];
    const bool ok = tk_f_hypothesis(d.ua + first, d.ub + first, n, k, p.seed + (unsigned)d.fc[slot], s_M, s_V, lane, F);
    double *Fk = d.F + ((size_t)slot * p.K + k) * 9;                  // k < K rows per slot
#pragma unroll
    for (int e = 0; e < 9; e++) Fk[e] = F[e];
    d.valid[(size_t)slot * p.K + k] = ok ? 1 : 0;
}

// ---- ex_score: a wave per hypothesis ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * EX_SCORE_WAVES) void ex_score(ExDev d, ExPar p) {
    const int lane = threadIdx.x & 63, k = blockIdx.x * EX_SCORE_WAVES + (threadIdx.x >> 6), slot = blockIdx.y;
    const int n = min(d.hdr[slot * EH_INTS + EH_N], EX_MAXN);
    if (!ex_searched(n, p.min_corres) || k >= p.K || !d.valid[(size_t)slot * p.K + k]) return;      // the whole wave
    const size_t first = (size_t)d.hdr[slot * EH_INTS + EH_FIRST];
    const float2 *ua = d.ua + first, *ub = d.ub + first;
    double F[9];
#pragma unroll
    for (int e = 0; e < 9; e++) F[e] = d.F[((size_t)slot * p.K + k) * 9 + e];
    int cnt = 0;
    for (int base = 0; base < n; base += 64) {
        const int j = base + lane;
        const bool in = j < n && tk_f_inlier(F, ua[j], ub[j], p.thr2);
        cnt += __popcll(__ballot(in));
    }
    if (lane == 0) atomicMax(d.best + slot, ((unsigned long long)(cnt + 1) << 32) | (unsigned long long)(unsigned)(p.K - 1 - k));
}

// ---- ex_solve: a workgroup per slot ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EX_NT) void ex_solve(ExDev d, ExPar p) {
    __shared__ double s_M[10][TK_F_LANES], s_V[16][TK_F_LANES];          // 13 312 bytes: the decomposition's columns (wave 0), then column 0 for Jacobi(G, 4)
    __shared__ double s_B[16][EX_H + 1];                                 // 32 896 bytes: entry e of the row-major 4 x 4 block B_i at [e][i]; a thread per i writes
                                                                         // without bank conflicts, and the odd row length spreads the rows the sums read
    __shared__ double s_Rc[9];
    __shared__ int s_i[8];                                               // flags, best_k, score, front[4], chosen
    const int t = threadIdx.x, slot = blockIdx.x;
    const int n = min(d.hdr[slot * EH_INTS + EH_N], EX_MAXN);
    const int fc0 = min(max(d.fc[slot], 0), EX_H - 1);                   // the host has refused a full slot: fc0 + 1 <= EX_H rows of the histories
    double *ric = d.ric + (size_t)slot * 9;
    double *hRc = d.hist + (size_t)slot * 3 * EX_H * 9, *hRimu = hRc + (size_t)EX_H * 9, *hRcg = hRimu + (size_t)EX_H * 9;
    double *ang = d.ang + (size_t)slot * EX_H, *wgt = d.wgt + (size_t)slot * EX_H;
    vilf_exrot_result *row = d.rows + slot;
    if (n < 0) {                                                         // skipped: the state is not touched (the whole workgroup leaves)
        if (t < 9) row->ric[t] = ric[t];
        if (t == 0) { row->frame_count = d.fc[slot]; row->flags = VILF_EXROT_SKIPPED; row->count = -1; row->best_k = -1; row->chosen = -1; }
        return;
    }
    // solveRelativeR: wave 0, every lane the same numbers
    if (t < 64) {
        const int lane = t;
        int flags = 0, best_k = -1, score = 0, chosen = -1, c0 = 0, c1 = 0, c2 = 0, c3 = 0;
        double Rc[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
        if (ex_searched(n, p.min_corres)) {
            flags |= VILF_EXROT_COUNT;
            const unsigned long long word = d.best[slot];
            if (word != 0ull) {
                flags |= VILF_EXROT_HYPOTHESIS;
                best_k = min(max(p.K - 1 - (int)(unsigned)(word & 0xffffffffull), 0), p.K - 1);
                score = (int)(word >> 32) - 1;
                double E[9], R1[9], R2[9], tv[3];
#pragma unroll
                for (int e = 0; e < 9; e++) E[e] = d.F[((size_t)slot * p.K + best_k) * 9 + e];
                if (su_decompose(E, s_M, s_V, lane, R1, R2, tv)) {
                    flags |= VILF_EXROT_FINITE;
                    const size_t first = (size_t)d.hdr[slot * EH_INTS + EH_FIRST];
                    const float2 *ua = d.ua + first, *ub = d.ub + first;
                    for (int base = 0; base < n; base += 64) {
                        const int j = base + lane;
                        bool g0 = false, g1 = false, g2 = false, g3 = false;
                        if (j < n) {
                            double za, zb;
                            su_depths(R1, tv, ua[j], ub[j], za, zb);            // under -t both depths are these, negated exactly
                            g0 = za > 0.0 && zb > 0.0; g1 = -za > 0.0 && -zb > 0.0;
                            su_depths(R2, tv, ua[j], ub[j], za, zb);
                            g2 = za > 0.0 && zb > 0.0; g3 = -za > 0.0 && -zb > 0.0;
                        }
                        c0 += __popcll(__ballot(g0)); c1 += __popcll(__ballot(g1)); c2 += __popcll(__ballot(g2)); c3 += __popcll(__ballot(g3));
                    }
                    chosen = max(c0, c1) > max(c2, c3) ? 0 : 1;
#pragma unroll
                    for (int r = 0; r < 3; r++)
#pragma unroll
                        for (int c = 0; c < 3; c++) Rc[r * 3 + c] = chosen == 0 ? R1[c * 3 + r] : R2[c * 3 + r];      // Rc = ans^T
                }
            }
        }
        if (lane == 0) {
            // history: Rimu, Rc_g with the ric before this push, the append
            double Rimu[9], T[9], Rcg[9], rc[9];
#pragma unroll
            for (int e = 0; e < 9; e++) rc[e] = ric[e];
            ex_q_to_R(d.dq + (size_t)slot * 4, Rimu);
            ex_mat3(rc, true, Rimu, T);
            ex_mat3(T, false, rc, Rcg);
#pragma unroll
            for (int e = 0; e < 9; e++) { hRc[(size_t)fc0 * 9 + e] = Rc[e]; hRimu[(size_t)fc0 * 9 + e] = Rimu[e]; hRcg[(size_t)fc0 * 9 + e] = Rcg[e]; s_Rc[e] = Rc[e]; }
            s_i[0] = flags; s_i[1] = best_k; s_i[2] = score; s_i[3] = c0; s_i[4] = c1; s_i[5] = c2; s_i[6] = c3; s_i[7] = chosen;
        }
    }
    __threadfence_block();
    __syncthreads();                                                     // thread 0's append is visible to the workgroup
    const int cnt = fc0 + 1;                                             // the slot's frame_count after the push, <= EX_H <= EX_NT
    // weights and blocks: a thread per entry
    if (t < cnt) {
        double x1, y1, z1, w1, x2, y2, z2, w2;
        ex_quat(hRc + (size_t)t * 9, x1, y1, z1, w1);
        ex_quat(hRcg + (size_t)t * 9, x2, y2, z2, w2);
        const double xc = -x2, yc = -y2, zc = -z2, wc = w2;
        const double dw = __dsub_rn(__dsub_rn(__dsub_rn(__dmul_rn(w1, wc), __dmul_rn(x1, xc)), __dmul_rn(y1, yc)), __dmul_rn(z1, zc));
        const double dx = __dsub_rn(__dadd_rn(__dadd_rn(__dmul_rn(w1, xc), __dmul_rn(x1, wc)), __dmul_rn(y1, zc)), __dmul_rn(z1, yc));
        const double dy = __dsub_rn(__dadd_rn(__dadd_rn(__dmul_rn(w1, yc), __dmul_rn(y1, wc)), __dmul_rn(z1, xc)), __dmul_rn(x1, zc));
        const double dz = __dsub_rn(__dadd_rn(__dadd_rn(__dmul_rn(w1, zc), __dmul_rn(z1, wc)), __dmul_rn(x1, yc)), __dmul_rn(y1, xc));
        const double vn = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz)));
        const double a = __dmul_rn(57.29577951308232, __dmul_rn(2.0, ex_atan2p(vn, fabs(dw))));
        const double hub = a > p.huber ? __ddiv_rn(p.huber, a) : 1.0;
        ang[t] = a; wgt[t] = hub;
        double x, y, z, w;
        ex_quat(hRimu + (size_t)t * 9, x, y, z, w);
        const double L[16] = {w1, -z1, y1, x1, z1, w1, -x1, y1, -y1, x1, w1, z1, -x1, -y1, -z1, w1};
        const double R[16] = {w, z, -y, x, -z, w, x, y, y, -x, w, z, -x, -y, -z, w};
#pragma unroll
        for (int e = 0; e < 16; e++) s_B[e][t] = __dmul_rn(hub, __dsub_rn(L[e], R[e]));
    }
    __syncthreads();
    // G in the text's order: thread e sums the upper entry e
    if (t < 10) {
        int pp = 0, e = t;
        while (e >= 4 - pp) { e -= 4 - pp; pp++; }
        const int qq = pp + e;
        double acc = 0.0;
        for (int i = 0; i < cnt; i++)
#pragma unroll
            for (int r = 0; r < 4; r++) acc = __dadd_rn(acc, __dmul_rn(s_B[r * 4 + pp][i], s_B[r * 4 + qq][i]));
        s_M[t][0] = acc;                                                 // t = tk_iu(4, pp, qq)
    }
    __syncthreads();
    if (t == 0) {
        tk_jacobi<4>(s_M, s_V, 0);
        const int at = tk_smallest<4>(s_M, 0);
        double sig[4], x[4], Q[9];
#pragma unroll
        for (int k = 0; k < 4; k++) { const double g = s_M[tk_iu(4, k, k)][0]; sig[k] = g > 0.0 ? __dsqrt_rn(g) : 0.0; x[k] = s_V[k * 4 + at][0]; }
        // descending, a fixed network of five exchanges
#define EX_CSWAP(i, j) { const double hi_ = sig[i] < sig[j] ? sig[j] : sig[i], lo_ = sig[i] < sig[j] ? sig[i] : sig[j]; sig[i] = hi_; sig[j] = lo_; }
        EX_CSWAP(0, 1) EX_CSWAP(2, 3) EX_CSWAP(0, 2) EX_CSWAP(1, 3) EX_CSWAP(1, 2)
#undef EX_CSWAP
        ex_q_to_R(x, Q);
        row->frame_count = cnt; row->flags = s_i[0]; row->count = n; row->best_k = s_i[1]; row->score = s_i[2];
        row->front[0] = s_i[3]; row->front[1] = s_i[4]; row->front[2] = s_i[5]; row->front[3] = s_i[6];
        row->chosen = s_i[7]; row->ok = (cnt >= p.min_frames && sig[2] > p.min_sigma) ? 1 : 0;
        row->angle = ang[fc0]; row->weight = wgt[fc0];                   // written by thread fc0 before the barriers above
#pragma unroll
        for (int e = 0; e < 9; e++) row->Rc[e] = s_Rc[e];
#pragma unroll
        for (int k = 0; k < 4; k++) { row->sigma[k] = sig[k]; row->x[k] = x[k]; }
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) { const double v = Q[c * 3 + r]; ric[r * 3 + c] = v; row->ric[r * 3 + c] = v; }
        d.fc[slot] = cnt;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
namespace {
bool ex_finite_pos(double v) { return std::isfinite(v) && v > 0; }
// the state: frame_count and ric of every slot first (what a reset uploads), then the histories, the angles and the weights
struct ExState { size_t fc, ric, hist, ang, wgt, bytes; };
ExState ex_state(int S) {
    Layout l;
    ExState o;
    o.fc = l.take((size_t)S * 4); o.ric = l.take((size_t)S * 72); o.hist = l.take((size_t)S * 3 * EX_H * 72); o.ang = l.take((size_t)S * EX_H * 8);
    o.wgt = l.take((size_t)S * EX_H * 8); o.bytes = l.at;
    return o;
}
}  // namespace

extern "C" void vilf_exrot_default_params(vilf_exrot_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->n_hypotheses = 512; p->seed = 0; p->min_corres = 9; p->min_frames = 10;
    p->ransac_threshold = 3.0; p->huber_deg = 5.0; p->min_sigma = 0.25;
}

extern "C" int vilf_exrot_reset(vilf_handle *h, int n_slots) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    if (n_slots < 1 || n_slots > VILF_EXROT_MAX_SLOTS) { h->err = "vilf_exrot_reset: 1 <= n_slots <= VILF_EXROT_MAX_SLOTS"; return VILF_ERR_INVALID_ARGUMENT; }
    HIPCHECK(h, hipSetDevice(h->device));
    ExrotCtx *c = vilf_stage_make<ExrotCtx>(h, ST_EXROT);
    const ExState o = ex_state(n_slots);
    c->n_slots = 0;                               // the layout depends on the number of slots: nothing of the old state survives
    if (!c->state.ensure(o.bytes) || !c->io.up.ensure(o.hist)) { h->err = "vilf_exrot_reset: out of memory"; return VILF_ERR_DEVICE; }
    char *ub = (char *)c->io.up.p;
    std::memset(ub, 0, o.hist);
    for (int s = 0; s < n_slots; s++) { double *r = (double *)(ub + o.ric) + (size_t)s * 9; r[0] = r[4] = r[8] = 1.0; }
    HIPCHECK(h, vilf_copy_sync(h, c->state.p, ub, o.hist, hipMemcpyHostToDevice));
    c->n_slots = n_slots;
    c->fc.assign((size_t)n_slots, 0);
    return VILF_OK;
}

extern "C" int vilf_exrot_push(vilf_handle *h, const vilf_exrot_params *p, int n_slots, const vilf_exrot_pair *pairs, vilf_exrot_result *out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    if (!p || !pairs || !out) { h->err = "vilf_exrot_push: null pointer"; return VILF_ERR_INVALID_ARGUMENT; }
    ExrotCtx *c = vilf_stage<ExrotCtx>(h, ST_EXROT);
    if (n_slots < 1 || n_slots > VILF_EXROT_MAX_SLOTS || !c || n_slots != c->n_slots) {
        h->err = "vilf_exrot_push: n_slots is outside 1 .. VILF_EXROT_MAX_SLOTS or not that of the last vilf_exrot_reset"; return VILF_ERR_INVALID_ARGUMENT;
    }
    if (p->n_hypotheses < 1 || p->n_hypotheses > EX_MAXK || !ex_finite_pos(p->ransac_threshold) || !ex_finite_pos(p->huber_deg) || !ex_finite_pos(p->min_sigma) ||
        p->min_corres < 0 || p->min_frames < 0) {
        h->err = "vilf_exrot_push: 1 <= n_hypotheses <= VILF_TRACK_MAX_HYPOTHESES, positive finite threshold, huber_deg and min_sigma, counts >= 0";
        return VILF_ERR_INVALID_ARGUMENT;
    }
    size_t total = 0;
    for (int s = 0; s < n_slots; s++) {
        const vilf_exrot_pair &P = pairs[s];
        if (P.n < -1 || P.n > VILF_MAX_FEATURES) { h->err = "vilf_exrot_push: -1 <= n <= VILF_MAX_FEATURES"; return VILF_ERR_INVALID_ARGUMENT; }
        if (P.n < 0) continue;
        if (P.n > 0 && (!P.a || !P.b)) { h->err = "vilf_exrot_push: null pointer in a pair"; return VILF_ERR_INVALID_ARGUMENT; }
        if (c->fc[s] >= EX_H) { h->err = "vilf_exrot_push: a slot holds VILF_EXROT_MAX_HISTORY entries; reset"; return VILF_ERR_INVALID_ARGUMENT; }
        for (int e = 0; e < 4; e++)
            if (!std::isfinite(P.delta_q[e])) { h->err = "vilf_exrot_push: a delta_q entry that is not finite"; return VILF_ERR_INVALID_ARGUMENT; }
        for (size_t e = 0; e < (size_t)P.n * 2; e++)
            if (!std::isfinite(P.a[e]) || !std::isfinite(P.b[e])) { h->err = "vilf_exrot_push: a coordinate that is not finite"; return VILF_ERR_INVALID_ARGUMENT; }
        total += (size_t)P.n;
    }
    HIPCHECK(h, hipSetDevice(h->device));
    const int S = n_slots, K = p->n_hypotheses;
    const size_t rows = std::max<size_t>(total, 1);
    // upload: the slots' integers, delta_q, then the points of both sides as float32
    Layout li, lw;
    const size_t i_hdr = li.take((size_t)S * EH_INTS * 4), i_dq = li.take((size_t)S * 32), i_ua = li.take(rows * 8), i_ub = li.take(rows * 8), in_bytes = li.at;
    const size_t o_F = lw.take((size_t)S * K * 72), o_valid = lw.take((size_t)S * K * 4), o_best = lw.take((size_t)S * 8), work_bytes = lw.at;
    const size_t out_bytes = (size_t)S * sizeof(vilf_exrot_result);
    if (!c->io.ensure(in_bytes, out_bytes) || !c->work.ensure(work_bytes)) {
        h->err = "vilf_exrot_push: out of memory"; return VILF_ERR_DEVICE;
    }
    {
        char *ub = (char *)c->io.up.p;
        int *hdr = (int *)(ub + i_hdr);
        double *dq = (double *)(ub + i_dq);
        float *ua = (float *)(ub + i_ua), *ubp = (float *)(ub + i_ub);
        size_t at = 0;
        for (int s = 0; s < S; s++) {
            const vilf_exrot_pair &P = pairs[s];
            hdr[s * EH_INTS + EH_N] = P.n; hdr[s * EH_INTS + EH_FIRST] = (int)at;
            for (int e = 0; e < 4; e++) dq[(size_t)s * 4 + e] = P.n >= 0 ? P.delta_q[e] : 0.0;
            for (int j = 0; j < P.n; j++) {
                ua[(at + j) * 2] = (float)P.a[j * 2]; ua[(at + j) * 2 + 1] = (float)P.a[j * 2 + 1];
                ubp[(at + j) * 2] = (float)P.b[j * 2]; ubp[(at + j) * 2 + 1] = (float)P.b[j * 2 + 1];
            }
            if (P.n > 0) at += (size_t)P.n;
        }
    }
    HIPCHECK(h, c->io.upload(h, in_bytes));
    // the result rows start from 0: a kernel writes only what the text gives a value
    HIPCHECK(h, hipMemsetAsync(c->io.out.p, 0, out_bytes, h->stream));
    const ExState o = ex_state(S);
    ExDev d;
    char *ib = c->io.in.as<char>(), *wb = c->work.as<char>(), *sb = c->state.as<char>();
    d.hdr = (const int *)(ib + i_hdr); d.dq = (const double *)(ib + i_dq); d.ua = (const float2 *)(ib + i_ua); d.ub = (const float2 *)(ib + i_ub);
    d.fc = (int *)(sb + o.fc); d.ric = (double *)(sb + o.ric); d.hist = (double *)(sb + o.hist); d.ang = (double *)(sb + o.ang); d.wgt = (double *)(sb + o.wgt);
    d.F = (double *)(wb + o_F); d.valid = (int *)(wb + o_valid); d.best = (unsigned long long *)(wb + o_best);
    d.rows = c->io.out.as<vilf_exrot_result>();
    ExPar ep;
    ep.K = K; ep.seed = p->seed; ep.min_corres = p->min_corres; ep.min_frames = p->min_frames;
    ep.thr2 = p->ransac_threshold * p->ransac_threshold; ep.huber = p->huber_deg; ep.min_sigma = p->min_sigma;
    ProfMarks prof(h, c->prof);
    hipLaunchKernelGGL(ex_hypotheses, dim3((K + TK_F_LANES - 1) / TK_F_LANES, S), dim3(TK_F_LANES), 0, h->stream, d, ep);
    prof.mark(0);
    hipLaunchKernelGGL(ex_score, dim3((K + EX_SCORE_WAVES - 1) / EX_SCORE_WAVES, S), dim3(64 * EX_SCORE_WAVES), 0, h->stream, d, ep);
    prof.mark(1);
    hipLaunchKernelGGL(ex_solve, dim3(S), dim3(EX_NT), 0, h->stream, d, ep);
    prof.mark(2);
    HIPCHECK(h, hipGetLastError());
    HIPCHECK(h, c->io.download(h, out_bytes));
    std::memcpy(out, c->io.down.p, out_bytes);
    for (int s = 0; s < S; s++) if (pairs[s].n >= 0) c->fc[s] += 1;
    return VILF_OK;
}

extern "C" int vilf_exrot_get_history(vilf_handle *h, int slot, int *count_out, double *Rc_out, double *Rimu_out, double *Rcg_out, double *angle_out, double *weight_out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    ExrotCtx *c = vilf_stage<ExrotCtx>(h, ST_EXROT);
    if (!count_out || !c || c->n_slots < 1 || slot < 0 || slot >= c->n_slots) {
        h->err = "vilf_exrot_get_history: a null count_out, no vilf_exrot_reset yet or a slot outside 0 .. n_slots - 1"; return VILF_ERR_INVALID_ARGUMENT;
    }
    HIPCHECK(h, hipSetDevice(h->device));
    const ExState o = ex_state(c->n_slots);
    const int cnt = std::min(c->fc[(size_t)slot], EX_H);
    const size_t hb = (size_t)EX_H * 72, bytes = 3 * hb + 2 * (size_t)EX_H * 8;
    if (!c->io.down.ensure(bytes)) { h->err = "vilf_exrot_get_history: out of memory"; return VILF_ERR_DEVICE; }
    char *db = (char *)c->io.down.p;
    const char *sb = c->state.as<char>();
    if (cnt > 0) {
        HIPCHECK(h, hipMemcpyAsync(db, sb + o.hist + (size_t)slot * 3 * hb, 3 * hb, hipMemcpyDeviceToHost, h->stream));
        HIPCHECK(h, hipMemcpyAsync(db + 3 * hb, sb + o.ang + (size_t)slot * EX_H * 8, (size_t)EX_H * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHECK(h, hipMemcpyAsync(db + 3 * hb + (size_t)EX_H * 8, sb + o.wgt + (size_t)slot * EX_H * 8, (size_t)EX_H * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHECK(h, hipStreamSynchronize(h->stream));
    }
    *count_out = cnt;
    if (Rc_out) std::memcpy(Rc_out, db, (size_t)cnt * 72);
    if (Rimu_out) std::memcpy(Rimu_out, db + hb, (size_t)cnt * 72);
    if (Rcg_out) std::memcpy(Rcg_out, db + 2 * hb, (size_t)cnt * 72);
    if (angle_out) std::memcpy(angle_out, db + 3 * hb, (size_t)cnt * 8);
    if (weight_out) std::memcpy(weight_out, db + 3 * hb + (size_t)EX_H * 8, (size_t)cnt * 8);
    return VILF_OK;
}

extern "C" int vilf_exrot_profile(vilf_handle *h, double ms_out[3], long launches_out[3]) { return vilf_stage_profile(h, ST_EXROT, &ExrotCtx::prof, ms_out, launches_out); }
