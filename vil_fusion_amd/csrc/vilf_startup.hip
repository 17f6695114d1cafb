// vilf_startup.hip — the first stage of the visual start-up on the device (≙ Estimator::relativePose, estimator.cpp:461-490, with getCorresponding and
//   solveRelativeRT). The arithmetic is stated once, in include/vilfusion.h ("Visual start-up: relativePose"); the search is the tracker's (vilf_fmat.hpp);
//   the decomposition and the depths are shared with the rotation calibration (vilf_pose.hpp).
// All pairs of all windows = one chain of four launches on the handle's stream, slot = window * SU_NP + pair; the host waits once, at the one download:
//   su_gather      a workgroup per (pair, window): membership flags in LDS, rank counting -> the correspondences in feature order as float32 points, the
//                  parallax sum (wave 0: strided partials, fixed butterfly), count and gate flags
//   su_hypotheses  grid (ceil(K / 64), pair, window), a lane per hypothesis: tk_f_hypothesis on the slot's points; a pair whose gates failed leaves at once
//   su_score       grid (ceil(K / 4), pair, window), a wave per hypothesis: ballot + popcount, one packed 64-bit atomicMax per hypothesis
//   su_pose        a wave per (pair, window): the winner's mask again, E^T E through the same Jacobi (every lane the same numbers in its own LDS column), the four
//                  cheirality counts by ballot, the choice, the row, the points of the chosen candidate, atomicMin of the pair index into the window's l
#include <hip/hip_runtime.h>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include "vilf_internal.hpp"
#include "vilf_device.hpp"
#include "vilf_fmat.hpp"
#include "vilf_pose.hpp"

#define SU_NP (VILF_MAX_FRAMES - 1)         // pairs of a window
#define SU_MAXN VILF_MAX_FEATURES            // correspondences of a pair
#define SU_MAXK VILF_TRACK_MAX_HYPOTHESES
#define SU_STAGES 4
#define SU_WIN_INTS VILF_SU_WIN_INTS               // a window's integers on the device (vilf_internal.hpp)
static_assert(SU_WIN_INTS % 2 == 0, "the points behind the integers are 8-byte aligned");
enum { SC_M = 0, SC_FLAGS = 1, SC_BEST = 2 /* unsigned long long at ints 2, 3: (score + 1) << 32 | (K - 1 - k); 0 = no valid hypothesis */, SC_INTS = 8 };

// the device arrays of one call; everything is indexed by slot (or by window for lwin)
struct SuDev {
    const int *win; const double *pts;               // the uploaded windows
    float2 *ua, *ub; int *ctl; double *F; int *valid;      // [slot][SU_MAXN], [slot][SC_INTS], [slot][K][9], [slot][K]
    int *lwin; vilf_startup_pair *rows; int *feat; unsigned char *mask; double *points;      // the download: [window], [slot], [slot][SU_MAXN] ..
};
struct SuPar { int K; unsigned seed; int min_count, min_solve, min_inliers; double thr2, focal, min_parallax, dist; };

// ---- launch contract -----------------------------------------------------------------------------------------------------
#define SU_NT 256                           // su_gather: grid (SU_NP, windows), one workgroup per slot
#define SU_SCORE_WAVES 4                    // su_score: block 256, grid (ceil(K / 4), SU_NP, windows), a wave per hypothesis; no workgroup barrier
                                            // su_hypotheses: block TK_F_LANES (one wave), grid (ceil(K / 64), SU_NP, windows); su_pose: block 64, grid (SU_NP, windows)
__global__ void su_gather(SuDev d, SuPar p);
__global__ void su_hypotheses(SuDev d, SuPar p);
__global__ void su_score(SuDev d, SuPar p);
__global__ void su_pose(SuDev d, SuPar p);

struct StartupCtx : VilfStage {
    StageIO io;
    DBuf work;
    int last_windows = 0;
    StageProf<SU_STAGES> prof;
    void profile_reset() override { prof.reset(); }
};

namespace {
VD bool su_searched(int flags) { return (flags & (VILF_SU_COUNT | VILF_SU_PARALLAX | VILF_SU_SOLVE_COUNT)) == (VILF_SU_COUNT | VILF_SU_PARALLAX | VILF_SU_SOLVE_COUNT); }
VD bool su_good(double z1, double z2, double dist) { return z1 > 0.0 && z1 < dist && z2 > 0.0 && z2 < dist; }
}  // namespace

// ---- su_gather: a workgroup per slot ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SU_NT) void su_gather(SuDev d, SuPar p) {
    __shared__ unsigned char s_in[SU_MAXN];
    __shared__ double s_d[SU_MAXN];
    __shared__ int s_m;
    const int t = threadIdx.x, i = blockIdx.x, w = blockIdx.y, slot = w * SU_NP + i;
    const int *win = d.win + (size_t)w * SU_WIN_INTS, *start = win + 4, *first = win + 4 + SU_MAXN;
    const int newest = win[0] - 1, n = min(win[1], SU_MAXN);          // the host has checked both
    const double *pts = d.pts + (size_t)win[2] * 2;
    float2 *ua = d.ua + (size_t)slot * SU_MAXN, *ub = d.ub + (size_t)slot * SU_MAXN;
    int *feat = d.feat + (size_t)slot * SU_MAXN;
    for (int f = t; f < n; f += SU_NT) {
        const int st = start[f], nobs = first[f + 1] - first[f];
        s_in[f] = (i < newest && st <= i && st + nobs - 1 >= newest) ? 1 : 0;
    }
    __syncthreads();
    for (int f = t; f < n; f += SU_NT) {
        if (!s_in[f]) continue;
        int rank = 0;
        for (int j = 0; j < f; j++) rank += s_in[j];           // feature order; rank < n <= SU_MAXN, the rows of ua, ub, feat, s_d
        const int st = start[f];
        const double *pa = pts + (size_t)(first[f] + i - st) * 2, *pb = pts + (size_t)(first[f] + newest - st) * 2;      // 0 <= i - st <= newest - st < n_obs
        const float2 a = make_float2((float)pa[0], (float)pa[1]), b = make_float2((float)pb[0], (float)pb[1]);
        ua[rank] = a; ub[rank] = b; feat[rank] = f;
        const double dx = __dsub_rn((double)a.x, (double)b.x), dy = __dsub_rn((double)a.y, (double)b.y);
        s_d[rank] = __dsqrt_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)));
    }
    if (t == 0) {
        int m = 0;
        for (int j = 0; j < n; j++) m += s_in[j];
        s_m = m;
    }
    __syncthreads();
    const int m = s_m;
    for (int j = m + t; j < SU_MAXN; j += SU_NT) feat[j] = 0;       // the download is 0 behind the count
    if (t < 64) {                                                   // wave 0: the parallax sum in the text's order
        double acc = 0.0;
        for (int j = t; j < m; j += 64) acc = __dadd_rn(acc, s_d[j]);
        for (int o = 32; o > 0; o >>= 1) acc = __dadd_rn(acc, __shfl_xor(acc, o));
        if (t == 0) {
            const double par = m > 0 ? __dmul_rn(__ddiv_rn(acc, (double)m), p.focal) : 0.0;
            int flags = 0;
            if (m > p.min_count) flags |= VILF_SU_COUNT;
            if (par > p.min_parallax) flags |= VILF_SU_PARALLAX;
            if (m >= p.min_solve && m >= 8) flags |= VILF_SU_SOLVE_COUNT;
            int *ctl = d.ctl + (size_t)slot * SC_INTS;
            ctl[SC_M] = m; ctl[SC_FLAGS] = flags;
            *(unsigned long long *)(ctl + SC_BEST) = 0ull;
            d.rows[slot].parallax = par;
            if (i == 0) d.lwin[w] = INT_MAX;
        }
    }
}

// ---- su_hypotheses: a lane per hypothesis ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TK_F_LANES) void su_hypotheses(SuDev d, SuPar p) {
    __shared__ double s_M[45][TK_F_LANES], s_V[81][TK_F_LANES];          // 64 512 bytes: a column per lane
    const int lane = threadIdx.x, k = blockIdx.x * TK_F_LANES + lane, slot = blockIdx.z * SU_NP + blockIdx.y;
    const int *ctl = d.ctl + (size_t)slot * SC_INTS;
    const int n = min(ctl[SC_M], SU_MAXN);
    if (!su_searched(ctl[SC_FLAGS]) || n < 8 || k >= p.K) return;
    double F[9];
    const bool ok = tk_f_hypothesis(d.ua + (size_t)slot * SU_MAXN, d.ub + (size_t)slot * SU_MAXN, n, k, p.seed + (unsigned)blockIdx.y, s_M, s_V, lane, F);
    double *Fk = d.F + ((size_t)slot * p.K + k) * 9;                  // k < K rows per slot
#pragma unroll
    for (int e = 0; e < 9; e++) Fk[e] = F[e];
    d.valid[(size_t)slot * p.K + k] = ok ? 1 : 0;
}

// ---- su_score: a wave per hypothesis ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * SU_SCORE_WAVES) void su_score(SuDev d, SuPar p) {
    const int lane = threadIdx.x & 63, k = blockIdx.x * SU_SCORE_WAVES + (threadIdx.x >> 6), slot = blockIdx.z * SU_NP + blockIdx.y;
    int *ctl = d.ctl + (size_t)slot * SC_INTS;
    const int n = min(ctl[SC_M], SU_MAXN);
    if (!su_searched(ctl[SC_FLAGS]) || n < 8 || k >= p.K || !d.valid[(size_t)slot * p.K + k]) return;      // the whole wave
    const float2 *ua = d.ua + (size_t)slot * SU_MAXN, *ub = d.ub + (size_t)slot * SU_MAXN;
    double F[9];
#pragma unroll
    for (int e = 0; e < 9; e++) F[e] = d.F[((size_t)slot * p.K + k) * 9 + e];
    int cnt = 0;
    for (int base = 0; base < n; base += 64) {
        const int j = base + lane;
        const bool in = j < n && tk_f_inlier(F, ua[j], ub[j], p.thr2);
        cnt += __popcll(__ballot(in));
    }
    if (lane == 0) atomicMax((unsigned long long *)(ctl + SC_BEST), ((unsigned long long)(cnt + 1) << 32) | (unsigned long long)(unsigned)(p.K - 1 - k));
}

// ---- su_pose: a wave per slot ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void su_pose(SuDev d, SuPar p) {
    __shared__ double s_M[6][TK_F_LANES], s_V[9][TK_F_LANES];            // 7 680 bytes: every lane decomposes the same E in its own column
    const int lane = threadIdx.x, i = blockIdx.x, w = blockIdx.y, slot = w * SU_NP + i;
    const int *ctl = d.ctl + (size_t)slot * SC_INTS;
    const int n = min(ctl[SC_M], SU_MAXN);
    int flags = ctl[SC_FLAGS];
    const unsigned long long word = *(const unsigned long long *)(ctl + SC_BEST);
    const float2 *ua = d.ua + (size_t)slot * SU_MAXN, *ub = d.ub + (size_t)slot * SU_MAXN;
    unsigned char *mask = d.mask + (size_t)slot * SU_MAXN;
    double *points = d.points + (size_t)slot * SU_MAXN * 3;
    int best_k = -1, score = 0, chosen = -1, inl = 0, c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    double E[9], R1[9], R2[9], tv[3], Rc[9], tc[3];
#pragma unroll
    for (int e = 0; e < 9; e++) { E[e] = 0.0; R1[e] = 0.0; R2[e] = 0.0; Rc[e] = 0.0; }
    tv[0] = tv[1] = tv[2] = 0.0; tc[0] = tc[1] = tc[2] = 0.0;
    const bool searched = su_searched(flags) && n >= 8 && word != 0ull;
    if (searched) {
        flags |= VILF_SU_HYPOTHESIS;
        best_k = min(max(p.K - 1 - (int)(unsigned)(word & 0xffffffffull), 0), p.K - 1);
        score = (int)(word >> 32) - 1;
#pragma unroll
        for (int e = 0; e < 9; e++) E[e] = d.F[((size_t)slot * p.K + best_k) * 9 + e];
        const bool fin = su_decompose(E, s_M, s_V, lane, R1, R2, tv);        // G = E^T E and its Jacobi, R1, R2, t = u3 (vilf_pose.hpp)
        if (fin) {
            flags |= VILF_SU_FINITE;
            for (int base = 0; base < n; base += 64) {
                const int j = base + lane;
                bool g0 = false, g1 = false, g2 = false, g3 = false;
                if (j < n && tk_f_inlier(E, ua[j], ub[j], p.thr2)) {
                    double za, zb;
                    su_depths(R1, tv, ua[j], ub[j], za, zb);            // under -t both depths are these, negated exactly
                    g0 = su_good(za, zb, p.dist); g2 = su_good(-za, -zb, p.dist);
                    su_depths(R2, tv, ua[j], ub[j], za, zb);
                    g1 = su_good(za, zb, p.dist); g3 = su_good(-za, -zb, p.dist);
                }
                c0 += __popcll(__ballot(g0)); c1 += __popcll(__ballot(g1)); c2 += __popcll(__ballot(g2)); c3 += __popcll(__ballot(g3));
            }
            if (c0 >= c1 && c0 >= c2 && c0 >= c3) { chosen = 0; inl = c0; }
            else if (c1 >= c0 && c1 >= c2 && c1 >= c3) { chosen = 1; inl = c1; }
            else if (c2 >= c0 && c2 >= c1 && c2 >= c3) { chosen = 2; inl = c2; }
            else { chosen = 3; inl = c3; }
            if (inl > p.min_inliers) flags |= VILF_SU_INLIERS;
#pragma unroll
            for (int e = 0; e < 9; e++) Rc[e] = (chosen & 1) ? R2[e] : R1[e];
#pragma unroll
            for (int r = 0; r < 3; r++) tc[r] = (chosen & 2) ? -tv[r] : tv[r];
        } else {
#pragma unroll
            for (int e = 0; e < 9; e++) { R1[e] = 0.0; R2[e] = 0.0; }
        }
    }
    // the per-correspondence outputs, 0 behind the count and for a pair without a chosen candidate
    for (int base = 0; base < SU_MAXN; base += 64) {
        const int j = base + lane;
        if (j >= SU_MAXN) break;
        unsigned char mk = 0;
        double x = 0.0, y = 0.0, z = 0.0;
        if (searched && j < n && tk_f_inlier(E, ua[j], ub[j], p.thr2)) {
            mk = 1;
            if (chosen >= 0) {
                double za, zb;
                su_depths(Rc, tc, ua[j], ub[j], za, zb);
                if (su_good(za, zb, p.dist)) { mk = 3; x = __dmul_rn(za, (double)ua[j].x); y = __dmul_rn(za, (double)ua[j].y); z = za; }
            }
        }
        mask[j] = mk; points[(size_t)j * 3] = x; points[(size_t)j * 3 + 1] = y; points[(size_t)j * 3 + 2] = z;
    }
    if (lane == 0) {
        vilf_startup_pair *row = d.rows + slot;                      // parallax is su_gather's
        row->count = n; row->flags = flags; row->best_k = best_k; row->score = score;
        row->cheirality[0] = c0; row->cheirality[1] = c1; row->cheirality[2] = c2; row->cheirality[3] = c3;
        row->chosen = chosen; row->inlier_cnt = inl;
#pragma unroll
        for (int e = 0; e < 9; e++) row->F[e] = E[e];
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) row->R[r * 3 + c] = Rc[c * 3 + r];             // Rotation = R^T
            row->T[r] = chosen >= 0 ? -vilf_dot3(Rc[r], tc[0], Rc[3 + r], tc[1], Rc[6 + r], tc[2]) : 0.0;
        }
        if (flags == VILF_SU_PASS) atomicMin(d.lwin + w, i);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
namespace {
// the download: l of every window, the rows, then the per-correspondence arrays
struct SuOut { size_t lwin, rows, feat, mask, points, bytes; };
SuOut su_out(int W) {
    const size_t slots = (size_t)W * SU_NP;
    Layout l;
    SuOut o;
    o.lwin = l.take((size_t)W * 4); o.rows = l.take(slots * sizeof(vilf_startup_pair)); o.feat = l.take(slots * SU_MAXN * 4); o.mask = l.take(slots * SU_MAXN);
    o.points = l.take(slots * SU_MAXN * 24); o.bytes = l.at;
    return o;
}
bool su_finite_pos(double v) { return std::isfinite(v) && v > 0; }
}  // namespace

// the checks of the windows that both stages of the start-up make (who = the entry point, for the message) -> *total_out = the rows of all pts
int vilf_startup_check_windows(vilf_handle *h, const char *who, int n_windows, const vilf_startup_window *windows, size_t *total_out) {
    size_t total = 0;
    for (int w = 0; w < n_windows; w++) {
        const vilf_startup_window &W = windows[w];
        if (W.n_frames < 2 || W.n_frames > VILF_MAX_FRAMES || W.n_features < 0 || W.n_features > VILF_MAX_FEATURES) {
            h->err = std::string(who) + ": 2 <= n_frames <= VILF_MAX_FRAMES, 0 <= n_features <= VILF_MAX_FEATURES"; return VILF_ERR_INVALID_ARGUMENT;
        }
        if (!W.first_obs || (W.n_features > 0 && !W.start_frame)) { h->err = std::string(who) + ": null pointer in a window"; return VILF_ERR_INVALID_ARGUMENT; }
        if (W.first_obs[0] != 0) { h->err = std::string(who) + ": first_obs[0] != 0"; return VILF_ERR_INVALID_ARGUMENT; }
        for (int f = 0; f < W.n_features; f++) {
            const long long nobs = (long long)W.first_obs[f + 1] - W.first_obs[f];
            if (nobs < 0 || W.start_frame[f] < 0 || (long long)W.start_frame[f] + nobs > W.n_frames) {
                h->err = std::string(who) + ": first_obs decreases, start_frame < 0 or start_frame + n_obs > n_frames"; return VILF_ERR_INVALID_ARGUMENT;
            }
        }
        const size_t rows = (size_t)W.first_obs[W.n_features];          // <= n_features * n_frames
        if (rows > 0 && !W.pts) { h->err = std::string(who) + ": null pointer in a window"; return VILF_ERR_INVALID_ARGUMENT; }
        for (size_t e = 0; e < rows * 2; e++)
            if (!std::isfinite(W.pts[e])) { h->err = std::string(who) + ": a coordinate that is not finite"; return VILF_ERR_INVALID_ARGUMENT; }
        total += rows;
    }
    *total_out = total;
    return VILF_OK;
}
// the windows as the kernels read them: SU_WIN_INTS integers per window, then all points
void vilf_startup_pack_windows(int n_windows, const vilf_startup_window *windows, int *ints, double *pts) {
    size_t at = 0;
    for (int w = 0; w < n_windows; w++) {
        const vilf_startup_window &Wn = windows[w];
        int *wi = ints + (size_t)w * SU_WIN_INTS;
        std::memset(wi, 0, (size_t)SU_WIN_INTS * 4);
        wi[0] = Wn.n_frames; wi[1] = Wn.n_features; wi[2] = (int)at;
        if (Wn.n_features > 0) std::memcpy(wi + 4, Wn.start_frame, (size_t)Wn.n_features * 4);
        std::memcpy(wi + 4 + SU_MAXN, Wn.first_obs, (size_t)(Wn.n_features + 1) * 4);
        const size_t rows = (size_t)Wn.first_obs[Wn.n_features];
        if (rows > 0) std::memcpy(pts + at * 2, Wn.pts, rows * 16);
        at += rows;
    }
}

extern "C" void vilf_startup_default_params(vilf_startup_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->n_hypotheses = 512; p->seed = 0; p->min_count = 20; p->min_solve_count = 15; p->min_inliers = 12;
    p->ransac_threshold = 0.3 / 460.0; p->focal_length = 460.0; p->min_parallax = 30.0; p->distance_threshold = 50.0;
}

extern "C" int vilf_startup_relative_pose(vilf_handle *h, const vilf_startup_params *p, int n_windows, const vilf_startup_window *windows, vilf_startup_result *out,
                                          vilf_startup_pair *pairs_out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    if (!p || !windows || !out) { h->err = "vilf_startup_relative_pose: null pointer"; return VILF_ERR_INVALID_ARGUMENT; }
    if (n_windows < 1 || n_windows > VILF_STARTUP_MAX_WINDOWS) { h->err = "vilf_startup_relative_pose: 1 <= n_windows <= VILF_STARTUP_MAX_WINDOWS"; return VILF_ERR_INVALID_ARGUMENT; }
    if (p->n_hypotheses < 1 || p->n_hypotheses > SU_MAXK || !su_finite_pos(p->ransac_threshold) || !su_finite_pos(p->focal_length) || !su_finite_pos(p->distance_threshold) ||
        !std::isfinite(p->min_parallax) || p->min_count < 0 || p->min_solve_count < 0 || p->min_inliers < 0) {
        h->err = "vilf_startup_relative_pose: 1 <= n_hypotheses <= VILF_TRACK_MAX_HYPOTHESES, positive finite threshold, focal length and distance, a finite min_parallax, count gates >= 0";
        return VILF_ERR_INVALID_ARGUMENT;
    }
    size_t total = 0;
    { const int rcw = vilf_startup_check_windows(h, "vilf_startup_relative_pose", n_windows, windows, &total); if (rcw != VILF_OK) return rcw; }
    HIPCHECK(h, hipSetDevice(h->device));
    StartupCtx *c = vilf_stage_make<StartupCtx>(h, ST_STARTUP);
    c->last_windows = 0;
    const int W = n_windows, K = p->n_hypotheses;
    const size_t slots = (size_t)W * SU_NP;
    // upload: the windows' integers, then all points
    const size_t in_ints = (size_t)W * SU_WIN_INTS * 4, in_bytes = in_ints + std::max<size_t>(total, 1) * 16;
    Layout lw;
    const size_t o_ua = lw.take(slots * SU_MAXN * 8), o_ub = lw.take(slots * SU_MAXN * 8), o_ctl = lw.take(slots * SC_INTS * 4), o_F = lw.take(slots * (size_t)K * 72),
                 o_valid = lw.take(slots * (size_t)K * 4), work_bytes = lw.at;
    const SuOut o = su_out(W);
    if (!c->io.ensure(in_bytes, o.bytes) || !c->work.ensure(work_bytes)) {
        h->err = "vilf_startup_relative_pose: out of memory"; return VILF_ERR_DEVICE;
    }
    vilf_startup_pack_windows(W, windows, (int *)c->io.up.p, (double *)((char *)c->io.up.p + in_ints));
    HIPCHECK(h, c->io.upload(h, in_bytes));
    SuDev d;
    char *ib = c->io.in.as<char>(), *wb = c->work.as<char>(), *ob = c->io.out.as<char>();
    d.win = (const int *)ib; d.pts = (const double *)(ib + in_ints);
    d.ua = (float2 *)(wb + o_ua); d.ub = (float2 *)(wb + o_ub); d.ctl = (int *)(wb + o_ctl); d.F = (double *)(wb + o_F); d.valid = (int *)(wb + o_valid);
    d.lwin = (int *)(ob + o.lwin); d.rows = (vilf_startup_pair *)(ob + o.rows); d.feat = (int *)(ob + o.feat); d.mask = (unsigned char *)(ob + o.mask);
    d.points = (double *)(ob + o.points);
    SuPar sp;
    sp.K = K; sp.seed = p->seed; sp.min_count = p->min_count; sp.min_solve = p->min_solve_count; sp.min_inliers = p->min_inliers;
    sp.thr2 = p->ransac_threshold * p->ransac_threshold; sp.focal = p->focal_length; sp.min_parallax = p->min_parallax; sp.dist = p->distance_threshold;
    ProfMarks prof(h, c->prof);
    hipLaunchKernelGGL(su_gather, dim3(SU_NP, W), dim3(SU_NT), 0, h->stream, d, sp);
    prof.mark(0);
    hipLaunchKernelGGL(su_hypotheses, dim3((K + TK_F_LANES - 1) / TK_F_LANES, SU_NP, W), dim3(TK_F_LANES), 0, h->stream, d, sp);
    prof.mark(1);
    hipLaunchKernelGGL(su_score, dim3((K + SU_SCORE_WAVES - 1) / SU_SCORE_WAVES, SU_NP, W), dim3(64 * SU_SCORE_WAVES), 0, h->stream, d, sp);
    prof.mark(2);
    hipLaunchKernelGGL(su_pose, dim3(SU_NP, W), dim3(64), 0, h->stream, d, sp);
    prof.mark(3);
    HIPCHECK(h, hipGetLastError());
    HIPCHECK(h, c->io.download(h, o.bytes));
    const char *hb = (const char *)c->io.down.p;
    const int *lwin = (const int *)(hb + o.lwin);
    const vilf_startup_pair *rows = (const vilf_startup_pair *)(hb + o.rows);
    for (int w = 0; w < W; w++) {
        vilf_startup_result r;
        std::memset(&r, 0, sizeof(r));
        r.l = lwin[w] >= 0 && lwin[w] < SU_NP ? lwin[w] : -1;
        if (r.l >= 0) {
            const vilf_startup_pair &row = rows[(size_t)w * SU_NP + r.l];
            r.inlier_cnt = row.inlier_cnt;
            std::memcpy(r.R, row.R, sizeof(r.R)); std::memcpy(r.T, row.T, sizeof(r.T));
        }
        out[w] = r;
    }
    if (pairs_out) std::memcpy(pairs_out, rows, slots * sizeof(vilf_startup_pair));
    c->last_windows = W;
    return VILF_OK;
}

extern "C" int vilf_startup_get_correspondences(vilf_handle *h, int n_windows, int *feature_out, unsigned char *mask_out, double *points_out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    StartupCtx *c = vilf_stage<StartupCtx>(h, ST_STARTUP);
    if (!c || c->last_windows < 1 || n_windows != c->last_windows) {
        h->err = "vilf_startup_get_correspondences: n_windows is not that of the last vilf_startup_relative_pose"; return VILF_ERR_INVALID_ARGUMENT;
    }
    const SuOut o = su_out(n_windows);
    const size_t cells = (size_t)n_windows * SU_NP * SU_MAXN;
    const char *hb = (const char *)c->io.down.p;
    if (feature_out) std::memcpy(feature_out, hb + o.feat, cells * 4);
    if (mask_out) std::memcpy(mask_out, hb + o.mask, cells);
    if (points_out) std::memcpy(points_out, hb + o.points, cells * 24);
    return VILF_OK;
}

extern "C" int vilf_startup_profile(vilf_handle *h, double ms_out[4], long launches_out[4]) { return vilf_stage_profile(h, ST_STARTUP, &StartupCtx::prof, ms_out, launches_out); }
