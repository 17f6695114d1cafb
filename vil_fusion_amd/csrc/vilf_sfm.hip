// vilf_sfm.hip — the second stage of the visual start-up on the device (≙ GlobalSFM::construct, initial/initial_sfm.cpp:117-217, with triangulatePoint,
//   solveFrameByPnP and triangulateTwoFrames). The arithmetic is stated once, in include/vilfusion.h ("Visual start-up: GlobalSFM frame chain"); the Jacobi is the
//   tracker's (vilf_fmat.hpp). The chain is sequential across the frames of a window and parallel across its features and across windows:
//   su_sfm_chain   a workgroup of 256 per window walks the chain with barriers; state, positions and poses stay in LDS. A thread takes a feature for a
//                  triangulation (its 4 x 4 Jacobi in its own LDS column of its wave's arrays); a PnP gathers its members by rank counting into LDS (they alias
//                  the Jacobi columns, the two never live at once), sums strided over the members, and every thread solves the same 6 x 6 system in registers (vilf_pnp.hpp)
//   su_pnp_batch   a workgroup per problem around the same PnP
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include "vilf_internal.hpp"
#include "vilf_device.hpp"
#include "vilf_fmat.hpp"
#include "vilf_pnp.hpp"

#define SF_MAXN VILF_MAX_FEATURES
#define SF_MAXF VILF_MAX_FRAMES
#define SF_WIN_INTS VILF_SU_WIN_INTS
#define SF_JROWS 26                         // a wave's Jacobi columns: 10 rows of G, 16 of V
#define SF_WORDS 256                        // the membership bytes as words, >= SF_MAXN / 4
static_assert(SF_MAXN % 4 == 0 && SF_MAXN / 4 <= SF_WORDS, "the membership bytes fit their words");

// the device arrays of a chain call (indexed by window) ..
struct SfDev {
    const int *win; const double *pts; const int *l; const double *rel;                                   // the windows as stage one uploads them; [window], [window][12]: R, T
    vilf_startup_structure *res; vilf_startup_frame *rows; unsigned char *state; double *pos;             // the download: [window], [window][SF_MAXF], [window][SF_MAXN] (x 3)
};
// .. and of a batch of PnP problems (indexed by problem)
struct SfPnpDev { const int *prob; const double *guess, *pts3, *pts2; vilf_startup_frame *rows; };        // [problem][4]: n, min_count, first row, 0; [problem][12]; all points

// ---- launch contract -----------------------------------------------------------------------------------------------------
// both kernels: block SF_NT (vilf_pnp.hpp), one workgroup per window / per problem; su_sfm_chain takes SF_LDS_BYTES of dynamic LDS
#define SF_OFF_POS (4 * SF_JROWS * TK_F_LANES)                   // in doubles: the Jacobi columns of the four waves first (the PnP's members alias them)
#define SF_OFF_POSE (SF_OFF_POS + 3 * SF_MAXN)
#define SF_OFF_RED (SF_OFF_POSE + SF_MAXF * 12)
#define SF_OFF_RED2 (SF_OFF_RED + 4 * SF_TERMS)
#define SF_OFF_WORDS (SF_OFF_RED2 + 4)
#define SF_LDS_BYTES ((size_t)SF_OFF_WORDS * 8 + SF_WORDS * 4 + SF_MAXN + 8)
static_assert(SF_LDS_BYTES <= 160 * 1024, "the chain's LDS fits a CU");
static_assert(SF_MAXN * 12 + SF_MAXN * 8 <= 4 * SF_JROWS * TK_F_LANES * 8 && (SF_MAXN * 12) % 8 == 0, "the members fit the Jacobi columns they alias");
__global__ void su_sfm_chain(SfDev d, SfPar p);
__global__ void su_pnp_batch(SfPnpDev d, SfPar p);

struct SfmCtx : VilfStage {
    StageIO io, pnp;                        // the chain's staging, the PnP batch's
    int last_windows = 0;
    StageProf<2> prof;
    bool attr = false;
    void profile_reset() override { prof.reset(); }
};

namespace {

// a frame's row, by one thread; R, t are read only with VILF_SFM_POSE
VD void sf_write_row(vilf_startup_frame *o, const SfRow &row, const double *R, const double *t) {
    const bool pose = (row.flags & VILF_SFM_POSE) != 0;
    o->count = row.m; o->flags = row.flags; o->accepted = row.accepted; o->pad_ = 0; o->cost0 = row.cost0; o->cost1 = row.cost1;
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) { o->R[r * 3 + c] = pose ? R[r * 3 + c] : 0.0; o->Q[r * 3 + c] = pose ? R[c * 3 + r] : 0.0; }
        o->t[r] = pose ? t[r] : 0.0;
        o->T[r] = pose ? -vilf_dot3(R[r], t[0], R[3 + r], t[1], R[6 + r], t[2]) : 0.0;
    }
}
}  // namespace

// ---- su_sfm_chain: a workgroup per window --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SF_NT) void su_sfm_chain(SfDev d, SfPar p) {
    extern __shared__ double sf_lds[];
    double (*s_J)[TK_F_LANES] = (double (*)[TK_F_LANES])sf_lds;
    float *s_X = (float *)sf_lds;                                          // the PnP's members, over the Jacobi columns
    float2 *s_u = (float2 *)(s_X + 3 * SF_MAXN);
    double *s_pos = sf_lds + SF_OFF_POS, *s_P = sf_lds + SF_OFF_POSE, *s_red = sf_lds + SF_OFF_RED, *s_red2 = sf_lds + SF_OFF_RED2;
    unsigned *s_word = (unsigned *)(sf_lds + SF_OFF_WORDS);
    unsigned char *s_in = (unsigned char *)s_word, *s_state = (unsigned char *)(s_word + SF_WORDS);
    const int tid = threadIdx.x, lane = tid & 63, w = blockIdx.x;
    const int *win = d.win + (size_t)w * SF_WIN_INTS, *start = win + 4, *first = win + 4 + SF_MAXN;
    const int nf = min(max(win[0], 2), SF_MAXF), n = min(max(win[1], 0), SF_MAXN), newest = nf - 1;      // the host has checked all three
    const double *pts = d.pts + (size_t)win[2] * 2;
    const int l = d.l[w];
    vilf_startup_frame *rows = d.rows + (size_t)w * SF_MAXF;
    unsigned char *state_out = d.state + (size_t)w * SF_MAXN;
    double *pos_out = d.pos + (size_t)w * SF_MAXN * 3;
    double (*M)[TK_F_LANES] = s_J + (tid >> 6) * SF_JROWS, (*V)[TK_F_LANES] = M + 10;
    // everything starts at 0: the rows (as doubles), the state, the positions, the poses
    for (int e = tid; e < (int)(SF_MAXF * sizeof(vilf_startup_frame) / 8); e += SF_NT) ((double *)rows)[e] = 0.0;
    for (int f = tid; f < SF_MAXN; f += SF_NT) { s_state[f] = 0; s_pos[3 * f] = 0.0; s_pos[3 * f + 1] = 0.0; s_pos[3 * f + 2] = 0.0; }
    for (int e = tid; e < SF_MAXF * 12; e += SF_NT) s_P[e] = 0.0;
    __syncthreads();
    int fail = -1;
    const bool run = l >= 0 && l < newest;
    if (run) {
        if (tid == 0) {                                                    // the two given poses
            const double *R = d.rel + (size_t)w * 12, *T = R + 9;
            double Rl[9], tl[3], Rn[9], tn[3];
#pragma unroll
            for (int r = 0; r < 3; r++) {
#pragma unroll
                for (int c = 0; c < 3; c++) { Rl[r * 3 + c] = r == c ? 1.0 : 0.0; Rn[r * 3 + c] = R[c * 3 + r]; }
                tl[r] = 0.0;
                tn[r] = -vilf_dot3(R[r], T[0], R[3 + r], T[1], R[6 + r], T[2]);
            }
#pragma unroll
            for (int r = 0; r < 3; r++) {
#pragma unroll
                for (int c = 0; c < 3; c++) { s_P[l * 12 + r * 4 + c] = Rl[r * 3 + c]; s_P[newest * 12 + r * 4 + c] = Rn[r * 3 + c]; }
                s_P[l * 12 + r * 4 + 3] = tl[r]; s_P[newest * 12 + r * 4 + 3] = tn[r];
            }
            SfRow row;
            row.m = 0; row.flags = VILF_SFM_FIXED | VILF_SFM_POSE; row.accepted = 0; row.cost0 = 0.0; row.cost1 = 0.0;
            sf_write_row(rows + l, row, Rl, tl);
            sf_write_row(rows + newest, row, Rn, tn);
        }
        __syncthreads();
        // the chain as one list of steps, each an optional PnP and a triangulation: F forward (frame l + k against newest), S of (l, l + 1 + k), B backward
        // (frame l - 1 - k against l), and the rest
        const int F = newest - l, S = newest - l - 1, B = l, steps = F + S + B + 1;
        for (int step = 0; step < steps && fail < 0; step++) {
            int pf = -1, guess = -1, fa = -1, fb = -1;                     // PnP of frame pf from the pose of guess; triangulate (fa, fb), fa = -1: the rest
            if (step < F) { const int i = l + step; if (step > 0) { pf = i; guess = i - 1; } fa = i; fb = newest; }
            else if (step < F + S) { fa = l; fb = l + 1 + (step - F); }
            else if (step < F + S + B) { const int i = l - 1 - (step - F - S); pf = i; guess = i + 1; fa = i; fb = l; }
            if (pf >= 0) {
                // the members: triangulated and seen in pf, in feature order
                if (tid < SF_WORDS) s_word[tid] = 0u;
                __syncthreads();
                for (int f = tid; f < n; f += SF_NT) {
                    const int st = start[f], nobs = first[f + 1] - first[f];
                    s_in[f] = (s_state[f] && st <= pf && pf < st + nobs) ? 1 : 0;
                }
                __syncthreads();
                int m = 0;
                for (int k = 0; k < SF_MAXN / 4; k++) m += __popc(s_word[k]);
                for (int f = tid; f < n; f += SF_NT) {
                    if (!s_in[f]) continue;
                    int rank = __popc(s_word[f >> 2] & ((1u << ((f & 3) * 8)) - 1u));
                    for (int k = 0; k < (f >> 2); k++) rank += __popc(s_word[k]);      // rank < m <= n <= SF_MAXN, the rows of s_X, s_u
                    const double *pt = pts + (size_t)(first[f] + pf - start[f]) * 2;          // 0 <= pf - start < n_obs
                    s_X[3 * rank] = (float)s_pos[3 * f]; s_X[3 * rank + 1] = (float)s_pos[3 * f + 1]; s_X[3 * rank + 2] = (float)s_pos[3 * f + 2];
                    s_u[rank] = make_float2((float)pt[0], (float)pt[1]);
                }
                __syncthreads();
                double R[9], t[3];
#pragma unroll
                for (int r = 0; r < 3; r++) {
#pragma unroll
                    for (int c = 0; c < 3; c++) R[r * 3 + c] = s_P[guess * 12 + r * 4 + c];
                    t[r] = s_P[guess * 12 + r * 4 + 3];
                }
                SfRow row;
                const bool ok = sf_pnp(s_X, s_u, m, p.min_count, p, R, t, s_red, s_red2, tid, row);
                if (tid == 0) {
                    sf_write_row(rows + pf, row, R, t);
                    if (ok) {
#pragma unroll
                        for (int r = 0; r < 3; r++) {
#pragma unroll
                            for (int c = 0; c < 3; c++) s_P[pf * 12 + r * 4 + c] = R[r * 3 + c];
                            s_P[pf * 12 + r * 4 + 3] = t[r];
                        }
                    }
                }
                if (!ok) fail = pf;
                __syncthreads();                                           // the pose is in LDS, the members are read: the Jacobi columns are free again
            }
            if (fail < 0) {
                for (int f = tid; f < n; f += SF_NT) {
                    if (s_state[f]) continue;
                    const int st = start[f], nobs = first[f + 1] - first[f];
                    int ka = fa, kb = fb;
                    if (fa < 0) { if (nobs < 2) continue; ka = st; kb = st + nobs - 1; }
                    else if (!(st <= fa && fa < st + nobs && st <= fb && fb < st + nobs)) continue;
                    const double *pa = pts + (size_t)(first[f] + ka - st) * 2, *pb = pts + (size_t)(first[f] + kb - st) * 2;
                    const double *P0 = s_P + ka * 12, *P1 = s_P + kb * 12;                   // 0 <= ka, kb < nf <= SF_MAXF
                    const double x0 = pa[0], y0 = pa[1], x1 = pb[0], y1 = pb[1];
                    double A[16];
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        A[c] = __dsub_rn(__dmul_rn(x0, P0[8 + c]), P0[c]); A[4 + c] = __dsub_rn(__dmul_rn(y0, P0[8 + c]), P0[4 + c]);
                        A[8 + c] = __dsub_rn(__dmul_rn(x1, P1[8 + c]), P1[c]); A[12 + c] = __dsub_rn(__dmul_rn(y1, P1[8 + c]), P1[4 + c]);
                    }
#pragma unroll
                    for (int a = 0; a < 4; a++)
#pragma unroll
                        for (int b = a; b < 4; b++) {
                            double acc = 0.0;
#pragma unroll
                            for (int r = 0; r < 4; r++) acc = __dadd_rn(acc, __dmul_rn(A[r * 4 + a], A[r * 4 + b]));
                            M[tk_iu(4, a, b)][lane] = acc;
                        }
                    tk_jacobi<4>(M, V, lane);
                    const int at = tk_smallest<4>(M, lane);
                    const double v3 = V[12 + at][lane];
                    const double X0 = __ddiv_rn(V[at][lane], v3), X1 = __ddiv_rn(V[4 + at][lane], v3), X2 = __ddiv_rn(V[8 + at][lane], v3);
                    if (isfinite(X0) && isfinite(X1) && isfinite(X2)) { s_state[f] = 1; s_pos[3 * f] = X0; s_pos[3 * f + 1] = X1; s_pos[3 * f + 2] = X2; }
                }
                __syncthreads();
            }
        }
    }
    // the structure and the window's result
    int cnt = 0;
    for (int f = tid; f < SF_MAXN; f += SF_NT) {
        const unsigned char s = s_state[f];
        cnt += s;
        state_out[f] = s; pos_out[3 * f] = s_pos[3 * f]; pos_out[3 * f + 1] = s_pos[3 * f + 1]; pos_out[3 * f + 2] = s_pos[3 * f + 2];
    }
    if (tid < SF_WORDS) s_word[tid] = 0u;
    __syncthreads();
    if (cnt) atomicAdd((int *)s_word, cnt);
    __syncthreads();
    if (tid == 0) {
        vilf_startup_structure r;
        r.ok = run && fail < 0 ? 1 : 0; r.fail_frame = fail; r.n_triangulated = (int)s_word[0]; r.l = l;
        d.res[w] = r;
    }
}

// ---- su_pnp_batch: a workgroup per problem -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SF_NT) void su_pnp_batch(SfPnpDev d, SfPar p) {
    __shared__ float s_X[3 * SF_MAXN];
    __shared__ float2 s_u[SF_MAXN];
    __shared__ double s_red[4 * SF_TERMS], s_red2[4];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int *pr = d.prob + (size_t)b * 4;
    const int n = min(max(pr[0], 0), SF_MAXN), min_count = pr[1];         // the host has checked n
    const double *p3 = d.pts3 + (size_t)pr[2] * 3, *p2 = d.pts2 + (size_t)pr[2] * 2;
    for (int j = tid; j < n; j += SF_NT) {
        s_X[3 * j] = (float)p3[3 * j]; s_X[3 * j + 1] = (float)p3[3 * j + 1]; s_X[3 * j + 2] = (float)p3[3 * j + 2];
        s_u[j] = make_float2((float)p2[2 * j], (float)p2[2 * j + 1]);
    }
    __syncthreads();
    double R[9], t[3];
#pragma unroll
    for (int e = 0; e < 9; e++) R[e] = d.guess[(size_t)b * 12 + e];
#pragma unroll
    for (int r = 0; r < 3; r++) t[r] = d.guess[(size_t)b * 12 + 9 + r];
    SfRow row;
    sf_pnp(s_X, s_u, n, min_count, p, R, t, s_red, s_red2, tid, row);
    if (tid == 0) sf_write_row(d.rows + b, row, R, t);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
namespace {
// the download of a chain call: the results, the rows, the state, the positions
struct SfOut { size_t res, rows, state, pos, bytes; };
SfOut sf_out(int W) {
    Layout l;
    SfOut o;
    o.res = l.take((size_t)W * sizeof(vilf_startup_structure)); o.rows = l.take((size_t)W * SF_MAXF * sizeof(vilf_startup_frame)); o.state = l.take((size_t)W * SF_MAXN);
    o.pos = l.take((size_t)W * SF_MAXN * 24); o.bytes = l.at;
    return o;
}
bool sf_params_ok(const vilf_startup_sfm_params *p) {
    return p->pnp_iterations >= 1 && p->pnp_iterations <= 64 && p->min_pnp_count >= 0 && p->warn_pnp_count >= 0 && std::isfinite(p->lambda0) && p->lambda0 > 0;
}
SfPar sf_par(const vilf_startup_sfm_params *p) {
    SfPar sp;
    sp.min_count = p->min_pnp_count; sp.warn_count = p->warn_pnp_count; sp.iters = p->pnp_iterations; sp.lambda0 = p->lambda0;
    return sp;
}
const char *SF_PARAMS_TEXT = ": 1 <= pnp_iterations <= 64, counts >= 0, a positive finite lambda0";
}  // namespace

extern "C" void vilf_startup_default_sfm_params(vilf_startup_sfm_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->min_pnp_count = 10; p->warn_pnp_count = 15; p->pnp_iterations = 10; p->lambda0 = 1e-3;
}

// validation, upload and launch of the chain into the buffers given; nothing is waited for and nothing comes back (vilf_startup_sfm, vilf_startup_construct)
int vilf_sfm_enqueue(vilf_handle *h, const char *who, const vilf_startup_sfm_params *p, int n_windows, const vilf_startup_window *windows, const vilf_startup_result *rel,
                     StageIO *io, size_t extra_out, VilfSfmQueued *q) {
    const std::string name(who);
    if (n_windows < 1 || n_windows > VILF_STARTUP_MAX_WINDOWS) { h->err = name + ": 1 <= n_windows <= VILF_STARTUP_MAX_WINDOWS"; return VILF_ERR_INVALID_ARGUMENT; }
    if (!sf_params_ok(p)) { h->err = name + SF_PARAMS_TEXT; return VILF_ERR_INVALID_ARGUMENT; }
    size_t total = 0;
    { const int rcw = vilf_startup_check_windows(h, who, n_windows, windows, &total); if (rcw != VILF_OK) return rcw; }
    for (int w = 0; w < n_windows; w++) {
        if (rel[w].l < -1 || rel[w].l > windows[w].n_frames - 2) { h->err = name + ": -1 <= l <= n_frames - 2"; return VILF_ERR_INVALID_ARGUMENT; }
        if (rel[w].l < 0) continue;
        bool fin = true;
        for (int e = 0; e < 9; e++) fin = fin && std::isfinite(rel[w].R[e]);
        for (int e = 0; e < 3; e++) fin = fin && std::isfinite(rel[w].T[e]);
        if (!fin) { h->err = name + ": a relative_R or relative_T that is not finite"; return VILF_ERR_INVALID_ARGUMENT; }
    }
    HIPCHECK(h, hipSetDevice(h->device));
    SfmCtx *c = vilf_stage_make<SfmCtx>(h, ST_SFM);
    const int W = n_windows;
    // upload: the windows' integers, l of every window (padded to 8 bytes), the relative poses, then all points
    Layout li;
    li.take((size_t)W * SF_WIN_INTS * 4, 8);
    const size_t o_l = li.take((size_t)((W + 1) & ~1) * 4, 8), o_rel = li.take((size_t)W * 96, 8), o_pts = li.take(std::max<size_t>(total, 1) * 16, 8), in_bytes = li.at;
    const SfOut o = sf_out(W);
    if (!io->ensure(in_bytes, o.bytes + extra_out)) {
        h->err = name + ": out of memory"; return VILF_ERR_DEVICE;
    }
    {
        char *ub = (char *)io->up.p;
        vilf_startup_pack_windows(W, windows, (int *)ub, (double *)(ub + o_pts));
        int *lw = (int *)(ub + o_l);
        double *rl = (double *)(ub + o_rel);
        for (int w = 0; w < W; w++) {
            lw[w] = rel[w].l;
            for (int e = 0; e < 9; e++) rl[(size_t)w * 12 + e] = rel[w].l >= 0 ? rel[w].R[e] : 0.0;
            for (int e = 0; e < 3; e++) rl[(size_t)w * 12 + 9 + e] = rel[w].l >= 0 ? rel[w].T[e] : 0.0;
        }
        if (W & 1) lw[W] = 0;
    }
    if (!c->attr) {
        HIPCHECK(h, hipFuncSetAttribute(reinterpret_cast<const void *>(su_sfm_chain), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SF_LDS_BYTES));
        c->attr = true;
    }
    HIPCHECK(h, io->upload(h, in_bytes));
    SfDev d;
    char *ib = io->in.as<char>(), *ob = io->out.as<char>();
    d.win = (const int *)ib; d.l = (const int *)(ib + o_l); d.rel = (const double *)(ib + o_rel); d.pts = (const double *)(ib + o_pts);
    d.res = (vilf_startup_structure *)(ob + o.res); d.rows = (vilf_startup_frame *)(ob + o.rows); d.state = (unsigned char *)(ob + o.state); d.pos = (double *)(ob + o.pos);
    ProfMarks prof(h, c->prof);
    hipLaunchKernelGGL(su_sfm_chain, dim3(W), dim3(SF_NT), SF_LDS_BYTES, h->stream, d, sf_par(p));
    prof.mark(0);
    HIPCHECK(h, hipGetLastError());
    q->win = d.win; q->pts = d.pts; q->l = d.l; q->res = d.res; q->rows = d.rows; q->state = d.state; q->pos = d.pos;
    q->o_res = o.res; q->o_rows = o.rows; q->o_state = o.state; q->o_pos = o.pos; q->out_bytes = o.bytes;
    return VILF_OK;
}

extern "C" int vilf_startup_sfm(vilf_handle *h, const vilf_startup_sfm_params *p, int n_windows, const vilf_startup_window *windows, const vilf_startup_result *rel,
                                vilf_startup_structure *out, vilf_startup_frame *frames_out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    if (!p || !windows || !rel || !out) { h->err = "vilf_startup_sfm: null pointer"; return VILF_ERR_INVALID_ARGUMENT; }
    SfmCtx *c = vilf_stage_make<SfmCtx>(h, ST_SFM);
    const int kept = c->last_windows;
    c->last_windows = 0;
    VilfSfmQueued q;
    { const int rcq = vilf_sfm_enqueue(h, "vilf_startup_sfm", p, n_windows, windows, rel, &c->io, 0, &q); if (rcq != VILF_OK) { if (rcq == VILF_ERR_INVALID_ARGUMENT) c->last_windows = kept; return rcq; } }
    const int W = n_windows;
    HIPCHECK(h, c->io.download(h, q.out_bytes));
    const char *hb = (const char *)c->io.down.p;
    std::memcpy(out, hb + q.o_res, (size_t)W * sizeof(vilf_startup_structure));
    if (frames_out) std::memcpy(frames_out, hb + q.o_rows, (size_t)W * SF_MAXF * sizeof(vilf_startup_frame));
    c->last_windows = W;
    return VILF_OK;
}

extern "C" int vilf_startup_get_structure(vilf_handle *h, int n_windows, unsigned char *state_out, double *positions_out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    SfmCtx *c = vilf_stage<SfmCtx>(h, ST_SFM);
    if (!c || c->last_windows < 1 || n_windows != c->last_windows) {
        h->err = "vilf_startup_get_structure: n_windows is not that of the last vilf_startup_sfm"; return VILF_ERR_INVALID_ARGUMENT;
    }
    const SfOut o = sf_out(n_windows);
    const char *hb = (const char *)c->io.down.p;
    if (state_out) std::memcpy(state_out, hb + o.state, (size_t)n_windows * SF_MAXN);
    if (positions_out) std::memcpy(positions_out, hb + o.pos, (size_t)n_windows * SF_MAXN * 24);
    return VILF_OK;
}

extern "C" int vilf_startup_pnp(vilf_handle *h, const vilf_startup_sfm_params *p, int n_problems, const vilf_startup_pnp_problem *problems, vilf_startup_frame *out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    if (!p || !problems || !out) { h->err = "vilf_startup_pnp: null pointer"; return VILF_ERR_INVALID_ARGUMENT; }
    if (n_problems < 1 || n_problems > VILF_STARTUP_MAX_PROBLEMS) { h->err = "vilf_startup_pnp: 1 <= n_problems <= VILF_STARTUP_MAX_PROBLEMS"; return VILF_ERR_INVALID_ARGUMENT; }
    if (!sf_params_ok(p)) { h->err = std::string("vilf_startup_pnp") + SF_PARAMS_TEXT; return VILF_ERR_INVALID_ARGUMENT; }
    size_t total = 0;
    for (int b = 0; b < n_problems; b++) {
        const vilf_startup_pnp_problem &q = problems[b];
        if (q.n < 0 || q.n > VILF_MAX_FEATURES || q.min_count < 0) { h->err = "vilf_startup_pnp: 0 <= n <= VILF_MAX_FEATURES, min_count >= 0"; return VILF_ERR_INVALID_ARGUMENT; }
        if (q.n > 0 && (!q.pts3 || !q.pts2)) { h->err = "vilf_startup_pnp: null pointer in a problem"; return VILF_ERR_INVALID_ARGUMENT; }
        bool fin = true;
        for (int e = 0; e < q.n * 3; e++) fin = fin && std::isfinite(q.pts3[e]);
        for (int e = 0; e < q.n * 2; e++) fin = fin && std::isfinite(q.pts2[e]);
        for (int e = 0; e < 9; e++) fin = fin && std::isfinite(q.R[e]);
        for (int e = 0; e < 3; e++) fin = fin && std::isfinite(q.t[e]);
        if (!fin) { h->err = "vilf_startup_pnp: a coordinate or an entry of the guess that is not finite"; return VILF_ERR_INVALID_ARGUMENT; }
        total += (size_t)q.n;
    }
    HIPCHECK(h, hipSetDevice(h->device));
    SfmCtx *c = vilf_stage_make<SfmCtx>(h, ST_SFM);
    const int B = n_problems;
    const size_t rows = std::max<size_t>(total, 1);
    Layout li;
    li.take((size_t)B * 16, 8);
    const size_t o_guess = li.take((size_t)B * 96, 8), o_p3 = li.take(rows * 24, 8), o_p2 = li.take(rows * 16, 8), in_bytes = li.at, out_bytes = (size_t)B * sizeof(vilf_startup_frame);
    if (!c->pnp.ensure(in_bytes, out_bytes)) { h->err = "vilf_startup_pnp: out of memory"; return VILF_ERR_DEVICE; }
    {
        char *ub = (char *)c->pnp.up.p;
        int *pi = (int *)ub;
        double *g = (double *)(ub + o_guess), *p3 = (double *)(ub + o_p3), *p2 = (double *)(ub + o_p2);
        size_t at = 0;
        for (int b = 0; b < B; b++) {
            const vilf_startup_pnp_problem &q = problems[b];
            pi[4 * b] = q.n; pi[4 * b + 1] = q.min_count; pi[4 * b + 2] = (int)at; pi[4 * b + 3] = 0;
            std::memcpy(g + (size_t)b * 12, q.R, 72); std::memcpy(g + (size_t)b * 12 + 9, q.t, 24);
            if (q.n > 0) { std::memcpy(p3 + at * 3, q.pts3, (size_t)q.n * 24); std::memcpy(p2 + at * 2, q.pts2, (size_t)q.n * 16); }
            at += (size_t)q.n;
        }
    }
    HIPCHECK(h, c->pnp.upload(h, in_bytes));
    SfPnpDev d;
    char *ib = c->pnp.in.as<char>();
    d.prob = (const int *)ib; d.guess = (const double *)(ib + o_guess); d.pts3 = (const double *)(ib + o_p3); d.pts2 = (const double *)(ib + o_p2);
    d.rows = c->pnp.out.as<vilf_startup_frame>();
    ProfMarks prof(h, c->prof);
    hipLaunchKernelGGL(su_pnp_batch, dim3(B), dim3(SF_NT), 0, h->stream, d, sf_par(p));
    prof.mark(1);
    HIPCHECK(h, hipGetLastError());
    HIPCHECK(h, c->pnp.download(h, out_bytes));
    std::memcpy(out, c->pnp.down.p, out_bytes);
    return VILF_OK;
}

extern "C" int vilf_startup_sfm_profile(vilf_handle *h, double ms_out[2], long launches_out[2]) { return vilf_stage_profile(h, ST_SFM, &SfmCtx::prof, ms_out, launches_out); }
