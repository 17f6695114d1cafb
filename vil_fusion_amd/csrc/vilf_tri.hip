// vilf_tri.hip — FeatureManager::triangulate and getDepthVector on the device (≙ feature_manager.cpp:218-274, :194-216), batched over windows. The arithmetic is
//   stated once, in include/vilfusion.h ("Feature manager: triangulate"); every sum order there is sequential per feature, so a lane owns a candidate.
// The host applies the used and the candidate rule while it packs (candidates are about a tenth of the features) and hands the device ONE dense list of the
// candidates of all windows, so that the waves are full; it writes the outputs of the features that are no candidates itself. One upload, two launches on the
// handle's stream, one wait, one download:
//   tri_cameras    a thread per (window that has candidates, frame): tc = Ps + Rs tic, Rc = Rs ric. The same numbers for every feature of the window; every value has
//                  one stated formula, so computing them once changes no bit
//   tri_solve      a lane per candidate: the design matrix (at most 22 x 4) and V in the lane's own LDS column, 60 sweeps of the one-sided Jacobi, the winner, the
//                  depth, the reset. Nothing indexed at run time lives in registers
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <string>
#include "vilf_internal.hpp"
#include "vilf_device.hpp"

#define TRI_NF VILF_MAX_FRAMES
#define TRI_ROWS (2 * VILF_MAX_FRAMES)      // rows of a design matrix
#define TRI_POSE_DBL (12 * TRI_NF + 12)     // a window's upload: Ps [11][3], Rs [11][9], tic, ric (frames the window does not have are 0)
#define TRI_CAM_DBL 12                      // a camera: tc [3], Rc [9]
#define TRI_SWEEPS 60

// ---- launch contract -----------------------------------------------------------------------------------------------------
#define TRI_LANES 64                        // tri_solve: block 64 (one wave), grid ceil(n_cand / 64); 104 doubles of LDS per lane = 53 248 bytes per workgroup.
                                            // tri_cameras: block 64, grid ceil(n_slots * TRI_NF / 64). Neither has a barrier: a thread past the end leaves at once
struct TriDev {
    const double *pose;                     // [n_slots][TRI_POSE_DBL]
    const int4 *cand;                       // [n_cand]: first camera (slot * TRI_NF + start_frame), n_obs, first row of its points, 0
    const double *pts;                      // the candidates' points [rows][3]
    double *cam;                            // [n_slots][TRI_NF][TRI_CAM_DBL]
    double *depth; unsigned *meta;          // [n_cand]: the depth; flags | sweeps << 8
    int n_slots, n_cand;
    double init_depth;
};
__global__ void tri_cameras(TriDev d);
__global__ void tri_solve(TriDev d);

struct TriCtx : VilfStage {
    StageIO io;
    DBuf cam;
    StageProf<1> prof;
    void profile_reset() override { prof.reset(); }
};

namespace {
// the sum from 0.0 of three products
VD double tri_sum3(double a0, double b0, double a1, double b1, double a2, double b2) {
    return __dadd_rn(__dadd_rn(__dadd_rn(0.0, __dmul_rn(a0, b0)), __dmul_rn(a1, b1)), __dmul_rn(a2, b2));
}
}  // namespace

// ---- tri_cameras: a thread per (slot, frame) ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void tri_cameras(TriDev d) {
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= d.n_slots * TRI_NF) return;
    const int slot = g / TRI_NF, k = g - slot * TRI_NF;
    const double *w = d.pose + (size_t)slot * TRI_POSE_DBL, *P = w + 3 * k, *R = w + 3 * TRI_NF + 9 * k, *tic = w + 12 * TRI_NF, *ric = tic + 3;
    double *c = d.cam + (size_t)g * TRI_CAM_DBL;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        c[r] = __dadd_rn(P[r], vilf_dot3(R[3 * r], tic[0], R[3 * r + 1], tic[1], R[3 * r + 2], tic[2]));
#pragma unroll
        for (int q = 0; q < 3; q++) c[3 + 3 * r + q] = tri_sum3(R[3 * r], ric[q], R[3 * r + 1], ric[3 + q], R[3 * r + 2], ric[6 + q]);
    }
}

// ---- tri_solve: a lane per candidate -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TRI_LANES) void tri_solve(TriDev d) {
    __shared__ double s_A[4 * TRI_ROWS][TRI_LANES], s_V[16][TRI_LANES];          // 53 248 bytes: a column per lane
    const int lane = threadIdx.x, g = blockIdx.x * TRI_LANES + lane;
    if (g >= d.n_cand) return;
    const int4 cd = d.cand[g];
    const int nobs = min(max(cd.y, 0), TRI_NF), rows = 2 * nobs;                 // the host has checked: 2 <= n_obs, start_frame + n_obs <= n_frames <= TRI_NF
    const double *cam0 = d.cam + (size_t)cd.x * TRI_CAM_DBL;
    const double *pt = d.pts + (size_t)cd.z * 3;
    double t0[3], R0[9];
#pragma unroll
    for (int e = 0; e < 3; e++) t0[e] = cam0[e];
#pragma unroll
    for (int e = 0; e < 9; e++) R0[e] = cam0[3 + e];
    for (int o = 0; o < nobs; o++) {
        const double *cj = cam0 + (size_t)o * TRI_CAM_DBL;
        double dd[3], t[3], R[9];
#pragma unroll
        for (int e = 0; e < 3; e++) dd[e] = __dsub_rn(cj[e], t0[e]);
#pragma unroll
        for (int r = 0; r < 3; r++) {
            t[r] = vilf_dot3(R0[r], dd[0], R0[3 + r], dd[1], R0[6 + r], dd[2]);
#pragma unroll
            for (int c = 0; c < 3; c++) R[3 * r + c] = tri_sum3(R0[r], cj[3 + c], R0[3 + r], cj[6 + c], R0[6 + r], cj[9 + c]);
        }
        double P[3][4];
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) P[r][c] = R[3 * c + r];
            P[r][3] = -vilf_dot3(R[r], t[0], R[3 + r], t[1], R[6 + r], t[2]);
        }
        const double x = pt[3 * o], y = pt[3 * o + 1], z = pt[3 * o + 2];
        const double n = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y)), __dmul_rn(z, z)));
        const double f0 = __ddiv_rn(x, n), f1 = __ddiv_rn(y, n), f2 = __ddiv_rn(z, n);
#pragma unroll
        for (int c = 0; c < 4; c++) {
            s_A[8 * o + c][lane] = __dsub_rn(__dmul_rn(f0, P[2][c]), __dmul_rn(f2, P[0][c]));
            s_A[8 * o + 4 + c][lane] = __dsub_rn(__dmul_rn(f1, P[2][c]), __dmul_rn(f2, P[1][c]));
        }
    }
#pragma unroll
    for (int e = 0; e < 16; e++) s_V[e][lane] = (e % 5 == 0) ? 1.0 : 0.0;
    int sweeps = 0;
    for (int sweep = 0; sweep < TRI_SWEEPS; sweep++) {
        bool rotated = false;
        sweeps++;
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int q = p + 1; q < 4; q++) {
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
                for (int i = 0; i < rows; i++) {
                    const double ap = s_A[4 * i + p][lane], aq = s_A[4 * i + q][lane];
                    alpha = __dadd_rn(alpha, __dmul_rn(ap, ap)); beta = __dadd_rn(beta, __dmul_rn(aq, aq)); gamma = __dadd_rn(gamma, __dmul_rn(ap, aq));
                }
                if (fabs(gamma) <= __dmul_rn(1e-17, __dsqrt_rn(__dmul_rn(alpha, beta))) || gamma == 0.0) continue;
                rotated = true;
                const double zeta = __ddiv_rn(__dsub_rn(beta, alpha), __dmul_rn(2.0, gamma));
                const double tt = __ddiv_rn(zeta >= 0.0 ? 1.0 : -1.0, __dadd_rn(fabs(zeta), __dsqrt_rn(__dadd_rn(1.0, __dmul_rn(zeta, zeta)))));
                const double c = __ddiv_rn(1.0, __dsqrt_rn(__dadd_rn(1.0, __dmul_rn(tt, tt)))), s = __dmul_rn(c, tt);
                for (int i = 0; i < rows; i++) {
                    const double ap = s_A[4 * i + p][lane], aq = s_A[4 * i + q][lane];
                    s_A[4 * i + p][lane] = __dsub_rn(__dmul_rn(c, ap), __dmul_rn(s, aq));
                    s_A[4 * i + q][lane] = __dadd_rn(__dmul_rn(s, ap), __dmul_rn(c, aq));
                }
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const double vp = s_V[4 * i + p][lane], vq = s_V[4 * i + q][lane];
                    s_V[4 * i + p][lane] = __dsub_rn(__dmul_rn(c, vp), __dmul_rn(s, vq));
                    s_V[4 * i + q][lane] = __dadd_rn(__dmul_rn(s, vp), __dmul_rn(c, vq));
                }
            }
        if (!rotated) break;
    }
    int best = 0;
    double bound = INFINITY;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        double nn = 0.0;
        for (int i = 0; i < rows; i++) { const double a = s_A[4 * i + c][lane]; nn = __dadd_rn(nn, __dmul_rn(a, a)); }
        if (nn < bound) { bound = nn; best = c; }
    }
    double depth = __ddiv_rn(s_V[8 + best][lane], s_V[12 + best][lane]);
    unsigned flags = VILF_TRI_USED | VILF_TRI_DONE;
    if (depth < 0.1) { depth = d.init_depth; flags |= VILF_TRI_RESET; }
    if (!isfinite(depth)) flags |= VILF_TRI_NONFINITE;
    d.depth[g] = depth;
    d.meta[g] = flags | ((unsigned)sweeps << 8);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
namespace {
bool tri_used(long long nobs, int start, int window_size) { return nobs >= 2 && start < window_size - 2; }
bool tri_all_finite(const double *p, int n) { for (int i = 0; i < n; i++) if (!std::isfinite(p[i])) return false; return true; }
}  // namespace

extern "C" int vilf_features_triangulate(vilf_handle *h, int n_windows, const vilf_tri_window *windows, vilf_tri_result *out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    if (!windows || !out) { h->err = "vilf_features_triangulate: null pointer"; return VILF_ERR_INVALID_ARGUMENT; }
    if (n_windows < 1 || n_windows > VILF_TRI_MAX_WINDOWS) { h->err = "vilf_features_triangulate: 1 <= n_windows <= VILF_TRI_MAX_WINDOWS"; return VILF_ERR_INVALID_ARGUMENT; }
    const int ws = h->opts.window_size;
    const double init_depth = h->opts.init_depth;
    // the checks, and the counts the packing needs: windows with candidates (slots), candidates, their observations
    size_t n_slots = 0, n_cand = 0, n_rows = 0;
    for (int w = 0; w < n_windows; w++) {
        const vilf_tri_window &W = windows[w];
        if (W.n_frames < 2 || W.n_frames > VILF_MAX_FRAMES || W.n_features < 0 || W.n_features > VILF_MAX_FEATURES) {
            h->err = "vilf_features_triangulate: 2 <= n_frames <= VILF_MAX_FRAMES, 0 <= n_features <= VILF_MAX_FEATURES"; return VILF_ERR_INVALID_ARGUMENT;
        }
        if (!W.Ps || !W.Rs || !W.first_obs || (W.n_features > 0 && (!W.start_frame || !W.depth_in || !W.depth_out))) {
            h->err = "vilf_features_triangulate: null pointer in a window"; return VILF_ERR_INVALID_ARGUMENT;
        }
        if (W.first_obs[0] != 0) { h->err = "vilf_features_triangulate: first_obs[0] != 0"; return VILF_ERR_INVALID_ARGUMENT; }
        size_t cand_here = 0;
        for (int f = 0; f < W.n_features; f++) {
            const long long nobs = (long long)W.first_obs[f + 1] - W.first_obs[f];
            if (nobs < 0) { h->err = "vilf_features_triangulate: first_obs decreases"; return VILF_ERR_INVALID_ARGUMENT; }
            if (!tri_used(nobs, W.start_frame[f], ws)) continue;
            if (W.start_frame[f] < 0 || (long long)W.start_frame[f] + nobs > W.n_frames) {
                h->err = "vilf_features_triangulate: a used feature with start_frame < 0 or start_frame + n_obs > n_frames"; return VILF_ERR_INVALID_ARGUMENT;
            }
            if (!(W.depth_in[f] > 0)) { cand_here++; n_rows += (size_t)nobs; }
        }
        if (W.first_obs[W.n_features] > 0 && !W.points) { h->err = "vilf_features_triangulate: null pointer in a window"; return VILF_ERR_INVALID_ARGUMENT; }
        if (!tri_all_finite(W.Ps, 3 * W.n_frames) || !tri_all_finite(W.Rs, 9 * W.n_frames) || !tri_all_finite(W.tic, 3) || !tri_all_finite(W.ric, 9)) {
            h->err = "vilf_features_triangulate: an entry of Ps, Rs, tic or ric that is not finite"; return VILF_ERR_INVALID_ARGUMENT;
        }
        if (cand_here) { n_slots++; n_cand += cand_here; }
    }
    HIPCHECK(h, hipSetDevice(h->device));
    TriCtx *c = vilf_stage_make<TriCtx>(h, ST_TRI);
    // upload: the poses of the windows that have candidates, the candidate list, the candidates' points. Download: the depths, then flags | sweeps << 8
    Layout li, lo;
    const size_t o_pose = li.take(std::max<size_t>(n_slots, 1) * TRI_POSE_DBL * 8), o_cand = li.take(std::max<size_t>(n_cand, 1) * sizeof(int4)),
                 o_pts = li.take(std::max<size_t>(n_rows, 1) * 24), in_bytes = li.at;
    const size_t o_depth = lo.take(std::max<size_t>(n_cand, 1) * 8), o_meta = lo.take(std::max<size_t>(n_cand, 1) * 4), out_bytes = lo.at;
    const size_t cam_bytes = std::max<size_t>(n_slots, 1) * TRI_NF * TRI_CAM_DBL * 8;
    if (!c->io.ensure(in_bytes, out_bytes) || !c->cam.ensure(cam_bytes)) {
        h->err = "vilf_features_triangulate: out of memory"; return VILF_ERR_DEVICE;
    }
    {
        char *ub = (char *)c->io.up.p;
        double *pose = (double *)(ub + o_pose), *pts = (double *)(ub + o_pts);
        int4 *cand = (int4 *)(ub + o_cand);
        size_t slot = 0, at = 0, row = 0;
        for (int w = 0; w < n_windows; w++) {
            const vilf_tri_window &W = windows[w];
            bool any = false;
            for (int f = 0; f < W.n_features; f++) {
                const int nobs = W.first_obs[f + 1] - W.first_obs[f];
                if (!tri_used(nobs, W.start_frame[f], ws) || W.depth_in[f] > 0) continue;
                any = true;
                cand[at++] = make_int4((int)(slot * TRI_NF) + W.start_frame[f], nobs, (int)row, 0);
                std::memcpy(pts + row * 3, W.points + (size_t)W.first_obs[f] * 3, (size_t)nobs * 24);
                row += (size_t)nobs;
            }
            if (!any) continue;
            double *ps = pose + slot * TRI_POSE_DBL;
            std::memset(ps, 0, TRI_POSE_DBL * 8);
            std::memcpy(ps, W.Ps, (size_t)W.n_frames * 24);
            std::memcpy(ps + 3 * TRI_NF, W.Rs, (size_t)W.n_frames * 72);
            std::memcpy(ps + 12 * TRI_NF, W.tic, 24);
            std::memcpy(ps + 12 * TRI_NF + 3, W.ric, 72);
            slot++;
        }
    }
    if (n_cand > 0) {
        HIPCHECK(h, c->io.upload(h, in_bytes));
        TriDev d;
        char *ib = c->io.in.as<char>(), *ob = c->io.out.as<char>();
        d.pose = (const double *)(ib + o_pose); d.cand = (const int4 *)(ib + o_cand); d.pts = (const double *)(ib + o_pts);
        d.cam = c->cam.as<double>(); d.depth = (double *)(ob + o_depth); d.meta = (unsigned *)(ob + o_meta);
        d.n_slots = (int)n_slots; d.n_cand = (int)n_cand; d.init_depth = init_depth;
        ProfMarks prof(h, c->prof);
        hipLaunchKernelGGL(tri_cameras, dim3((unsigned)((n_slots * TRI_NF + 63) / 64)), dim3(64), 0, h->stream, d);
        prof.mark(0);
        hipLaunchKernelGGL(tri_solve, dim3((unsigned)((n_cand + TRI_LANES - 1) / TRI_LANES)), dim3(TRI_LANES), 0, h->stream, d);
        prof.mark(0);
        HIPCHECK(h, hipGetLastError());
        HIPCHECK(h, c->io.download(h, out_bytes));
    }
    // the outputs in feature order: the candidates' from the download, the others' from the host
    const double *depth = (const double *)((const char *)c->io.down.p + o_depth);
    const unsigned *meta = (const unsigned *)((const char *)c->io.down.p + o_meta);
    size_t at = 0;
    for (int w = 0; w < n_windows; w++) {
        const vilf_tri_window &W = windows[w];
        vilf_tri_result r = {0, 0, 0, 0};
        for (int f = 0; f < W.n_features; f++) {
            const int nobs = W.first_obs[f + 1] - W.first_obs[f];
            const bool used = tri_used(nobs, W.start_frame[f], ws);
            double dep = W.depth_in[f];
            unsigned fl = used ? VILF_TRI_USED : 0, sw = 0;
            if (used && !(dep > 0)) {
                dep = depth[at]; fl = meta[at] & 0xffu; sw = (meta[at] >> 8) & 0xffu; at++;
                r.n_candidates++;
                if (fl & VILF_TRI_RESET) r.n_reset++;
                if (fl & VILF_TRI_NONFINITE) r.n_nonfinite++;
                W.depth_out[f] = dep;
            } else std::memcpy(W.depth_out + f, W.depth_in + f, 8);
            if (used) {
                if (W.inv_depth_out) W.inv_depth_out[r.n_used] = dep > 0 ? 1.0 / dep : 1.0 / init_depth;
                r.n_used++;
            }
            if (W.flags_out) W.flags_out[f] = (unsigned char)fl;
            if (W.sweeps_out) W.sweeps_out[f] = (unsigned char)sw;
        }
        out[w] = r;
    }
    return VILF_OK;
}

extern "C" int vilf_features_profile(vilf_handle *h, double ms_out[1], long launches_out[1]) { return vilf_stage_profile(h, ST_TRI, &TriCtx::prof, ms_out, launches_out); }
