// vilf_track.hip — the camera half of the feature-tracker node on the device (≙ FeatureTracker::readImage, feature_tracker/feature_tracker.cpp:119-209, and the
//   updateID loop, feature_tracker_node.cpp:285-292). The arithmetic is stated once, in include/vilfusion.h ("Image feature tracker"); OpenCV is not a dependency.
// One frame = one chain of launches on the handle's stream, counts stay on the device:
//   tk_pyr_down      a 32 x 8 tile of a level through LDS with its 2-pixel halo (one launch per level); the "next" pyramid becomes "current" by a pointer swap
//   tk_lk            a wave per point, all levels in one launch: the 441 window positions dealt over the 64 lanes, T / Tx / Ty in registers across the iterations,
//                    exact integer sums reduced over the wave, the 2 x 2 solve and the stopping rules the same in every lane; at most 30 iterations, no spin
//   tk_setmask       one workgroup: rank by (track_cnt descending, index), then wave 0 keeps the points greedily by their discs
//   tk_paint         a workgroup per kept point: its disc into the byte mask of forbidden pixels
//   tk_response      a 32 x 8 tile: Sobel at the tile + 1 ring, the 3 x 3 sums, lambda; the maximum over the allowed pixels by an atomic max on the bit pattern
//   tk_candidates    threshold / 3 x 3 maximum / allowed -> pixel indices compacted with a counter (the buffer holds W * H entries, see vilf_track_init)
//   radix sorts      by index, then tk_keys + a stable sort by ~bits(lambda): the order (lambda descending, index ascending), whatever the compaction order was
//   tk_corners       one wave: the candidates in order, the lanes test one candidate against the accepted corners in LDS
//   tk_finish        one workgroup: ids, undistortion, velocity against the previous frame's (id, un) table, which it then replaces
// The two optional steps (vilf_track_configure; both off unless asked for):
//   tk_clahe_lut     a workgroup per tile: the 256-bin histogram of the padded tile by LDS integer atomics, clip, redistribute, prefix sum -> the tile's 256-byte LUT
//   tk_clahe_remap   a 32 x 8 tile: the four neighbouring LUTs interpolated in float32, written into level 0 of the "next" pyramid (the raw image has its own buffer)
//   tk_f_lift        one workgroup: the survivors of LK's status, in list order, both points lifted to the float32 pixels of the virtual camera
//   tk_f_hypotheses  a lane per hypothesis: sample, Hartley, M = A^T A and the Jacobi vectors in LDS (a column per lane), rank 2, denormalise -> F_k, valid_k
//   tk_f_score       a wave per hypothesis: the lanes stride over the points, an integer wave sum, one 64-bit atomicMax of (score + 1, K - 1 - k)
//   tk_f_apply       one workgroup: the winner's inlier mask into LK's status bytes, which tk_setmask reads as before
// The dynamic-object and fisheye masks (vilf_track_read_image_mask, vilf_track_set_fisheye_mask; a tracker that uses neither issues the launches above, no more):
//   tk_mask_erode    a 32 x 8 tile: the mask binarised into LDS with a halo of r (outside the image = set), every thread tests its pixel against the element's row spans
//   tk_mask_probe    a thread per point: static = LK's status AND the four probes of E, into a status array of its own (setMask's bytes are not touched)
//   tk_f_lift / tk_f_hypotheses / tk_f_score as they are, on the static status array, then
//   tk_fm_apply      one workgroup: the winner by the same packed word, every survivor lifted again and tested one-sidedly against the winner's F
//   tk_mask_init     the forbidden-pixel map from E and the fisheye mask, in place of the memset in front of tk_paint
// Per frame the host uploads the image (and the mask) and downloads the list (count + rows, one copy).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include "vilf_internal.hpp"
#include "vilf_device.hpp"
#include "vilf_kernels.hpp"
#include "vilf_sort.hpp"
#include "vilf_fmat.hpp"
#include "vilf_image.hpp"                 // tk_r, TkCam, tk_undistort: the reflected index and the undistortion text, shared with vilf_kf.hip

#define TK_WIN 21
#define TK_NPOS (TK_WIN * TK_WIN)
#define TK_SLOTS ((TK_NPOS + 63) / 64)     // window positions per lane
#define TK_LEVELS 4
#define TK_MAX_ITERS 30
#define TK_MAXN VILF_MAX_FEATURES           // rows of the list; accepted corners of one detection
#define TK_STAGES 5
#define TK_FE_STAGES 2                      // CLAHE, rejectWithF
#define TK_MK_STAGES 2                      // erode, probe + rejectWithF_mask
#define TK_ER_MAX VILF_TRACK_MAX_ERODE
#define TK_F_MAXK VILF_TRACK_MAX_HYPOTHESES

struct TkPyr { unsigned char *lv[TK_LEVELS]; int w[TK_LEVELS], h[TK_LEVELS], lmax; };      // rows are tight (stride = width)
// a feature list in one allocation: hdr[16] (hdr[0] = rows), then ids, track_cnt, cur_pts, un_pts, velocity, each for `cap` rows
struct TkList { int *hdr, *ids, *cnt; float2 *pts, *un, *vel; };
#define TK_LIST_HDR 16
static inline size_t tk_list_bytes(int cap) { return TK_LIST_HDR * 4 + (size_t)cap * 32; }
static inline TkList tk_list(void *base, int cap) {
    TkList l;
    l.hdr = (int *)base; l.ids = l.hdr + TK_LIST_HDR; l.cnt = l.ids + cap;
    l.pts = (float2 *)(l.cnt + cap); l.un = l.pts + cap; l.vel = l.un + cap;
    return l;
}
// control words of one tracker (device): written by the kernels, never read by the host
enum { TC_N = 0, TC_KEPT, TC_NMAX, TC_NCAND, TC_NID, TC_PREVN, TC_LAMMAX = 8 /* unsigned long long at ints 8, 9 */, TC_INTS = 16 };
// rejectWithF on the device: the lifted survivors and their rows in the list, control words (FC_*), F and valid flag per hypothesis, the result record
// (best, inliers, F as 11 doubles)
enum { FC_M = 0, FC_BEST = 2 /* unsigned long long at ints 2, 3: (score + 1) << 32 | (K - 1 - k); 0 = no valid hypothesis */, FC_INTS = 4 };
#define TK_F_RES 11
struct TkF { float2 *ua, *ub; int *src, *fctl; double *F; int *valid; double *res; };

// ---- launch contract -----------------------------------------------------------------------------------------------------
#define TK_TW 32                        // tk_pyr_down, tk_response: block (32, 8), grid = tiles of the output
#define TK_TH 8
#define TK_PYR_LW (2 * TK_TW + 3)
#define TK_PYR_LH (2 * TK_TH + 3)
#define TK_LK_WAVES 4                   // tk_lk: grid = ceil(points / 4), a wave per point; no workgroup barrier
#define TK_NT 256                       // tk_setmask, tk_finish: one workgroup; tk_paint: grid = list capacity; tk_candidates, tk_keys: 1-D over the pixels / slots
#define TK_CORNERS_NT 64                // tk_corners: one wave
__global__ void tk_pyr_down(const unsigned char *src, int sw, int sh, unsigned char *dst, int dw, int dh);
__global__ void tk_lk(TkPyr prev, TkPyr next, const float2 *pts, const int *n_dev, int n_host, float2 *out, unsigned char *status, int border);
__global__ void tk_setmask(TkList cur, const float2 *fwd, const unsigned char *status, TkList nxt, int *ctl, int max_cnt, long long md2, const unsigned char *fish, int W, int H);   // fish: the fisheye mask or null
__global__ void tk_paint(const float2 *pts, const int *ctl, unsigned char *mask, int W, int H, long long md, long long md2);
__global__ void tk_response(const unsigned char *img, const unsigned char *mask, int W, int H, int *ctl, double *lam);
__global__ void tk_candidates(const double *lam, const unsigned char *mask, int W, int H, int *ctl, unsigned *cidx, int cap);
__global__ void tk_keys(const double *lam, const unsigned *cidx, const int *ctl, int cap, unsigned long long *key, int *val);
__global__ void tk_corners(const int *val, int W, int cap, int *ctl, TkList l, long long md2);
__global__ void tk_finish(TkList l, int *ctl, int *prev_ids, float2 *prev_un, TkCam cam, double dt, int has_prev);
// TK_F_LANES (vilf_fmat.hpp)              tk_f_hypotheses: block 64 (one wave), grid = ceil(K / 64), a lane per hypothesis, its matrices a column of the LDS arrays; no barrier
#define TK_F_WAVES 4                    // tk_f_score: block 256, grid = ceil(K / 4), a wave per hypothesis; no workgroup barrier
__global__ void tk_clahe_lut(const unsigned char *img, int W, int H, int tw, int th, int limit, float scale, unsigned char *lut);      // grid (tx, ty), block TK_NT
__global__ void tk_clahe_remap(const unsigned char *img, int W, int H, int tx, int ty, float inv_tw, float inv_th, const unsigned char *lut, unsigned char *out);   // block (32, 8), tiles of the image
__global__ void tk_f_lift(const float2 *cur, const float2 *fwd, const unsigned char *status, const int *n_dev, int n_host, TkCam cam, double focal, double half_w, double half_h, TkF f);   // one workgroup, TK_NT
__global__ void tk_f_hypotheses(TkF f, int K, unsigned seed);
__global__ void tk_f_score(TkF f, int K, double thr2);
__global__ void tk_f_apply(TkF f, int K, double thr2, unsigned char *status);      // one workgroup, TK_NT
struct TkSpans { int r, hw[TK_ER_MAX + 1]; };      // the structuring element: row |dy| covers |dx| <= hw[|dy|]
__global__ void tk_mask_erode(const unsigned char *mask, int W, int H, TkSpans sp, unsigned char *E);      // block (32, 8), tiles of the image; LDS (8 + 2 * 16) x (32 + 2 * 16) bytes
__global__ void tk_mask_probe(const unsigned char *E, const float2 *fwd, const unsigned char *status, const int *n_dev, int n_host, int W, int H, int d, unsigned char *is_static);   // 1-D over the list's rows, TK_NT
__global__ void tk_fm_apply(TkF f, int K, const float2 *cur, const float2 *fwd, const int *n_dev, int n_host, TkCam cam, double focal, double half_w, double half_h, double epi, unsigned char *status);   // one workgroup, TK_NT
__global__ void tk_mask_init(const unsigned char *E, const unsigned char *fish, size_t n, unsigned char *mask);      // 1-D, TK_NT, four pixels per thread

struct TrackCtx : VilfStage {
    vilf_track_params p;
    TkPyr pyr[4];                       // [0], [1]: current / next of the tracker (cur says which); [2], [3]: the stateless calls
    int cur = 0, lcur = 0;
    long frames = 0;
    double t_prev = 0;
    int n_host = 0;                     // rows of the list as downloaded by the last vilf_track_read_image
    size_t ncell = 0;                   // W * H
    DBuf pyrmem[4], list[2], tmplist, ctl, tmpctl, prev_ids, prev_un, fwd, status, lkpts, mask, lam, cidx, cidx2, cval, key, key2, val, val2, temp;
    DBuf raw, lut, fmem;                // the optional steps: the image before CLAHE, the tiles' LUTs (VILF_TRACK_MAX_TILES), everything of rejectWithF (tk_f)
    DBuf mraw, er, fish, sstatus;       // the masks: the uploaded mask image, E, the fisheye mask (has_fish), the static status of the probe
    PinBuf mstage;                      // a mask on its way to the device
    vilf_track_mask_params mp;          // the defaults after vilf_track_init
    bool has_fish = false;
    StageProf<TK_MK_STAGES> mk_prof;
    vilf_track_frontend fe;             // both off and the defaults after vilf_track_init
    StageProf<TK_FE_STAGES> fe_prof;
    PinBuf pin, stage[4];               // the downloaded list; the image on its way to level 0 of pyramid k
    StageProf<TK_STAGES> prof;
    void profile_reset() override { prof.reset(); fe_prof.reset(); mk_prof.reset(); }
};

namespace {
#define TK_WSYNC __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier()

VD long long tk_wave_sum(long long v) {          // exact, so the order is free; every lane gets the total
    for (int o = 32; o > 0; o >>= 1) {
        const int lo = __shfl_xor((int)(unsigned)(v & 0xffffffffll), o), hi = __shfl_xor((int)(v >> 32), o);
        v += ((long long)hi << 32) | (long long)(unsigned)lo;
    }
    return v;
}
struct TkCorner { int ix, iy, w00, w01, w10, w11; bool ok; };
// top-left corner of the window around (x, y) and the fixed-point bilinear weights; ok = inside the bounds rule (a NaN is outside)
VD TkCorner tk_corner(float x, float y, int W, int H) {
    TkCorner c;
    const float cx = __fsub_rn(x, 10.f), cy = __fsub_rn(y, 10.f), fx = floorf(cx), fy = floorf(cy);
    c.ok = fx >= -(float)TK_WIN && fx < (float)W && fy >= -(float)TK_WIN && fy < (float)H;
    const float a = c.ok ? __fsub_rn(cx, fx) : 0.f, b = c.ok ? __fsub_rn(cy, fy) : 0.f;
    c.ix = c.ok ? (int)fx : 0; c.iy = c.ok ? (int)fy : 0;
    const float na = __fsub_rn(1.f, a), nb = __fsub_rn(1.f, b);
    c.w00 = (int)rintf(__fmul_rn(__fmul_rn(na, nb), 16384.f));
    c.w01 = (int)rintf(__fmul_rn(__fmul_rn(a, nb), 16384.f));
    c.w10 = (int)rintf(__fmul_rn(__fmul_rn(na, b), 16384.f));
    c.w11 = 16384 - c.w00 - c.w01 - c.w10;
    return c;
}
// the bilinear form of the image at window position (x, y): (sum w I + 256) >> 9
VD int tk_bilinear(const unsigned char *I, int W, int H, int x, int y, const TkCorner &c) {
    const int x0 = tk_r(x, W), x1 = tk_r(x + 1, W);
    const unsigned char *r0 = I + (size_t)tk_r(y, H) * W, *r1 = I + (size_t)tk_r(y + 1, H) * W;
    return (c.w00 * (int)r0[x0] + c.w01 * (int)r0[x1] + c.w10 * (int)r1[x0] + c.w11 * (int)r1[x1] + 256) >> 9;
}
}  // namespace

// ---- tk_pyr_down ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TK_TW * TK_TH) void tk_pyr_down(const unsigned char *src, int sw, int sh, unsigned char *dst, int dw, int dh) {
    __shared__ unsigned char s[TK_PYR_LH][TK_PYR_LW + 1];
    const int tx = threadIdx.x, ty = threadIdx.y, t = ty * TK_TW + tx;
    const int x0 = blockIdx.x * TK_TW, y0 = blockIdx.y * TK_TH;
    for (int i = t; i < TK_PYR_LH * TK_PYR_LW; i += TK_TW * TK_TH) {
        const int ly = i / TK_PYR_LW, lx = i % TK_PYR_LW;
        s[ly][lx] = src[(size_t)tk_r(2 * y0 - 2 + ly, sh) * sw + tk_r(2 * x0 - 2 + lx, sw)];
    }
    __syncthreads();
    const int x = x0 + tx, y = y0 + ty;
    if (x >= dw || y >= dh) return;
    const int k[5] = {1, 4, 6, 4, 1};
    int acc = 0;
#pragma unroll
    for (int j = 0; j < 5; j++)
#pragma unroll
        for (int i = 0; i < 5; i++) acc += k[i] * k[j] * (int)s[2 * ty + j][2 * tx + i];
    dst[(size_t)y * dw + x] = (unsigned char)((acc + 128) >> 8);
}

// ---- tk_lk: a wave per point -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * TK_LK_WAVES) void tk_lk(TkPyr prev, TkPyr next, const float2 *pts, const int *n_dev, int n_host, float2 *out, unsigned char *status, int border) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * TK_LK_WAVES + (threadIdx.x >> 6);
    const int n = n_dev ? *n_dev : n_host;
    if (i >= n) return;                                  // the whole wave
    const float2 p = pts[i];
    float qx = 0.f, qy = 0.f;
    int st = 1;
    for (int L = prev.lmax; L >= 0; L--) {
        const int W = prev.w[L], H = prev.h[L];
        const unsigned char *I = prev.lv[L], *J = next.lv[L];
        const float scale = 1.f / (float)(1 << L);
        const float px = __fmul_rn(p.x, scale), py = __fmul_rn(p.y, scale);
        if (L == prev.lmax) { qx = px; qy = py; } else { qx = __fmul_rn(2.f, qx); qy = __fmul_rn(2.f, qy); }
        const TkCorner c = tk_corner(px, py, W, H);
        if (!c.ok) { if (L == 0) st = 0; continue; }
        // template: T, Tx, Ty of this lane's window positions
        int T[TK_SLOTS], Tx[TK_SLOTS], Ty[TK_SLOTS];
        long long s11 = 0, s12 = 0, s22 = 0;
#pragma unroll
        for (int k = 0; k < TK_SLOTS; k++) {
            const int pos = lane + 64 * k;
            T[k] = 0; Tx[k] = 0; Ty[k] = 0;
            if (pos < TK_NPOS) {
                const int x = c.ix + pos % TK_WIN, y = c.iy + pos / TK_WIN;
                int v[4][4];                             // the pixels (x - 1 .. x + 2, y - 1 .. y + 2), read through R
                int cx[4];
#pragma unroll
                for (int a = 0; a < 4; a++) cx[a] = tk_r(x - 1 + a, W);
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const unsigned char *row = I + (size_t)tk_r(y - 1 + b, H) * W;
#pragma unroll
                    for (int a = 0; a < 4; a++) v[b][a] = (int)row[cx[a]];
                }
                int gx[2][2], gy[2][2];                  // Scharr at (x + a, y + b); 0 outside the image
#pragma unroll
                for (int b = 0; b < 2; b++)
#pragma unroll
                    for (int a = 0; a < 2; a++) {
                        const bool in = (unsigned)(x + a) < (unsigned)W && (unsigned)(y + b) < (unsigned)H;
                        const int r = 1 + b, q = 1 + a;
                        const int sx = 3 * (v[r - 1][q + 1] - v[r - 1][q - 1]) + 10 * (v[r][q + 1] - v[r][q - 1]) + 3 * (v[r + 1][q + 1] - v[r + 1][q - 1]);
                        const int sy = 3 * (v[r + 1][q - 1] - v[r - 1][q - 1]) + 10 * (v[r + 1][q] - v[r - 1][q]) + 3 * (v[r + 1][q + 1] - v[r - 1][q + 1]);
                        gx[b][a] = in ? sx : 0; gy[b][a] = in ? sy : 0;
                    }
                T[k] = (c.w00 * v[1][1] + c.w01 * v[1][2] + c.w10 * v[2][1] + c.w11 * v[2][2] + 256) >> 9;
                Tx[k] = (c.w00 * gx[0][0] + c.w01 * gx[0][1] + c.w10 * gx[1][0] + c.w11 * gx[1][1] + 8192) >> 14;
                Ty[k] = (c.w00 * gy[0][0] + c.w01 * gy[0][1] + c.w10 * gy[1][0] + c.w11 * gy[1][1] + 8192) >> 14;
                s11 += (long long)Tx[k] * Tx[k]; s12 += (long long)Tx[k] * Ty[k]; s22 += (long long)Ty[k] * Ty[k];
            }
        }
        const double sc = 0x1p-20;
        const double a11 = __dmul_rn((double)tk_wave_sum(s11), sc), a12 = __dmul_rn((double)tk_wave_sum(s12), sc), a22 = __dmul_rn((double)tk_wave_sum(s22), sc);
        const double D = __dsub_rn(__dmul_rn(a11, a22), __dmul_rn(a12, a12)), d = __dsub_rn(a11, a22);
        const double e = __ddiv_rn(__dsub_rn(__dadd_rn(a11, a22), __dsqrt_rn(__dadd_rn(__dmul_rn(d, d), __dmul_rn(__dmul_rn(4.0, a12), a12)))), 882.0);
        if (e < 1e-4 || D < 1.1920929e-7) { if (L == 0) st = 0; continue; }
        const double inv = __ddiv_rn(1.0, D);
        double pdx = 0.0, pdy = 0.0;
        for (int it = 0; it < TK_MAX_ITERS; it++) {
            const TkCorner cj = tk_corner(qx, qy, W, H);
            if (!cj.ok) { if (L == 0) st = 0; break; }
            long long t1 = 0, t2 = 0;
#pragma unroll
            for (int k = 0; k < TK_SLOTS; k++) {
                const int pos = lane + 64 * k;
                if (pos < TK_NPOS) {
                    const int df = tk_bilinear(J, W, H, cj.ix + pos % TK_WIN, cj.iy + pos / TK_WIN, cj) - T[k];
                    t1 += (long long)df * Tx[k]; t2 += (long long)df * Ty[k];
                }
            }
            const double b1 = __dmul_rn((double)tk_wave_sum(t1), sc), b2 = __dmul_rn((double)tk_wave_sum(t2), sc);
            const double dx = __dmul_rn(__dsub_rn(__dmul_rn(a12, b2), __dmul_rn(a22, b1)), inv), dy = __dmul_rn(__dsub_rn(__dmul_rn(a12, b1), __dmul_rn(a11, b2)), inv);
            qx = (float)__dadd_rn((double)qx, dx); qy = (float)__dadd_rn((double)qy, dy);
            if (__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)) <= 1e-4) break;
            if (it > 0 && fabs(__dadd_rn(dx, pdx)) < 0.01 && fabs(__dadd_rn(dy, pdy)) < 0.01) {
                qx = (float)__dsub_rn((double)qx, __dmul_rn(dx, 0.5)); qy = (float)__dsub_rn((double)qy, __dmul_rn(dy, 0.5));
                break;
            }
            pdx = dx; pdy = dy;
        }
    }
    if (border) {                                        // inBorder (feature_tracker.cpp:5-11)
        const float rx = rintf(qx), ry = rintf(qy);
        if (!(rx >= 1.f && rx <= (float)(prev.w[0] - 2) && ry >= 1.f && ry <= (float)(prev.h[0] - 2))) st = 0;
    }
    if (lane == 0) { out[i] = make_float2(qx, qy); status[i] = (unsigned char)st; }
}

// ---- tk_setmask: one workgroup -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TK_NT) void tk_setmask(TkList cur, const float2 *fwd, const unsigned char *status, TkList nxt, int *ctl, int max_cnt, long long md2, const unsigned char *fish, int W, int H) {
    __shared__ int s_cnt[TK_MAXN], s_order[TK_MAXN], s_src[TK_MAXN];
    __shared__ int2 s_px[TK_MAXN], s_acc[TK_MAXN];
    __shared__ int s_m, s_nk;
    const int t = threadIdx.x, n = min(ctl[TC_N], TK_MAXN);
    if (t == 0) s_m = 0;
    for (int i = t; i < n; i += TK_NT) {
        const float2 f = fwd[i];
        const int2 px = make_int2((int)rintf(f.x), (int)rintf(f.y));
        bool keep = status[i] != 0;
        if (fish) {                                      // a survivor's pixel is inside the image (inBorder); the address is clamped all the same, the value selected after the load
            const unsigned char v = fish[(size_t)min(max(px.y, 0), H - 1) * W + min(max(px.x, 0), W - 1)];
            keep = keep && v == 255;
        }
        s_cnt[i] = keep ? cur.cnt[i] : -1;               // track counts are positive
        s_px[i] = px;
    }
    __syncthreads();
    for (int i = t; i < n; i += TK_NT) {
        const int ci = s_cnt[i];
        if (ci < 0) continue;
        int rank = 0;
        for (int j = 0; j < n; j++) { const int cj = s_cnt[j]; rank += (cj > ci || (cj == ci && j < i)) ? 1 : 0; }      // cj >= 0 > -1 only for survivors when ci >= 0
        s_order[rank] = i;
        atomicAdd(&s_m, 1);
    }
    __syncthreads();
    if (t < 64) {                                        // wave 0: the survivors in order, each against the kept pixels
        const int m = s_m;
        int nk = 0;
        for (int r = 0; r < m; r++) {
            const int src = s_order[r];
            const int2 c = s_px[src];
            bool hit = false;
            for (int k = t; k < nk; k += 64) {
                const int2 a = s_acc[k];
                const long long dx = (long long)c.x - a.x, dy = (long long)c.y - a.y;
                hit |= dx * dx + dy * dy <= md2;
            }
            if (!__any(hit)) {
                if (t == 0) { s_acc[nk] = c; s_src[nk] = src; }
                nk++;
                TK_WSYNC;
            }
        }
        if (t == 0) s_nk = nk;
    }
    __syncthreads();
    const int nk = s_nk;
    for (int k = t; k < nk; k += TK_NT) {
        const int src = s_src[k];
        nxt.ids[k] = cur.ids[src]; nxt.cnt[k] = cur.cnt[src] + 1; nxt.pts[k] = fwd[src];
    }
    if (t == 0) {
        ctl[TC_KEPT] = nk; ctl[TC_NMAX] = max_cnt - nk; ctl[TC_NCAND] = 0;
        *(unsigned long long *)(ctl + TC_LAMMAX) = 0ull;
    }
}

// ---- tk_paint: a workgroup per kept point ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(TK_NT) void tk_paint(const float2 *pts, const int *ctl, unsigned char *mask, int W, int H, long long md, long long md2) {
    const int b = blockIdx.x;
    if (b >= ctl[TC_KEPT] || ctl[TC_NMAX] <= 0) return;
    const float2 f = pts[b];
    const long long px = (long long)rintf(f.x), py = (long long)rintf(f.y);
    const long long x0 = max(px - md, 0ll), x1 = min(px + md, (long long)W - 1), y0 = max(py - md, 0ll), y1 = min(py + md, (long long)H - 1);
    if (x1 < x0 || y1 < y0) return;
    const long long bw = x1 - x0 + 1, cells = bw * (y1 - y0 + 1);        // <= W * H
    for (long long i = threadIdx.x; i < cells; i += TK_NT) {
        const long long x = x0 + i % bw, y = y0 + i / bw, dx = x - px, dy = y - py;
        if (dx * dx + dy * dy <= md2) mask[y * W + x] = 1;
    }
}

// ---- tk_response: Sobel, 3 x 3 sums, lambda ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(TK_TW * TK_TH) void tk_response(const unsigned char *img, const unsigned char *mask, int W, int H, int *ctl, double *lam) {
    __shared__ unsigned char s_i[TK_TH + 4][TK_TW + 4];          // pixel (x0 - 2 + lx, y0 - 2 + ly) through R
    __shared__ short s_sx[TK_TH + 2][TK_TW + 2], s_sy[TK_TH + 2][TK_TW + 2];
    __shared__ unsigned long long s_max;
    if (ctl[TC_NMAX] <= 0) return;
    const int tx = threadIdx.x, ty = threadIdx.y, t = ty * TK_TW + tx;
    const int x0 = blockIdx.x * TK_TW, y0 = blockIdx.y * TK_TH;
    if (t == 0) s_max = 0ull;
    for (int i = t; i < (TK_TH + 4) * (TK_TW + 4); i += TK_TW * TK_TH) {
        const int ly = i / (TK_TW + 4), lx = i % (TK_TW + 4);
        s_i[ly][lx] = img[(size_t)tk_r(y0 - 2 + ly, H) * W + tk_r(x0 - 2 + lx, W)];
    }
    __syncthreads();
    for (int i = t; i < (TK_TH + 2) * (TK_TW + 2); i += TK_TW * TK_TH) {
        const int ly = i / (TK_TW + 2), lx = i % (TK_TW + 2);
        // the Sobel value of the neighbour coordinate taken through R; its own reads go through R again. A pixel x < W of the tile needs the positions
        // x - 1 .. x + 1 <= W: R(-1) = 1 reads the columns 0, 2; R(W) = W - 2 reads W - 3, W - 1; a position inside the image reads p - 1 .. p + 1 or their
        // reflections p + 1, p - 1. All of these lie in [x0 - 2, x0 + TK_TW + 2), the columns the tile holds. Positions past W (no pixel needs them) are clamped
        // into the tile. Rows likewise.
        const int gx = tk_r(x0 - 1 + lx, W), gy = tk_r(y0 - 1 + ly, H);
        const int cl = min(max(tk_r(gx - 1, W) - x0 + 2, 0), TK_TW + 3), cc = min(max(gx - x0 + 2, 0), TK_TW + 3), cr = min(max(tk_r(gx + 1, W) - x0 + 2, 0), TK_TW + 3);
        const int ru = min(max(tk_r(gy - 1, H) - y0 + 2, 0), TK_TH + 3), rc = min(max(gy - y0 + 2, 0), TK_TH + 3), rd = min(max(tk_r(gy + 1, H) - y0 + 2, 0), TK_TH + 3);
        const int sx = ((int)s_i[ru][cr] + 2 * (int)s_i[rc][cr] + (int)s_i[rd][cr]) - ((int)s_i[ru][cl] + 2 * (int)s_i[rc][cl] + (int)s_i[rd][cl]);
        const int sy = ((int)s_i[rd][cl] + 2 * (int)s_i[rd][cc] + (int)s_i[rd][cr]) - ((int)s_i[ru][cl] + 2 * (int)s_i[ru][cc] + (int)s_i[ru][cr]);
        s_sx[ly][lx] = (short)sx; s_sy[ly][lx] = (short)sy;
    }
    __syncthreads();
    const int x = x0 + tx, y = y0 + ty;
    if (x < W && y < H) {
        int P = 0, Q = 0, S = 0;
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
            for (int i = 0; i < 3; i++) { const int a = s_sx[ty + j][tx + i], b = s_sy[ty + j][tx + i]; P += a * a; Q += a * b; S += b * b; }
        const double Pd = (double)P, Qd = (double)Q, Sd = (double)S, d = __dsub_rn(Pd, Sd);
        const double l = __dsub_rn(__dadd_rn(Pd, Sd), __dsqrt_rn(__dadd_rn(__dmul_rn(d, d), __dmul_rn(__dmul_rn(4.0, Qd), Qd))));
        const size_t at = (size_t)y * W + x;
        lam[at] = l;
        if (!mask[at] && l > 0.0) atomicMax(&s_max, (unsigned long long)__double_as_longlong(l));      // non-negative doubles order as their bit patterns
    }
    __syncthreads();
    if (t == 0 && s_max) atomicMax((unsigned long long *)(ctl + TC_LAMMAX), s_max);
}

// ---- tk_candidates ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TK_NT) void tk_candidates(const double *lam, const unsigned char *mask, int W, int H, int *ctl, unsigned *cidx, int cap) {
    if (ctl[TC_NMAX] <= 0) return;
    const long long at = (long long)blockIdx.x * TK_NT + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool is = false;
    if (at < (long long)W * H) {
        const int x = (int)(at % W), y = (int)(at / W);
        if (x >= 1 && x <= W - 2 && y >= 1 && y <= H - 2 && !mask[at]) {
            const double lmax = __longlong_as_double((long long)*(const unsigned long long *)(ctl + TC_LAMMAX));
            const double l = lam[at];
            is = l > __dmul_rn(0.01, lmax);
            for (int j = -1; j <= 1; j++) for (int i = -1; i <= 1; i++) is = is && l >= lam[at + (long long)j * W + i];
        }
    }
    const unsigned long long b = __ballot(is);
    if (!b) return;
    int base = 0;
    if (lane == 0) base = atomicAdd(ctl + TC_NCAND, __popcll(b));
    base = __shfl(base, 0);
    const int slot = base + __popcll(b & ((1ull << lane) - 1ull));
    if (is && slot < cap) cidx[slot] = (unsigned)at;
}

// ---- tk_keys: slot s of the index-sorted candidates -> (~bits(lambda), index); the slots behind the count sort last ------------------------------
__global__ __launch_bounds__(TK_NT) void tk_keys(const double *lam, const unsigned *cidx, const int *ctl, int cap, unsigned long long *key, int *val) {
    const long long s = (long long)blockIdx.x * TK_NT + threadIdx.x;
    if (s >= cap) return;
    const int cnt = min(ctl[TC_NCAND], cap);
    const unsigned at = s < cnt ? cidx[s] : 0xffffffffu;
    if (at < (unsigned)cap) { key[s] = ~(unsigned long long)__double_as_longlong(lam[at]); val[s] = (int)at; }
    else { key[s] = ~0ull; val[s] = -1; }
}

// ---- tk_corners: one wave ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TK_CORNERS_NT) void tk_corners(const int *val, int W, int cap, int *ctl, TkList l, long long md2) {
    __shared__ int2 s_acc[TK_MAXN];
    const int lane = threadIdx.x, cnt = min(ctl[TC_NCAND], cap), kept = ctl[TC_KEPT], n_max = min(ctl[TC_NMAX], TK_MAXN);
    int nacc = 0;
    for (int base = 0; base < cnt && nacc < n_max; base += 64) {
        const int mine = base + lane < cnt ? val[base + lane] : 0;
        const int m = min(64, cnt - base);
        for (int j = 0; j < m && nacc < n_max; j++) {
            const int at = __shfl(mine, j);
            if ((unsigned)at >= (unsigned)cap) continue;          // never a candidate's index; the same in every lane
            const int2 c = make_int2(at % W, at / W);
            bool hit = false;
            for (int k = lane; k < nacc; k += 64) {
                const int2 a = s_acc[k];
                const long long dx = (long long)c.x - a.x, dy = (long long)c.y - a.y;
                hit |= dx * dx + dy * dy < md2;
            }
            if (!__any(hit)) {
                if (lane == 0) {
                    s_acc[nacc] = c;
                    l.pts[kept + nacc] = make_float2((float)c.x, (float)c.y); l.ids[kept + nacc] = -1; l.cnt[kept + nacc] = 1;
                }
                nacc++;
                TK_WSYNC;
            }
        }
    }
    if (lane == 0) ctl[TC_N] = kept + nacc;
}

// ---- tk_finish: ids, undistortion, velocity -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TK_NT) void tk_finish(TkList l, int *ctl, int *prev_ids, float2 *prev_un, TkCam cam, double dt, int has_prev) {
    const int t = threadIdx.x, n = min(ctl[TC_N], TK_MAXN), kept = ctl[TC_KEPT], n_id = ctl[TC_NID], prev_n = ctl[TC_PREVN];
    for (int i = t; i < n; i += TK_NT) {
        const int id = i < kept ? l.ids[i] : n_id + (i - kept);      // the new points stand behind the kept ones, in list order (updateID)
        const float2 p = l.pts[i];
        double ux, uy;
        tk_undistort(cam, p, ux, uy);
        const float2 un = make_float2((float)ux, (float)uy);
        float2 v = make_float2(0.f, 0.f);
        if (has_prev && i < kept) {
            for (int k = 0; k < prev_n; k++)
                if (prev_ids[k] == id) {
                    const float2 q = prev_un[k];
                    v = make_float2((float)__ddiv_rn(__dsub_rn((double)un.x, (double)q.x), dt), (float)__ddiv_rn(__dsub_rn((double)un.y, (double)q.y), dt));
                    break;
                }
        }
        l.ids[i] = id; l.un[i] = un; l.vel[i] = v;
    }
    __syncthreads();                                     // every read of the previous table is done
    for (int i = t; i < n; i += TK_NT) { prev_ids[i] = l.ids[i]; prev_un[i] = l.un[i]; }
    if (t == 0) { ctl[TC_PREVN] = n; ctl[TC_NID] = n_id + (n - min(kept, n)); l.hdr[0] = n; }
}

// ---- tk_clahe_lut: a workgroup per tile ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TK_NT) void tk_clahe_lut(const unsigned char *img, int W, int H, int tw, int th, int limit, float scale, unsigned char *lut) {
    __shared__ int s_h[256], s_ex;
    const int t = threadIdx.x, x0 = blockIdx.x * tw, y0 = blockIdx.y * th, area = tw * th;
    s_h[t] = 0;
    if (t == 0) s_ex = 0;
    __syncthreads();
    for (int i = t; i < area; i += TK_NT) {                  // the padded tile through R: every read lies inside the image
        const int lx = i % tw, ly = i / tw;
        atomicAdd(&s_h[img[(size_t)tk_r(y0 + ly, H) * W + tk_r(x0 + lx, W)]], 1);      // integers: exact, so the order is free
    }
    __syncthreads();
    int hst = s_h[t];
    if (limit > 0) {
        const long long e = tk_wave_sum((long long)max(hst - limit, 0));
        if ((t & 63) == 0) atomicAdd(&s_ex, (int)e);
    }
    __syncthreads();
    if (limit > 0) {
        const int excess = s_ex, batch = excess / 256, residual = excess - 256 * batch;
        hst = min(hst, limit) + batch;
        if (residual > 0) { const int step = max(256 / residual, 1); hst += (t % step == 0 && t / step < residual) ? 1 : 0; }
    }
    s_h[t] = hst;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {                      // inclusive prefix sum of the 256 bins
        const int v = t >= o ? s_h[t - o] : 0;
        __syncthreads();
        s_h[t] += v;
        __syncthreads();
    }
    const float v = rintf(__fmul_rn((float)s_h[t], scale));
    lut[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 256 + t] = (unsigned char)fminf(fmaxf(v, 0.f), 255.f);
}

// ---- tk_clahe_remap -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TK_TW * TK_TH) void tk_clahe_remap(const unsigned char *img, int W, int H, int tx, int ty, float inv_tw, float inv_th, const unsigned char *lut, unsigned char *out) {
    const int x = blockIdx.x * TK_TW + threadIdx.x, y = blockIdx.y * TK_TH + threadIdx.y;
    if (x >= W || y >= H) return;
    const float txf = __fsub_rn(__fmul_rn((float)x, inv_tw), 0.5f), tyf = __fsub_rn(__fmul_rn((float)y, inv_th), 0.5f);
    const float fx1 = floorf(txf), fy1 = floorf(tyf);
    const float xa = __fsub_rn(txf, fx1), ya = __fsub_rn(tyf, fy1), nxa = __fsub_rn(1.f, xa), nya = __fsub_rn(1.f, ya);
    const int x1 = min(max((int)fx1, 0), tx - 1), x2 = min(max((int)fx1 + 1, 0), tx - 1), y1 = min(max((int)fy1, 0), ty - 1), y2 = min(max((int)fy1 + 1, 0), ty - 1);
    const size_t at = (size_t)y * W + x;
    const int v = img[at];
    const float l11 = (float)lut[((size_t)y1 * tx + x1) * 256 + v], l12 = (float)lut[((size_t)y1 * tx + x2) * 256 + v];
    const float l21 = (float)lut[((size_t)y2 * tx + x1) * 256 + v], l22 = (float)lut[((size_t)y2 * tx + x2) * 256 + v];
    const float top = __fadd_rn(__fmul_rn(l11, nxa), __fmul_rn(l12, xa)), bot = __fadd_rn(__fmul_rn(l21, nxa), __fmul_rn(l22, xa));
    const float r = rintf(__fadd_rn(__fmul_rn(top, nya), __fmul_rn(bot, ya)));
    out[at] = (unsigned char)fminf(fmaxf(r, 0.f), 255.f);
}

// ---- rejectWithF ------------------------------------------------------------------------------------------------------------------------------
namespace {
// the lift of rejectWithF: liftProjective in fp64, then the virtual camera's pixel, rounded to float32
VD float2 tk_f_liftpt(const TkCam &cam, float2 p, double focal, double half_w, double half_h) {
    double ux, uy;
    tk_undistort(cam, p, ux, uy);
    return make_float2((float)__dadd_rn(__dmul_rn(focal, ux), half_w), (float)__dadd_rn(__dmul_rn(focal, uy), half_h));
}
}  // namespace

// ---- tk_f_lift: one workgroup -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TK_NT) void tk_f_lift(const float2 *cur, const float2 *fwd, const unsigned char *status, const int *n_dev, int n_host, TkCam cam, double focal, double half_w, double half_h, TkF f) {
    __shared__ unsigned char s_st[TK_MAXN];
    const int t = threadIdx.x, n = min(n_dev ? *n_dev : n_host, TK_MAXN);
    for (int i = t; i < n; i += TK_NT) s_st[i] = status[i] ? 1 : 0;
    __syncthreads();
    for (int i = t; i < n; i += TK_NT) {
        if (!s_st[i]) continue;
        int rank = 0;
        for (int j = 0; j < i; j++) rank += s_st[j];         // list order; rank < n <= TK_MAXN, the rows of ua, ub, src
        f.ua[rank] = tk_f_liftpt(cam, cur[i], focal, half_w, half_h);
        f.ub[rank] = tk_f_liftpt(cam, fwd[i], focal, half_w, half_h);
        f.src[rank] = i;
    }
    if (t == 0) {
        int m = 0;
        for (int j = 0; j < n; j++) m += s_st[j];
        f.fctl[FC_M] = m;
        *(unsigned long long *)(f.fctl + FC_BEST) = 0ull;
    }
}

// ---- tk_f_hypotheses: a lane per hypothesis ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TK_F_LANES) void tk_f_hypotheses(TkF f, int K, unsigned seed) {
    __shared__ double s_M[45][TK_F_LANES], s_V[81][TK_F_LANES];          // 64 512 bytes: a column per lane, so a lane's accesses never meet another's
    const int lane = threadIdx.x, k = blockIdx.x * TK_F_LANES + lane, n = f.fctl[FC_M];
    if (n < 8 || k >= K) return;
    double F[9];
    const bool ok = tk_f_hypothesis(f.ua, f.ub, n, k, seed, s_M, s_V, lane, F);      // sample indices < n <= TK_MAXN, the rows of ua, ub
#pragma unroll
    for (int e = 0; e < 9; e++) f.F[(size_t)k * 9 + e] = F[e];      // k < K <= TK_F_MAXK rows
    f.valid[k] = ok ? 1 : 0;
}

// ---- tk_f_score: a wave per hypothesis --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * TK_F_WAVES) void tk_f_score(TkF f, int K, double thr2) {
    const int lane = threadIdx.x & 63, k = blockIdx.x * TK_F_WAVES + (threadIdx.x >> 6), n = f.fctl[FC_M];
    if (n < 8 || k >= K || !f.valid[k]) return;             // the whole wave
    double F[9];
#pragma unroll
    for (int e = 0; e < 9; e++) F[e] = f.F[(size_t)k * 9 + e];
    int cnt = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const bool in = i < n && tk_f_inlier(F, f.ua[i], f.ub[i], thr2);
        cnt += __popcll(__ballot(in));
    }
    if (lane == 0) atomicMax((unsigned long long *)(f.fctl + FC_BEST), ((unsigned long long)(cnt + 1) << 32) | (unsigned long long)(unsigned)(K - 1 - k));
}

// ---- tk_f_apply: one workgroup ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TK_NT) void tk_f_apply(TkF f, int K, double thr2, unsigned char *status) {
    const int t = threadIdx.x, n = min(f.fctl[FC_M], TK_MAXN);
    const unsigned long long word = *(const unsigned long long *)(f.fctl + FC_BEST);
    if (n < 8 || word == 0ull) {                             // nothing is rejected
        if (t < TK_F_RES) f.res[t] = t == 0 ? -1.0 : t == 1 ? (double)n : 0.0;
        return;
    }
    const int k = min(max(K - 1 - (int)(unsigned)(word & 0xffffffffull), 0), K - 1);
    double F[9];
#pragma unroll
    for (int e = 0; e < 9; e++) F[e] = f.F[(size_t)k * 9 + e];
    for (int i = t; i < n; i += TK_NT)
        if (!tk_f_inlier(F, f.ua[i], f.ub[i], thr2)) status[f.src[i]] = 0;      // src < the list's rows
    if (t == 0) { f.res[0] = (double)k; f.res[1] = (double)((long long)(word >> 32) - 1); }
    if (t < 9) f.res[2 + t] = F[t];
}

// ---- tk_mask_erode: a tile through LDS with a halo of r ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(TK_TW * TK_TH) void tk_mask_erode(const unsigned char *mask, int W, int H, TkSpans sp, unsigned char *E) {
    __shared__ unsigned char s[TK_TH + 2 * TK_ER_MAX][TK_TW + 2 * TK_ER_MAX];      // 1 = set; pixel (x0 - r + lx, y0 - r + ly)
    const int tx = threadIdx.x, ty = threadIdx.y, t = ty * TK_TW + tx;
    const int x0 = blockIdx.x * TK_TW, y0 = blockIdx.y * TK_TH;
    const int r = min(max(sp.r, 0), TK_ER_MAX), lw = TK_TW + 2 * r, lh = TK_TH + 2 * r;
    for (int i = t; i < lw * lh; i += TK_TW * TK_TH) {
        const int ly = i / lw, lx = i % lw, gx = x0 - r + lx, gy = y0 - r + ly;
        const bool in = (unsigned)gx < (unsigned)W && (unsigned)gy < (unsigned)H;
        const unsigned char v = mask[(size_t)min(max(gy, 0), H - 1) * W + min(max(gx, 0), W - 1)];      // clamped address, the value selected afterwards
        s[ly][lx] = (in && v == 0) ? 0 : 1;              // outside the image does not erode
    }
    __syncthreads();
    const int x = x0 + tx, y = y0 + ty;
    if (x >= W || y >= H) return;
    unsigned all = 1;
    for (int dy = -r; dy <= r; dy++) {
        const int hw = min(max(sp.hw[dy < 0 ? -dy : dy], 0), r);
        const unsigned char *row = &s[ty + r + dy][tx + r];      // rows ty .. ty + 2 r < lh, columns tx + r - hw .. tx + r + hw < lw
        for (int dx = -hw; dx <= hw; dx++) all &= row[dx];
    }
    E[(size_t)y * W + x] = all ? 255 : 0;
}

// ---- tk_mask_probe: a thread per point ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TK_NT) void tk_mask_probe(const unsigned char *E, const float2 *fwd, const unsigned char *status, const int *n_dev, int n_host, int W, int H, int d, unsigned char *is_static) {
    const int i = blockIdx.x * TK_NT + threadIdx.x, n = min(n_dev ? *n_dev : n_host, TK_MAXN);
    if (i >= n) return;
    const float2 f = fwd[i];
    const float rx = rintf(f.x), ry = rintf(f.y);
    const bool guard = rx > (float)d && ry > (float)d && rx < (float)(W - d) && ry < (float)(H - d);      // false for a NaN
    const int x = guard ? (int)rx : 0, y = guard ? (int)ry : 0;
    const int xl = min(max(x - d, 0), W - 1), xr = min(max(x + d, 0), W - 1), xc = min(max(x, 0), W - 1);
    const int yu = min(max(y - d, 0), H - 1), yd = min(max(y + d, 0), H - 1), yc = min(max(y, 0), H - 1);
    const unsigned char up = E[(size_t)yu * W + xc], dn = E[(size_t)yd * W + xc], lf = E[(size_t)yc * W + xl], rt = E[(size_t)yc * W + xr];
    const bool probe = !guard || (up != 0 && dn != 0 && lf != 0 && rt != 0);
    is_static[i] = ((status ? status[i] != 0 : true) && probe) ? 1 : 0;
}

// ---- tk_fm_apply: one workgroup ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TK_NT) void tk_fm_apply(TkF f, int K, const float2 *cur, const float2 *fwd, const int *n_dev, int n_host, TkCam cam, double focal, double half_w, double half_h, double epi,
                                                     unsigned char *status) {
    const int t = threadIdx.x, m = min(f.fctl[FC_M], TK_MAXN), n = min(n_dev ? *n_dev : n_host, TK_MAXN);
    const unsigned long long word = *(const unsigned long long *)(f.fctl + FC_BEST);
    if (m < 8 || word == 0ull) {                             // nothing is rejected
        if (t < TK_F_RES) f.res[t] = t == 0 ? -1.0 : t == 1 ? (double)m : 0.0;
        return;
    }
    const int k = min(max(K - 1 - (int)(unsigned)(word & 0xffffffffull), 0), K - 1);
    double F[9];
#pragma unroll
    for (int e = 0; e < 9; e++) F[e] = f.F[(size_t)k * 9 + e];
    for (int i = t; i < n; i += TK_NT) {
        if (!status[i]) continue;
        const float2 a = tk_f_liftpt(cam, cur[i], focal, half_w, half_h), b = tk_f_liftpt(cam, fwd[i], focal, half_w, half_h);
        const double x = (double)a.x, y = (double)a.y, xp = (double)b.x, yp = (double)b.y;
        const double A = __dadd_rn(__dadd_rn(__dmul_rn(F[0], x), __dmul_rn(F[1], y)), F[2]), B = __dadd_rn(__dadd_rn(__dmul_rn(F[3], x), __dmul_rn(F[4], y)), F[5]);
        const double Cc = __dadd_rn(__dadd_rn(__dmul_rn(F[6], x), __dmul_rn(F[7], y)), F[8]);
        const double dd = __ddiv_rn(fabs(__dadd_rn(__dadd_rn(__dmul_rn(A, xp), __dmul_rn(B, yp)), Cc)), __dsqrt_rn(__dadd_rn(__dmul_rn(A, A), __dmul_rn(B, B))));
        if (dd > epi) status[i] = 0;                         // one-sided; a NaN compares false and the point stays
    }
    if (t == 0) { f.res[0] = (double)k; f.res[1] = (double)((long long)(word >> 32) - 1); }
    if (t < 9) f.res[2 + t] = F[t];
}

// ---- tk_mask_init: forbidden = dynamic (E == 0) or outside the fisheye mask (== 0) ------------------------------------------------------------------------
__global__ __launch_bounds__(TK_NT) void tk_mask_init(const unsigned char *E, const unsigned char *fish, size_t n, unsigned char *mask) {
    const size_t at = ((size_t)blockIdx.x * TK_NT + threadIdx.x) * 4;
    if (at >= n) return;
    if (at + 4 <= n) {                                       // the buffers come from hipMalloc, so at is 4-byte aligned in all of them
        const unsigned e = E ? *(const unsigned *)(E + at) : 0xffffffffu, g = fish ? *(const unsigned *)(fish + at) : 0xffffffffu;
        unsigned out = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) out |= (((e >> (8 * b)) & 0xffu) == 0u || ((g >> (8 * b)) & 0xffu) == 0u) ? (1u << (8 * b)) : 0u;
        *(unsigned *)(mask + at) = out;
    } else {
        for (size_t i = at; i < n; i++) mask[i] = ((E && E[i] == 0) || (fish && fish[i] == 0)) ? 1 : 0;
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
namespace {
int tk_sort_bits(size_t cap) { int b = 1; while (((size_t)1 << b) <= cap) b++; return b; }      // the fill pattern (all ones) sorts behind every pixel index

// image (row stride in bytes) -> level 0 .. `levels` of a pyramid, on the stream. The rows go through the pyramid's pinned staging (every entry point ends with
// a wait for the stream, so the staging is free again): a copy from pageable memory, row by row, cost 2.6 ms per frame at 1226 x 370
int tk_upload(vilf_handle *h, const TkPyr &P, unsigned char *dst, unsigned char *stage, const unsigned char *img, int row_stride) {
    const size_t W = (size_t)P.w[0], H = (size_t)P.h[0];
    if ((size_t)row_stride == W) std::memcpy(stage, img, W * H);
    else for (size_t y = 0; y < H; y++) std::memcpy(stage + y * W, img + y * (size_t)row_stride, W);
    HIPCHECK(h, hipMemcpyAsync(dst, stage, W * H, hipMemcpyHostToDevice, h->stream));
    return VILF_OK;
}
int tk_levels(vilf_handle *h, TkPyr &P, int levels) {
    for (int L = 1; L <= levels; L++)
        hipLaunchKernelGGL(tk_pyr_down, dim3((P.w[L] + TK_TW - 1) / TK_TW, (P.h[L] + TK_TH - 1) / TK_TH), dim3(TK_TW, TK_TH), 0, h->stream, P.lv[L - 1], P.w[L - 1], P.h[L - 1], P.lv[L], P.w[L], P.h[L]);
    HIPCHECK(h, hipGetLastError());
    return VILF_OK;
}
int tk_build(vilf_handle *h, TkPyr &P, unsigned char *stage, const unsigned char *img, int row_stride, int levels) {
    const int rc = tk_upload(h, P, P.lv[0], stage, img, row_stride);
    return rc != VILF_OK ? rc : tk_levels(h, P, levels);
}
// CLAHE of the W x H image at src -> dst (both on the device, rows tight) with the configured clip and tiles; the geometry and the integer limit of the text
int tk_clahe(vilf_handle *h, TrackCtx *c, const unsigned char *src, unsigned char *dst) {
    const int W = c->p.width, H = c->p.height, tx = c->fe.clahe_tiles_x, ty = c->fe.clahe_tiles_y;
    const bool fits = W % tx == 0 && H % ty == 0;
    const int Wp = fits ? W : W + (tx - W % tx), Hp = fits ? H : H + (ty - H % ty), tw = Wp / tx, th = Hp / ty, area = tw * th;      // area <= 4 W H <= 2^30
    const int limit = c->fe.clahe_clip > 0 ? std::max(1, (int)((c->fe.clahe_clip * (double)area) / 256.0)) : 0;
    hipLaunchKernelGGL(tk_clahe_lut, dim3(tx, ty), dim3(TK_NT), 0, h->stream, src, W, H, tw, th, limit, 255.f / (float)area, c->lut.as<unsigned char>());
    hipLaunchKernelGGL(tk_clahe_remap, dim3((W + TK_TW - 1) / TK_TW, (H + TK_TH - 1) / TK_TH), dim3(TK_TW, TK_TH), 0, h->stream, src, W, H, tx, ty, 1.f / (float)tw, 1.f / (float)th,
                       c->lut.as<unsigned char>(), dst);
    HIPCHECK(h, hipGetLastError());
    return VILF_OK;
}
// the arrays of rejectWithF inside fmem
enum : size_t { TKF_UA = 0, TKF_UB = TKF_UA + TK_MAXN * 8, TKF_SRC = TKF_UB + TK_MAXN * 8, TKF_CTL = TKF_SRC + TK_MAXN * 4, TKF_F = TKF_CTL + 64,
                TKF_VALID = TKF_F + (size_t)TK_F_MAXK * 72, TKF_RES = TKF_VALID + (size_t)TK_F_MAXK * 4, TKF_BYTES = TKF_RES + TK_F_RES * 8 };
static_assert(TKF_CTL % 8 == 0 && TKF_F % 8 == 0 && TKF_RES % 8 == 0, "the 64-bit words of fmem are aligned");
TkF tk_f(TrackCtx *c) {
    char *b = c->fmem.as<char>();
    TkF f;
    f.ua = (float2 *)(b + TKF_UA); f.ub = (float2 *)(b + TKF_UB); f.src = (int *)(b + TKF_SRC); f.fctl = (int *)(b + TKF_CTL);
    f.F = (double *)(b + TKF_F); f.valid = (int *)(b + TKF_VALID); f.res = (double *)(b + TKF_RES);
    return f;
}
TkCam tk_cam(const vilf_track_params &p) { return ::tk_cam(p.fx, p.fy, p.cx, p.cy, p.k1, p.k2, p.p1, p.p2); }
// rejectWithF on the pairs (cur[i], fwd[i]) whose status is set (the count on the device, or n_host): the outliers' status bytes are cleared. Fixed grids; the
// kernels read the survivors' count themselves and leave at once when it is below 8
int tk_reject(vilf_handle *h, TrackCtx *c, const float2 *cur, const float2 *fwd, unsigned char *status, const int *n_dev, int n_host) {
    const TkF f = tk_f(c);
    const int K = c->fe.n_hypotheses;
    const double thr2 = c->fe.f_threshold * c->fe.f_threshold;
    hipLaunchKernelGGL(tk_f_lift, dim3(1), dim3(TK_NT), 0, h->stream, cur, fwd, status, n_dev, n_host, tk_cam(c->p), c->fe.focal_length, c->p.width / 2.0, c->p.height / 2.0, f);
    hipLaunchKernelGGL(tk_f_hypotheses, dim3((K + TK_F_LANES - 1) / TK_F_LANES), dim3(TK_F_LANES), 0, h->stream, f, K, c->fe.seed);
    hipLaunchKernelGGL(tk_f_score, dim3((K + TK_F_WAVES - 1) / TK_F_WAVES), dim3(64 * TK_F_WAVES), 0, h->stream, f, K, thr2);
    hipLaunchKernelGGL(tk_f_apply, dim3(1), dim3(TK_NT), 0, h->stream, f, K, thr2, status);
    HIPCHECK(h, hipGetLastError());
    return VILF_OK;
}
// a W x H byte image (a mask) -> dst on the device, through the pinned mask staging, on the stream
int tk_upload_mask(vilf_handle *h, TrackCtx *c, unsigned char *dst, const unsigned char *src, int row_stride) {
    const size_t W = (size_t)c->p.width, H = (size_t)c->p.height;
    unsigned char *stage = (unsigned char *)c->mstage.p;
    if ((size_t)row_stride == W) std::memcpy(stage, src, W * H);
    else for (size_t y = 0; y < H; y++) std::memcpy(stage + y * W, src + y * (size_t)row_stride, W);
    HIPCHECK(h, hipMemcpyAsync(dst, stage, W * H, hipMemcpyHostToDevice, h->stream));
    return VILF_OK;
}
// the erosion of the text: mask -> E (both on the device, rows tight) with the configured radius
int tk_erode(vilf_handle *h, TrackCtx *c, const unsigned char *mask, unsigned char *E) {
    const int W = c->p.width, H = c->p.height, r = c->mp.erode_radius;
    TkSpans sp;
    std::memset(&sp, 0, sizeof(sp));
    sp.r = r;
    for (int d = 0; d <= r; d++) sp.hw[d] = (int)std::nearbyint(std::sqrt((double)(r * r - d * d)));      // round-half-to-even, the default rounding mode
    hipLaunchKernelGGL(tk_mask_erode, dim3((W + TK_TW - 1) / TK_TW, (H + TK_TH - 1) / TK_TH), dim3(TK_TW, TK_TH), 0, h->stream, mask, W, H, sp, E);
    HIPCHECK(h, hipGetLastError());
    return VILF_OK;
}
// rejectWithF_mask: the search of rejectWithF on the pairs flagged in is_static (the mask parameters' threshold; K, seed and focal length as configured), then every
// pair whose status is set is tested against the winner. Fixed grids, the counts are read on the device
int tk_reject_mask(vilf_handle *h, TrackCtx *c, const float2 *cur, const float2 *fwd, const unsigned char *is_static, unsigned char *status, const int *n_dev, int n_host) {
    const TkF f = tk_f(c);
    const int K = c->fe.n_hypotheses;
    const double thr2 = c->mp.f_threshold * c->mp.f_threshold, hw = c->p.width / 2.0, hh = c->p.height / 2.0;
    const TkCam cam = tk_cam(c->p);
    hipLaunchKernelGGL(tk_f_lift, dim3(1), dim3(TK_NT), 0, h->stream, cur, fwd, is_static, n_dev, n_host, cam, c->fe.focal_length, hw, hh, f);
    hipLaunchKernelGGL(tk_f_hypotheses, dim3((K + TK_F_LANES - 1) / TK_F_LANES), dim3(TK_F_LANES), 0, h->stream, f, K, c->fe.seed);
    hipLaunchKernelGGL(tk_f_score, dim3((K + TK_F_WAVES - 1) / TK_F_WAVES), dim3(64 * TK_F_WAVES), 0, h->stream, f, K, thr2);
    hipLaunchKernelGGL(tk_fm_apply, dim3(1), dim3(TK_NT), 0, h->stream, f, K, cur, fwd, n_dev, n_host, cam, c->fe.focal_length, hw, hh, c->mp.epi_threshold, status);
    HIPCHECK(h, hipGetLastError());
    return VILF_OK;
}
vilf_track_mask_params tk_mp_defaults() {
    vilf_track_mask_params mp;
    std::memset(&mp, 0, sizeof(mp));
    mp.erode_radius = 5; mp.probe = 5; mp.reject = 1; mp.f_threshold = 0.1; mp.epi_threshold = 1.0;
    return mp;
}
vilf_track_frontend tk_fe_defaults() {
    vilf_track_frontend fe;
    std::memset(&fe, 0, sizeof(fe));
    fe.clahe_clip = 3.0; fe.clahe_tiles_x = 8; fe.clahe_tiles_y = 8; fe.f_threshold = 1.0; fe.focal_length = 460.0; fe.n_hypotheses = 512;
    return fe;
}
// mask, response, candidates, the two sorts, the greedy acceptance: ctl holds kept / n_max / candidate count 0 / lambda max 0, l.pts the kept points. E: the eroded
// dynamic mask (device) or null; the fisheye mask is the tracker's. With neither the forbidden-pixel map starts from a memset, as it always did
int tk_detect(vilf_handle *h, TrackCtx *c, const unsigned char *img, const unsigned char *E, int *ctl, TkList l, int list_cap) {
    const int W = c->p.width, H = c->p.height, cap = (int)c->ncell;
    const long long md = c->p.min_dist, md2 = md * md;
    const unsigned char *fish = c->has_fish ? c->fish.as<unsigned char>() : nullptr;
    if (E || fish) hipLaunchKernelGGL(tk_mask_init, dim3((unsigned)((c->ncell + 4 * TK_NT - 1) / (4 * TK_NT))), dim3(TK_NT), 0, h->stream, E, fish, c->ncell, c->mask.as<unsigned char>());
    else HIPCHECK(h, hipMemsetAsync(c->mask.p, 0, c->ncell, h->stream));
    HIPCHECK(h, hipMemsetAsync(c->cidx.p, 0xff, c->ncell * 4, h->stream));
    hipLaunchKernelGGL(tk_paint, dim3(list_cap), dim3(TK_NT), 0, h->stream, l.pts, ctl, c->mask.as<unsigned char>(), W, H, md, md2);
    hipLaunchKernelGGL(tk_response, dim3((W + TK_TW - 1) / TK_TW, (H + TK_TH - 1) / TK_TH), dim3(TK_TW, TK_TH), 0, h->stream, img, c->mask.as<unsigned char>(), W, H, ctl, c->lam.as<double>());
    const unsigned nb = (unsigned)((c->ncell + TK_NT - 1) / TK_NT);
    hipLaunchKernelGGL(tk_candidates, dim3(nb), dim3(TK_NT), 0, h->stream, c->lam.as<double>(), c->mask.as<unsigned char>(), W, H, ctl, c->cidx.as<unsigned>(), cap);
    HIPCHECK(h, hipGetLastError());
    if (vilf_sort_pairs_u32(h->stream, c->temp.p, c->temp.cap, c->cidx.as<unsigned>(), c->cidx2.as<unsigned>(), c->cidx.as<int>(), c->cval.as<int>(), c->ncell, tk_sort_bits(c->ncell)) != 0) {
        h->err = "feature tracker: radix sort failed"; return VILF_ERR_DEVICE;
    }
    hipLaunchKernelGGL(tk_keys, dim3(nb), dim3(TK_NT), 0, h->stream, c->lam.as<double>(), c->cidx2.as<unsigned>(), ctl, cap, c->key.as<unsigned long long>(), c->val.as<int>());
    if (vilf_sort_pairs_u64(h->stream, c->temp.p, c->temp.cap, c->key.as<unsigned long long>(), c->key2.as<unsigned long long>(), c->val.as<int>(), c->val2.as<int>(), c->ncell, 64) != 0) {
        h->err = "feature tracker: radix sort failed"; return VILF_ERR_DEVICE;
    }
    hipLaunchKernelGGL(tk_corners, dim3(1), dim3(TK_CORNERS_NT), 0, h->stream, c->val2.as<int>(), W, cap, ctl, l, md2);
    HIPCHECK(h, hipGetLastError());
    return VILF_OK;
}
TrackCtx *tk_ctx(vilf_handle *h, const char *who) {
    TrackCtx *c = vilf_stage<TrackCtx>(h, ST_TRACK);
    if (!c) h->err = std::string(who) + ": no tracker (vilf_track_init)";
    return c;
}
}  // namespace

extern "C" int vilf_track_init(vilf_handle *h, const vilf_track_params *p) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    if (!p) { h->err = "vilf_track_init: null parameters"; return VILF_ERR_INVALID_ARGUMENT; }
    if (p->width <= TK_WIN || p->height <= TK_WIN || p->max_cnt < 1 || p->max_cnt > VILF_MAX_FEATURES || p->min_dist < 1 || !(p->fx > 0) || !(p->fy > 0) ||
        !std::isfinite(p->fx) || !std::isfinite(p->fy) || !std::isfinite(p->cx) || !std::isfinite(p->cy) || !std::isfinite(p->k1) || !std::isfinite(p->k2) || !std::isfinite(p->p1) || !std::isfinite(p->p2)) {
        h->err = "vilf_track_init: both sides > 21, 1 <= max_cnt <= VILF_MAX_FEATURES, min_dist >= 1, positive focal lengths, finite camera parameters";
        return VILF_ERR_INVALID_ARGUMENT;
    }
    if ((long long)p->width * p->height > (1ll << 28)) { h->err = "vilf_track_init: more than 2^28 pixels"; return VILF_ERR_UNSUPPORTED; }
    HIPCHECK(h, hipSetDevice(h->device));
    HIPCHECK(h, hipStreamSynchronize(h->stream));
    vilf_stage_drop(h, ST_TRACK);
    TrackCtx *c = new TrackCtx();
    c->p = *p;
    c->fe = tk_fe_defaults();
    c->mp = tk_mp_defaults();
    c->ncell = (size_t)p->width * p->height;
    bool ok = true;
    for (int k = 0; k < 4 && ok; k++) {
        TkPyr &P = c->pyr[k];
        int w = p->width, hh = p->height;
        size_t total = 0, off[TK_LEVELS];
        P.lmax = 0;
        for (int L = 0; L < TK_LEVELS; L++) {
            if (L > 0) { w = (w + 1) / 2; hh = (hh + 1) / 2; if (P.lmax == L - 1 && w > TK_WIN && hh > TK_WIN) P.lmax = L; }
            P.w[L] = w; P.h[L] = hh; off[L] = total; total += ((size_t)w * hh + 255) / 256 * 256;
        }
        ok = c->pyrmem[k].ensure(total) && c->stage[k].ensure(c->ncell);
        for (int L = 0; L < TK_LEVELS && ok; L++) P.lv[L] = c->pyrmem[k].as<unsigned char>() + off[L];
    }
    const size_t n = c->ncell;
    // the candidate buffers hold W * H entries. W * H / 4 + 1 would do if two neighbouring 3 x 3 maxima had to differ, but equal neighbours are both maxima: a
    // texture of period 3 in x and y has the same lambda > 0 at every inner pixel, and all of them are candidates. A buffer of one entry per pixel cannot overflow.
    ok = ok && c->list[0].ensure(tk_list_bytes(TK_MAXN)) && c->list[1].ensure(tk_list_bytes(TK_MAXN)) && c->tmplist.ensure(tk_list_bytes(2 * TK_MAXN)) && c->ctl.ensure(TC_INTS * 4) &&
         c->tmpctl.ensure(TC_INTS * 4) && c->prev_ids.ensure(TK_MAXN * 4) && c->prev_un.ensure(TK_MAXN * 8) && c->fwd.ensure(TK_MAXN * 8) && c->status.ensure(TK_MAXN) &&
         c->lkpts.ensure(TK_MAXN * 8) && c->mask.ensure(n) && c->lam.ensure(n * 8) && c->cidx.ensure(n * 4) && c->cidx2.ensure(n * 4) && c->cval.ensure(n * 4) && c->key.ensure(n * 8) &&
         c->key2.ensure(n * 8) && c->val.ensure(n * 4) && c->val2.ensure(n * 4) && c->temp.ensure(std::max(vilf_sort_temp_bytes(n, 8), vilf_sort_temp_bytes(n, 4)) + 256) &&
         c->pin.ensure(tk_list_bytes(TK_MAXN)) && c->raw.ensure(n) && c->lut.ensure((size_t)VILF_TRACK_MAX_TILES * 256) && c->fmem.ensure(TKF_BYTES) &&
         c->mraw.ensure(n) && c->er.ensure(n) && c->fish.ensure(n) && c->sstatus.ensure(TK_MAXN) && c->mstage.ensure(n);
    if (!ok) { delete c; h->err = "hipMalloc failed (feature tracker)"; return VILF_ERR_DEVICE; }
    h->stage[ST_TRACK] = c;
    return vilf_track_reset(h);
}

extern "C" int vilf_track_reset(vilf_handle *h) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    TrackCtx *c = tk_ctx(h, "vilf_track_reset");
    if (!c) return VILF_ERR_INVALID_ARGUMENT;
    HIPCHECK(h, hipSetDevice(h->device));
    HIPCHECK(h, hipMemsetAsync(c->ctl.p, 0, TC_INTS * 4, h->stream));
    HIPCHECK(h, hipMemsetAsync(c->list[0].p, 0, TK_LIST_HDR * 4, h->stream));
    HIPCHECK(h, hipMemsetAsync(c->list[1].p, 0, TK_LIST_HDR * 4, h->stream));
    HIPCHECK(h, hipStreamSynchronize(h->stream));
    c->frames = 0; c->n_host = 0; c->t_prev = 0; c->cur = 0; c->lcur = 0;
    return VILF_OK;
}

namespace {
// one frame of readImage (mask == null) or readImage_mask: the arguments are checked by the two entry points
int tk_frame(vilf_handle *h, TrackCtx *c, const unsigned char *img, int row_stride, const unsigned char *mask, int mask_row_stride, double stamp, int *n_out) {
    HIPCHECK(h, hipSetDevice(h->device));
    if (h->profiling) c->profile_reset();                   // the stages of the last frame
    const bool eq = c->fe.equalize != 0, rej = !mask && c->fe.reject_f != 0 && c->frames > 0, trk = mask && c->frames > 0;      // the masked entry point has its own rejection
    TkPyr &cur = c->pyr[c->cur], &nxt = c->pyr[c->cur ^ 1];
    TkList lc = tk_list(c->list[c->lcur].p, TK_MAXN), ln = tk_list(c->list[c->lcur ^ 1].p, TK_MAXN);
    int *ctl = c->ctl.as<int>();
    const long long md = c->p.min_dist;
    ProfMarks prof(h, c->prof);
    if (eq) {                                                // the raw image into its own buffer, the equalised one straight into level 0
        { const int rc = tk_upload(h, nxt, c->raw.as<unsigned char>(), (unsigned char *)c->stage[c->cur ^ 1].p, img, row_stride); if (rc != VILF_OK) return rc; }
        if (mask) { const int rc = tk_upload_mask(h, c, c->mraw.as<unsigned char>(), mask, mask_row_stride); if (rc != VILF_OK) return rc; }
        ProfMarks fe(h, c->fe_prof);
        { const int rc = tk_clahe(h, c, c->raw.as<unsigned char>(), nxt.lv[0]); if (rc != VILF_OK) return rc; }
        fe.mark(0);
        { const int rc = tk_levels(h, nxt, nxt.lmax); if (rc != VILF_OK) return rc; }
    } else if (mask) {                                       // both uploads in front of the kernels
        { const int rc = tk_upload(h, nxt, nxt.lv[0], (unsigned char *)c->stage[c->cur ^ 1].p, img, row_stride); if (rc != VILF_OK) return rc; }
        { const int rc = tk_upload_mask(h, c, c->mraw.as<unsigned char>(), mask, mask_row_stride); if (rc != VILF_OK) return rc; }
        { const int rc = tk_levels(h, nxt, nxt.lmax); if (rc != VILF_OK) return rc; }
    } else { const int rc = tk_build(h, nxt, (unsigned char *)c->stage[c->cur ^ 1].p, img, row_stride, nxt.lmax); if (rc != VILF_OK) return rc; }
    if (mask) {                                              // E serves the probe and the detection, so it is made on the first frame too
        ProfMarks mk(h, c->mk_prof);
        { const int rc = tk_erode(h, c, c->mraw.as<unsigned char>(), c->er.as<unsigned char>()); if (rc != VILF_OK) return rc; }
        mk.mark(0);
    }
    prof.mark(0);
    if (c->frames > 0)
        hipLaunchKernelGGL(tk_lk, dim3((c->p.max_cnt + TK_LK_WAVES - 1) / TK_LK_WAVES), dim3(64 * TK_LK_WAVES), 0, h->stream, cur, nxt, lc.pts, ctl + TC_N, 0, c->fwd.as<float2>(), c->status.as<unsigned char>(), 1);
    if (rej) {                                               // between the inBorder drop (LK's status) and setMask, which reads the same status bytes
        ProfMarks fe(h, c->fe_prof);
        { const int rc = tk_reject(h, c, lc.pts, c->fwd.as<float2>(), c->status.as<unsigned char>(), ctl + TC_N, 0); if (rc != VILF_OK) return rc; }
        fe.mark(1);
    }
    if (trk) {                                               // probe -> the static status; the rejection clears LK's status bytes, which tk_setmask reads
        ProfMarks mk(h, c->mk_prof);
        hipLaunchKernelGGL(tk_mask_probe, dim3((c->p.max_cnt + TK_NT - 1) / TK_NT), dim3(TK_NT), 0, h->stream, c->er.as<unsigned char>(), c->fwd.as<float2>(), c->status.as<unsigned char>(), ctl + TC_N, 0,
                           c->p.width, c->p.height, c->mp.probe, c->sstatus.as<unsigned char>());
        if (c->mp.reject) { const int rc = tk_reject_mask(h, c, lc.pts, c->fwd.as<float2>(), c->sstatus.as<unsigned char>(), c->status.as<unsigned char>(), ctl + TC_N, 0); if (rc != VILF_OK) return rc; }
        mk.mark(1);
    }
    prof.mark(1);
    hipLaunchKernelGGL(tk_setmask, dim3(1), dim3(TK_NT), 0, h->stream, lc, c->fwd.as<float2>(), c->status.as<unsigned char>(), ln, ctl, c->p.max_cnt, md * md,
                       c->has_fish ? c->fish.as<unsigned char>() : (const unsigned char *)nullptr, c->p.width, c->p.height);
    HIPCHECK(h, hipGetLastError());
    prof.mark(2);
    { const int rc = tk_detect(h, c, nxt.lv[0], mask ? c->er.as<unsigned char>() : nullptr, ctl, ln, c->p.max_cnt); if (rc != VILF_OK) return rc; }
    prof.mark(3);
    hipLaunchKernelGGL(tk_finish, dim3(1), dim3(TK_NT), 0, h->stream, ln, ctl, c->prev_ids.as<int>(), c->prev_un.as<float2>(), tk_cam(c->p), stamp - c->t_prev, c->frames > 0 ? 1 : 0);
    HIPCHECK(h, hipGetLastError());
    prof.mark(4);
    HIPCHECK(h, vilf_copy_sync(h, c->pin.p, ln.hdr, tk_list_bytes(TK_MAXN), hipMemcpyDeviceToHost));
    if (h->profiling) { const int rcf = vilf_prof_flush(h); if (rcf != VILF_OK) return rcf; }
    c->cur ^= 1; c->lcur ^= 1; c->frames++; c->t_prev = stamp;
    c->n_host = std::min(std::max(((const int *)c->pin.p)[0], 0), c->p.max_cnt);
    if (n_out) *n_out = c->n_host;
    return VILF_OK;
}
}  // namespace

extern "C" int vilf_track_read_image(vilf_handle *h, const unsigned char *img, int row_stride, double stamp, int *n_out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    TrackCtx *c = tk_ctx(h, "vilf_track_read_image");
    if (!c) return VILF_ERR_INVALID_ARGUMENT;
    if (!img || row_stride < c->p.width) { h->err = "vilf_track_read_image: null image or row_stride < width"; return VILF_ERR_INVALID_ARGUMENT; }
    return tk_frame(h, c, img, row_stride, nullptr, 0, stamp, n_out);
}

extern "C" int vilf_track_read_image_mask(vilf_handle *h, const unsigned char *img, int row_stride, const unsigned char *mask, int mask_row_stride, double stamp, int *n_out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    TrackCtx *c = tk_ctx(h, "vilf_track_read_image_mask");
    if (!c) return VILF_ERR_INVALID_ARGUMENT;
    if (!img || !mask || row_stride < c->p.width || mask_row_stride < c->p.width) { h->err = "vilf_track_read_image_mask: null image or mask, or a row stride < width"; return VILF_ERR_INVALID_ARGUMENT; }
    return tk_frame(h, c, img, row_stride, mask, mask_row_stride, stamp, n_out);
}

extern "C" int vilf_track_get(vilf_handle *h, int cap, int *ids, int *track_cnt, float *cur_pts, float *un_pts, float *velocity, int *n_out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    TrackCtx *c = tk_ctx(h, "vilf_track_get");
    if (!c) return VILF_ERR_INVALID_ARGUMENT;
    const int n = c->n_host;
    if (cap < n) { h->err = "vilf_track_get: the list holds " + std::to_string(n) + " rows, cap is " + std::to_string(cap); return VILF_ERR_INVALID_ARGUMENT; }
    const TkList l = tk_list(c->pin.p, TK_MAXN);          // the host copy of the last frame's list
    if (ids) std::memcpy(ids, l.ids, (size_t)n * 4);
    if (track_cnt) std::memcpy(track_cnt, l.cnt, (size_t)n * 4);
    if (cur_pts) std::memcpy(cur_pts, l.pts, (size_t)n * 8);
    if (un_pts) std::memcpy(un_pts, l.un, (size_t)n * 8);
    if (velocity) std::memcpy(velocity, l.vel, (size_t)n * 8);
    if (n_out) *n_out = n;
    return VILF_OK;
}

extern "C" int vilf_track_pyramid(vilf_handle *h, const unsigned char *img, int row_stride, int level, unsigned char *out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    TrackCtx *c = tk_ctx(h, "vilf_track_pyramid");
    if (!c) return VILF_ERR_INVALID_ARGUMENT;
    TkPyr &P = c->pyr[2];
    if (!img || !out || row_stride < c->p.width || level < 0 || level > P.lmax) { h->err = "vilf_track_pyramid: null pointer, row_stride < width or a level outside 0 .. Lmax"; return VILF_ERR_INVALID_ARGUMENT; }
    HIPCHECK(h, hipSetDevice(h->device));
    { const int rc = tk_build(h, P, (unsigned char *)c->stage[2].p, img, row_stride, level); if (rc != VILF_OK) return rc; }
    HIPCHECK(h, vilf_copy_sync(h, out, P.lv[level], (size_t)P.w[level] * P.h[level], hipMemcpyDeviceToHost));
    return VILF_OK;
}

extern "C" int vilf_track_lk(vilf_handle *h, const unsigned char *img_prev, const unsigned char *img_next, const float *pts, int n, float *pts_out, unsigned char *status_out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    TrackCtx *c = tk_ctx(h, "vilf_track_lk");
    if (!c) return VILF_ERR_INVALID_ARGUMENT;
    if (!img_prev || !img_next || n < 0 || (n > 0 && (!pts || !pts_out || !status_out))) { h->err = "vilf_track_lk: null pointer or negative count"; return VILF_ERR_INVALID_ARGUMENT; }
    if (n == 0) return VILF_OK;
    HIPCHECK(h, hipSetDevice(h->device));
    const size_t sn = (size_t)std::max(n, TK_MAXN);
    if (sn * 8 > c->lkpts.cap || sn * 8 > c->fwd.cap || sn > c->status.cap) HIPCHECK(h, hipStreamSynchronize(h->stream));      // a buffer is about to be replaced
    if (!c->lkpts.ensure(sn * 8) || !c->fwd.ensure(sn * 8) || !c->status.ensure(sn)) { h->err = "hipMalloc failed (feature tracker, points)"; return VILF_ERR_DEVICE; }
    TkPyr &A = c->pyr[2], &B = c->pyr[3];
    { const int rc = tk_build(h, A, (unsigned char *)c->stage[2].p, img_prev, A.w[0], A.lmax); if (rc != VILF_OK) return rc; }
    { const int rc = tk_build(h, B, (unsigned char *)c->stage[3].p, img_next, B.w[0], B.lmax); if (rc != VILF_OK) return rc; }
    HIPCHECK(h, hipMemcpyAsync(c->lkpts.p, pts, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(tk_lk, dim3((n + TK_LK_WAVES - 1) / TK_LK_WAVES), dim3(64 * TK_LK_WAVES), 0, h->stream, A, B, c->lkpts.as<float2>(), (const int *)nullptr, n, c->fwd.as<float2>(), c->status.as<unsigned char>(), 0);
    HIPCHECK(h, hipGetLastError());
    HIPCHECK(h, hipMemcpyAsync(pts_out, c->fwd.p, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(h, vilf_copy_sync(h, status_out, c->status.p, (size_t)n, hipMemcpyDeviceToHost));
    return VILF_OK;
}

namespace {
// vilf_track_detect (eroded == null) and vilf_track_detect_masked
int tk_detect_call(vilf_handle *h, const char *who, const unsigned char *img, const unsigned char *eroded, bool masked, const float *kept_pts, int n_kept, int n_max, float *pts_out, int *n_out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    TrackCtx *c = tk_ctx(h, who);
    if (!c) return VILF_ERR_INVALID_ARGUMENT;
    if (!img || (masked && !eroded) || !n_out || n_kept < 0 || n_kept > TK_MAXN || (n_kept > 0 && !kept_pts) || n_max > TK_MAXN || (n_max > 0 && !pts_out)) {
        h->err = std::string(who) + ": null pointer, or more than VILF_MAX_FEATURES kept points or new corners"; return VILF_ERR_INVALID_ARGUMENT;
    }
    for (int i = 0; i < 2 * n_kept; i++)
        if (!(std::fabs(kept_pts[i]) <= 1.0e6f)) { h->err = std::string(who) + ": a kept point that is not finite or beyond 1e6 pixels"; return VILF_ERR_INVALID_ARGUMENT; }
    *n_out = 0;
    if (n_max <= 0) return VILF_OK;
    HIPCHECK(h, hipSetDevice(h->device));
    TkPyr &P = c->pyr[2];
    TkList l = tk_list(c->tmplist.p, 2 * TK_MAXN);
    int ctl[TC_INTS];
    std::memset(ctl, 0, sizeof(ctl));
    ctl[TC_N] = n_kept; ctl[TC_KEPT] = n_kept; ctl[TC_NMAX] = n_max;
    HIPCHECK(h, hipMemcpyAsync(c->tmpctl.p, ctl, sizeof(ctl), hipMemcpyHostToDevice, h->stream));
    if (n_kept > 0) HIPCHECK(h, hipMemcpyAsync(l.pts, kept_pts, (size_t)n_kept * 8, hipMemcpyHostToDevice, h->stream));
    { const int rc = tk_build(h, P, (unsigned char *)c->stage[2].p, img, P.w[0], 0); if (rc != VILF_OK) return rc; }
    if (eroded) { const int rc = tk_upload_mask(h, c, c->er.as<unsigned char>(), eroded, c->p.width); if (rc != VILF_OK) return rc; }      // E is scratch of a single call
    { const int rc = tk_detect(h, c, P.lv[0], eroded ? c->er.as<unsigned char>() : nullptr, c->tmpctl.as<int>(), l, std::max(n_kept, 1)); if (rc != VILF_OK) return rc; }
    HIPCHECK(h, vilf_copy_sync(h, ctl, c->tmpctl.p, sizeof(ctl), hipMemcpyDeviceToHost));
    const int n_new = std::min(std::max(ctl[TC_N] - n_kept, 0), n_max);
    if (n_new > 0) HIPCHECK(h, vilf_copy_sync(h, pts_out, l.pts + n_kept, (size_t)n_new * 8, hipMemcpyDeviceToHost));
    *n_out = n_new;
    return VILF_OK;
}
}  // namespace

extern "C" int vilf_track_detect(vilf_handle *h, const unsigned char *img, const float *kept_pts, int n_kept, int n_max, float *pts_out, int *n_out) {
    return tk_detect_call(h, "vilf_track_detect", img, nullptr, false, kept_pts, n_kept, n_max, pts_out, n_out);
}

extern "C" int vilf_track_detect_masked(vilf_handle *h, const unsigned char *img, const unsigned char *eroded, const float *kept_pts, int n_kept, int n_max, float *pts_out, int *n_out) {
    return tk_detect_call(h, "vilf_track_detect_masked", img, eroded, true, kept_pts, n_kept, n_max, pts_out, n_out);
}

extern "C" int vilf_track_profile(vilf_handle *h, double ms_out[5], long launches_out[5]) { return vilf_stage_profile(h, ST_TRACK, &TrackCtx::prof, ms_out, launches_out); }

extern "C" int vilf_track_configure(vilf_handle *h, const vilf_track_frontend *fe) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    TrackCtx *c = tk_ctx(h, "vilf_track_configure");
    if (!c) return VILF_ERR_INVALID_ARGUMENT;
    if (!fe) { h->err = "vilf_track_configure: null parameters"; return VILF_ERR_INVALID_ARGUMENT; }
    if (fe->clahe_tiles_x < 1 || fe->clahe_tiles_y < 1 || (long long)fe->clahe_tiles_x * fe->clahe_tiles_y > VILF_TRACK_MAX_TILES || !std::isfinite(fe->clahe_clip) || fe->clahe_clip < 0 ||
        !std::isfinite(fe->f_threshold) || !(fe->f_threshold > 0) || !std::isfinite(fe->focal_length) || !(fe->focal_length > 0) || fe->n_hypotheses < 1 ||
        fe->n_hypotheses > VILF_TRACK_MAX_HYPOTHESES) {
        h->err = "vilf_track_configure: 1 <= tiles, tiles_x * tiles_y <= VILF_TRACK_MAX_TILES, a finite clip >= 0, a positive finite threshold and focal length, 1 <= n_hypotheses <= VILF_TRACK_MAX_HYPOTHESES";
        return VILF_ERR_INVALID_ARGUMENT;
    }
    c->fe = *fe;
    return VILF_OK;
}

extern "C" int vilf_track_clahe(vilf_handle *h, const unsigned char *img, int row_stride, unsigned char *out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    TrackCtx *c = tk_ctx(h, "vilf_track_clahe");
    if (!c) return VILF_ERR_INVALID_ARGUMENT;
    if (!img || !out || row_stride < c->p.width) { h->err = "vilf_track_clahe: null pointer or row_stride < width"; return VILF_ERR_INVALID_ARGUMENT; }
    HIPCHECK(h, hipSetDevice(h->device));
    TkPyr &A = c->pyr[2], &B = c->pyr[3];                     // the stateless calls' pyramids: the image into level 0 of one, the result into level 0 of the other
    { const int rc = tk_upload(h, A, A.lv[0], (unsigned char *)c->stage[2].p, img, row_stride); if (rc != VILF_OK) return rc; }
    { const int rc = tk_clahe(h, c, A.lv[0], B.lv[0]); if (rc != VILF_OK) return rc; }
    HIPCHECK(h, vilf_copy_sync(h, out, B.lv[0], c->ncell, hipMemcpyDeviceToHost));
    return VILF_OK;
}

extern "C" int vilf_track_reject_f(vilf_handle *h, const float *cur_pts, const float *forw_pts, int n, unsigned char *status_out, double F_out[9], int *best_out, int *n_inliers_out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    TrackCtx *c = tk_ctx(h, "vilf_track_reject_f");
    if (!c) return VILF_ERR_INVALID_ARGUMENT;
    if (n < 0 || n > TK_MAXN || !F_out || !best_out || !n_inliers_out || (n > 0 && (!cur_pts || !forw_pts || !status_out))) {
        h->err = "vilf_track_reject_f: null pointer, n < 0 or n > VILF_MAX_FEATURES"; return VILF_ERR_INVALID_ARGUMENT;
    }
    for (int i = 0; i < 2 * n; i++)
        if (!std::isfinite(cur_pts[i]) || !std::isfinite(forw_pts[i])) { h->err = "vilf_track_reject_f: a coordinate that is not finite"; return VILF_ERR_INVALID_ARGUMENT; }
    if (n >= 8) {
        HIPCHECK(h, hipSetDevice(h->device));
        // lkpts, fwd and status are scratch of a single call (a frame's LK or vilf_track_lk): nothing of the tracked state lives in them between calls
        HIPCHECK(h, hipMemcpyAsync(c->lkpts.p, cur_pts, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
        HIPCHECK(h, hipMemcpyAsync(c->fwd.p, forw_pts, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
        HIPCHECK(h, hipMemsetAsync(c->status.p, 1, (size_t)n, h->stream));
        { const int rc = tk_reject(h, c, c->lkpts.as<float2>(), c->fwd.as<float2>(), c->status.as<unsigned char>(), nullptr, n); if (rc != VILF_OK) return rc; }
        double res[TK_F_RES];
        HIPCHECK(h, hipMemcpyAsync(status_out, c->status.p, (size_t)n, hipMemcpyDeviceToHost, h->stream));
        HIPCHECK(h, vilf_copy_sync(h, res, tk_f(c).res, sizeof(res), hipMemcpyDeviceToHost));
        *best_out = (int)res[0]; *n_inliers_out = (int)res[1];
        for (int e = 0; e < 9; e++) F_out[e] = res[2 + e];
        return VILF_OK;
    }
    for (int i = 0; i < n; i++) status_out[i] = 1;           // fewer than 8 pairs: rejectWithF does nothing (:385)
    for (int e = 0; e < 9; e++) F_out[e] = 0.0;
    *best_out = -1; *n_inliers_out = n;
    return VILF_OK;
}

extern "C" int vilf_track_profile_frontend(vilf_handle *h, double ms_out[2], long launches_out[2]) { return vilf_stage_profile(h, ST_TRACK, &TrackCtx::fe_prof, ms_out, launches_out); }

extern "C" int vilf_track_configure_mask(vilf_handle *h, const vilf_track_mask_params *mp) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    TrackCtx *c = tk_ctx(h, "vilf_track_configure_mask");
    if (!c) return VILF_ERR_INVALID_ARGUMENT;
    if (!mp) { h->err = "vilf_track_configure_mask: null parameters"; return VILF_ERR_INVALID_ARGUMENT; }
    if (mp->erode_radius < 0 || mp->erode_radius > VILF_TRACK_MAX_ERODE || mp->probe < 1 || mp->probe > 64 || (mp->reject != 0 && mp->reject != 1) || !std::isfinite(mp->f_threshold) ||
        !(mp->f_threshold > 0) || !std::isfinite(mp->epi_threshold) || !(mp->epi_threshold > 0)) {
        h->err = "vilf_track_configure_mask: 0 <= erode_radius <= VILF_TRACK_MAX_ERODE, 1 <= probe <= 64, reject 0 or 1, positive finite thresholds";
        return VILF_ERR_INVALID_ARGUMENT;
    }
    c->mp = *mp;
    return VILF_OK;
}

extern "C" int vilf_track_set_fisheye_mask(vilf_handle *h, const unsigned char *mask, int row_stride) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    TrackCtx *c = tk_ctx(h, "vilf_track_set_fisheye_mask");
    if (!c) return VILF_ERR_INVALID_ARGUMENT;
    if (!mask) { c->has_fish = false; return VILF_OK; }
    if (row_stride < c->p.width) { h->err = "vilf_track_set_fisheye_mask: row_stride < width"; return VILF_ERR_INVALID_ARGUMENT; }
    HIPCHECK(h, hipSetDevice(h->device));
    { const int rc = tk_upload_mask(h, c, c->fish.as<unsigned char>(), mask, row_stride); if (rc != VILF_OK) return rc; }
    HIPCHECK(h, hipStreamSynchronize(h->stream));
    c->has_fish = true;
    return VILF_OK;
}

extern "C" int vilf_track_erode(vilf_handle *h, const unsigned char *mask, int row_stride, unsigned char *out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    TrackCtx *c = tk_ctx(h, "vilf_track_erode");
    if (!c) return VILF_ERR_INVALID_ARGUMENT;
    if (!mask || !out || row_stride < c->p.width) { h->err = "vilf_track_erode: null pointer or row_stride < width"; return VILF_ERR_INVALID_ARGUMENT; }
    HIPCHECK(h, hipSetDevice(h->device));
    // mraw, er and sstatus are scratch of a single call (a masked frame or a stateless call): nothing of the tracked state lives in them between calls
    { const int rc = tk_upload_mask(h, c, c->mraw.as<unsigned char>(), mask, row_stride); if (rc != VILF_OK) return rc; }
    { const int rc = tk_erode(h, c, c->mraw.as<unsigned char>(), c->er.as<unsigned char>()); if (rc != VILF_OK) return rc; }
    HIPCHECK(h, vilf_copy_sync(h, out, c->er.p, c->ncell, hipMemcpyDeviceToHost));
    return VILF_OK;
}

extern "C" int vilf_track_probe(vilf_handle *h, const unsigned char *eroded, const float *pts, int n, unsigned char *static_out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    TrackCtx *c = tk_ctx(h, "vilf_track_probe");
    if (!c) return VILF_ERR_INVALID_ARGUMENT;
    if (!eroded || n < 0 || n > TK_MAXN || (n > 0 && (!pts || !static_out))) { h->err = "vilf_track_probe: null pointer, n < 0 or n > VILF_MAX_FEATURES"; return VILF_ERR_INVALID_ARGUMENT; }
    for (int i = 0; i < 2 * n; i++)
        if (!std::isfinite(pts[i])) { h->err = "vilf_track_probe: a coordinate that is not finite"; return VILF_ERR_INVALID_ARGUMENT; }
    if (n == 0) return VILF_OK;
    HIPCHECK(h, hipSetDevice(h->device));
    { const int rc = tk_upload_mask(h, c, c->er.as<unsigned char>(), eroded, c->p.width); if (rc != VILF_OK) return rc; }
    HIPCHECK(h, hipMemcpyAsync(c->fwd.p, pts, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(tk_mask_probe, dim3((n + TK_NT - 1) / TK_NT), dim3(TK_NT), 0, h->stream, c->er.as<unsigned char>(), c->fwd.as<float2>(), (const unsigned char *)nullptr, (const int *)nullptr, n,
                       c->p.width, c->p.height, c->mp.probe, c->sstatus.as<unsigned char>());
    HIPCHECK(h, hipGetLastError());
    HIPCHECK(h, vilf_copy_sync(h, static_out, c->sstatus.p, (size_t)n, hipMemcpyDeviceToHost));
    return VILF_OK;
}

extern "C" int vilf_track_reject_f_mask(vilf_handle *h, const float *cur_pts, const float *forw_pts, const unsigned char *is_static, int n, unsigned char *status_out, double F_out[9], int *best_out,
                                        int *n_static_inliers_out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    TrackCtx *c = tk_ctx(h, "vilf_track_reject_f_mask");
    if (!c) return VILF_ERR_INVALID_ARGUMENT;
    if (n < 0 || n > TK_MAXN || !F_out || !best_out || !n_static_inliers_out || (n > 0 && (!cur_pts || !forw_pts || !is_static || !status_out))) {
        h->err = "vilf_track_reject_f_mask: null pointer, n < 0 or n > VILF_MAX_FEATURES"; return VILF_ERR_INVALID_ARGUMENT;
    }
    for (int i = 0; i < 2 * n; i++)
        if (!std::isfinite(cur_pts[i]) || !std::isfinite(forw_pts[i])) { h->err = "vilf_track_reject_f_mask: a coordinate that is not finite"; return VILF_ERR_INVALID_ARGUMENT; }
    int m = 0;
    for (int i = 0; i < n; i++) m += is_static[i] ? 1 : 0;
    if (m >= 8) {
        HIPCHECK(h, hipSetDevice(h->device));
        HIPCHECK(h, hipMemcpyAsync(c->lkpts.p, cur_pts, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
        HIPCHECK(h, hipMemcpyAsync(c->fwd.p, forw_pts, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
        HIPCHECK(h, hipMemcpyAsync(c->sstatus.p, is_static, (size_t)n, hipMemcpyHostToDevice, h->stream));
        HIPCHECK(h, hipMemsetAsync(c->status.p, 1, (size_t)n, h->stream));
        { const int rc = tk_reject_mask(h, c, c->lkpts.as<float2>(), c->fwd.as<float2>(), c->sstatus.as<unsigned char>(), c->status.as<unsigned char>(), nullptr, n); if (rc != VILF_OK) return rc; }
        double res[TK_F_RES];
        HIPCHECK(h, hipMemcpyAsync(status_out, c->status.p, (size_t)n, hipMemcpyDeviceToHost, h->stream));
        HIPCHECK(h, vilf_copy_sync(h, res, tk_f(c).res, sizeof(res), hipMemcpyDeviceToHost));
        *best_out = (int)res[0]; *n_static_inliers_out = (int)res[1];
        for (int e = 0; e < 9; e++) F_out[e] = res[2 + e];
        return VILF_OK;
    }
    for (int i = 0; i < n; i++) status_out[i] = 1;           // fewer than 8 static pairs: rejectWithF_mask does nothing
    for (int e = 0; e < 9; e++) F_out[e] = 0.0;
    *best_out = -1; *n_static_inliers_out = m;
    return VILF_OK;
}

extern "C" int vilf_track_profile_mask(vilf_handle *h, double ms_out[2], long launches_out[2]) { return vilf_stage_profile(h, ST_TRACK, &TrackCtx::mk_prof, ms_out, launches_out); }
