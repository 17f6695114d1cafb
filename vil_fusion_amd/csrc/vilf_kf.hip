// vilf_kf.hip — the first stage of the visual loop closure on the device (≙ KeyFrame::computeWindowBRIEFPoint, computeBRIEFPoint, searchByBRIEFDes / searchInAera,
//   pose_graph/keyframe.cpp:75-171, with BRIEF::compute, ThirdParty/DVision/BRIEF.cpp:39-106). The arithmetic is stated once, in include/vilfusion.h ("Visual loop
//   closure, first stage"); OpenCV is not a dependency. Everything about a key frame stays in a device store sized at creation (KfCtx).
// One key frame from an image = one chain of launches on the handle's stream:
//   kf_blur          a 32 x 8 tile: the raw bytes with a four-pixel halo into LDS, the horizontal pass into LDS as uint16, the vertical pass out of it
//   kf_fast_score    a 32 x 8 tile with a three-pixel halo in LDS: the 16 differences in registers, the best arc of either sign -> one score byte per pixel
//   kf_nms_count     a wave per row: the survivors of the 3 x 3 maximum rule, counted with __ballot / __popcll
//   kf_nms_scan      one workgroup: the exclusive scan of the row counts, the total
//   kf_nms_place     a wave per row again: a survivor goes to row offset + its rank in the row, so the order is row-major whatever the scheduling; no atomics
//   kf_brief         a wave per point: lane l evaluates tests l, l + 64, l + 128, l + 192, four ballots are the four words; serves FAST and window points
//   kf_lift          a lane per FAST point: the tracker's undistortion (vilf_image.hpp), rounded to float32
// The host reads the total of kf_nms_scan once per key frame, between kf_nms_scan and kf_nms_place: the capacity check, and the grids of what follows.
// One search = one launch for all the old key frames of the call:
//   kf_match         grid (blocks of 64 window points, old key frames), four waves: lane l of every wave keeps window descriptor l of the block in registers; the
//                    old descriptors go through LDS in chunks of VILF_KF_MATCH_CHUNK, wave w takes entries 64 w .. 64 w + 63 of each chunk (every lane reads the
//                    same address: a broadcast); the four (distance, index) pairs per window point meet in LDS under the lexicographic minimum, which is the
//                    reference's "first of the smallest" under any split. The number of matches per old key frame is an integer atomicAdd of ballot counts.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "vilf_internal.hpp"
#include "vilf_device.hpp"
#include "vilf_kernels.hpp"
#include "vilf_image.hpp"
#include "vilf_kf.hpp"

#define KF_MAX_POINTS (1 << 20)         // vilf_kf_brief

// the packed pattern: test i as (x1 + 64) | (y1 + 64) << 8 | (x2 + 64) << 16 | (y2 + 64) << 24, every byte 0 .. 128
static_assert(VILF_KF_MAX_OFFSET == 64 && VILF_KF_BITS == 256 && KF_WORDS * 64 == VILF_KF_BITS, "a byte per offset; four tests per lane");

// ---- launch contract -----------------------------------------------------------------------------------------------------
#define KF_TW 32                        // kf_blur, kf_fast_score: block (32, 8), grid = tiles of the image
#define KF_TH 8
#define KF_BLUR_R 4
#define KF_BLUR_LW (KF_TW + 2 * KF_BLUR_R)
#define KF_BLUR_LH (KF_TH + 2 * KF_BLUR_R)
#define KF_FAST_R 3
#define KF_FAST_LW (KF_TW + 2 * KF_FAST_R)
#define KF_FAST_LH (KF_TH + 2 * KF_FAST_R)
#define KF_CHUNK VILF_KF_MATCH_CHUNK    // kf_match: 256 descriptors = 8 KB of LDS
static_assert(KF_CHUNK == 64 * KF_WAVES, "kf_match: a wave takes 64 entries of a chunk");
__global__ void kf_blur(const unsigned char *src, int W, int H, unsigned char *dst);
__global__ void kf_fast_score(const unsigned char *img, int W, int H, int thr, unsigned char *score);
__global__ void kf_nms_count(const unsigned char *score, int W, int H, int *rowcnt);                       // grid = ceil(H / 4)
__global__ void kf_nms_scan(const int *rowcnt, int H, int *rowoff, int *total);                            // one workgroup
__global__ void kf_nms_place(const unsigned char *score, int W, int H, const int *rowoff, int limit, float2 *pts, unsigned char *pscore);   // grid = ceil(H / 4); pscore may be null
__global__ void kf_brief(const unsigned char *blur, int W, int H, const unsigned *pat, const float2 *pts, int n, unsigned long long *desc);   // grid = ceil(n / 4)
__global__ void kf_lift(const float2 *pts, int n, TkCam cam, float2 *out);                                 // grid = ceil(n / 256)
// kf_match, the store (KfCtx) and the match as an enqueue: vilf_kf.hpp, shared with the second stage

// ---- kf_blur -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KF_TW * KF_TH) void kf_blur(const unsigned char *src, int W, int H, unsigned char *dst) {
    __shared__ unsigned char raw[KF_BLUR_LH][KF_BLUR_LW];
    __shared__ unsigned short hb[KF_BLUR_LH][KF_TW];
    const int tx = threadIdx.x, ty = threadIdx.y, t = ty * KF_TW + tx;
    const int x0 = blockIdx.x * KF_TW, y0 = blockIdx.y * KF_TH;
    const int q[9] = {7, 17, 32, 46, 52, 46, 32, 17, 7};
    for (int i = t; i < KF_BLUR_LH * KF_BLUR_LW; i += KF_TW * KF_TH) {
        const int ly = i / KF_BLUR_LW, lx = i % KF_BLUR_LW;
        raw[ly][lx] = src[(size_t)tk_r(y0 - KF_BLUR_R + ly, H) * W + tk_r(x0 - KF_BLUR_R + lx, W)];
    }
    __syncthreads();
    for (int i = t; i < KF_BLUR_LH * KF_TW; i += KF_TW * KF_TH) {
        const int ly = i / KF_TW, lx = i % KF_TW;
        int acc = 0;
#pragma unroll
        for (int k = 0; k < 9; k++) acc += q[k] * (int)raw[ly][lx + k];
        hb[ly][lx] = (unsigned short)acc;                    // at most 256 * 255
    }
    __syncthreads();
    const int x = x0 + tx, y = y0 + ty;
    if (x >= W || y >= H) return;
    int v = 0;
#pragma unroll
    for (int k = 0; k < 9; k++) v += q[k] * (int)hb[ty + k][tx];
    dst[(size_t)y * W + x] = (unsigned char)((v + 32768) >> 16);
}

// ---- kf_fast_score -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KF_TW * KF_TH) void kf_fast_score(const unsigned char *img, int W, int H, int thr, unsigned char *score) {
    __shared__ unsigned char s[KF_FAST_LH][KF_FAST_LW + 2];
    const int tx = threadIdx.x, ty = threadIdx.y, t = ty * KF_TW + tx;
    const int x0 = blockIdx.x * KF_TW, y0 = blockIdx.y * KF_TH;
    for (int i = t; i < KF_FAST_LH * KF_FAST_LW; i += KF_TW * KF_TH) {
        const int ly = i / KF_FAST_LW, lx = i % KF_FAST_LW;
        const int gx = min(max(x0 - KF_FAST_R + lx, 0), W - 1), gy = min(max(y0 - KF_FAST_R + ly, 0), H - 1);      // a clamped read is only ever used by an untested pixel
        s[ly][lx] = img[(size_t)gy * W + gx];
    }
    __syncthreads();
    const int x = x0 + tx, y = y0 + ty;
    if (x >= W || y >= H) return;
    int sc = 0;
    if (x >= KF_FAST_R && x < W - KF_FAST_R && y >= KF_FAST_R && y < H - KF_FAST_R) {
        const int cx[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1}, cy[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};
        const int c = (int)s[ty + KF_FAST_R][tx + KF_FAST_R];
        int d[16];
#pragma unroll
        for (int k = 0; k < 16; k++) d[k] = c - (int)s[ty + KF_FAST_R + cy[k]][tx + KF_FAST_R + cx[k]];
        int A = -256, B = -256;
#pragma unroll
        for (int a = 0; a < 16; a++) {
            int lo = d[a], hi = d[a];
#pragma unroll
            for (int j = 1; j < 9; j++) { lo = min(lo, d[(a + j) & 15]); hi = max(hi, d[(a + j) & 15]); }
            A = max(A, lo); B = max(B, -hi);
        }
        const int m = max(A, B);
        sc = m > thr ? m - 1 : 0;
    }
    score[(size_t)y * W + x] = (unsigned char)sc;
}

namespace {
// the 3 x 3 rule at a pixel: a corner whose score is strictly above all eight neighbours' (an untested pixel scores 0 and is never kept, so every read is inside)
VD bool kf_keep(const unsigned char *score, int W, int H, int x, int y) {
    if (x < KF_FAST_R || x >= W - KF_FAST_R || y < KF_FAST_R || y >= H - KF_FAST_R) return false;
    const unsigned char *r = score + (size_t)y * W + x;
    const int s = r[0];
    if (s == 0) return false;
    return s > (int)r[-W - 1] && s > (int)r[-W] && s > (int)r[-W + 1] && s > (int)r[-1] && s > (int)r[1] && s > (int)r[W - 1] && s > (int)r[W] && s > (int)r[W + 1];
}
}  // namespace

// ---- kf_nms_count / kf_nms_scan / kf_nms_place -----------------------------------------------------------------------------------
__global__ __launch_bounds__(KF_NT) void kf_nms_count(const unsigned char *score, int W, int H, int *rowcnt) {
    const int lane = threadIdx.x & 63, y = blockIdx.x * KF_WAVES + (threadIdx.x >> 6);
    if (y >= H) return;                                  // the whole wave
    int cnt = 0;
    for (int xb = 0; xb < W; xb += 64) cnt += __popcll(__ballot(kf_keep(score, W, H, xb + lane, y)));
    if (lane == 0) rowcnt[y] = cnt;
}
__global__ __launch_bounds__(KF_NT) void kf_nms_scan(const int *rowcnt, int H, int *rowoff, int *total) {
    __shared__ int s[KF_NT];
    const int t = threadIdx.x, per = (H + KF_NT - 1) / KF_NT, r0 = min(t * per, H), r1 = min(r0 + per, H);
    int sum = 0;
    for (int r = r0; r < r1; r++) sum += rowcnt[r];
    s[t] = sum;
    __syncthreads();
    for (int o = 1; o < KF_NT; o <<= 1) {                 // inclusive scan of the threads' sums
        const int v = t >= o ? s[t - o] : 0;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    int run = s[t] - sum;
    for (int r = r0; r < r1; r++) { rowoff[r] = run; run += rowcnt[r]; }
    if (t == KF_NT - 1) *total = s[t];
}
__global__ __launch_bounds__(KF_NT) void kf_nms_place(const unsigned char *score, int W, int H, const int *rowoff, int limit, float2 *pts, unsigned char *pscore) {
    const int lane = threadIdx.x & 63, y = blockIdx.x * KF_WAVES + (threadIdx.x >> 6);
    if (y >= H) return;
    int base = rowoff[y];
    for (int xb = 0; xb < W; xb += 64) {
        const int x = xb + lane;
        const bool keep = kf_keep(score, W, H, x, y);
        const unsigned long long b = __ballot(keep);
        const int i = base + __popcll(b & ((1ull << lane) - 1ull));
        if (keep && i < limit) {                         // the host sized the target from the total: the bound never bites, it keeps a wrong total from writing outside
            pts[i] = make_float2((float)x, (float)y);
            if (pscore) pscore[i] = score[(size_t)y * W + x];
        }
        base += __popcll(b);
    }
}

// ---- kf_brief: a wave per point ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KF_NT) void kf_brief(const unsigned char *blur, int W, int H, const unsigned *pat, const float2 *pts, int n, unsigned long long *desc) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * KF_WAVES + (threadIdx.x >> 6);
    if (i >= n) return;                                  // the whole wave
    const float2 p = pts[i];
    unsigned long long w[KF_WORDS];
#pragma unroll
    for (int k = 0; k < KF_WORDS; k++) {
        const unsigned c = pat[lane + 64 * k];
        const int X1 = (int)__fadd_rn(p.x, (float)((int)(c & 0xff) - 64)), Y1 = (int)__fadd_rn(p.y, (float)((int)((c >> 8) & 0xff) - 64));
        const int X2 = (int)__fadd_rn(p.x, (float)((int)((c >> 16) & 0xff) - 64)), Y2 = (int)__fadd_rn(p.y, (float)((int)(c >> 24) - 64));
        const bool in = (unsigned)X1 < (unsigned)W && (unsigned)Y1 < (unsigned)H && (unsigned)X2 < (unsigned)W && (unsigned)Y2 < (unsigned)H;
        bool bit = false;
        if (in) bit = blur[(size_t)Y1 * W + X1] < blur[(size_t)Y2 * W + X2];
        w[k] = __ballot(bit);
    }
    if (lane == 0) {
        ulonglong2 *o = (ulonglong2 *)(desc + (size_t)i * KF_WORDS);      // 32-byte rows of a hipMalloc'ed array
        o[0] = make_ulonglong2(w[0], w[1]);
        o[1] = make_ulonglong2(w[2], w[3]);
    }
}

// ---- kf_lift -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KF_NT) void kf_lift(const float2 *pts, int n, TkCam cam, float2 *out) {
    const int i = blockIdx.x * KF_NT + threadIdx.x;
    if (i >= n) return;
    double ux, uy;
    tk_undistort(cam, pts[i], ux, uy);
    out[i] = make_float2((float)ux, (float)uy);
}

// ---- kf_match ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KF_NT) void kf_match(const KfMeta *meta, const unsigned long long *kp_desc, const float2 *kp_pt, const float2 *kp_norm, const unsigned long long *win_desc,
                                                  int cur, const int *old, int max_dist, int accept_dist, KfMatchOut out) {
    __shared__ ulonglong2 sd[KF_CHUNK * 2];              // a descriptor = two 16-byte halves
    __shared__ int rd[KF_WAVES][64], ri[KF_WAVES][64];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, cand = blockIdx.y;
    const int nw = meta[cur].n_win, wi = blockIdx.x * 64 + lane;
    const bool valid = wi < nw;
    const int4 om = ((const int4 *)meta)[old[cand]];      // one 16-byte load of the row
    const struct { int kp_off, n_kp; } o = {om.x, om.y};
    unsigned long long w0 = 0, w1 = 0, w2 = 0, w3 = 0;
    if (valid) {
        const ulonglong2 *w = (const ulonglong2 *)(win_desc + ((size_t)cur * KF_WIN_CAP + wi) * KF_WORDS);
        const ulonglong2 a = w[0], b = w[1];
        w0 = a.x; w1 = a.y; w2 = b.x; w3 = b.y;
    }
    const ulonglong2 *D = (const ulonglong2 *)(kp_desc + (size_t)o.kp_off * KF_WORDS);
    int best = max_dist, bi = -1;
    for (int c0 = 0; c0 < o.n_kp; c0 += KF_CHUNK) {      // the trip count is the workgroup's: o is uniform
        const int cnt = min(KF_CHUNK, o.n_kp - c0);
        for (int i = t; i < cnt * 2; i += KF_NT) sd[i] = D[(size_t)c0 * 2 + i];
        __syncthreads();
        const int j1 = min(64 * wave + 64, cnt);
        for (int j = 64 * wave; j < j1; j++) {           // j ascends within a wave, chunk after chunk: the first of equal distances stays
            const ulonglong2 a = sd[2 * j], b = sd[2 * j + 1];
            const int d = __popcll(w0 ^ a.x) + __popcll(w1 ^ a.y) + __popcll(w2 ^ b.x) + __popcll(w3 ^ b.y);
            if (d < best) { best = d; bi = c0 + j; }
        }
        __syncthreads();
    }
    rd[wave][lane] = best; ri[wave][lane] = bi;
    __syncthreads();
    if (wave != 0) return;
    for (int w = 1; w < KF_WAVES; w++) {                 // found pairs have distance < max_dist, so a "none" (max_dist, -1) never beats one
        const int d = rd[w][lane], i = ri[w][lane];
        if (d < best || (d == best && i < bi && i >= 0)) { best = d; bi = i; }
    }
    const bool st = valid && bi >= 0 && best < accept_dist;
    if (valid) {
        const size_t r = (size_t)cand * nw + wi;
        float2 p = make_float2(0.f, 0.f), pn = p;
        if (st) { p = kp_pt[o.kp_off + bi]; pn = kp_norm[o.kp_off + bi]; }
        out.status[r] = st ? 1 : 0;
        out.pt[r] = p;
        out.ptn[r] = pn;
        out.idx[r] = bi;
        out.dist[r] = best;
    }
    const int m = __popcll(__ballot(st));
    if (lane == 0 && m > 0) atomicAdd(&out.nmatched[cand], m);       // an integer sum: the order of the blocks does not show
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
KfCtx *vilf_kf_ctx(vilf_handle *h, const char *who) {
    KfCtx *c = vilf_stage<KfCtx>(h, ST_KF);
    if (!c) h->err = std::string(who) + ": no key-frame store (vilf_kf_create)";
    return c;
}
int vilf_kf_finish(vilf_handle *h) {                      // a fault of the launches is reported by the call that made them
    HIPCHECK(h, hipGetLastError());
    HIPCHECK(h, hipStreamSynchronize(h->stream));
    if (h->profiling) return vilf_prof_flush(h);
    return VILF_OK;
}
namespace {
bool kf_points_ok(const float *pts, int n) {
    for (int i = 0; i < 2 * n; i++) if (!std::isfinite(pts[i]) || std::fabs(pts[i]) > 1.0e6f) return false;
    return true;
}
inline dim3 kf_tiles(int W, int H) { return dim3((W + KF_TW - 1) / KF_TW, (H + KF_TH - 1) / KF_TH); }
// the image -> c->img (rows tight), through the pinned staging
int kf_upload(vilf_handle *h, KfCtx *c, const unsigned char *img, int row_stride) {
    const size_t W = (size_t)c->p.width, H = (size_t)c->p.height;
    unsigned char *stage = (unsigned char *)c->stage.p;
    if ((size_t)row_stride == W) std::memcpy(stage, img, W * H);
    else for (size_t y = 0; y < H; y++) std::memcpy(stage + y * W, img + y * (size_t)row_stride, W);
    HIPCHECK(h, hipMemcpyAsync(c->img.p, stage, W * H, hipMemcpyHostToDevice, h->stream));
    return VILF_OK;
}
int kf_run_blur(vilf_handle *h, KfCtx *c) {
    const int W = c->p.width, H = c->p.height;
    hipLaunchKernelGGL(kf_blur, kf_tiles(W, H), dim3(KF_TW, KF_TH), 0, h->stream, c->img.as<unsigned char>(), W, H, c->blur.as<unsigned char>());
    HIPCHECK(h, hipGetLastError());
    return VILF_OK;
}
// score, row counts, scan; the host waits for the total
int kf_run_fast_count(vilf_handle *h, KfCtx *c, int *n_out) {
    const int W = c->p.width, H = c->p.height, rows = (H + KF_WAVES - 1) / KF_WAVES;
    hipLaunchKernelGGL(kf_fast_score, kf_tiles(W, H), dim3(KF_TW, KF_TH), 0, h->stream, c->img.as<unsigned char>(), W, H, c->p.fast_threshold, c->score.as<unsigned char>());
    hipLaunchKernelGGL(kf_nms_count, dim3(rows), dim3(KF_NT), 0, h->stream, c->score.as<unsigned char>(), W, H, c->rowcnt.as<int>());
    hipLaunchKernelGGL(kf_nms_scan, dim3(1), dim3(KF_NT), 0, h->stream, c->rowcnt.as<int>(), H, c->rowoff.as<int>(), c->total.as<int>());
    HIPCHECK(h, hipGetLastError());
    int *pin = (int *)c->pin.p;
    HIPCHECK(h, vilf_copy_sync(h, pin, c->total.p, 4, hipMemcpyDeviceToHost));
    *n_out = pin[0];
    return VILF_OK;
}
int kf_run_place(vilf_handle *h, KfCtx *c, int n, float2 *pts, unsigned char *pscore) {
    const int W = c->p.width, H = c->p.height, rows = (H + KF_WAVES - 1) / KF_WAVES;
    if (n > 0) hipLaunchKernelGGL(kf_nms_place, dim3(rows), dim3(KF_NT), 0, h->stream, c->score.as<unsigned char>(), W, H, c->rowoff.as<int>(), n, pts, pscore);
    HIPCHECK(h, hipGetLastError());
    return VILF_OK;
}
int kf_run_brief(vilf_handle *h, KfCtx *c, const float2 *pts, int n, unsigned long long *desc) {
    if (n > 0) hipLaunchKernelGGL(kf_brief, dim3((n + KF_WAVES - 1) / KF_WAVES), dim3(KF_NT), 0, h->stream, c->blur.as<unsigned char>(), c->p.width, c->p.height, c->pat.as<unsigned>(), pts, n, desc);
    HIPCHECK(h, hipGetLastError());
    return VILF_OK;
}
// offsets into the pinned words: the total, a meta row, then window points or old indices
enum : size_t { KF_PIN_META = 16, KF_PIN_DATA = 64, KF_PIN_BYTES = KF_PIN_DATA + (size_t)KF_WIN_CAP * 8 };
static_assert(KF_PIN_BYTES >= KF_PIN_DATA + VILF_KF_MAX_CANDIDATES * 4, "the old indices fit where the window points do");
// what both ways of adding a key frame refuse; on success the new key frame is number c->size
int kf_check_add(vilf_handle *h, KfCtx *c, const char *who, int n_window, const float *window_uv) {
    if (n_window < 0 || n_window > KF_WIN_CAP || (n_window > 0 && !window_uv)) { h->err = std::string(who) + ": 0 <= n_window <= VILF_MAX_FEATURES and its points"; return VILF_ERR_INVALID_ARGUMENT; }
    if (!kf_points_ok(window_uv, n_window)) { h->err = std::string(who) + ": a window point is not finite or lies beyond 1e6 pixels"; return VILF_ERR_INVALID_ARGUMENT; }
    if (c->size >= c->capK) { h->err = std::string(who) + ": the store holds its " + std::to_string(c->capK) + " key frames"; return VILF_ERR_INVALID_ARGUMENT; }
    return VILF_OK;
}
// the new key frame's row of the table, on the stream; the caller commits after the wait
int kf_put_meta(vilf_handle *h, KfCtx *c, const KfMeta &m) {
    KfMeta *pm = (KfMeta *)((char *)c->pin.p + KF_PIN_META);
    *pm = m;
    HIPCHECK(h, hipMemcpyAsync(c->meta_d.as<KfMeta>() + c->size, pm, sizeof(KfMeta), hipMemcpyHostToDevice, h->stream));
    return VILF_OK;
}
void kf_commit(KfCtx *c, const KfMeta &m) { c->meta.push_back(m); c->size++; c->used += m.n_kp; }
}  // namespace

extern "C" void vilf_kf_default_params(vilf_kf_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->fast_threshold = 20; p->match_max_dist = 128; p->match_accept_dist = 80;
}

extern "C" int vilf_kf_create(vilf_handle *h, const vilf_kf_params *p, int cap_keyframes, long cap_keypoints) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    if (!p) { h->err = "vilf_kf_create: null parameters"; return VILF_ERR_INVALID_ARGUMENT; }
    if (p->width <= 21 || p->height <= 21 || cap_keyframes < 1 || cap_keypoints < 1 || cap_keypoints > (1l << 30) || p->fast_threshold < 1 || p->fast_threshold > 254 ||
        p->match_max_dist < 0 || p->match_max_dist > VILF_KF_BITS + 1 || p->match_accept_dist < 0 || p->match_accept_dist > VILF_KF_BITS + 1 || !(p->fx > 0) || !(p->fy > 0) ||
        !std::isfinite(p->fx) || !std::isfinite(p->fy) || !std::isfinite(p->cx) || !std::isfinite(p->cy) || !std::isfinite(p->k1) || !std::isfinite(p->k2) || !std::isfinite(p->p1) || !std::isfinite(p->p2)) {
        h->err = "vilf_kf_create: both sides > 21, capacities >= 1 (key points <= 2^30), 1 <= fast_threshold <= 254, match distances in 0 .. 257, positive focal lengths, finite camera parameters";
        return VILF_ERR_INVALID_ARGUMENT;
    }
    std::vector<unsigned> pat(VILF_KF_BITS);
    for (int i = 0; i < VILF_KF_BITS; i++) {
        const int v[4] = {p->x1[i], p->y1[i], p->x2[i], p->y2[i]};
        for (int k = 0; k < 4; k++) if (v[k] < -VILF_KF_MAX_OFFSET || v[k] > VILF_KF_MAX_OFFSET) { h->err = "vilf_kf_create: a pattern entry beyond +-64"; return VILF_ERR_INVALID_ARGUMENT; }
        pat[i] = (unsigned)(v[0] + 64) | (unsigned)(v[1] + 64) << 8 | (unsigned)(v[2] + 64) << 16 | (unsigned)(v[3] + 64) << 24;
    }
    if ((long long)p->width * p->height > (1ll << 28)) { h->err = "vilf_kf_create: more than 2^28 pixels"; return VILF_ERR_UNSUPPORTED; }
    HIPCHECK(h, hipSetDevice(h->device));
    { const int rcf = vilf_prof_flush(h); if (rcf != VILF_OK) return rcf; }      // no pending span may point into the store that goes
    HIPCHECK(h, hipStreamSynchronize(h->stream));
    KfCtx *c = new KfCtx();
    c->p = *p; c->capK = cap_keyframes; c->capP = cap_keypoints; c->ncell = (size_t)p->width * p->height;
    const size_t K = (size_t)cap_keyframes, P = (size_t)cap_keypoints, N = c->ncell, Hh = (size_t)p->height;
    if (!c->kp_pt.ensure(P * 8) || !c->kp_norm.ensure(P * 8) || !c->kp_desc.ensure(P * 32) || !c->win_pt.ensure(K * KF_WIN_CAP * 8) || !c->win_desc.ensure(K * KF_WIN_CAP * 32) ||
        !c->meta_d.ensure(K * sizeof(KfMeta)) || !c->pat.ensure(VILF_KF_BITS * 4) || !c->img.ensure(N) || !c->blur.ensure(N) || !c->score.ensure(N) || !c->rowcnt.ensure(Hh * 4) ||
        !c->rowoff.ensure(Hh * 4) || !c->total.ensure(16) || !c->old_d.ensure(VILF_KF_MAX_CANDIDATES * 4) || !c->stage.ensure(N) || !c->pin.ensure(KF_PIN_BYTES)) {
        delete c;
        h->err = "hipMalloc failed (key-frame store)";
        return VILF_ERR_DEVICE;
    }
    if (vilf_copy_sync(h, c->pat.p, pat.data(), VILF_KF_BITS * 4, hipMemcpyHostToDevice) != hipSuccess) {
        delete c;
        h->err = "vilf_kf_create: the pattern's upload failed";
        return VILF_ERR_DEVICE;
    }
    vilf_stage_drop(h, ST_KF);
    h->stage[ST_KF] = c;
    return VILF_OK;
}

extern "C" int vilf_kf_add_keyframe(vilf_handle *h, const unsigned char *img, int row_stride, const float *window_uv, int n_window, int *index_out, int *n_keypoints_out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    KfCtx *c = vilf_kf_ctx(h, "vilf_kf_add_keyframe");
    if (!c) return VILF_ERR_INVALID_ARGUMENT;
    if (!img || row_stride < c->p.width) { h->err = "vilf_kf_add_keyframe: null image or row_stride < width"; return VILF_ERR_INVALID_ARGUMENT; }
    { const int rc = kf_check_add(h, c, "vilf_kf_add_keyframe", n_window, window_uv); if (rc != VILF_OK) return rc; }
    HIPCHECK(h, hipSetDevice(h->device));
    float2 *wpt = c->win_pt.as<float2>() + (size_t)c->size * KF_WIN_CAP;
    unsigned long long *wdesc = c->win_desc.as<unsigned long long>() + (size_t)c->size * KF_WIN_CAP * KF_WORDS;
    ProfMarks prof(h, c->prof);
    { const int rc = kf_upload(h, c, img, row_stride); if (rc != VILF_OK) return rc; }
    if (n_window > 0) {
        float *pw = (float *)((char *)c->pin.p + KF_PIN_DATA);
        std::memcpy(pw, window_uv, (size_t)n_window * 8);
        HIPCHECK(h, hipMemcpyAsync(wpt, pw, (size_t)n_window * 8, hipMemcpyHostToDevice, h->stream));
    }
    { const int rc = kf_run_blur(h, c); if (rc != VILF_OK) return rc; }
    prof.mark(0);
    int n = 0;
    { const int rc = kf_run_fast_count(h, c, &n); if (rc != VILF_OK) return rc; }
    if (n < 0 || (long)n > c->capP - c->used) {          // nothing of the store has been touched: the window slot and the rows behind `used` belong to no key frame
        if (h->profiling) vilf_prof_flush(h);
        h->err = "vilf_kf_add_keyframe: " + std::to_string(n) + " FAST points exceed the " + std::to_string(c->capP - c->used) + " free key points";
        return VILF_ERR_INVALID_ARGUMENT;
    }
    float2 *kpt = c->kp_pt.as<float2>() + c->used;
    { const int rc = kf_run_place(h, c, n, kpt, nullptr); if (rc != VILF_OK) return rc; }
    prof.mark(1);
    { const int rc = kf_run_brief(h, c, kpt, n, c->kp_desc.as<unsigned long long>() + (size_t)c->used * KF_WORDS); if (rc != VILF_OK) return rc; }
    { const int rc = kf_run_brief(h, c, wpt, n_window, wdesc); if (rc != VILF_OK) return rc; }
    if (n > 0) hipLaunchKernelGGL(kf_lift, dim3((n + KF_NT - 1) / KF_NT), dim3(KF_NT), 0, h->stream, kpt, n, tk_cam(c->p.fx, c->p.fy, c->p.cx, c->p.cy, c->p.k1, c->p.k2, c->p.p1, c->p.p2),
                                  c->kp_norm.as<float2>() + c->used);
    const KfMeta m{(int)c->used, n, n_window, 0};
    { const int rc = kf_put_meta(h, c, m); if (rc != VILF_OK) return rc; }
    prof.mark(2);
    { const int rc = vilf_kf_finish(h); if (rc != VILF_OK) return rc; }
    if (index_out) *index_out = c->size;
    if (n_keypoints_out) *n_keypoints_out = n;
    kf_commit(c, m);
    return VILF_OK;
}

extern "C" int vilf_kf_add_loaded(vilf_handle *h, int n_kp, const float *keypoints, const float *keypoints_norm, const unsigned long long *descriptors,
                                  int n_window, const float *window_uv, const unsigned long long *window_descriptors, int *index_out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    KfCtx *c = vilf_kf_ctx(h, "vilf_kf_add_loaded");
    if (!c) return VILF_ERR_INVALID_ARGUMENT;
    if (n_kp < 0 || (n_kp > 0 && (!keypoints || !keypoints_norm || !descriptors)) || (n_window > 0 && !window_descriptors)) {
        h->err = "vilf_kf_add_loaded: n_kp >= 0 and every array whose count is positive"; return VILF_ERR_INVALID_ARGUMENT;
    }
    { const int rc = kf_check_add(h, c, "vilf_kf_add_loaded", n_window, window_uv); if (rc != VILF_OK) return rc; }
    if ((long)n_kp > c->capP - c->used) {
        h->err = "vilf_kf_add_loaded: " + std::to_string(n_kp) + " key points exceed the " + std::to_string(c->capP - c->used) + " free ones";
        return VILF_ERR_INVALID_ARGUMENT;
    }
    HIPCHECK(h, hipSetDevice(h->device));
    const size_t u = (size_t)c->used, k = (size_t)c->size, nk = (size_t)n_kp, nw = (size_t)n_window;
    ProfMarks prof(h, c->prof);
    if (nk) {
        HIPCHECK(h, hipMemcpyAsync(c->kp_pt.as<float2>() + u, keypoints, nk * 8, hipMemcpyHostToDevice, h->stream));
        HIPCHECK(h, hipMemcpyAsync(c->kp_norm.as<float2>() + u, keypoints_norm, nk * 8, hipMemcpyHostToDevice, h->stream));
        HIPCHECK(h, hipMemcpyAsync(c->kp_desc.as<unsigned long long>() + u * KF_WORDS, descriptors, nk * 32, hipMemcpyHostToDevice, h->stream));
    }
    if (nw) {
        HIPCHECK(h, hipMemcpyAsync(c->win_pt.as<float2>() + k * KF_WIN_CAP, window_uv, nw * 8, hipMemcpyHostToDevice, h->stream));
        HIPCHECK(h, hipMemcpyAsync(c->win_desc.as<unsigned long long>() + k * KF_WIN_CAP * KF_WORDS, window_descriptors, nw * 32, hipMemcpyHostToDevice, h->stream));
    }
    const KfMeta m{(int)c->used, n_kp, n_window, 0};
    { const int rc = kf_put_meta(h, c, m); if (rc != VILF_OK) return rc; }
    prof.mark(0);
    { const int rc = vilf_kf_finish(h); if (rc != VILF_OK) return rc; }     // the caller's arrays are free again
    if (index_out) *index_out = c->size;
    kf_commit(c, m);
    return VILF_OK;
}

extern "C" int vilf_kf_get(vilf_handle *h, int index, int cap_kp, float *keypoints, float *keypoints_norm, unsigned long long *descriptors, int *n_kp_out,
                           int cap_window, float *window_uv, unsigned long long *window_descriptors, int *n_window_out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    KfCtx *c = vilf_kf_ctx(h, "vilf_kf_get");
    if (!c) return VILF_ERR_INVALID_ARGUMENT;
    if (index < 0 || index >= c->size) { h->err = "vilf_kf_get: index out of range"; return VILF_ERR_INVALID_ARGUMENT; }
    const KfMeta m = c->meta[index];
    if (((keypoints || keypoints_norm || descriptors) && cap_kp < m.n_kp) || ((window_uv || window_descriptors) && cap_window < m.n_win)) {
        h->err = "vilf_kf_get: the key frame has " + std::to_string(m.n_kp) + " key points and " + std::to_string(m.n_win) + " window points";
        return VILF_ERR_INVALID_ARGUMENT;
    }
    HIPCHECK(h, hipSetDevice(h->device));
    const size_t u = (size_t)m.kp_off, k = (size_t)index, nk = (size_t)m.n_kp, nw = (size_t)m.n_win;
    ProfMarks prof(h, c->prof);
    if (nk && keypoints) HIPCHECK(h, hipMemcpyAsync(keypoints, c->kp_pt.as<float2>() + u, nk * 8, hipMemcpyDeviceToHost, h->stream));
    if (nk && keypoints_norm) HIPCHECK(h, hipMemcpyAsync(keypoints_norm, c->kp_norm.as<float2>() + u, nk * 8, hipMemcpyDeviceToHost, h->stream));
    if (nk && descriptors) HIPCHECK(h, hipMemcpyAsync(descriptors, c->kp_desc.as<unsigned long long>() + u * KF_WORDS, nk * 32, hipMemcpyDeviceToHost, h->stream));
    if (nw && window_uv) HIPCHECK(h, hipMemcpyAsync(window_uv, c->win_pt.as<float2>() + k * KF_WIN_CAP, nw * 8, hipMemcpyDeviceToHost, h->stream));
    if (nw && window_descriptors) HIPCHECK(h, hipMemcpyAsync(window_descriptors, c->win_desc.as<unsigned long long>() + k * KF_WIN_CAP * KF_WORDS, nw * 32, hipMemcpyDeviceToHost, h->stream));
    prof.mark(4);
    { const int rc = vilf_kf_finish(h); if (rc != VILF_OK) return rc; }
    if (n_kp_out) *n_kp_out = m.n_kp;
    if (n_window_out) *n_window_out = m.n_win;
    return VILF_OK;
}

extern "C" int vilf_kf_size(vilf_handle *h, int *n_out) {
    if (!h || !n_out) return VILF_ERR_INVALID_ARGUMENT;
    const KfCtx *c = vilf_stage<KfCtx>(h, ST_KF);
    *n_out = c ? c->size : 0;
    return VILF_OK;
}

int vilf_kf_match_check(vilf_handle *h, KfCtx *c, const char *who, int cur, int n_old, const int *old_index) {
    if (cur < 0 || cur >= c->size || n_old < 1 || n_old > VILF_KF_MAX_CANDIDATES || !old_index) {
        h->err = std::string(who) + ": cur inside the store, 1 <= n_old <= VILF_KF_MAX_CANDIDATES and their indices"; return VILF_ERR_INVALID_ARGUMENT;
    }
    for (int i = 0; i < n_old; i++) if (old_index[i] < 0 || old_index[i] >= c->size) { h->err = std::string(who) + ": an old index outside the store"; return VILF_ERR_INVALID_ARGUMENT; }
    return VILF_OK;
}

int vilf_kf_match_enqueue(vilf_handle *h, KfCtx *c, int cur, int n_old, const int *old_index, const KfMatchOut &out) {
    const int nw = c->meta[cur].n_win;
    int *po = (int *)((char *)c->pin.p + KF_PIN_DATA);
    std::memcpy(po, old_index, (size_t)n_old * 4);
    HIPCHECK(h, hipMemcpyAsync(c->old_d.p, po, (size_t)n_old * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(h, hipMemsetAsync(out.nmatched, 0, (size_t)n_old * 4, h->stream));
    if (nw > 0) hipLaunchKernelGGL(kf_match, dim3((nw + 63) / 64, n_old), dim3(KF_NT), 0, h->stream, c->meta_d.as<KfMeta>(), c->kp_desc.as<unsigned long long>(), c->kp_pt.as<float2>(),
                                   c->kp_norm.as<float2>(), c->win_desc.as<unsigned long long>(), cur, c->old_d.as<int>(), c->p.match_max_dist, c->p.match_accept_dist, out);
    HIPCHECK(h, hipGetLastError());
    return VILF_OK;
}

extern "C" int vilf_kf_match(vilf_handle *h, int cur, int n_old, const int *old_index, unsigned char *status, float *pt_old, float *pt_old_norm, int *best_index,
                             int *best_dist, int *n_matched) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    KfCtx *c = vilf_kf_ctx(h, "vilf_kf_match");
    if (!c) return VILF_ERR_INVALID_ARGUMENT;
    { const int rc = vilf_kf_match_check(h, c, "vilf_kf_match", cur, n_old, old_index); if (rc != VILF_OK) return rc; }
    HIPCHECK(h, hipSetDevice(h->device));
    const int nw = c->meta[cur].n_win;
    const size_t rows = (size_t)n_old * nw;
    // the results of one call, one allocation: points, lifted points, indices, distances, counts, status bytes
    Layout l;
    const size_t o_pt = l.take(rows * 8, 8), o_ptn = l.take(rows * 8, 8), o_idx = l.take(rows * 4, 4), o_dist = l.take(rows * 4, 4), o_cnt = l.take((size_t)n_old * 4, 4),
                 o_st = l.take(rows, 1), bytes = l.at;
    if (!c->res.ensure(bytes) || !c->down.ensure(bytes)) { h->err = "allocation failed (key-frame match)"; return VILF_ERR_DEVICE; }
    char *b = c->res.as<char>();
    const KfMatchOut out{(unsigned char *)(b + o_st), (float2 *)(b + o_pt), (float2 *)(b + o_ptn), (int *)(b + o_idx), (int *)(b + o_dist), (int *)(b + o_cnt)};
    ProfMarks prof(h, c->prof);
    { const int rc = vilf_kf_match_enqueue(h, c, cur, n_old, old_index, out); if (rc != VILF_OK) return rc; }
    prof.mark(3);
    HIPCHECK(h, hipMemcpyAsync(c->down.p, b, bytes, hipMemcpyDeviceToHost, h->stream));      // one copy of the whole record, then the caller's arrays from the pinned image
    prof.mark(4);
    { const int rc = vilf_kf_finish(h); if (rc != VILF_OK) return rc; }
    const char *d = (const char *)c->down.p;
    if (rows && status) std::memcpy(status, d + o_st, rows);
    if (rows && pt_old) std::memcpy(pt_old, d + o_pt, rows * 8);
    if (rows && pt_old_norm) std::memcpy(pt_old_norm, d + o_ptn, rows * 8);
    if (rows && best_index) std::memcpy(best_index, d + o_idx, rows * 4);
    if (rows && best_dist) std::memcpy(best_dist, d + o_dist, rows * 4);
    if (n_matched) std::memcpy(n_matched, d + o_cnt, (size_t)n_old * 4);
    return VILF_OK;
}

extern "C" int vilf_kf_blur(vilf_handle *h, const unsigned char *img, int row_stride, unsigned char *out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    KfCtx *c = vilf_kf_ctx(h, "vilf_kf_blur");
    if (!c) return VILF_ERR_INVALID_ARGUMENT;
    if (!img || !out || row_stride < c->p.width) { h->err = "vilf_kf_blur: null pointer or row_stride < width"; return VILF_ERR_INVALID_ARGUMENT; }
    HIPCHECK(h, hipSetDevice(h->device));
    ProfMarks prof(h, c->prof);
    { const int rc = kf_upload(h, c, img, row_stride); if (rc != VILF_OK) return rc; }
    { const int rc = kf_run_blur(h, c); if (rc != VILF_OK) return rc; }
    prof.mark(0);
    HIPCHECK(h, hipMemcpyAsync(out, c->blur.p, c->ncell, hipMemcpyDeviceToHost, h->stream));
    prof.mark(4);
    return vilf_kf_finish(h);
}

extern "C" int vilf_kf_fast(vilf_handle *h, const unsigned char *img, int row_stride, int cap, float *pts_out, unsigned char *score_out, int *n_out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    KfCtx *c = vilf_kf_ctx(h, "vilf_kf_fast");
    if (!c) return VILF_ERR_INVALID_ARGUMENT;
    if (!img || !pts_out || !n_out || cap < 0 || row_stride < c->p.width) { h->err = "vilf_kf_fast: null pointer, cap < 0 or row_stride < width"; return VILF_ERR_INVALID_ARGUMENT; }
    HIPCHECK(h, hipSetDevice(h->device));
    ProfMarks prof(h, c->prof);
    { const int rc = kf_upload(h, c, img, row_stride); if (rc != VILF_OK) return rc; }
    prof.mark(0);
    int n = 0;
    { const int rc = kf_run_fast_count(h, c, &n); if (rc != VILF_OK) return rc; }
    if (n < 0 || n > cap) {
        if (h->profiling) vilf_prof_flush(h);
        h->err = "vilf_kf_fast: " + std::to_string(n) + " key points, room for " + std::to_string(cap);
        return VILF_ERR_INVALID_ARGUMENT;
    }
    const size_t sn = (size_t)std::max(n, 1);
    if (!c->tpts.ensure(sn * 8) || !c->tscore.ensure(sn)) { h->err = "hipMalloc failed (key points)"; return VILF_ERR_DEVICE; }
    { const int rc = kf_run_place(h, c, n, c->tpts.as<float2>(), c->tscore.as<unsigned char>()); if (rc != VILF_OK) return rc; }
    prof.mark(1);
    if (n > 0) HIPCHECK(h, hipMemcpyAsync(pts_out, c->tpts.p, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream));
    if (n > 0 && score_out) HIPCHECK(h, hipMemcpyAsync(score_out, c->tscore.p, (size_t)n, hipMemcpyDeviceToHost, h->stream));
    prof.mark(4);
    { const int rc = vilf_kf_finish(h); if (rc != VILF_OK) return rc; }
    *n_out = n;
    return VILF_OK;
}

extern "C" int vilf_kf_brief(vilf_handle *h, const unsigned char *img, int row_stride, const float *pts, int n, unsigned long long *desc_out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    KfCtx *c = vilf_kf_ctx(h, "vilf_kf_brief");
    if (!c) return VILF_ERR_INVALID_ARGUMENT;
    if (!img || n < 0 || n > KF_MAX_POINTS || (n > 0 && (!pts || !desc_out)) || row_stride < c->p.width) {
        h->err = "vilf_kf_brief: null pointer, n outside 0 .. 2^20 or row_stride < width"; return VILF_ERR_INVALID_ARGUMENT;
    }
    if (!kf_points_ok(pts, n)) { h->err = "vilf_kf_brief: a point is not finite or lies beyond 1e6 pixels"; return VILF_ERR_INVALID_ARGUMENT; }
    if (n == 0) return VILF_OK;
    HIPCHECK(h, hipSetDevice(h->device));
    if (!c->tpts.ensure((size_t)n * 8) || !c->tdesc.ensure((size_t)n * 32)) { h->err = "hipMalloc failed (descriptors)"; return VILF_ERR_DEVICE; }
    ProfMarks prof(h, c->prof);
    { const int rc = kf_upload(h, c, img, row_stride); if (rc != VILF_OK) return rc; }
    HIPCHECK(h, hipMemcpyAsync(c->tpts.p, pts, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    { const int rc = kf_run_blur(h, c); if (rc != VILF_OK) return rc; }
    prof.mark(0);
    { const int rc = kf_run_brief(h, c, c->tpts.as<float2>(), n, c->tdesc.as<unsigned long long>()); if (rc != VILF_OK) return rc; }
    prof.mark(2);
    HIPCHECK(h, hipMemcpyAsync(desc_out, c->tdesc.p, (size_t)n * 32, hipMemcpyDeviceToHost, h->stream));
    prof.mark(4);
    return vilf_kf_finish(h);
}

extern "C" int vilf_kf_profile(vilf_handle *h, double ms_out[5], long launches_out[5]) { return vilf_stage_profile(h, ST_KF, &KfCtx::prof, ms_out, launches_out); }
