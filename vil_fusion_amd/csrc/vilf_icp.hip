// vilf_icp.hip — ICP verification of a loop candidate of the global_fusion node on the device (≙ icpCalculation, global_fusion/poseGraphOptimization.cpp:376-443:
//   loopFindNearKeyframeCLoud :194-219 + pcl::VoxelGrid for the two sub-maps, pcl::IterativeClosestPoint, getFitnessScore). The semantics are stated once, in
//   include/vilfusion.h. The key-frame clouds stay in a device store sized at creation (IcpCtx); a call works on `segments`: segment 2 c is the source sub-map of
//   pair c, segment 2 c + 1 its target; a segment's place in every work array is fixed by its point count before the voxel filter, which the host knows.
//   icp_bbox        a workgroup per segment: the clouds of the sub-map (one contiguous range of the store) under the root's pose (or each under its own), the bounding box
//   icp_leaf_keys   a thread per point: key = segment << 40 | leaf index; the library's stable radix sort (vilf_sort.hip) then keeps concatenation order within a leaf
//   icp_voxel       a workgroup per segment: leaf heads ranked by a ballot scan, a thread per leaf sums its points in order; the target's search grid is sized here
//   icp_cell_keys, icp_cell_table   the target sorted by grid cell (x fastest) with a cell-start table: built once per pair, the target does not move
//   icp_search      (blocks of 256 source points, pair): moves the source by the step of the round before, nearest target point by growing shells of cells, per-block
//                   partial sums in fp64; round < 0 is the fitness pass
//   icp_step        a wave per pair: the blocks' partials in block order, Umeyama, 3 x 3 Jacobi SVD, the float composition, the convergence rules, the round's record
// One align call is ONE chain of launches (max_iterations x (icp_search, icp_step) + the fitness pass); the host waits once, at the end. A pair whose `done` flag is set
// makes the later launches of its grid row return at once. No floating-point atomics and no result that depends on which wave finishes first: partial sums have fixed
// places and are added in a fixed order, every minimum is lexicographic in (d2, target index).
// The global map (≙ publishGlobalMap :310-336) is built from the same store by kernels of its own, spread over the whole grid (a sub-map runs one workgroup per segment):
//   gmap_xf_bbox    a workgroup per chunk of one cloud (host table chunk -> cloud, first point, count, place): the points under their cloud's own pose, a min/max partial
//   gmap_box        one workgroup: the partials -> minb, divb, the overflow flag, by icp_bbox's rules
//   gmap_leaf_keys  a thread per point: key = leaf index, value = place in concatenation order; then the same stable radix sort
//   gmap_count, gmap_scan, gmap_centroids   leaf heads per block of sorted keys, the scan of the block counts, a thread per head: rank = block base + ballot rank,
//                   its run summed in sorted order (across block boundaries), the centroid written at `rank` of the map's own buffer
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>
#include "vilf_internal.hpp"
#include "vilf_device.hpp"
#include "vilf_kernels.hpp"
#include "vilf_sort.hpp"

#define ICP_LEAF_BITS 40               // leaf index of the voxel filter within a segment's key
#define ICP_GRID_MAX (1 << 18)         // cells of a target's search grid at most
#define ICP_CELL_BITS 19               // cell index within a segment's key; 1 << 18 = "not a target point", sorts behind every cell
#define ICP_MAX_SHELLS 6               // icp_search: shells of cells walked before the fallback scan of the whole target
#define ICP_NSUM 17                    // n, sum s (3), sum t (3), sum s t^T (9), sum d2
#define ICP_MAX_ITER 1000

struct IcpHdr {                        // per segment
    float mn[3], mx[3];                // bounding box of the transformed points
    int minb[3], divb[3];              // VoxelGrid: floor(min * inv), leaves per axis
    int n_in, n_out;                   // points before / after the voxel filter
    float cell, inv_cell;              // search grid over the same box (targets)
    int gd[3], ncells;
};
struct IcpState {                      // per pair
    int done, converged, criterion, iterations, n_corr, pad_;
    double mse_prev, mse, fitness;
    float fin[16], pend[16];           // final; the step the next icp_search applies to the source
};
struct IcpDev {
    const float4 *pts; const int *off; const float *mats;                  // the store, its cloud offsets, [size][12] pose matrices of this call
    const int *seg_p0, *seg_w0, *seg_root, *seg_lo, *seg_hi; int nseg;     // per segment: first store point, place in the work arrays ([nseg + 1]), root, cloud range
    float4 *tp, *vox, *cur, *tgs;                                          // transformed points; voxel centroids; the moving source; target sorted by cell (w = index bits)
    unsigned long long *k1, *k2; int *v1, *v2;
    IcpHdr *hdr; IcpState *st; int *cell_start; double *part; vilf_icp_iter *hist; int *nn_idx; float *nn_d2; int *flag;
    int own_pose, max_blocks, max_iter, W;
    float leaf;
    double max_d2, eps_t, eps_mse, rot_thres, mse_rel;
};

// ---- launch contract -----------------------------------------------------------------------------------------------------
#define ICP_SEG_NT 1024                // icp_bbox, icp_voxel: grid = segments
#define ICP_SEG_WAVES (ICP_SEG_NT / 64)
struct IcpSegShared { float mn[ICP_SEG_WAVES][3], mx[ICP_SEG_WAVES][3]; int wave_heads[ICP_SEG_WAVES]; int base; };
#define ICP_SEG_LDS_BYTES (ICP_SEG_WAVES * 6 * 4 + ICP_SEG_WAVES * 4 + 4)
static_assert(sizeof(IcpSegShared) == ICP_SEG_LDS_BYTES && ICP_SEG_LDS_BYTES <= VILF_LDS_CU_BYTES / 2, "icp_bbox / icp_voxel: 452 B");
#define ICP_PT_NT 256                  // icp_leaf_keys, icp_cell_keys, icp_cell_table: grid = ceil(W / 256), a thread per work element, no LDS
#define ICP_SRCH_NT 256                // icp_search: grid = (max_blocks, pairs)
#define ICP_SRCH_WAVES (ICP_SRCH_NT / 64)
struct IcpSearchShared { double w[ICP_SRCH_WAVES][ICP_NSUM]; };
#define ICP_SRCH_LDS_BYTES (ICP_SRCH_WAVES * ICP_NSUM * 8)
static_assert(sizeof(IcpSearchShared) == ICP_SRCH_LDS_BYTES && ICP_SRCH_LDS_BYTES <= VILF_LDS_CU_BYTES / 8, "icp_search: 544 B");
#define ICP_STEP_NT 64                 // icp_step: grid = pairs, one wave
struct IcpStepShared { double s[ICP_NSUM]; };
static_assert(sizeof(IcpStepShared) <= VILF_LDS_CU_BYTES / 8, "icp_step: 136 B");
struct GmapHdr { int minb[3], divb[3]; int n_in, n_out; };
struct GmapDev {
    const float4 *pts; const float *mats; const int4 *chunks;              // the store, [size][12] pose matrices, per chunk: cloud, first store point, count, first place
    float *part; int nchunks;                                              // [nchunks][6] min / max of a chunk
    float4 *tp, *map;                                                      // transformed points in concatenation order; the centroids in ascending leaf index
    unsigned long long *k1, *k2; int *v1, *v2;
    GmapHdr *hdr; int *bcount, *bbase, *flag;                              // heads per block of GM_RUN_NT sorted keys, their exclusive scan
    int W, nblk;
    float leaf;
};
#define GM_XF_NT 256                   // gmap_xf_bbox: grid = chunks, a chunk holds at most GM_CHUNK points of one cloud
#define GM_CHUNK 1024
#define GM_XF_WAVES (GM_XF_NT / 64)
struct GmapBoxShared { float mn[GM_XF_WAVES][3], mx[GM_XF_WAVES][3]; };    // gmap_box: grid = 1, the same block and LDS
#define GM_BOX_LDS_BYTES (GM_XF_WAVES * 6 * 4)
static_assert(sizeof(GmapBoxShared) == GM_BOX_LDS_BYTES && GM_BOX_LDS_BYTES <= VILF_LDS_CU_BYTES / 8, "gmap_xf_bbox / gmap_box: 96 B");
#define GM_RUN_NT 1024                 // gmap_count, gmap_centroids: grid = ceil(W / 1024), a thread per sorted key; gmap_scan: grid = 1, block counts in chunks of 1024
#define GM_RUN_WAVES (GM_RUN_NT / 64)
struct GmapRunShared { int wave[GM_RUN_WAVES]; };
#define GM_RUN_LDS_BYTES (GM_RUN_WAVES * 4)
static_assert(sizeof(GmapRunShared) == GM_RUN_LDS_BYTES && GM_RUN_LDS_BYTES <= VILF_LDS_CU_BYTES / 2, "gmap_count / gmap_scan / gmap_centroids: 64 B");
__global__ void gmap_xf_bbox(GmapDev G);                                   // gmap_leaf_keys: ICP_PT_NT, grid = ceil(W / 256), no LDS
__global__ void gmap_box(GmapDev G);
__global__ void gmap_leaf_keys(GmapDev G);
__global__ void gmap_count(GmapDev G);
__global__ void gmap_scan(GmapDev G);
__global__ void gmap_centroids(GmapDev G);
__global__ void icp_bbox(IcpDev D);
__global__ void icp_leaf_keys(IcpDev D);
__global__ void icp_voxel(IcpDev D);
__global__ void icp_cell_keys(IcpDev D);
__global__ void icp_cell_table(IcpDev D);
__global__ void icp_search(IcpDev D, int round);
__global__ void icp_step(IcpDev D, int round);

struct IcpCtx : VilfStage {
    vilf_icp_params p;
    int cap_kf = 0, size = 0;
    long cap_pts = 0;
    std::vector<int> off;              // [size + 1] host mirror of the cloud offsets
    DBuf pts, doff, mats, segs, tp, vox, cur, tgs, k1, k2, v1, v2, temp, hdr, st, cells, part, hist, nn_idx, nn_d2, flag;
    std::vector<int> h_segs;           // the last call's segment arrays (host)
    std::vector<float> h_mats;
    std::vector<IcpState> h_st;
    int last_n = 0, last_W = 0;        // pairs and work elements of the last align call (vilf_icp_get_history / get_search)
    StageProf<8> prof;
    DBuf gm_chunks, gm_part, gm_hdr, gm_bcount, gm_bbase, gm_map;      // the global map: gm_map is its own, no align or sub-map call writes it
    std::vector<int> h_chunks;
    bool gm_built = false;
    long gm_n = 0;
    StageProf<4> gm_prof;
    void profile_reset() override { prof.reset(); gm_prof.reset(); }
};

namespace {
// local2global (:185-187): ((m0 x + m1 y) + m2 z) + m3, every operation rounded on its own
VD float icp_row(const float *m, float x, float y, float z) { return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[0], x), __fmul_rn(m[1], y)), __fmul_rn(m[2], z)), m[3]); }
VD float4 icp_xf(const float *m, float4 p) { return make_float4(icp_row(m, p.x, p.y, p.z), icp_row(m + 4, p.x, p.y, p.z), icp_row(m + 8, p.x, p.y, p.z), p.w); }
// the segment of work element i: the last s with seg_w0[s] <= i
VD int icp_segment(const IcpDev &D, int i) {
    int a = 0, b = D.nseg;
    while (b - a > 1) { const int m = (a + b) >> 1; if (D.seg_w0[m] <= i) a = m; else b = m; }
    return a;
}
VD void icp_scan(const float4 *tg, int a, int b, float qx, float qy, float qz, float &bd, int &bi) {
    for (int j = a; j < b; j++) {
        const float4 t = tg[j];
        const float dx = __fsub_rn(qx, t.x), dy = __fsub_rn(qy, t.y), dz = __fsub_rn(qz, t.z);
        const float d = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
        const int idx = __float_as_int(t.w);
        if (d < bd || (d == bd && idx < bi)) { bd = d; bi = idx; }
    }
}
VD int icp_cell_of(float v, float mn, float inv, int n) { const float f = floorf((v - mn) * inv); return !(f > 0.f) ? 0 : (f >= (float)n ? n - 1 : (int)f); }
}  // namespace

// ---- icp_bbox: a workgroup per segment ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(ICP_SEG_NT) void icp_bbox(IcpDev D) {
    __shared__ IcpSegShared sh;
    const int s = blockIdx.x, t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int p0 = D.seg_p0[s], w0 = D.seg_w0[s], n = D.seg_w0[s + 1] - w0;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    const float *root = D.mats + 12 * (size_t)D.seg_root[s];
    for (int j = t; j < n; j += ICP_SEG_NT) {
        const float *m = root;
        if (D.own_pose) {              // the cloud store point p0 + j belongs to: the last k in [lo, hi] with off[k] <= p0 + j
            int a = D.seg_lo[s], b = D.seg_hi[s] + 1;
            while (b - a > 1) { const int k = (a + b) >> 1; if (D.off[k] <= p0 + j) a = k; else b = k; }
            m = D.mats + 12 * (size_t)a;
        }
        const float4 q = icp_xf(m, D.pts[(size_t)p0 + j]);
        D.tp[(size_t)w0 + j] = q;
        mn[0] = fminf(mn[0], q.x); mn[1] = fminf(mn[1], q.y); mn[2] = fminf(mn[2], q.z);
        mx[0] = fmaxf(mx[0], q.x); mx[1] = fmaxf(mx[1], q.y); mx[2] = fmaxf(mx[2], q.z);
    }
    for (int o = 32; o > 0; o >>= 1) for (int k = 0; k < 3; k++) { mn[k] = fminf(mn[k], __shfl_xor(mn[k], o)); mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], o)); }
    if (lane == 0) for (int k = 0; k < 3; k++) { sh.mn[wave][k] = mn[k]; sh.mx[wave][k] = mx[k]; }
    lds_barrier();
    if (t == 0) {
        IcpHdr *H = D.hdr + s;
        H->n_in = n; H->n_out = 0;
        const float inv = __fdiv_rn(1.0f, D.leaf);
        double leaves = 1.0;               // exact: a product of integers below 2^71 compared with 2^40
        for (int k = 0; k < 3; k++) {
            float a = sh.mn[0][k], b = sh.mx[0][k];
            for (int w = 1; w < ICP_SEG_WAVES; w++) { a = fminf(a, sh.mn[w][k]); b = fmaxf(b, sh.mx[w][k]); }
            if (n == 0) { a = 0.f; b = 0.f; }
            const float fa = floorf(__fmul_rn(a, inv)), fb = floorf(__fmul_rn(b, inv));
            const bool bad = !(fabsf(fa) < 1e9f && fabsf(fb) < 1e9f);      // a point that is not finite (the host rejects them; a pose could still make one) or an absurd extent
            if (bad) { a = 0.f; b = 0.f; }      // the call fails by the flag; everything downstream of the box stays finite and bounded
            H->mn[k] = a; H->mx[k] = b;
            H->minb[k] = bad ? 0 : (int)fa;
            H->divb[k] = bad ? 1 : (int)fb - (int)fa + 1;
            if (bad || leaves * (double)H->divb[k] >= (double)(1l << ICP_LEAF_BITS)) { D.flag[0] = 1; H->divb[k] = 1; } else leaves *= (double)H->divb[k];
        }
    }
}

// ---- icp_leaf_keys: a thread per point -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(ICP_PT_NT) void icp_leaf_keys(IcpDev D) {
    const int i = blockIdx.x * ICP_PT_NT + threadIdx.x;
    if (i >= D.W) return;
    const int s = icp_segment(D, i);
    const IcpHdr *H = D.hdr + s;
    const float4 q = D.tp[i];
    const float inv = __fdiv_rn(1.0f, D.leaf);
    long c[3];
    const float v[3] = {q.x, q.y, q.z};
    for (int k = 0; k < 3; k++) { long a = (long)floorf(__fmul_rn(v[k], inv)) - H->minb[k]; c[k] = a < 0 ? 0 : (a >= H->divb[k] ? H->divb[k] - 1 : a); }   // a clamp acts only after the overflow flag
    const unsigned long long leaf = (unsigned long long)(c[0] + c[1] * (long)H->divb[0] + c[2] * (long)H->divb[0] * (long)H->divb[1]);
    D.k1[i] = ((unsigned long long)s << ICP_LEAF_BITS) | leaf;
    D.v1[i] = i;
}

// ---- icp_voxel: a workgroup per segment -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(ICP_SEG_NT) void icp_voxel(IcpDev D) {
    __shared__ IcpSegShared sh;
    const int s = blockIdx.x, t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int w0 = D.seg_w0[s], n = D.seg_w0[s + 1] - w0;
    const unsigned long long *ks = D.k2 + w0;
    const int *vs = D.v2 + w0;
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += ICP_SEG_NT) {
        const int i = c0 + t;
        const bool head = i < n && (i == 0 || ks[i] != ks[i - 1]);
        const unsigned long long bal = __ballot(head);
        if (lane == 0) sh.wave_heads[wave] = __popcll(bal);
        lds_barrier();
        int before = 0, total = 0;
        for (int w = 0; w < ICP_SEG_WAVES; w++) { const int c = sh.wave_heads[w]; before += w < wave ? c : 0; total += c; }
        if (head) {
            const int rank = base + before + __popcll(bal & ((1ull << lane) - 1ull));
            const unsigned long long key = ks[i];
            float sx = 0.f, sy = 0.f, sz = 0.f, si = 0.f;
            int e = i;
            for (; e < n && ks[e] == key; e++) { const float4 p = D.tp[vs[e]]; sx = __fadd_rn(sx, p.x); sy = __fadd_rn(sy, p.y); sz = __fadd_rn(sz, p.z); si = __fadd_rn(si, p.w); }
            const float cnt = (float)(e - i);
            D.vox[(size_t)w0 + rank] = make_float4(__fdiv_rn(sx, cnt), __fdiv_rn(sy, cnt), __fdiv_rn(sz, cnt), __fdiv_rn(si, cnt));
        }
        base += total;
        lds_barrier();
    }
    if (t == 0) {
        IcpHdr *H = D.hdr + s;
        H->n_out = base;
        // the search grid over the same box: cells of 4 leaves, grown until the table fits. icp_bbox keeps the box finite and below 2e9 leaves a side, so 72 growths
        // suffice; the loop is bounded all the same and ends in one cell for the whole target (the search then scans it: slow, still exact)
        float cell = 4.0f * D.leaf;
        H->gd[0] = H->gd[1] = H->gd[2] = 1; H->ncells = 1;
        for (int grow = 0; grow < 128; grow++) {
            long nc = 1;
            int gd[3];
            for (int k = 0; k < 3; k++) { const float q = (H->mx[k] - H->mn[k]) / cell; gd[k] = (q >= 0.f && q < 1e6f ? (int)q : 1000000) + 1; nc *= gd[k]; }
            if (nc <= ICP_GRID_MAX) { for (int k = 0; k < 3; k++) H->gd[k] = gd[k]; H->ncells = (int)nc; break; }
            cell *= 1.25f;
        }
        if (!(cell > 0.f && cell < 1e30f)) cell = 1e30f;
        H->cell = cell; H->inv_cell = 1.0f / cell;
    }
}

// ---- icp_cell_keys / icp_cell_table: the target sorted by cell --------------------------------------------------------------------
__global__ __launch_bounds__(ICP_PT_NT) void icp_cell_keys(IcpDev D) {
    const int i = blockIdx.x * ICP_PT_NT + threadIdx.x;
    if (i >= D.W) return;
    const int s = icp_segment(D, i);
    const IcpHdr *H = D.hdr + s;
    unsigned long long cell = 1ull << (ICP_CELL_BITS - 1);
    if ((s & 1) && i - D.seg_w0[s] < H->n_out) {
        const float4 q = D.vox[i];
        const int cx = icp_cell_of(q.x, H->mn[0], H->inv_cell, H->gd[0]), cy = icp_cell_of(q.y, H->mn[1], H->inv_cell, H->gd[1]), cz = icp_cell_of(q.z, H->mn[2], H->inv_cell, H->gd[2]);
        cell = (unsigned long long)(cx + H->gd[0] * (cy + H->gd[1] * cz));
    }
    D.k1[i] = ((unsigned long long)s << ICP_CELL_BITS) | cell;
    D.v1[i] = i;
}

__global__ __launch_bounds__(ICP_PT_NT) void icp_cell_table(IcpDev D) {
    const int i = blockIdx.x * ICP_PT_NT + threadIdx.x;
    if (i >= D.W) return;
    const int s = icp_segment(D, i);
    if (!(s & 1)) return;
    const IcpHdr *H = D.hdr + s;
    const int w0 = D.seg_w0[s], p = i - w0, n = H->n_out;
    int *start = D.cell_start + (size_t)(s >> 1) * (ICP_GRID_MAX + 1);
    if (n == 0) { if (p == 0) for (int c = 0; c <= H->ncells; c++) start[c] = 0; return; }
    if (p >= n) return;
    const unsigned long long mask = (1ull << ICP_CELL_BITS) - 1;
    const int cell = (int)(D.k2[i] & mask), prev = p ? (int)(D.k2[i - 1] & mask) : -1;
    const int v = D.v2[i];
    const float4 q = D.vox[v];
    D.tgs[i] = make_float4(q.x, q.y, q.z, __int_as_float(v - w0));
    for (int c = prev + 1; c <= cell; c++) start[c] = p;
    if (p == n - 1) for (int c = cell + 1; c <= H->ncells; c++) start[c] = n;
}

// ---- icp_search: blocks of 256 source points of a pair ---------------------------------------------------------------------------------
__global__ __launch_bounds__(ICP_SRCH_NT) void icp_search(IcpDev D, int round) {
    __shared__ IcpSearchShared sh;
    const int c = blockIdx.y, t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const IcpState *S = D.st + c;
    if (round >= 0 && S->done) return;
    const IcpHdr *HS = D.hdr + 2 * c, *HT = D.hdr + 2 * c + 1;
    const int ns = HS->n_out, nt = HT->n_out, i = blockIdx.x * ICP_SRCH_NT + t;
    if ((int)blockIdx.x * ICP_SRCH_NT >= ns) return;
    const int ws = D.seg_w0[2 * c], wt = D.seg_w0[2 * c + 1];
    double v[ICP_NSUM];
    for (int k = 0; k < ICP_NSUM; k++) v[k] = 0.0;
    if (i < ns) {
        float m[12];
        for (int k = 0; k < 12; k++) m[k] = S->pend[k];
        const float4 q = icp_xf(m, round == 0 ? D.vox[(size_t)ws + i] : D.cur[(size_t)ws + i]);
        D.cur[(size_t)ws + i] = q;
        float bd = INFINITY;
        int bi = INT_MAX;
        if (nt > 0) {
            const float4 *tg = D.tgs + wt;
            const int *start = D.cell_start + (size_t)c * (ICP_GRID_MAX + 1);
            const int g0 = HT->gd[0], g1 = HT->gd[1], g2 = HT->gd[2];
            const int qx = icp_cell_of(q.x, HT->mn[0], HT->inv_cell, g0), qy = icp_cell_of(q.y, HT->mn[1], HT->inv_cell, g1), qz = icp_cell_of(q.z, HT->mn[2], HT->inv_cell, g2);
            bool found = false;
            // after the shells 0 .. r every point not yet seen is at least r cells away along some axis (also for a query outside the grid, whose cell is the
            // clamped one); 0.999: the cell of a point is computed in float
            for (int r = 0; r <= ICP_MAX_SHELLS; r++) {
                if (r >= 2) { const float lb = (float)(r - 1) * HT->cell * 0.999f; if (bi != INT_MAX && bd < lb * lb) { found = true; break; } }
                for (int cz = max(qz - r, 0); cz <= min(qz + r, g2 - 1); cz++) for (int cy = max(qy - r, 0); cy <= min(qy + r, g1 - 1); cy++) {
                    const int row = g0 * (cy + g1 * cz);
                    if (abs(cz - qz) == r || abs(cy - qy) == r) {       // a whole row of the shell: one range of the sorted target
                        const int x0 = max(qx - r, 0), x1 = min(qx + r, g0 - 1);
                        icp_scan(tg, start[row + x0], start[row + x1 + 1], q.x, q.y, q.z, bd, bi);
                    } else {
                        if (qx - r >= 0) icp_scan(tg, start[row + qx - r], start[row + qx - r + 1], q.x, q.y, q.z, bd, bi);
                        if (r > 0 && qx + r < g0) icp_scan(tg, start[row + qx + r], start[row + qx + r + 1], q.x, q.y, q.z, bd, bi);
                    }
                }
            }
            if (!found) { const float lb = (float)ICP_MAX_SHELLS * HT->cell * 0.999f; found = bi != INT_MAX && bd < lb * lb; }
            if (!found) icp_scan(tg, 0, nt, q.x, q.y, q.z, bd, bi);      // far from every target point: the whole target, still exact
        }
        if (round <= 0) { const size_t o = (size_t)(round < 0 ? D.W : 0) + ws + i; D.nn_idx[o] = bi == INT_MAX ? -1 : bi; D.nn_d2[o] = bd; }
        if (bi != INT_MAX) {
            if (round < 0) { v[0] = 1.0; v[16] = (double)bd; }
            else if ((double)bd <= D.max_d2) {
                const float4 tp = D.vox[(size_t)wt + bi];
                const double s3[3] = {(double)q.x, (double)q.y, (double)q.z}, t3[3] = {(double)tp.x, (double)tp.y, (double)tp.z};
                v[0] = 1.0;
                for (int k = 0; k < 3; k++) { v[1 + k] = s3[k]; v[4 + k] = t3[k]; for (int l = 0; l < 3; l++) v[7 + 3 * k + l] = __dmul_rn(s3[k], t3[l]); }
                v[16] = (double)bd;
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) for (int k = 0; k < ICP_NSUM; k++) v[k] = __dadd_rn(v[k], __shfl_xor(v[k], o));
    if (lane == 0) for (int k = 0; k < ICP_NSUM; k++) sh.w[wave][k] = v[k];
    lds_barrier();
    if (t < ICP_NSUM) {
        double a = sh.w[0][t];
        for (int w = 1; w < ICP_SRCH_WAVES; w++) a = __dadd_rn(a, sh.w[w][t]);
        D.part[((size_t)c * D.max_blocks + blockIdx.x) * ICP_NSUM + t] = a;
    }
}

// ---- icp_step: a wave per pair -------------------------------------------------------------------------------------------------
namespace {
// H = U diag V^T by one-sided Jacobi; returns R = U diag(1, 1, det U det V) V^T
__device__ void icp_rotation(const double Hm[3][3], double R[3][3]) {
    double A[3][3], V[3][3];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { A[i][j] = Hm[i][j]; V[i][j] = i == j ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 40; sweep++) {
        bool rotated = false;
        for (int p = 0; p < 2; p++) for (int q = p + 1; q < 3; q++) {
            double al = 0, be = 0, ga = 0;
            for (int i = 0; i < 3; i++) { al += A[i][p] * A[i][p]; be += A[i][q] * A[i][q]; ga += A[i][p] * A[i][q]; }
            if (fabs(ga) <= 1e-17 * sqrt(al * be) || ga == 0.0) continue;
            rotated = true;
            const double zeta = (be - al) / (2.0 * ga), tt = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta)), cs = 1.0 / sqrt(1.0 + tt * tt), sn = cs * tt;
            for (int i = 0; i < 3; i++) {
                const double ap = A[i][p], aq = A[i][q], vp = V[i][p], vq = V[i][q];
                A[i][p] = cs * ap - sn * aq; A[i][q] = sn * ap + cs * aq;
                V[i][p] = cs * vp - sn * vq; V[i][q] = sn * vp + cs * vq;
            }
        }
        if (!rotated) break;
    }
    double sg[3];
    int ord[3] = {0, 1, 2};
    for (int j = 0; j < 3; j++) sg[j] = sqrt(A[0][j] * A[0][j] + A[1][j] * A[1][j] + A[2][j] * A[2][j]);
    for (int a = 0; a < 2; a++) for (int b = 0; b < 2 - a; b++) if (sg[ord[b]] < sg[ord[b + 1]]) { const int x = ord[b]; ord[b] = ord[b + 1]; ord[b + 1] = x; }
    double u[3][3], vv[3][3];      // [column][row]
    for (int j = 0; j < 3; j++) for (int i = 0; i < 3; i++) vv[j][i] = V[i][ord[j]];
    for (int i = 0; i < 3; i++) u[0][i] = sg[ord[0]] > 0 ? A[i][ord[0]] / sg[ord[0]] : (i == 0 ? 1.0 : 0.0);
    if (sg[ord[1]] > 1e-300 * sg[ord[0]] && sg[ord[1]] > 0) for (int i = 0; i < 3; i++) u[1][i] = A[i][ord[1]] / sg[ord[1]];
    else {                          // rank one: any unit vector orthogonal to u0
        const int k = fabs(u[0][0]) <= fabs(u[0][1]) && fabs(u[0][0]) <= fabs(u[0][2]) ? 0 : (fabs(u[0][1]) <= fabs(u[0][2]) ? 1 : 2);
        double e[3] = {0, 0, 0}; e[k] = 1.0;
        const double d = u[0][k];
        double nn = 0;
        for (int i = 0; i < 3; i++) { u[1][i] = e[i] - d * u[0][i]; nn += u[1][i] * u[1][i]; }
        for (int i = 0; i < 3; i++) u[1][i] /= sqrt(nn);
    }
    // the third left vector as u0 x u1 (det U = +1): R does not depend on its sign, the factor below follows it
    u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1]; u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2]; u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
    const double detV = vv[0][0] * (vv[1][1] * vv[2][2] - vv[1][2] * vv[2][1]) - vv[0][1] * (vv[1][0] * vv[2][2] - vv[1][2] * vv[2][0]) + vv[0][2] * (vv[1][0] * vv[2][1] - vv[1][1] * vv[2][0]);
    const double d3 = detV < 0 ? -1.0 : 1.0;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R[i][j] = u[0][i] * vv[0][j] + u[1][i] * vv[1][j] + d3 * u[2][i] * vv[2][j];
}
}  // namespace

__global__ __launch_bounds__(ICP_STEP_NT) void icp_step(IcpDev D, int round) {
    __shared__ IcpStepShared sh;
    const int c = blockIdx.x, t = threadIdx.x;
    IcpState *S = D.st + c;
    if (round >= 0 && S->done) return;
    const int ns = D.hdr[2 * c].n_out, nb = (ns + ICP_SRCH_NT - 1) / ICP_SRCH_NT;
    if (t < ICP_NSUM) {
        double a = 0.0;
        for (int b = 0; b < nb; b++) a = __dadd_rn(a, D.part[((size_t)c * D.max_blocks + b) * ICP_NSUM + t]);
        sh.s[t] = a;
    }
    lds_barrier();
    if (t != 0) return;
    const double n = sh.s[0];
    if (round < 0) { S->fitness = n > 0 ? sh.s[16] / n : DBL_MAX; return; }
    vilf_icp_iter *rec = D.hist + (size_t)c * D.max_iter + round;
    rec->n_correspondences = (int)n; rec->criterion = VILF_ICP_NONE; rec->mse = 0; rec->cos_angle = 0; rec->translation_sqr = 0;
    S->n_corr = (int)n;
    if (n < 3.0) {
        rec->criterion = VILF_ICP_NO_CORRESPONDENCES;
        S->done = 1; S->converged = 0; S->criterion = VILF_ICP_NO_CORRESPONDENCES;
        for (int k = 0; k < 16; k++) S->pend[k] = (k % 5 == 0) ? 1.f : 0.f;
        return;
    }
    double ms[3], mt[3], Hm[3][3], R[3][3];
    for (int k = 0; k < 3; k++) { ms[k] = sh.s[1 + k] / n; mt[k] = sh.s[4 + k] / n; }
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Hm[i][j] = sh.s[7 + 3 * j + i] / n - mt[i] * ms[j];      // sum t s^T / n - mean_t mean_s^T
    icp_rotation(Hm, R);
    float T[16];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) T[4 * i + j] = (float)R[i][j];
        T[4 * i + 3] = (float)(mt[i] - (R[i][0] * ms[0] + R[i][1] * ms[1] + R[i][2] * ms[2]));
    }
    T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
    float F[16];
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++)
        F[4 * i + j] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[4 * i], S->fin[j]), __fmul_rn(T[4 * i + 1], S->fin[4 + j])), __fmul_rn(T[4 * i + 2], S->fin[8 + j])), __fmul_rn(T[4 * i + 3], S->fin[12 + j]));
    for (int k = 0; k < 16; k++) { S->fin[k] = F[k]; S->pend[k] = T[k]; }
    const int it = ++S->iterations;
    const double mse = sh.s[16] / n, cosa = 0.5 * ((((double)T[0] + (double)T[5]) + (double)T[10]) - 1.0);
    const double tsq = ((double)T[3] * (double)T[3] + (double)T[7] * (double)T[7]) + (double)T[11] * (double)T[11];
    const double prev = S->mse_prev, dm = fabs(mse - prev);
    int crit = VILF_ICP_NONE;
    if (it >= D.max_iter) crit = VILF_ICP_ITERATIONS;
    else if (cosa >= D.rot_thres && tsq <= D.eps_t) crit = VILF_ICP_TRANSFORM;
    else if (dm < D.eps_mse) crit = VILF_ICP_ABS_MSE;
    else if (dm / prev < D.mse_rel) crit = VILF_ICP_REL_MSE;
    S->mse_prev = mse; S->mse = mse;
    rec->mse = mse; rec->cos_angle = cosa; rec->translation_sqr = tsq; rec->criterion = crit;
    if (crit != VILF_ICP_NONE) { S->done = 1; S->converged = 1; S->criterion = crit; }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
namespace {
// pcl::getTransformation as a float affine, rows of [R | t] (vilfusion.h)
void icp_pose_matrix(const double *p6, float *m) {
    const float x = (float)p6[0], y = (float)p6[1], z = (float)p6[2], roll = (float)p6[3], pitch = (float)p6[4], yaw = (float)p6[5];
    const float A = (float)std::cos((double)yaw), B = (float)std::sin((double)yaw), C = (float)std::cos((double)pitch), D = (float)std::sin((double)pitch);
    const float E = (float)std::cos((double)roll), F = (float)std::sin((double)roll);
    // volatile: every product is rounded before it is added (the host compiler may contract otherwise)
    volatile float DE = D * E, DF = D * F;
    volatile float a_df = A * DF, b_e = B * E, b_f = B * F, a_de = A * DE, a_e = A * E, b_df = B * DF, b_de = B * DE, a_f = A * F;
    m[0] = A * C; m[1] = a_df - b_e; m[2] = b_f + a_de; m[3] = x;
    m[4] = B * C; m[5] = a_e + b_df; m[6] = b_de - a_f; m[7] = y;
    m[8] = -D; m[9] = C * F; m[10] = C * E; m[11] = z;
}
void icp_guess_matrix(const double *qt, float *T) {
    for (int k = 0; k < 16; k++) T[k] = (k % 5 == 0) ? 1.f : 0.f;
    if (!qt) return;
    const double nrm = std::sqrt(qt[0] * qt[0] + qt[1] * qt[1] + qt[2] * qt[2] + qt[3] * qt[3]);
    const double x = qt[0] / nrm, y = qt[1] / nrm, z = qt[2] / nrm, w = qt[3] / nrm;
    const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                         2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) T[4 * i + j] = (float)R[3 * i + j]; T[4 * i + 3] = (float)qt[4 + i]; }
}
// getTranslationAndEulerAngles + Rot3::RzRyRx
void icp_result_pose(const float *T, double *pose6, double *qt) {
    const float roll = (float)std::atan2((double)T[9], (double)T[10]), pitch = (float)std::asin(std::max(-1.0, std::min(1.0, -(double)T[8]))), yaw = (float)std::atan2((double)T[4], (double)T[0]);
    pose6[0] = T[3]; pose6[1] = T[7]; pose6[2] = T[11]; pose6[3] = roll; pose6[4] = pitch; pose6[5] = yaw;
    const double cr = std::cos(0.5 * roll), sr = std::sin(0.5 * roll), cp = std::cos(0.5 * pitch), sp = std::sin(0.5 * pitch), cy = std::cos(0.5 * yaw), sy = std::sin(0.5 * yaw);
    double q[4] = {sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy};
    if (q[3] < 0) for (double &v : q) v = -v;
    for (int k = 0; k < 4; k++) qt[k] = q[k];
    qt[4] = T[3]; qt[5] = T[7]; qt[6] = T[11];
}
struct IcpSegHost { int key, half, root; };
inline int icp_bits(unsigned long long v) { int b = 1; while ((v >> b) && b < 63) b++; return b; }
}  // namespace

extern "C" void vilf_icp_default_params(vilf_icp_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->max_correspondence_distance = 100.0; p->max_iterations = 100; p->history_keyframes = 25; p->transformation_epsilon = 1e-6; p->euclidean_fitness_epsilon = 1e-6;
    p->rotation_threshold = 0.99999; p->mse_relative = 1e-5; p->fitness_threshold = 0.3; p->leaf_size = 0.4; p->own_pose = 0;
}

extern "C" int vilf_icp_create(vilf_handle *h, const vilf_icp_params *p, int cap_keyframes, long cap_points) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    vilf_icp_params d;
    vilf_icp_default_params(&d);
    if (p) d = *p;
    if (cap_keyframes < 1 || cap_points < 1 || cap_points > INT_MAX / 2) { h->err = "vilf_icp_create: capacities must be positive (points below 2^30)"; return VILF_ERR_INVALID_ARGUMENT; }
    if (!(d.max_correspondence_distance > 0) || d.max_iterations < 1 || d.max_iterations > ICP_MAX_ITER || d.history_keyframes < 0 || !(d.leaf_size > 0) || !std::isfinite(d.leaf_size) ||
        std::isnan(d.transformation_epsilon) || std::isnan(d.euclidean_fitness_epsilon) || std::isnan(d.rotation_threshold) || std::isnan(d.mse_relative) || std::isnan(d.fitness_threshold)) {
        h->err = "vilf_icp_create: max_correspondence_distance > 0, 1 <= max_iterations <= 1000, history_keyframes >= 0, leaf_size > 0";
        return VILF_ERR_INVALID_ARGUMENT;
    }
    HIPCHECK(h, hipSetDevice(h->device));
    HIPCHECK(h, hipStreamSynchronize(h->stream));
    vilf_stage_drop(h, ST_ICP);
    IcpCtx *c = new IcpCtx();
    c->p = d; c->cap_kf = cap_keyframes; c->cap_pts = cap_points;
    c->off.assign(1, 0);
    if (!c->pts.ensure((size_t)cap_points * 16) || !c->doff.ensure(((size_t)cap_keyframes + 1) * 4) || !c->mats.ensure((size_t)cap_keyframes * 48) || !c->flag.ensure(4)) {
        delete c;
        h->err = "hipMalloc failed (ICP cloud store)";
        return VILF_ERR_DEVICE;
    }
    h->stage[ST_ICP] = c;
    return VILF_OK;
}

extern "C" int vilf_icp_add_clouds(vilf_handle *h, int n, const float *xyzi, const int *offsets, int *first_index_out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    IcpCtx *c = vilf_stage<IcpCtx>(h, ST_ICP);
    if (!c) { h->err = "vilf_icp_add_clouds: no store (vilf_icp_create)"; return VILF_ERR_INVALID_ARGUMENT; }
    if (n < 0 || !offsets || offsets[0] < 0) { h->err = "vilf_icp_add_clouds: bad arguments"; return VILF_ERR_INVALID_ARGUMENT; }
    for (int i = 0; i < n; i++) if (offsets[i + 1] < offsets[i]) { h->err = "vilf_icp_add_clouds: offsets must not decrease"; return VILF_ERR_INVALID_ARGUMENT; }
    const long total = (long)offsets[n] - offsets[0];
    if (total > 0 && !xyzi) { h->err = "vilf_icp_add_clouds: null cloud"; return VILF_ERR_INVALID_ARGUMENT; }
    for (size_t i = 4 * (size_t)offsets[0]; i < 4 * (size_t)offsets[n]; i++)
        if (!std::isfinite(xyzi[i])) { h->err = "vilf_icp_add_clouds: point " + std::to_string(i / 4) + " is not finite"; return VILF_ERR_INVALID_ARGUMENT; }
    const long have = c->off.back();
    if (c->size + (long)n > c->cap_kf || have + total > c->cap_pts) {
        h->err = "vilf_icp_add_clouds: " + std::to_string(c->size) + " + " + std::to_string(n) + " key frames / " + std::to_string(have) + " + " + std::to_string(total) +
                 " points exceed the capacity " + std::to_string(c->cap_kf) + " / " + std::to_string(c->cap_pts);
        return VILF_ERR_UNSUPPORTED;
    }
    if (first_index_out) *first_index_out = c->size;
    if (n == 0) return VILF_OK;
    HIPCHECK(h, hipSetDevice(h->device));
    if (total > 0) HIPCHECK(h, vilf_copy_sync(h, c->pts.as<float4>() + have, xyzi + 4 * (size_t)offsets[0], (size_t)total * 16, hipMemcpyHostToDevice));
    for (int i = 0; i < n; i++) c->off.push_back((int)(have + offsets[i + 1] - offsets[0]));
    c->size += n;
    HIPCHECK(h, vilf_copy_sync(h, c->doff.p, c->off.data(), c->off.size() * 4, hipMemcpyHostToDevice));
    return VILF_OK;
}

extern "C" int vilf_icp_add_cloud(vilf_handle *h, const float *xyzi, int n, int *index_out) {
    if (n < 0) { if (h) h->err = "vilf_icp_add_cloud: negative point count"; return VILF_ERR_INVALID_ARGUMENT; }
    const int off[2] = {0, n};
    return vilf_icp_add_clouds(h, 1, xyzi, off, index_out);
}

extern "C" int vilf_icp_size(vilf_handle *h, int *n_out) {
    if (!h || !n_out) return VILF_ERR_INVALID_ARGUMENT;
    const IcpCtx *c = vilf_stage<IcpCtx>(h, ST_ICP);
    *n_out = c ? c->size : 0;
    return VILF_OK;
}

// segments -> voxel-filtered sub-maps in D.vox; with_icp: the pairs' grids, rounds and fitness behind them, in the same chain. The host does not wait in here.
static int icp_enqueue(vilf_handle *h, IcpCtx *c, const std::vector<IcpSegHost> &segs, const double *poses6, const double *guess_qt, bool with_icp, IcpDev &D) {
    const int nseg = (int)segs.size(), npair = nseg / 2;
    for (size_t i = 0; i < 6 * (size_t)c->size; i++) if (!std::isfinite(poses6[i])) { h->err = "vilf_icp: the pose of key frame " + std::to_string(i / 6) + " is not finite"; return VILF_ERR_INVALID_ARGUMENT; }
    if (with_icp && guess_qt) for (int i = 0; i < npair; i++) {
        const double *g = guess_qt + 7 * (size_t)i;
        bool fin = true;
        for (int k = 0; k < 7; k++) fin = fin && std::isfinite(g[k]);
        if (!fin || !(g[0] * g[0] + g[1] * g[1] + g[2] * g[2] + g[3] * g[3] > 0)) { h->err = "vilf_icp: the guess of pair " + std::to_string(i) + " is not finite or has a zero quaternion"; return VILF_ERR_INVALID_ARGUMENT; }
    }
    std::vector<int> &hs = c->h_segs;
    hs.assign((size_t)5 * nseg + 1, 0);
    int *p0 = hs.data(), *w0 = p0 + nseg, *root = w0 + nseg + 1, *lo = root + nseg, *hi = lo + nseg;
    long W = 0;
    int max_src = 0;
    for (int s = 0; s < nseg; s++) {
        const int a = std::max(segs[s].key - segs[s].half, 0), b = std::min((long)segs[s].key + segs[s].half, (long)c->size - 1);
        lo[s] = a; hi[s] = b; root[s] = segs[s].root;
        p0[s] = b >= a ? c->off[a] : 0;
        w0[s] = (int)W;
        const int cnt = b >= a ? c->off[b + 1] - c->off[a] : 0;
        W += cnt;
        if (!(s & 1)) max_src = std::max(max_src, cnt);
        if (W > INT_MAX / 2) { h->err = "vilf_icp: the sub-maps of one call hold more than 2^30 points"; return VILF_ERR_UNSUPPORTED; }
    }
    w0[nseg] = (int)W;
    c->h_mats.resize((size_t)c->size * 12);
    for (int k = 0; k < c->size; k++) icp_pose_matrix(poses6 + 6 * (size_t)k, c->h_mats.data() + 12 * (size_t)k);
    const size_t Wn = std::max<long>(W, 1), tb = vilf_sort_temp_bytes(Wn, 8);
    const int max_blocks = std::max(1, (max_src + ICP_SRCH_NT - 1) / ICP_SRCH_NT);
    HIPCHECK(h, hipSetDevice(h->device));
    bool ok = c->segs.ensure(hs.size() * 4) && c->tp.ensure(Wn * 16) && c->vox.ensure(Wn * 16) && c->k1.ensure(Wn * 8) && c->k2.ensure(Wn * 8) && c->v1.ensure(Wn * 4) &&
              c->v2.ensure(Wn * 4) && c->temp.ensure(tb + 256) && c->hdr.ensure((size_t)nseg * sizeof(IcpHdr));
    if (with_icp) ok = ok && c->cur.ensure(Wn * 16) && c->tgs.ensure(Wn * 16) && c->st.ensure((size_t)npair * sizeof(IcpState)) && c->cells.ensure((size_t)npair * (ICP_GRID_MAX + 1) * 4) &&
                       c->part.ensure((size_t)npair * max_blocks * ICP_NSUM * 8) && c->hist.ensure((size_t)npair * c->p.max_iterations * sizeof(vilf_icp_iter)) &&
                       c->nn_idx.ensure(2 * Wn * 4) && c->nn_d2.ensure(2 * Wn * 4);
    if (!ok) { h->err = "hipMalloc failed (ICP work arrays)"; return VILF_ERR_DEVICE; }
    HIPCHECK(h, hipMemcpyAsync(c->segs.p, hs.data(), hs.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(h, hipMemcpyAsync(c->mats.p, c->h_mats.data(), c->h_mats.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(h, hipMemsetAsync(c->flag.p, 0, 4, h->stream));
    const int *ds = c->segs.as<int>();
    D = IcpDev{c->pts.as<float4>(), c->doff.as<int>(), c->mats.as<float>(), ds, ds + nseg, ds + 2 * nseg + 1, ds + 3 * nseg + 1, ds + 4 * nseg + 1, nseg,
               c->tp.as<float4>(), c->vox.as<float4>(), c->cur.as<float4>(), c->tgs.as<float4>(), c->k1.as<unsigned long long>(), c->k2.as<unsigned long long>(), c->v1.as<int>(), c->v2.as<int>(),
               c->hdr.as<IcpHdr>(), c->st.as<IcpState>(), c->cells.as<int>(), c->part.as<double>(), c->hist.as<vilf_icp_iter>(), c->nn_idx.as<int>(), c->nn_d2.as<float>(), c->flag.as<int>(),
               c->p.own_pose, max_blocks, c->p.max_iterations, (int)W, (float)c->p.leaf_size,
               c->p.max_correspondence_distance * c->p.max_correspondence_distance, c->p.transformation_epsilon, c->p.euclidean_fitness_epsilon, c->p.rotation_threshold, c->p.mse_relative};
    ProfMarks prof(h, c->prof);
    const dim3 gw((unsigned)((Wn + ICP_PT_NT - 1) / ICP_PT_NT));
    hipLaunchKernelGGL(icp_bbox, dim3(nseg), dim3(ICP_SEG_NT), 0, h->stream, D); prof.mark(0);
    hipLaunchKernelGGL(icp_leaf_keys, gw, dim3(ICP_PT_NT), 0, h->stream, D); prof.mark(1);
    if (W > 0 && vilf_sort_pairs_u64(h->stream, c->temp.p, c->temp.cap, D.k1, D.k2, D.v1, D.v2, (size_t)W, ICP_LEAF_BITS + icp_bits((unsigned long long)nseg)) != 0) { h->err = "vilf_icp: radix sort failed"; return VILF_ERR_DEVICE; }
    prof.mark(2);
    hipLaunchKernelGGL(icp_voxel, dim3(nseg), dim3(ICP_SEG_NT), 0, h->stream, D); prof.mark(3);
    if (with_icp) {
        std::vector<IcpState> &st = c->h_st;
        st.resize((size_t)npair);
        for (int i = 0; i < npair; i++) {
            std::memset(&st[i], 0, sizeof(IcpState));
            st[i].mse_prev = DBL_MAX; st[i].fitness = DBL_MAX;
            icp_guess_matrix(guess_qt ? guess_qt + 7 * (size_t)i : nullptr, st[i].fin);
            std::memcpy(st[i].pend, st[i].fin, sizeof(st[i].fin));
        }
        HIPCHECK(h, hipMemcpyAsync(c->st.p, st.data(), st.size() * sizeof(IcpState), hipMemcpyHostToDevice, h->stream));
        prof = ProfMarks(h, c->prof);      // the states' upload belongs to no slot
        hipLaunchKernelGGL(icp_cell_keys, gw, dim3(ICP_PT_NT), 0, h->stream, D); prof.mark(4);
        if (W > 0 && vilf_sort_pairs_u64(h->stream, c->temp.p, c->temp.cap, D.k1, D.k2, D.v1, D.v2, (size_t)W, ICP_CELL_BITS + icp_bits((unsigned long long)nseg)) != 0) { h->err = "vilf_icp: radix sort failed"; return VILF_ERR_DEVICE; }
        prof.mark(2);
        hipLaunchKernelGGL(icp_cell_table, gw, dim3(ICP_PT_NT), 0, h->stream, D); prof.mark(4);
        for (int r = 0; r < c->p.max_iterations; r++) {
            hipLaunchKernelGGL(icp_search, dim3(max_blocks, npair), dim3(ICP_SRCH_NT), 0, h->stream, D, r); prof.mark(5);
            hipLaunchKernelGGL(icp_step, dim3(npair), dim3(ICP_STEP_NT), 0, h->stream, D, r); prof.mark(6);
        }
        hipLaunchKernelGGL(icp_search, dim3(max_blocks, npair), dim3(ICP_SRCH_NT), 0, h->stream, D, -1); prof.mark(5);
        hipLaunchKernelGGL(icp_step, dim3(npair), dim3(ICP_STEP_NT), 0, h->stream, D, -1); prof.mark(6);
    }
    HIPCHECK(h, hipGetLastError());
    return VILF_OK;
}

static int icp_finish(vilf_handle *h, IcpCtx *c) {
    int flag = 0;
    HIPCHECK(h, vilf_copy_sync(h, &flag, c->flag.p, 4, hipMemcpyDeviceToHost));
    if (h->profiling) { const int rcf = vilf_prof_flush(h); if (rcf != VILF_OK) return rcf; }
    if (flag) { h->err = "vilf_icp: a sub-map's bounding box holds 2^40 leaves or more (or a point that is not finite)"; return VILF_ERR_UNSUPPORTED; }
    return VILF_OK;
}

extern "C" int vilf_icp_submap(vilf_handle *h, int key, int submap_size, int root, const double *poses6, float *xyzi_out, int cap, int *n_out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    IcpCtx *c = vilf_stage<IcpCtx>(h, ST_ICP);
    if (!c || !poses6 || !n_out || cap < 0 || (cap > 0 && !xyzi_out)) { h->err = "vilf_icp_submap: no store (vilf_icp_create) or null argument"; return VILF_ERR_INVALID_ARGUMENT; }
    if (key < 0 || key >= c->size || root < 0 || root >= c->size || submap_size < 0) { h->err = "vilf_icp_submap: key or root outside the store"; return VILF_ERR_INVALID_ARGUMENT; }
    c->last_n = 0;
    IcpDev D;
    int rc = icp_enqueue(h, c, {IcpSegHost{key, submap_size, root}}, poses6, nullptr, false, D);
    if (rc != VILF_OK) return rc;
    rc = icp_finish(h, c);
    if (rc != VILF_OK) return rc;
    IcpHdr H;
    HIPCHECK(h, vilf_copy_sync(h, &H, c->hdr.p, sizeof(H), hipMemcpyDeviceToHost));
    *n_out = H.n_out;
    const int m = std::min(cap, H.n_out);
    if (m > 0) HIPCHECK(h, vilf_copy_sync(h, xyzi_out, c->vox.p, (size_t)m * 16, hipMemcpyDeviceToHost));
    return VILF_OK;
}

extern "C" int vilf_icp_align_pairs(vilf_handle *h, int n, const int *prev, const int *curr, const double *poses6, const double *guess_qt, vilf_icp_result *out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    IcpCtx *c = vilf_stage<IcpCtx>(h, ST_ICP);
    if (!c) { h->err = "vilf_icp_align: no store (vilf_icp_create)"; return VILF_ERR_INVALID_ARGUMENT; }
    if (n < 0 || (n > 0 && (!prev || !curr || !poses6 || !out))) { h->err = "vilf_icp_align: null argument"; return VILF_ERR_INVALID_ARGUMENT; }
    if (n > 32767) { h->err = "vilf_icp_align_pairs: at most 32767 pairs in one call"; return VILF_ERR_UNSUPPORTED; }
    for (int i = 0; i < n; i++) if (prev[i] < 0 || prev[i] >= c->size || curr[i] < 0 || curr[i] >= c->size) { h->err = "vilf_icp_align: key frame outside the store"; return VILF_ERR_INVALID_ARGUMENT; }
    if (n == 0) return VILF_OK;
    std::vector<IcpSegHost> segs;
    for (int i = 0; i < n; i++) { segs.push_back(IcpSegHost{curr[i], 0, prev[i]}); segs.push_back(IcpSegHost{prev[i], c->p.history_keyframes, prev[i]}); }
    c->last_n = 0;
    IcpDev D;
    int rc = icp_enqueue(h, c, segs, poses6, guess_qt, true, D);
    if (rc != VILF_OK) return rc;
    rc = icp_finish(h, c);
    if (rc != VILF_OK) return rc;
    std::vector<IcpState> st((size_t)n);
    std::vector<IcpHdr> hd((size_t)2 * n);
    HIPCHECK(h, hipMemcpyAsync(st.data(), c->st.p, st.size() * sizeof(IcpState), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(h, vilf_copy_sync(h, hd.data(), c->hdr.p, hd.size() * sizeof(IcpHdr), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) {
        vilf_icp_result *r = out + i;
        std::memset(r, 0, sizeof(*r));
        r->converged = st[i].converged; r->criterion = st[i].criterion; r->iterations = st[i].iterations;
        r->n_source = hd[2 * i].n_out; r->n_target = hd[2 * i + 1].n_out; r->n_correspondences = st[i].n_corr;
        r->fitness = st[i].fitness; r->final_mse = st[i].mse;
        r->accepted = r->converged && r->fitness <= c->p.fitness_threshold;
        std::memcpy(r->transform, st[i].fin, sizeof(r->transform));
        icp_result_pose(r->transform, r->pose6, r->pose_qt);
    }
    c->last_n = n; c->last_W = D.W;
    return VILF_OK;
}

extern "C" int vilf_icp_align(vilf_handle *h, int prev, int curr, const double *poses6, const double *guess_qt, vilf_icp_result *out) {
    return vilf_icp_align_pairs(h, 1, &prev, &curr, poses6, guess_qt, out);
}

extern "C" int vilf_icp_get_history(vilf_handle *h, int pair, vilf_icp_iter *out, int cap, int *n_out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    IcpCtx *c = vilf_stage<IcpCtx>(h, ST_ICP);
    if (!c || !n_out || cap < 0 || (cap > 0 && !out) || pair < 0 || pair >= c->last_n) { h->err = "vilf_icp_get_history: no align call before, or pair out of range"; return VILF_ERR_INVALID_ARGUMENT; }
    HIPCHECK(h, hipSetDevice(h->device));
    IcpState st;
    HIPCHECK(h, vilf_copy_sync(h, &st, c->st.as<IcpState>() + pair, sizeof(st), hipMemcpyDeviceToHost));
    const int rounds = st.iterations + (st.criterion == VILF_ICP_NO_CORRESPONDENCES ? 1 : 0);      // the round that found too few pairs has a record, not a step
    *n_out = rounds;
    const int m = std::min(cap, rounds);
    if (m > 0) HIPCHECK(h, vilf_copy_sync(h, out, c->hist.as<vilf_icp_iter>() + (size_t)pair * c->p.max_iterations, (size_t)m * sizeof(vilf_icp_iter), hipMemcpyDeviceToHost));
    return VILF_OK;
}

extern "C" int vilf_icp_get_search(vilf_handle *h, int pair, int which, int *index_out, float *d2_out, int cap, int *n_out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    IcpCtx *c = vilf_stage<IcpCtx>(h, ST_ICP);
    if (!c || !n_out || cap < 0 || pair < 0 || pair >= c->last_n || which < 0 || which > 1) { h->err = "vilf_icp_get_search: no align call before, or pair out of range"; return VILF_ERR_INVALID_ARGUMENT; }
    HIPCHECK(h, hipSetDevice(h->device));
    IcpHdr H;
    HIPCHECK(h, vilf_copy_sync(h, &H, c->hdr.as<IcpHdr>() + 2 * pair, sizeof(H), hipMemcpyDeviceToHost));
    *n_out = H.n_out;
    const int m = std::min(cap, H.n_out);
    const size_t o = (size_t)(which ? c->last_W : 0) + c->h_segs[(size_t)(c->h_segs.size() - 1) / 5 + 2 * pair];      // seg_w0 of the source segment
    if (m > 0 && index_out) HIPCHECK(h, vilf_copy_sync(h, index_out, c->nn_idx.as<int>() + o, (size_t)m * 4, hipMemcpyDeviceToHost));
    if (m > 0 && d2_out) HIPCHECK(h, vilf_copy_sync(h, d2_out, c->nn_d2.as<float>() + o, (size_t)m * 4, hipMemcpyDeviceToHost));
    return VILF_OK;
}

extern "C" int vilf_get_profile_icp(vilf_handle *h, double ms_out[8], long launches_out[8]) { return vilf_stage_profile(h, ST_ICP, &IcpCtx::prof, ms_out, launches_out); }

// ---- the global map (≙ publishGlobalMap :310-336) -----------------------------------------------------------------------------------
__global__ __launch_bounds__(GM_XF_NT) void gmap_xf_bbox(GmapDev G) {
    __shared__ GmapBoxShared sh;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int4 ch = G.chunks[blockIdx.x];              // x: cloud, y: first store point, z: count (<= GM_CHUNK), w: first place
    float m[12];
    for (int k = 0; k < 12; k++) m[k] = G.mats[12 * (size_t)ch.x + k];
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int j = t; j < ch.z; j += GM_XF_NT) {
        const float4 q = icp_xf(m, G.pts[(size_t)ch.y + j]);
        G.tp[(size_t)ch.w + j] = q;
        mn[0] = fminf(mn[0], q.x); mn[1] = fminf(mn[1], q.y); mn[2] = fminf(mn[2], q.z);
        mx[0] = fmaxf(mx[0], q.x); mx[1] = fmaxf(mx[1], q.y); mx[2] = fmaxf(mx[2], q.z);
    }
    for (int o = 32; o > 0; o >>= 1) for (int k = 0; k < 3; k++) { mn[k] = fminf(mn[k], __shfl_xor(mn[k], o)); mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], o)); }
    if (lane == 0) for (int k = 0; k < 3; k++) { sh.mn[wave][k] = mn[k]; sh.mx[wave][k] = mx[k]; }
    lds_barrier();
    if (t < 3) {
        float a = sh.mn[0][t], b = sh.mx[0][t];
        for (int w = 1; w < GM_XF_WAVES; w++) { a = fminf(a, sh.mn[w][t]); b = fmaxf(b, sh.mx[w][t]); }
        G.part[6 * (size_t)blockIdx.x + t] = a; G.part[6 * (size_t)blockIdx.x + 3 + t] = b;
    }
}

// the chunks' partials -> the box; the tail is icp_bbox's. Minimum and maximum do not depend on the order they are taken in.
__global__ __launch_bounds__(GM_XF_NT) void gmap_box(GmapDev G) {
    __shared__ GmapBoxShared sh;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int c = t; c < G.nchunks; c += GM_XF_NT) for (int k = 0; k < 3; k++) { mn[k] = fminf(mn[k], G.part[6 * (size_t)c + k]); mx[k] = fmaxf(mx[k], G.part[6 * (size_t)c + 3 + k]); }
    for (int o = 32; o > 0; o >>= 1) for (int k = 0; k < 3; k++) { mn[k] = fminf(mn[k], __shfl_xor(mn[k], o)); mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], o)); }
    if (lane == 0) for (int k = 0; k < 3; k++) { sh.mn[wave][k] = mn[k]; sh.mx[wave][k] = mx[k]; }
    lds_barrier();
    if (t == 0) {
        GmapHdr *H = G.hdr;
        H->n_in = G.W; H->n_out = 0;
        const float inv = __fdiv_rn(1.0f, G.leaf);
        double leaves = 1.0;               // exact: a product of integers below 2^71 compared with 2^40
        for (int k = 0; k < 3; k++) {
            float a = sh.mn[0][k], b = sh.mx[0][k];
            for (int w = 1; w < GM_XF_WAVES; w++) { a = fminf(a, sh.mn[w][k]); b = fmaxf(b, sh.mx[w][k]); }
            if (G.W == 0) { a = 0.f; b = 0.f; }
            const float fa = floorf(__fmul_rn(a, inv)), fb = floorf(__fmul_rn(b, inv));
            const bool bad = !(fabsf(fa) < 1e9f && fabsf(fb) < 1e9f);
            H->minb[k] = bad ? 0 : (int)fa;
            H->divb[k] = bad ? 1 : (int)fb - (int)fa + 1;
            if (bad || leaves * (double)H->divb[k] >= (double)(1l << ICP_LEAF_BITS)) { G.flag[0] = 1; H->divb[k] = 1; } else leaves *= (double)H->divb[k];
        }
    }
}

__global__ __launch_bounds__(ICP_PT_NT) void gmap_leaf_keys(GmapDev G) {
    const int i = blockIdx.x * ICP_PT_NT + threadIdx.x;
    if (i >= G.W) return;
    const GmapHdr *H = G.hdr;
    const float4 q = G.tp[i];
    const float inv = __fdiv_rn(1.0f, G.leaf);
    long c[3];
    const float v[3] = {q.x, q.y, q.z};
    for (int k = 0; k < 3; k++) { long a = (long)floorf(__fmul_rn(v[k], inv)) - H->minb[k]; c[k] = a < 0 ? 0 : (a >= H->divb[k] ? H->divb[k] - 1 : a); }   // a clamp acts only after the overflow flag
    G.k1[i] = (unsigned long long)(c[0] + c[1] * (long)H->divb[0] + c[2] * (long)H->divb[0] * (long)H->divb[1]);
    G.v1[i] = i;
}

__global__ __launch_bounds__(GM_RUN_NT) void gmap_count(GmapDev G) {
    __shared__ GmapRunShared sh;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const long i = (long)blockIdx.x * GM_RUN_NT + t;
    const bool head = i < G.W && (i == 0 || G.k2[i] != G.k2[i - 1]);
    const unsigned long long bal = __ballot(head);
    if (lane == 0) sh.wave[wave] = __popcll(bal);
    lds_barrier();
    if (t == 0) { int total = 0; for (int w = 0; w < GM_RUN_WAVES; w++) total += sh.wave[w]; G.bcount[blockIdx.x] = total; }
}

__global__ __launch_bounds__(GM_RUN_NT) void gmap_scan(GmapDev G) {
    __shared__ GmapRunShared sh;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    int base = 0;
    for (int c0 = 0; c0 < G.nblk; c0 += GM_RUN_NT) {
        const int i = c0 + t, v = i < G.nblk ? G.bcount[i] : 0;
        int inc = v;
        for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(inc, o); if (lane >= o) inc += u; }
        if (lane == 63) sh.wave[wave] = inc;
        lds_barrier();
        int before = 0, total = 0;
        for (int w = 0; w < GM_RUN_WAVES; w++) { const int c = sh.wave[w]; before += w < wave ? c : 0; total += c; }
        if (i < G.nblk) G.bbase[i] = base + before + inc - v;
        base += total;
        lds_barrier();
    }
    if (t == 0) G.hdr->n_out = base;
}

__global__ __launch_bounds__(GM_RUN_NT) void gmap_centroids(GmapDev G) {
    __shared__ GmapRunShared sh;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const long i = (long)blockIdx.x * GM_RUN_NT + t;
    const unsigned long long key = i < G.W ? G.k2[i] : 0ull;
    const bool head = i < G.W && (i == 0 || key != G.k2[i - 1]);
    const unsigned long long bal = __ballot(head);
    if (lane == 0) sh.wave[wave] = __popcll(bal);
    lds_barrier();
    if (!head) return;
    int before = 0;
    for (int w = 0; w < wave; w++) before += sh.wave[w];
    const int rank = G.bbase[blockIdx.x] + before + __popcll(bal & ((1ull << lane) - 1ull));
    float sx = 0.f, sy = 0.f, sz = 0.f, si = 0.f;
    long e = i;
    for (; e < G.W && G.k2[e] == key; e++) { const float4 p = G.tp[G.v2[e]]; sx = __fadd_rn(sx, p.x); sy = __fadd_rn(sy, p.y); sz = __fadd_rn(sz, p.z); si = __fadd_rn(si, p.w); }
    const float cnt = (float)(e - i);
    G.map[rank] = make_float4(__fdiv_rn(sx, cnt), __fdiv_rn(sy, cnt), __fdiv_rn(sz, cnt), __fdiv_rn(si, cnt));
}

extern "C" int vilf_icp_global_map(vilf_handle *h, int first, int count, int skip, const double *poses6, long *n_out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    IcpCtx *c = vilf_stage<IcpCtx>(h, ST_ICP);
    if (!c || !poses6 || !n_out) { h->err = "vilf_icp_global_map: no store (vilf_icp_create) or null argument"; return VILF_ERR_INVALID_ARGUMENT; }
    if (first < 0 || count < 0 || skip < 1 || (long)first + count > c->size) { h->err = "vilf_icp_global_map: first >= 0, count >= 0, skip >= 1, first + count <= size"; return VILF_ERR_INVALID_ARGUMENT; }
    for (size_t i = 0; i < 6 * (size_t)c->size; i++) if (!std::isfinite(poses6[i])) { h->err = "vilf_icp_global_map: the pose of key frame " + std::to_string(i / 6) + " is not finite"; return VILF_ERR_INVALID_ARGUMENT; }
    c->gm_built = false; c->gm_n = 0; c->last_n = 0;
    std::vector<int> &hc = c->h_chunks;
    hc.clear();
    long W = 0;
    for (long k = first; k < (long)first + count; k += skip) {
        const int p0 = c->off[k], n = c->off[k + 1] - p0;
        if (W + n > INT_MAX / 2) { h->err = "vilf_icp_global_map: more than 2^30 points selected"; return VILF_ERR_UNSUPPORTED; }
        for (int j = 0; j < n; j += GM_CHUNK) { const int q[4] = {(int)k, p0 + j, std::min(GM_CHUNK, n - j), (int)(W + j)}; hc.insert(hc.end(), q, q + 4); }
        W += n;
    }
    const int nchunks = (int)(hc.size() / 4), nblk = (int)((W + GM_RUN_NT - 1) / GM_RUN_NT);
    c->h_mats.resize((size_t)c->size * 12);
    for (int k = 0; k < c->size; k++) icp_pose_matrix(poses6 + 6 * (size_t)k, c->h_mats.data() + 12 * (size_t)k);
    const size_t Wn = std::max<long>(W, 1), tb = vilf_sort_temp_bytes(Wn, 8);
    HIPCHECK(h, hipSetDevice(h->device));
    const bool ok = c->gm_chunks.ensure(std::max<size_t>(hc.size(), 4) * 4) && c->gm_part.ensure(std::max(nchunks, 1) * (size_t)24) && c->gm_hdr.ensure(sizeof(GmapHdr)) &&
                    c->gm_bcount.ensure(std::max(nblk, 1) * (size_t)4) && c->gm_bbase.ensure(std::max(nblk, 1) * (size_t)4) && c->gm_map.ensure(Wn * 16) && c->tp.ensure(Wn * 16) &&
                    c->k1.ensure(Wn * 8) && c->k2.ensure(Wn * 8) && c->v1.ensure(Wn * 4) && c->v2.ensure(Wn * 4) && c->temp.ensure(tb + 256);
    if (!ok) { h->err = "hipMalloc failed (global map work arrays)"; return VILF_ERR_DEVICE; }
    if (nchunks > 0) HIPCHECK(h, hipMemcpyAsync(c->gm_chunks.p, hc.data(), hc.size() * 4, hipMemcpyHostToDevice, h->stream));
    if (c->size > 0) HIPCHECK(h, hipMemcpyAsync(c->mats.p, c->h_mats.data(), c->h_mats.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(h, hipMemsetAsync(c->flag.p, 0, 4, h->stream));
    const GmapDev G{c->pts.as<float4>(), c->mats.as<float>(), c->gm_chunks.as<int4>(), c->gm_part.as<float>(), nchunks, c->tp.as<float4>(), c->gm_map.as<float4>(),
                    c->k1.as<unsigned long long>(), c->k2.as<unsigned long long>(), c->v1.as<int>(), c->v2.as<int>(), c->gm_hdr.as<GmapHdr>(), c->gm_bcount.as<int>(),
                    c->gm_bbase.as<int>(), c->flag.as<int>(), (int)W, nblk, (float)c->p.leaf_size};
    ProfMarks prof(h, c->gm_prof);
    if (nchunks > 0) hipLaunchKernelGGL(gmap_xf_bbox, dim3(nchunks), dim3(GM_XF_NT), 0, h->stream, G);
    hipLaunchKernelGGL(gmap_box, dim3(1), dim3(GM_XF_NT), 0, h->stream, G); prof.mark(0);
    if (W > 0) {
        hipLaunchKernelGGL(gmap_leaf_keys, dim3((unsigned)((W + ICP_PT_NT - 1) / ICP_PT_NT)), dim3(ICP_PT_NT), 0, h->stream, G); prof.mark(1);
        if (vilf_sort_pairs_u64(h->stream, c->temp.p, c->temp.cap, G.k1, G.k2, G.v1, G.v2, (size_t)W, ICP_LEAF_BITS) != 0) { h->err = "vilf_icp_global_map: radix sort failed"; return VILF_ERR_DEVICE; }
        prof.mark(2);
        hipLaunchKernelGGL(gmap_count, dim3(nblk), dim3(GM_RUN_NT), 0, h->stream, G);
        hipLaunchKernelGGL(gmap_scan, dim3(1), dim3(GM_RUN_NT), 0, h->stream, G);
        hipLaunchKernelGGL(gmap_centroids, dim3(nblk), dim3(GM_RUN_NT), 0, h->stream, G); prof.mark(3);
    }
    HIPCHECK(h, hipGetLastError());
    GmapHdr H;
    HIPCHECK(h, hipMemcpyAsync(&H, c->gm_hdr.p, sizeof(H), hipMemcpyDeviceToHost, h->stream));
    const int rc = icp_finish(h, c);       // the one wait of the build
    if (rc != VILF_OK) { if (rc == VILF_ERR_UNSUPPORTED) h->err = "vilf_icp_global_map: the map's bounding box holds 2^40 leaves or more"; return rc; }
    c->gm_built = true; c->gm_n = H.n_out;
    *n_out = c->gm_n;
    return VILF_OK;
}

extern "C" int vilf_icp_global_map_size(vilf_handle *h, long *n_out) {
    if (!h || !n_out) return VILF_ERR_INVALID_ARGUMENT;
    const IcpCtx *c = vilf_stage<IcpCtx>(h, ST_ICP);
    *n_out = c ? c->gm_n : 0;
    return VILF_OK;
}

extern "C" int vilf_icp_global_map_get(vilf_handle *h, long offset, long count, float *xyzi_out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    IcpCtx *c = vilf_stage<IcpCtx>(h, ST_ICP);
    if (!c || !c->gm_built) { h->err = "vilf_icp_global_map_get: no map (vilf_icp_global_map)"; return VILF_ERR_INVALID_ARGUMENT; }
    if (offset < 0 || count < 0 || offset > c->gm_n || count > c->gm_n - offset || (count > 0 && !xyzi_out)) {
        h->err = "vilf_icp_global_map_get: [" + std::to_string(offset) + ", " + std::to_string(offset) + " + " + std::to_string(count) + ") outside the map of " + std::to_string(c->gm_n) + " points, or null output";
        return VILF_ERR_INVALID_ARGUMENT;
    }
    if (count == 0) return VILF_OK;
    HIPCHECK(h, hipSetDevice(h->device));
    HIPCHECK(h, vilf_copy_sync(h, xyzi_out, c->gm_map.as<float4>() + offset, (size_t)count * 16, hipMemcpyDeviceToHost));
    return VILF_OK;
}

extern "C" int vilf_get_profile_icp_map(vilf_handle *h, double ms_out[4], long launches_out[4]) { return vilf_stage_profile(h, ST_ICP, &IcpCtx::gm_prof, ms_out, launches_out); }
