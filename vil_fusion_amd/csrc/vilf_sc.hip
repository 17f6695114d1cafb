// vilf_sc.hip — Scan Context loop detection of the global_fusion node on the device (≙ SCManager, global_fusion/include/Scancontext/Scancontext.h).
//   vilf_sc_add_keyframe(s) ≙ makeAndSaveScancontextAndKeys (:193-204), vilf_sc_detect ≙ detectLoopClosureID (:210-300), vilf_sc_detect_range = the same for a
//   range of key frames as one chain of launches. The semantics are stated once, in include/vilfusion.h.
// Everything about a key frame stays in a device database sized at creation (ScDb). One detection =
//   sc_ringkey_topk  a wave per query: the k snapshot entries nearest to its ring key (float squared L2), k selection passes, ties to the lower index
//   sc_distance      a workgroup per query (its normalised descriptor staged once in LDS), a wave per candidate: sector-key alignment, C = A^T B on the
//                    matrix cores (60 x 60, K = 20, padded to 64 x 64: 16 tiles x 5 v_mfma_f64_16x16x4_f64), the 60 wrapped-diagonal sums in column order,
//                    the effective-column counts from the two column masks, the minimum over the searched shifts; a wave keeps the best of its candidates
//   sc_reduce        a wave per query: the winner over the waves' slots, the threshold, the result record
// A candidate's place in the search order travels with its distance and every minimum is lexicographic (distance, place), so no result depends on the order in
// which waves or workgroups finish; there are no atomics on global memory.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>
#include "vilf_internal.hpp"
#include "vilf_device.hpp"
#include "vilf_kernels.hpp"

#define SC_RINGS 20
#define SC_SECTORS 60
#define SC_BINS (SC_RINGS * SC_SECTORS)
#define SC_PADC 64                     // columns of the normalised copy (the MFMA operand): 60 + 4 of zeros
#define SC_NRM (SC_RINGS * SC_PADC)    // doubles per key frame of that copy, [ring][column]
#define SC_KMAX 16                     // sc_ringkey_topk: candidates per query
#define SC_NO_POINT (-1000.0f)         // NO_POINT, Scancontext.h:49
#define SC_NO_DIST 10000000.0          // the reference's initial min_dist / min_sc_dist (:169, :243)
static_assert(SC_RINGS % 4 == 0 && SC_PADC % 16 == 0 && SC_PADC >= SC_SECTORS && SC_SECTORS <= 64, "16 x 16 x 4 tiles; a lane per shift and a bit per column");

// the database: arrays of `capacity` key frames
struct ScDb {
    double *desc;                      // [SC_RINGS][SC_SECTORS]
    double *nrm;                       // [SC_RINGS][SC_PADC]: every column divided by its norm (a zero column stays zero)
    float *rkey;                       // [SC_RINGS]
    double *skey;                      // [SC_SECTORS]
    double *norm;                      // [SC_SECTORS]
    unsigned long long *mask;          // bit c: column c has a non-zero norm
};
// which key frames are queried and what each may see. Query q is key frame first + q; fixed_snap >= 0 is the snapshot bound kept by vilf_sc_detect on the host,
// -1 derives it per query as the replay does (vilfusion.h)
struct ScQuery { int first, fixed_snap, exclude_recent, period, k /*0: every snapshot entry*/; };

// ---- launch contract -----------------------------------------------------------------------------------------------------
#define SC_DESC_NT 256                 // sc_descriptor: grid = clouds
struct ScDescShared { int bin[SC_BINS]; double desc[SC_BINS]; double norm[SC_PADC]; };
#define SC_DESC_LDS_BYTES (SC_BINS * 4 + SC_BINS * 8 + SC_PADC * 8)
static_assert(sizeof(ScDescShared) == SC_DESC_LDS_BYTES && SC_DESC_LDS_BYTES <= VILF_LDS_CU_BYTES / 8, "sc_descriptor: 14.6 KB, eight workgroups per CU");
#define SC_TOPK_NT 64                  // sc_ringkey_topk: grid = queries, one wave
#define SC_DIST_WAVES 4
#define SC_DIST_NT (64 * SC_DIST_WAVES)    // sc_distance: grid = (queries, SC_DIST_GY_MAX at most); wave w of workgroup y owns slot 4 y + w of its query
#define SC_DIST_GY_MAX 64
#define SC_CSTRIDE 65                  // row stride of a wave's 16 x 64 slab of C: lane s reads [row][(c - s) mod 60], consecutive addresses across the lanes
struct ScDistShared { double a[SC_NRM]; double akey[SC_PADC]; double bkey[SC_DIST_WAVES][SC_PADC]; double c[SC_DIST_WAVES][16 * SC_CSTRIDE]; };
#define SC_DIST_LDS_BYTES ((SC_NRM + SC_PADC + SC_DIST_WAVES * SC_PADC + SC_DIST_WAVES * 16 * SC_CSTRIDE) * 8)
static_assert(sizeof(ScDistShared) == SC_DIST_LDS_BYTES && SC_DIST_LDS_BYTES <= VILF_LDS_CU_BYTES / 3, "sc_distance: 46 KB, three workgroups per CU");
#define SC_RED_NT 64                   // sc_reduce: grid = queries, one wave
__global__ void sc_descriptor(const float4 *pts, const int *off, int first, ScDb db, double radius, double height);
__global__ void sc_ringkey_topk(ScDb db, ScQuery Q, int *cand);
__global__ void sc_distance(ScDb db, ScQuery Q, int shift_radius, const int *cand, double *slot_d, int2 *slot_js);
__global__ void sc_reduce(ScDb db, ScQuery Q, int nslots, double thres, const int *cand, const double *slot_d, const int2 *slot_js, vilf_sc_result *res);

struct ScCtx : VilfStage {
    vilf_sc_params p;
    int capacity = 0, size = 0;
    long calls = 0;                    // tree_making_period_conter (:327)
    int snap = 0;                      // size of polarcontext_invkeys_to_search_
    DBuf desc, nrm, rkey, skey, norm, mask, pts, off, cand, slot_d, slot_js, res;
    StageProf<4> prof;                 // vilf_set_profiling: sc_descriptor, sc_ringkey_topk, sc_distance, sc_reduce
    void profile_reset() override { prof.reset(); }
    ScDb db() { return ScDb{desc.as<double>(), nrm.as<double>(), rkey.as<float>(), skey.as<double>(), norm.as<double>(), mask.as<unsigned long long>()}; }
};

namespace {
#define SC_WSYNC __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier()

// order-preserving integer image of a float (no NaN comes here): a signed compare of the images is the compare of the floats
VD int sc_fkey(float f) { const int i = __float_as_int(f); return i >= 0 ? i : i ^ 0x7fffffff; }
VD float sc_fval(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }
// the number of snapshot entries query key frame k may see (0: detectLoopClosureID returns early, :221-225)
__host__ __device__ inline int sc_snapshot(const ScQuery &Q, int k) {
    if (k < Q.exclude_recent) return 0;
    return Q.fixed_snap >= 0 ? Q.fixed_snap : Q.period * ((k - Q.exclude_recent) / Q.period) + 1;
}
// xy2theta (common.h:79-92) in degrees: atan on a float argument, correctly rounded; the scaling in double; one rounding to float at the return
VD float sc_theta(float x, float y) {
    const double c = 180.0 / M_PI;
    if (x >= 0.f && y >= 0.f) return (float)__dmul_rn(c, (double)(float)atan((double)__fdiv_rn(y, x)));
    if (x < 0.f && y >= 0.f) return (float)__dsub_rn(180.0, __dmul_rn(c, (double)(float)atan((double)__fdiv_rn(y, -x))));
    if (x < 0.f && y < 0.f) return (float)__dadd_rn(180.0, __dmul_rn(c, (double)(float)atan((double)__fdiv_rn(y, x))));
    return (float)__dsub_rn(360.0, __dmul_rn(c, (double)(float)atan((double)__fdiv_rn(-y, x))));
}
}  // namespace

// ---- sc_descriptor: one workgroup per cloud -------------------------------------------------------------------------------------
__global__ __launch_bounds__(SC_DESC_NT) void sc_descriptor(const float4 *pts, const int *off, int first, ScDb db, double radius, double height) {
    __shared__ ScDescShared s;
    const int t = threadIdx.x, p0 = off[blockIdx.x], p1 = off[blockIdx.x + 1];
    const size_t kf = (size_t)first + blockIdx.x;
    const int none = sc_fkey(SC_NO_POINT);
    for (int i = t; i < SC_BINS; i += SC_DESC_NT) s.bin[i] = none;
    lds_barrier();
    for (int p = p0 + t; p < p1; p += SC_DESC_NT) {
        const float4 v = pts[p];
        if (!(isfinite(v.x) && isfinite(v.y) && isfinite(v.z)) || (v.x == 0.f && v.y == 0.f)) continue;
        const float z = (float)__dadd_rn((double)v.z, height);
        // sqrtf, not __fsqrt_rn: without OCML_BASIC_ROUNDED_OPERATIONS the header maps that one to the native v_sqrt_f32 (1 ulp), which put a point one float above a
        // ring boundary into the ring below (range 60.000004 came out as 60); the plain square root is the correctly rounded one
        const float range = __builtin_sqrtf(__fadd_rn(__fmul_rn(v.x, v.x), __fmul_rn(v.y, v.y)));
        if ((double)range > radius) continue;
        const float theta = sc_theta(v.x, v.y);
        const double fr = ceil(__dmul_rn(__ddiv_rn((double)range, radius), (double)SC_RINGS)), fs = ceil(__dmul_rn(__ddiv_rn((double)theta, 360.0), (double)SC_SECTORS));
        const int ring = fr < 1.0 ? 1 : (fr > (double)SC_RINGS ? SC_RINGS : (int)fr), sector = fs < 1.0 ? 1 : (fs > (double)SC_SECTORS ? SC_SECTORS : (int)fs);
        atomicMax(&s.bin[(ring - 1) * SC_SECTORS + sector - 1], sc_fkey(z));      // `desc < pt.z` (:73): a z + height <= NO_POINT never enters, the bin stays empty
    }
    lds_barrier();
    for (int i = t; i < SC_BINS; i += SC_DESC_NT) {
        const int k = s.bin[i];
        const double d = k == none ? 0.0 : (double)sc_fval(k);
        s.desc[i] = d;
        db.desc[kf * SC_BINS + i] = d;
    }
    lds_barrier();
    if (t < SC_PADC) {              // wave 0, a lane per column: sector key, norm, mask
        const int c = t < SC_SECTORS ? t : 0;
        double sum = 0.0, sq = 0.0;
        for (int r = 0; r < SC_RINGS; r++) { const double d = s.desc[r * SC_SECTORS + c]; sum = __dadd_rn(sum, d); sq = __dadd_rn(sq, __dmul_rn(d, d)); }
        const double nrm = t < SC_SECTORS ? __dsqrt_rn(sq) : 0.0;
        s.norm[t] = nrm;
        const unsigned long long m = __ballot(nrm != 0.0);
        if (t < SC_SECTORS) { db.skey[kf * SC_SECTORS + t] = __ddiv_rn(sum, (double)SC_RINGS); db.norm[kf * SC_SECTORS + t] = nrm; }
        if (t == 0) db.mask[kf] = m;
    } else if (t < SC_PADC + SC_RINGS) {      // wave 1, a lane per ring: ring key
        const int r = t - SC_PADC;
        double sum = 0.0;
        for (int c = 0; c < SC_SECTORS; c++) sum = __dadd_rn(sum, s.desc[r * SC_SECTORS + c]);
        db.rkey[kf * SC_RINGS + r] = (float)__ddiv_rn(sum, (double)SC_SECTORS);
    }
    lds_barrier();
    for (int i = t; i < SC_NRM; i += SC_DESC_NT) {
        const int r = i / SC_PADC, c = i % SC_PADC;
        const double n = s.norm[c], d = s.desc[r * SC_SECTORS + (c < SC_SECTORS ? c : 0)];
        db.nrm[kf * SC_NRM + i] = n != 0.0 ? __ddiv_rn(d, n) : 0.0;
    }
}

// ---- sc_ringkey_topk: a wave per query ------------------------------------------------------------------------------------
__global__ __launch_bounds__(SC_TOPK_NT) void sc_ringkey_topk(ScDb db, ScQuery Q, int *cand) {
    const int q = blockIdx.x, lane = threadIdx.x, kf = Q.first + q, S = sc_snapshot(Q, kf);
    const int k = min(Q.k, S);
    float qk[SC_RINGS];
    for (int i = 0; i < SC_RINGS; i++) qk[i] = db.rkey[(size_t)kf * SC_RINGS + i];
    float last_d = -1.f;
    int last_i = -1;
    for (int r = 0; r < k; r++) {
        // the smallest (distance, index) above the one chosen in the pass before
        float bd = 0.f;
        int bi = INT_MAX;
        for (int e = lane; e < S; e += SC_TOPK_NT) {
            const float *ek = db.rkey + (size_t)e * SC_RINGS;
            float d = 0.f;
            for (int i = 0; i < SC_RINGS; i++) { const float df = __fsub_rn(qk[i], ek[i]); d = __fadd_rn(d, __fmul_rn(df, df)); }
            const bool after = d > last_d || (d == last_d && e > last_i);
            if (after && (bi == INT_MAX || d < bd)) { bd = d; bi = e; }       // e ascends within a lane: the first of equal distances stays
        }
        for (int o = 32; o > 0; o >>= 1) {
            const float od = __shfl_xor(bd, o);
            const int oi = __shfl_xor(bi, o);
            if (oi != INT_MAX && (bi == INT_MAX || od < bd || (od == bd && oi < bi))) { bd = od; bi = oi; }
        }
        if (lane == 0) cand[q * SC_KMAX + r] = bi == INT_MAX ? 0 : bi;          // nothing left to choose (distances that are not numbers): entry 0, as the reference's zero-initialised index array
        last_d = bd; last_i = bi;
        if (bi == INT_MAX) last_d = INFINITY;
    }
}

// ---- sc_distance: a workgroup per query, a wave per candidate ---------------------------------------------------------------------
__global__ __launch_bounds__(SC_DIST_NT, 3) void sc_distance(ScDb db, ScQuery Q, int shift_radius, const int *cand, double *slot_d, int2 *slot_js) {
    __shared__ ScDistShared s;
    const int q = blockIdx.x, t = threadIdx.x, wave = t >> 6, lane = t & 63, kf = Q.first + q, S = sc_snapshot(Q, kf);
    const int ncand = Q.k ? min(Q.k, S) : S, nslots = gridDim.y * SC_DIST_WAVES, slot = blockIdx.y * SC_DIST_WAVES + wave;
    if (blockIdx.y * SC_DIST_WAVES >= ncand) return;          // the whole workgroup: sc_reduce reads the slots below ncand only
    for (int i = t; i < SC_NRM; i += SC_DIST_NT) s.a[i] = db.nrm[(size_t)kf * SC_NRM + i];
    if (t < SC_PADC) s.akey[t] = db.skey[(size_t)kf * SC_SECTORS + (t < SC_SECTORS ? t : 0)];
    const unsigned long long maskA = db.mask[kf], all = (1ull << SC_SECTORS) - 1;
    lds_barrier();
    const int lr = lane >> 4, lc = lane & 15;
    double best_d = 0.0;
    int best_j = INT_MAX, best_s = 0;
    for (int j = slot; j < ncand; j += nslots) {
        const int ci = Q.k ? cand[q * SC_KMAX + j] : j;
        const double *B = db.nrm + (size_t)ci * SC_NRM;
        double b[SC_RINGS / 4][SC_PADC / 16];                 // the candidate's operand fragments: B[k = 4 step + lane / 16][column 16 tj + lane % 16]
        for (int st = 0; st < SC_RINGS / 4; st++) for (int tj = 0; tj < SC_PADC / 16; tj++) b[st][tj] = B[(4 * st + lr) * SC_PADC + 16 * tj + lc];
        s.bkey[wave][lane] = db.skey[(size_t)ci * SC_SECTORS + (lane < SC_SECTORS ? lane : 0)];
        const unsigned long long maskB = db.mask[ci];
        SC_WSYNC;
        // fastAlignUsingVkey (:104-125): lane s holds |vkey1 - circshift(vkey2, s)|
        double vn = 0.0;
#pragma unroll 4
        for (int c = 0; c < SC_SECTORS; c++) {
            int x = c - lane; x += x < 0 ? SC_SECTORS : 0; x = x < 0 ? 0 : x;       // lanes 60..63 compute a value nobody reads
            const double df = __dsub_rn(s.akey[c], s.bkey[wave][x]);
            vn = __dadd_rn(vn, __dmul_rn(df, df));
        }
        vn = __dsqrt_rn(vn);
        int as = lane < SC_SECTORS && vn < SC_NO_DIST ? lane : INT_MAX;
        for (int o = 32; o > 0; o >>= 1) {
            const double od = __shfl_xor(vn, o);
            const int os = __shfl_xor(as, o);
            if (os != INT_MAX && (as == INT_MAX || od < vn || (od == vn && os < as))) { vn = od; as = os; }
        }
        const int align = as == INT_MAX ? 0 : as;
        // C = A^T B, 16 rows (query columns) at a time; lane s sums its wrapped diagonal in column order
        double sum = 0.0;
#pragma unroll 1
        for (int ti = 0; ti < SC_PADC / 16; ti++) {
            typedef double d4 __attribute__((ext_vector_type(4)));
            d4 acc[SC_PADC / 16];
            for (int tj = 0; tj < SC_PADC / 16; tj++) acc[tj] = d4{0.0, 0.0, 0.0, 0.0};
            for (int st = 0; st < SC_RINGS / 4; st++) {
                const double a = s.a[(4 * st + lr) * SC_PADC + 16 * ti + lc];
                for (int tj = 0; tj < SC_PADC / 16; tj++) acc[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[st][tj], acc[tj], 0, 0, 0);
            }
            for (int tj = 0; tj < SC_PADC / 16; tj++) for (int r = 0; r < 4; r++) s.c[wave][(lr + 4 * r) * SC_CSTRIDE + 16 * tj + lc] = acc[tj][r];
            SC_WSYNC;
            for (int cl = 0; cl < 16; cl++) {
                const int c = 16 * ti + cl;
                if (c >= SC_SECTORS) break;
                int x = c - lane; x += x < 0 ? SC_SECTORS : 0; x = x < 0 ? 0 : x;
                sum += s.c[wave][cl * SC_CSTRIDE + x];
            }
            SC_WSYNC;
        }
        // distDirectSC (:127-151): columns where either norm is zero add nothing above (their normalised column is zero) and are not counted
        const unsigned long long rot = lane < SC_SECTORS ? ((maskB << lane) | (maskB >> (SC_SECTORS - lane))) & all : 0ull;
        const double dist = 1.0 - sum / (double)__popcll(maskA & rot);
        int dd = lane - align; dd = dd < 0 ? -dd : dd; dd = min(dd, SC_SECTORS - dd);
        double pd = dist;
        int ps = lane < SC_SECTORS && dd <= shift_radius && dist < SC_NO_DIST ? lane : INT_MAX;      // NaN (no effective column) never wins
        for (int o = 32; o > 0; o >>= 1) {
            const double od = __shfl_xor(pd, o);
            const int os = __shfl_xor(ps, o);
            if (os != INT_MAX && (ps == INT_MAX || od < pd || (od == pd && os < ps))) { pd = od; ps = os; }
        }
        if (ps != INT_MAX && (best_j == INT_MAX || pd < best_d)) { best_d = pd; best_j = j; best_s = ps; }      // j ascends: the first of equal distances stays
    }
    if (lane == 0) { slot_d[(size_t)q * nslots + slot] = best_d; slot_js[(size_t)q * nslots + slot] = make_int2(best_j, best_s); }
}

// ---- sc_reduce: a wave per query ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SC_RED_NT) void sc_reduce(ScDb db, ScQuery Q, int nslots, double thres, const int *cand, const double *slot_d, const int2 *slot_js, vilf_sc_result *res) {
    const int q = blockIdx.x, lane = threadIdx.x, kf = Q.first + q, S = sc_snapshot(Q, kf);
    const int ncand = Q.k ? min(Q.k, S) : S;
    double bd = 0.0;
    int bj = INT_MAX, bs = 0;
    for (int i = lane; i < min(nslots, ncand); i += SC_RED_NT) {
        const double d = slot_d[(size_t)q * nslots + i];
        const int2 js = slot_js[(size_t)q * nslots + i];
        if (js.x != INT_MAX && (bj == INT_MAX || d < bd || (d == bd && js.x < bj))) { bd = d; bj = js.x; bs = js.y; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(bd, o);
        const int oj = __shfl_xor(bj, o), os = __shfl_xor(bs, o);
        if (oj != INT_MAX && (bj == INT_MAX || od < bd || (od == bd && oj < bj))) { bd = od; bj = oj; bs = os; }
    }
    vilf_sc_result *r = res + q;
    if (lane < SC_KMAX) r->candidates[lane] = lane < ncand ? (Q.k ? cand[q * SC_KMAX + lane] : lane) : -1;
    if (lane == 0) {
        const bool found = bj != INT_MAX;
        const int nearest = ncand == 0 ? -1 : (found ? (Q.k ? cand[q * SC_KMAX + bj] : bj) : 0);       // nn_idx starts at 0 (:245)
        const double md = found ? bd : SC_NO_DIST;
        r->loop_id = md < thres ? nearest : -1;
        r->nearest = nearest;
        r->shift = found ? bs : 0;
        r->n_candidates = ncand;
        r->min_dist = md;
        r->yaw_diff_rad = (float)__ddiv_rn(__dmul_rn(__dmul_rn((double)r->shift, 360.0 / (double)SC_SECTORS), M_PI), 180.0);     // deg2rad(nn_align * PC_UNIT_SECTORANGLE) :288
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
extern "C" void vilf_sc_default_params(vilf_sc_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->num_rings = SC_RINGS; p->num_sectors = SC_SECTORS; p->max_radius = 80.0; p->lidar_height = 2.0;
    p->num_exclude_recent = 30; p->num_candidates = 3; p->search_ratio = 0.1; p->dist_thres = 0.2; p->tree_making_period = 30;
}

extern "C" int vilf_sc_create(vilf_handle *h, const vilf_sc_params *p, int capacity) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    vilf_sc_params d;
    vilf_sc_default_params(&d);
    if (p) d = *p;
    if (capacity < 1) { h->err = "vilf_sc_create: capacity must be positive"; return VILF_ERR_INVALID_ARGUMENT; }
    if (d.num_rings != SC_RINGS || d.num_sectors != SC_SECTORS) { h->err = "vilf_sc_create: the kernels are built for 20 rings x 60 sectors"; return VILF_ERR_UNSUPPORTED; }
    if (!(d.max_radius > 0) || !std::isfinite(d.max_radius) || !std::isfinite(d.lidar_height) || d.num_exclude_recent < 1 || d.num_candidates < 0 || d.num_candidates > SC_KMAX ||
        !(d.search_ratio >= 0 && d.search_ratio <= 1) || std::isnan(d.dist_thres) || d.tree_making_period < 1) {
        h->err = "vilf_sc_create: max_radius > 0, num_exclude_recent >= 1, 0 <= num_candidates <= 16, 0 <= search_ratio <= 1, tree_making_period >= 1";
        return VILF_ERR_INVALID_ARGUMENT;
    }
    HIPCHECK(h, hipSetDevice(h->device));
    HIPCHECK(h, hipStreamSynchronize(h->stream));
    vilf_stage_drop(h, ST_SC);
    ScCtx *c = new ScCtx();
    c->p = d; c->capacity = capacity;
    const size_t n = (size_t)capacity;
    if (!c->desc.ensure(n * SC_BINS * 8) || !c->nrm.ensure(n * SC_NRM * 8) || !c->rkey.ensure(n * SC_RINGS * 4) || !c->skey.ensure(n * SC_SECTORS * 8) ||
        !c->norm.ensure(n * SC_SECTORS * 8) || !c->mask.ensure(n * 8)) {
        delete c;
        h->err = "hipMalloc failed (scan context database)";
        return VILF_ERR_DEVICE;
    }
    h->stage[ST_SC] = c;
    return VILF_OK;
}

extern "C" int vilf_sc_add_keyframes(vilf_handle *h, int n, const float *xyzi, const int *offsets, int *first_index_out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    ScCtx *c = vilf_stage<ScCtx>(h, ST_SC);
    if (!c) { h->err = "vilf_sc_add_keyframes: no database (vilf_sc_create)"; return VILF_ERR_INVALID_ARGUMENT; }
    if (n < 0 || !offsets || offsets[0] < 0) { h->err = "vilf_sc_add_keyframes: bad arguments"; return VILF_ERR_INVALID_ARGUMENT; }
    for (int i = 0; i < n; i++) if (offsets[i + 1] < offsets[i]) { h->err = "vilf_sc_add_keyframes: offsets must not decrease"; return VILF_ERR_INVALID_ARGUMENT; }
    const int total = offsets[n];
    if (total > 0 && !xyzi) { h->err = "vilf_sc_add_keyframes: null cloud"; return VILF_ERR_INVALID_ARGUMENT; }
    if (c->size + (long)n > c->capacity) {
        h->err = "vilf_sc_add_keyframes: " + std::to_string(c->size) + " + " + std::to_string(n) + " key frames exceed the capacity " + std::to_string(c->capacity);
        return VILF_ERR_UNSUPPORTED;
    }
    if (first_index_out) *first_index_out = c->size;
    if (n == 0) return VILF_OK;
    HIPCHECK(h, hipSetDevice(h->device));
    if (!c->pts.ensure(std::max<size_t>(total, 1) * 16) || !c->off.ensure((size_t)(n + 1) * 4)) { h->err = "hipMalloc failed (scan context clouds)"; return VILF_ERR_DEVICE; }
    if (total > 0) HIPCHECK(h, hipMemcpyAsync(c->pts.p, xyzi, (size_t)total * 16, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(h, hipMemcpyAsync(c->off.p, offsets, (size_t)(n + 1) * 4, hipMemcpyHostToDevice, h->stream));
    ProfMarks prof(h, c->prof);
    hipLaunchKernelGGL(sc_descriptor, dim3(n), dim3(SC_DESC_NT), 0, h->stream, c->pts.as<float4>(), c->off.as<int>(), c->size, c->db(), c->p.max_radius, c->p.lidar_height);
    HIPCHECK(h, hipGetLastError());
    prof.mark(0);
    HIPCHECK(h, hipStreamSynchronize(h->stream));       // the caller's clouds are free again; a fault of the launch is reported by this call
    if (h->profiling) { const int rcf = vilf_prof_flush(h); if (rcf != VILF_OK) return rcf; }
    c->size += n;
    return VILF_OK;
}

extern "C" int vilf_sc_add_keyframe(vilf_handle *h, const float *xyzi, int n_points, int *index_out) {
    if (n_points < 0) { if (h) h->err = "vilf_sc_add_keyframe: negative point count"; return VILF_ERR_INVALID_ARGUMENT; }
    const int off[2] = {0, n_points};
    return vilf_sc_add_keyframes(h, 1, xyzi, off, index_out);
}

// one chain of launches for the queries first .. first + n - 1
static int sc_search(vilf_handle *h, ScCtx *c, int first, int n, int fixed_snap, vilf_sc_result *out) {
    const ScQuery Q{first, fixed_snap, c->p.num_exclude_recent, c->p.tree_making_period, c->p.num_candidates};
    const int max_snap = sc_snapshot(Q, first + n - 1);
    const int max_cand = Q.k ? std::min(Q.k, max_snap) : max_snap;
    const int gy = std::max(1, std::min(SC_DIST_GY_MAX, (max_cand + SC_DIST_WAVES - 1) / SC_DIST_WAVES)), nslots = gy * SC_DIST_WAVES;
    const int shift_radius = (int)std::round(0.5 * c->p.search_ratio * SC_SECTORS);      // SEARCH_RADIUS :161
    HIPCHECK(h, hipSetDevice(h->device));
    const size_t sn = (size_t)n;
    if (!c->cand.ensure(sn * SC_KMAX * 4) || !c->slot_d.ensure(sn * nslots * 8) || !c->slot_js.ensure(sn * nslots * 8) || !c->res.ensure(sn * sizeof(vilf_sc_result))) {
        h->err = "hipMalloc failed (scan context search)";
        return VILF_ERR_DEVICE;
    }
    ProfMarks prof(h, c->prof);
    if (Q.k && max_cand > 0) hipLaunchKernelGGL(sc_ringkey_topk, dim3(n), dim3(SC_TOPK_NT), 0, h->stream, c->db(), Q, c->cand.as<int>());
    prof.mark(1);
    if (max_cand > 0) hipLaunchKernelGGL(sc_distance, dim3(n, gy), dim3(SC_DIST_NT), 0, h->stream, c->db(), Q, shift_radius, c->cand.as<int>(), c->slot_d.as<double>(), c->slot_js.as<int2>());
    prof.mark(2);
    hipLaunchKernelGGL(sc_reduce, dim3(n), dim3(SC_RED_NT), 0, h->stream, c->db(), Q, nslots, c->p.dist_thres, c->cand.as<int>(), c->slot_d.as<double>(), c->slot_js.as<int2>(), c->res.as<vilf_sc_result>());
    HIPCHECK(h, hipGetLastError());
    prof.mark(3);
    HIPCHECK(h, vilf_copy_sync(h, out, c->res.p, sn * sizeof(vilf_sc_result), hipMemcpyDeviceToHost));
    if (h->profiling) { const int rcf = vilf_prof_flush(h); if (rcf != VILF_OK) return rcf; }
    return VILF_OK;
}

extern "C" int vilf_sc_detect(vilf_handle *h, vilf_sc_result *out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    ScCtx *c = vilf_stage<ScCtx>(h, ST_SC);
    if (!c || !out) { h->err = "vilf_sc_detect: no database (vilf_sc_create) or null result"; return VILF_ERR_INVALID_ARGUMENT; }
    if (c->size == 0) { h->err = "vilf_sc_detect: the database is empty"; return VILF_ERR_INVALID_ARGUMENT; }
    if (c->size < c->p.num_exclude_recent + 1) {        // the early return (:221-225): the call is not counted
        out->loop_id = -1; out->nearest = -1; out->shift = 0; out->n_candidates = 0; out->min_dist = SC_NO_DIST; out->yaw_diff_rad = 0.f;
        for (int &v : out->candidates) v = -1;
        return VILF_OK;
    }
    if (c->calls % c->p.tree_making_period == 0) c->snap = c->size - c->p.num_exclude_recent;      // the tree is rebuilt (:228-240)
    c->calls++;
    return sc_search(h, c, c->size - 1, 1, c->snap, out);
}

extern "C" int vilf_sc_detect_range(vilf_handle *h, int first, int n, vilf_sc_result *out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    ScCtx *c = vilf_stage<ScCtx>(h, ST_SC);
    if (!c) { h->err = "vilf_sc_detect_range: no database (vilf_sc_create)"; return VILF_ERR_INVALID_ARGUMENT; }
    if (first < 0 || n < 0 || (long)first + n > c->size || (n > 0 && !out)) { h->err = "vilf_sc_detect_range: range outside the database or null result"; return VILF_ERR_INVALID_ARGUMENT; }
    if (n == 0) return VILF_OK;
    return sc_search(h, c, first, n, -1, out);
}

extern "C" int vilf_sc_get(vilf_handle *h, int index, double *desc, float *ring_key, double *sector_key) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    ScCtx *c = vilf_stage<ScCtx>(h, ST_SC);
    if (!c || index < 0 || index >= c->size) { h->err = "vilf_sc_get: no database or index out of range"; return VILF_ERR_INVALID_ARGUMENT; }
    HIPCHECK(h, hipSetDevice(h->device));
    const size_t i = (size_t)index;
    if (desc) HIPCHECK(h, hipMemcpyAsync(desc, c->desc.as<double>() + i * SC_BINS, SC_BINS * 8, hipMemcpyDeviceToHost, h->stream));
    if (ring_key) HIPCHECK(h, hipMemcpyAsync(ring_key, c->rkey.as<float>() + i * SC_RINGS, SC_RINGS * 4, hipMemcpyDeviceToHost, h->stream));
    if (sector_key) HIPCHECK(h, hipMemcpyAsync(sector_key, c->skey.as<double>() + i * SC_SECTORS, SC_SECTORS * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(h, hipStreamSynchronize(h->stream));
    return VILF_OK;
}

extern "C" int vilf_sc_size(vilf_handle *h, int *n_out) {
    if (!h || !n_out) return VILF_ERR_INVALID_ARGUMENT;
    const ScCtx *c = vilf_stage<ScCtx>(h, ST_SC);
    *n_out = c ? c->size : 0;
    return VILF_OK;
}

extern "C" int vilf_get_profile_sc(vilf_handle *h, double ms_out[4], long launches_out[4]) { return vilf_stage_profile(h, ST_SC, &ScCtx::prof, ms_out, launches_out); }
