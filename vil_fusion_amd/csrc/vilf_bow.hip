// vilf_bow.hip — candidate retrieval of the visual loop closure on the device (≙ PoseGraph::detectLoop and addKeyFrameIntoVoc, pose_graph/pose_graph.cpp:307-404, with
//   TemplatedVocabulary::transform, BowVector and TemplatedDatabase::queryL1 of ThirdParty/DBoW). The arithmetic is stated once, in include/vilfusion.h ("Visual loop
//   closure, candidate retrieval"). The vocabulary and the database hang off the key-frame store (KfCtx, vilf_kf.hpp), whose key-point descriptors are what is read.
// The vectors of n key frames = one chain of launches on the handle's stream over all their descriptors (their rows of the store are contiguous):
//   bow_transform    16 lanes per descriptor, 16 descriptors per workgroup: at every level lane g takes children g, g + 16, ... of the node (they lie side by side: the
//                    32-byte descriptor reads of a group are one contiguous run), popcount over the four words, the lexicographic (distance, position) minimum
//                    across the group by four xor shuffles. The sort key of a descriptor is (key frame - first) << wbits | word, a stopped word takes the key
//                    voc_words and so sorts behind its key frame's words
//   radix sort       vilf_sort_pairs_u64 over the keys: stable, and the sorted rows of a key frame are the rows it had before
//   bow_compact      a workgroup per key frame: run heads ranked by ballot counts, a lane per unique word adds its weight count - 1 times, lane 0 sums the norm in
//                    word order (a serial sum by definition), every lane divides
// The queries of n key frames = one chain of launches:
//   bow_score        grid (blocks of BOW_EPB entries, queries), four waves, a wave per (query, entry) pair: the query vector sits in LDS (VILF_BOW_LDS_WORDS; a longer
//                    one is read from global memory), the lanes read 64 of the entry's words coalesced and bisect the query for each; the hits' terms are added in
//                    lane order = ascending word order by a wave-uniform loop over the ballot. No atomics
//   bow_select       a wave per query: max_results rounds of the lexicographic (s, e) minimum above the last one taken; one row per query comes down
// The decision runs on the host after the download.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>
#include "vilf_internal.hpp"
#include "vilf_sort.hpp"
#include "vilf_kf.hpp"

// ---- launch contract -----------------------------------------------------------------------------------------------------
#define BOW_NT 256                      // every kernel
#define BOW_GROUP 16                    // bow_transform: lanes per descriptor
#define BOW_DPB (BOW_NT / BOW_GROUP)    // bow_transform: descriptors per workgroup
#define BOW_EPB 32                      // bow_score: entries per workgroup, eight per wave
#define BOW_SCORE_CAP ((size_t)1 << 23) // score cells (64 MB) of one batch of queries; a replay of more goes in several batches on the stream
#define BOW_MAX_DESC (1 << 24)          // vilf_kf_bow_transform
#define BOW_ABSENT INFINITY             // bow_score -> bow_select: the entry is not eligible or shares no word
static_assert(64 % BOW_GROUP == 0 && BOW_GROUP == 16, "bow_transform reduces a group with the xor shuffles 8, 4, 2, 1");
static_assert(VILF_BOW_LDS_WORDS * 12 <= 48 * 1024, "bow_score: the query vector in LDS");
static_assert(sizeof(vilf_bow_node) == 48 && sizeof(vilf_bow_word) == 8, "the records of the VINS binary file");

struct BowVocD { const int2 *kids; const ulonglong2 *desc; const int *word; const double *weight; };
struct BowRow { int n_results, n_words; int id[VILF_BOW_MAX_RESULTS]; double s[VILF_BOW_MAX_RESULTS]; };
// grid = ceil(n / BOW_DPB); key / val may be null (the stateless transform), word_out / weight_out may be null (the vectors)
__global__ void bow_transform(BowVocD V, const unsigned long long *desc, int n, const KfMeta *meta, int first, int nkf, int row0, int wbits, int stop_word,
                              unsigned long long *key, int *val, int *word_out, double *weight_out);
// grid = the key frames of the call; key: the sorted keys, row r of the store at r - row0; heads: workspace of as many rows
__global__ void bow_compact(const KfMeta *meta, int first, int row0, int wbits, int stop_word, int weighting, const unsigned long long *key, const double *wweight, int *heads,
                            int *bow_word, double *bow_val, int *bow_n);
// grid (ceil(max entries / BOW_EPB), queries); query q is key frame qfirst + q against entries 0 .. qfirst + q - 1; score [queries][stride]
__global__ void bow_score(const KfMeta *meta, const int *bow_n, const int *bow_word, const double *bow_val, int qfirst, int min_gap, int stride, double *score);
// grid = ceil(queries / 4)
__global__ void bow_select(const double *score, int stride, int qfirst, int nq, int max_results, const int *bow_n, BowRow *rows);

// ---- bow_transform ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BOW_NT) void bow_transform(BowVocD V, const unsigned long long *desc, int n, const KfMeta *meta, int first, int nkf, int row0, int wbits, int stop_word,
                                                        unsigned long long *key, int *val, int *word_out, double *weight_out) {
    const int t = threadIdx.x, g = t & (BOW_GROUP - 1), i = blockIdx.x * BOW_DPB + t / BOW_GROUP;
    const bool valid = i < n;
    ulonglong2 a = make_ulonglong2(0, 0), b = a;
    if (valid) { const ulonglong2 *f = (const ulonglong2 *)(desc + (size_t)i * KF_WORDS); a = f[0]; b = f[1]; }
    int node = 0;
    bool done = !valid;
    for (int level = 0; level <= VILF_BOW_MAX_DEPTH; level++) {      // the host has refused a deeper tree; the trip count is the wave's
        int2 kd = make_int2(0, 0);
        if (!done) kd = V.kids[node];
        if (kd.y == 0) done = true;                                  // a leaf
        if (__ballot(!done) == 0ull) break;
        int bd = INT_MAX, bj = INT_MAX;
        for (int j = g; j < kd.y; j += BOW_GROUP) {                  // j ascends in a lane: the first of equal distances stays
            const ulonglong2 c = V.desc[2 * (size_t)(kd.x + j)], e = V.desc[2 * (size_t)(kd.x + j) + 1];
            const int d = __popcll(a.x ^ c.x) + __popcll(a.y ^ c.y) + __popcll(b.x ^ e.x) + __popcll(b.y ^ e.y);
            if (d < bd) { bd = d; bj = j; }
        }
#pragma unroll
        for (int o = BOW_GROUP / 2; o > 0; o >>= 1) {                // every lane of the wave takes part; a group's lanes only meet their own
            const int od = __shfl_xor(bd, o), oj = __shfl_xor(bj, o);
            if (od < bd || (od == bd && oj < bj)) { bd = od; bj = oj; }
        }
        if (!done) node = kd.x + bj;                                 // kd.y >= 1: lane 0 of the group had a child, bj < kd.y
    }
    if (!valid || g != 0) return;
    const int w = V.word[node];
    const double wt = V.weight[node];
    if (word_out) { word_out[i] = w; weight_out[i] = wt; }
    if (key) {
        const int r = row0 + i;
        int lo = first, hi = first + nkf - 1;                        // the last key frame of the call whose rows start at or before r: empty key frames share
        while (lo < hi) {                                            // their offset with the next one and lose
            const int mid = (lo + hi + 1) >> 1;
            if (meta[mid].kp_off <= r) lo = mid; else hi = mid - 1;
        }
        key[i] = ((unsigned long long)(lo - first) << wbits) | (unsigned long long)(wt > 0.0 ? w : stop_word);      // not stopped: w > 0 (:1092, :1115)
        val[i] = i;
    }
}

// ---- bow_compact -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BOW_NT) void bow_compact(const KfMeta *meta, int first, int row0, int wbits, int stop_word, int weighting, const unsigned long long *key,
                                                      const double *wweight, int *heads, int *bow_word, double *bow_val, int *bow_n) {
    __shared__ int s_heads[BOW_NT / 64], s_live[BOW_NT / 64];
    __shared__ double s_norm;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, kf = first + blockIdx.x;
    const int off = meta[kf].kp_off, n = meta[kf].n_kp;
    const unsigned long long wmask = (1ull << wbits) - 1ull;
    const unsigned long long *k = key + (off - row0);
    int *hd = heads + (off - row0);
    int nu = 0, nlive = 0;
    for (int c0 = 0; c0 < n; c0 += BOW_NT) {                         // the trip count is the workgroup's
        const int i = c0 + t;
        bool head = false, live = false;
        if (i < n) {
            const int w = (int)(k[i] & wmask);
            live = w != stop_word;
            head = live && (i == 0 || (int)(k[i - 1] & wmask) != w);
        }
        const unsigned long long bh = __ballot(head), bl = __ballot(live);
        if (lane == 0) { s_heads[wave] = __popcll(bh); s_live[wave] = __popcll(bl); }
        __syncthreads();
        int before = 0, all = 0, live_all = 0;
        for (int w = 0; w < BOW_NT / 64; w++) { before += w < wave ? s_heads[w] : 0; all += s_heads[w]; live_all += s_live[w]; }
        if (head) hd[nu + before + __popcll(bh & ((1ull << lane) - 1ull))] = i;      // a rank is at most i: inside the key frame's rows
        nu += all; nlive += live_all;
        __syncthreads();
    }
    for (int u = t; u < nu; u += BOW_NT) {
        const int i0 = hd[u], i1 = u + 1 < nu ? hd[u + 1] : nlive;   // the stopped keys sort behind the live ones
        const int w = (int)(k[i0] & wmask);
        const double wt = wweight[w];
        double v = wt;
        if (weighting == VILF_BOW_TF_IDF || weighting == VILF_BOW_TF) for (int c = 1; c < i1 - i0; c++) v = v + wt;      // addWeight: ((w + w) + w) ...
        bow_word[off + u] = w;
        bow_val[off + u] = v;
    }
    __syncthreads();
    if (t == 0) {
        double s = 0.0;
        for (int u = 0; u < nu; u++) s = s + fabs(bow_val[off + u]);      // normalize: in word order, one rounding per addition
        s_norm = s;
        bow_n[kf] = nu;
    }
    __syncthreads();
    const double norm = s_norm;
    if (norm > 0.0) for (int u = t; u < nu; u += BOW_NT) bow_val[off + u] = __ddiv_rn(bow_val[off + u], norm);
}

// ---- bow_score -------------------------------------------------------------------------------------------------------------------
namespace {
// one (query, entry) pair by one wave: qw / qv the query's words and values (LDS or global), ew / ev the entry's
__device__ __forceinline__ double bow_pair(const int *qw, const double *qv, int nq, const int *ew, const double *ev, int ne, int lane) {
    double s = 0.0;
    bool have = false;
    for (int c0 = 0; c0 < ne; c0 += 64) {                            // the trip count is the wave's
        const int i = c0 + lane;
        bool hit = false;
        double term = 0.0;
        if (i < ne) {
            const int w = ew[i];
            int lo = 0, hi = nq;                                     // the first query word >= w
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (qw[mid] < w) lo = mid + 1; else hi = mid;
            }
            if (lo < nq && qw[lo] == w) {
                const double q = qv[lo], d = ev[i];
                term = (fabs(q - d) - fabs(q)) - fabs(d);            // :681
                hit = true;
            }
        }
        unsigned long long m = __ballot(hit);
        while (m) {                                                  // lane order = ascending word id
            const int l = __ffsll((long long)m) - 1;
            const double tl = __shfl(term, l);
            s = have ? s + tl : tl;
            have = true;
            m &= m - 1ull;
        }
    }
    return have ? s : (double)BOW_ABSENT;
}
}  // namespace

__global__ __launch_bounds__(BOW_NT) void bow_score(const KfMeta *meta, const int *bow_n, const int *bow_word, const double *bow_val, int qfirst, int min_gap, int stride,
                                                    double *score) {
    __shared__ int s_w[VILF_BOW_LDS_WORDS];
    __shared__ double s_v[VILF_BOW_LDS_WORDS];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, q = blockIdx.y, qk = qfirst + q;
    const int E = qk, e0 = blockIdx.x * BOW_EPB, e1 = min(e0 + BOW_EPB, E), max_id = qk - min_gap;
    if (e0 >= E) return;                                             // the whole workgroup
    const int nq = bow_n[qk], qoff = meta[qk].kp_off;
    const bool in_lds = nq <= VILF_BOW_LDS_WORDS;
    if (in_lds) for (int i = t; i < nq; i += BOW_NT) { s_w[i] = bow_word[qoff + i]; s_v[i] = bow_val[qoff + i]; }
    __syncthreads();
    for (int e = e0 + wave; e < e1; e += BOW_NT / 64) {
        double s = (double)BOW_ABSENT;
        if (e < max_id || max_id == -1 || e == E - 1) {              // :679
            const int ne = bow_n[e], eoff = meta[e].kp_off;
            s = in_lds ? bow_pair(s_w, s_v, nq, bow_word + eoff, bow_val + eoff, ne, lane) : bow_pair(bow_word + qoff, bow_val + qoff, nq, bow_word + eoff, bow_val + eoff, ne, lane);
        }
        if (lane == 0) score[(size_t)q * stride + e] = s;
    }
}

// ---- bow_select ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BOW_NT) void bow_select(const double *score, int stride, int qfirst, int nq, int max_results, const int *bow_n, BowRow *rows) {
    const int lane = threadIdx.x & 63, q = blockIdx.x * (BOW_NT / 64) + (threadIdx.x >> 6);
    if (q >= nq) return;                                             // the whole wave
    const int E = qfirst + q;
    const double *row = score + (size_t)q * stride;
    BowRow *out = rows + q;
    double last_s = -INFINITY;
    int last_e = -1, cnt = 0;
    for (int r = 0; r < max_results; r++) {
        double bs = (double)BOW_ABSENT;
        int be = INT_MAX;
        for (int e = lane; e < E; e += 64) {
            const double s = row[e];
            if (s < (double)BOW_ABSENT && (s > last_s || (s == last_s && e > last_e)) && (s < bs || (s == bs && e < be))) { bs = s; be = e; }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const double os = __shfl_xor(bs, o);
            const int oe = __shfl_xor(be, o);
            if (oe != INT_MAX && (be == INT_MAX || os < bs || (os == bs && oe < be))) { bs = os; be = oe; }
        }
        if (be == INT_MAX) break;                                    // the same in every lane
        if (lane == 0) { out->id[r] = be; out->s[r] = bs; }
        last_s = bs; last_e = be; cnt++;
    }
    if (lane >= cnt && lane < VILF_BOW_MAX_RESULTS) { out->id[lane] = -1; out->s[lane] = 0.0; }
    if (lane == 0) { out->n_results = cnt; out->n_words = bow_n[E]; }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
namespace {
int bow_bits(unsigned long long v) { int b = 1; while (b < 63 && (v >> b) != 0) b++; return b; }      // bits that hold 0 .. v

KfCtx *bow_ctx(vilf_handle *h, const char *who) {
    KfCtx *c = vilf_kf_ctx(h, who);
    if (c && !c->voc_set) { h->err = std::string(who) + ": no vocabulary (vilf_kf_bow_set_vocabulary)"; return nullptr; }
    return c;
}
bool bow_params_ok(const vilf_bow_params *p) {
    return p && p->max_results >= 1 && p->max_results <= VILF_BOW_MAX_RESULTS && p->min_gap >= 0 && !std::isnan(p->neighbour_score) && !std::isnan(p->loop_score);
}
BowVocD bow_voc(KfCtx *c) { return BowVocD{c->voc_kids.as<int2>(), c->voc_desc.as<ulonglong2>(), c->voc_word.as<int>(), c->voc_weight.as<double>()}; }

// the vectors of key frames first .. first + n - 1 into their rows of the store, and their sizes into pinned ints [n] (read after the wait)
int bow_vectors(vilf_handle *h, KfCtx *c, int first, int n, ProfMarks<BOW_STAGES> &prof) {
    const int row0 = c->meta[first].kp_off;
    const KfMeta &last = c->meta[first + n - 1];
    const size_t N = (size_t)(last.kp_off + last.n_kp - row0);
    if (!c->bow_down.ensure(std::max((size_t)n * 4, (size_t)64))) { h->err = "allocation failed (BoW vectors)"; return VILF_ERR_DEVICE; }
    if (N > 0) {
        const size_t tb = vilf_sort_temp_bytes(N, 8);
        if (!c->bow_k1.ensure(N * 8) || !c->bow_k2.ensure(N * 8) || !c->bow_v1.ensure(N * 4) || !c->bow_v2.ensure(N * 4) || !c->bow_tw.ensure(N * 4) || !c->bow_temp.ensure(tb)) {
            h->err = "hipMalloc failed (BoW vectors)"; return VILF_ERR_DEVICE;
        }
        const int stop = c->voc_words, kbits = c->voc_wbits + bow_bits((unsigned long long)(n - 1));
        hipLaunchKernelGGL(bow_transform, dim3((unsigned)((N + BOW_DPB - 1) / BOW_DPB)), dim3(BOW_NT), 0, h->stream, bow_voc(c), c->kp_desc.as<unsigned long long>() + (size_t)row0 * KF_WORDS,
                           (int)N, c->meta_d.as<KfMeta>(), first, n, row0, c->voc_wbits, stop, c->bow_k1.as<unsigned long long>(), c->bow_v1.as<int>(), (int *)nullptr, (double *)nullptr);
        HIPCHECK(h, hipGetLastError());
        prof.mark(0);
        if (vilf_sort_pairs_u64(h->stream, c->bow_temp.p, c->bow_temp.cap, c->bow_k1.as<unsigned long long>(), c->bow_k2.as<unsigned long long>(), c->bow_v1.as<int>(), c->bow_v2.as<int>(),
                                N, kbits) != 0) { h->err = "vilf_kf_bow: radix sort failed"; return VILF_ERR_DEVICE; }
    }
    // a key frame without key points reads no key and writes its size 0
    hipLaunchKernelGGL(bow_compact, dim3(n), dim3(BOW_NT), 0, h->stream, c->meta_d.as<KfMeta>(), first, row0, c->voc_wbits, c->voc_words, c->voc_weighting,
                       c->bow_k2.as<unsigned long long>(), c->voc_wweight.as<double>(), c->bow_tw.as<int>(), c->bow_word.as<int>(), c->bow_val.as<double>(), c->bow_n_d.as<int>());
    HIPCHECK(h, hipGetLastError());
    prof.mark(1);
    HIPCHECK(h, hipMemcpyAsync(c->bow_down.p, c->bow_n_d.as<int>() + first, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    return VILF_OK;
}
void bow_commit(KfCtx *c, int first, int n) {
    std::memcpy(c->bow_n.data() + first, c->bow_down.p, (size_t)n * 4);
    c->bow_size = first + n;
}

// the queries of key frames first .. first + n - 1, each against the entries before it -> c->bow_rows [n], enqueued
int bow_queries(vilf_handle *h, KfCtx *c, const vilf_bow_params *p, int first, int n, ProfMarks<BOW_STAGES> &prof) {
    const size_t widest = (size_t)std::max(first + n - 1, 1);
    const size_t cells = std::min((size_t)n * widest, std::max(BOW_SCORE_CAP, widest));
    if (!c->bow_score_d.ensure(cells * 8) || !c->bow_rows.ensure((size_t)n * sizeof(BowRow))) { h->err = "hipMalloc failed (BoW query)"; return VILF_ERR_DEVICE; }
    for (int q0 = 0; q0 < n;) {
        int nb = std::min(n - q0, 32768);                            // grid.y
        while (nb > 1 && (size_t)nb * (size_t)(first + q0 + nb - 1) > cells) nb = (nb + 1) / 2;
        const int maxE = first + q0 + nb - 1, stride = std::max(maxE, 1);
        if (maxE > 0) hipLaunchKernelGGL(bow_score, dim3((maxE + BOW_EPB - 1) / BOW_EPB, nb), dim3(BOW_NT), 0, h->stream, c->meta_d.as<KfMeta>(), c->bow_n_d.as<int>(), c->bow_word.as<int>(),
                                         c->bow_val.as<double>(), first + q0, p->min_gap, stride, c->bow_score_d.as<double>());
        prof.mark(2);
        hipLaunchKernelGGL(bow_select, dim3((nb + BOW_NT / 64 - 1) / (BOW_NT / 64)), dim3(BOW_NT), 0, h->stream, c->bow_score_d.as<double>(), stride, first + q0, nb, p->max_results,
                           c->bow_n_d.as<int>(), c->bow_rows.as<BowRow>() + q0);
        HIPCHECK(h, hipGetLastError());
        prof.mark(3);
        q0 += nb;
    }
    return VILF_OK;
}
// the decision of detectLoop (:351-387) for key frame `frame` from its downloaded row
void bow_decide(const vilf_bow_params *p, int frame, const BowRow &r, vilf_bow_result *o) {
    o->n_results = r.n_results; o->n_words = r.n_words;
    for (int i = 0; i < VILF_BOW_MAX_RESULTS; i++) { o->id[i] = i < r.n_results ? r.id[i] : -1; o->score[i] = i < r.n_results ? -r.s[i] / 2.0 : 0.0; }
    bool find_loop = false;
    if (o->n_results >= 1 && o->score[0] > p->neighbour_score)
        for (int i = 1; i < o->n_results; i++) if (o->score[i] > p->loop_score) find_loop = true;
    o->find_loop = find_loop ? 1 : 0;
    o->loop_index = -1;
    if (find_loop && frame > p->min_gap) {
        int min_index = -1;
        for (int i = 0; i < o->n_results; i++) if (min_index == -1 || (o->id[i] < min_index && o->score[i] > p->loop_score)) min_index = o->id[i];
        o->loop_index = min_index;
    }
}
int bow_rows_down(vilf_handle *h, KfCtx *c, int n, size_t at) {      // the rows behind `at` bytes of the pinned block
    if (!c->bow_down.ensure(at + (size_t)n * sizeof(BowRow))) { h->err = "allocation failed (BoW query)"; return VILF_ERR_DEVICE; }
    HIPCHECK(h, hipMemcpyAsync((char *)c->bow_down.p + at, c->bow_rows.p, (size_t)n * sizeof(BowRow), hipMemcpyDeviceToHost, h->stream));
    return VILF_OK;
}
}  // namespace

extern "C" void vilf_kf_bow_default_params(vilf_bow_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->max_results = 4; p->min_gap = 50; p->neighbour_score = 0.05; p->loop_score = 0.015;
}

extern "C" int vilf_kf_bow_set_vocabulary(vilf_handle *h, const vilf_bow_vocabulary *v) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    const char *who = "vilf_kf_bow_set_vocabulary";
    KfCtx *c = vilf_kf_ctx(h, who);
    if (!c) return VILF_ERR_INVALID_ARGUMENT;
    auto bad = [&](const std::string &what) { h->err = std::string(who) + ": " + what; return VILF_ERR_INVALID_ARGUMENT; };
    if (!v || !v->nodes || !v->words || v->nNodes < 1 || v->nWords < 1 || v->nWords > v->nNodes) return bad("null pointer, or nNodes / nWords < 1, or more words than nodes");
    if (v->weightingType < 0 || v->weightingType > 3 || v->scoringType < 0 || v->scoringType > 5) return bad("weightingType outside 0 .. 3 or scoringType outside 0 .. 5");
    if (v->scoringType != VILF_BOW_L1_NORM) { h->err = std::string(who) + ": only L1_NORM scoring is served"; return VILF_ERR_UNSUPPORTED; }
    const int nN = v->nNodes, nW = v->nWords, nn = nN + 1;
    std::vector<int> rec(nn, -1), cnt(nn, 0), start(nn + 1, 0);      // by the caller's id: its record, its children
    for (int i = 0; i < nN; i++) {
        const vilf_bow_node &r = v->nodes[i];
        if (r.nodeId < 1 || r.nodeId > nN || rec[r.nodeId] != -1) return bad("the node ids are not a permutation of 1 .. nNodes");
        rec[r.nodeId] = i;
        if (!std::isfinite(r.weight) || r.weight < 0.0) return bad("a weight is negative or not finite");
    }
    for (int i = 0; i < nN; i++) {
        const vilf_bow_node &r = v->nodes[i];
        if (r.parentId < 0 || r.parentId > nN || r.parentId == r.nodeId) return bad("a parent does not exist");
        cnt[r.parentId]++;
    }
    for (int id = 0; id < nn; id++) start[id + 1] = start[id] + cnt[id];
    std::vector<int> child(nN), fill(start.begin(), start.end() - 1);
    for (int i = 0; i < nN; i++) child[fill[v->nodes[i].parentId]++] = v->nodes[i].nodeId;      // in file order (loadBin :1538)
    std::vector<int> order, newid(nn, -1), depth(nn, 0);               // breadth-first: order[new] = the caller's id
    order.reserve(nn);
    order.push_back(0); newid[0] = 0;
    std::vector<int2> kids(nn);
    for (size_t at = 0; at < order.size(); at++) {
        const int id = order[at];
        kids[at] = make_int2(cnt[id] ? (int)order.size() : 0, cnt[id]);
        for (int k = start[id]; k < start[id + 1]; k++) {
            const int ch = child[k];
            if (newid[ch] != -1) return bad("a node is reached twice");      // cannot happen with one parent each; kept as the bound of the walk
            newid[ch] = (int)order.size(); depth[ch] = depth[id] + 1;
            if (depth[ch] > VILF_BOW_MAX_DEPTH) return bad("a node lies deeper than VILF_BOW_MAX_DEPTH");
            order.push_back(ch);
        }
    }
    if ((int)order.size() != nn) return bad("a node is not reachable from the root");
    std::vector<int> word_of(nn, -1);
    std::vector<char> used(nW, 0);
    for (int i = 0; i < nW; i++) {
        const vilf_bow_word &w = v->words[i];
        if (w.nodeId < 1 || w.nodeId > nN) return bad("a word names a node that does not exist");
        if (w.wordId < 0 || w.wordId >= nW || used[w.wordId]) return bad("a word id outside 0 .. nWords - 1 or used twice");
        if (cnt[w.nodeId] != 0) return bad("a word on an inner node");
        if (word_of[w.nodeId] != -1) return bad("a leaf named by two words");
        used[w.wordId] = 1; word_of[w.nodeId] = w.wordId;
    }
    for (int id = 1; id < nn; id++) if (cnt[id] == 0 && word_of[id] == -1) return bad("a leaf without a word");
    std::vector<unsigned long long> desc((size_t)nn * KF_WORDS, 0ull);
    std::vector<int> word(nn, -1);
    std::vector<double> weight(nn, 0.0), wweight(nW, 0.0);
    for (int j = 1; j < nn; j++) {
        const vilf_bow_node &r = v->nodes[rec[order[j]]];
        std::memcpy(&desc[(size_t)j * KF_WORDS], r.descriptor, 32);
        word[j] = word_of[order[j]]; weight[j] = r.weight;
        if (word[j] >= 0) wweight[word[j]] = r.weight;
    }
    HIPCHECK(h, hipSetDevice(h->device));
    { const int rcf = vilf_prof_flush(h); if (rcf != VILF_OK) return rcf; }
    HIPCHECK(h, hipStreamSynchronize(h->stream));
    DBuf d_kids, d_desc, d_word, d_weight, d_ww, d_bw, d_bv, d_bn;
    const size_t P = (size_t)c->capP, K = (size_t)c->capK;
    if (!d_kids.ensure((size_t)nn * 8) || !d_desc.ensure((size_t)nn * 32) || !d_word.ensure((size_t)nn * 4) || !d_weight.ensure((size_t)nn * 8) || !d_ww.ensure((size_t)nW * 8) ||
        !d_bw.ensure(P * 4) || !d_bv.ensure(P * 8) || !d_bn.ensure(K * 4)) { h->err = "hipMalloc failed (vocabulary)"; return VILF_ERR_DEVICE; }
    HIPCHECK(h, vilf_copy_sync(h, d_kids.p, kids.data(), (size_t)nn * 8, hipMemcpyHostToDevice));
    HIPCHECK(h, vilf_copy_sync(h, d_desc.p, desc.data(), (size_t)nn * 32, hipMemcpyHostToDevice));
    HIPCHECK(h, vilf_copy_sync(h, d_word.p, word.data(), (size_t)nn * 4, hipMemcpyHostToDevice));
    HIPCHECK(h, vilf_copy_sync(h, d_weight.p, weight.data(), (size_t)nn * 8, hipMemcpyHostToDevice));
    HIPCHECK(h, vilf_copy_sync(h, d_ww.p, wweight.data(), (size_t)nW * 8, hipMemcpyHostToDevice));
    HIPCHECK(h, hipMemsetAsync(d_bn.p, 0, K * 4, h->stream));
    HIPCHECK(h, hipStreamSynchronize(h->stream));
    c->voc_kids = std::move(d_kids); c->voc_desc = std::move(d_desc); c->voc_word = std::move(d_word); c->voc_weight = std::move(d_weight); c->voc_wweight = std::move(d_ww);
    c->bow_word = std::move(d_bw); c->bow_val = std::move(d_bv); c->bow_n_d = std::move(d_bn);
    c->voc_set = true; c->voc_nodes = nn; c->voc_words = nW; c->voc_weighting = v->weightingType; c->voc_wbits = bow_bits((unsigned long long)nW);
    c->bow_size = 0; c->bow_n.assign(K, 0);
    return VILF_OK;
}

extern "C" int vilf_kf_bow_add_range(vilf_handle *h, int first, int n) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    KfCtx *c = bow_ctx(h, "vilf_kf_bow_add_range");
    if (!c) return VILF_ERR_INVALID_ARGUMENT;
    if (first != c->bow_size || n < 0 || (long)first + n > c->size) {
        h->err = "vilf_kf_bow_add_range: first must be the database's size (" + std::to_string(c->bow_size) + "), n >= 0 and every key frame in the store"; return VILF_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) return VILF_OK;
    HIPCHECK(h, hipSetDevice(h->device));
    ProfMarks prof(h, c->bow_prof);
    { const int rc = bow_vectors(h, c, first, n, prof); if (rc != VILF_OK) return rc; }
    prof.mark(4);
    { const int rc = vilf_kf_finish(h); if (rc != VILF_OK) return rc; }
    bow_commit(c, first, n);
    return VILF_OK;
}

extern "C" int vilf_kf_bow_add(vilf_handle *h, int index) { return vilf_kf_bow_add_range(h, index, 1); }

extern "C" int vilf_kf_bow_detect(vilf_handle *h, const vilf_bow_params *p, int cur, vilf_bow_result *out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    KfCtx *c = bow_ctx(h, "vilf_kf_bow_detect");
    if (!c) return VILF_ERR_INVALID_ARGUMENT;
    if (!out || !bow_params_ok(p)) { h->err = "vilf_kf_bow_detect: null pointer, max_results outside 1 .. VILF_BOW_MAX_RESULTS, min_gap < 0 or a score that is NaN"; return VILF_ERR_INVALID_ARGUMENT; }
    if (cur != c->bow_size || cur >= c->size) {
        h->err = "vilf_kf_bow_detect: cur must be the database's size (" + std::to_string(c->bow_size) + ") and a key frame of the store"; return VILF_ERR_INVALID_ARGUMENT;
    }
    HIPCHECK(h, hipSetDevice(h->device));
    if (!c->bow_down.ensure(64 + sizeof(BowRow))) { h->err = "allocation failed (BoW query)"; return VILF_ERR_DEVICE; }      // sized before the first copy into it is enqueued
    ProfMarks prof(h, c->bow_prof);
    { const int rc = bow_vectors(h, c, cur, 1, prof); if (rc != VILF_OK) return rc; }      // into rows no entry owns yet: the database changes at the commit below
    { const int rc = bow_queries(h, c, p, cur, 1, prof); if (rc != VILF_OK) return rc; }
    { const int rc = bow_rows_down(h, c, 1, 64); if (rc != VILF_OK) return rc; }
    prof.mark(4);
    { const int rc = vilf_kf_finish(h); if (rc != VILF_OK) return rc; }
    bow_commit(c, cur, 1);
    bow_decide(p, cur, *(const BowRow *)((const char *)c->bow_down.p + 64), out);
    return VILF_OK;
}

extern "C" int vilf_kf_bow_detect_range(vilf_handle *h, const vilf_bow_params *p, int first, int n, vilf_bow_result *out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    KfCtx *c = bow_ctx(h, "vilf_kf_bow_detect_range");
    if (!c) return VILF_ERR_INVALID_ARGUMENT;
    if (!bow_params_ok(p) || first < 0 || n < 0 || (long)first + n > c->bow_size || (n > 0 && !out)) {
        h->err = "vilf_kf_bow_detect_range: null pointer, a parameter outside its range, or a range outside the database"; return VILF_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) return VILF_OK;
    HIPCHECK(h, hipSetDevice(h->device));
    ProfMarks prof(h, c->bow_prof);
    { const int rc = bow_queries(h, c, p, first, n, prof); if (rc != VILF_OK) return rc; }
    { const int rc = bow_rows_down(h, c, n, 0); if (rc != VILF_OK) return rc; }
    prof.mark(4);
    { const int rc = vilf_kf_finish(h); if (rc != VILF_OK) return rc; }
    const BowRow *rows = (const BowRow *)c->bow_down.p;
    for (int i = 0; i < n; i++) bow_decide(p, first + i, rows[i], out + i);
    return VILF_OK;
}

extern "C" int vilf_kf_bow_get(vilf_handle *h, int index, int cap, int *word_out, double *value_out, int *n_out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    KfCtx *c = bow_ctx(h, "vilf_kf_bow_get");
    if (!c) return VILF_ERR_INVALID_ARGUMENT;
    if (index < 0 || index >= c->bow_size) { h->err = "vilf_kf_bow_get: index outside the database"; return VILF_ERR_INVALID_ARGUMENT; }
    const int nb = c->bow_n[index];
    if ((word_out || value_out) && cap < nb) { h->err = "vilf_kf_bow_get: the vector has " + std::to_string(nb) + " words"; return VILF_ERR_INVALID_ARGUMENT; }
    HIPCHECK(h, hipSetDevice(h->device));
    const size_t off = (size_t)c->meta[index].kp_off;
    ProfMarks prof(h, c->bow_prof);
    if (nb && word_out) HIPCHECK(h, hipMemcpyAsync(word_out, c->bow_word.as<int>() + off, (size_t)nb * 4, hipMemcpyDeviceToHost, h->stream));
    if (nb && value_out) HIPCHECK(h, hipMemcpyAsync(value_out, c->bow_val.as<double>() + off, (size_t)nb * 8, hipMemcpyDeviceToHost, h->stream));
    prof.mark(4);
    { const int rc = vilf_kf_finish(h); if (rc != VILF_OK) return rc; }
    if (n_out) *n_out = nb;
    return VILF_OK;
}

extern "C" int vilf_kf_bow_transform(vilf_handle *h, const unsigned long long *desc, int n, int *word_out, double *weight_out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    KfCtx *c = bow_ctx(h, "vilf_kf_bow_transform");
    if (!c) return VILF_ERR_INVALID_ARGUMENT;
    if (n < 0 || n > BOW_MAX_DESC || (n > 0 && (!desc || !word_out || !weight_out))) { h->err = "vilf_kf_bow_transform: null pointer or n outside 0 .. 2^24"; return VILF_ERR_INVALID_ARGUMENT; }
    if (n == 0) return VILF_OK;
    HIPCHECK(h, hipSetDevice(h->device));
    const size_t N = (size_t)n;
    if (!c->bow_tdesc.ensure(N * 32) || !c->bow_tw.ensure(N * 4) || !c->bow_twt.ensure(N * 8)) { h->err = "hipMalloc failed (BoW transform)"; return VILF_ERR_DEVICE; }
    ProfMarks prof(h, c->bow_prof);
    HIPCHECK(h, hipMemcpyAsync(c->bow_tdesc.p, desc, N * 32, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(bow_transform, dim3((unsigned)((N + BOW_DPB - 1) / BOW_DPB)), dim3(BOW_NT), 0, h->stream, bow_voc(c), c->bow_tdesc.as<unsigned long long>(), n, (const KfMeta *)nullptr, 0, 0, 0,
                       c->voc_wbits, c->voc_words, (unsigned long long *)nullptr, (int *)nullptr, c->bow_tw.as<int>(), c->bow_twt.as<double>());
    HIPCHECK(h, hipGetLastError());
    prof.mark(0);
    HIPCHECK(h, hipMemcpyAsync(word_out, c->bow_tw.p, N * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(h, hipMemcpyAsync(weight_out, c->bow_twt.p, N * 8, hipMemcpyDeviceToHost, h->stream));
    prof.mark(4);
    return vilf_kf_finish(h);
}

extern "C" int vilf_kf_bow_size(vilf_handle *h, int *n_out) {
    if (!h || !n_out) return VILF_ERR_INVALID_ARGUMENT;
    const KfCtx *c = vilf_stage<KfCtx>(h, ST_KF);
    *n_out = c ? c->bow_size : 0;
    return VILF_OK;
}

extern "C" int vilf_kf_bow_profile(vilf_handle *h, double ms_out[5], long launches_out[5]) { return vilf_stage_profile(h, ST_KF, &KfCtx::bow_prof, ms_out, launches_out); }
