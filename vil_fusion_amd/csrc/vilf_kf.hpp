// vilf_kf.hpp — what the two stages of the visual loop closure share on the host: the key-frame store (vilf_kf.hip owns it, vilf_kfloop.hip reads it and hangs a
//   key frame's geometry on it) and the match as an enqueue, whose results stay on the device for the second stage. Candidate retrieval (vilf_bow.hip) hangs its
//   vocabulary and its database of BoW vectors on the same store: it reads the store's key-point descriptors.
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include "vilf_internal.hpp"

#define KF_STAGES 5                     // upload + blur, FAST, descriptors + lift, match, download
#define KFL_STAGES 5                    // gather, hypotheses, score, refine, download
#define BOW_STAGES 5                    // transform, sort + compact, score, select, download
#define KF_WORDS VILF_KF_WORDS
#define KF_WIN_CAP VILF_MAX_FEATURES    // window points of a key frame: slot k of the window arrays starts at k * KF_WIN_CAP
#define KF_NT 256                       // every 1-D kernel; kf_nms_count, kf_nms_place, kf_brief: four waves = four rows / points per workgroup
#define KF_WAVES (KF_NT / 64)

// a key frame's place in the store: its key points are rows kp_off .. kp_off + n_kp - 1 of the key-point arrays
struct KfMeta { int kp_off, n_kp, n_win, pad_; };
static_assert(sizeof(KfMeta) == 16, "kf_match reads a row as one int4");

struct KfMatchOut { unsigned char *status; float2 *pt, *ptn; int *idx, *dist, *nmatched; };
__global__ void kf_match(const KfMeta *meta, const unsigned long long *kp_desc, const float2 *kp_pt, const float2 *kp_norm, const unsigned long long *win_desc, int cur,
                         const int *old, int max_dist, int accept_dist, KfMatchOut out);                  // grid (ceil(n_window / 64), n_old), n_window > 0

struct KfCtx : VilfStage {
    vilf_kf_params p;
    int capK = 0, size = 0;
    long capP = 0, used = 0;
    size_t ncell = 0;                   // W * H
    std::vector<KfMeta> meta;           // host mirror of meta_d
    DBuf kp_pt, kp_norm, kp_desc, win_pt, win_desc, meta_d, pat;            // the store
    DBuf img, blur, score, rowcnt, rowoff, total, tpts, tscore, tdesc, old_d, res;      // one call's workspace
    PinBuf stage, pin, down;            // the image on its way to the device; counts, a meta row, window points and old indices on theirs; a search's results on their way back
    StageProf<KF_STAGES> prof;
    // the second stage (vilf_kfloop.hip): a key frame's geometry, allocated for the whole store by the first vilf_kf_set_geometry
    DBuf geo_X, geo_pose;               // point_3d [capK][KF_WIN_CAP][3] float32; origin_vio_R, origin_vio_T [capK][12] fp64
    std::vector<char> has_geo;          // [capK]
    std::vector<double> geo_pose_h;     // host mirror of geo_pose, for the decision
    DBuf loop_d;                        // one vilf_kf_find_connection's workspace
    PinBuf loop_down;
    StageProf<KFL_STAGES> loop_prof;
    // candidate retrieval (vilf_bow.hip): the vocabulary, breadth-first (node 0 = the root, a node's children side by side), and the database of BoW vectors
    bool voc_set = false;
    int voc_nodes = 0, voc_words = 0, voc_weighting = 0, voc_wbits = 0;      // nodes with the root; voc_wbits: the bits of a sort key's word field (voc_words is the "stopped" key)
    DBuf voc_kids, voc_desc, voc_word, voc_weight, voc_wweight;              // int2 (first child, children) [nodes]; uint64 [nodes][4]; int [nodes] (-1: inner); double [nodes]; double [words]
    int bow_size = 0;                   // entries of the database: key frames 0 .. bow_size - 1
    std::vector<int> bow_n;             // [capK] host mirror of bow_n_d
    DBuf bow_word, bow_val, bow_n_d;    // [capP] int, [capP] double: the vector of key frame e in rows kp_off .. kp_off + bow_n[e] - 1; [capK] int
    DBuf bow_k1, bow_k2, bow_v1, bow_v2, bow_temp, bow_tw, bow_twt, bow_tdesc, bow_score_d, bow_rows;     // one call's workspace
    PinBuf bow_down;
    StageProf<BOW_STAGES> bow_prof;
    void profile_reset() override { prof.reset(); loop_prof.reset(); bow_prof.reset(); }
};

KfCtx *vilf_kf_ctx(vilf_handle *h, const char *who);       // the store, or null with the handle's error set
int vilf_kf_finish(vilf_handle *h);                        // the wait that ends a call: a fault of the launches is reported by the call that made them
// what vilf_kf_match refuses (cur, n_old, old_index), under the caller's name
int vilf_kf_match_check(vilf_handle *h, KfCtx *c, const char *who, int cur, int n_old, const int *old_index);
// the match without its wait and download: the old indices go up (c->old_d keeps them for what follows on the stream), the counts are zeroed, kf_match is launched
int vilf_kf_match_enqueue(vilf_handle *h, KfCtx *c, int cur, int n_old, const int *old_index, const KfMatchOut &out);
