// vilf_internal.hpp — library-internal definitions shared by the host translation units (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include <cstring>
#include "../../include/vilfusion.h"
#include "vilf_batch.hpp"

// ---- what every stage file's host half is built from -------------------------------------------------------------------------------------------------
//   DBuf / PinBuf   a device / pinned host buffer that grows on demand and frees itself: move-only, release() for the places that free in mid-life
//   VilfStage       the base of every stage's context; the handle keeps them in stage[] (vilf_stage<C>, vilf_stage_make<C>, vilf_stage_drop), vilf_destroy deletes
//                   and vilf_set_profiling resets them in one loop. A context's members free themselves; a destructor is written only for raw resources
//   StageProf<N>    the accumulated times and launch counts of a stage's N slots; ProfMarks books the spans between marks into it, vilf_stage_profile /
//                   vilf_handle_profile are the body of every vilf_*_profile getter
//   Layout          the offsets of the arrays packed into one block; StageIO is the in / out / up / down quadruple of a batched stage with its two copies
template <hipError_t (*Free)(void *)> struct VilfBuf {
    void *p = nullptr;
    size_t cap = 0;
    VilfBuf() = default;
    VilfBuf(const VilfBuf &) = delete;
    VilfBuf &operator=(const VilfBuf &) = delete;
    VilfBuf(VilfBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    VilfBuf &operator=(VilfBuf &&o) noexcept {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~VilfBuf() { release(); }
    void release() { if (p) Free(p); p = nullptr; cap = 0; }
};
struct DBuf : VilfBuf<hipFree> {
    bool ensure(size_t bytes) {
        if (bytes <= cap) return true;
        release();
        size_t want = bytes + bytes / 8 + 256;
        if (hipMalloc(&p, want) != hipSuccess) return false;
        cap = want;
        return true;
    }
    template <typename T> T *as() { return reinterpret_cast<T *>(p); }
};

enum {
    D_NFEAT, D_NFAC, D_POSE, D_SB, D_FEAT, D_CPOSE, D_CSB, D_CFEAT, D_POSE0, D_SB0, D_FEAT0, D_EX, D_GR0, D_GP0,
    D_FSTART, D_FNOBS, D_FOBS0, D_FFAC0, D_FCONST, D_PSOBS, D_PSSLOT, D_PAIROFF, D_IMU, D_LIDAR,
    D_PHDR, D_PX0, D_PJ, D_PR, D_PH, D_PG, D_FACW, D_HPP, D_W, D_HF, D_GF, D_IMUH, D_IMUG, D_LIDH, D_LIDG, D_G, D_DIAGH,
    D_SCALE, D_DIAG, D_GRAD, D_GN, D_ST, D_OPS, D_ORS, D_OVS, D_OBAS, D_OBGS, D_COV, D_WORK, D_HOOK, D_DBG, D_LUTI, D_LUTL, D_LUTV,
    D_MFLAG, D_MINFO, D_MF0, D_MSTP, D_MSTS, D_MSTF, D_MSTE, D_MBUF, D_MHD, D_MGD, D_MWF, D_MHF, D_MGF, D_MAMM, D_MX, D_MROT, D_MLAM, D_MAR, D_MBR, D_QLV, D_QLD, D_QLLOG, D_QLIT, D_QLINFO,
    D_PAIRD, D_FACREC, D_CF, D_STAMPS, D_LIVE, D_SBTAB, D_SPLITC, D_SPLITB, D_UPSTAGE, D_DNSTAGE, D_OBSV, D_OBSTD, D_OBSROW, D_TD, D_PHDR0, D_PX00, D_PJ0, D_PR0, D_PH0, D_PG0,      // priors as uploaded (restored by vilf_batch_rewind after a marginalization)
    D_FWROW, D_ROWFEAT, D_NROWS,                      // the row map of W (w_row_map, vilf_api.hip)
    D_COUNT
};

// pinned host staging kept across calls (vilf_batch_upload / download): no allocation, no zero fill, truly asynchronous copies
struct PinBuf : VilfBuf<hipHostFree> {
    bool ensure(size_t bytes) {
        if (bytes <= cap) return true;
        release();
        const size_t want = bytes + bytes / 8 + 4096;
        if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) return false;
        std::memset(p, 0, want);
        cap = want;
        return true;
    }
};

struct VilfStage {
    virtual ~VilfStage() = default;
    virtual void profile_reset() {}
};
// the handle's stages, in the order vilf_destroy frees them
enum {
    ST_S2M, ST_S2B,      // scan-to-map state: single stream / batched streams (S2B, vilf_s2m.hip)
    ST_FEAT,             // LiDAR feature extraction workspace (FeatCtx, vilf_feat.hip)
    ST_PG,               // pose-graph workspace (PgCtx, vilf_pg.hip)
    ST_LW,               // large-window solve workspace (LwCtx, vilf_lw.hip)
    ST_SC,               // Scan Context descriptor database and search workspace (ScCtx, vilf_sc.hip)
    ST_ICP,              // key-frame cloud store and ICP workspace of the loop verification (IcpCtx, vilf_icp.hip)
    ST_TRACK,            // image feature tracker: pyramids, feature list, detection workspace (TrackCtx, vilf_track.hip)
    ST_STARTUP,          // visual start-up: the pairs' correspondences, hypotheses and result rows (StartupCtx, vilf_startup.hip)
    ST_SFM,              // visual start-up, second stage: the windows, the frame rows and the structure (SfmCtx, vilf_sfm.hip)
    ST_BA,               // visual start-up, third stage: the start values, the BA's frames and structure (BaCtx, vilf_ba.hip)
    ST_TRI,              // feature triangulation: the packed candidates, the cameras and the depths (TriCtx, vilf_tri.hip)
    ST_EXROT,            // camera-IMU rotation calibration: the slots' frame counts, ric and histories (ExrotCtx, vilf_exrot.hip)
    ST_KF,               // visual loop closure: the key-frame store and its workspace (KfCtx, vilf_kf.hip)
    ST_PG4,              // visual loop closure, third stage: the 4-DoF pose graph's workspace (Pg4Ctx, vilf_pg4.hip)
    VILF_STAGE_COUNT
};

template <int N> struct StageProf {
    double ms[N] = {};
    long launches[N] = {};
    void reset() { for (int i = 0; i < N; i++) { ms[i] = 0; launches[i] = 0; } }
    void read(double *ms_out, long *launches_out) const { for (int i = 0; i < N; i++) { ms_out[i] = ms[i]; launches_out[i] = launches[i]; } }
};

struct Layout {
    size_t at = 0;
    size_t take(size_t bytes, size_t align = 256) {      // the next array's offset: at, aligned up
        const size_t o = (at + align - 1) & ~(align - 1);
        at = o + bytes;
        return o;
    }
};

// deep copy of a window snapshot (estimate_extrinsic / estimate_td: the batched entry points run the general single-window solve per slot and need the inputs again)
struct OwnedWindow {
    vilf_window_in in;
    std::vector<double> pose, sb, feat, obs, vel, ctd, row, gR0, gP0;
    std::vector<uint8_t> fconst;
    std::vector<int32_t> fstart, foff;
    std::vector<vilf_imu_preint> imu;
    std::vector<vilf_lidar_constraint> lidar;
};

// class plan of one window's visual factors (class_plan, vilf_api.hip): computed by the upload's validation pass, used by its packer
struct WindowPlan { int cls[VB_NPAIR], cstart[VB_NPAIR], ccount[VB_NPAIR], nslot; };
struct vilf_handle {
    vilf_options opts;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    DBuf d[D_COUNT];
    VbBatch batch;
    int B = 0;
    bool resident = false;
    bool async_upload = false, upload_inflight = false;   // vilf_set_async_upload: vilf_batch_upload does not wait for its copies; the next upload of the handle does, before it touches the staging
    bool defer_upload_sync = false;   // vilf_window_solve: upload, solve and download are one call — the host waits once, at the download
    std::vector<vilf_prior> priors;          // per slot (host mirror)
    std::vector<char> prior_dirty;
    std::vector<char> prior_dense;           // slot's live prior (imported from the host) holds a speed-bias block other than SpeedBias[0]
    int prior_dense_count = 0;
    std::vector<char> prior_dev_newer;       // slot's prior was produced on the device (marginalize) and not yet mirrored
    int prior_slots_valid = 0;               // the device prior arrays hold slots 0 .. prior_slots_valid-1 (survive a re-upload of the windows)
    bool prior_backup_valid = false;         // D_P*0 hold the priors as last uploaded
    bool prior_restore_needed = false;       // a marginalization has overwritten the device priors since that backup
    int mg_Mcap = 0;
    VbMarg marg;
    std::vector<int> h_nfeat, h_nframes;
    std::vector<double> h_ex, h_td;
    std::vector<OwnedWindow> own;            // only with estimate_extrinsic / estimate_td
    PinBuf pin_up, pin_down;                 // host staging of the batched upload / download
    bool luts_ready = false;                 // static scatter / gather tables uploaded
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int profiling = 0;                       // per-kernel HIP-event timing of the solve launches
    // deferred profile spans: an asynchronous call (sync == 0) records its events and leaves them here; they are read at the next point that waits for the
    // stream anyway (a synchronous call, vilf_batch_summaries, vilf_get_profile*) — per-kernel times without a host round trip between the stages of a frame
    struct ProfSpan { hipEvent_t a, b; double *ms; long *cnt; };
    std::vector<ProfSpan> prof_pending;
    std::vector<hipEvent_t> prof_used, prof_free;
    hipEvent_t wait_ev = nullptr;            // vilf_wait_for
    void *stamp_pinned = nullptr; size_t stamp_cap = 0; hipEvent_t stamp_ev = nullptr;   // vilf_batch_newest_poses_device: pinned staging of the caller's stamps
    StageProf<4> kernel_prof;                // linearize, solve, step, other (accumulated since last reset)
    std::vector<hipEvent_t> s2m_ev;         // scan-to-map profiling (same switch): group of launches -> ms
    std::vector<int> s2m_groups;
    StageProf<4> marg_prof;                  // k_marg_prepare, k_marg_schur, k_marg_finish, k_prior_prep
    StageProf<8> s2m_prof;
    std::vector<WindowPlan> plans;
    double last_solve_usec = 0;
    bool solve_time_pending = false;         // the last solve was enqueued with sync == 0: ev0 / ev1 are read by the next call that waits for the stream
    int split_gen = 0;      // generation counter of the k_linearize_split launches of this handle
    bool solve_dense_fallback = false;       // a prior imported from the host holds a speed-bias block other than SpeedBias[0]: k_solve (dense) instead of k_solve_sb
    VilfStage *stage[VILF_STAGE_COUNT] = {};   // the stages' contexts (ST_*), created by the first call that needs one
};

// a copy ordered on the handle's stream and waited for: the library's streams are non-blocking (they do not synchronise with the legacy default stream), so a plain
// hipMemcpy would neither wait for the kernels before it nor hold back the ones after it
static inline hipError_t vilf_copy_sync(vilf_handle *h, void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
    hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, h->stream);
    return e != hipSuccess ? e : hipStreamSynchronize(h->stream);
}
#define HIPCHECK(h, call)                                                                                        \
    do {                                                                                                         \
        hipError_t e_ = (call);                                                                                  \
        if (e_ != hipSuccess) {                                                                                  \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                                        \
            return VILF_ERR_DEVICE;                                                                              \
        }                                                                                                        \
    } while (0)


hipEvent_t vilf_prof_event(vilf_handle *h);                                 // an event recorded on the handle's stream now (from the pool)
void vilf_prof_span(vilf_handle *h, hipEvent_t a, hipEvent_t b, double *ms, long *cnt);   // elapsed(a, b) is added to *ms at the next flush
int vilf_prof_flush(vilf_handle *h);                                        // waits for the stream, reads every pending span

// a stage's context, typed (null until a call has made it); the same, made by the first call that needs it; a stage freed in mid-life
template <class C> C *vilf_stage(const vilf_handle *h, int s) { return static_cast<C *>(h->stage[s]); }
template <class C> C *vilf_stage_make(vilf_handle *h, int s) {
    if (!h->stage[s]) h->stage[s] = new C();
    return vilf_stage<C>(h, s);
}
static inline void vilf_stage_drop(vilf_handle *h, int s) { delete h->stage[s]; h->stage[s] = nullptr; }

// the body of every vilf_*_profile getter: the pending spans are read, then the record is copied out (zeros while the stage does not exist)
template <int N> int vilf_profile_read(vilf_handle *h, const StageProf<N> *p, double *ms_out, long *launches_out) {
    { const int rcf = vilf_prof_flush(h); if (rcf != VILF_OK) return rcf; }
    (p ? *p : StageProf<N>()).read(ms_out, launches_out);
    return VILF_OK;
}
template <class C, int N> int vilf_stage_profile(vilf_handle *h, int s, StageProf<N> C::*prof, double *ms_out, long *launches_out) {
    if (!h || !ms_out || !launches_out) return VILF_ERR_INVALID_ARGUMENT;
    const C *c = vilf_stage<C>(h, s);
    return vilf_profile_read(h, c ? &(c->*prof) : nullptr, ms_out, launches_out);
}
template <int N> int vilf_handle_profile(vilf_handle *h, StageProf<N> vilf_handle::*prof, double *ms_out, long *launches_out) {
    if (!h || !ms_out || !launches_out) return VILF_ERR_INVALID_ARGUMENT;
    return vilf_profile_read(h, &(h->*prof), ms_out, launches_out);
}
// the marks of a call: every mark closes the span since the one before it (the first: since the construction) into its slot. Nothing happens while profiling is off
template <int N> struct ProfMarks {
    vilf_handle *h; StageProf<N> *p; hipEvent_t e;
    ProfMarks(vilf_handle *h_, StageProf<N> &p_) : h(h_), p(&p_), e(h_->profiling ? vilf_prof_event(h_) : nullptr) {}
    void mark(int slot) {
        if (!h->profiling) return;
        hipEvent_t b = vilf_prof_event(h);
        vilf_prof_span(h, e, b, &p->ms[slot], &p->launches[slot]);
        e = b;
    }
};
// a batched stage's staging: the upload block on the device and its pinned image, the download block and its pinned image
struct StageIO {
    DBuf in, out;
    PinBuf up, down;
    bool ensure(size_t in_bytes, size_t out_bytes) { return in.ensure(in_bytes) && out.ensure(out_bytes) && up.ensure(in_bytes) && down.ensure(out_bytes); }
    hipError_t upload(vilf_handle *h, size_t bytes) { return hipMemcpyAsync(in.p, up.p, bytes, hipMemcpyHostToDevice, h->stream); }
    hipError_t download(vilf_handle *h, size_t bytes) { return vilf_copy_sync(h, down.p, out.p, bytes, hipMemcpyDeviceToHost); }
};
#define VILF_SU_WIN_INTS (4 + VILF_MAX_FEATURES + VILF_MAX_FEATURES + 2)      // a start-up window's integers on the device: n_frames, n_features, first row of its points, 0; start_frame; first_obs (+ 1 pad)
int vilf_startup_check_windows(vilf_handle *h, const char *who, int n_windows, const vilf_startup_window *windows, size_t *total_out);   // what both stages refuse in the windows
void vilf_startup_pack_windows(int n_windows, const vilf_startup_window *windows, int *ints, double *pts);                            // VILF_SU_WIN_INTS per window, then all points
// the chain without its wait and download, for vilf_startup_construct (vilf_ba.hip): validation, upload and launch as vilf_startup_sfm into the caller's buffers; out is
// sized for the chain's download (out_bytes) and extra_out bytes behind it
struct VilfSfmQueued {
    const int *win; const double *pts; const int *l;                                                                    // on the device, as su_sfm_chain reads them
    const vilf_startup_structure *res; const vilf_startup_frame *rows; const unsigned char *state; const double *pos;   // on the device, where su_sfm_chain writes them
    size_t o_res, o_rows, o_state, o_pos, out_bytes;                                                                    // the same four within out, and the chain's bytes
};
int vilf_sfm_enqueue(vilf_handle *h, const char *who, const vilf_startup_sfm_params *p, int n_windows, const vilf_startup_window *windows, const vilf_startup_result *rel,
                     StageIO *io, size_t extra_out, VilfSfmQueued *q);
int vilf_lw_chol_max_n();                                                      // largest n vilf_lw_chol_solve takes (its back substitution keeps the solution in LDS)
int vilf_lw_chol_solve(vilf_handle *h, int n, double *S, double *y, int *info);   // blocked Cholesky solve on the handle's stream (vilf_lw.hip): S = [(n + 1) x n] row-major, row n = rhs
int vilf_lw_group_solve(vilf_handle *h, int G, const vilf_window_in *const *ins, vilf_window_out *const *outs, const int *slot1);   // G windows in one chain of launches; slot1[g] = resident batch slot + 1 (0 / nullptr: not resident)
int vilf_lw_window_solve(vilf_handle *h, const vilf_window_in *in, vilf_window_out *out, int batch_slot1);   // batch_slot1 = resident slot + 1 (0: not resident)   // window sizes other than 10, estimate_extrinsic / estimate_td (vilf_lw.hip)
