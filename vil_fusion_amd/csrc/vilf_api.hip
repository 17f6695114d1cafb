// vilf_api.hip — host side of the C ABI (include/vilfusion.h): packing of window snapshots into the HBM batch layout
// (vilf_batch.hpp), kernel launches on the handle's HIP stream, download. No CPU compute fallback: without a GPU
// vilf_create() fails with VILF_ERR_NO_GPU.
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include <cstring>
#include <cstdio>
#include <cmath>
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <thread>
#include <atomic>
#include <type_traits>
#include "vilf_internal.hpp"
#include "vilf_kernels.hpp"
#include "vilf_sort.hpp"

namespace {

// Frame pairs -> the four wave classes of k_linearize (longest-processing-time: pairs by falling factor count onto the lightest class, ties by pair index:
// deterministic), start of every pair inside its class list, and the number of factor slots (whole chunks) the window needs.
int class_plan(const vilf_window_in &in, int *cls, int *cstart, int *ccount) {
    int pcount[VB_NPAIR] = {0};
    for (int f = 0; f < in.n_features; f++) {
        const int s = in.feature_start_frame[f], n = in.feature_obs_offset[f + 1] - in.feature_obs_offset[f];
        for (int k = 1; k < n; k++) { const int j = s + k; pcount[j * (j - 1) / 2 + s]++; }
    }
    int order[VB_NPAIR], load[4] = {0, 0, 0, 0};
    for (int p = 0; p < VB_NPAIR; p++) order[p] = p;
    std::stable_sort(order, order + VB_NPAIR, [&](int a, int b) { return pcount[a] > pcount[b]; });
    for (int k = 0; k < VB_NPAIR; k++) { const int p = order[k]; int best = 0; for (int c = 1; c < 4; c++) if (load[c] < load[best]) best = c; cls[p] = best; load[best] += pcount[p]; }
    int pos[4] = {0, 0, 0, 0};
    for (int p = 0; p < VB_NPAIR; p++) { cstart[p] = pos[cls[p]]; ccount[p] = pcount[p]; pos[cls[p]] += pcount[p]; }
    const int longest = std::max(std::max(pos[0], pos[1]), std::max(pos[2], pos[3]));
    return VB_CHUNK * std::max(1, (longest + VB_CLS - 1) / VB_CLS);
}

// Row map of W: one row per feature whose depth is a variable, none for a constant one (its row would be all zeros). The reduce of k_solve_sb deals the k-steps of
// four rows to its three waves in turn (k-step s on wave s % 3). Feature f stays on the wave it had when rows were features, (f >> 2) % 3, and every wave keeps its
// features in ascending order, now packed four to a k-step: the j-th variable feature of wave c gets k-step c + 3 (j >> 2), k-slot j & 3. Where the waves' lists differ
// in length the shorter ones end in padding rows (row_feat = -1: never written, zero). n_rows = 4 x k-steps; never more than F rounded up to 4, so the rows fit the
// Fmax rows W always had. The kernels know nothing of this rule: they read f_wrow / row_feat / n_rows.
int w_row_map(int F, int cap, const unsigned char *fconst, int *f_wrow, int *row_feat) {
    int cnt[3] = {0, 0, 0}, nsteps = 0;
    for (int k = 0; k < cap; k++) row_feat[k] = -1;
    for (int f = 0; f < F; f++) {
        if (fconst[f]) { f_wrow[f] = -1; continue; }
        const int c = (f >> 2) % 3, j = cnt[c]++, s = c + 3 * (j >> 2);
        f_wrow[f] = 4 * s + (j & 3); row_feat[4 * s + (j & 3)] = f;
        nsteps = std::max(nsteps, s + 1);
    }
    return 4 * nsteps;
}

void quat_from_R(const double *m, double *q /*xyzw*/) {   // Eigen Quaterniond(Matrix3d)
    double t = m[0] + m[4] + m[8];
    if (t > 0) {
        t = std::sqrt(t + 1.0); q[3] = 0.5 * t; t = 0.5 / t;
        q[0] = (m[7] - m[5]) * t; q[1] = (m[2] - m[6]) * t; q[2] = (m[3] - m[1]) * t;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > m[4 * i]) i = 2;
        int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0);
        q[i] = 0.5 * t; t = 0.5 / t;
        q[3] = (m[3 * k + j] - m[3 * j + k]) * t;
        q[j] = (m[3 * j + i] + m[3 * i + j]) * t;
        q[k] = (m[3 * k + i] + m[3 * i + k]) * t;
    }
}
void quat_to_R(const double *q, double *R) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z, twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}

}  // namespace

// Small batches (the reference's real-time use is ONE window per frame): the host image of an upload goes to the device in ONE copy and a kernel hands its spans
// out to the library's arrays — the ~25 separate copies of the batched path cost 13 us each (4.5 busy + the gap to the next) before the first kernel of a solve
// could start: 0.43 of a single window's 1.7 ms. The same backwards for the results.
struct UpJob { const char *src; char *dst; unsigned long long bytes; };
struct UpJobs { int n; UpJob j[40]; };
__global__ __launch_bounds__(256) void k_copy_spans(UpJobs jobs) {
    const UpJob jb = jobs.j[blockIdx.y];
    const unsigned long long stride = (unsigned long long)gridDim.x * 256, i0 = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if ((((unsigned long long)jb.src | (unsigned long long)jb.dst) & 15ull) == 0) {          // the usual case: 16-byte aligned on both sides
        const unsigned long long n16 = jb.bytes >> 4;
        const uint4 *s4 = reinterpret_cast<const uint4 *>(jb.src); uint4 *d4 = reinterpret_cast<uint4 *>(jb.dst);
        for (unsigned long long i = i0; i < n16; i += stride) d4[i] = s4[i];
        if (blockIdx.x == 0) for (unsigned long long i = (n16 << 4) + threadIdx.x; i < jb.bytes; i += 256) jb.dst[i] = jb.src[i];
    } else if ((((unsigned long long)jb.src | (unsigned long long)jb.dst) & 7ull) == 0) {    // rows of an odd number of doubles, not the first window
        const unsigned long long n8 = jb.bytes >> 3;
        const unsigned long long *s8 = reinterpret_cast<const unsigned long long *>(jb.src); unsigned long long *d8 = reinterpret_cast<unsigned long long *>(jb.dst);
        for (unsigned long long i = i0; i < n8; i += stride) d8[i] = s8[i];
        if (blockIdx.x == 0) for (unsigned long long i = (n8 << 3) + threadIdx.x; i < jb.bytes; i += 256) jb.dst[i] = jb.src[i];
    } else for (unsigned long long i = i0; i < jb.bytes; i += stride) jb.dst[i] = jb.src[i];
}

extern "C" const char *vilf_version(void) { return "vilfusion-hip 0.1 (gfx950)"; }

extern "C" void vilf_default_options(vilf_options *o) {
    std::memset(o, 0, sizeof(*o));
    o->window_size = 10;
    o->max_num_iterations = 8;
    o->max_solver_time = -1.0;
    o->focal_length = 460.0;
    o->cauchy_a = 1.0;
    o->G[2] = 9.81007;
    o->estimate_extrinsic = 0; o->estimate_td = 0; o->use_lidar_const = 1;
    // config/kitti/kitti_config.yaml:10-23,48-61; rotation matrices re-orthonormalised through a quaternion as in
    // vins_estimator/parameters.cpp:108-110,123-125
    const double ric[9] = {0.00781297, -0.0042792, 0.99996, -0.999859, -0.014868, 0.00774856, 0.0148343, -0.99988, -0.00439476};
    const double tic[3] = {1.1439, -0.312718, 0.726546};
    const double rcl[9] = {7.027555e-03, -9.999753e-01, 2.599616e-05, -2.254837e-03, -4.184312e-05, -9.999975e-01, 9.999728e-01, 7.027479e-03, -2.255075e-03};
    const double tcl[3] = {-7.137748e-03, -7.482656e-02, -3.336324e-01};
    double q[4], n;
    quat_from_R(ric, q); n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]); for (double &v : q) v /= n; quat_to_R(q, o->RIC);
    quat_from_R(rcl, q); n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]); for (double &v : q) v /= n; quat_to_R(q, o->RCL);
    for (int i = 0; i < 3; i++) { o->TIC[i] = tic[i]; o->TCL[i] = tcl[i]; }
    o->TR = 0; o->ROW = 370; o->init_depth = 5.0;
    o->edge_leaf_size = 0.4; o->surf_leaf_size = 0.8; o->huber_a = 0.1;
    o->s2m_outer_iterations = 2; o->s2m_max_iterations = 4; o->s2m_crop_half = 100.0;
}

extern "C" int vilf_create(const vilf_options *opts, int device, void *hip_stream, vilf_handle **out) {
    if (!opts || !out) return VILF_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return VILF_ERR_NO_GPU;
    if (device < 0 || device >= ndev) return VILF_ERR_INVALID_ARGUMENT;
    if (opts->window_size < 1 || opts->window_size > 4096) return VILF_ERR_UNSUPPORTED;   // 10 = the reference's compile-time WINDOW_SIZE (batched LDS kernels); other sizes: single-window general path (vilf_lw.hip)
    vilf_handle *h = new vilf_handle();
    h->opts = *opts;
    h->device = device;
    if (hipSetDevice(device) != hipSuccess) { delete h; return VILF_ERR_DEVICE; }
    if (hip_stream) { h->stream = (hipStream_t)hip_stream; h->own_stream = false; }
    // the library's own stream does not synchronise with the legacy default stream: two handles of one process (the estimator and the LiDAR stage, as the reference's
    // separate nodes) run side by side — with a blocking stream every default-stream operation of the process (a torch tensor op, a hipMemcpy) serialised them
    else { if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { delete h; return VILF_ERR_DEVICE; } h->own_stream = true; }
    hipEventCreate(&h->ev0); hipEventCreate(&h->ev1);
    const struct { const void *kernel; int bytes; } dyn_lds[] = {      // the kernels that take more than the default 64 KB of dynamic LDS, or may (totals: vilf_kernels.hpp)
        {(const void *)k_marg_schur, MGS_EXACT_LDS_BYTES}, {(const void *)k_marg_finish, MGF_LDS_BYTES}, {(const void *)k_prior_prep, PRIOR_PREP_LDS_BYTES},
        {(const void *)k_mf_tridiag, MGF_LDS_BYTES}, {(const void *)k_mf_chol, MGF_LDS_BYTES}, {(const void *)k_mf_apply, MGF_LDS_BYTES + MFA_LDS_EXTRA_BYTES},
        {(const void *)k_mf_ql, QL_LDS_BYTES}, {(const void *)k_linearize, VB_LIN_LDS_BYTES}, {(const void *)k_linearize_last, VB_LIN_LDS_BYTES},
        {(const void *)k_linearize_split, VB_LIN_LDS_BYTES}, {(const void *)k_solve, SOLVE_LDS_BYTES}, {(const void *)k_solve_sb, SB_LDS_BYTES}};
    for (const auto &k : dyn_lds)
        if (hipFuncSetAttribute(k.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, k.bytes) != hipSuccess) { delete h; return VILF_ERR_DEVICE; }
    std::memset(&h->batch, 0, sizeof(h->batch));
    // k_solve_sb's gather index table: decoded once on the device (the same arithmetic the kernel used to run per launch), read by every solve
    if (!h->d[D_SBTAB].ensure((size_t)SB_TAB_ROWS * SBT * 16)) { delete h; return VILF_ERR_DEVICE; }
    hipLaunchKernelGGL(k_sb_table, dim3(1), dim3(SBT), 0, h->stream, h->d[D_SBTAB].as<int>());
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) { delete h; return VILF_ERR_DEVICE; }
    *out = h;
    return VILF_OK;
}

extern "C" void vilf_destroy(vilf_handle *h) {
    if (!h) return;
    hipSetDevice(h->device);
    hipStreamSynchronize(h->stream);
    for (int s = 0; s < VILF_STAGE_COUNT; s++) vilf_stage_drop(h, s);
    for (auto &b : h->d) b.release();
    h->pin_up.release(); h->pin_down.release();
    if (h->ev0) hipEventDestroy(h->ev0);
    if (h->ev1) hipEventDestroy(h->ev1);
    for (hipEvent_t e : h->prof_used) hipEventDestroy(e);
    for (hipEvent_t e : h->prof_free) hipEventDestroy(e);
    if (h->wait_ev) hipEventDestroy(h->wait_ev);
    if (h->stamp_ev) hipEventDestroy(h->stamp_ev);
    if (h->stamp_pinned) (void)hipHostFree(h->stamp_pinned);
    h->s2m_ev.clear(); h->prof_used.clear(); h->prof_free.clear(); h->prof_pending.clear();
    if (h->own_stream) hipStreamDestroy(h->stream);
    delete h;
}

// ---- deferred profile spans (see vilf_handle::prof_pending)
hipEvent_t vilf_prof_event(vilf_handle *h) {
    hipEvent_t e = nullptr;
    if (!h->prof_free.empty()) { e = h->prof_free.back(); h->prof_free.pop_back(); } else hipEventCreate(&e);
    h->prof_used.push_back(e);
    hipEventRecord(e, h->stream);
    return e;
}
void vilf_prof_span(vilf_handle *h, hipEvent_t a, hipEvent_t b, double *ms, long *cnt) { h->prof_pending.push_back(vilf_handle::ProfSpan{a, b, ms, cnt}); }
int vilf_prof_flush(vilf_handle *h) {
    if (h->prof_used.empty()) return VILF_OK;
    HIPCHECK(h, hipStreamSynchronize(h->stream));
    for (const vilf_handle::ProfSpan &p : h->prof_pending) { float t = 0; hipEventElapsedTime(&t, p.a, p.b); *p.ms += t; *p.cnt += 1; }
    h->prof_pending.clear();
    for (hipEvent_t e : h->prof_used) h->prof_free.push_back(e);
    h->prof_used.clear();
    return VILF_OK;
}
// The work enqueued on h's stream from now on starts after everything enqueued on other's stream so far has finished: a dependency on the device, the host
// does not wait. (The LiDAR stage and the window solve of a frame run on two handles: this orders them without a host round trip between them.)
extern "C" int vilf_set_async_upload(vilf_handle *h, int on) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    h->async_upload = on != 0;
    return VILF_OK;
}
extern "C" int vilf_wait_for(vilf_handle *h, vilf_handle *other) {
    if (!h || !other) return VILF_ERR_INVALID_ARGUMENT;
    if (h->device != other->device) { h->err = "vilf_wait_for: the handles are on different devices"; return VILF_ERR_INVALID_ARGUMENT; }
    if (h == other || h->stream == other->stream) return VILF_OK;
    HIPCHECK(h, hipSetDevice(h->device));
    if (!h->wait_ev) HIPCHECK(h, hipEventCreateWithFlags(&h->wait_ev, hipEventDisableTiming));
    HIPCHECK(h, hipEventRecord(h->wait_ev, other->stream));
    HIPCHECK(h, hipStreamWaitEvent(h->stream, h->wait_ev, 0));
    return VILF_OK;
}

extern "C" const char *vilf_last_error(const vilf_handle *h) { return h ? h->err.c_str() : "null handle"; }

extern "C" int vilf_reset(vilf_handle *h) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    for (auto &p : h->priors) p.valid = 0;
    std::fill(h->prior_dirty.begin(), h->prior_dirty.end(), 1);
    std::fill(h->prior_dev_newer.begin(), h->prior_dev_newer.end(), 0);
    return VILF_OK;
}

extern "C" int vilf_synchronize(vilf_handle *h) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    HIPCHECK(h, hipStreamSynchronize(h->stream));
    { const int rcf = vilf_prof_flush(h); if (rcf != VILF_OK) return rcf; }      // pending profile spans: the stream is idle, reading them costs nothing
    return VILF_OK;
}

static int pull_device_priors(vilf_handle *h) {
    if (!h->resident) return VILF_OK;
    for (int w = 0; w < h->B && w < (int)h->prior_dev_newer.size(); w++) {
        if (!h->prior_dev_newer[w]) continue;
        vilf_prior &p = h->priors[w];
        std::memset(&p, 0, sizeof(p));
        int hdr[VB_PRIOR_HDR];
        HIPCHECK(h, vilf_copy_sync(h, hdr, h->d[D_PHDR].as<int>() + (size_t)w * VB_PRIOR_HDR, sizeof(hdr), hipMemcpyDeviceToHost));
        p.valid = hdr[0]; p.n = hdr[1]; p.n_blocks = hdr[2]; p.m = hdr[75];
        if (p.valid) {
            std::vector<double> x0(VB_PRIOR_X0_LD);
            HIPCHECK(h, vilf_copy_sync(h, x0.data(), h->d[D_PX0].as<double>() + (size_t)w * VB_PRIOR_X0_LD, x0.size() * 8, hipMemcpyDeviceToHost));
            for (int i = 0; i < p.n_blocks; i++) { p.block_id[i] = hdr[3 + i]; p.block_size[i] = hdr[27 + i]; p.block_idx[i] = hdr[51 + i]; for (int k = 0; k < 9; k++) p.block_x0[i][k] = x0[i * 9 + k]; }
            HIPCHECK(h, vilf_copy_sync(h, p.linearized_jacobians, h->d[D_PJ].as<double>() + (size_t)w * VB_PRIOR_LD * VB_PRIOR_LD, sizeof(double) * p.n * p.n, hipMemcpyDeviceToHost));
            HIPCHECK(h, vilf_copy_sync(h, p.linearized_residuals, h->d[D_PR].as<double>() + (size_t)w * VB_PRIOR_LD, sizeof(double) * p.n, hipMemcpyDeviceToHost));
        }
        h->prior_dev_newer[w] = 0;
    }
    return VILF_OK;
}

// host -> device for the slots whose host mirror changed (vilf_prior_import, first upload). Slots whose prior was produced on the
// device (marginalization) or is unchanged are left alone: in the running system the prior never crosses PCIe.
static int upload_priors(vilf_handle *h) {
    const int B = h->B;
    std::vector<int> dirty;
    for (int w = 0; w < B; w++) if (h->prior_dirty[w]) dirty.push_back(w);
    if (dirty.empty()) return VILF_OK;
    h->prior_backup_valid = false; h->prior_restore_needed = false;
    for (int w : dirty) {
        const vilf_prior &p = h->priors[w];
        h->prior_dev_newer[w] = 0;
        if (p.valid) for (int i = 0; i < p.n_blocks; i++) if (p.block_id[i] > 2 * VB_NF + (h->opts.estimate_td ? 1 : 0)) { h->err = "prior touches feature blocks (or Td without estimate_td): unsupported"; return VILF_ERR_UNSUPPORTED; }
        char dense_w = 0;
        if (p.valid) for (int i = 0; i < p.n_blocks; i++) if (p.block_id[i] > VB_NF && p.block_id[i] < 2 * VB_NF) dense_w = 1;
        if ((int)h->prior_dense.size() <= w) h->prior_dense.resize(w + 1, 0);
        h->prior_dense_count += dense_w - h->prior_dense[w]; h->prior_dense[w] = dense_w;
    }
    h->solve_dense_fallback = h->prior_dense_count > 0;      // recomputed with every upload: a later prior without such a block returns the handle to k_solve_sb
    auto fill = [&](const vilf_prior &p, int *hd, double *x0) {
        std::memset(hd, 0, VB_PRIOR_HDR * sizeof(int)); std::memset(x0, 0, VB_PRIOR_X0_LD * sizeof(double));
        if (!p.valid) return;
        hd[0] = 1; hd[1] = p.n; hd[2] = p.n_blocks; hd[75] = p.m;
        for (int i = 0; i < p.n_blocks; i++) {
            hd[3 + i] = p.block_id[i]; hd[27 + i] = p.block_size[i]; hd[51 + i] = p.block_idx[i];
            for (int k = 0; k < 9; k++) x0[i * 9 + k] = p.block_x0[i][k];
        }
    };
    if ((int)dirty.size() * 4 > B) {          // most slots: one bulk copy per array
        std::vector<int> hdr((size_t)B * VB_PRIOR_HDR, 0);
        std::vector<double> x0((size_t)B * VB_PRIOR_X0_LD, 0.0), J((size_t)B * VB_PRIOR_LD * VB_PRIOR_LD, 0.0), r((size_t)B * VB_PRIOR_LD, 0.0);
        if ((int)dirty.size() < B) {           // keep what the other slots hold on the device
            { int rcp = pull_device_priors(h); if (rcp != VILF_OK) return rcp; }
            for (int w = 0; w < B; w++) h->prior_dirty[w] = 1;
        }
        for (int w = 0; w < B; w++) {
            const vilf_prior &p = h->priors[w];
            fill(p, &hdr[(size_t)w * VB_PRIOR_HDR], &x0[(size_t)w * VB_PRIOR_X0_LD]);
            if (!p.valid) continue;
            std::memcpy(&J[(size_t)w * VB_PRIOR_LD * VB_PRIOR_LD], p.linearized_jacobians, sizeof(double) * p.n * p.n);
            std::memcpy(&r[(size_t)w * VB_PRIOR_LD], p.linearized_residuals, sizeof(double) * p.n);
        }
        HIPCHECK(h, hipMemcpyAsync(h->d[D_PHDR].p, hdr.data(), hdr.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
        HIPCHECK(h, hipMemcpyAsync(h->d[D_PX0].p, x0.data(), x0.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHECK(h, hipMemcpyAsync(h->d[D_PJ].p, J.data(), J.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHECK(h, hipMemcpyAsync(h->d[D_PR].p, r.data(), r.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHECK(h, hipStreamSynchronize(h->stream));   // host vectors go out of scope
    } else {                                   // a few slots: per-slot copies
        for (int w : dirty) {
            const vilf_prior &p = h->priors[w];
            int hd[VB_PRIOR_HDR]; double x0[VB_PRIOR_X0_LD];
            fill(p, hd, x0);
            HIPCHECK(h, hipMemcpyAsync(h->d[D_PHDR].as<int>() + (size_t)w * VB_PRIOR_HDR, hd, sizeof(hd), hipMemcpyHostToDevice, h->stream));
            HIPCHECK(h, hipMemcpyAsync(h->d[D_PX0].as<double>() + (size_t)w * VB_PRIOR_X0_LD, x0, sizeof(x0), hipMemcpyHostToDevice, h->stream));
            if (p.valid) {
                HIPCHECK(h, hipMemcpyAsync(h->d[D_PJ].as<double>() + (size_t)w * VB_PRIOR_LD * VB_PRIOR_LD, p.linearized_jacobians, sizeof(double) * p.n * p.n, hipMemcpyHostToDevice, h->stream));
                HIPCHECK(h, hipMemcpyAsync(h->d[D_PR].as<double>() + (size_t)w * VB_PRIOR_LD, p.linearized_residuals, sizeof(double) * p.n, hipMemcpyHostToDevice, h->stream));
            }
            HIPCHECK(h, hipStreamSynchronize(h->stream));   // hd / x0 are stack buffers
        }
    }
    hipLaunchKernelGGL(k_prior_prep, dim3(B), dim3(VB_NT), PRIOR_PREP_LDS_BYTES, h->stream, h->batch, h->d[D_PH].as<double>(), h->d[D_PG].as<double>(), (unsigned)PRIOR_PREP_LDS_BYTES, (const int *)nullptr);
    HIPCHECK(h, hipGetLastError());
    for (int w = 0; w < B; w++) h->prior_dirty[w] = 0;
    h->prior_slots_valid = std::max(h->prior_slots_valid, B);
    return VILF_OK;
}

// ---- the window batch's device arrays ---------------------------------------------------------------------------------
// One row per per-window array. Everything vilf_batch_upload does with an array — the device allocation, its span of the pinned staging, the per-window-range
// copies, the job list of the staged copy kernel, the whole-batch copies of the small arrays — is derived from this table; bind_batch_arrays is the one other place
// that lists the arrays (it names the VbBatch fields). A new uploaded array is an enum entry (vilf_internal.hpp), a row here, a line in bind_batch_arrays and
// the packer's writes (pack_window).
enum ArrayUse : uint8_t {
    A_WINDOW,      // packed per window, copied per range of windows (large batches: the copies of a quarter overlap the packing of the next)
    A_WINDOW_TD,   // the same with estimate_td; without it an 8-byte placeholder that nothing reads
    A_SMALL,       // packed per window, copied as one whole-batch array once every window is packed
    A_PRIOR,       // written by upload_priors / the marginalization; twin = the same array of the second prior set (allocated by the first marginalization)
    A_WORK,        // not uploaded: trial point, workspace, results
};
struct BatchDims { size_t B, F, O, C; bool est_td; };      // windows, Fmax, Omax, FACmax of an upload
struct ArrayRow {
    int id; size_t elem;          // buffer; bytes per element
    int k, f, o, c;               // elements per window = k + f Fmax + o Omax + c FACmax
    ArrayUse use;
    int twin = -1;                // a second buffer of the same size: of an uploaded array the *_init copy the same host span also seeds; of a prior array see A_PRIOR
    int copies = 1;               // 2: one per linearisation workspace (VbState::ws)
    size_t per_window(const BatchDims &d) const { return elem * (k + f * d.F + o * d.O + c * d.C); }
    size_t bytes(const BatchDims &d) const { return use == A_WINDOW_TD && !d.est_td ? 8 : copies * d.B * per_window(d); }
    bool by_range(const BatchDims &d) const { return use == A_WINDOW || (use == A_WINDOW_TD && d.est_td); }
    bool uploaded(const BatchDims &d) const { return by_range(d) || use == A_SMALL; }
};
constexpr ArrayRow kBatchArrays[] = {
    // uploaded per window, in the order their copies are enqueued
    {D_POSE, 8, VB_POSE_LD, 0, 0, 0, A_WINDOW, D_POSE0}, {D_SB, 8, VB_SB_LD, 0, 0, 0, A_WINDOW, D_SB0}, {D_FEAT, 8, 0, 1, 0, 0, A_WINDOW, D_FEAT0},
    {D_FSTART, 4, 0, 1, 0, 0, A_WINDOW}, {D_FNOBS, 4, 0, 1, 0, 0, A_WINDOW}, {D_FFAC0, 4, 0, 1, 0, 0, A_WINDOW}, {D_FCONST, 1, 0, 1, 0, 0, A_WINDOW}, {D_PSSLOT, 4, 0, 0, 0, 1, A_WINDOW},
    {D_FWROW, 4, 0, 1, 0, 0, A_WINDOW}, {D_ROWFEAT, 4, 0, 1, 0, 0, A_WINDOW},      // the row map of W (w_row_map)
    {D_FOBS0, 4, 0, 1, 0, 0, A_WINDOW_TD}, {D_PSOBS, 4, 0, 0, 0, 1, A_WINDOW_TD},      // observation indices: only the td factors of k_marg_prepare look an observation up
    {D_FACREC, 8, 0, 0, 0, 8, A_WINDOW}, {D_IMU, 8, VB_IMU_LD, 0, 0, 0, A_WINDOW}, {D_LIDAR, 8, VB_LIDAR_LD, 0, 0, 0, A_WINDOW}, {D_COV, 8, VB_COV_LD, 0, 0, 0, A_WINDOW},
    {D_OBSV, 8, 0, 0, 2, 0, A_WINDOW_TD}, {D_OBSTD, 8, 0, 0, 1, 0, A_WINDOW_TD}, {D_OBSROW, 8, 0, 0, 1, 0, A_WINDOW_TD},
    // uploaded whole, in that order
    {D_NFEAT, 4, 1, 0, 0, 0, A_SMALL}, {D_NFAC, 4, 1, 0, 0, 0, A_SMALL}, {D_EX, 8, VB_EX_LD, 0, 0, 0, A_SMALL}, {D_GR0, 8, 9, 0, 0, 0, A_SMALL}, {D_GP0, 8, 3, 0, 0, 0, A_SMALL},
    {D_PAIROFF, 4, VB_PTAB, 0, 0, 0, A_SMALL}, {D_MFLAG, 4, 1, 0, 0, 0, A_SMALL}, {D_TD, 8, 1, 0, 0, 0, A_SMALL}, {D_NROWS, 4, 1, 0, 0, 0, A_SMALL},
    // the two prior sets: live, and as uploaded (restored by vilf_batch_rewind after a marginalization)
    {D_PHDR, 4, VB_PRIOR_HDR, 0, 0, 0, A_PRIOR, D_PHDR0}, {D_PX0, 8, VB_PRIOR_X0_LD, 0, 0, 0, A_PRIOR, D_PX00}, {D_PJ, 8, VB_PRIOR_LD * VB_PRIOR_LD, 0, 0, 0, A_PRIOR, D_PJ0},
    {D_PR, 8, VB_PRIOR_LD, 0, 0, 0, A_PRIOR, D_PR0}, {D_PH, 8, VB_PRIOR_LD * VB_PRIOR_LD, 0, 0, 0, A_PRIOR, D_PH0}, {D_PG, 8, VB_PRIOR_LD, 0, 0, 0, A_PRIOR, D_PG0},
    // trial point, workspace, results
    {D_CPOSE, 8, VB_POSE_LD, 0, 0, 0, A_WORK}, {D_CSB, 8, VB_SB_LD, 0, 0, 0, A_WORK}, {D_CFEAT, 8, 0, 1, 0, 0, A_WORK}, {D_CF, 8, 0, 1, 0, 0, A_WORK},
    {D_FACW, 8, 0, 0, 0, VB_FACW, A_WORK}, {D_HPP, 8, 66 * 36, 0, 0, 0, A_WORK, -1, 2}, {D_W, 8, 0, VB_WLD, 0, 0, A_WORK, -1, 2}, {D_HF, 8, 0, 1, 0, 0, A_WORK, -1, 2},
    {D_GF, 8, 0, 1, 0, 0, A_WORK, -1, 2}, {D_IMUH, 8, 9000, 0, 0, 0, A_WORK, -1, 2}, {D_IMUG, 8, 300, 0, 0, 0, A_WORK, -1, 2}, {D_LIDH, 8, 1440, 0, 0, 0, A_WORK, -1, 2},
    {D_LIDG, 8, 120, 0, 0, 0, A_WORK, -1, 2}, {D_G, 8, VB_P, 0, 0, 0, A_WORK, -1, 2}, {D_DIAGH, 8, VB_P, 0, 0, 0, A_WORK, -1, 2}, {D_PAIRD, 8, VB_NPAIR * VB_PAIRD, 0, 0, 0, A_WORK, -1, 2},
    {D_SCALE, 8, VB_P, 1, 0, 0, A_WORK}, {D_DIAG, 8, VB_P, 1, 0, 0, A_WORK}, {D_GRAD, 8, VB_P, 1, 0, 0, A_WORK}, {D_GN, 8, VB_P, 1, 0, 0, A_WORK},
    {D_ST, sizeof(VbState), 1, 0, 0, 0, A_WORK}, {D_OPS, 8, VB_OUT3_LD, 0, 0, 0, A_WORK}, {D_ORS, 8, VB_OUTR_LD, 0, 0, 0, A_WORK}, {D_OVS, 8, VB_OUT3_LD, 0, 0, 0, A_WORK},
    {D_OBAS, 8, VB_OUT3_LD, 0, 0, 0, A_WORK}, {D_OBGS, 8, VB_OUT3_LD, 0, 0, 0, A_WORK}, {D_WORK, 8, 10 * 450, 0, 0, 0, A_WORK},
};
constexpr int upload_destinations() { int n = 0; for (const ArrayRow &r : kBatchArrays) if (r.use <= A_SMALL) n += 1 + (r.twin >= 0); return n; }
static_assert(upload_destinations() <= (int)(sizeof(UpJobs::j) / sizeof(UpJob)), "the staged upload hands every destination to ONE launch of k_copy_spans");
static size_t batch_array_bytes(int id, const BatchDims &d) { for (const ArrayRow &r : kBatchArrays) if (r.id == id) return r.bytes(d); return 0; }

// the batch descriptor's view of the live prior set, and the swap of the two sets (vilf_batch_marginalize / vilf_batch_rewind: no copy)
static void bind_prior_pointers(vilf_handle *h) {
    VbBatch &b = h->batch;
    b.prior_hdr = h->d[D_PHDR].as<int>(); b.prior_x0 = h->d[D_PX0].as<double>(); b.prior_J = h->d[D_PJ].as<double>(); b.prior_r = h->d[D_PR].as<double>();
    b.prior_H = h->d[D_PH].as<double>(); b.prior_g = h->d[D_PG].as<double>();
}
static void swap_prior_sets(vilf_handle *h) {
    for (const ArrayRow &r : kBatchArrays) if (r.use == A_PRIOR) std::swap(h->d[r.id], h->d[r.twin]);
    bind_prior_pointers(h);
}
// qil = Quaterniond(RIC*RCL), til = RIC*TCL + TIC (lidar_factor.h:28-29)
static void lidar_extrinsic(const vilf_options &o, VbBatch &b) {
    double M[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) M[3 * i + j] = o.RIC[3 * i] * o.RCL[j] + o.RIC[3 * i + 1] * o.RCL[3 + j] + o.RIC[3 * i + 2] * o.RCL[6 + j];
    quat_from_R(M, b.qil);
    for (int i = 0; i < 3; i++) b.til[i] = o.RIC[3 * i] * o.TCL[0] + o.RIC[3 * i + 1] * o.TCL[1] + o.RIC[3 * i + 2] * o.TCL[2] + o.TIC[i];
}
// the batch descriptor: options, sizes and the typed pointers into the arrays of the table
static void bind_batch_arrays(vilf_handle *h, const BatchDims &dm) {
    VbBatch &b = h->batch;
    std::memset(&b, 0, sizeof(b));          // (obs, ps_feat, dbg, the live / split lists: null)
    const vilf_options &o = h->opts;
    b.B = (int)dm.B; b.w0 = 0; b.Fmax = (int)dm.F; b.Omax = (int)dm.O; b.FACmax = (int)dm.C;
    b.sqrt_info = o.focal_length / 1.5; b.cauchy_b = o.cauchy_a * o.cauchy_a;
    for (int i = 0; i < 3; i++) b.G[i] = o.G[i];
    lidar_extrinsic(o, b);
    b.use_lidar = o.use_lidar_const; b.max_iterations = o.max_num_iterations;
    b.min_relative_decrease = 1e-3; b.function_tolerance = 1e-6; b.gradient_tolerance = 1e-10; b.parameter_tolerance = 1e-8;
    b.min_radius = 1e-32; b.initial_radius = 1e4; b.min_lm_diagonal = 1e-6; b.max_lm_diagonal = 1e32;
    b.est_td = o.estimate_td ? 1 : 0; b.tr_over_row = o.TR / o.ROW; b.row_half = o.ROW / 2;
    DBuf *d = h->d;
    b.n_feat = d[D_NFEAT].as<int>(); b.n_fac = d[D_NFAC].as<int>(); b.pose = d[D_POSE].as<double>(); b.sb = d[D_SB].as<double>(); b.feat = d[D_FEAT].as<double>();
    b.cand_pose = d[D_CPOSE].as<double>(); b.cand_sb = d[D_CSB].as<double>(); b.cand_feat = d[D_CFEAT].as<double>();
    b.pose_init = d[D_POSE0].as<double>(); b.sb_init = d[D_SB0].as<double>(); b.feat_init = d[D_FEAT0].as<double>();
    b.ex = d[D_EX].as<double>(); b.gauge_R0 = d[D_GR0].as<double>(); b.gauge_P0 = d[D_GP0].as<double>(); b.td = d[D_TD].as<double>();
    b.f_start = d[D_FSTART].as<int>(); b.f_nobs = d[D_FNOBS].as<int>(); b.f_obs0 = d[D_FOBS0].as<int>(); b.f_fac0 = d[D_FFAC0].as<int>(); b.f_const = d[D_FCONST].as<uint8_t>();
    b.f_wrow = d[D_FWROW].as<int>(); b.row_feat = d[D_ROWFEAT].as<int>(); b.n_rows = d[D_NROWS].as<int>();
    b.obs_vel = d[D_OBSV].as<double>(); b.obs_ctd = d[D_OBSTD].as<double>(); b.obs_row = d[D_OBSROW].as<double>(); b.ps_obs = d[D_PSOBS].as<int>(); b.ps_slot = d[D_PSSLOT].as<int>();
    b.pair_off = d[D_PAIROFF].as<int>(); b.facrec = d[D_FACREC].as<double>(); b.imu = d[D_IMU].as<double>(); b.lidar = d[D_LIDAR].as<double>();
    bind_prior_pointers(h);
    b.facw = d[D_FACW].as<double>(); b.Hpp = d[D_HPP].as<double>(); b.W = d[D_W].as<double>(); b.hf = d[D_HF].as<double>(); b.gf = d[D_GF].as<double>(); b.cf = d[D_CF].as<double>();
    b.imuH = d[D_IMUH].as<double>(); b.imug = d[D_IMUG].as<double>(); b.lidH = d[D_LIDH].as<double>(); b.lidg = d[D_LIDG].as<double>(); b.g = d[D_G].as<double>();
    b.diagH = d[D_DIAGH].as<double>(); b.pairD = d[D_PAIRD].as<double>(); b.scale = d[D_SCALE].as<double>(); b.diag = d[D_DIAG].as<double>(); b.grad = d[D_GRAD].as<double>(); b.gn = d[D_GN].as<double>();
    b.st = d[D_ST].as<VbState>(); b.out_Ps = d[D_OPS].as<double>(); b.out_Rs = d[D_ORS].as<double>(); b.out_Vs = d[D_OVS].as<double>(); b.out_Bas = d[D_OBAS].as<double>(); b.out_Bgs = d[D_OBGS].as<double>();
    b.sb_tab = d[D_SBTAB].as<int>();
}

// ---- vilf_batch_upload, stage by stage ------------------------------------------------------------------------------------
namespace {
struct Lap {        // VILF_DEBUG_TIMING: host time of every phase of an upload to stderr (tools/dev_upload_timing.py)
    const bool on = std::getenv("VILF_DEBUG_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void operator()(const char *what) { if (on) { const auto now = std::chrono::steady_clock::now(); fprintf(stderr, "[vilf_batch_upload] %-28s %.2f ms\n", what, std::chrono::duration<double, std::milli>(now - t).count()); t = now; } }
};
// what the stages of one upload share: the caller's windows, the batch maxima, and each uploaded array's span of the pinned staging
struct Upload {
    vilf_handle *h; const vilf_window_in *wins;
    int nthr;                       // host threads of the validation and the packing
    BatchDims dims;
    bool keep_inputs;               // estimate_extrinsic / estimate_td: the batched solve runs the general path per slot and needs the inputs again (OwnedWindow)
    char *image; size_t image_bytes;      // the pinned staging; its bytes in use, rounded up to 64
    size_t at[D_COUNT], ld[D_COUNT];      // per buffer id: where its span starts in the image (uploaded arrays only), bytes per window
    template <typename T> T *row(int id, int w) const { return reinterpret_cast<T *>(image + at[id] + (size_t)w * ld[id]); }
};
// validation of one window; nullptr = accepted. *mf: its features that start in frame 0 (the marginalization drops them with the oldest frame)
const char *check_window(const vilf_options &o, const vilf_window_in &in, int *mf) {
    if (in.n_frames != VB_NF) return "n_frames must be window_size + 1 = 11";
    if (in.n_features < 0 || in.n_features > VILF_MAX_FEATURES) return "n_features out of range";
    if (!in.para_pose || !in.para_speed_bias || !in.imu || (in.n_features && (!in.para_feature || !in.feature_const || !in.feature_start_frame || !in.feature_obs_offset || !in.obs_point)))
        return "null input array";
    if (o.use_lidar_const && !in.lidar) return "lidar constraints missing (use_lidar_const = 1)";
    if (o.estimate_td && in.n_features && (!in.obs_velocity || !in.obs_cur_td || !in.obs_row)) return "estimate_td needs obs_velocity / obs_cur_td / obs_row";
    // the observation CSR must be exactly [0 .. n_obs): the packer indexes obs_point / the factor arrays through it
    if (in.n_obs < 0 || (in.n_features && (in.feature_obs_offset[0] != 0 || in.feature_obs_offset[in.n_features] != in.n_obs)) || (!in.n_features && in.n_obs != 0))
        return "feature_obs_offset must start at 0 and end at n_obs";
    *mf = 0;
    for (int f = 0; f < in.n_features; f++) {
        const int s = in.feature_start_frame[f], n = in.feature_obs_offset[f + 1] - in.feature_obs_offset[f];     // n >= 2 also makes the offsets increasing
        if (s < 0 || n < 2 || s + n > VB_NF) return "feature track outside the window";
        if (s == 0) (*mf)++;
    }
    return nullptr;
}
// Stage 1: validation, the class plan of every window (h->plans, kept for the packer) and the batch-wide maxima (u.dims, h->mg_Mcap), on the host threads: one thread
// took 4.3 of the 16.5 ms a 2048-window upload cost
int plan_windows(Upload &u, int B) {
    vilf_handle *h = u.h;
    struct Local { int F = 4, O = 4, C = 4, M = 2; const char *err = nullptr; };
    std::vector<Local> loc(u.nthr);
    h->plans.resize(B);
    auto check = [&](int t) {
        Local &L = loc[t];
        for (int w = t; w < B; w += u.nthr) {
            const vilf_window_in &in = u.wins[w]; int mf = 0;
            if (const char *msg = check_window(h->opts, in, &mf)) { if (!L.err) L.err = msg; continue; }
            WindowPlan &pl = h->plans[w];
            pl.nslot = class_plan(in, pl.cls, pl.cstart, pl.ccount);
            L.C = std::max(L.C, pl.nslot); L.F = std::max(L.F, in.n_features); L.O = std::max(L.O, in.n_obs); L.M = std::max(L.M, MG_MD + mf + 1);
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < u.nthr; t++) pool.emplace_back(check, t);
    check(0);                                    // (the calling thread takes a share)
    for (std::thread &th : pool) th.join();
    Local m;
    for (const Local &L : loc) {
        if (L.err) { h->err = L.err; return VILF_ERR_INVALID_ARGUMENT; }
        m.F = std::max(m.F, L.F); m.O = std::max(m.O, L.O); m.C = std::max(m.C, L.C); m.M = std::max(m.M, L.M);
    }
    u.dims = BatchDims{(size_t)B, (size_t)((m.F + 3) & ~3), (size_t)m.O, (size_t)((m.C + 63) & ~63), h->opts.estimate_td != 0};
    h->mg_Mcap = (m.M + 1) & ~1;
    return VILF_OK;
}
// Stage 2: the device buffers of the table (the second prior set is the marginalization's) and the persistent PINNED staging, one 64-byte-aligned span per
// uploaded array: allocating and zero-filling ~250 MB of std::vectors per call was half of the upload time, and copies from pageable memory are neither fast nor
// asynchronous. Every slice a kernel reads is rewritten by pack_window; padding is never read.
int reserve(Upload &u, Lap &lap) {
    vilf_handle *h = u.h;
    size_t off = 0;
    for (const ArrayRow &r : kBatchArrays) {
        const size_t bytes = r.bytes(u.dims);
        if (!h->d[r.id].ensure(bytes) || (r.twin >= 0 && r.use != A_PRIOR && !h->d[r.twin].ensure(bytes))) { h->err = "hipMalloc failed"; return VILF_ERR_DEVICE; }
        u.ld[r.id] = r.per_window(u.dims);
        if (!r.uploaded(u.dims)) continue;
        u.at[r.id] = off = (off + 63) & ~(size_t)63;
        off += u.dims.B * u.ld[r.id];
    }
    lap("validate + device buffers");
    u.image_bytes = (off + 63) & ~(size_t)63;
    if (!h->pin_up.ensure(off + 64)) { h->err = "hipHostMalloc failed (upload staging)"; return VILF_ERR_DEVICE; }
    u.image = static_cast<char *>(h->pin_up.p);
    // the host's own mirrors of what the read-back needs without a copy; the retained inputs
    h->h_nfeat.assign(u.dims.B, 0); h->h_ex.assign(u.dims.B * VB_EX_LD, 0.0); h->h_td.assign(u.dims.B, 0.0);
    h->own.clear(); h->own.resize(u.keep_inputs ? u.dims.B : 0);
    lap("host vectors");
    return VILF_OK;
}
void fill_imu_rec(const vilf_imu_preint &p, double *rec) {      // the raw part of an IMU record (layout: vilf_device.hpp); rec[287], the factor's weight, is the caller's
    rec[0] = p.sum_dt;
    for (int i = 0; i < 3; i++) { rec[1 + i] = p.delta_p[i]; rec[8 + i] = p.delta_v[i]; rec[11 + i] = p.linearized_ba[i]; rec[14 + i] = p.linearized_bg[i]; }
    for (int i = 0; i < 4; i++) rec[4 + i] = p.delta_q[i];
    auto blk = [&](int off, int r0, int c0) { for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) rec[off + 3 * i + j] = p.jacobian[(r0 + i) * 15 + c0 + j]; };
    blk(17, 0, 9); blk(26, 0, 12); blk(35, 3, 12); blk(44, 6, 9); blk(53, 6, 12);
}
void retain_window(OwnedWindow &o, const vilf_window_in &in) {      // deep copy: the caller's arrays need not outlive the upload
    const size_t F = in.n_features, O = in.n_obs;
    auto keep = [](auto &v, auto *&p, size_t n) { if (p) { v.assign(p, p + n); p = v.empty() ? nullptr : v.data(); } };      // the copy's pointer follows its data
    o.in = in;
    keep(o.pose, o.in.para_pose, VB_POSE_LD); keep(o.sb, o.in.para_speed_bias, VB_SB_LD); keep(o.feat, o.in.para_feature, F); keep(o.fconst, o.in.feature_const, F);
    keep(o.fstart, o.in.feature_start_frame, F); keep(o.foff, o.in.feature_obs_offset, F + 1); keep(o.obs, o.in.obs_point, 3 * O);
    keep(o.vel, o.in.obs_velocity, 2 * O); keep(o.ctd, o.in.obs_cur_td, O); keep(o.row, o.in.obs_row, O);
    keep(o.imu, o.in.imu, VB_NF); keep(o.lidar, o.in.lidar, VB_NF); keep(o.gR0, o.in.gauge_R0, 9); keep(o.gP0, o.in.gauge_P0, 3);
}
// Stage 3: one window into its slices of the staging (and of the host mirrors). A window writes its own slices only: safe from several host threads.
void pack_window(const Upload &u, int w) {
    vilf_handle *h = u.h;
    const vilf_window_in &in = u.wins[w];
    const int F = in.n_features;
    *u.row<int>(D_NFEAT, w) = F; h->h_nfeat[w] = F; *u.row<int>(D_MFLAG, w) = in.marginalization_flag;
    *u.row<double>(D_TD, w) = in.para_td; h->h_td[w] = in.para_td;
    std::memcpy(u.row<double>(D_POSE, w), in.para_pose, VB_POSE_LD * 8); std::memcpy(u.row<double>(D_SB, w), in.para_speed_bias, VB_SB_LD * 8);
    std::memcpy(u.row<double>(D_EX, w), in.para_ex_pose, VB_EX_LD * 8); std::memcpy(&h->h_ex[(size_t)w * VB_EX_LD], in.para_ex_pose, VB_EX_LD * 8);
    if (in.gauge_R0) std::memcpy(u.row<double>(D_GR0, w), in.gauge_R0, 72); else quat_to_R(in.para_pose + 3, u.row<double>(D_GR0, w));
    std::memcpy(u.row<double>(D_GP0, w), in.gauge_P0 ? in.gauge_P0 : in.para_pose, 24);
    if (u.dims.est_td && in.n_obs) {
        std::memcpy(u.row<double>(D_OBSV, w), in.obs_velocity, (size_t)in.n_obs * 16);
        std::memcpy(u.row<double>(D_OBSTD, w), in.obs_cur_td, (size_t)in.n_obs * 8);
        std::memcpy(u.row<double>(D_OBSROW, w), in.obs_row, (size_t)in.n_obs * 8);
    }
    if (u.keep_inputs) retain_window(h->own[w], in);
    // the pair table and the factor slots: null records first (flag bit 17; the kernels sweep slots), then every factor at the next slot of its pair's class list
    const WindowPlan &pl = h->plans[w];
    *u.row<int>(D_NFAC, w) = pl.nslot;
    int cur[VB_NPAIR], *po = u.row<int>(D_PAIROFF, w);
    for (int p = 0; p < VB_NPAIR; p++) { po[2 * p] = pl.cstart[p]; po[2 * p + 1] = pl.ccount[p] | (pl.cls[p] << 24); cur[p] = pl.cstart[p]; }
    po[2 * VB_NPAIR] = 0; po[2 * VB_NPAIR + 1] = 0;
    double *facrec = u.row<double>(D_FACREC, w), *feat = u.row<double>(D_FEAT, w);
    int *psslot = u.row<int>(D_PSSLOT, w), *fstart = u.row<int>(D_FSTART, w), *fnobs = u.row<int>(D_FNOBS, w), *ffac0 = u.row<int>(D_FFAC0, w);
    int *psobs = u.dims.est_td ? u.row<int>(D_PSOBS, w) : nullptr, *fobs0 = u.dims.est_td ? u.row<int>(D_FOBS0, w) : nullptr;
    uint8_t *fconst = u.row<uint8_t>(D_FCONST, w);
    const unsigned long long nul = 1ULL << 17;
    // the flags and the feature maps first: a factor record carries its feature's row of W (bits 18 and up of the second flag word)
    for (int f = 0; f < F; f++) fconst[f] = in.feature_const[f] ? 1 : 0;
    int *fwrow = u.row<int>(D_FWROW, w);
    *u.row<int>(D_NROWS, w) = w_row_map(F, (int)u.dims.F, fconst, fwrow, u.row<int>(D_ROWFEAT, w));
    for (int g = 0; g < pl.nslot; g++) { double *rec = &facrec[(size_t)g * 8]; for (int k = 0; k < 7; k++) rec[k] = 0.0; std::memcpy(&rec[7], &nul, 8); psslot[g] = 0; if (psobs) psobs[g] = 0; }
    int q = 0;                                            // factor index in feature-major order
    for (int f = 0; f < F; f++) {
        const int o0 = in.feature_obs_offset[f], o1 = in.feature_obs_offset[f + 1], s = in.feature_start_frame[f], cst = in.feature_const[f] ? 1 : 0;
        feat[f] = in.para_feature[f]; fstart[f] = s; fnobs[f] = o1 - o0; ffac0[f] = q;
        if (fobs0) fobs0[f] = o0;
        const double *pi = in.obs_point + 3 * (size_t)o0;
        for (int t = o0 + 1; t < o1; t++, q++) {
            const int j = s + (t - o0), p = j * (j - 1) / 2 + s, pos = VB_SLOT(pl.cls[p], cur[p]);
            cur[p]++; psslot[pos] = q;
            if (psobs) psobs[pos] = t;
            double *rec = &facrec[(size_t)pos * 8]; const double *pj = in.obs_point + 3 * (size_t)t;
            for (int k = 0; k < 3; k++) { rec[k] = pi[k]; rec[3 + k] = pj[k]; }
            const unsigned long long a = (unsigned long long)(unsigned)f | ((unsigned long long)(unsigned)q << 32);
            const unsigned long long b2 = (unsigned long long)s | ((unsigned long long)j << 8) | ((unsigned long long)cst << 16) | (cst ? 0ULL : (unsigned long long)fwrow[f] << 18);
            std::memcpy(&rec[6], &a, 8); std::memcpy(&rec[7], &b2, 8);
        }
    }
    for (int k = 0; k < 10; k++) {
        const vilf_imu_preint &p = in.imu[k + 1];
        double *rec = u.row<double>(D_IMU, w) + (size_t)k * IMU_REC, *l = u.row<double>(D_LIDAR, w) + 7 * k;
        fill_imu_rec(p, rec);
        rec[287] = (p.sum_dt > 10.0) ? 0.0 : 1.0;                           // estimator.cpp:745
        std::memcpy(u.row<double>(D_COV, w) + 225 * k, p.covariance, 225 * 8);
        if (in.lidar) { const vilf_lidar_constraint &c = in.lidar[k + 1]; for (int i = 0; i < 4; i++) l[i] = c.q[i]; for (int i = 0; i < 3; i++) l[4 + i] = c.t[i]; }
        else for (int i = 0; i < 7; i++) l[i] = (i == 3) ? 1.0 : 0.0;
    }
}
// Stage 4: pack and copy. The per-window arrays of windows [w0, w1), every one a single copy (two where the same span also seeds the *_init copy) ...
int copy_windows(const Upload &u, int w0, int w1) {
    vilf_handle *h = u.h;
    for (const ArrayRow &r : kBatchArrays) {
        if (!r.by_range(u.dims)) continue;
        const size_t at = (size_t)w0 * u.ld[r.id], bytes = (size_t)(w1 - w0) * u.ld[r.id];
        const char *src = u.image + u.at[r.id] + at;
        HIPCHECK(h, hipMemcpyAsync(h->d[r.id].as<char>() + at, src, bytes, hipMemcpyHostToDevice, h->stream));
        if (r.twin >= 0) HIPCHECK(h, hipMemcpyAsync(h->d[r.twin].as<char>() + at, src, bytes, hipMemcpyHostToDevice, h->stream));
    }
    return VILF_OK;
}
// ... by one of three strategies. staged (a small batch): the whole host image in ONE copy, k_copy_spans hands its spans out to the arrays (see there). One pass: pack, a
// copy per array. Large batches: packing and copying overlap — the windows are packed in order by the host threads (an atomic cursor), and as soon as every window of a
// quarter of the batch is done the calling thread enqueues that quarter's slices, so the DMA engine works while the threads pack the next part (pack 5.1 ms + copy 6.6 ms one
// after the other before; eight parts: no better — 200 copy calls of the calling thread compete with the packers).
int pack_and_copy(const Upload &u, bool staged, Lap &lap) {
    vilf_handle *h = u.h;
    const int B = (int)u.dims.B;
    const int nchunk = (u.nthr > 1 && B >= 256) ? 4 : 1, csz = (B + nchunk - 1) / nchunk;
    std::atomic<int> next(0);
    std::vector<std::atomic<int>> done(nchunk); for (auto &d : done) d.store(0);
    auto packer = [&]() { for (int w = next.fetch_add(1); w < B; w = next.fetch_add(1)) { pack_window(u, w); done[w / csz].fetch_add(1, std::memory_order_release); } };
    std::vector<std::thread> pool;
    if (u.nthr <= 1) packer();
    else for (int t = 0; t < u.nthr; t++) pool.emplace_back(packer);
    int rc = VILF_OK;
    for (int c = 0; c < nchunk && !staged; c++) {
        const int w0 = c * csz, w1 = std::min(B, w0 + csz);
        while (done[c].load(std::memory_order_acquire) < w1 - w0) std::this_thread::yield();
        if (rc == VILF_OK) rc = copy_windows(u, w0, w1);
    }
    for (std::thread &th : pool) th.join();
    if (rc != VILF_OK) return rc;
    lap("pack + per-window copies");
    if (staged) {
        UpJobs jobs; jobs.n = 0; size_t big = 0;
        for (const ArrayRow &r : kBatchArrays) {
            if (!r.uploaded(u.dims)) continue;
            const size_t bytes = u.dims.B * u.ld[r.id];
            const char *src = h->d[D_UPSTAGE].as<char>() + u.at[r.id];
            jobs.j[jobs.n++] = UpJob{src, h->d[r.id].as<char>(), bytes};
            if (r.twin >= 0) jobs.j[jobs.n++] = UpJob{src, h->d[r.twin].as<char>(), bytes};
            big = std::max(big, bytes);
        }
        HIPCHECK(h, hipMemcpyAsync(h->d[D_UPSTAGE].p, u.image, u.image_bytes, hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(k_copy_spans, dim3((unsigned)std::max<size_t>(1, std::min<size_t>(64, big / 65536 + 1)), (unsigned)jobs.n), dim3(256), 0, h->stream, jobs);
        HIPCHECK(h, hipGetLastError());
    } else {
        // (from the pinned image, like everything else: an asynchronous upload must not read pageable memory the next call rewrites)
        for (const ArrayRow &r : kBatchArrays)
            if (r.use == A_SMALL) HIPCHECK(h, hipMemcpyAsync(h->d[r.id].p, u.image + u.at[r.id], u.dims.B * u.ld[r.id], hipMemcpyHostToDevice, h->stream));
        if (!h->async_upload) HIPCHECK(h, hipStreamSynchronize(h->stream));
    }
    lap("small arrays + sync");
    return VILF_OK;
}
// Stage 6, once per handle: the static scatter tables of the tile assembly (same for every window): source element -> LDS offset
int build_scatter_tables(vilf_handle *h) {
    auto perm = [](int a, int l) { return l < 6 ? 6 * a + l : 66 + 9 * a + (l - 6); };
    // packed entry: bits 0..14 = LDS offset + 1 (0: element not stored, upper block triangle), bits 15..22 = row, bits 23..30 = column
    auto off1 = [](int r, int c) { const int tr = r >> 4, tc = c >> 4; if (tr < tc) return 0; return (tr * (tr + 1) / 2 + tc) * 256 + 16 * (r & 15) + ((c & 15) ^ (r & 15)) + 1; };
    auto off = [&](int r, int c) { return off1(r, c) | (r << 15) | (c << 23); };
    std::vector<int> li(9000), ll(1440), lv(2 * 2376);
    for (int k = 0; k < 10; k++) {
        for (int e = 0; e < 900; e++) { const int p = e / 30, q = e % 30; li[900 * k + e] = off(perm(k + p / 15, p % 15), perm(k + q / 15, q % 15)); }
        for (int e = 0; e < 144; e++) { const int p = e / 12, q = e % 12; ll[144 * k + e] = off(perm(k + p / 6, p % 6), perm(k + q / 6, q % 6)); }
    }
    for (int t = 0; t < 2376; t++) {
        const int blk = t / 36, e = t % 36, l = e / 6, m = e % 6;
        int a = 0; while ((a + 1) * (a + 2) / 2 <= blk) a++;
        const int bb = blk - a * (a + 1) / 2, r = 6 * a + l, c = 6 * bb + m;
        lv[2 * t] = off(r, c);
        lv[2 * t + 1] = (a != bb && (r >> 4) == (c >> 4)) ? off1(c, r) : 0;
    }
    if (!h->d[D_LUTI].ensure(li.size() * 4) || !h->d[D_LUTL].ensure(ll.size() * 4) || !h->d[D_LUTV].ensure(lv.size() * 4)) return VILF_ERR_DEVICE;
    HIPCHECK(h, vilf_copy_sync(h, h->d[D_LUTI].p, li.data(), li.size() * 4, hipMemcpyHostToDevice));
    HIPCHECK(h, vilf_copy_sync(h, h->d[D_LUTL].p, ll.data(), ll.size() * 4, hipMemcpyHostToDevice));
    HIPCHECK(h, vilf_copy_sync(h, h->d[D_LUTV].p, lv.data(), lv.size() * 4, hipMemcpyHostToDevice));
    h->luts_ready = true;
    return VILF_OK;
}

}  // namespace

extern "C" int vilf_batch_upload(vilf_handle *h, int B, const vilf_window_in *wins) {
    if (!h || B <= 0 || !wins) return VILF_ERR_INVALID_ARGUMENT;
    Lap lap;
    HIPCHECK(h, hipSetDevice(h->device));
    if (h->upload_inflight) { HIPCHECK(h, hipStreamSynchronize(h->stream)); h->upload_inflight = false; }      // vilf_set_async_upload: the last upload's copies may still read the staging
    // the device-resident priors of slots 0..B-1 survive this call unless the slot range grows (buffers may be re-allocated)
    const bool keep_priors = h->resident && B <= h->prior_slots_valid;
    if (!keep_priors) { int rcp = pull_device_priors(h); if (rcp != VILF_OK) return rcp; }
    Upload u{};
    u.h = h; u.wins = wins; u.keep_inputs = h->opts.estimate_extrinsic || h->opts.estimate_td;
    u.nthr = B >= 64 ? (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency())) : 1;
    int rc = plan_windows(u, B);
    if (rc != VILF_OK) return rc;
    h->B = B; h->resident = false;
    if ((int)h->priors.size() < B) { vilf_prior z; std::memset(&z, 0, sizeof(z)); h->priors.resize(B, z); }
    if (!keep_priors) { h->prior_dirty.assign(h->priors.size(), 1); h->prior_dev_newer.assign(h->priors.size(), 0); h->prior_slots_valid = 0; }
    h->prior_dirty.resize(h->priors.size(), 1); h->prior_dev_newer.resize(h->priors.size(), 0);
    if ((rc = reserve(u, lap)) != VILF_OK) return rc;
    // a small batch takes the staged copy: one copy of the whole host image + k_copy_spans
    const bool staged = u.nthr <= 1 && u.image_bytes <= ((size_t)64 << 20) && !std::getenv("VILF_NO_STAGED_UPLOAD") && h->d[D_UPSTAGE].ensure(u.image_bytes + 4096);
    if ((rc = pack_and_copy(u, staged, lap)) != VILF_OK) return rc;
    bind_batch_arrays(h, u.dims);
    if (getenv("VILF_DEBUG_STAMPS")) { if (!h->d[D_DBG].ensure(3 * 32 * 8)) return VILF_ERR_DEVICE; hipMemsetAsync(h->d[D_DBG].p, 0, 3 * 32 * 8, h->stream); h->batch.dbg = h->d[D_DBG].as<long long>(); }
    HIPCHECK(h, hipMemsetAsync(h->d[D_W].p, 0, batch_array_bytes(D_W, u.dims), h->stream));   // W rows are zero outside the rewritten ranges
    if (!h->luts_ready && (rc = build_scatter_tables(h)) != VILF_OK) return rc;
    h->batch.lut_imu = h->d[D_LUTI].as<int>(); h->batch.lut_lid = h->d[D_LUTL].as<int>(); h->batch.lut_vis = h->d[D_LUTV].as<int>();
    const int nimu = B * 10;
    hipLaunchKernelGGL(k_imu_prep, dim3((nimu + 3) / 4), dim3(IMU_PREP_NT), 0, h->stream, nimu, h->d[D_COV].as<double>(), h->d[D_WORK].as<double>(), h->d[D_IMU].as<double>());
    HIPCHECK(h, hipGetLastError());
    if ((rc = upload_priors(h)) != VILF_OK) return rc;
    hipLaunchKernelGGL(k_reset, dim3(B), dim3(VB_NT), 0, h->stream, h->batch, 0);
    HIPCHECK(h, hipGetLastError());
    if (h->async_upload || (h->defer_upload_sync && staged)) h->upload_inflight = true;          // the next upload of this handle waits before it touches the staging (also when
                                                                                                 // vilf_window_solve returns early on an error, before its own wait for the stream)
    else HIPCHECK(h, hipStreamSynchronize(h->stream));
    h->resident = true;
    return VILF_OK;
}

// the row map of W as the upload builds it (w_row_map), for a window of F features with the given constant flags: f_wrow[F], row_feat[cap], returns n_rows. A test
// hook (no handle, no device); not part of include/vilfusion.h.
extern "C" int vilf_debug_w_row_map(int F, int cap, const unsigned char *feature_const, int *f_wrow, int *row_feat) {
    if (F < 0 || cap < ((F + 3) & ~3) || !f_wrow || !row_feat || (F && !feature_const)) return VILF_ERR_INVALID_ARGUMENT;
    return w_row_map(F, cap, feature_const, f_wrow, row_feat);
}
// the class plan of a window's visual factors as the upload makes it (class_plan), from the two track tables alone: per frame pair its class, its start inside the
// class list and its factor count; returns the window's factor slots (whole chunks of VB_CHUNK). The tracks must satisfy check_window's rule. A test hook (no handle,
// no device); not part of include/vilfusion.h.
extern "C" int vilf_debug_class_plan(int n_features, const int *feature_start_frame, const int *feature_obs_offset, int *cls, int *cstart, int *ccount) {
    if (n_features < 0 || n_features > VILF_MAX_FEATURES || !cls || !cstart || !ccount || (n_features && (!feature_start_frame || !feature_obs_offset))) return VILF_ERR_INVALID_ARGUMENT;
    for (int f = 0; f < n_features; f++) {
        const int s = feature_start_frame[f], n = feature_obs_offset[f + 1] - feature_obs_offset[f];
        if (s < 0 || n < 2 || s + n > VB_NF) return VILF_ERR_INVALID_ARGUMENT;
    }
    vilf_window_in in{};
    in.n_features = n_features; in.feature_start_frame = feature_start_frame; in.feature_obs_offset = feature_obs_offset;
    return class_plan(in, cls, cstart, ccount);
}
// the library's radix sort (vilf_sort.hip) through host buffers — a test hook (tests/test_scan2map.py compares it with a stable host sort); not part of include/vilfusion.h.
// keys: n values of 4 (key64 == 0) or 8 bytes; the low `bits` bits are sorted, equal keys keep their order.
extern "C" int vilf_debug_sort_pairs(vilf_handle *h, const void *keys, const int *vals, size_t n, int bits, int key64, void *keys_out, int *vals_out) {
    if (!h || !keys || !vals || !keys_out || !vals_out || n == 0) return VILF_ERR_INVALID_ARGUMENT;
    const size_t kb = key64 ? 8 : 4, tb = vilf_sort_temp_bytes(n, kb);
    void *dk = nullptr, *dk2 = nullptr, *dv = nullptr, *dv2 = nullptr, *dt = nullptr;
    int rc = VILF_OK;
    if (hipMalloc(&dk, n * kb) != hipSuccess || hipMalloc(&dk2, n * kb) != hipSuccess || hipMalloc(&dv, n * 4) != hipSuccess || hipMalloc(&dv2, n * 4) != hipSuccess || hipMalloc(&dt, tb) != hipSuccess) rc = VILF_ERR_DEVICE;
    if (rc == VILF_OK && (hipMemcpyAsync(dk, keys, n * kb, hipMemcpyHostToDevice, h->stream) != hipSuccess || hipMemcpyAsync(dv, vals, n * 4, hipMemcpyHostToDevice, h->stream) != hipSuccess)) rc = VILF_ERR_DEVICE;
    if (rc == VILF_OK) {
        const int r = key64 ? vilf_sort_pairs_u64(h->stream, dt, tb, (const unsigned long long *)dk, (unsigned long long *)dk2, (const int *)dv, (int *)dv2, n, bits)
                            : vilf_sort_pairs_u32(h->stream, dt, tb, (const unsigned *)dk, (unsigned *)dk2, (const int *)dv, (int *)dv2, n, bits);
        if (r != 0) rc = VILF_ERR_DEVICE;
    }
    if (rc == VILF_OK && (hipMemcpyAsync(keys_out, dk2, n * kb, hipMemcpyDeviceToHost, h->stream) != hipSuccess || hipMemcpyAsync(vals_out, dv2, n * 4, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
                          hipStreamSynchronize(h->stream) != hipSuccess)) rc = VILF_ERR_DEVICE;
    hipFree(dk); hipFree(dk2); hipFree(dv); hipFree(dv2); hipFree(dt);
    return rc;
}
// k_imu_prep for n covariances through host buffers, launched as vilf_batch_upload launches it (four factors of 16 lanes per block) — a test hook (tests/test_imu_exact.py
// compares every lane group and the tail with an exact sqrt_info); not part of include/vilfusion.h. cov: [n][225] row-major in, out: [n][225] = the IMU_SQRT block of each record.
extern "C" int vilf_debug_imu_sqrt_info(vilf_handle *h, int n, const double *cov, double *out) {
    if (!h || n <= 0 || !cov || !out) return VILF_ERR_INVALID_ARGUMENT;
    HIPCHECK(h, hipSetDevice(h->device));
    const size_t sn = (size_t)n;
    double *d_cov = nullptr, *d_rec = nullptr;
    int rc = VILF_OK;
    if (hipMalloc(&d_cov, sn * 225 * 8) != hipSuccess || hipMalloc(&d_rec, sn * IMU_REC * 8) != hipSuccess) rc = VILF_ERR_DEVICE;
    if (rc == VILF_OK && (hipMemcpyAsync(d_cov, cov, sn * 225 * 8, hipMemcpyHostToDevice, h->stream) != hipSuccess || hipMemsetAsync(d_rec, 0, sn * IMU_REC * 8, h->stream) != hipSuccess)) rc = VILF_ERR_DEVICE;
    if (rc == VILF_OK) {
        hipLaunchKernelGGL(k_imu_prep, dim3((unsigned)((n + 3) / 4)), dim3(IMU_PREP_NT), 0, h->stream, n, d_cov, (double *)nullptr, d_rec);
        if (hipGetLastError() != hipSuccess) rc = VILF_ERR_DEVICE;
    }
    std::vector<double> rec(sn * IMU_REC);
    if (rc == VILF_OK && (hipMemcpyAsync(rec.data(), d_rec, sn * IMU_REC * 8, hipMemcpyDeviceToHost, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess)) rc = VILF_ERR_DEVICE;
    if (rc == VILF_OK) for (size_t i = 0; i < sn; i++) std::memcpy(out + i * 225, &rec[i * IMU_REC + IMU_SQRT], 225 * 8);
    hipFree(d_cov); hipFree(d_rec);
    return rc;
}
// dynamic LDS the window kernels are launched with (bytes): [0] k_linearize / k_linearize_split / k_linearize_last, [1] k_solve_sb; [2], the larger of the two, is
// kept for callers that read three values. Diagnostic (bench.py quotes them beside the registers it reads from the code objects); not part of include/vilfusion.h.
extern "C" int vilf_debug_lds_bytes(vilf_handle *h, int out3[3]) {
    if (!h || !out3) return VILF_ERR_INVALID_ARGUMENT;
    out3[0] = VB_LIN_LDS_BYTES; out3[1] = SB_LDS_BYTES; out3[2] = std::max(VB_LIN_LDS_BYTES, SB_LDS_BYTES);
    return VILF_OK;
}
extern "C" int vilf_debug_stamps(vilf_handle *h, long long *out96) {
    if (!h || !h->batch.dbg) return VILF_ERR_INVALID_ARGUMENT;
    HIPCHECK(h, vilf_copy_sync(h, out96, h->batch.dbg, 96 * 8, hipMemcpyDeviceToHost));
    return VILF_OK;
}

extern "C" int vilf_batch_rewind(vilf_handle *h) {
    if (!h || !h->resident) return VILF_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(k_reset, dim3(h->B), dim3(VB_NT), 0, h->stream, h->batch, 1);
    HIPCHECK(h, hipGetLastError());
    if ((h->opts.estimate_extrinsic || h->opts.estimate_td) && (int)h->own.size() == h->B) {      // Ex_Pose / td are variables then: their uploaded values are part of the state
        for (int w = 0; w < h->B; w++) { std::memcpy(&h->h_ex[(size_t)w * VB_EX_LD], h->own[w].in.para_ex_pose, VB_EX_LD * 8); h->h_td[w] = h->own[w].in.para_td; }
        HIPCHECK(h, hipMemcpyAsync(h->d[D_EX].p, h->h_ex.data(), (size_t)h->B * VB_EX_LD * 8, hipMemcpyHostToDevice, h->stream));
        HIPCHECK(h, hipMemcpyAsync(h->d[D_TD].p, h->h_td.data(), (size_t)h->B * 8, hipMemcpyHostToDevice, h->stream));
    }
    if (h->prior_restore_needed && h->prior_backup_valid) {          // a marginalization replaced the priors: the set as uploaded becomes the live one again (swap, no copy)
        swap_prior_sets(h);
        // the device now holds the authoritative priors; the host mirror may have seen the marginalized ones through an export
        for (int w = 0; w < h->B; w++) { h->prior_dev_newer[w] = 1; h->prior_dirty[w] = 0; }
        // (the restored set is the uploaded one: prior_dense / solve_dense_fallback describe exactly it)
        h->prior_restore_needed = false;
    }
    return VILF_OK;
}

// usec_solve of an asynchronous solve: its two events are read once the stream has been waited for (summaries / download_states)
static void solve_time_resolve(vilf_handle *h) {
    if (!h->solve_time_pending) return;
    float ms = 0;
    if (hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess) h->last_solve_usec = ms * 1000.0;
    h->solve_time_pending = false;
}
extern "C" int vilf_batch_solve(vilf_handle *h, int sync) {
    if (!h || !h->resident) return VILF_ERR_INVALID_ARGUMENT;
    HIPCHECK(h, hipSetDevice(h->device));
    if (h->opts.estimate_extrinsic || h->opts.estimate_td) {
        // Ex_Pose / td as variables (estimator.cpp:701-717; both off in the KITTI configuration): every slot through the general single-window path
        // (vilf_lw.hip: ProjectionTdFactor / Ex_Pose Jacobians, the slot's device-resident prior), one after the other. State, gauge-fixed outputs and the
        // summary are written back to the slot, so download / summaries / marginalization continue as after the batched kernels.
        if ((int)h->own.size() != h->B) { h->err = "batch inputs not retained"; return VILF_ERR_INVALID_ARGUMENT; }
        { int rc = upload_priors(h); if (rc != VILF_OK) return rc; }      // (the slots whose host mirror changed; nothing otherwise)
        const auto t0 = std::chrono::steady_clock::now();
        // all slots as ONE group: a single chain of launches solves them side by side (vilf_lw_group_solve), priors in and states / summaries back in bulk copies
        const size_t B = h->B;
        std::vector<double> bufP(B * VB_POSE_LD), bufS(B * VB_SB_LD), bufF(B * (h->batch.Fmax + 4)), Ps(B * VB_OUT3_LD), Rs(B * VB_OUTR_LD), Vs(B * VB_OUT3_LD), Bas(B * VB_OUT3_LD), Bgs(B * VB_OUT3_LD);
        std::vector<vilf_window_out> outv(B);
        std::vector<const vilf_window_in *> inp(B);
        std::vector<vilf_window_out *> outp(B);
        std::vector<int> slot1(B);
        for (size_t w = 0; w < B; w++) {
            vilf_window_out &out = outv[w];
            std::memset(&out, 0, sizeof(out));
            out.para_pose = &bufP[w * VB_POSE_LD]; out.para_speed_bias = &bufS[w * VB_SB_LD]; out.para_feature = &bufF[w * (h->batch.Fmax + 4)];
            out.Ps = &Ps[w * VB_OUT3_LD]; out.Rs = &Rs[w * VB_OUTR_LD]; out.Vs = &Vs[w * VB_OUT3_LD]; out.Bas = &Bas[w * VB_OUT3_LD]; out.Bgs = &Bgs[w * VB_OUT3_LD];
            inp[w] = &h->own[w].in; outp[w] = &out; slot1[w] = (int)w + 1;
        }
        const int rc = vilf_lw_group_solve(h, h->B, inp.data(), outp.data(), slot1.data());
        if (rc < 0) return rc;
        h->last_solve_usec = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        h->solve_time_pending = false;
        (void)sync;                             // the general path reads its results back: always synchronous
        return VILF_OK;
    }
    { int rc = upload_priors(h); if (rc != VILF_OK) return rc; }          // (the slots whose host mirror changed; nothing otherwise)
    const dim3 grid(h->B), block(VB_NT);
    // k_solve_sb eliminates SpeedBias[1..10] as a block-tridiagonal chain: valid while the priors hold no speed-bias block but SpeedBias[0] (all the
    // reference ever produces, estimator.cpp:960-971); VILF_SOLVE_DENSE=1 forces the dense-Cholesky kernel (tests compare the two)
    // (solve_dense_fallback describes the priors as uploaded; after a device marginalization the live priors hold SpeedBias[0] only — prior_restore_needed — until a rewind)
    const bool dense = (h->solve_dense_fallback && !h->prior_restore_needed) || std::getenv("VILF_SOLVE_DENSE") != nullptr;
    const bool prof = h->profiling != 0;
    if (prof && h->prof_used.size() > 4096) { const int rcf = vilf_prof_flush(h); if (rcf != VILF_OK) return rcf; }      // asynchronous calls without a reader: bound the pool
    std::vector<int> kinds;
    int ne = 0;
    std::vector<hipEvent_t> pev;
    auto mark = [&](int kind) { if (prof) { pev.push_back(vilf_prof_event(h)); ne++; kinds.push_back(kind); } };
    hipEventRecord(h->ev0, h->stream);
    h->batch.w0 = 0;
    // live-window lists (vilf_batch.hpp): the launches of iteration i address their windows through the list k_linearize of iteration i - 1 left, once something has stopped
    const int max_it = h->opts.max_num_iterations;
    const bool use_live = !std::getenv("VILF_NO_LIVE_LIST") && max_it + 2 <= 64 && h->d[D_LIVE].ensure(((size_t)2 * h->B + 128) * sizeof(int));
    // small batches: every window's linearisation over several workgroups (k_linearize_split: one per factor chunk + two for the IMU / LiDAR / prior parts)
    const int nch = h->batch.FACmax / VB_CHUNK;
    const bool split = !dense && h->B <= VB_SPLIT_MAXB && nch >= 1 && nch <= VB_SPLIT_MAXCH && !std::getenv("VILF_NO_LIN_SPLIT") &&
                       h->d[D_SPLITC].ensure((size_t)h->B * VB_SPLIT_CTL * sizeof(int)) && h->d[D_SPLITB].ensure((size_t)h->B * VB_SPLIT_DBL * sizeof(double));
    if (split) HIPCHECK(h, hipMemsetAsync(h->d[D_SPLITC].p, 0, (size_t)h->B * VB_SPLIT_CTL * sizeof(int), h->stream));
    auto with_lists = [&](int it) {
        VbBatch bb = h->batch;
        if (use_live && !split) { bb.live_ctl = h->d[D_LIVE].as<int>(); bb.live_buf = bb.live_ctl + 128; bb.live_it = it; }
        return bb;
    };
    auto linearize = [&](const VbBatch &bb0, int iteration_zero) {
        if (split) {
            VbBatch bb = bb0;
            bb.split_nr = nch + 2; bb.split_ctl = h->d[D_SPLITC].as<int>(); bb.split_buf = h->d[D_SPLITB].as<double>();
            if (++h->split_gen <= 0) h->split_gen = 1;            // the launch's generation: what its hand-over flags carry (never 0 = the cleared state)
            bb.split_gen = h->split_gen;
            bb.split_fault = std::getenv("VILF_SPLIT_FAULT") != nullptr;
            hipLaunchKernelGGL(k_linearize_split, dim3((unsigned)(h->B * (nch + 2))), block, VB_LIN_LDS_BYTES, h->stream, bb, iteration_zero);
        } else hipLaunchKernelGGL(k_linearize, grid, block, VB_LIN_LDS_BYTES, h->stream, bb0, iteration_zero);
    };
    mark(3);
    hipLaunchKernelGGL(k_reset, grid, block, 0, h->stream, with_lists(0), 0);
    mark(0);
    linearize(h->batch, 1);
    // options.max_solver_time (estimator.cpp:847-850: SOLVER_TIME, x 4/5 when the oldest frame is marginalized): Ceres tests the wall clock at the top of
    // every iteration. The iterations of a batch run in lockstep, so the host waits for the stream before each one (only when the limit is on) and
    // stops the windows whose limit has passed (termination NO_CONVERGENCE, like Ceres' "maximum solver time reached").
    const double tlim = h->opts.max_solver_time;
    const auto t_begin = std::chrono::steady_clock::now();
    bool stopped_old = false;
    for (int it = 0; it < h->opts.max_num_iterations; it++) {
        if (tlim > 0) {
            HIPCHECK(h, hipStreamSynchronize(h->stream));
            const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
            if (el >= tlim) { hipLaunchKernelGGL(k_time_limit, grid, dim3(WIN1_NT), 0, h->stream, h->batch, h->d[D_MFLAG].as<int>(), 0); break; }
            if (el >= tlim * 4.0 / 5.0 && !stopped_old) { hipLaunchKernelGGL(k_time_limit, grid, dim3(WIN1_NT), 0, h->stream, h->batch, h->d[D_MFLAG].as<int>(), 1); stopped_old = true; }
        }
        mark(1);
        const bool last = it + 1 == h->opts.max_num_iterations;
        const VbBatch bs = with_lists(it + 1), bl = bs;
        if (dense) hipLaunchKernelGGL(k_solve, grid, dim3(SNT), SOLVE_LDS_BYTES, h->stream, bs);
        else hipLaunchKernelGGL(k_solve_sb, grid, dim3(SBT), SB_LDS_BYTES, h->stream, bs);
        mark(last ? 2 : 0);      // kind 2 ("k_step" in the bench line): the step-only launch that ends a solve
        // the step of the last iteration needs no linearisation behind it (nothing solves with it): residuals only
        if (last) hipLaunchKernelGGL(k_linearize_last, grid, block, VB_LIN_LDS_BYTES, h->stream, bl);
        else linearize(bl, 0);
    }
    mark(3);
    hipLaunchKernelGGL(k_finalize, grid, dim3(WIN1_NT), 0, h->stream, h->batch);
    if (prof) {
        pev.push_back(vilf_prof_event(h)); ne++;
        for (size_t i = 0; i < kinds.size(); i++) vilf_prof_span(h, pev[i], pev[i + 1], &h->kernel_prof.ms[kinds[i]], &h->kernel_prof.launches[kinds[i]]);
    }
    hipEventRecord(h->ev1, h->stream);
    HIPCHECK(h, hipGetLastError());
    h->solve_time_pending = true;
    if (sync) {
        HIPCHECK(h, hipStreamSynchronize(h->stream));
        solve_time_resolve(h);
        if (prof) { const int rcf = vilf_prof_flush(h); if (rcf != VILF_OK) return rcf; }
    }                                           // sync == 0 with profiling on: the spans stay pending (read by the next call that waits for the stream)
    return VILF_OK;
}

// per-kernel timing with HIP events on the handle's stream (bench.py roofline). kind: 0 linearize, 1 solve, 2 step, 3 other
extern "C" int vilf_set_profiling(vilf_handle *h, int on) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    { const int rcf = vilf_prof_flush(h); if (rcf != VILF_OK) return rcf; }
    // hipEventCreate is slow enough to starve the stream when it happens between launches (measured: 1.9 ms per frame for ~50 events): the pool is filled here
    if (on) { HIPCHECK(h, hipSetDevice(h->device)); while (h->prof_free.size() < 1024) { hipEvent_t e; HIPCHECK(h, hipEventCreate(&e)); h->prof_free.push_back(e); } }
    h->profiling = on;
    h->kernel_prof.reset(); h->s2m_prof.reset(); h->marg_prof.reset();
    for (VilfStage *s : h->stage) if (s) s->profile_reset();
    return VILF_OK;
}
extern "C" int vilf_get_profile(vilf_handle *h, double ms_out[4], long launches_out[4]) { return vilf_handle_profile(h, &vilf_handle::kernel_prof, ms_out, launches_out); }

extern "C" int vilf_get_profile_marginalize(vilf_handle *h, double ms_out[4], long launches_out[4]) { return vilf_handle_profile(h, &vilf_handle::marg_prof, ms_out, launches_out); }

// a window whose kernel gave up a bounded device-side wait (VbState::dev_error): no numbers are handed out for it
static int vb_check_dev_error(vilf_handle *h, const VbState *st, int first, int n) {
    for (int i = 0; i < n; i++) if (st[i].dev_error) {
        h->err = "window " + std::to_string(first + i) + ": a workgroup of k_linearize_split gave up waiting for another one's hand-over (bounded wait; the results of this solve are not valid)";
        return VILF_ERR_DEVICE;
    }
    return VILF_OK;
}
static vilf_summary summary_of(const VbState &s, double usec_solve) {
    vilf_summary m;
    m.num_iterations = s.iteration; m.num_successful_steps = s.num_successful; m.num_linear_solves = s.num_linear_solves; m.termination = s.termination;
    m.initial_cost = s.initial_cost; m.final_cost = s.x_cost; m.final_radius = s.radius; m.usec_solve = usec_solve;
    return m;
}
extern "C" int vilf_batch_summaries(vilf_handle *h, int first, int n, vilf_summary *sums) {
    if (!h || !h->resident || first < 0 || n < 0 || first + n > h->B || !sums) return VILF_ERR_INVALID_ARGUMENT;
    std::vector<VbState> st(n);
    HIPCHECK(h, hipMemcpyAsync(st.data(), h->batch.st + first, sizeof(VbState) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(h, hipStreamSynchronize(h->stream));
    solve_time_resolve(h);
    { const int rcf = vilf_prof_flush(h); if (rcf != VILF_OK) return rcf; }     // the stream is idle: pending profile spans cost nothing to read now
    { const int rce = vb_check_dev_error(h, st.data(), first, n); if (rce != VILF_OK) return rce; }
    for (int i = 0; i < n; i++) sums[i] = summary_of(st[i], h->last_solve_usec);
    return VILF_OK;
}

// the eight result rows of a window in the order of vilf_window_out's pointers (para_pose, para_speed_bias, para_feature, Ps, Rs, Vs, Bas, Bgs): device array, doubles per window
struct ResultRow { const double *dev; size_t ld; };
static void result_rows(const vilf_handle *h, ResultRow rows[8]) {
    const VbBatch &b = h->batch;
    const ResultRow r[8] = {{b.pose, VB_POSE_LD}, {b.sb, VB_SB_LD}, {b.feat, (size_t)b.Fmax}, {b.out_Ps, VB_OUT3_LD}, {b.out_Rs, VB_OUTR_LD}, {b.out_Vs, VB_OUT3_LD}, {b.out_Bas, VB_OUT3_LD}, {b.out_Bgs, VB_OUT3_LD}};
    std::copy(r, r + 8, rows);
}
// window w's output from host copies of its eight rows, the host mirrors of Ex_Pose / td (kept current by the general path with estimate_extrinsic / estimate_td) and its summary
static void fill_window_out(const vilf_handle *h, int w, const ResultRow rows[8], const double *const host[8], const vilf_summary &sum, vilf_window_out &o) {
    double *const dst[8] = {o.para_pose, o.para_speed_bias, o.para_feature, o.Ps, o.Rs, o.Vs, o.Bas, o.Bgs};
    for (int k = 0; k < 8; k++) {
        const size_t cnt = k == 2 ? (size_t)h->h_nfeat[w] : rows[k].ld;
        if (dst[k] && cnt) std::memcpy(dst[k], host[k], cnt * 8);
    }
    const double *exw = &h->h_ex[(size_t)w * VB_EX_LD];
    for (int k = 0; k < 3; k++) o.tic[k] = exw[k];
    quat_to_R(exw + 3, o.ric);
    o.td = h->h_td[w];
    o.summary = sum;
}

extern "C" int vilf_batch_download(vilf_handle *h, int first, int n, vilf_window_out *outs) {
    if (!h || !h->resident || first < 0 || n < 0 || first + n > h->B || !outs) return VILF_ERR_INVALID_ARGUMENT;
    ResultRow rows[8]; result_rows(h, rows);
    size_t per = 0; const size_t sn = n;
    for (const ResultRow &r : rows) per += r.ld;
    const double *host[8];                    // host copy of every row, windows first .. first + n - 1
    std::vector<double> pageable;
    std::vector<vilf_summary> sums(n);
    // a few windows (the single-window entry point): the nine result arrays are gathered on the device (k_copy_spans) and come back in ONE copy through pinned memory
    const size_t img0 = ((sn * per * 8 + 63) & ~(size_t)63) + sn * sizeof(VbState);
    if (n <= 64 && !std::getenv("VILF_NO_STAGED_UPLOAD") && h->d[D_DNSTAGE].ensure(img0 + 256) && h->pin_down.ensure(img0 + 256)) {
        UpJobs jobs; jobs.n = 0;
        char *dst = h->d[D_DNSTAGE].as<char>();
        size_t off = 0;
        auto gather = [&](const void *src, size_t bytes) { jobs.j[jobs.n++] = UpJob{static_cast<const char *>(src), dst + off, bytes}; const size_t at = off; off += (bytes + 15) & ~(size_t)15; return at; };
        const char *img = static_cast<const char *>(h->pin_down.p);
        for (int k = 0; k < 8; k++) host[k] = reinterpret_cast<const double *>(img + gather(rows[k].dev + (size_t)first * rows[k].ld, sn * rows[k].ld * 8));
        const VbState *st = reinterpret_cast<const VbState *>(img + gather(h->batch.st + first, sn * sizeof(VbState)));
        hipLaunchKernelGGL(k_copy_spans, dim3(1, (unsigned)jobs.n), dim3(256), 0, h->stream, jobs);
        HIPCHECK(h, hipGetLastError());
        HIPCHECK(h, hipMemcpyAsync(h->pin_down.p, dst, off, hipMemcpyDeviceToHost, h->stream));
        HIPCHECK(h, hipStreamSynchronize(h->stream));
        solve_time_resolve(h);
        { const int rcf = vilf_prof_flush(h); if (rcf != VILF_OK) return rcf; }
        { const int rce = vb_check_dev_error(h, st, first, n); if (rce != VILF_OK) return rce; }
        for (int i = 0; i < n; i++) sums[i] = summary_of(st[i], h->last_solve_usec);
    } else {
        pageable.resize(sn * per);
        size_t off = 0;
        for (int k = 0; k < 8; k++) {
            host[k] = pageable.data() + off;
            HIPCHECK(h, hipMemcpyAsync(pageable.data() + off, rows[k].dev + (size_t)first * rows[k].ld, sn * rows[k].ld * 8, hipMemcpyDeviceToHost, h->stream));
            off += sn * rows[k].ld;
        }
        const int rc = vilf_batch_summaries(h, first, n, sums.data());   // synchronises the stream
        if (rc != VILF_OK) return rc;
    }
    for (int i = 0; i < n; i++) {
        const double *mine[8];
        for (int k = 0; k < 8; k++) mine[k] = host[k] + (size_t)i * rows[k].ld;
        fill_window_out(h, first + i, rows, mine, sums[i], outs[i]);
    }
    return VILF_OK;
}

// The estimator's outputs only (double2vector(): Ps / Rs / Vs / Bas / Bgs, estimator.cpp:549-638) plus the summaries, into caller-owned contiguous arrays
// [n][33] / [n][99] / ...: five device-to-host copies through pinned staging and one wait — what a per-frame caller needs back; the parameter arrays
// (para_Pose, para_Feature ...) stay on the device for the marginalization. Any pointer may be NULL.
extern "C" int vilf_batch_download_states(vilf_handle *h, int first, int n, double *Ps, double *Rs, double *Vs, double *Bas, double *Bgs, vilf_summary *sums) {
    if (!h || !h->resident || first < 0 || n < 0 || first + n > h->B) return VILF_ERR_INVALID_ARGUMENT;
    if (n == 0) return VILF_OK;
    ResultRow all[8];
    result_rows(h, all);
    const ResultRow *rows = all + 3;          // out_Ps ... out_Bgs
    double *const dst[5] = {Ps, Rs, Vs, Bas, Bgs};
    const size_t sn = n;
    size_t per = 0;
    for (int k = 0; k < 5; k++) per += rows[k].ld;
    if (!h->pin_down.ensure(sn * per * 8 + sn * sizeof(VbState) + 256)) { h->err = "hipHostMalloc failed (download staging)"; return VILF_ERR_DEVICE; }
    double *pin[5], *end = static_cast<double *>(h->pin_down.p);
    for (int k = 0; k < 5; k++) { pin[k] = end; end += sn * rows[k].ld; }
    VbState *pS = reinterpret_cast<VbState *>(end);
    for (int k = 0; k < 5; k++) if (dst[k]) HIPCHECK(h, hipMemcpyAsync(pin[k], rows[k].dev + (size_t)first * rows[k].ld, sn * rows[k].ld * 8, hipMemcpyDeviceToHost, h->stream));
    if (sums) HIPCHECK(h, hipMemcpyAsync(pS, h->batch.st + first, sn * sizeof(VbState), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(h, hipStreamSynchronize(h->stream));
    solve_time_resolve(h);
    for (int k = 0; k < 5; k++) if (dst[k]) std::memcpy(dst[k], pin[k], sn * rows[k].ld * 8);
    if (sums) { const int rce = vb_check_dev_error(h, pS, first, n); if (rce != VILF_OK) return rce; }
    if (sums) for (int i = 0; i < n; i++) sums[i] = summary_of(pS[i], h->last_solve_usec);
    return VILF_OK;
}

// n independent windows of sizes other than the reference's WINDOW_SIZE + 1 = 11 frames, solved side by side in one chain of launches (vilf_lw.hip). 11-frame
// windows belong to the vilf_batch_* entry points (LDS kernels, priors, marginalization).
extern "C" int vilf_window_solve_group(vilf_handle *h, int n, const vilf_window_in *in, vilf_window_out *out) {
    if (!h || n < 1 || !in || !out) return VILF_ERR_INVALID_ARGUMENT;
    std::vector<const vilf_window_in *> inp(n);
    std::vector<vilf_window_out *> outp(n);
    for (int i = 0; i < n; i++) {
        if (in[i].n_frames == VB_NF) { h->err = "vilf_window_solve_group: 11-frame windows go through vilf_batch_upload / vilf_batch_solve"; return VILF_ERR_UNSUPPORTED; }
        if (!out[i].Ps || !out[i].Rs || !out[i].Vs || !out[i].Bas || !out[i].Bgs) return VILF_ERR_INVALID_ARGUMENT;
        inp[i] = &in[i]; outp[i] = &out[i];
    }
    return vilf_lw_group_solve(h, n, inp.data(), outp.data(), nullptr);
}
extern "C" int vilf_window_solve(vilf_handle *h, const vilf_window_in *in, vilf_window_out *out) {
    if (!h || !in || !out) return VILF_ERR_INVALID_ARGUMENT;
    if (in->n_frames != VB_NF) {          // not the reference's WINDOW_SIZE = 10: the general path (one window spread over the device, no prior)
        if (in->n_frames != h->opts.window_size + 1) { h->err = "n_frames must be options.window_size + 1"; return VILF_ERR_INVALID_ARGUMENT; }
        return vilf_lw_window_solve(h, in, out, 0);
    }
    auto t0 = std::chrono::steady_clock::now();
    h->defer_upload_sync = true;
    int rc = vilf_batch_upload(h, 1, in);
    h->defer_upload_sync = false;
    if (rc != VILF_OK) return rc;
    if (h->opts.estimate_extrinsic || h->opts.estimate_td)      // Ex_Pose / td as variables (estimator.cpp:701-717): the general single-window path, with the slot-0 prior
        return vilf_lw_window_solve(h, in, out, 1);      // slot 0
    rc = vilf_batch_solve(h, 1);
    if (rc != VILF_OK) return rc;
    rc = vilf_batch_download(h, 0, 1, out);
    if (rc != VILF_OK) return rc;
    out->summary.usec_solve = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    return (out->summary.termination == VILF_TERM_FAILURE) ? VILF_SOLVER_ABNORMAL : VILF_OK;
}

// block table of a prior whose n and n_blocks are in range: global sizes 7 (pose), 9 (speed-bias) or 1 (td), local columns inside [0, n) — the kernels index
// LDS vectors with it
static bool prior_block_table_ok(const vilf_prior *prior) {
    for (int i = 0; i < prior->n_blocks; i++) {
        const int gs = prior->block_size[i], ls = gs == 7 ? 6 : gs, idx = prior->block_idx[i];
        if ((gs != 7 && gs != 9 && gs != 1) || prior->block_id[i] < 0 || idx < 0 || idx + ls > prior->n) return false;
    }
    return true;
}

extern "C" int vilf_prior_import(vilf_handle *h, int slot, const vilf_prior *prior) {
    if (!h || slot < 0 || !prior) return VILF_ERR_INVALID_ARGUMENT;
    if (prior->valid && (prior->n <= 0 || prior->n > VILF_PRIOR_MAX_DIM || prior->n_blocks <= 0 || prior->n_blocks > VILF_PRIOR_MAX_BLOCKS)) return VILF_ERR_INVALID_ARGUMENT;
    if (prior->valid && !prior_block_table_ok(prior)) { h->err = "prior block table out of range"; return VILF_ERR_INVALID_ARGUMENT; }
    if ((int)h->priors.size() <= slot) { vilf_prior z; std::memset(&z, 0, sizeof(z)); h->priors.resize(slot + 1, z); h->prior_dirty.resize(slot + 1, 1); }
    h->priors[slot] = *prior;
    h->prior_dirty[slot] = 1;
    if ((int)h->prior_dev_newer.size() <= slot) h->prior_dev_newer.resize(slot + 1, 0);
    h->prior_dev_newer[slot] = 0;
    return VILF_OK;
}

extern "C" int vilf_prior_export(vilf_handle *h, int slot, vilf_prior *out) {
    if (!h || slot < 0 || slot >= (int)h->priors.size() || !out) return VILF_ERR_INVALID_ARGUMENT;
    { int rcp = pull_device_priors(h); if (rcp != VILF_OK) return rcp; }
    *out = h->priors[slot];
    return VILF_OK;
}

// The marginalization workspace: every array's size and its VbMarg field once, and where the new priors go. sPool: slots of the exact (Jacobi) fallback's pool.
// Two sets of prior buffers. When the live set is still the one the windows were uploaded / rewound with, the new priors go to the other set and the sets swap
// afterwards: the uploaded priors stay intact for vilf_batch_rewind at no cost (this used to be a 1.7 GB device copy per marginalization and another per rewind).
// A second marginalization without a rewind in between writes in place, as before, so that the snapshot survives.
static int reserve_marg_workspace(vilf_handle *h, size_t sPool, bool to_other_set) {
    const BatchDims dm{(size_t)h->B, (size_t)h->batch.Fmax, (size_t)h->batch.Omax, (size_t)h->batch.FACmax, h->batch.est_td != 0};
    const size_t sB = dm.B, sF = dm.F, sC = dm.C, M = h->mg_Mcap;
    VbMarg &g = h->marg;
    DBuf *d = h->d;
    bool ok = true;
    auto take = [&](int id, size_t bytes, auto *&field) { ok = ok && d[id].ensure(bytes); field = d[id].as<std::remove_reference_t<decltype(*field)>>(); };
    g.Mcap = (int)M; g.init_depth = h->opts.init_depth; g.mflag = d[D_MFLAG].as<int>();
    take(D_MINFO, sB * MG_INFO * 4, g.info); take(D_MF0, sB * sF * 4, g.f0rank);
    take(D_MSTP, sB * VB_POSE_LD * 8, g.st_pose); take(D_MSTS, sB * VB_SB_LD * 8, g.st_sb); take(D_MSTF, sB * sF * 8, g.st_feat); take(D_MSTE, sB * VB_EX_LD * 8, g.st_ex);
    take(D_MBUF, sB * MG_MROW * sC * 8, g.Mbuf); take(D_MHD, sB * MG_ND * MG_ND * 8, g.Hd); take(D_MGD, sB * MG_ND * 8, g.gd); take(D_MWF, sB * sF * MG_ND * 8, g.Wf);
    take(D_MHF, sB * sF * 8, g.hfm); take(D_MGF, sB * sF * 8, g.gfm);
    take(D_MAMM, M > MG_MLDS ? sPool * M * M * 8 : 8, g.Amm); take(D_MX, sPool * M * (MG_NK + 1) * 8, g.X); take(D_MROT, sPool * MG_SWEEPS * (M - 1) * M * 8, g.rot); take(D_MLAM, sPool * M * 8, g.lam);
    take(D_MAR, sB * MG_NK * MG_NK * 8, g.Ar); take(D_MBR, sB * MG_NK * 8, g.br);
    take(D_QLV, sB * MG_NK * (MG_NK + 1) * 8, g.qlV); take(D_QLD, sB * 2 * (MG_NK + 2) * 8, g.qlD); take(D_QLLOG, sB * 2 * QL_RCAP * 8, g.qlLog);
    take(D_QLIT, sB * QL_ICAP * 4, g.qlIt); take(D_QLINFO, sB * 4 * 4, g.qlInfo);
    if (!ok) { h->err = "hipMalloc failed (marginalization workspace)"; return VILF_ERR_DEVICE; }
    if (to_other_set)
        for (const ArrayRow &r : kBatchArrays) if (r.use == A_PRIOR && !d[r.twin].ensure(r.bytes(dm))) { h->err = "hipMalloc failed (second prior set)"; return VILF_ERR_DEVICE; }
    const bool o = to_other_set;
    g.prior_hdr_out = d[o ? D_PHDR0 : D_PHDR].as<int>(); g.prior_x0_out = d[o ? D_PX00 : D_PX0].as<double>(); g.prior_J_out = d[o ? D_PJ0 : D_PJ].as<double>();
    g.prior_r_out = d[o ? D_PR0 : D_PR].as<double>(); g.prior_H_out = d[o ? D_PH0 : D_PH].as<double>(); g.prior_g_out = d[o ? D_PG0 : D_PG].as<double>();
    return VILF_OK;
}

extern "C" int vilf_batch_marginalize(vilf_handle *h, int sync) {
    if (!h || !h->resident) return VILF_ERR_INVALID_ARGUMENT;
    HIPCHECK(h, hipSetDevice(h->device));
    { int rc = upload_priors(h); if (rc != VILF_OK) return rc; }
    const size_t sB = h->B, M = h->mg_Mcap;
    // the exact (Jacobi) fallback's workspace — rotation log, Amm, X, eigenvalues — is a pool of slots, not one per window: the log alone is 24 (M - 1) M doubles
    // (20 MB at 300 dropped features). The pool is as large as 8 GB allow; flagged windows beyond it are taken by further launches of the exact pass.
    const size_t slot_bytes = (MG_SWEEPS * (M - 1) * M + (M > MG_MLDS ? M * M : 0) + M * (MG_NK + 1) + M) * 8;
    size_t sPool = std::max<size_t>(1, std::min<size_t>(sB, ((size_t)8 << 30) / std::max<size_t>(slot_bytes, 1)));
    if (const char *e = std::getenv("VILF_MARG_POOL")) sPool = std::max<size_t>(1, std::min<size_t>(sB, (size_t)std::atoi(e)));      // test hook: several rounds on a small batch
    const bool to_other_set = !h->prior_restore_needed;
    { const int rc = reserve_marg_workspace(h, sPool, to_other_set); if (rc != VILF_OK) return rc; }
    VbMarg &g = h->marg;
    const dim3 grid(h->B), block(VB_NT);
    ProfMarks prof(h, h->marg_prof);
    if (h->batch.est_td) hipLaunchKernelGGL(k_marg_prepare_td, grid, block, 0, h->stream, h->batch, g);
    else hipLaunchKernelGGL(k_marg_prepare, grid, block, 0, h->stream, h->batch, g);
    prof.mark(0);
    hipLaunchKernelGGL(k_marg_schur, grid, block, MGS_FAST_LDS_BYTES, h->stream, h->batch, g,
                       std::getenv("VILF_MARG_FORCE_EXACT") ? 2 : 0);      // test hook: exercise the Jacobi path on well-conditioned windows too
    g.pool = (int)sPool;
    for (int r = 0; r < (int)((sB + sPool - 1) / sPool); r++) {      // one launch unless the pool is smaller than the batch (large Mcap)
        g.pool_round = r;
        hipLaunchKernelGGL(k_marg_schur, grid, block, MGS_EXACT_LDS_BYTES, h->stream, h->batch, g, 1);
    }
    g.pool_round = 0;
    prof.mark(1);
    // kept block: the Cholesky form of the new prior where the reference's 1e-8 truncation provably removes nothing (k_mf_chol; it marks the windows it has
    // finished, the launches below skip those), otherwise the
    // eigen-solver of the kept block in three launches (tred2 per workgroup, the QL recurrence of every window one lane each, rotation replay +
    // prior output per workgroup); k_marg_finish (everything in one workgroup) only takes windows whose rotation log overflowed
    // The kept-block kernels come in two LDS sizes by dimension class (n < MGF_SMALL_N: three workgroups per CU) — for a large batch. A small one (the single window of the
    // real-time case) does not fill the device either way and takes ONE launch of each with the full LDS: four launches less in a chain of mostly empty ones (~5 us each).
    const bool one_class = h->B <= 64;
    // kernel(batch, marg, n_lo, n_hi, tail...) over the kept dimensions [lo, inf): one launch, or one per dimension class, each with its class's LDS (+ extra)
    auto by_class = [&](auto kernel, size_t extra, int lo, auto... tail) {
        if (one_class) hipLaunchKernelGGL(kernel, grid, block, MGF_LDS_BYTES + extra, h->stream, h->batch, g, lo, 1 << 30, tail...);
        else {
            hipLaunchKernelGGL(kernel, grid, block, MGF_SMALL_LDS_BYTES + extra, h->stream, h->batch, g, lo, MGF_SMALL_N, tail...);
            hipLaunchKernelGGL(kernel, grid, block, MGF_LDS_BYTES + extra, h->stream, h->batch, g, MGF_SMALL_N, 1 << 30, tail...);
        }
    };
    {
        const int no_chol = std::getenv("VILF_MARG_NO_CHOL") ? 1 : 0;         // test hook: the eigen-solver for every window
        // n <= 75 (every prior the reference produces without td): the augmented factorisation on the matrix cores (k_mf_chol_tiles, 34 KB of LDS); wider kept blocks:
        // the column-by-column kernel.
        hipLaunchKernelGGL(k_mf_chol_tiles, grid, block, MFT_LDS_BYTES, h->stream, h->batch, g, no_chol);
        by_class(k_mf_chol, 0, SB_ND + 1, no_chol);
    }
    by_class(k_mf_tridiag, 0, 0);
    hipLaunchKernelGGL(k_mf_ql, dim3((h->B + QL_LPW - 1) / QL_LPW), dim3(QL_NT), QL_LDS_BYTES, h->stream, h->batch, g,
                       std::getenv("VILF_MARG_FORCE_QL_FALLBACK") ? 1 : 0);        // test hook
    by_class(k_mf_apply, MFA_LDS_EXTRA_BYTES, 0);
    by_class(k_marg_finish, 0, 0, 1);
    if (to_other_set) {
        hipLaunchKernelGGL(k_prior_keep, grid, block, 0, h->stream, h->batch, g);
        swap_prior_sets(h);
        h->prior_backup_valid = true;           // the other set now holds the priors as uploaded
    }
    prof.mark(2);
    hipLaunchKernelGGL(k_prior_prep, grid, block, PRIOR_PREP_LDS_BYTES, h->stream, h->batch, h->d[D_PH].as<double>(), h->d[D_PG].as<double>(), (unsigned)PRIOR_PREP_LDS_BYTES, (const int *)g.qlInfo);
    prof.mark(3);
    HIPCHECK(h, hipGetLastError());
    if (h->profiling && sync) { const int rcf = vilf_prof_flush(h); if (rcf != VILF_OK) return rcf; }
    for (int w = 0; w < h->B; w++) { h->prior_dev_newer[w] = 1; h->prior_dirty[w] = 0; }
    h->prior_restore_needed = true;
    if (sync) {
        std::vector<int> info(sB * MG_INFO);
        HIPCHECK(h, hipMemcpyAsync(info.data(), g.info, info.size() * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHECK(h, hipStreamSynchronize(h->stream));
        for (int w = 0; w < h->B; w++) {
            const int st = info[(size_t)w * MG_INFO];
            if (st == 2) h->prior_dev_newer[w] = 0;     // SECOND_NEW without Pose[WINDOW_SIZE-1] in the prior: prior unchanged (estimator.cpp:982-983)
            if (st == 3) { h->err = "marginalization: block table / dimension outside the supported range"; return VILF_ERR_UNSUPPORTED; }
        }
    }
    return VILF_OK;
}
extern "C" int vilf_window_marginalize(vilf_handle *h) { return vilf_batch_marginalize(h, 1); }

// which path every window of the last vilf_batch_marginalize took: counts[0] windows that produced a new prior; [1] of those, dropped block Amm by the arrow
// Cholesky (the rest: Jacobi eigen-decomposition with the 1e-8 pseudo-inverse); [2] kept block by Cholesky (J0 = L^T; the rest: tred2 / tql2 eigen-solver);
// [3] windows whose prior was left unchanged (SECOND_NEW without Pose[WINDOW_SIZE - 1] in it) or unsupported
extern "C" int vilf_batch_marginalize_stats(vilf_handle *h, int counts[4]) {
    if (!h || !counts || !h->resident || !h->marg.info || !h->marg.qlInfo) return VILF_ERR_INVALID_ARGUMENT;
    HIPCHECK(h, hipSetDevice(h->device));
    const size_t sB = h->B;
    std::vector<int> info(sB * MG_INFO), qi(sB * 4);
    HIPCHECK(h, hipMemcpyAsync(info.data(), h->marg.info, info.size() * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(h, hipMemcpyAsync(qi.data(), h->marg.qlInfo, qi.size() * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(h, hipStreamSynchronize(h->stream));
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    for (size_t w = 0; w < sB; w++) {
        if (info[w * MG_INFO] != 0) { counts[3]++; continue; }
        counts[0]++;
        if (info[w * MG_INFO + 7] == 0) counts[1]++;
        if (qi[w * 4 + 3] == 1) counts[2]++;
    }
    return VILF_OK;
}

// ---- Ceres-layout hooks --------------------------------------------------------------------------------------
static int hook_buf(vilf_handle *h, size_t doubles) { return h->d[D_HOOK].ensure(doubles * 8) ? VILF_OK : VILF_ERR_DEVICE; }

extern "C" int vilf_eval_projection(vilf_handle *h, const double *const *p, const double pts_i[3], const double pts_j[3], double *residuals, double **jac) {
    if (!h || !p || !residuals) return VILF_ERR_INVALID_ARGUMENT;
    if (hook_buf(h, 256) != VILF_OK) return VILF_ERR_DEVICE;
    double in[32];
    std::memcpy(in, p[0], 56); std::memcpy(in + 7, p[1], 56); std::memcpy(in + 14, p[2], 56);
    std::memcpy(in + 21, pts_i, 24); std::memcpy(in + 24, pts_j, 24);
    double *d = h->d[D_HOOK].as<double>();
    HIPCHECK(h, hipMemcpyAsync(d, in, sizeof(in), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_hook_projection, dim3(1), dim3(HOOK_NT), 0, h->stream, d, d + 7, d + 14, p[3][0], d + 21, d + 24, h->opts.focal_length / 1.5, d + 32);
    double out[28];
    HIPCHECK(h, hipMemcpyAsync(out, d + 32, sizeof(out), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(h, hipStreamSynchronize(h->stream));
    residuals[0] = out[0]; residuals[1] = out[1];
    if (jac) {
        for (int blk = 0; blk < 2; blk++)
            if (jac[blk]) for (int r = 0; r < 2; r++) { for (int c = 0; c < 6; c++) jac[blk][7 * r + c] = out[2 + 12 * blk + 6 * r + c]; jac[blk][7 * r + 6] = 0; }
        if (jac[2]) {                               // Ex_Pose block (projection_factor.cpp:97-104): the device routine of the general path (ProjectionTdFactor with td = td_i = td_j, zero velocity
                                                    // = ProjectionFactor); its residual and other blocks are the same function of the same inputs
            double in2[40] = {0};
            std::memcpy(in2, in, 27 * 8);
            in2[31] = p[3][0]; in2[37] = 0.0; in2[38] = h->opts.focal_length / 1.5;
            HIPCHECK(h, hipMemcpyAsync(d + 64, in2, sizeof(in2), hipMemcpyHostToDevice, h->stream));
            hipLaunchKernelGGL(k_hook_projection_td, dim3(1), dim3(HOOK_NT), 0, h->stream, d + 64, d + 64 + 40);
            double out2[42];
            HIPCHECK(h, hipMemcpyAsync(out2, d + 64 + 40, sizeof(out2), hipMemcpyDeviceToHost, h->stream));
            HIPCHECK(h, hipStreamSynchronize(h->stream));
            for (int r = 0; r < 2; r++) { for (int c = 0; c < 6; c++) jac[2][7 * r + c] = out2[26 + 6 * r + c]; jac[2][7 * r + 6] = 0; }
        }
        if (jac[3]) { jac[3][0] = out[26]; jac[3][1] = out[27]; }
    }
    return VILF_OK;
}

extern "C" int vilf_eval_projection_td(vilf_handle *h, const double *const *p, const double pts_i[3], const double pts_j[3], const double vel_i[2], const double vel_j[2],
                                       double td_i, double td_j, double row_i, double row_j, double *residuals, double **jac) {
    if (!h || !p || !residuals || !pts_i || !pts_j || !vel_i || !vel_j) return VILF_ERR_INVALID_ARGUMENT;
    if (hook_buf(h, 128) != VILF_OK) return VILF_ERR_DEVICE;
    double in[40];
    std::memcpy(in, p[0], 56); std::memcpy(in + 7, p[1], 56); std::memcpy(in + 14, p[2], 56);
    std::memcpy(in + 21, pts_i, 24); std::memcpy(in + 24, pts_j, 24); std::memcpy(in + 27, vel_i, 16); std::memcpy(in + 29, vel_j, 16);
    const double ROW = h->opts.ROW;
    in[31] = p[3][0]; in[32] = p[4][0]; in[33] = td_i; in[34] = td_j; in[35] = row_i - ROW / 2; in[36] = row_j - ROW / 2;      // projection_td_factor.cpp:19-20
    in[37] = h->opts.TR / ROW; in[38] = h->opts.focal_length / 1.5;
    double *d = h->d[D_HOOK].as<double>();
    HIPCHECK(h, hipMemcpyAsync(d, in, sizeof(in), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_hook_projection_td, dim3(1), dim3(HOOK_NT), 0, h->stream, d, d + 40);
    double out[42];
    HIPCHECK(h, hipMemcpyAsync(out, d + 40, sizeof(out), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(h, hipStreamSynchronize(h->stream));
    residuals[0] = out[0]; residuals[1] = out[1];
    if (jac) {
        const int off[3] = {2, 14, 26};
        for (int blk = 0; blk < 3; blk++)
            if (jac[blk]) for (int r = 0; r < 2; r++) { for (int c = 0; c < 6; c++) jac[blk][7 * r + c] = out[off[blk] + 6 * r + c]; jac[blk][7 * r + 6] = 0; }
        if (jac[3]) { jac[3][0] = out[38]; jac[3][1] = out[39]; }
        if (jac[4]) { jac[4][0] = out[40]; jac[4][1] = out[41]; }
    }
    return VILF_OK;
}

static void pack_imu_rec(const vilf_imu_preint *p, double *rec) {
    std::memset(rec, 0, IMU_REC * 8);
    fill_imu_rec(*p, rec);
    rec[287] = 1.0;
}

// IMUFactor::Evaluate on the device for one factor (k_imu_prep + k_hook_imu); *d_out: the hook buffer, results at + 2048 (weighted), + 3072 (raw), sqrt_info inside the record at + 40
static int run_imu_hook(vilf_handle *h, const double *const *p, const vilf_imu_preint *pre, double **d_out) {
    if (hook_buf(h, 4096) != VILF_OK) return VILF_ERR_DEVICE;
    double *d = *d_out = h->d[D_HOOK].as<double>();
    std::vector<double> in(40 + IMU_REC + 225, 0.0);
    std::memcpy(&in[0], p[0], 56); std::memcpy(&in[7], p[1], 72); std::memcpy(&in[16], p[2], 56); std::memcpy(&in[23], p[3], 72);
    for (int i = 0; i < 3; i++) in[32 + i] = h->opts.G[i];
    pack_imu_rec(pre, &in[40]);
    std::memcpy(&in[40 + IMU_REC], pre->covariance, 225 * 8);
    HIPCHECK(h, vilf_copy_sync(h, d, in.data(), in.size() * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_imu_prep, dim3(1), dim3(IMU_PREP_NT), 0, h->stream, 1, d + 40 + IMU_REC, d + 1024, d + 40);
    hipLaunchKernelGGL(k_hook_imu, dim3(1), dim3(HOOK_NT), 0, h->stream, d, d + 7, d + 16, d + 23, d + 40, d + 32, d + 2048, d + 3072);
    return VILF_OK;
}
extern "C" int vilf_eval_imu(vilf_handle *h, const double *const *p, const vilf_imu_preint *pre, double *residuals, double **jac) {
    if (!h || !p || !pre || !residuals) return VILF_ERR_INVALID_ARGUMENT;
    double *d;
    { const int rc = run_imu_hook(h, p, pre, &d); if (rc != VILF_OK) return rc; }
    std::vector<double> out(15 + 450);
    HIPCHECK(h, hipMemcpyAsync(out.data(), d + 2048, out.size() * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < 15; i++) residuals[i] = out[i];
    if (jac) {
        const int off[4] = {0, 6, 15, 21}, loc[4] = {6, 9, 6, 9}, glob[4] = {7, 9, 7, 9};
        for (int blk = 0; blk < 4; blk++)
            if (jac[blk]) for (int r = 0; r < 15; r++) { for (int c = 0; c < glob[blk]; c++) jac[blk][glob[blk] * r + c] = (c < loc[blk]) ? out[15 + 30 * r + off[blk] + c] : 0.0; }
    }
    return VILF_OK;
}

// the parts of IMUFactor::Evaluate on their own: residual / Jacobians BEFORE the multiplication by sqrt_info (Ceres layout as above), and the 15 x 15 sqrt_info the device
// computes once per upload (k_imu_prep) — the tests compare each tightly instead of only their ill-conditioned product
extern "C" int vilf_eval_imu_raw(vilf_handle *h, const double *const *p, const vilf_imu_preint *pre, double *residuals, double **jac, double *sqrt_info_out) {
    if (!h || !p || !pre || !residuals) return VILF_ERR_INVALID_ARGUMENT;
    double *d;
    { const int rc = run_imu_hook(h, p, pre, &d); if (rc != VILF_OK) return rc; }
    std::vector<double> raw(450 + 15), S(225);
    HIPCHECK(h, hipMemcpyAsync(raw.data(), d + 3072, raw.size() * 8, hipMemcpyDeviceToHost, h->stream));       // scratch of k_hook_imu: J_raw [15 x 30], r_raw [15]
    HIPCHECK(h, hipMemcpyAsync(S.data(), d + 40 + IMU_SQRT, 225 * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < 15; i++) residuals[i] = raw[450 + i];
    if (jac) {
        const int off[4] = {0, 6, 15, 21}, loc[4] = {6, 9, 6, 9}, glob[4] = {7, 9, 7, 9};
        for (int blk = 0; blk < 4; blk++)
            if (jac[blk]) for (int r = 0; r < 15; r++) { for (int c = 0; c < glob[blk]; c++) jac[blk][glob[blk] * r + c] = (c < loc[blk]) ? raw[30 * r + off[blk] + c] : 0.0; }
    }
    if (sqrt_info_out) std::memcpy(sqrt_info_out, S.data(), 225 * 8);
    return VILF_OK;
}

extern "C" int vilf_eval_lidar_between(vilf_handle *h, const double *const *p, const vilf_lidar_constraint *c, double *residuals, double **jac) {
    if (!h || !p || !c || !residuals) return VILF_ERR_INVALID_ARGUMENT;
    if (hook_buf(h, 256) != VILF_OK) return VILF_ERR_DEVICE;
    if (!h->resident) lidar_extrinsic(h->opts, h->batch);   // qil / til are derived at upload; derive here too
    double in[32];
    std::memcpy(in, p[0], 56); std::memcpy(in + 7, p[1], 56);
    std::memcpy(in + 14, h->batch.qil, 32); std::memcpy(in + 18, h->batch.til, 24);
    for (int i = 0; i < 4; i++) in[21 + i] = c->q[i];
    for (int i = 0; i < 3; i++) in[25 + i] = c->t[i];
    double *d = h->d[D_HOOK].as<double>();
    HIPCHECK(h, hipMemcpyAsync(d, in, sizeof(in), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_hook_lidar, dim3(1), dim3(HOOK_NT), 0, h->stream, d, d + 7, d + 14, d + 18, d + 21, d + 32);
    double out[78];
    HIPCHECK(h, hipMemcpyAsync(out, d + 32, sizeof(out), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < 6; i++) residuals[i] = out[i];
    if (jac)
        for (int blk = 0; blk < 2; blk++)
            if (jac[blk]) for (int r = 0; r < 6; r++) { for (int cc = 0; cc < 6; cc++) jac[blk][7 * r + cc] = out[6 + 36 * blk + 6 * r + cc]; jac[blk][7 * r + 6] = 0; }
    return VILF_OK;
}

extern "C" int vilf_eval_edge(vilf_handle *h, const double pose[7], const double cp[3], const double a[3], const double bb[3], double r[3], double *J) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    if (hook_buf(h, 128) != VILF_OK) return VILF_ERR_DEVICE;
    double in[16];
    std::memcpy(in, pose, 56); std::memcpy(in + 7, cp, 24); std::memcpy(in + 10, a, 24); std::memcpy(in + 13, bb, 24);
    double *d = h->d[D_HOOK].as<double>();
    HIPCHECK(h, hipMemcpyAsync(d, in, sizeof(in), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_hook_edge, dim3(1), dim3(HOOK_NT), 0, h->stream, d, d + 7, d + 10, d + 13, d + 16);
    double out[21];
    HIPCHECK(h, hipMemcpyAsync(out, d + 16, sizeof(out), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < 3; i++) r[i] = out[i];
    if (J) for (int i = 0; i < 3; i++) { for (int c = 0; c < 6; c++) J[7 * i + c] = out[3 + 6 * i + c]; J[7 * i + 6] = 0; }
    return VILF_OK;
}

extern "C" int vilf_eval_surf(vilf_handle *h, const double pose[7], const double cp[3], const double n[3], double dd, double r[1], double *J) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    if (hook_buf(h, 128) != VILF_OK) return VILF_ERR_DEVICE;
    double in[16];
    std::memcpy(in, pose, 56); std::memcpy(in + 7, cp, 24); std::memcpy(in + 10, n, 24);
    double *d = h->d[D_HOOK].as<double>();
    HIPCHECK(h, hipMemcpyAsync(d, in, sizeof(in), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_hook_surf, dim3(1), dim3(HOOK_NT), 0, h->stream, d, d + 7, d + 10, dd, d + 16);
    double out[7];
    HIPCHECK(h, hipMemcpyAsync(out, d + 16, sizeof(out), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(h, hipStreamSynchronize(h->stream));
    r[0] = out[0];
    if (J) { for (int c = 0; c < 6; c++) J[c] = out[1 + c]; J[6] = 0; }
    return VILF_OK;
}

static int plus_hook(vilf_handle *h, const double x[7], const double dl[6], double xp[7], int kind) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    if (hook_buf(h, 64) != VILF_OK) return VILF_ERR_DEVICE;
    double in[13];
    std::memcpy(in, x, 56); std::memcpy(in + 7, dl, 48);
    double *d = h->d[D_HOOK].as<double>();
    HIPCHECK(h, hipMemcpyAsync(d, in, sizeof(in), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_hook_plus, dim3(1), dim3(HOOK_NT), 0, h->stream, d, d + 7, kind, d + 16);
    HIPCHECK(h, hipMemcpyAsync(xp, d + 16, 56, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(h, hipStreamSynchronize(h->stream));
    return VILF_OK;
}
extern "C" int vilf_pose_plus(vilf_handle *h, const double x[7], const double d[6], double xp[7]) { return plus_hook(h, x, d, xp, 0); }
extern "C" int vilf_se3_plus(vilf_handle *h, const double x[7], const double d[6], double xp[7]) { return plus_hook(h, x, d, xp, 1); }

extern "C" int vilf_eval_prior(vilf_handle *h, const vilf_prior *p, const double *const *params, double *residuals, double **jac) {
    if (!h || !p || !params || !residuals || !p->valid || p->n < 1 || p->n > VILF_PRIOR_MAX_DIM || p->n_blocks < 1 || p->n_blocks > VILF_PRIOR_MAX_BLOCKS) return VILF_ERR_INVALID_ARGUMENT;
    if (!prior_block_table_ok(p)) { h->err = "prior block table out of range"; return VILF_ERR_INVALID_ARGUMENT; }      // k_hook_prior indexes its LDS vector with the table
    const int n = p->n, nb = p->n_blocks;
    for (int i = 0; i < nb; i++) if (!params[i]) return VILF_ERR_INVALID_ARGUMENT;
    const size_t doubles = 32 + 2 * 24 * 9 + (size_t)n * n + 2 * (size_t)n + 16;
    if (hook_buf(h, doubles) != VILF_OK) return VILF_ERR_DEVICE;
    std::vector<double> in(32 + 2 * 24 * 9 + (size_t)n * n + n, 0.0);
    int *hdr = reinterpret_cast<int *>(in.data());             // 64 ints in the first 32 doubles
    hdr[0] = n; hdr[1] = nb;
    for (int i = 0; i < nb; i++) {
        hdr[2 + i] = p->block_size[i]; hdr[26 + i] = p->block_idx[i];
        if (!params[i]) return VILF_ERR_INVALID_ARGUMENT;
        for (int k = 0; k < p->block_size[i] && k < 9; k++) { in[32 + 9 * i + k] = p->block_x0[i][k]; in[32 + 216 + 9 * i + k] = params[i][k]; }
    }
    std::memcpy(&in[32 + 432], p->linearized_jacobians, sizeof(double) * n * n);
    std::memcpy(&in[32 + 432 + (size_t)n * n], p->linearized_residuals, sizeof(double) * n);
    double *d = h->d[D_HOOK].as<double>();
    HIPCHECK(h, hipMemcpyAsync(d, in.data(), in.size() * 8, hipMemcpyHostToDevice, h->stream));
    double *d_out = d + in.size();
    hipLaunchKernelGGL(k_hook_prior, dim3(1), dim3(HOOK_PRIOR_NT), 0, h->stream, reinterpret_cast<const int *>(d), d + 32, d + 32 + 216, d + 32 + 432, d + 32 + 432 + (size_t)n * n, d_out);
    HIPCHECK(h, hipMemcpyAsync(residuals, d_out, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(h, hipStreamSynchronize(h->stream));
    if (jac)                                                   // jacobians[i] = J0[:, idx : idx + local] in global size (pose: 7th column 0), :364-376
        for (int i = 0; i < nb; i++) {
            if (!jac[i]) continue;
            const int gs = p->block_size[i], ls = gs == 7 ? 6 : gs, idx = p->block_idx[i];
            for (int r = 0; r < n; r++) for (int c = 0; c < gs; c++) jac[i][(size_t)r * gs + c] = c < ls ? p->linearized_jacobians[(size_t)r * n + idx + c] : 0.0;
        }
    return VILF_OK;
}
