// vilf_ba.hip — the third stage of the visual start-up on the device (≙ the full bundle adjustment of GlobalSFM::construct, initial/initial_sfm.cpp:232-310, with
//   ReprojectionError3D, initial_sfm.h:25-54). The arithmetic is stated once, in include/vilfusion.h ("Visual start-up: GlobalSFM full BA").
//   su_sfm_ba      a workgroup of 256 per window runs the whole Levenberg-Marquardt with barriers. Poses, positions, every member's V^-1 and point gradient and the
//                  reduced camera system S stay in LDS across the iterations. A thread takes the features tid, tid + 256, ..: its point terms, its share of every
//                  total over the members, its back-substitution. The couplings W are not stored (11 frames x 18 numbers per member would not fit): they are
//                  computed again where they are needed, frame pair by frame pair. S is factorised in place, column by column (right-looking: the trailing
//                  update of column k takes u_ik L_jk out of entry (j, i), which is the text's order of subtractions), all threads on the entries, two barriers a column.
//   vilf_startup_construct enqueues the chain (vilf_sfm_enqueue, vilf_sfm.hip) and this kernel behind it; the chain's rows and structure are read where it wrote them.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <algorithm>
#include "vilf_internal.hpp"
#include "vilf_device.hpp"

#define BA_MAXN VILF_MAX_FEATURES
#define BA_MAXF VILF_MAX_FRAMES
#define BA_MAXC (6 * BA_MAXF - 9)           // the camera unknowns of a full window: 57
#define BA_WIN_INTS VILF_SU_WIN_INTS
#define BA_CAM 28                           // a frame's camera terms: 21 of U, 6 of g, c
#define BA_PAIR 42                          // a frame pair's terms: 36 of T, 6 of the right-hand side

struct BaPar { int iters; double lambda0, ftol, cthr; };
struct BaDev {
    const int *win; const double *pts; const int *l;               // the windows as stage one uploads them; [window]
    const int *chain_ok; int chain_stride;                         // chain_ok[window * chain_stride]
    const double *pose; int pose_stride;                           // frame k of window w at pose + (w * BA_MAXF + k) * pose_stride: c_R (9), c_t (3)
    const unsigned char *state; const double *pos;                 // [window][BA_MAXN] (x 3)
    vilf_startup_ba_result *res; vilf_startup_ba_frame *frames; unsigned char *state_out; double *pos_out;   // the download
};

// ---- launch contract -----------------------------------------------------------------------------------------------------
#define BA_NT 256                           // block BA_NT, one workgroup per window, BA_LDS_BYTES of dynamic LDS
#define BA_OFF_VI 0                                              // in doubles
#define BA_OFF_GP (BA_OFF_VI + 6 * BA_MAXN)
#define BA_OFF_POS (BA_OFF_GP + 3 * BA_MAXN)
#define BA_OFF_POSN (BA_OFF_POS + 3 * BA_MAXN)
#define BA_OFF_S (BA_OFF_POSN + 3 * BA_MAXN)
#define BA_OFF_X (BA_OFF_S + BA_MAXC * BA_MAXC)
#define BA_OFF_U (BA_OFF_X + BA_MAXC + 1)
#define BA_OFF_G (BA_OFF_U + BA_MAXF * 21)
#define BA_OFF_P (BA_OFF_G + BA_MAXF * 6)
#define BA_OFF_PN (BA_OFF_P + BA_MAXF * 12)
#define BA_OFF_CK (BA_OFF_PN + BA_MAXF * 12)
#define BA_OFF_RED (BA_OFF_CK + 2 * BA_MAXF)
#define BA_OFF_FLAG (BA_OFF_RED + 2 * 4 * BA_PAIR)
#define BA_LDS_BYTES ((size_t)BA_OFF_FLAG * 8 + 4 * 4 + BA_MAXN)
static_assert(BA_LDS_BYTES <= 160 * 1024, "the BA's LDS fits a CU");
static_assert(BA_MAXN <= 4 * BA_NT, "a thread takes at most four features");
__global__ void su_sfm_ba(BaDev d, BaPar p);

struct BaCtx : VilfStage {
    StageIO io;
    int last_windows = 0;
    size_t last_state = 0, last_pos = 0;                           // where the last call's download holds the state and the positions
    StageProf<1> prof;
    bool attr = false;
    void profile_reset() override { prof.reset(); }
};

namespace {
VD double ba_pair(double a0, double b0, double a1, double b1) { return __dadd_rn(__dmul_rn(a0, b0), __dmul_rn(a1, b1)); }

// the paragraph "sums over features": the butterfly within the wave, then waves 0 + 1 + 2 + 3; red [4][K]. Thread e < K returns with the total of term e, the
// others with 0. Two calls in a row take different red.
template <int K> VD double ba_total(double (&v)[K], double *red, int tid) {
#pragma unroll
    for (int k = 0; k < K; k++)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] = __dadd_rn(v[k], __shfl_xor(v[k], o));
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) red[(tid >> 6) * K + k] = v[k];
    }
    __syncthreads();
    return tid < K ? __dadd_rn(__dadd_rn(__dadd_rn(red[tid], red[K + tid]), red[2 * K + tid]), red[3 * K + tid]) : 0.0;
}

// the paragraphs "residual" and "Jacobian" of one observation under the pose P (3 x 4, row-major): the camera's rows J0, J1 (all six entries; the caller uses the
// first n_k), the point's rows P0, P1
VD void ba_obs(const double *P, const double *X, const double *u, double *J0, double *J1, double *P0, double *P1, double &e0, double &e1) {
    double q[3];
#pragma unroll
    for (int r = 0; r < 3; r++) q[r] = vilf_dot3(P[r * 4], X[0], P[r * 4 + 1], X[1], P[r * 4 + 2], X[2]);
    const double p0 = __dadd_rn(q[0], P[3]), p1 = __dadd_rn(q[1], P[7]), p2 = __dadd_rn(q[2], P[11]);
    const double iz = __ddiv_rn(1.0, p2), xn = __dmul_rn(p0, iz), yn = __dmul_rn(p1, iz);
    e0 = __dsub_rn(xn, u[0]); e1 = __dsub_rn(yn, u[1]);
    const double c0 = __dmul_rn(xn, iz), c1 = __dmul_rn(yn, iz);
    J0[0] = -__dmul_rn(c0, q[1]); J0[1] = __dadd_rn(__dmul_rn(iz, q[2]), __dmul_rn(c0, q[0])); J0[2] = -__dmul_rn(iz, q[1]); J0[3] = iz; J0[4] = 0.0; J0[5] = -c0;
    J1[0] = -__dadd_rn(__dmul_rn(iz, q[2]), __dmul_rn(c1, q[1])); J1[1] = __dmul_rn(c1, q[0]); J1[2] = __dmul_rn(iz, q[0]); J1[3] = 0.0; J1[4] = iz; J1[5] = -c1;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        P0[c] = __dsub_rn(__dmul_rn(iz, P[c]), __dmul_rn(c0, P[8 + c]));
        P1[c] = __dsub_rn(__dmul_rn(iz, P[4 + c]), __dmul_rn(c1, P[8 + c]));
    }
}
// the residual alone, squared
VD double ba_sq(const double *P, const double *X, const double *u) {
    double q[3];
#pragma unroll
    for (int r = 0; r < 3; r++) q[r] = vilf_dot3(P[r * 4], X[0], P[r * 4 + 1], X[1], P[r * 4 + 2], X[2]);
    const double p0 = __dadd_rn(q[0], P[3]), p1 = __dadd_rn(q[1], P[7]), p2 = __dadd_rn(q[2], P[11]);
    const double iz = __ddiv_rn(1.0, p2), e0 = __dsub_rn(__dmul_rn(p0, iz), u[0]), e1 = __dsub_rn(__dmul_rn(p1, iz), u[1]);
    return ba_pair(e0, e0, e1, e1);
}
// the paragraph "coupling": W [6][3] of an observation
VD void ba_w(const double *J0, const double *J1, const double *P0, const double *P1, double (&W)[6][3]) {
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int c = 0; c < 3; c++) W[a][c] = ba_pair(J0[a], P0[c], J1[a], P1[c]);
}
VD int ba_free(int k, int l, int newest) { return k == l ? 0 : (k == newest ? 3 : 6); }      // n_k
VD int ba_first(int k, int l) { return 6 * (k - (k > l ? 1 : 0)); }                           // o_k
}  // namespace

// ---- su_sfm_ba: a workgroup per window -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BA_NT) void su_sfm_ba(BaDev d, BaPar p) {
    extern __shared__ double ba_lds[];
    double *s_vi = ba_lds + BA_OFF_VI, *s_gp = ba_lds + BA_OFF_GP, *s_pos = ba_lds + BA_OFF_POS, *s_posn = ba_lds + BA_OFF_POSN, *s_S = ba_lds + BA_OFF_S;
    double *s_x = ba_lds + BA_OFF_X, *s_U = ba_lds + BA_OFF_U, *s_g = ba_lds + BA_OFF_G, *s_P = ba_lds + BA_OFF_P, *s_Pn = ba_lds + BA_OFF_PN;
    double *s_ck = ba_lds + BA_OFF_CK, *s_ck2 = s_ck + BA_MAXF, *s_red = ba_lds + BA_OFF_RED;
    int *s_flag = (int *)(ba_lds + BA_OFF_FLAG);                            // 0: a pivot of a member's V, 1: not finite, 2: members, 3: residuals
    unsigned char *s_state = (unsigned char *)(s_flag + 4);
    const int tid = threadIdx.x, w = blockIdx.x;
    const int *win = d.win + (size_t)w * BA_WIN_INTS, *start = win + 4, *first = win + 4 + BA_MAXN;
    const int nf = min(max(win[0], 2), BA_MAXF), n = min(max(win[1], 0), BA_MAXN), newest = nf - 1;      // the host has checked all three
    const double *pts = d.pts + (size_t)win[2] * 2;
    const int l = d.l[w];
    vilf_startup_ba_frame *frames = d.frames + (size_t)w * BA_MAXF;
    unsigned char *state_out = d.state_out + (size_t)w * BA_MAXN;
    double *pos_out = d.pos_out + (size_t)w * BA_MAXN * 3;
    const bool run = l >= 0 && l < newest && d.chain_ok[(size_t)w * d.chain_stride] != 0;
    for (int e = tid; e < (int)(BA_MAXF * sizeof(vilf_startup_ba_frame) / 8); e += BA_NT) ((double *)frames)[e] = 0.0;
    if (!run) {                                                             // skipped: everything 0 but l
        for (int f = tid; f < BA_MAXN; f += BA_NT) { state_out[f] = 0; pos_out[3 * f] = 0.0; pos_out[3 * f + 1] = 0.0; pos_out[3 * f + 2] = 0.0; }
        if (tid == 0) {
            vilf_startup_ba_result r;
            r.ok = 0; r.flags = 0; r.iterations = 0; r.accepted = 0; r.n_camera = 0; r.n_members = 0; r.n_residuals = 0; r.l = l; r.cost0 = 0.0; r.cost1 = 0.0; r.lambda = 0.0;
            d.res[w] = r;
        }
        return;
    }
    // the start: state, positions (0 where the state is 0), poses as 3 x 4; the members and their observations are counted
    if (tid < 4) s_flag[tid] = 0;
    __syncthreads();
    {
        const unsigned char *st_in = d.state + (size_t)w * BA_MAXN;
        const double *pos_in = d.pos + (size_t)w * BA_MAXN * 3;
        int members = 0, obs = 0;
        for (int f = tid; f < BA_MAXN; f += BA_NT) {
            const unsigned char s = f < n && st_in[f] ? 1 : 0;
            s_state[f] = s;
#pragma unroll
            for (int c = 0; c < 3; c++) s_pos[3 * f + c] = s ? pos_in[3 * f + c] : 0.0;
            if (s) { members++; obs += first[f + 1] - first[f]; }
        }
        for (int e = tid; e < nf * 12; e += BA_NT) {
            const int k = e / 12, r = (e % 12) / 4, c = e % 4;
            const double *ps = d.pose + ((size_t)w * BA_MAXF + k) * d.pose_stride;
            s_P[e] = c < 3 ? ps[r * 3 + c] : ps[9 + r];
        }
        if (members) { atomicAdd(s_flag + 2, members); atomicAdd(s_flag + 3, obs); }
    }
    __syncthreads();
    const int nc = 6 * nf - 9, n_members = s_flag[2], n_res = s_flag[3];
    double lam = p.lambda0, cost = 0.0, cost0 = 0.0;
    int iterations = 0, accepted = 0, par = 0;
    bool converged = false;
    for (int it = 0; it < p.iters && !converged; it++) {
        iterations++;
        if (tid == 0) s_flag[0] = 0;
        __syncthreads();
        // the point terms of the thread's members: V, gp, the damped LDL^T, V^-1
        for (int f = tid; f < n; f += BA_NT) {
            if (!s_state[f]) continue;
            const int st = start[f], nobs = first[f + 1] - first[f];
            const double *pt = pts + (size_t)first[f] * 2;
            const double X[3] = {s_pos[3 * f], s_pos[3 * f + 1], s_pos[3 * f + 2]};
            double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, gp[3] = {0.0, 0.0, 0.0};
            for (int o = 0; o < nobs; o++) {
                double J0[6], J1[6], P0[3], P1[3], e0, e1;
                ba_obs(s_P + (st + o) * 12, X, pt + 2 * o, J0, J1, P0, P1, e0, e1);                  // st + o < nf: the host has checked the table
                v[0] = __dadd_rn(v[0], ba_pair(P0[0], P0[0], P1[0], P1[0])); v[1] = __dadd_rn(v[1], ba_pair(P0[0], P0[1], P1[0], P1[1]));
                v[2] = __dadd_rn(v[2], ba_pair(P0[0], P0[2], P1[0], P1[2])); v[3] = __dadd_rn(v[3], ba_pair(P0[1], P0[1], P1[1], P1[1]));
                v[4] = __dadd_rn(v[4], ba_pair(P0[1], P0[2], P1[1], P1[2])); v[5] = __dadd_rn(v[5], ba_pair(P0[2], P0[2], P1[2], P1[2]));
#pragma unroll
                for (int c = 0; c < 3; c++) gp[c] = __dadd_rn(gp[c], ba_pair(P0[c], e0, P1[c], e1));
            }
            const double v00 = __dadd_rn(v[0], __dmul_rn(lam, v[0])), v11 = __dadd_rn(v[3], __dmul_rn(lam, v[3])), v22 = __dadd_rn(v[5], __dmul_rn(lam, v[5]));
            const double d0 = v00, L10 = __ddiv_rn(v[1], d0), L20 = __ddiv_rn(v[2], d0);
            const double d1 = __dsub_rn(v11, __dmul_rn(v[1], L10)), u = __dsub_rn(v[4], __dmul_rn(v[2], L10)), L21 = __ddiv_rn(u, d1);
            const double d2 = __dsub_rn(__dsub_rn(v22, __dmul_rn(v[2], L20)), __dmul_rn(u, L21));
            if (!(d0 > 0.0 && d1 > 0.0 && d2 > 0.0)) s_flag[0] = 1;
            const double i0 = __ddiv_rn(1.0, d0), i1 = __ddiv_rn(1.0, d1), i2 = __ddiv_rn(1.0, d2);
            const double m10 = -L10, m21 = -L21, m20 = __dsub_rn(__dmul_rn(L21, L10), L20);
            const double Vi22 = i2, Vi12 = __dmul_rn(m21, i2), Vi02 = __dmul_rn(m20, i2), Vi11 = __dadd_rn(i1, __dmul_rn(m21, Vi12));
            const double Vi01 = __dadd_rn(__dmul_rn(m10, i1), __dmul_rn(m21, Vi02));
            const double Vi00 = __dadd_rn(__dadd_rn(i0, __dmul_rn(m10, __dmul_rn(m10, i1))), __dmul_rn(m20, Vi02));
            double *vi = s_vi + 6 * f;
            vi[0] = Vi00; vi[1] = Vi01; vi[2] = Vi02; vi[3] = Vi11; vi[4] = Vi12; vi[5] = Vi22;
#pragma unroll
            for (int c = 0; c < 3; c++) s_gp[3 * f + c] = gp[c];
        }
        // the camera terms and the cost, frame by frame
        for (int k = 0; k < nf; k++) {
            double s[BA_CAM];
#pragma unroll
            for (int e = 0; e < BA_CAM; e++) s[e] = 0.0;
            for (int f = tid; f < n; f += BA_NT) {
                const int st = start[f], o = k - st;
                if (!s_state[f] || o < 0 || o >= first[f + 1] - first[f]) continue;
                double J0[6], J1[6], P0[3], P1[3], e0, e1;
                ba_obs(s_P + k * 12, s_pos + 3 * f, pts + (size_t)(first[f] + o) * 2, J0, J1, P0, P1, e0, e1);
                int q = 0;
#pragma unroll
                for (int a = 0; a < 6; a++)
#pragma unroll
                    for (int b = a; b < 6; b++, q++) s[q] = __dadd_rn(s[q], ba_pair(J0[a], J0[b], J1[a], J1[b]));
#pragma unroll
                for (int a = 0; a < 6; a++) s[21 + a] = __dadd_rn(s[21 + a], ba_pair(J0[a], e0, J1[a], e1));
                s[27] = __dadd_rn(s[27], ba_pair(e0, e0, e1, e1));
            }
            const double tot = ba_total<BA_CAM>(s, s_red + par * 4 * BA_PAIR, tid);
            par ^= 1;
            if (tid < 21) s_U[k * 21 + tid] = tot;
            else if (tid < 27) s_g[k * 6 + tid - 21] = tot;
            else if (tid == 27) s_ck[k] = tot;
        }
        __syncthreads();
        cost = 0.0;
        for (int k = 0; k < nf; k++) cost = __dadd_rn(cost, s_ck[k]);
        if (it == 0) cost0 = cost;
        bool pos = s_flag[0] == 0;
        if (pos) {
            // the reduced system, frame pair by frame pair
            for (int j = 0; j < nf; j++) {
                const int nj = ba_free(j, l, newest), oj = ba_first(j, l);
                if (nj == 0) continue;
                for (int k = j; k < nf; k++) {
                    const int nk = ba_free(k, l, newest), ok = ba_first(k, l);
                    if (nk == 0) continue;
                    double t[BA_PAIR];
#pragma unroll
                    for (int e = 0; e < BA_PAIR; e++) t[e] = 0.0;
                    for (int f = tid; f < n; f += BA_NT) {
                        const int st = start[f], nobs = first[f + 1] - first[f];
                        if (!s_state[f] || j < st || k >= st + nobs) continue;                     // j <= k: seen in both
                        double J0[6], J1[6], P0[3], P1[3], e0, e1, Wj[6][3], Wk[6][3], Y[6][3];
                        ba_obs(s_P + j * 12, s_pos + 3 * f, pts + (size_t)(first[f] + j - st) * 2, J0, J1, P0, P1, e0, e1);
                        ba_w(J0, J1, P0, P1, Wj);
                        if (k != j) {
                            ba_obs(s_P + k * 12, s_pos + 3 * f, pts + (size_t)(first[f] + k - st) * 2, J0, J1, P0, P1, e0, e1);
                            ba_w(J0, J1, P0, P1, Wk);
                        } else {
#pragma unroll
                            for (int a = 0; a < 6; a++)
#pragma unroll
                                for (int c = 0; c < 3; c++) Wk[a][c] = Wj[a][c];
                        }
                        const double *vi = s_vi + 6 * f, *gp = s_gp + 3 * f;
                        const double V0[3] = {vi[0], vi[1], vi[2]}, V1[3] = {vi[1], vi[3], vi[4]}, V2[3] = {vi[2], vi[4], vi[5]};
#pragma unroll
                        for (int a = 0; a < 6; a++)
#pragma unroll
                            for (int c = 0; c < 3; c++) Y[a][c] = vilf_dot3(Wj[a][0], V0[c], Wj[a][1], V1[c], Wj[a][2], V2[c]);
#pragma unroll
                        for (int a = 0; a < 6; a++) {
#pragma unroll
                            for (int b = 0; b < 6; b++) t[a * 6 + b] = __dadd_rn(t[a * 6 + b], vilf_dot3(Y[a][0], Wk[b][0], Y[a][1], Wk[b][1], Y[a][2], Wk[b][2]));
                            t[36 + a] = __dadd_rn(t[36 + a], vilf_dot3(Y[a][0], gp[0], Y[a][1], gp[1], Y[a][2], gp[2]));
                        }
                    }
                    const double tot = ba_total<BA_PAIR>(t, s_red + par * 4 * BA_PAIR, tid);
                    par ^= 1;
                    if (tid < 36) {
                        const int a = tid / 6, b = tid % 6;
                        if (a < nj && b < nk && (j != k || a <= b)) {
                            double val = -tot;
                            if (j == k) {
                                const double Uab = s_U[k * 21 + a * 6 - a * (a - 1) / 2 + (b - a)];        // the upper index of (a, b), a <= b
                                val = __dsub_rn(a == b ? __dadd_rn(Uab, __dmul_rn(lam, Uab)) : Uab, tot);
                            }
                            s_S[(oj + a) * BA_MAXC + ok + b] = val;                                      // oj + a, ok + b < nc <= BA_MAXC
                        }
                    } else if (tid < BA_PAIR && j == k && tid - 36 < nk) {
                        s_x[ok + tid - 36] = -__dsub_rn(s_g[k * 6 + tid - 36], tot);
                    }
                }
            }
            __syncthreads();
            // the LDL^T of S in place: d on the diagonal, u above it, L below it
            for (int kk = 0; kk < nc && pos; kk++) {
                const double dk = s_S[kk * BA_MAXC + kk];
                if (!(dk > 0.0)) { pos = false; break; }                                                // the same number in every thread
                for (int i = kk + 1 + tid; i < nc; i += BA_NT) s_S[i * BA_MAXC + kk] = __ddiv_rn(s_S[kk * BA_MAXC + i], dk);
                __syncthreads();
                const int m = nc - kk - 1;
                for (int e = tid; e < m * m; e += BA_NT) {
                    const int jj = kk + 1 + e / m, ii = kk + 1 + e % m;
                    if (ii >= jj) s_S[jj * BA_MAXC + ii] = __dsub_rn(s_S[jj * BA_MAXC + ii], __dmul_rn(s_S[kk * BA_MAXC + ii], s_S[jj * BA_MAXC + kk]));
                }
                __syncthreads();
            }
        }
        if (pos) {
            for (int kk = 0; kk < nc; kk++) {                                                            // y
                const double yk = s_x[kk];
                for (int i = kk + 1 + tid; i < nc; i += BA_NT) s_x[i] = __dsub_rn(s_x[i], __dmul_rn(s_S[i * BA_MAXC + kk], yk));
                __syncthreads();
            }
            for (int i = tid; i < nc; i += BA_NT) s_x[i] = __ddiv_rn(s_x[i], s_S[i * BA_MAXC + i]);      // z
            __syncthreads();
            for (int kk = nc - 1; kk > 0; kk--) {                                                        // x
                const double xk = s_x[kk];
                for (int i = tid; i < kk; i += BA_NT) s_x[i] = __dsub_rn(s_x[i], __dmul_rn(s_S[kk * BA_MAXC + i], xk));
                __syncthreads();
            }
            // the candidate: a frame per thread, then the thread's members
            if (tid < nf) {
                const int k = tid, nk = ba_free(k, l, newest), ok = ba_first(k, l);
                const double *P = s_P + k * 12;
                double *Pn = s_Pn + k * 12;
                if (nk == 0) {
#pragma unroll
                    for (int e = 0; e < 12; e++) Pn[e] = P[e];
                } else {
                    const double a0 = __dmul_rn(0.5, s_x[ok]), a1 = __dmul_rn(0.5, s_x[ok + 1]), a2 = __dmul_rn(0.5, s_x[ok + 2]);
                    const double nq = __dsqrt_rn(__dadd_rn(__dadd_rn(__dadd_rn(1.0, __dmul_rn(a0, a0)), __dmul_rn(a1, a1)), __dmul_rn(a2, a2)));
                    const double qs = __ddiv_rn(1.0, nq), qx = __ddiv_rn(a0, nq), qy = __ddiv_rn(a1, nq), qz = __ddiv_rn(a2, nq);
                    const double xx = __dmul_rn(qx, qx), yy = __dmul_rn(qy, qy), zz = __dmul_rn(qz, qz), xy = __dmul_rn(qx, qy), xz = __dmul_rn(qx, qz), yz = __dmul_rn(qy, qz);
                    const double sx = __dmul_rn(qs, qx), sy = __dmul_rn(qs, qy), sz = __dmul_rn(qs, qz);
                    const double Q[9] = {__dsub_rn(1.0, __dmul_rn(2.0, __dadd_rn(yy, zz))), __dmul_rn(2.0, __dsub_rn(xy, sz)), __dmul_rn(2.0, __dadd_rn(xz, sy)),
                                         __dmul_rn(2.0, __dadd_rn(xy, sz)), __dsub_rn(1.0, __dmul_rn(2.0, __dadd_rn(xx, zz))), __dmul_rn(2.0, __dsub_rn(yz, sx)),
                                         __dmul_rn(2.0, __dsub_rn(xz, sy)), __dmul_rn(2.0, __dadd_rn(yz, sx)), __dsub_rn(1.0, __dmul_rn(2.0, __dadd_rn(xx, yy)))};
#pragma unroll
                    for (int r = 0; r < 3; r++) {
#pragma unroll
                        for (int c = 0; c < 3; c++) Pn[r * 4 + c] = vilf_dot3(Q[r * 3], P[c], Q[r * 3 + 1], P[4 + c], Q[r * 3 + 2], P[8 + c]);
                        Pn[r * 4 + 3] = nk == 6 ? __dadd_rn(P[r * 4 + 3], s_x[ok + 3 + r]) : P[r * 4 + 3];
                    }
                }
            }
            for (int f = tid; f < n; f += BA_NT) {
                if (!s_state[f]) continue;
                const int st = start[f], nobs = first[f + 1] - first[f];
                const double *pt = pts + (size_t)first[f] * 2;
                const double X[3] = {s_pos[3 * f], s_pos[3 * f + 1], s_pos[3 * f + 2]};
                double s[3] = {s_gp[3 * f], s_gp[3 * f + 1], s_gp[3 * f + 2]};
                for (int o = 0; o < nobs; o++) {
                    const int k = st + o, nk = ba_free(k, l, newest), ok = ba_first(k, l);
                    if (nk == 0) continue;
                    double J0[6], J1[6], P0[3], P1[3], e0, e1, W[6][3];
                    ba_obs(s_P + k * 12, X, pt + 2 * o, J0, J1, P0, P1, e0, e1);
                    ba_w(J0, J1, P0, P1, W);
#pragma unroll
                    for (int a = 0; a < 6; a++) {
                        if (a < nk) {
                            const double xa = s_x[ok + a];
#pragma unroll
                            for (int c = 0; c < 3; c++) s[c] = __dadd_rn(s[c], __dmul_rn(W[a][c], xa));
                        }
                    }
                }
                const double *vi = s_vi + 6 * f;
                s_posn[3 * f] = __dadd_rn(X[0], -vilf_dot3(vi[0], s[0], vi[1], s[1], vi[2], s[2]));
                s_posn[3 * f + 1] = __dadd_rn(X[1], -vilf_dot3(vi[1], s[0], vi[3], s[1], vi[4], s[2]));
                s_posn[3 * f + 2] = __dadd_rn(X[2], -vilf_dot3(vi[2], s[0], vi[4], s[1], vi[5], s[2]));
            }
            __syncthreads();
            // the candidate's cost
            double c[BA_MAXF];
#pragma unroll
            for (int k = 0; k < BA_MAXF; k++) c[k] = 0.0;
            for (int f = tid; f < n; f += BA_NT) {
                if (!s_state[f]) continue;
                const int st = start[f], nobs = first[f + 1] - first[f];
                const double *pt = pts + (size_t)first[f] * 2;
                const double X[3] = {s_posn[3 * f], s_posn[3 * f + 1], s_posn[3 * f + 2]};
#pragma unroll
                for (int k = 0; k < BA_MAXF; k++) {
                    const int o = k - st;
                    if (o >= 0 && o < nobs) c[k] = __dadd_rn(c[k], ba_sq(s_Pn + k * 12, X, pt + 2 * o));
                }
            }
            const double tot = ba_total<BA_MAXF>(c, s_red + par * 4 * BA_PAIR, tid);
            par ^= 1;
            if (tid < BA_MAXF) s_ck2[tid] = tot;
            __syncthreads();
            double cn = 0.0;
            for (int k = 0; k < nf; k++) cn = __dadd_rn(cn, s_ck2[k]);
            if (cn < cost) {
                for (int e = tid; e < nf * 12; e += BA_NT) s_P[e] = s_Pn[e];
                for (int f = tid; f < n; f += BA_NT) {
                    if (!s_state[f]) continue;
                    s_pos[3 * f] = s_posn[3 * f]; s_pos[3 * f + 1] = s_posn[3 * f + 1]; s_pos[3 * f + 2] = s_posn[3 * f + 2];
                }
                converged = __dsub_rn(cost, cn) <= __dmul_rn(p.ftol, cost);
                cost = cn; accepted++;
            } else {
                pos = false;
            }
        }
        lam = pos ? __ddiv_rn(lam, 10.0) : __dmul_rn(lam, 10.0);
        __syncthreads();
    }
    // the verdict and the download
    {
        bool fin = true;
        for (int e = tid; e < nf * 12; e += BA_NT) fin = fin && isfinite(s_P[e]);
        for (int f = tid; f < n; f += BA_NT)
            if (s_state[f]) fin = fin && isfinite(s_pos[3 * f]) && isfinite(s_pos[3 * f + 1]) && isfinite(s_pos[3 * f + 2]);
        if (!fin) s_flag[1] = 1;
    }
    __syncthreads();
    if (tid < nf) {
        const double *P = s_P + tid * 12;
        vilf_startup_ba_frame *o = frames + tid;
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) { o->R[r * 3 + c] = P[r * 4 + c]; o->Q[r * 3 + c] = P[c * 4 + r]; }
            o->t[r] = P[r * 4 + 3];
            o->T[r] = -vilf_dot3(P[r], P[3], P[4 + r], P[7], P[8 + r], P[11]);
        }
    }
    for (int f = tid; f < BA_MAXN; f += BA_NT) { state_out[f] = s_state[f]; pos_out[3 * f] = s_pos[3 * f]; pos_out[3 * f + 1] = s_pos[3 * f + 1]; pos_out[3 * f + 2] = s_pos[3 * f + 2]; }
    if (tid == 0) {
        vilf_startup_ba_result r;
        const bool fin = s_flag[1] == 0 && isfinite(cost);
        r.flags = (converged ? VILF_BA_CONVERGED : 0) | (__dmul_rn(0.5, cost) < p.cthr ? VILF_BA_COST : 0) | (fin ? VILF_BA_FINITE : 0);
        r.ok = fin && (r.flags & (VILF_BA_CONVERGED | VILF_BA_COST)) ? 1 : 0;
        r.iterations = iterations; r.accepted = accepted; r.n_camera = nc; r.n_members = n_members; r.n_residuals = n_res; r.l = l;
        r.cost0 = cost0; r.cost1 = cost; r.lambda = lam;
        d.res[w] = r;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
namespace {
// the BA's part of a download: the results, the frames, the state, the positions
struct BaOut { size_t res, frames, state, pos, bytes; };
BaOut ba_out(int W, size_t base) {
    Layout l{base};
    BaOut o;
    o.res = l.take((size_t)W * sizeof(vilf_startup_ba_result)); o.frames = l.take((size_t)W * BA_MAXF * sizeof(vilf_startup_ba_frame)); o.state = l.take((size_t)W * BA_MAXN);
    o.pos = l.take((size_t)W * BA_MAXN * 24); o.bytes = l.at;
    return o;
}
bool ba_pos_fin(double v) { return std::isfinite(v) && v > 0; }
bool ba_params_ok(const vilf_startup_ba_params *p) {
    return p->ba_iterations >= 1 && p->ba_iterations <= 64 && ba_pos_fin(p->lambda0) && ba_pos_fin(p->function_tolerance) && ba_pos_fin(p->cost_threshold);
}
BaPar ba_par(const vilf_startup_ba_params *p) {
    BaPar bp;
    bp.iters = p->ba_iterations; bp.lambda0 = p->lambda0; bp.ftol = p->function_tolerance; bp.cthr = p->cost_threshold;
    return bp;
}
const char *BA_PARAMS_TEXT = ": 1 <= ba_iterations <= 64, a positive finite lambda0, function_tolerance and cost_threshold";
int ba_launch(vilf_handle *h, BaCtx *c, int W, const BaDev &d, const vilf_startup_ba_params *p) {
    if (!c->attr) {
        HIPCHECK(h, hipFuncSetAttribute(reinterpret_cast<const void *>(su_sfm_ba), hipFuncAttributeMaxDynamicSharedMemorySize, (int)BA_LDS_BYTES));
        c->attr = true;
    }
    ProfMarks prof(h, c->prof);
    hipLaunchKernelGGL(su_sfm_ba, dim3(W), dim3(BA_NT), BA_LDS_BYTES, h->stream, d, ba_par(p));
    prof.mark(0);
    HIPCHECK(h, hipGetLastError());
    return VILF_OK;
}
}  // namespace

extern "C" void vilf_startup_default_ba_params(vilf_startup_ba_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->ba_iterations = 20; p->lambda0 = 1e-3; p->function_tolerance = 1e-6; p->cost_threshold = 5e-3;
}

extern "C" int vilf_startup_ba(vilf_handle *h, const vilf_startup_ba_params *p, int n_windows, const vilf_startup_window *windows, const vilf_startup_ba_start *start,
                               vilf_startup_ba_result *out, vilf_startup_ba_frame *frames_out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    if (!p || !windows || !start || !out) { h->err = "vilf_startup_ba: null pointer"; return VILF_ERR_INVALID_ARGUMENT; }
    if (n_windows < 1 || n_windows > VILF_STARTUP_MAX_WINDOWS) { h->err = "vilf_startup_ba: 1 <= n_windows <= VILF_STARTUP_MAX_WINDOWS"; return VILF_ERR_INVALID_ARGUMENT; }
    if (!ba_params_ok(p)) { h->err = std::string("vilf_startup_ba") + BA_PARAMS_TEXT; return VILF_ERR_INVALID_ARGUMENT; }
    size_t total = 0;
    { const int rcw = vilf_startup_check_windows(h, "vilf_startup_ba", n_windows, windows, &total); if (rcw != VILF_OK) return rcw; }
    for (int w = 0; w < n_windows; w++) {
        const vilf_startup_ba_start &s = start[w];
        const vilf_startup_window &Wn = windows[w];
        if (s.l < -1 || s.l > Wn.n_frames - 2) { h->err = "vilf_startup_ba: -1 <= l <= n_frames - 2"; return VILF_ERR_INVALID_ARGUMENT; }
        if (s.l < 0 || !s.chain_ok) continue;
        if (!s.R || !s.t || (Wn.n_features > 0 && (!s.state || !s.positions))) { h->err = "vilf_startup_ba: null pointer in a start"; return VILF_ERR_INVALID_ARGUMENT; }
        bool fin = true;
        for (int e = 0; e < Wn.n_frames * 9; e++) fin = fin && std::isfinite(s.R[e]);
        for (int e = 0; e < Wn.n_frames * 3; e++) fin = fin && std::isfinite(s.t[e]);
        for (int f = 0; f < Wn.n_features; f++) {
            if (s.state[f] > 1) { h->err = "vilf_startup_ba: a state other than 0 / 1"; return VILF_ERR_INVALID_ARGUMENT; }
            if (!s.state[f]) continue;
            if (Wn.first_obs[f + 1] - Wn.first_obs[f] < 2) { h->err = "vilf_startup_ba: a member with fewer than two observations"; return VILF_ERR_INVALID_ARGUMENT; }
            for (int e = 0; e < 3; e++) fin = fin && std::isfinite(s.positions[3 * f + e]);
        }
        if (!fin) { h->err = "vilf_startup_ba: a pose entry or a member's position that is not finite"; return VILF_ERR_INVALID_ARGUMENT; }
    }
    HIPCHECK(h, hipSetDevice(h->device));
    BaCtx *c = vilf_stage_make<BaCtx>(h, ST_BA);
    c->last_windows = 0;
    const int W = n_windows;
    // upload: the windows' integers, l and chain_ok of every window, the poses, the positions, the state, then all points
    Layout li;
    li.take((size_t)W * BA_WIN_INTS * 4, 4);
    const size_t o_l = li.take((size_t)W * 4, 4), o_ok = li.take((size_t)W * 4, 4), o_pose = li.take((size_t)W * BA_MAXF * 96), o_pos = li.take((size_t)W * BA_MAXN * 24, 8),
                 o_state = li.take((size_t)W * BA_MAXN, 1), o_pts = li.take(std::max<size_t>(total, 1) * 16), in_bytes = li.at;
    const BaOut o = ba_out(W, 0);
    if (!c->io.ensure(in_bytes, o.bytes)) { h->err = "vilf_startup_ba: out of memory"; return VILF_ERR_DEVICE; }
    {
        char *ub = (char *)c->io.up.p;
        vilf_startup_pack_windows(W, windows, (int *)ub, (double *)(ub + o_pts));
        int *lw = (int *)(ub + o_l), *okw = (int *)(ub + o_ok);
        double *pose = (double *)(ub + o_pose), *pos = (double *)(ub + o_pos);
        unsigned char *st = (unsigned char *)(ub + o_state);
        std::memset(pose, 0, (size_t)W * BA_MAXF * 96); std::memset(pos, 0, (size_t)W * BA_MAXN * 24); std::memset(st, 0, (size_t)W * BA_MAXN);
        for (int w = 0; w < W; w++) {
            const vilf_startup_ba_start &s = start[w];
            const bool run = s.l >= 0 && s.chain_ok;
            lw[w] = s.l; okw[w] = run ? 1 : 0;
            if (!run) continue;
            for (int k = 0; k < windows[w].n_frames; k++) {
                std::memcpy(pose + ((size_t)w * BA_MAXF + k) * 12, s.R + 9 * k, 72);
                std::memcpy(pose + ((size_t)w * BA_MAXF + k) * 12 + 9, s.t + 3 * k, 24);
            }
            for (int f = 0; f < windows[w].n_features; f++) {
                if (!s.state[f]) continue;
                st[(size_t)w * BA_MAXN + f] = 1;
                std::memcpy(pos + ((size_t)w * BA_MAXN + f) * 3, s.positions + 3 * f, 24);
            }
        }
    }
    HIPCHECK(h, c->io.upload(h, in_bytes));
    BaDev d;
    char *ib = c->io.in.as<char>(), *ob = c->io.out.as<char>();
    d.win = (const int *)ib; d.l = (const int *)(ib + o_l); d.chain_ok = (const int *)(ib + o_ok); d.chain_stride = 1; d.pose = (const double *)(ib + o_pose); d.pose_stride = 12;
    d.pos = (const double *)(ib + o_pos); d.state = (const unsigned char *)(ib + o_state); d.pts = (const double *)(ib + o_pts);
    d.res = (vilf_startup_ba_result *)(ob + o.res); d.frames = (vilf_startup_ba_frame *)(ob + o.frames); d.state_out = (unsigned char *)(ob + o.state); d.pos_out = (double *)(ob + o.pos);
    { const int rcl = ba_launch(h, c, W, d, p); if (rcl != VILF_OK) return rcl; }
    HIPCHECK(h, c->io.download(h, o.bytes));
    const char *hb = (const char *)c->io.down.p;
    std::memcpy(out, hb + o.res, (size_t)W * sizeof(vilf_startup_ba_result));
    if (frames_out) std::memcpy(frames_out, hb + o.frames, (size_t)W * BA_MAXF * sizeof(vilf_startup_ba_frame));
    c->last_windows = W; c->last_state = o.state; c->last_pos = o.pos;
    return VILF_OK;
}

extern "C" int vilf_startup_construct(vilf_handle *h, const vilf_startup_sfm_params *sp, const vilf_startup_ba_params *bp, int n_windows, const vilf_startup_window *windows,
                                      const vilf_startup_result *rel, vilf_startup_ba_result *out, vilf_startup_ba_frame *frames_out, vilf_startup_structure *chain_out,
                                      vilf_startup_frame *chain_frames_out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    if (!sp || !bp || !windows || !rel || !out) { h->err = "vilf_startup_construct: null pointer"; return VILF_ERR_INVALID_ARGUMENT; }
    if (!ba_params_ok(bp)) { h->err = std::string("vilf_startup_construct") + BA_PARAMS_TEXT; return VILF_ERR_INVALID_ARGUMENT; }
    BaCtx *c = vilf_stage_make<BaCtx>(h, ST_BA);
    const int kept = c->last_windows;
    c->last_windows = 0;
    // the chain writes into this call's buffers, the BA's download lies behind the chain's: one copy brings both
    const int W = n_windows;
    VilfSfmQueued q;
    const size_t extra = W >= 1 && W <= VILF_STARTUP_MAX_WINDOWS ? ba_out(W, 0).bytes + 256 : 0;
    { const int rcq = vilf_sfm_enqueue(h, "vilf_startup_construct", sp, n_windows, windows, rel, &c->io, extra, &q); if (rcq != VILF_OK) { if (rcq == VILF_ERR_INVALID_ARGUMENT) c->last_windows = kept; return rcq; } }   // refused: no buffer was touched
    const BaOut o = ba_out(W, q.out_bytes);
    BaDev d;
    char *ob = c->io.out.as<char>();
    d.win = q.win; d.pts = q.pts; d.l = q.l;
    d.chain_ok = (const int *)q.res; d.chain_stride = (int)(sizeof(vilf_startup_structure) / 4);                          // vilf_startup_structure.ok comes first
    d.pose = (const double *)q.rows + offsetof(vilf_startup_frame, R) / 8; d.pose_stride = (int)(sizeof(vilf_startup_frame) / 8);
    d.state = q.state; d.pos = q.pos;
    d.res = (vilf_startup_ba_result *)(ob + o.res); d.frames = (vilf_startup_ba_frame *)(ob + o.frames); d.state_out = (unsigned char *)(ob + o.state); d.pos_out = (double *)(ob + o.pos);
    { const int rcl = ba_launch(h, c, W, d, bp); if (rcl != VILF_OK) return rcl; }
    HIPCHECK(h, c->io.download(h, o.bytes));
    const char *hb = (const char *)c->io.down.p;
    std::memcpy(out, hb + o.res, (size_t)W * sizeof(vilf_startup_ba_result));
    if (frames_out) std::memcpy(frames_out, hb + o.frames, (size_t)W * BA_MAXF * sizeof(vilf_startup_ba_frame));
    if (chain_out) std::memcpy(chain_out, hb + q.o_res, (size_t)W * sizeof(vilf_startup_structure));
    if (chain_frames_out) std::memcpy(chain_frames_out, hb + q.o_rows, (size_t)W * BA_MAXF * sizeof(vilf_startup_frame));
    c->last_windows = W; c->last_state = o.state; c->last_pos = o.pos;
    return VILF_OK;
}
static_assert(offsetof(vilf_startup_structure, ok) == 0 && sizeof(vilf_startup_structure) % 4 == 0, "the BA reads ok at the head of the chain's result");
static_assert(offsetof(vilf_startup_frame, R) % 8 == 0 && offsetof(vilf_startup_frame, t) == offsetof(vilf_startup_frame, R) + 72 && sizeof(vilf_startup_frame) % 8 == 0,
              "the BA reads c_R and c_t of a chain row as twelve doubles");

extern "C" int vilf_startup_get_ba_structure(vilf_handle *h, int n_windows, unsigned char *state_out, double *positions_out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    BaCtx *c = vilf_stage<BaCtx>(h, ST_BA);
    if (!c || c->last_windows < 1 || n_windows != c->last_windows) {
        h->err = "vilf_startup_get_ba_structure: n_windows is not that of the last vilf_startup_ba or vilf_startup_construct"; return VILF_ERR_INVALID_ARGUMENT;
    }
    const char *hb = (const char *)c->io.down.p;
    if (state_out) std::memcpy(state_out, hb + c->last_state, (size_t)n_windows * BA_MAXN);
    if (positions_out) std::memcpy(positions_out, hb + c->last_pos, (size_t)n_windows * BA_MAXN * 24);
    return VILF_OK;
}

extern "C" int vilf_startup_ba_profile(vilf_handle *h, double ms_out[1], long launches_out[1]) { return vilf_stage_profile(h, ST_BA, &BaCtx::prof, ms_out, launches_out); }
