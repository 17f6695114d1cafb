// vilf_pg4.hip — the 4-DoF (yaw + translation) pose graph of the visual loop closure on the device (include/vilfusion.h, "Visual loop closure, third stage").
//   vilf_pg4_optimize ≙ PoseGraph::optimize4DoF (pose_graph/pose_graph.cpp:406-582) with FourDOFError / FourDOFWeightError / AngleLocalParameterization
//   (pose_graph/pose_graph.h:101-250); Ceres's Levenberg-Marquardt restated in the header, the drift (:552-560) on the host.
// The shape is vilf_pg.hip's (chain + Woodbury), with another manifold, another band and another minimiser. Nodes in groups of four (16 unknowns): an edge
// (i - j, i), j <= 4, joins a group to itself or to its neighbour, so the sequential part of H is block tridiagonal in 16 x 16 blocks.
//   pg4_init          one thread per node: yaw, pitch, roll = R2ypr(vio_R), t = vio_T
//   pg4_seq_edges     one thread per sequential edge: rel_t, rel_yaw from the start
//   pg4_linearize     one thread per edge: residual, the two 4 x 4 Jacobian blocks, Huber; used for the state and for the candidate
//   pg4_assemble      one thread per unknown row: its row of the group's diagonal block D, of the coupling block E to the group before, g = J^T r and diag(H)
//                     (loops included), summed over the node's edges in edge order (host-built adjacency: no atomics, fixed order)
//   pg4_chain_factor  one wave: S = D[k] + diag / mu - F[k-1] F[k-1]^T, 16 x 16 Cholesky in LDS (256 entries, four a lane), F[k] = E[k] L^-T, 1 / L_aa
//   pg4_build_rhs / pg4_chain_solve   T^-1 applied to 1 + 4 L right-hand sides (-g and the Jacobian rows of every loop), one thread per column
//   pg4_capacitance   C = I + U T^-1 U^T (4 L x 4 L) and its right-hand side; solved by vilf_lw_chol_solve
//   pg4_step          a wave per unknown row: delta = z - Y C^-1 U z; the candidate state
//   pg4_model         one thread per edge: |J_e delta|^2 at the state
//   pg4_decide        one workgroup: the sums (tree order), rho, accept or reject, the radius, the stop rules, the history row; the LM record lives on the device
// The host reads that record once per attempt (DESIGN.md §3u says why) and flips the state / candidate buffers on an accepted step.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "vilf_internal.hpp"
#include "vilf_device.hpp"

struct Pg4Ctx : VilfStage {
    DBuf in, edges, adj_off, adj_item, loop_f, pr, fixed, x[2], rec[2], D[2], E[2], g[2], dg[2], C, Cinv, F, Y, Cm, w, delta, qe, lm, hist, info, out;
    StageProf<5> prof;
    void profile_reset() override { prof.reset(); }
};

namespace {
using namespace vd;
#define PG4_REC 40                    // per edge: r[4] A[16] B[16] rho pad
#define PG4_NB 16                     // unknowns of a group
struct Pg4Edge { int i, j, loop, pad; double rel_t[3], rel_yaw; };
struct Pg4Lm { double mu, factor, cost, cost0, gmax; int flags, iterations, accepted, pivot_rejections, last, pad; };
struct Pg4Par { double huber, wl, initial_radius, max_radius, min_radius, mrd, ftol, gtol, ptol; };

VD double pg4_norm_angle(double a) { return a > 180.0 ? a - 360.0 : (a < -180.0 ? a + 360.0 : a); }

__global__ void __launch_bounds__(64) pg4_init(int n, int n_pad, const double *vio_R, const double *vio_T, double *x, double *pr) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_pad) return;
    if (k >= n) { x[4 * k] = 0.0; x[4 * k + 1] = 0.0; x[4 * k + 2] = 0.0; x[4 * k + 3] = 0.0; return; }
    double ypr[3];
    R2ypr(vio_R + 9 * (size_t)k, ypr);
    x[4 * k] = ypr[0]; x[4 * k + 1] = vio_T[3 * k]; x[4 * k + 2] = vio_T[3 * k + 1]; x[4 * k + 3] = vio_T[3 * k + 2];
    pr[2 * k] = ypr[1]; pr[2 * k + 1] = ypr[2];
}
__global__ void __launch_bounds__(64) pg4_seq_edges(int nS, Pg4Edge *edges, const double *vio_R, const double *vio_T, const double *x) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nS) return;
    Pg4Edge &ed = edges[e];
    const int i = ed.i, j = ed.j;
    const double d[3] = {vio_T[3 * j] - vio_T[3 * i], vio_T[3 * j + 1] - vio_T[3 * i + 1], vio_T[3 * j + 2] - vio_T[3 * i + 2]};
    double rt[3];
    m3T_vec(vio_R + 9 * (size_t)i, d, rt);
    ed.rel_t[0] = rt[0]; ed.rel_t[1] = rt[1]; ed.rel_t[2] = rt[2];
    ed.rel_yaw = x[4 * j] - x[4 * i];
}
__global__ void __launch_bounds__(64) pg4_linearize(int nE, const Pg4Edge *edges, const double *x, const double *pr, const int *fixed, double huber, double wl, double *rec_all) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nE) return;
    const Pg4Edge ed = edges[f];
    const double *xi = x + 4 * (size_t)ed.i, *xj = x + 4 * (size_t)ed.j;
    const double PI = 3.14159265358979323846;
    const double ypr[3] = {xi[0], pr[2 * ed.i], pr[2 * ed.i + 1]}, pr0[3] = {0.0, ypr[1], ypr[2]};
    double R[9], M[9];
    ypr2R(ypr, R);
    ypr2R(pr0, M);                                                               // R = Rz(yaw) M
    const double d[3] = {xj[1] - xi[1], xj[2] - xi[2], xj[3] - xi[3]};
    const double yr = ypr[0] / 180.0 * PI, cy = cos(yr), sy = sin(yr);
    const double dz[3] = {-sy * d[0] + cy * d[1], -cy * d[0] - sy * d[1], 0.0};    // (d Rz / d yaw)^T d, per radian
    double e[4], dyaw[3], A[16], B[16];
    m3T_vec(R, d, e);
    m3T_vec(M, dz, dyaw);
    const double w = ed.loop ? wl : 1.0;
    for (int k = 0; k < 3; k++) e[k] -= ed.rel_t[k];
    e[3] = w * pg4_norm_angle(xj[0] - xi[0] - ed.rel_yaw);
    for (int k = 0; k < 16; k++) { A[k] = 0.0; B[k] = 0.0; }
    for (int r = 0; r < 3; r++) {
        A[4 * r] = dyaw[r] * (PI / 180.0);
        for (int c = 0; c < 3; c++) { A[4 * r + 1 + c] = -R[3 * c + r]; B[4 * r + 1 + c] = R[3 * c + r]; }
    }
    A[12] = -w; B[12] = w;
    const double s = e[0] * e[0] + e[1] * e[1] + e[2] * e[2] + e[3] * e[3];
    double rho = s;
    if (ed.loop && s > huber * huber) {
        const double rs = sqrt(s), k = sqrt(huber / rs);
        rho = 2.0 * huber * rs - huber * huber;
        for (int q = 0; q < 4; q++) e[q] *= k;
        for (int q = 0; q < 16; q++) { A[q] *= k; B[q] *= k; }
    }
    const bool fi = fixed[ed.i] != 0, fj = fixed[ed.j] != 0;
    double *rec = rec_all + (size_t)f * PG4_REC;
    for (int q = 0; q < 4; q++) rec[q] = e[q];
    for (int q = 0; q < 16; q++) { rec[4 + q] = fi ? 0.0 : A[q]; rec[20 + q] = fj ? 0.0 : B[q]; }
    rec[36] = rho;
}

// adjacency item of a node: edge id | side << 28 (0: the node is the edge's i -> A, 1: j -> B) | kind << 29 (0 sequential, the other node in the same group;
// 1 sequential, the other node in the group before; 2 sequential, the other node in the group after; 3 loop). D and E are zero on entry.
__global__ void __launch_bounds__(64) pg4_assemble(int NG, const int *adj_off, const int *adj_item, const Pg4Edge *edges, const double *rec_all, const int *fixed, double *D, double *E,
                             double *g, double *dg) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= PG4_NB * NG) return;
    const int G = row / PG4_NB, q = row % PG4_NB, a = q / 4, c = q % 4, k = 4 * G + a;
    double *Dp = D + (size_t)G * 256 + q * 16;
    double gs = 0.0, ds = 0.0;
    if (fixed[k]) { Dp[q] = 1.0; g[row] = 0.0; dg[row] = 0.0; return; }      // a fixed (or padding) node: identity block, no coupling, no gradient
    for (int it = adj_off[k]; it < adj_off[k + 1]; it++) {
        const int item = adj_item[it], f = item & 0x0fffffff, side = (item >> 28) & 1, kind = (item >> 29) & 3;
        const double *rec = rec_all + (size_t)f * PG4_REC;
        const double *J = rec + (side ? 20 : 4), *Jo = rec + (side ? 4 : 20);
        const double j0 = J[c], j1 = J[4 + c], j2 = J[8 + c], j3 = J[12 + c];
        gs += j0 * rec[0] + j1 * rec[1] + j2 * rec[2] + j3 * rec[3];
        ds += j0 * j0 + j1 * j1 + j2 * j2 + j3 * j3;
        if (kind == 3) continue;
        for (int b = 0; b < 4; b++) Dp[4 * a + b] += j0 * J[b] + j1 * J[4 + b] + j2 * J[8 + b] + j3 * J[12 + b];
        if (kind == 2) continue;
        const int other = side ? edges[f].i : edges[f].j, ao = other & 3;
        double *P = (kind == 0 ? Dp : E + (size_t)(G - 1) * 256 + q * 16) + 4 * ao;      // kind 1 only occurs with G >= 1 (host)
        for (int b = 0; b < 4; b++) P[b] += j0 * Jo[b] + j1 * Jo[4 + b] + j2 * Jo[8 + b] + j3 * Jo[12 + b];
    }
    g[row] = gs; dg[row] = ds;
}

// block Cholesky of the chain. E[k] (rows: group k + 1, columns: group k). One wave, entry e = lane + 64 q of a 16 x 16 block, (a, b) = (e / 16, e % 16). Only the
// lower triangle of S is kept. A column step reads (pivot, column, the entries it updates), then writes, with one barrier between and one after: the scaled column
// and the updated trailing entries are disjoint. Cinv [16 NG] = 1 / L_aa: the solves multiply by it (a dependent fp64 division is the longest operation there is).
__global__ void __launch_bounds__(64) pg4_chain_factor(int NG, const double *__restrict__ D, const double *__restrict__ E, const double *__restrict__ dg, const Pg4Lm *__restrict__ lm,
                                                       double *__restrict__ C, double *__restrict__ Cinv, double *__restrict__ F, int *status) {
    __shared__ double sS[256], sF[256], sInv[16];
    const int lane = threadIdx.x;
    const double inv_mu = 1.0 / lm->mu;
#pragma unroll
    for (int q = 0; q < 4; q++) sF[lane + 64 * q] = 0.0;
    __syncthreads();
    for (int k = 0; k < NG; k++) {
        const double *Dk = D + (size_t)k * 256, *Ek = E + (size_t)k * 256;
        double y[16];
        if (lane < 16 && k + 1 < NG) {                                          // row `lane` of E[k], in flight during the factorisation
#pragma unroll
            for (int c = 0; c < 16; c++) y[c] = Ek[16 * lane + c];
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int e = lane + 64 * q, a = e >> 4, b = e & 15;
            double v = 0.0;
            if (b <= a) {
                double s = 0.0;
#pragma unroll
                for (int r = 0; r < 16; r++) s += sF[16 * a + r] * sF[16 * b + r];
                v = Dk[e] - s;
                if (a == b) v += dg[16 * k + a] * inv_mu;
            }
            sS[e] = v;
        }
        __syncthreads();
        bool ok = true;
        for (int j = 0; j < 16; j++) {
            const double piv = sS[17 * j];                                     // the same value in every lane: the branch is uniform
            if (!(piv > 0.0)) { ok = false; break; }
            const double l = sqrt(piv), inv = 1.0 / l;
            double nv[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int e = lane + 64 * q, a = e >> 4, b = e & 15;
                nv[q] = (a > j && b > j && b <= a) ? sS[e] - (sS[16 * a + j] * inv) * (sS[16 * b + j] * inv) : 0.0;
            }
            const double colv = (lane > j && lane < 16) ? sS[16 * lane + j] * inv : l;
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int e = lane + 64 * q, a = e >> 4, b = e & 15;
                if (a > j && b > j && b <= a) sS[e] = nv[q];
            }
            if (lane >= j && lane < 16) sS[16 * lane + j] = colv;
            if (lane == 0) sInv[j] = inv;
            __syncthreads();
        }
        if (!ok) { if (lane == 0) *status = 1; return; }
#pragma unroll
        for (int q = 0; q < 4; q++) { const int e = lane + 64 * q; C[(size_t)k * 256 + e] = sS[e]; }      // the upper triangle is zero (S was built so)
        if (lane < 16) Cinv[16 * (size_t)k + lane] = sInv[lane];
        if (k + 1 < NG) {
            if (lane < 16) {                                                    // y L^T = E(lane, :), column by column in the lane's registers
#pragma unroll
                for (int c = 0; c < 16; c++) {
                    y[c] *= sInv[c];
#pragma unroll
                    for (int r = c + 1; r < 16; r++) y[r] -= y[c] * sS[16 * r + c];
                }
#pragma unroll
                for (int c = 0; c < 16; c++) sF[16 * lane + c] = y[c];
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; q++) F[(size_t)k * 256 + lane + 64 * q] = sF[lane + 64 * q];
        }
        __syncthreads();
    }
}

// Y [16 NG][NC] row-major, zero on entry: column 0 = -g, column 1 + 4 l + r = row r of loop l's Jacobian
__global__ void __launch_bounds__(256) pg4_build_rhs(int NG, int L, int NC, const int *loop_f, const Pg4Edge *edges, const double *rec_all, const double *g, double *Y) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < PG4_NB * NG) Y[(size_t)t * NC] = -g[t];
    if (t < 16 * L) {
        const int l = t / 16, r = (t % 16) / 4, c = t % 4, f = loop_f[l];
        const double *rec = rec_all + (size_t)f * PG4_REC;
        Y[(size_t)(4 * edges[f].i + c) * NC + 1 + 4 * l + r] = rec[4 + 4 * r + c];
        Y[(size_t)(4 * edges[f].j + c) * NC + 1 + 4 * l + r] = rec[20 + 4 * r + c];
    }
}
// a lane per column. The triangular solves run column by column (after b[a] is final, every later entry takes its share): the dependent chain is 16 steps, not 136.
// C, Cinv and F are the same for every lane and never written here: scalar loads.
__global__ void __launch_bounds__(64) pg4_chain_solve(int NG, int NC, const double *__restrict__ C, const double *__restrict__ Cinv, const double *__restrict__ F, double *__restrict__ Y) {
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= NC) return;
    double b[16], prev[16];
#pragma unroll
    for (int a = 0; a < 16; a++) prev[a] = 0.0;
    for (int k = 0; k < NG; k++) {
#pragma unroll
        for (int a = 0; a < 16; a++) b[a] = Y[(size_t)(16 * k + a) * NC + col];
        if (k > 0) {
            const double *Fk = F + (size_t)(k - 1) * 256;
#pragma unroll
            for (int r = 0; r < 16; r++) {
#pragma unroll
                for (int a = 0; a < 16; a++) b[a] -= Fk[16 * a + r] * prev[r];
            }
        }
        const double *Ck = C + (size_t)k * 256, *Ik = Cinv + (size_t)k * 16;
#pragma unroll
        for (int a = 0; a < 16; a++) {
            b[a] *= Ik[a];
#pragma unroll
            for (int r = a + 1; r < 16; r++) b[r] -= Ck[16 * r + a] * b[a];
        }
#pragma unroll
        for (int a = 0; a < 16; a++) { Y[(size_t)(16 * k + a) * NC + col] = b[a]; prev[a] = b[a]; }
    }
    for (int k = NG - 1; k >= 0; k--) {
#pragma unroll
        for (int a = 0; a < 16; a++) b[a] = Y[(size_t)(16 * k + a) * NC + col];
        if (k + 1 < NG) {
            const double *Fk = F + (size_t)k * 256;
#pragma unroll
            for (int r = 0; r < 16; r++) {
#pragma unroll
                for (int a = 0; a < 16; a++) b[a] -= Fk[16 * r + a] * prev[r];
            }
        }
        const double *Ck = C + (size_t)k * 256, *Ik = Cinv + (size_t)k * 16;
#pragma unroll
        for (int a = 15; a >= 0; a--) {
            b[a] *= Ik[a];
#pragma unroll
            for (int r = 0; r < a; r++) b[r] -= Ck[16 * a + r] * b[a];
        }
#pragma unroll
        for (int a = 0; a < 16; a++) { Y[(size_t)(16 * k + a) * NC + col] = b[a]; prev[a] = b[a]; }
    }
}
// capacitance matrix Cm = I + sym(U Y) (NL x NL) and rhs = U z, rhs stored as row NL of Cm
__global__ void __launch_bounds__(256) pg4_capacitance(int L, int NC, const int *loop_f, const Pg4Edge *edges, const double *rec_all, const double *Y, double *Cm) {
    const int NL = 4 * L;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)NL * (NL + 1)) return;
    const int a = (int)(t / (NL + 1)), b = (int)(t % (NL + 1));
    auto udot = [&](int row, int col) {                       // U row `row` . Y column `col`
        const int l = row / 4, r = row % 4, f = loop_f[l];
        const double *rec = rec_all + (size_t)f * PG4_REC;
        const int i = edges[f].i, j = edges[f].j;
        double s = 0.0;
        for (int c = 0; c < 4; c++) s += rec[4 + 4 * r + c] * Y[(size_t)(4 * i + c) * NC + col] + rec[20 + 4 * r + c] * Y[(size_t)(4 * j + c) * NC + col];
        return s;
    };
    if (b == NL) { Cm[(size_t)NL * NL + a] = udot(a, 0); return; }
    Cm[(size_t)b * NL + a] = 0.5 * (udot(a, 1 + b) + udot(b, 1 + a)) + (a == b ? 1.0 : 0.0);
}
// a wave per row: the lanes stride over the 4 L products, the wave sums them in its fixed tree
__global__ void __launch_bounds__(64) pg4_step(int rows, int NC, int NL, const double *Y, const double *w, const double *x, const int *fixed, double *delta, double *xc) {
    const int row = blockIdx.x, lane = threadIdx.x;                             // the grid is `rows` workgroups
    if (fixed[row / 4]) { if (lane == 0) { delta[row] = 0.0; xc[row] = x[row]; } return; }      // uniform over the wave
    const double *y = Y + (size_t)row * NC;
    double part = 0.0;
    for (int b = lane; b < NL; b += 64) part += y[1 + b] * w[b];
    const double s = y[0] - vilf_wave_sum64(part);
    if (lane != 0) return;
    delta[row] = s;
    xc[row] = (row % 4 == 0) ? pg4_norm_angle(x[row] + s) : x[row] + s;
}
__global__ void __launch_bounds__(64) pg4_model(int nE, const Pg4Edge *edges, const double *rec_all, const double *delta, double *qe) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nE) return;
    const double *rec = rec_all + (size_t)f * PG4_REC, *di = delta + 4 * (size_t)edges[f].i, *dj = delta + 4 * (size_t)edges[f].j;
    double q = 0.0;
    for (int r = 0; r < 4; r++) {
        double s = 0.0;
        for (int c = 0; c < 4; c++) s += rec[4 + 4 * r + c] * di[c] + rec[20 + 4 * r + c] * dj[c];
        q += s * s;
    }
    qe[f] = q;
}

// sum (or maximum) over the workgroup in a fixed tree order; the result in every thread
template <bool MAX> __device__ __forceinline__ double pg4_block_reduce(double v, double *s) {
    const int t = threadIdx.x;
    __syncthreads();
    s[t] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) s[t] = MAX ? fmax(s[t], s[t + w]) : s[t] + s[t + w];
        __syncthreads();
    }
    return s[0];
}
// first != 0: the record at the start from the state's rec_new and g_new. Otherwise the decision on the attempt: rec_new, g_new are the candidate's; qe, delta, g, x
// the state's. status[0]: the chain's pivots, status[4]: the dense Cholesky's.
__global__ void __launch_bounds__(256) pg4_decide(int first, int nE, int rows, const double *rec_new, const double *g_new, const double *qe, const double *delta,
                                                   const double *g, const double *x, const int *fixed, const int *status, Pg4Par par, Pg4Lm *lm, double *hist) {
    __shared__ double s[256];
    const int t = threadIdx.x;
    double cost = 0.0, gmax = 0.0, q = 0.0, dg = 0.0, dd = 0.0, xx = 0.0;
    for (int f = t; f < nE; f += 256) cost += rec_new[(size_t)f * PG4_REC + 36];
    for (int r = t; r < rows; r += 256) gmax = fmax(gmax, fabs(g_new[r]));
    cost = 0.5 * pg4_block_reduce<false>(cost, s);
    gmax = pg4_block_reduce<true>(gmax, s);
    if (!first) {
        for (int f = t; f < nE; f += 256) q += qe[f];
        for (int r = t; r < rows; r += 256) if (!fixed[r / 4]) { dg += delta[r] * g[r]; dd += delta[r] * delta[r]; xx += x[r] * x[r]; }
        q = pg4_block_reduce<false>(q, s); dg = pg4_block_reduce<false>(dg, s); dd = pg4_block_reduce<false>(dd, s); xx = pg4_block_reduce<false>(xx, s);
    }
    if (t != 0) return;
    if (first) {
        lm->mu = par.initial_radius; lm->factor = 2.0; lm->cost = cost; lm->cost0 = cost; lm->gmax = gmax;
        lm->flags = gmax <= par.gtol ? VILF_PG4_GRADIENT : 0;
        lm->iterations = 0; lm->accepted = 0; lm->pivot_rejections = 0; lm->last = 0; lm->pad = 0;
        return;
    }
    const int it = lm->iterations;
    const double mu = lm->mu, cost_old = lm->cost;
    const bool ok = !status[0] && !status[4] && isfinite(cost);
    double rho = 0.0;
    bool acc = false;
    if (ok) { const double model = -(dg + 0.5 * q); rho = (cost_old - cost) / model; acc = rho > par.mrd; }
    else lm->pivot_rejections++;
    double *hr = hist + 5 * it;
    hr[0] = cost_old; hr[1] = ok ? cost : cost_old; hr[2] = rho; hr[3] = mu; hr[4] = ok ? (acc ? 1.0 : 0.0) : -1.0;
    lm->iterations = it + 1;
    lm->last = acc ? 1 : 0;
    if (acc) {
        const double u = 2.0 * rho - 1.0;
        int flags = 0;
        lm->accepted++;
        lm->mu = fmin(mu / fmax(1.0 / 3.0, 1.0 - u * u * u), par.max_radius);
        lm->factor = 2.0;
        if (cost_old - cost <= par.ftol * cost_old) flags |= VILF_PG4_FUNCTION;
        if (gmax <= par.gtol) flags |= VILF_PG4_GRADIENT;
        if (sqrt(dd) <= par.ptol * (sqrt(xx) + par.ptol)) flags |= VILF_PG4_PARAMETER;
        lm->cost = cost; lm->gmax = gmax; lm->flags = flags;
    } else {
        lm->mu = mu / lm->factor;
        lm->factor *= 2.0;
        if (lm->mu < par.min_radius) lm->flags = VILF_PG4_RADIUS;
    }
}
// out [n][15]: t, (yaw, pitch, roll), R = ypr2R of it
__global__ void __launch_bounds__(64) pg4_finish(int n, const double *x, const double *pr, double *out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    double *o = out + 15 * (size_t)k;
    const double ypr[3] = {x[4 * k], pr[2 * k], pr[2 * k + 1]};
    double R[9];
    ypr2R(ypr, R);
    o[0] = x[4 * k + 1]; o[1] = x[4 * k + 2]; o[2] = x[4 * k + 3];
    o[3] = ypr[0]; o[4] = ypr[1]; o[5] = ypr[2];
    for (int q = 0; q < 9; q++) o[6 + q] = R[q];
}
bool pos_finite(double v) { return std::isfinite(v) && v > 0.0; }
bool nonneg_finite(double v) { return std::isfinite(v) && v >= 0.0; }
}  // namespace

extern "C" void vilf_pg4_default_params(vilf_pg4_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->max_iterations = 5;
    p->initial_radius = 1e4; p->max_radius = 1e16; p->min_radius = 1e-32;
    p->min_relative_decrease = 1e-3;
    p->function_tolerance = 1e-6; p->gradient_tolerance = 1e-10; p->parameter_tolerance = 1e-8;
    p->huber = 0.1; p->loop_yaw_scale = 0.1;
}

extern "C" int vilf_pg4_optimize(vilf_handle *h, const vilf_pg4_params *p, int n, const double *vio_R, const double *vio_T, const int *sequence, const int *fixed,
                                 int n_loops, const vilf_pg4_loop *loops, double *t_out, double *ypr_out, double *R_out, vilf_pg4_result *result, double *history_out) {
    if (!h) return VILF_ERR_INVALID_ARGUMENT;
    if (!p || !vio_R || !vio_T || !sequence || !fixed || !t_out || !ypr_out || !R_out || !result || n_loops < 0 || (n_loops && !loops)) { h->err = "pg4: null argument"; return VILF_ERR_INVALID_ARGUMENT; }
    if (n < 1 || n >= (1 << 26) || !fixed[0]) { h->err = "pg4: n < 1 or node 0 not fixed"; return VILF_ERR_INVALID_ARGUMENT; }
    if (p->max_iterations < 0 || p->max_iterations > VILF_PG4_MAX_ITERATIONS_LIMIT || !pos_finite(p->initial_radius) || !pos_finite(p->max_radius) || !pos_finite(p->min_radius) ||
        !pos_finite(p->huber) || !pos_finite(p->loop_yaw_scale) || !nonneg_finite(p->min_relative_decrease) || !nonneg_finite(p->function_tolerance) ||
        !nonneg_finite(p->gradient_tolerance) || !nonneg_finite(p->parameter_tolerance)) { h->err = "pg4: parameter out of range"; return VILF_ERR_INVALID_ARGUMENT; }
    for (size_t k = 0; k < (size_t)n * 9; k++) if (!std::isfinite(vio_R[k])) { h->err = "pg4: vio_R not finite"; return VILF_ERR_INVALID_ARGUMENT; }
    for (size_t k = 0; k < (size_t)n * 3; k++) if (!std::isfinite(vio_T[k])) { h->err = "pg4: vio_T not finite"; return VILF_ERR_INVALID_ARGUMENT; }
    for (int l = 0; l < n_loops; l++) {
        const vilf_pg4_loop &s = loops[l];
        if (s.from < 0 || s.from >= s.to || s.to >= n) { h->err = "pg4: loop endpoints out of range"; return VILF_ERR_INVALID_ARGUMENT; }
        if (!std::isfinite(s.rel_t[0]) || !std::isfinite(s.rel_t[1]) || !std::isfinite(s.rel_t[2]) || !std::isfinite(s.rel_yaw)) { h->err = "pg4: loop not finite"; return VILF_ERR_INVALID_ARGUMENT; }
    }
    const int L = n_loops, NL = 4 * L, NC = 1 + NL;
    if ((long)NL > (long)vilf_lw_chol_max_n()) {       // before anything is uploaded or enqueued: the capacitance block (4 L x 4 L) goes through vilf_lw_chol_solve
        h->err = "pg4: " + std::to_string(L) + " loops; the dense capacitance block supports " + std::to_string(vilf_lw_chol_max_n() / 4);
        return VILF_ERR_UNSUPPORTED;
    }
    HIPCHECK(h, hipSetDevice(h->device));
    Pg4Ctx *c = vilf_stage_make<Pg4Ctx>(h, ST_PG4);
    // ---- host: the edge list (sequential edges of node 0, 1, ..., then the loops), the nodes' adjacency in that order, the padded fixed flags
    const int NG = (n + 3) / 4, n_pad = 4 * NG, rows = PG4_NB * NG;
    std::vector<Pg4Edge> ed;
    std::vector<std::vector<int>> adj(n);
    auto link = [&](int i, int j, int f, bool loop) {
        const int gi = i / 4, gj = j / 4;                                        // i < j: gj == gi or gi + 1 for a sequential edge
        adj[i].push_back(f | (0 << 28) | ((loop ? 3 : (gi == gj ? 0 : 2)) << 29));
        adj[j].push_back(f | (1 << 28) | ((loop ? 3 : (gi == gj ? 0 : 1)) << 29));
    };
    for (int i = 0; i < n; i++) for (int j = 1; j <= VILF_PG4_BAND; j++) if (i - j >= 0 && sequence[i] == sequence[i - j]) {
        Pg4Edge e{}; e.i = i - j; e.j = i; e.loop = 0;
        link(e.i, e.j, (int)ed.size(), false); ed.push_back(e);
    }
    const int nS = (int)ed.size();
    std::vector<int> loop_f(std::max(L, 1), 0);
    for (int l = 0; l < L; l++) {
        Pg4Edge e{}; e.i = loops[l].from; e.j = loops[l].to; e.loop = 1;
        std::memcpy(e.rel_t, loops[l].rel_t, 24); e.rel_yaw = loops[l].rel_yaw;
        loop_f[l] = (int)ed.size();
        link(e.i, e.j, loop_f[l], true); ed.push_back(e);
    }
    const int nE = (int)ed.size();
    if (ed.empty()) ed.push_back(Pg4Edge{});
    std::vector<int> adj_off(n_pad + 1, 0), adj_item, fx(n_pad, 1);
    for (int k = 0; k < n_pad; k++) {
        adj_off[k + 1] = adj_off[k] + (k < n ? (int)adj[k].size() : 0);
        if (k < n) { adj_item.insert(adj_item.end(), adj[k].begin(), adj[k].end()); fx[k] = fixed[k] ? 1 : 0; }
    }
    if (adj_item.empty()) adj_item.push_back(0);
    const size_t sG = (size_t)NG, sR = (size_t)rows, in_R = (size_t)n * 72, in_T = (size_t)n * 24, nEa = std::max<size_t>(nE, 1);
    const int max_it = p->max_iterations;
    bool okm = c->in.ensure(in_R + in_T) && c->edges.ensure(ed.size() * sizeof(Pg4Edge)) && c->adj_off.ensure(adj_off.size() * 4) && c->adj_item.ensure(adj_item.size() * 4) &&
               c->loop_f.ensure(loop_f.size() * 4) && c->pr.ensure((size_t)n_pad * 16) && c->fixed.ensure((size_t)n_pad * 4) && c->C.ensure(sG * 2048) && c->Cinv.ensure(sG * 128) && c->F.ensure(sG * 2048) &&
               c->Y.ensure(sR * NC * 8) && c->Cm.ensure(std::max<size_t>((size_t)(NL + 1) * NL, 1) * 8) && c->w.ensure(std::max(NL, 1) * 8) && c->delta.ensure(sR * 8) &&
               c->qe.ensure(nEa * 8) && c->lm.ensure(sizeof(Pg4Lm)) && c->hist.ensure(VILF_PG4_MAX_ITERATIONS_LIMIT * 40) && c->info.ensure(64) && c->out.ensure((size_t)n * 120);
    for (int s = 0; s < 2 && okm; s++)
        okm = c->x[s].ensure(sR * 8) && c->rec[s].ensure(nEa * PG4_REC * 8) && c->D[s].ensure(sG * 2048) && c->E[s].ensure(sG * 2048) && c->g[s].ensure(sR * 8) && c->dg[s].ensure(sR * 8);
    if (!okm) { h->err = "hipMalloc failed (4-DoF pose graph)"; return VILF_ERR_DEVICE; }
    ProfMarks<5> prof(h, c->prof);
    double *d_R = c->in.as<double>(), *d_T = d_R + (size_t)n * 9;
    HIPCHECK(h, hipMemcpyAsync(d_R, vio_R, in_R, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(h, hipMemcpyAsync(d_T, vio_T, in_T, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(h, hipMemcpyAsync(c->edges.p, ed.data(), ed.size() * sizeof(Pg4Edge), hipMemcpyHostToDevice, h->stream));
    HIPCHECK(h, hipMemcpyAsync(c->adj_off.p, adj_off.data(), adj_off.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(h, hipMemcpyAsync(c->adj_item.p, adj_item.data(), adj_item.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(h, hipMemcpyAsync(c->loop_f.p, loop_f.data(), loop_f.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(h, hipMemcpyAsync(c->fixed.p, fx.data(), fx.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(h, hipStreamSynchronize(h->stream));                                // the uploads read pageable host vectors of this call
    Pg4Edge *d_ed = c->edges.as<Pg4Edge>();
    const int *d_fixed = c->fixed.as<int>(), *d_adj_off = c->adj_off.as<int>(), *d_adj_item = c->adj_item.as<int>(), *d_loop_f = c->loop_f.as<int>();
    int *d_info = c->info.as<int>();
    double *d_pr = c->pr.as<double>(), *d_hist = c->hist.as<double>(), *d_delta = c->delta.as<double>(), *d_qe = c->qe.as<double>(), *Y = c->Y.as<double>();
    Pg4Lm *d_lm = c->lm.as<Pg4Lm>();
    Pg4Par par{p->huber, p->loop_yaw_scale, p->initial_radius, p->max_radius, p->min_radius, p->min_relative_decrease, p->function_tolerance, p->gradient_tolerance, p->parameter_tolerance};
    auto grid = [](size_t items, int block) { return dim3((unsigned)std::max<size_t>((items + block - 1) / block, 1)); };
    auto linearize = [&](int s) -> hipError_t {                                // rec, D, E, g, diag(H) of buffer set s from its x
        if (nE) hipLaunchKernelGGL(pg4_linearize, grid(nE, 64), dim3(64), 0, h->stream, nE, d_ed, c->x[s].as<double>(), d_pr, d_fixed, par.huber, par.wl, c->rec[s].as<double>());
        hipError_t e = hipMemsetAsync(c->D[s].p, 0, sG * 2048, h->stream);
        if (e == hipSuccess) e = hipMemsetAsync(c->E[s].p, 0, sG * 2048, h->stream);
        hipLaunchKernelGGL(pg4_assemble, grid(rows, 64), dim3(64), 0, h->stream, NG, d_adj_off, d_adj_item, d_ed, c->rec[s].as<double>(), d_fixed, c->D[s].as<double>(),
                           c->E[s].as<double>(), c->g[s].as<double>(), c->dg[s].as<double>());
        return e;
    };
    Pg4Lm lm;
    int cur = 0;
    hipLaunchKernelGGL(pg4_init, grid(n_pad, 64), dim3(64), 0, h->stream, n, n_pad, d_R, d_T, c->x[0].as<double>(), d_pr);
    if (nS) hipLaunchKernelGGL(pg4_seq_edges, grid(nS, 64), dim3(64), 0, h->stream, nS, d_ed, d_R, d_T, c->x[0].as<double>());
    HIPCHECK(h, linearize(0));
    HIPCHECK(h, hipMemsetAsync(d_info, 0, 64, h->stream));
    hipLaunchKernelGGL(pg4_decide, dim3(1), dim3(256), 0, h->stream, 1, nE, rows, c->rec[0].as<double>(), c->g[0].as<double>(), d_qe, d_delta, c->g[0].as<double>(),
                       c->x[0].as<double>(), d_fixed, d_info, par, d_lm, d_hist);
    HIPCHECK(h, hipGetLastError());
    HIPCHECK(h, vilf_copy_sync(h, &lm, d_lm, sizeof(lm), hipMemcpyDeviceToHost));
    prof.mark(0);
    while (!lm.flags && lm.iterations < max_it) {
        const int s = cur, t = cur ^ 1;
        HIPCHECK(h, hipMemsetAsync(d_info, 0, 64, h->stream));
        hipLaunchKernelGGL(pg4_chain_factor, dim3(1), dim3(64), 0, h->stream, NG, c->D[s].as<double>(), c->E[s].as<double>(), c->dg[s].as<double>(), d_lm, c->C.as<double>(),
                           c->Cinv.as<double>(), c->F.as<double>(), d_info);
        HIPCHECK(h, hipMemsetAsync(Y, 0, sR * NC * 8, h->stream));
        hipLaunchKernelGGL(pg4_build_rhs, grid(std::max(rows, 16 * L), 256), dim3(256), 0, h->stream, NG, L, NC, d_loop_f, d_ed, c->rec[s].as<double>(), c->g[s].as<double>(), Y);
        hipLaunchKernelGGL(pg4_chain_solve, grid(NC, 64), dim3(64), 0, h->stream, NG, NC, c->C.as<double>(), c->Cinv.as<double>(), c->F.as<double>(), Y);
        prof.mark(1);
        if (L > 0) {
            hipLaunchKernelGGL(pg4_capacitance, grid((size_t)NL * (NL + 1), 256), dim3(256), 0, h->stream, L, NC, d_loop_f, d_ed, c->rec[s].as<double>(), Y, c->Cm.as<double>());
            const int rcs = vilf_lw_chol_solve(h, NL, c->Cm.as<double>(), c->w.as<double>(), d_info + 4);
            if (rcs != VILF_OK) return rcs;
        }
        prof.mark(2);
        hipLaunchKernelGGL(pg4_step, dim3(rows), dim3(64), 0, h->stream, rows, NC, NL, Y, c->w.as<double>(), c->x[s].as<double>(), d_fixed, d_delta, c->x[t].as<double>());
        if (nE) hipLaunchKernelGGL(pg4_model, grid(nE, 64), dim3(64), 0, h->stream, nE, d_ed, c->rec[s].as<double>(), d_delta, d_qe);
        HIPCHECK(h, linearize(t));
        hipLaunchKernelGGL(pg4_decide, dim3(1), dim3(256), 0, h->stream, 0, nE, rows, c->rec[t].as<double>(), c->g[t].as<double>(), d_qe, d_delta, c->g[s].as<double>(),
                           c->x[s].as<double>(), d_fixed, d_info, par, d_lm, d_hist);
        HIPCHECK(h, hipGetLastError());
        HIPCHECK(h, vilf_copy_sync(h, &lm, d_lm, sizeof(lm), hipMemcpyDeviceToHost));
        prof.mark(3);
        if (lm.last) cur = t;
    }
    if (!lm.flags) lm.flags = VILF_PG4_MAX_ITERATIONS;
    hipLaunchKernelGGL(pg4_finish, grid(n, 64), dim3(64), 0, h->stream, n, c->x[cur].as<double>(), d_pr, c->out.as<double>());
    HIPCHECK(h, hipGetLastError());
    std::vector<double> out((size_t)n * 15), hist((size_t)std::max(lm.iterations, 1) * 5);
    if (lm.iterations) HIPCHECK(h, hipMemcpyAsync(hist.data(), d_hist, (size_t)lm.iterations * 40, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(h, vilf_copy_sync(h, out.data(), c->out.p, out.size() * 8, hipMemcpyDeviceToHost));
    prof.mark(4);
    bool finite = std::isfinite(lm.cost) && std::isfinite(lm.mu);
    for (size_t k = 0; k < out.size(); k++) finite = finite && std::isfinite(out[k]);
    for (int k = 0; k < n; k++) {
        std::memcpy(t_out + 3 * (size_t)k, &out[15 * (size_t)k], 24);
        std::memcpy(ypr_out + 3 * (size_t)k, &out[15 * (size_t)k + 3], 24);
        std::memcpy(R_out + 9 * (size_t)k, &out[15 * (size_t)k + 6], 72);
    }
    if (history_out && lm.iterations) std::memcpy(history_out, hist.data(), (size_t)lm.iterations * 40);
    std::memset(result, 0, sizeof(*result));
    result->iterations = lm.iterations; result->accepted = lm.accepted; result->pivot_rejections = lm.pivot_rejections;
    result->flags = lm.flags | (finite ? VILF_PG4_FINITE : 0);
    result->cost0 = lm.cost0; result->cost1 = lm.cost; result->radius = lm.mu;
    // the drift of the last node (pose_graph.cpp:552-560), fp64 on the host
    const double PI = 3.14159265358979323846;
    const double *Ro = R_out + 9 * (size_t)(n - 1), *Rv = vio_R + 9 * (size_t)(n - 1), *Tv = vio_T + 3 * (size_t)(n - 1), *To = t_out + 3 * (size_t)(n - 1);
    const double yd = std::atan2(Ro[3], Ro[0]) * 180.0 / PI - std::atan2(Rv[3], Rv[0]) * 180.0 / PI, a = yd / 180.0 * PI, cs = std::cos(a), sn = std::sin(a);
    const double rd[9] = {cs, -sn, 0.0, sn, cs, 0.0, 0.0, 0.0, 1.0};
    result->yaw_drift = yd;
    std::memcpy(result->r_drift, rd, 72);
    for (int r = 0; r < 3; r++) result->t_drift[r] = To[r] - (rd[3 * r] * Tv[0] + rd[3 * r + 1] * Tv[1] + rd[3 * r + 2] * Tv[2]);
    return VILF_OK;
}

extern "C" int vilf_pg4_profile(vilf_handle *h, double ms_out[5], long launches_out[5]) { return vilf_stage_profile(h, ST_PG4, &Pg4Ctx::prof, ms_out, launches_out); }
