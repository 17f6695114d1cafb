// vilf_pnp.hpp — the device functions of the fixed-iteration Levenberg-Marquardt PnP that the visual start-up (vilf_sfm.hip, solveFrameByPnP) and the visual loop
//   closure (vilf_kfloop.hip, PnPRANSAC) share. The arithmetic is stated once, in include/vilfusion.h ("Visual start-up: GlobalSFM frame chain", paragraph
//   solveFrameByPnP); the loop closure's text refers to it. Every operation is an explicitly rounded intrinsic, so nothing contracts wherever a piece is inlined.
//     sf_residual, sf_add_terms, sf_solve, sf_candidate   one member's residual and 28 terms, the damped 6 x 6 LDL^T, the candidate pose: a lane's own registers
//     sf_total, sf_cost, sf_pnp                           the workgroup forms: SF_NT threads, members in LDS, 256 strided partial sums and the butterfly
#pragma once
#include <hip/hip_runtime.h>
#include "vilf_internal.hpp"
#include "vilf_device.hpp"

#define SF_TERMS 28                         // 21 of H, 6 of g, the cost
#define SF_NT 256                           // the workgroup of sf_total, sf_cost and sf_pnp

struct SfPar { int min_count, warn_count, iters; double lambda0; };
struct SfRow { int m, flags, accepted; double cost0, cost1; };

namespace {

// the paragraph "sums": the butterfly within the wave, then waves 0 + 1 + 2 + 3; red [4][K]. Every thread returns with the same K sums.
template <int K> VD void sf_total(double (&v)[K], double *red, int tid) {
#pragma unroll
    for (int k = 0; k < K; k++)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] = __dadd_rn(v[k], __shfl_xor(v[k], o));
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) red[(tid >> 6) * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) v[k] = __dadd_rn(__dadd_rn(__dadd_rn(red[k], red[K + k]), red[2 * K + k]), red[3 * K + k]);
}

// the paragraph "residual" for member j
VD void sf_residual(const double *R, const double *t, const float *X, float2 u, double *q, double &iz, double &xn, double &yn, double &e0, double &e1) {
    const double X0 = (double)X[0], X1 = (double)X[1], X2 = (double)X[2];
#pragma unroll
    for (int r = 0; r < 3; r++) q[r] = vilf_dot3(R[r * 3], X0, R[r * 3 + 1], X1, R[r * 3 + 2], X2);
    const double p0 = __dadd_rn(q[0], t[0]), p1 = __dadd_rn(q[1], t[1]), p2 = __dadd_rn(q[2], t[2]);
    iz = __ddiv_rn(1.0, p2); xn = __dmul_rn(p0, iz); yn = __dmul_rn(p1, iz);
    e0 = __dsub_rn(xn, (double)u.x); e1 = __dsub_rn(yn, (double)u.y);
}

// the paragraphs "Jacobian" and "terms" for one member: its 28 terms are added to s
VD void sf_add_terms(const double *R, const double *t, const float *X, float2 u, double (&s)[SF_TERMS]) {
    double q[3], iz, xn, yn, e0, e1;
    sf_residual(R, t, X, u, q, iz, xn, yn, e0, e1);
    const double c0 = __dmul_rn(xn, iz), c1 = __dmul_rn(yn, iz);
    const double J0[6] = {-__dmul_rn(c0, q[1]), __dadd_rn(__dmul_rn(iz, q[2]), __dmul_rn(c0, q[0])), -__dmul_rn(iz, q[1]), iz, 0.0, -c0};
    const double J1[6] = {-__dadd_rn(__dmul_rn(iz, q[2]), __dmul_rn(c1, q[1])), __dmul_rn(c1, q[0]), __dmul_rn(iz, q[0]), 0.0, iz, -c1};
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = a; b < 6; b++, k++) s[k] = __dadd_rn(s[k], __dadd_rn(__dmul_rn(J0[a], J0[b]), __dmul_rn(J1[a], J1[b])));
#pragma unroll
    for (int a = 0; a < 6; a++) s[21 + a] = __dadd_rn(s[21 + a], __dadd_rn(__dmul_rn(J0[a], e0), __dmul_rn(J1[a], e1)));
    s[27] = __dadd_rn(s[27], __dadd_rn(__dmul_rn(e0, e0), __dmul_rn(e1, e1)));
}

// the paragraph "solve": LDL^T of the damped system, every loop unrolled so that the factors stay in registers -> x and whether every pivot was > 0 (x is computed
// either way; a caller ignores it after a rejected pivot)
VD bool sf_solve(const double (&s)[SF_TERMS], double lam, double (&x)[6]) {
    double Hd[6][6], L[6][6], U[6][6], dg[6], y[6];
    {
        int k = 0;
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int b = a; b < 6; b++, k++) Hd[a][b] = a == b ? __dadd_rn(s[k], __dmul_rn(lam, s[k])) : s[k];
    }
    bool pos = true;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double acc = Hd[j][j];
#pragma unroll
        for (int k = 0; k < j; k++) acc = __dsub_rn(acc, __dmul_rn(U[j][k], L[j][k]));
        dg[j] = acc;
        pos = pos && acc > 0.0;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double a2 = Hd[j][i];
#pragma unroll
            for (int k = 0; k < j; k++) a2 = __dsub_rn(a2, __dmul_rn(U[i][k], L[j][k]));
            U[i][j] = a2; L[i][j] = __ddiv_rn(a2, acc);
        }
    }
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double acc = -s[21 + i];
#pragma unroll
        for (int k = 0; k < i; k++) acc = __dsub_rn(acc, __dmul_rn(L[i][k], y[k]));
        y[i] = acc;
    }
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        double acc = __ddiv_rn(y[i], dg[i]);
#pragma unroll
        for (int k = i + 1; k < 6; k++) acc = __dsub_rn(acc, __dmul_rn(L[k][i], x[k]));
        x[i] = acc;
    }
    return pos;
}

// the paragraph "candidate": (R, t) moved by the step x -> (Rn, tn)
VD void sf_candidate(const double *R, const double *t, const double (&x)[6], double *Rn, double *tn) {
    const double a0 = __dmul_rn(0.5, x[0]), a1 = __dmul_rn(0.5, x[1]), a2 = __dmul_rn(0.5, x[2]);
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
        for (int c = 0; c < 3; c++) Rn[r * 3 + c] = vilf_dot3(Q[r * 3], R[c], Q[r * 3 + 1], R[3 + c], Q[r * 3 + 2], R[6 + c]);
        tn[r] = __dadd_rn(t[r], x[3 + r]);
    }
}

VD double sf_cost(const double *R, const double *t, const float *sX, const float2 *su, int m, double *red2, int tid) {
    double c[1] = {0.0};
    for (int j = tid; j < m; j += SF_NT) {
        double q[3], iz, xn, yn, e0, e1;
        sf_residual(R, t, sX + 3 * j, su[j], q, iz, xn, yn, e0, e1);
        c[0] = __dadd_rn(c[0], __dadd_rn(__dmul_rn(e0, e0), __dmul_rn(e1, e1)));
    }
    sf_total<1>(c, red2, tid);
    return c[0];
}

// the paragraph solveFrameByPnP on the m members in sX [m][3], su [m] (LDS), from the guess in (R, t) -> the row and, if the frame does not fail, the pose in
// (R, t). Every thread of the workgroup calls it with the same arguments and leaves with the same results; red [4][SF_TERMS] and red2 [4] are LDS.
VD bool sf_pnp(const float *sX, const float2 *su, int m, int min_count, const SfPar &p, double *R, double *t, double *red, double *red2, int tid, SfRow &row) {
    row.m = m; row.flags = VILF_SFM_PNP | (m < p.warn_count ? VILF_SFM_FEW : 0); row.accepted = 0; row.cost0 = 0.0; row.cost1 = 0.0;
    if (m < min_count) { row.flags |= VILF_SFM_FAIL_COUNT; return false; }
    double lam = p.lambda0, cost = 0.0;
    for (int it = 0; it < p.iters; it++) {
        double s[SF_TERMS];
#pragma unroll
        for (int k = 0; k < SF_TERMS; k++) s[k] = 0.0;
        for (int j = tid; j < m; j += SF_NT) sf_add_terms(R, t, sX + 3 * j, su[j], s);
        sf_total<SF_TERMS>(s, red, tid);
        cost = s[27];
        if (it == 0) row.cost0 = cost;
        double x[6], Rn[9], tn[3];
        const bool pos = sf_solve(s, lam, x);
        sf_candidate(R, t, x, Rn, tn);
        const double cn = sf_cost(Rn, tn, sX, su, m, red2, tid);      // evaluated for a rejected pivot too (the barrier inside is met by all); its value is then not used
        if (pos && cn < cost) {
#pragma unroll
            for (int e = 0; e < 9; e++) R[e] = Rn[e];
#pragma unroll
            for (int r = 0; r < 3; r++) t[r] = tn[r];
            cost = cn; lam = __ddiv_rn(lam, 10.0); row.accepted++;
        } else {
            lam = __dmul_rn(lam, 10.0);
        }
    }
    row.cost1 = cost;
    bool fin = isfinite(cost);
#pragma unroll
    for (int e = 0; e < 9; e++) fin = fin && isfinite(R[e]);
#pragma unroll
    for (int r = 0; r < 3; r++) fin = fin && isfinite(t[r]);
    if (!fin) { row.flags |= VILF_SFM_FAIL_FINITE; return false; }
    row.flags |= VILF_SFM_POSE;
    return true;
}
}  // namespace
