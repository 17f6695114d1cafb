// vilf_fmat.hpp — the device functions of the fixed-K 8-point search that the feature tracker (vilf_track.hip, rejectWithF) and the visual start-up
//   (vilf_startup.hip, relativePose) share. The arithmetic is stated once, in include/vilfusion.h ("Image feature tracker", paragraph rejectWithF); the start-up
//   text refers to it. Every function works on column `lane` of LDS arrays [rows][TK_F_LANES], so a lane's accesses never meet another's and nothing that is
//   indexed at run time lives in registers.
#pragma once
#include <hip/hip_runtime.h>
#include "vilf_device.hpp"

#define TK_F_SWEEPS 10
#define TK_F_LANES 64                   // a lane per hypothesis (or per redundant copy), its matrices a column of the LDS arrays; no barrier

namespace {
VD unsigned tk_mix(unsigned x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }
VD int tk_iu(int N, int p, int q) { return p * N - p * (p - 1) / 2 + (q - p); }      // upper triangle, p <= q
VD int tk_is(int N, int p, int q) { return p <= q ? tk_iu(N, p, q) : tk_iu(N, q, p); }
// cyclic Jacobi of the symmetric N x N matrix in column `lane` of M (upper triangle) -> eigenvectors in the columns of V (row-major N x N in column `lane`)
template <int N> VD void tk_jacobi(double (*M)[TK_F_LANES], double (*V)[TK_F_LANES], int lane) {
    for (int r = 0; r < N; r++) for (int c = 0; c < N; c++) V[r * N + c][lane] = r == c ? 1.0 : 0.0;
    for (int sweep = 0; sweep < TK_F_SWEEPS; sweep++)
        for (int p = 0; p < N - 1; p++)
            for (int q = p + 1; q < N; q++) {
                const int ipq = tk_iu(N, p, q), ipp = tk_iu(N, p, p), iqq = tk_iu(N, q, q);
                const double apq = M[ipq][lane];
                if (apq == 0.0) continue;
                const double app = M[ipp][lane], aqq = M[iqq][lane];
                const double theta = __ddiv_rn(__dsub_rn(aqq, app), __dmul_rn(2.0, apq));
                const double t = __ddiv_rn(theta < 0.0 ? -1.0 : 1.0, __dadd_rn(fabs(theta), __dsqrt_rn(__dadd_rn(__dmul_rn(theta, theta), 1.0))));
                const double c = __ddiv_rn(1.0, __dsqrt_rn(__dadd_rn(__dmul_rn(t, t), 1.0))), s = __dmul_rn(t, c);
                for (int r = 0; r < N; r++) {
                    if (r == p || r == q) continue;
                    const int irp = tk_is(N, r, p), irq = tk_is(N, r, q);
                    const double arp = M[irp][lane], arq = M[irq][lane];
                    M[irp][lane] = __dsub_rn(__dmul_rn(c, arp), __dmul_rn(s, arq));
                    M[irq][lane] = __dadd_rn(__dmul_rn(s, arp), __dmul_rn(c, arq));
                }
                const double tap = __dmul_rn(t, apq);
                M[ipp][lane] = __dsub_rn(app, tap); M[iqq][lane] = __dadd_rn(aqq, tap); M[ipq][lane] = 0.0;
                for (int r = 0; r < N; r++) {
                    const double vrp = V[r * N + p][lane], vrq = V[r * N + q][lane];
                    V[r * N + p][lane] = __dsub_rn(__dmul_rn(c, vrp), __dmul_rn(s, vrq));
                    V[r * N + q][lane] = __dadd_rn(__dmul_rn(s, vrp), __dmul_rn(c, vrq));
                }
            }
}
template <int N> VD int tk_smallest(double (*M)[TK_F_LANES], int lane) {
    int at = 0;
    double best = M[0][lane];
    for (int i = 1; i < N; i++) { const double a = M[tk_iu(N, i, i)][lane]; if (a < best) { best = a; at = i; } }
    return at;
}
// Hartley normalisation of the eight points (x in P[0 .. 7], y in P[8 .. 15], column `lane`), in place -> centroid and scale
VD void tk_hartley(double (*P)[TK_F_LANES], int lane, double &cx, double &cy, double &s) {
    double sx = 0.0, sy = 0.0, md = 0.0;
    for (int j = 0; j < 8; j++) { sx = __dadd_rn(sx, P[j][lane]); sy = __dadd_rn(sy, P[8 + j][lane]); }
    cx = __ddiv_rn(sx, 8.0); cy = __ddiv_rn(sy, 8.0);
    for (int j = 0; j < 8; j++) {
        const double dx = __dsub_rn(P[j][lane], cx), dy = __dsub_rn(P[8 + j][lane], cy);
        md = __dadd_rn(md, __dsqrt_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy))));
    }
    md = __ddiv_rn(md, 8.0);
    s = __ddiv_rn(__dsqrt_rn(2.0), md);
    for (int j = 0; j < 8; j++) { P[j][lane] = __dmul_rn(__dsub_rn(P[j][lane], cx), s); P[8 + j][lane] = __dmul_rn(__dsub_rn(P[8 + j][lane], cy), s); }
}
// the score's inlier rule for the point pair (a, b) under F (row-major)
VD bool tk_f_inlier(const double *F, float2 a, float2 b, double thr2) {
    const double x = (double)a.x, y = (double)a.y, xp = (double)b.x, yp = (double)b.y;
    const double lp0 = __dadd_rn(__dadd_rn(__dmul_rn(F[0], x), __dmul_rn(F[1], y)), F[2]), lp1 = __dadd_rn(__dadd_rn(__dmul_rn(F[3], x), __dmul_rn(F[4], y)), F[5]);
    const double lp2 = __dadd_rn(__dadd_rn(__dmul_rn(F[6], x), __dmul_rn(F[7], y)), F[8]);
    const double l0 = __dadd_rn(__dadd_rn(__dmul_rn(F[0], xp), __dmul_rn(F[3], yp)), F[6]), l1 = __dadd_rn(__dadd_rn(__dmul_rn(F[1], xp), __dmul_rn(F[4], yp)), F[7]);
    const double d = __dadd_rn(__dadd_rn(__dmul_rn(xp, lp0), __dmul_rn(yp, lp1)), lp2), d2 = __dmul_rn(d, d);
    const double e1 = __ddiv_rn(d2, __dadd_rn(__dmul_rn(lp0, lp0), __dmul_rn(lp1, lp1))), e2 = __ddiv_rn(d2, __dadd_rn(__dmul_rn(l0, l0), __dmul_rn(l1, l1)));
    return e1 <= thr2 && e2 <= thr2;
}
// hypothesis k of the search over the n >= 8 point pairs (ua[i], ub[i]): sample, Hartley, M = A^T A, Jacobi, rank 2, denormalise -> F (row-major) and whether
// it is valid. s_M [45][TK_F_LANES] and s_V [81][TK_F_LANES] are the workgroup's LDS; the caller's lane owns column `lane` of both
VD bool tk_f_hypothesis(const float2 *ua, const float2 *ub, int n, int k, unsigned seed, double (*s_M)[TK_F_LANES], double (*s_V)[TK_F_LANES], int lane, double *F) {
    // sample: slot j in registers (every loop over the slots is unrolled, so S is never indexed by a run-time value)
    int S[8];
    const unsigned base = tk_mix(tk_mix(seed + 0x9e3779b9u) + (unsigned)k);
#pragma unroll
    for (int j = 0; j < 8; j++) {
        int i = (int)(((unsigned long long)tk_mix(base + (unsigned)j) * (unsigned long long)n) >> 32);
#pragma unroll
        for (int step = 0; step < j; step++) {
            bool dup = false;
#pragma unroll
            for (int e = 0; e < j; e++) dup |= S[e] == i;
            i = dup ? (i + 1 == n ? 0 : i + 1) : i;
        }
        S[j] = i;
    }
    // the sample's points: side 1 in s_V[0 .. 15], side 2 in s_V[16 .. 31] (V is not needed before the Jacobi)
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const float2 a = ua[S[j]], b = ub[S[j]];             // S[j] < n
        s_V[j][lane] = (double)a.x; s_V[8 + j][lane] = (double)a.y; s_V[16 + j][lane] = (double)b.x; s_V[24 + j][lane] = (double)b.y;
    }
    double cx1, cy1, s1, cx2, cy2, s2;
    tk_hartley(s_V, lane, cx1, cy1, s1);
    tk_hartley(s_V + 16, lane, cx2, cy2, s2);
    for (int e = 0; e < 45; e++) s_M[e][lane] = 0.0;
    for (int j = 0; j < 8; j++) {
        const double x = s_V[j][lane], y = s_V[8 + j][lane], xp = s_V[16 + j][lane], yp = s_V[24 + j][lane];
        const double r[9] = {__dmul_rn(xp, x), __dmul_rn(xp, y), xp, __dmul_rn(yp, x), __dmul_rn(yp, y), yp, x, y, 1.0};
        int e = 0;
#pragma unroll
        for (int p = 0; p < 9; p++)
#pragma unroll
            for (int q = p; q < 9; q++, e++) s_M[e][lane] = __dadd_rn(s_M[e][lane], __dmul_rn(r[p], r[q]));
    }
    tk_jacobi<9>(s_M, s_V, lane);
    double Fh[9];
    {
        const int at = tk_smallest<9>(s_M, lane);
#pragma unroll
        for (int c = 0; c < 9; c++) Fh[c] = s_V[c * 9 + at][lane];
    }
    // rank 2: the same Jacobi at size 3 on G = Fh^T Fh
#pragma unroll
    for (int p = 0; p < 3; p++)
#pragma unroll
        for (int q = p; q < 3; q++) {
            double acc = 0.0;
#pragma unroll
            for (int r = 0; r < 3; r++) acc = __dadd_rn(acc, __dmul_rn(Fh[r * 3 + p], Fh[r * 3 + q]));
            s_M[tk_iu(3, p, q)][lane] = acc;
        }
    tk_jacobi<3>(s_M, s_V, lane);
    {
        const int at = tk_smallest<3>(s_M, lane);
        const double v0 = s_V[at][lane], v1 = s_V[3 + at][lane], v2 = s_V[6 + at][lane];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const double w = __dadd_rn(__dadd_rn(__dmul_rn(Fh[r * 3], v0), __dmul_rn(Fh[r * 3 + 1], v1)), __dmul_rn(Fh[r * 3 + 2], v2));
            Fh[r * 3] = __dsub_rn(Fh[r * 3], __dmul_rn(w, v0)); Fh[r * 3 + 1] = __dsub_rn(Fh[r * 3 + 1], __dmul_rn(w, v1)); Fh[r * 3 + 2] = __dsub_rn(Fh[r * 3 + 2], __dmul_rn(w, v2));
        }
    }
    // F = T'^T Fh T
    const double t1x = __dmul_rn(s1, cx1), t1y = __dmul_rn(s1, cy1), t2x = __dmul_rn(s2, cx2), t2y = __dmul_rn(s2, cy2);
    double B[9];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        B[r * 3] = __dmul_rn(Fh[r * 3], s1); B[r * 3 + 1] = __dmul_rn(Fh[r * 3 + 1], s1);
        B[r * 3 + 2] = __dsub_rn(__dsub_rn(Fh[r * 3 + 2], __dmul_rn(Fh[r * 3], t1x)), __dmul_rn(Fh[r * 3 + 1], t1y));
    }
    bool ok = isfinite(s1) && isfinite(s2);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        F[c] = __dmul_rn(s2, B[c]); F[3 + c] = __dmul_rn(s2, B[3 + c]);
        F[6 + c] = __dsub_rn(__dsub_rn(B[6 + c], __dmul_rn(t2x, B[c])), __dmul_rn(t2y, B[3 + c]));
    }
#pragma unroll
    for (int e = 0; e < 9; e++) ok = ok && isfinite(F[e]);
    return ok;
}
}  // namespace
