// vilf_pose.hpp — the device functions of the essential-matrix decomposition and of the closed-form depths that the visual start-up (vilf_startup.hip, su_pose)
//   and the camera-IMU rotation calibration (vilf_exrot.hip, ex_solve) share. The arithmetic is stated once, in include/vilfusion.h ("Visual start-up:
//   relativePose", paragraphs recoverPose and cheirality). As in vilf_fmat.hpp every lane works on column `lane` of the LDS arrays.
#pragma once
#include <hip/hip_runtime.h>
#include "vilf_device.hpp"
#include "vilf_fmat.hpp"

namespace {
VD void su_cross(const double *p, const double *q, double *c) {
    c[0] = __dsub_rn(__dmul_rn(p[1], q[2]), __dmul_rn(p[2], q[1]));
    c[1] = __dsub_rn(__dmul_rn(p[2], q[0]), __dmul_rn(p[0], q[2]));
    c[2] = __dsub_rn(__dmul_rn(p[0], q[1]), __dmul_rn(p[1], q[0]));
}
// the two depths of the cheirality paragraph for (R, t) and the pair (a, b)
VD void su_depths(const double *R, const double *t, float2 a, float2 b, double &z1, double &z2) {
    const double ax = (double)a.x, ay = (double)a.y, bx = (double)b.x, by = (double)b.y;
    const double r0 = __dadd_rn(__dadd_rn(__dmul_rn(R[0], ax), __dmul_rn(R[1], ay)), R[2]), r1 = __dadd_rn(__dadd_rn(__dmul_rn(R[3], ax), __dmul_rn(R[4], ay)), R[5]);
    const double r2 = __dadd_rn(__dadd_rn(__dmul_rn(R[6], ax), __dmul_rn(R[7], ay)), R[8]);
    const double rr = vilf_dot3(r0, r0, r1, r1, r2, r2), xx = __dadd_rn(__dadd_rn(__dmul_rn(bx, bx), __dmul_rn(by, by)), 1.0);
    const double rx = __dadd_rn(__dadd_rn(__dmul_rn(r0, bx), __dmul_rn(r1, by)), r2), rt = vilf_dot3(r0, t[0], r1, t[1], r2, t[2]);
    const double xt = __dadd_rn(__dadd_rn(__dmul_rn(bx, t[0]), __dmul_rn(by, t[1])), t[2]);
    const double det = __dsub_rn(__dmul_rn(rr, xx), __dmul_rn(rx, rx));
    z1 = __ddiv_rn(__dsub_rn(__dmul_rn(rx, xt), __dmul_rn(xx, rt)), det);
    z2 = __ddiv_rn(__dsub_rn(__dmul_rn(rr, xt), __dmul_rn(rx, rt)), det);
}
// the recoverPose paragraph up to R1, R2 and t = u3: G = E^T E through the shared Jacobi in column `lane` of s_M (>= 6 rows) and s_V (>= 9 rows) -> whether
// every entry of the three is finite
VD bool su_decompose(const double *E, double (*s_M)[TK_F_LANES], double (*s_V)[TK_F_LANES], int lane, double *R1, double *R2, double *tv) {
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = a; b < 3; b++) {
            double acc = 0.0;
#pragma unroll
            for (int r = 0; r < 3; r++) acc = __dadd_rn(acc, __dmul_rn(E[r * 3 + a], E[r * 3 + b]));
            s_M[tk_iu(3, a, b)][lane] = acc;
        }
    tk_jacobi<3>(s_M, s_V, lane);
    const int i3 = tk_smallest<3>(s_M, lane), r0 = i3 == 0 ? 1 : 0, r1 = i3 == 2 ? 1 : 2;
    const bool up = s_M[tk_iu(3, r1, r1)][lane] > s_M[tk_iu(3, r0, r0)][lane];
    const int i1 = up ? r1 : r0, i2 = up ? r0 : r1;
    double v1[3], v2[3], v3[3], u1[3], u2[3], u3[3];
#pragma unroll
    for (int r = 0; r < 3; r++) { v1[r] = s_V[r * 3 + i1][lane]; v2[r] = s_V[r * 3 + i2][lane]; }
    su_cross(v1, v2, v3);
    {
        double wv[3];
#pragma unroll
        for (int r = 0; r < 3; r++) wv[r] = vilf_dot3(E[r * 3], v1[0], E[r * 3 + 1], v1[1], E[r * 3 + 2], v1[2]);
        const double nrm = __dsqrt_rn(vilf_dot3(wv[0], wv[0], wv[1], wv[1], wv[2], wv[2]));
#pragma unroll
        for (int r = 0; r < 3; r++) u1[r] = __ddiv_rn(wv[r], nrm);
#pragma unroll
        for (int r = 0; r < 3; r++) wv[r] = vilf_dot3(E[r * 3], v2[0], E[r * 3 + 1], v2[1], E[r * 3 + 2], v2[2]);
        const double nrm2 = __dsqrt_rn(vilf_dot3(wv[0], wv[0], wv[1], wv[1], wv[2], wv[2]));
#pragma unroll
        for (int r = 0; r < 3; r++) u2[r] = __ddiv_rn(wv[r], nrm2);
    }
    su_cross(u1, u2, u3);
    bool fin = true;
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double p21 = __dmul_rn(u2[r], v1[c]), p12 = __dmul_rn(u1[r], v2[c]), p33 = __dmul_rn(u3[r], v3[c]);
            R1[r * 3 + c] = __dadd_rn(__dsub_rn(p21, p12), p33);
            R2[r * 3 + c] = __dadd_rn(__dsub_rn(p12, p21), p33);
            fin = fin && isfinite(R1[r * 3 + c]) && isfinite(R2[r * 3 + c]);
        }
        tv[r] = u3[r];
        fin = fin && isfinite(tv[r]);
    }
    return fin;
}
}  // namespace
