// vilf_image.hpp — what the image texts of include/vilfusion.h share, each as one device function: the reflected index R(i, n) and the pinhole camera's
//   undistortion (the tracker's paragraphs "conventions" and "undistortion"). Used by the feature tracker (vilf_track.hip: the pyramid, LK, the detection, tk_finish
//   and the lifts of rejectWithF) and by the key-frame store of the visual loop closure (vilf_kf.hip: kf_blur, kf_lift).
#pragma once
#include <hip/hip_runtime.h>
#include "vilf_device.hpp"

// R(i, n): reflect-101, periodic with period 2 (n - 1); n >= 2
VD int tk_r(int i, int n) {
    if ((unsigned)i < (unsigned)n) return i;
    const int p = 2 * (n - 1);
    int m = i % p;
    m += m < 0 ? p : 0;
    return m < n ? m : p - m;
}
struct TkCam { double i11, i13, i22, i23, k1, k2, p1, p2; int distort; };
// the inverse-K entries of PinholeCamera::liftProjective (PinholeCamera.cc:457-461) from the camera's parameters
static inline TkCam tk_cam(double fx, double fy, double cx, double cy, double k1, double k2, double p1, double p2) {
    TkCam cam;
    cam.i11 = 1.0 / fx; cam.i13 = -cx / fx; cam.i22 = 1.0 / fy; cam.i23 = -cy / fy;
    cam.k1 = k1; cam.k2 = k2; cam.p1 = p1; cam.p2 = p2;
    cam.distort = (k1 != 0.0 || k2 != 0.0 || p1 != 0.0 || p2 != 0.0) ? 1 : 0;
    return cam;
}
// the undistortion text in fp64: liftProjective of the float32 pixel p, before any rounding to float32
VD void tk_undistort(const TkCam &cam, float2 p, double &ux, double &uy) {
    const double mx = __dadd_rn(__dmul_rn(cam.i11, (double)p.x), cam.i13), my = __dadd_rn(__dmul_rn(cam.i22, (double)p.y), cam.i23);
    ux = mx; uy = my;
    if (cam.distort) {
        for (int r = 0; r < 8; r++) {                // PinholeCamera::distortion (PinholeCamera.cc:646-662), every operation rounded on its own
            const double x2 = __dmul_rn(ux, ux), y2 = __dmul_rn(uy, uy), xy = __dmul_rn(ux, uy), rho2 = __dadd_rn(x2, y2);
            const double rad = __dadd_rn(__dmul_rn(cam.k1, rho2), __dmul_rn(__dmul_rn(cam.k2, rho2), rho2));
            const double ddx = __dadd_rn(__dadd_rn(__dmul_rn(ux, rad), __dmul_rn(__dmul_rn(2.0, cam.p1), xy)), __dmul_rn(cam.p2, __dadd_rn(rho2, __dmul_rn(2.0, x2))));
            const double ddy = __dadd_rn(__dadd_rn(__dmul_rn(uy, rad), __dmul_rn(__dmul_rn(2.0, cam.p2), xy)), __dmul_rn(cam.p1, __dadd_rn(rho2, __dmul_rn(2.0, y2))));
            ux = __dsub_rn(mx, ddx); uy = __dsub_rn(my, ddy);
        }
    }
}
