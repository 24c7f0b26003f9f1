// sincos_dev.h -- the double sine / cosine sequence shared by the device orders of pose.hip (ORBM_POSE_ORDER_DEVICE) and sim3.hip
// (ORBM_SIM3_MATH_DEVICE); orbm_pose_sincos (include/orbm.h) is its test hook.
#pragma once
#include <hip/hip_runtime.h>

// ---- sine and cosine of ORBM_POSE_ORDER_DEVICE: one sequence of + - * / in double (the det_sincos precedent of the extractor) --------
// k = x * 2/pi rounded to the nearest integer by adding and subtracting 1.5 * 2^52, a two-part pi/2, Taylor polynomials to z^8 on
// [-pi/4, pi/4].  Within 2 ulp of the C library on [-100, 100] (tests/test_pose_model.py).
__host__ __device__ inline void pose_sincos(double x, double* sn, double* cs) {
    const double TWO_OVER_PI = 6.36619772367581382433e-01;
    const double PIO2_HI = 1.57079632673412561417e+00, PIO2_LO = 6.07710050650619224932e-11;
    const double MAGIC = 6755399441055744.0;
    const double kf = (x * TWO_OVER_PI + MAGIC) - MAGIC;
    const double r = (x - kf * PIO2_HI) - kf * PIO2_LO;
    const double z = r * r;
    double ps = 1.0 / 355687428096000.0;
    ps = ps * z + (-1.0 / 1307674368000.0);
    ps = ps * z + (1.0 / 6227020800.0);
    ps = ps * z + (-1.0 / 39916800);
    ps = ps * z + (1.0 / 362880);
    ps = ps * z + (-1.0 / 5040);
    ps = ps * z + (1.0 / 120);
    ps = ps * z + (-1.0 / 6);
    const double s = r + r * (z * ps);
    double pc = 1.0 / 20922789888000.0;
    pc = pc * z + (-1.0 / 87178291200.0);
    pc = pc * z + (1.0 / 479001600);
    pc = pc * z + (-1.0 / 3628800);
    pc = pc * z + (1.0 / 40320);
    pc = pc * z + (-1.0 / 720);
    pc = pc * z + (1.0 / 24);
    pc = pc * z + (-1.0 / 2);
    const double c = 1.0 + z * pc;
    const int q = (int)((long long)kf & 3);
    *cs = (q == 0) ? c : (q == 1) ? -s : (q == 2) ? -c : s;
    *sn = (q == 0) ? s : (q == 1) ? c : (q == 2) ? -s : -c;
}
