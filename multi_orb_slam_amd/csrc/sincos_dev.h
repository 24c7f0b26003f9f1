// sincos_dev.h -- the double sine / cosine sequence shared by the device orders of pose.hip (ORBM_POSE_ORDER_DEVICE), sim3.hip
// (ORBM_SIM3_MATH_DEVICE) and sim3opt.hip; orbm_pose_sincos (include/orbm.h) is its test hook.  Next to it the exponential of
// sim3opt.hip's device order (test hook: orbm_sim3opt_exp), the atan2 of sim3.hip's (orbm_sim3_atan2), and the arc cosine and natural
// logarithm of essgraph.hip's (Sim3::log; test hook: orbm_sim3_log_eval).
#pragma once
#include <cmath>
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

// ---- exp of the device order of sim3opt.hip: + - * / and conversions in double -------------------------------------------------------
// k = x / ln 2 rounded to the nearest integer (the same 1.5 * 2^52 step), a two-part ln 2 whose high part has 21 trailing zero bits (k
// times it is exact), the Taylor polynomial to r^14 on [-ln2/2, ln2/2] in Horner form, then |k| exact doublings or halvings.  exp(0) is
// exactly 1.  Beyond the range of a double: infinity above, 0 below; a NaN stays one.
__host__ __device__ inline double pose_exp(double x) {
    if (!(x == x)) return x;
    if (x > 709.782712893384) return 1.79769313486231570815e+308 * 2.0;
    if (x < -745.2) return 0.0;
    const double INV_LN2 = 1.44269504088896338700e+00;
    const double LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;
    const double MAGIC = 6755399441055744.0;
    const double kf = (x * INV_LN2 + MAGIC) - MAGIC;
    const double r = (x - kf * LN2_HI) - kf * LN2_LO;
    double p = 1.0 / 87178291200.0;
    p = p * r + (1.0 / 6227020800.0);
    p = p * r + (1.0 / 479001600);
    p = p * r + (1.0 / 39916800);
    p = p * r + (1.0 / 3628800);
    p = p * r + (1.0 / 362880);
    p = p * r + (1.0 / 40320);
    p = p * r + (1.0 / 5040);
    p = p * r + (1.0 / 720);
    p = p * r + (1.0 / 120);
    p = p * r + (1.0 / 24);
    p = p * r + (1.0 / 6);
    p = p * r + (1.0 / 2);
    double e = 1.0 + (r + (r * r) * p);
    const int k = (int)kf;
    const double f = k < 0 ? 0.5 : 2.0;
    const int m = k < 0 ? -k : k;
    for (int i = 0; i < m; ++i) e = e * f;
    return e;
}

// ---- atan2 of ORBM_SIM3_MATH_DEVICE: y >= 0, x in [-1, 1] ------------------------------------------------------------------------------
// atan of |a| <= 1: three half-angle steps a <- a / (1 + sqrt(1 + a*a)) bring it below tan(pi/32), the odd series to a^19 there (the
// first term left out is below 2^-70 of the result), times 8.
__host__ __device__ inline double sim3_atan_unit(double a) {
    a = a / (1.0 + sqrt(1.0 + a * a));
    a = a / (1.0 + sqrt(1.0 + a * a));
    a = a / (1.0 + sqrt(1.0 + a * a));
    const double z = a * a;
    double q = 1.0 / 19;
    q = 1.0 / 17 - z * q;
    q = 1.0 / 15 - z * q;
    q = 1.0 / 13 - z * q;
    q = 1.0 / 11 - z * q;
    q = 1.0 / 9 - z * q;
    q = 1.0 / 7 - z * q;
    q = 1.0 / 5 - z * q;
    q = 1.0 / 3 - z * q;
    return 8.0 * (a - a * (z * q));
}
__host__ __device__ inline double sim3_atan2(double y, double x) {
    const double PI_HI = 3.141592653589793116e+00, PI_LO = 1.224646799147353207e-16;
    const double PIO2_HI = 1.570796326794896558e+00, PIO2_LO = 6.123233995736766036e-17;
    const double ax = fabs(x);
    if (ax >= y) {                                   // the angle is within pi/4 of the x axis
        const double r = sim3_atan_unit((ax == 0 && y == 0) ? 0.0 : y / ax);
        return x < 0 ? (PI_HI - r) + PI_LO : r;
    }
    return (PIO2_HI - sim3_atan_unit(x / y)) + PIO2_LO;
}

// ---- arc cosine of the device order of essgraph.hip: d in [-1, 1] ---------------------------------------------------------------------
// acos d = atan2(sqrt(1 - d^2), d) with 1 - d^2 as (1 - d)(1 + d): 1 - d is exact from d = 1/2 on, where the cancellation would be.
__host__ __device__ inline double pose_acos(double d) { return sim3_atan2(sqrt((1.0 - d) * (1.0 + d)), d); }

// ---- natural logarithm of the device order of essgraph.hip: + - * / in double --------------------------------------------------------
// x = 2^k m with m in [sqrt(1/2), sqrt(2)) by exact halvings or doublings, z = (m - 1) / (m + 1) (|z| < 0.1716), log m = 2 z (1 + z^2/3
// + ... + z^22/23) in Horner form (the first term left out is below 2^-58 of the result), the two-part ln 2 of pose_exp.  log(1) is
// exactly 0.  A NaN or a negative argument: NaN; 0: -infinity; infinity stays.
__host__ __device__ inline double pose_log(double x) {
    if (!(x == x) || x < 0) return (x - x) / (x - x);
    if (x == 0) return -1.0 / (x * x);
    if (x > 1.79769313486231570815e+308) return x;
    const double SQRT2 = 1.41421356237309514547e+00, SQRT1_2 = 7.07106781186547572737e-01;
    const double LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;
    int k = 0;
    while (x >= SQRT2) { x = x * 0.5; ++k; }
    while (x < SQRT1_2) { x = x * 2.0; --k; }
    const double z = (x - 1.0) / (x + 1.0);
    const double w = z * z;
    double p = 1.0 / 23;
    p = p * w + (1.0 / 21);
    p = p * w + (1.0 / 19);
    p = p * w + (1.0 / 17);
    p = p * w + (1.0 / 15);
    p = p * w + (1.0 / 13);
    p = p * w + (1.0 / 11);
    p = p * w + (1.0 / 9);
    p = p * w + (1.0 / 7);
    p = p * w + (1.0 / 5);
    p = p * w + (1.0 / 3);
    const double kf = (double)k;
    return kf * LN2_HI + ((2.0 * z + (2.0 * z) * (w * p)) + kf * LN2_LO);
}
