// cv_dev.h -- the OpenCV boundary: every OpenCV operation that a reference routine calls and this library restates, ONE definition each,
// for the kernels and the host routines of triangulate.hip, sim3.hip, mappoint.hip, frustum.hip and pose.hip.  Each is restated from
// OpenCV's published sources (2.4.x / 3.2), statement by statement in the number formats those have (the rules of host/cv_compat.h, the
// independent restatement that tests/test_cv_dev.py compares this one with); where a function says UNPINNED, OpenCV was never in a build
// to compare against and a later pin changes that one definition.  The library is built without contraction and
// without fast-math, and the tests compare bytes: nothing inside these bodies is to be reordered.
// Plain C++ apart from the attributes, so that a host compiler can include it.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#ifdef __HIPCC__
#define CV_DEV_FN __host__ __device__ inline
#else
#define CV_DEV_FN inline
#endif

// cv::gemm, the small path (flags == 0, an inner length of 3: cv_compat.h gemm_small_elem): products and sums in float, left to right,
// then d = (float)(t*alpha + c*beta) in double.  R*x + t, R*P, O1 - s*R*O2 and -sRinv*t all arrive here.
CV_DEV_FN float cv_gemm3(float a0, float a1, float a2, float b0, float b1, float b2, double alpha, float c, double beta) {
    float t = a0 * b0 + a1 * b1;
    t = t + a2 * b2;
    return (float)((double)t * alpha + (double)c * beta);
}
// ... with a: a row of the left matrix with element stride sa, b: a 3x1 right matrix.
CV_DEV_FN float cv_gemm3(const float* a, int sa, const float* b, double alpha, float c, double beta) {
    return cv_gemm3(a[0], a[sa], a[2 * sa], b[0], b[1], b[2], alpha, c, beta);
}
// cv::gemm's general path for Pr2 * Pr1.t() (GEMM_2_T, inner length 3): the products summed in double from 0.0 in one running sum (the
// four-way unrolled loop does not run below a length of 4), (s0 + s1 + s2 + s3) * alpha with the idle sums 0, one rounding to float.
// UNPINNED.
CV_DEV_FN float cv_gemm3_bt(const float* a, const float* b) {
    double s0 = 0;
    for (int k = 0; k < 3; ++k) s0 += (double)a[k] * (double)b[k];
    return (float)((((s0 + 0.0) + 0.0) + 0.0) * 1.0);
}
// cv::Mat::dot of a 1x3 row with a 1x3 row: products summed in double, in order
CV_DEV_FN double cv_dot3(const float* a, const float* b) {
    double s = 0;
    for (int k = 0; k < 3; ++k) s += (double)a[k] * (double)b[k];
    return s;
}
// cv::norm(NORM_L2) of three floats: squares summed in double, sqrt in double
CV_DEV_FN double cv_norm3(const float* a) {
    double s = 0;
    for (int k = 0; k < 3; ++k) s += (double)a[k] * (double)a[k];
    return sqrt(s);
}
// a scaled matrix evaluated on its own (host/cv_compat.h ew_scale): cv::add(M, 0) for a weight of exactly 1, cv::subtract(0, M) for -1,
// else convertTo, whose float kernel computes src * (float)alpha + 0.0f.  `x3D.rowRange(0,3)/w` is this with alpha = 1. / w, `C / P.cols`
// with alpha = 1. / 3, `2*ang*vec/norm(vec)` with alpha = (2 * ang) * (1. / norm), `ms12i * mR12i` with alpha = (double)ms12i,
// `normal/n` with alpha = 1.0 / n.  UNPINNED.
CV_DEV_FN float cv_scale(float x, double alpha) {
    const float al = (float)alpha;
    return alpha == 1 ? x + 0.0f : alpha == -1 ? 0.0f - x : x * al + 0.0f;
}
// s * M.t() (MatOp_T: the transpose, then convertTo when the weight is not 1): one element of the transposed matrix.  UNPINNED.
CV_DEV_FN float cv_scale_t(float x, double alpha) { return alpha != 1 ? x * (float)alpha + 0.0f : x; }
// cv::reduce(P, C, 1, CV_REDUCE_SUM) of a 3x3 CV_32F into CV_32F: one row, summed in float in column order.  UNPINNED.
CV_DEV_FN float cv_reduce_row(float a, float b, float c) { return (a + b) + c; }

// The two hypots are two different OpenCV routines:
// UNPINNED.  JacobiSVDImpl_ calls hypot(p, beta) of the C library; no libm function runs in a kernel, so kernel, host routine and model
// all take this sequence in its place.  A later pin changes this one definition.
CV_DEV_FN double cv_hypot_libm(double a, double b) { return sqrt(a * a + b * b); }
// hypot of lapack.cpp (the template JacobiImpl_ calls), in float.  UNPINNED.
CV_DEV_FN float cv_hypot_lapack(float a, float b) {
    a = fabsf(a); b = fabsf(b);
    if (a > b) { b = b / a; return a * (float)sqrt((double)(1 + b * b)); }
    if (b > 0) { a = a / b; return b * (float)sqrt((double)(1 + a * a)); }
    return 0.0f;
}

// A NaN leaves as the NaN x86 makes from an invalid operation (sign bit set), whatever made this one; the GCN ALUs make 0x7fc00000 /
// 0x7ff8000000000000 from the same operation.
CV_DEV_FN float x86_nan(float x) {
    if (x == x) return x;
    const uint32_t bits = 0xffc00000u;
    float f;
    memcpy(&f, &bits, 4);
    return f;
}
CV_DEV_FN double x86_nan(double x) {
    if (x == x) return x;
    const unsigned long long bits = 0xfff8000000000000ull;
    double d;
    memcpy(&d, &bits, 8);
    return d;
}
