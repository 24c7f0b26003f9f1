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

// ---- double matrices of run-time shape (pnp.hip) -----------------------------------------------------------------------------------------
// A strided view of doubles: element i lies at p[i * s].  s = 1 on the host and for a workgroup's shared block; s = the lanes of the
// workgroup where every lane owns one matrix in LDS (element-major, lane-minor: run-time indices cost nothing, nothing goes to scratch).
struct cv_vec {
    double* p;
    int s;
#ifdef __HIPCC__
    __host__ __device__
#endif
    inline double& operator[](int i) const { return p[(size_t)i * (size_t)s]; }
#ifdef __HIPCC__
    __host__ __device__
#endif
    inline cv_vec at(int off) const { cv_vec v = {p + (size_t)off * (size_t)s, s}; return v; }
};

// JacobiSVDImpl_<double> (modules/core/src/lapack.cpp, 3.2) as _SVDcompute and cv::solve call it for m >= n: At holds the TRANSPOSE of
// the m x n matrix (n rows of m, row stride m), W n values, Vt n x n (row stride n; written only when want_vt).  UNPINNED.
//   * eps = DBL_EPSILON*10, minval = DBL_MIN, at most max(m, 30) sweeps over the pairs in row-major order, ended by a sweep that rotates
//     nothing; W[i] and p are running double sums in element order; a pair is skipped when |p| <= eps*sqrt(a*b);
//   * hypot is cv_hypot_libm; c and s in double; the new W[i], W[j] are fresh sums of the rotated elements;
//   * the singular values are sqrt of fresh sums; selection sort, descending, strict `W[j] < W[k]`, rows of At (and Vt) following;
//   * the completion that makes U out of At (n1 = n rows): a row whose singular value is <= minval is replaced by a vector of +-1/m
//     drawn from cv::RNG(0x12345678) (one generator per call; `next() & 256` picks the sign), orthogonalised against the rows before it
//     in two passes (each pass rescales by 1/sum|t| when that exceeds eps*100, else by 0) and measured again, at most 100 times; then
//     every row is scaled by 1/sd (0 when sd <= minval).
// Returns 1 when a row entered the random completion, else 0.  At (rows) = U transposed, W = the singular values.
CV_DEV_FN int cv_jacobi_svd_f64(cv_vec At, int m, int n, cv_vec W, cv_vec Vt, bool want_vt) {
    const double eps = 2.2204460492503131e-16 * 10, minval = 2.2250738585072014e-308;
    for (int i = 0; i < n; ++i) {
        double sd = 0;
        for (int k = 0; k < m; ++k) { const double t = At[i * m + k]; sd += t * t; }
        W[i] = sd;
        if (want_vt) {
            for (int k = 0; k < n; ++k) Vt[i * n + k] = 0;
            Vt[i * n + i] = 1;
        }
    }
    const int max_iter = m > 30 ? m : 30;
    for (int iter = 0; iter < max_iter; ++iter) {
        bool changed = false;
        for (int i = 0; i < n - 1; ++i)
            for (int j = i + 1; j < n; ++j) {
                double a = W[i], p = 0, b = W[j];
                for (int k = 0; k < m; ++k) p += At[i * m + k] * At[j * m + k];
                if (fabs(p) <= eps * sqrt(a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = cv_hypot_libm(p, beta);
                double c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = sqrt(delta / gamma);
                    c = p / (gamma * s * 2);
                } else {
                    c = sqrt((gamma + beta) / (gamma * 2));
                    s = p / (gamma * c * 2);
                }
                a = b = 0;
                for (int k = 0; k < m; ++k) {
                    const double x = At[i * m + k], y = At[j * m + k];
                    const double t0 = c * x + s * y;
                    const double t1 = -s * x + c * y;
                    At[i * m + k] = t0; At[j * m + k] = t1;
                    a += t0 * t0; b += t1 * t1;
                }
                W[i] = a; W[j] = b;
                changed = true;
                if (want_vt)
                    for (int k = 0; k < n; ++k) {
                        const double x = Vt[i * n + k], y = Vt[j * n + k];
                        const double t0 = c * x + s * y;
                        const double t1 = -s * x + c * y;
                        Vt[i * n + k] = t0; Vt[j * n + k] = t1;
                    }
            }
        if (!changed) break;
    }
    for (int i = 0; i < n; ++i) {
        double sd = 0;
        for (int k = 0; k < m; ++k) { const double t = At[i * m + k]; sd += t * t; }
        W[i] = sqrt(sd);
    }
    for (int i = 0; i < n - 1; ++i) {
        int j = i;
        for (int k = i + 1; k < n; ++k) if (W[j] < W[k]) j = k;
        if (i != j) {
            { const double t = W[i]; W[i] = W[j]; W[j] = t; }
            for (int k = 0; k < m; ++k) { const double t = At[i * m + k]; At[i * m + k] = At[j * m + k]; At[j * m + k] = t; }
            if (want_vt) for (int k = 0; k < n; ++k) { const double t = Vt[i * n + k]; Vt[i * n + k] = Vt[j * n + k]; Vt[j * n + k] = t; }
        }
    }
    int random = 0;
    unsigned long long rng = 0x12345678ull;
    for (int i = 0; i < n; ++i) {
        double sd = W[i];
        for (int ii = 0; ii < 100 && sd <= minval; ++ii) {
            random = 1;
            const double val0 = 1. / m;
            for (int k = 0; k < m; ++k) {
                rng = (unsigned long long)(unsigned)rng * 4164903690ull + (unsigned)(rng >> 32);
                At[i * m + k] = ((unsigned)rng & 256u) != 0 ? val0 : -val0;
            }
            for (int iter = 0; iter < 2; ++iter)
                for (int j = 0; j < i; ++j) {
                    sd = 0;
                    for (int k = 0; k < m; ++k) sd += At[i * m + k] * At[j * m + k];
                    double asum = 0;
                    for (int k = 0; k < m; ++k) {
                        const double t = At[i * m + k] - sd * At[j * m + k];
                        At[i * m + k] = t;
                        asum += fabs(t);
                    }
                    asum = asum > eps * 100 ? 1 / asum : 0;
                    for (int k = 0; k < m; ++k) At[i * m + k] *= asum;
                }
            sd = 0;
            for (int k = 0; k < m; ++k) { const double t = At[i * m + k]; sd += t * t; }
            sd = sqrt(sd);
        }
        const double s = sd > minval ? 1 / sd : 0.;
        for (int k = 0; k < m; ++k) At[i * m + k] *= s;
    }
    return random;
}

// SVBkSb (modules/core/src/lapack.cpp) behind cvSolve(A, b, x, CV_SVD) with one right-hand side: threshold = DBL_EPSILON*2 * sum of w,
// only w[i] > threshold contributes; s = (sum over j of u_i[j]*b[j], in order) * (1/w[i]); x[j] = x[j] + s*v_i[j].  At, W, Vt as
// cv_jacobi_svd_f64 left them.  UNPINNED.
CV_DEV_FN void cv_svd_backsubst_vec(cv_vec At, int m, int n, cv_vec W, cv_vec Vt, cv_vec b, cv_vec x) {
    for (int j = 0; j < n; ++j) x[j] = 0;
    double threshold = 0;
    for (int i = 0; i < n; ++i) threshold += W[i];
    threshold *= 2.2204460492503131e-16 * 2;
    for (int i = 0; i < n; ++i) {
        double wi = W[i];
        if (fabs(wi) <= threshold) continue;
        wi = 1 / wi;
        double s = 0;
        for (int j = 0; j < m; ++j) s += At[i * m + j] * b[j];
        s *= wi;
        for (int j = 0; j < n; ++j) x[j] = x[j] + s * Vt[i * n + j];
    }
}
// ... behind cvInvert(A, Ainv, CV_SVD) of an n x n matrix (no right-hand side: the identity): buffer[j] = u[j][i] * (1/w[i]), then
// x[r][j] = x[r][j] + v_i[r]*buffer[j].  UNPINNED.
CV_DEV_FN void cv_svd_backsubst_inv(cv_vec At, int n, cv_vec W, cv_vec Vt, cv_vec x) {
    for (int j = 0; j < n * n; ++j) x[j] = 0;
    double threshold = 0;
    for (int i = 0; i < n; ++i) threshold += W[i];
    threshold *= 2.2204460492503131e-16 * 2;
    for (int i = 0; i < n; ++i) {
        double wi = W[i];
        if (fabs(wi) <= threshold) continue;
        wi = 1 / wi;
        for (int r = 0; r < n; ++r) {
            const double s = Vt[i * n + r];
            for (int j = 0; j < n; ++j) x[r * n + j] = x[r * n + j] + s * (At[i * n + j] * wi);
        }
    }
}
