// sim3.hip -- every RANSAC hypothesis of a loop's Sim3Solvers in one call (include/orbm.h, "Sim3Solver"): Sim3Solver::ComputeCentroid,
// ComputeSim3 (steps 1-8), Project, FromCameraToImage and CheckInliers (reference src/Sim3Solver.cc:271-522) restated, with the OpenCV
// operators they call.
//   sim3_cv_*        the OpenCV operators only Sim3Solver calls (cv::eigen, cv::Rodrigues), restated from OpenCV's published sources
//                    (2.4.x / 3.2) and UNPINNED (OpenCV is not in the build: DESIGN.md section 2): each is ONE function that a later
//                    pin changes.  The operators other routines call as well (gemm, dot, norm, scaled matrices) are cv_dev.h's.
//   sim3_atan2       the atan2 of ORBM_SIM3_MATH_DEVICE: + - * / sqrt in double (sincos_dev.h, next to that order's sine and cosine, pose_sincos).
//   sim3_horn        one hypothesis: three point pairs -> mR12i, mt12i, ms12i, mT12i, mT21i.  ONE statement sequence for the kernel and
//                    the host routine; the 4x4 Jacobi addresses its matrices with compile-time indices only (nothing goes to scratch).
//   sim3_inlier      one correspondence under one hypothesis: both projections, both threshold tests.
//   k_sim3_hyp       one lane per (problem, hypothesis), workgroups of 64: gathers the triple, runs sim3_horn in registers, writes the
//                    record to HBM (for the second kernel) and to the mapped result.
//   k_sim3_inliers   one wave per hypothesis: lane l takes correspondences l, l + 64, ... of the structure-of-arrays (coalesced);
//                    the sweep that turns sim3_inlier into mask words and a count is ransac_mask_sweep (ransac_dev.h).
// The two kernels go onto the stream back to back: one enqueue, one synchronisation per call (ransac_csr_call, ransac_dev.h; the
// checks of a call: ransac_validate<3>).
// No libm function runs in the kernels: + - * / sqrt in float and double, conversions.
#include <cfloat>
#include <cmath>
#include <vector>

#include "../../include/orbm.h"
#include "../../include/orb_debug.h"
#include "orb_common.h"
#include "matcher_internal.h"
#include "sincos_dev.h"
#include "cv_dev.h"
#include "stage_pack.h"
#include "ransac_dev.h"

namespace {

constexpr int SIM3_T = 64;   // lanes of a workgroup of either kernel = one wave

// ---- the OpenCV boundary, Sim3Solver's own part: UNPINNED -----------------------------------------------------------
__host__ __device__ __forceinline__ void sim3_rot(float& v0, float& v1, float c, float s) {
    const float a0 = v0, b0 = v1;
    v0 = a0 * c - b0 * s;
    v1 = a0 * s + b0 * c;
}
// one Jacobi rotation of JacobiImpl_<float> on the pivot (K, L), K < L: only the upper triangle of A is read and written
template <int K, int L>
__host__ __device__ __forceinline__ void sim3_jacobi_rotate(float (&A)[4][4], float (&V)[4][4], float (&e)[4]) {
    const float p = A[K][L];
    const float y = (e[L] - e[K]) * 0.5f;
    float t = fabsf(y) + cv_hypot_lapack(p, y);
    float s = cv_hypot_lapack(p, t);
    const float c = t / s;
    s = p / s; t = (p / t) * p;
    if (y < 0) { s = -s; t = -t; }
    A[K][L] = 0;
    e[K] -= t; e[L] += t;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i < K) sim3_rot(A[i][K], A[i][L], c, s);
        else if (i > K && i < L) sim3_rot(A[K][i], A[i][L], c, s);
        else if (i > L) sim3_rot(A[K][i], A[L][i], c, s);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) sim3_rot(V[K][i], V[L][i], c, s);
}
// cv::eigen(N, eval, evec) of a symmetric 4x4 CV_32F as far as evec.row(0) goes: JacobiImpl_<float> (modules/core/src/lapack.cpp) --
//   * V = identity, e = the diagonal; at most n*n*30 = 480 rotations;
//   * the pivot is the largest |A[k][l]|, k < l (OpenCV keeps per-row and per-column maxima to find it; here the six elements are
//     scanned in row-major order and the FIRST largest wins: ties are part of what is unpinned); the loop ends when |pivot| <= FLT_EPSILON;
//   * y = (e[l] - e[k]) / 2, t = |y| + hypot(p, y), s = hypot(p, t), c = t / s, s = p / s, t = (p / t) * p, both negated for y < 0;
//     e[k] -= t, e[l] += t, the rotation (a*c - b*s, a*s + b*c) of the rows / columns of A's upper triangle and of the rows k, l of V;
//   * the eigenvalues are sorted descending by a selection sort with strict `e[m] < e[i]`, rows of V following: row 0 is the row of the
//     first largest eigenvalue, the only one ComputeSim3 reads.
// The pivot pair is a run-time value, the indices are not: a switch over the six pairs, each arm with compile-time indices.
__host__ __device__ inline void sim3_cv_eigen_row0(float (&A)[4][4], float* q) {
    float V[4][4], e[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0f : 0.0f;
        e[i] = A[i][i];
    }
    for (int iter = 0; iter < 480; ++iter) {
        int pair = 0;
        float mv = fabsf(A[0][1]), v;
        v = fabsf(A[0][2]); if (mv < v) { mv = v; pair = 1; }
        v = fabsf(A[0][3]); if (mv < v) { mv = v; pair = 2; }
        v = fabsf(A[1][2]); if (mv < v) { mv = v; pair = 3; }
        v = fabsf(A[1][3]); if (mv < v) { mv = v; pair = 4; }
        v = fabsf(A[2][3]); if (mv < v) { mv = v; pair = 5; }
        if (mv <= FLT_EPSILON) break;
        switch (pair) {
        case 0: sim3_jacobi_rotate<0, 1>(A, V, e); break;
        case 1: sim3_jacobi_rotate<0, 2>(A, V, e); break;
        case 2: sim3_jacobi_rotate<0, 3>(A, V, e); break;
        case 3: sim3_jacobi_rotate<1, 2>(A, V, e); break;
        case 4: sim3_jacobi_rotate<1, 3>(A, V, e); break;
        default: sim3_jacobi_rotate<2, 3>(A, V, e); break;
        }
    }
    int m = 0;
    float em = e[0];
#pragma unroll
    for (int i = 1; i < 4; ++i) if (em < e[i]) { em = e[i]; m = i; }
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = m == 0 ? V[0][k] : m == 1 ? V[1][k] : m == 2 ? V[2][k] : V[3][k];
}

// (the atan2 of ORBM_SIM3_MATH_DEVICE, sim3_atan2, lives in sincos_dev.h since the essential graph's arc cosine is built on it)

// cv::Rodrigues of a 1x3 CV_32F into a 3x3 CV_32F (cvRodrigues2, modules/calib3d/src/calibration.cpp): double inside; theta = the norm;
// below DBL_EPSILON the identity; else c = cos, s = sin, c1 = 1 - c, r *= 1 / theta, R = c*I + c1*r*r^T + s*[r]x summed left to right,
// rounded to float.  math: where sin and cos come from.
__host__ __device__ inline void sim3_cv_rodrigues(const float* vec, int math, float* R) {
    double rx = (double)vec[0], ry = (double)vec[1], rz = (double)vec[2];
    const double theta = sqrt(rx * rx + ry * ry + rz * rz);
    if (theta < DBL_EPSILON) {
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = k % 4 == 0 ? 1.0f : 0.0f;
        return;
    }
    double c, s;
#ifndef __HIP_DEVICE_COMPILE__
    if (math == ORBM_SIM3_MATH_LIBM) { c = cos(theta); s = sin(theta); } else
#endif
    pose_sincos(theta, &s, &c);
    const double c1 = 1. - c, itheta = theta ? 1. / theta : 0.;
    rx *= itheta; ry *= itheta; rz *= itheta;
    const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
    const double r_x[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = (float)((c * (k % 4 == 0 ? 1.0 : 0.0) + c1 * rrt[k]) + s * r_x[k]);
}

// ---- one hypothesis: ComputeCentroid + ComputeSim3 (:275-407) ---------------------------------------------------------------------------
// P1, P2: P3Dc1i, P3Dc2i as [row x y z][column = point of the triple]
__host__ __device__ inline void sim3_horn(const float (&P1)[3][3], const float (&P2)[3][3], bool fix_scale, int math, orbm_sim3_hyp& o) {
    // Step 1: centroids and relative coordinates
    float Pr1[3][3], Pr2[3][3], O1[3], O2[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        O1[r] = cv_scale(cv_reduce_row(P1[r][0], P1[r][1], P1[r][2]), 1. / 3);
        O2[r] = cv_scale(cv_reduce_row(P2[r][0], P2[r][1], P2[r][2]), 1. / 3);
#pragma unroll
        for (int i = 0; i < 3; ++i) { Pr1[r][i] = P1[r][i] - O1[r]; Pr2[r][i] = P2[r][i] - O2[r]; }
    }
    // Step 2: M = Pr2 * Pr1.t()
    float M[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) M[i][j] = cv_gemm3_bt(Pr2[i], Pr1[j]);
    // Step 3: N -- the sums are float expressions assigned to doubles and stored as floats again
    float N[4][4];
    N[0][0] = (M[0][0] + M[1][1]) + M[2][2];
    N[0][1] = M[1][2] - M[2][1];
    N[0][2] = M[2][0] - M[0][2];
    N[0][3] = M[0][1] - M[1][0];
    N[1][1] = (M[0][0] - M[1][1]) - M[2][2];
    N[1][2] = M[0][1] + M[1][0];
    N[1][3] = M[2][0] + M[0][2];
    N[2][2] = (-M[0][0] + M[1][1]) - M[2][2];
    N[2][3] = M[1][2] + M[2][1];
    N[3][3] = (-M[0][0] - M[1][1]) + M[2][2];
    N[1][0] = N[0][1]; N[2][0] = N[0][2]; N[3][0] = N[0][3]; N[2][1] = N[1][2]; N[3][1] = N[1][3]; N[3][2] = N[2][3];
    // Step 4: the eigenvector of the highest eigenvalue, angle-axis, rotation
    float q[4];
    sim3_cv_eigen_row0(N, q);
    float vec[3] = {q[1], q[2], q[3]};
    const double nrm = cv_norm3(vec);
    double ang;
#ifndef __HIP_DEVICE_COMPILE__
    if (math == ORBM_SIM3_MATH_LIBM) ang = atan2(nrm, (double)q[0]); else
#endif
    ang = sim3_atan2(nrm, (double)q[0]);
    const double w = (2 * ang) * (1. / nrm);             // `2*ang*vec/norm(vec)`: one scaled matrix with the weights multiplied
#pragma unroll
    for (int k = 0; k < 3; ++k) vec[k] = cv_scale(vec[k], w);
    float R[9];
    sim3_cv_rodrigues(vec, math, R);
    // Step 5: P3 = mR12i * Pr2
    float P3[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) P3[i][j] = cv_gemm3(R[3 * i], R[3 * i + 1], R[3 * i + 2], Pr2[0][j], Pr2[1][j], Pr2[2][j], 1.0, 0.0f, 0.0);
    // Step 6: scale -- Mat::dot and the den loop accumulate in double in element order, cv::pow(., 2) squares in float
    float ms = 1.0f;
    if (!fix_scale) {
        double nom = 0, den = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                nom += (double)Pr1[i][j] * (double)P3[i][j];
                const float sq = P3[i][j] * P3[i][j];
                den += (double)sq;
            }
        ms = (float)(nom / den);
    }
    // Step 7: mt12i = O1 - ms12i*mR12i*O2: one gemm, alpha = -ms12i, C = O1, beta = 1
    const double s = (double)ms;
    float t[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = cv_gemm3(R[3 * i], R[3 * i + 1], R[3 * i + 2], O2[0], O2[1], O2[2], -s, O1[i], 1.0);
    // Step 8: mT12i = [ms12i*mR12i | mt12i], mT21i = [sRinv | -sRinv*mt12i] with sRinv = (1.0/ms12i)*mR12i.t()
    const double is = 1.0 / s;
    float sRinv[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            o.T12[4 * i + j] = x86_nan(cv_scale(R[3 * i + j], s));
            sRinv[i][j] = cv_scale_t(R[3 * j + i], is);
            o.T21[4 * i + j] = x86_nan(sRinv[i][j]);
            o.R12[3 * i + j] = x86_nan(R[3 * i + j]);
        }
        o.T12[4 * i + 3] = x86_nan(t[i]);
        o.t12[i] = x86_nan(t[i]);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) o.T21[4 * i + 3] = x86_nan(cv_gemm3(sRinv[i][0], sRinv[i][1], sRinv[i][2], t[0], t[1], t[2], -1.0, 0.0f, 0.0));
    o.T12[12] = 0.0f; o.T12[13] = 0.0f; o.T12[14] = 0.0f; o.T12[15] = 1.0f;
    o.T21[12] = 0.0f; o.T21[13] = 0.0f; o.T21[14] = 0.0f; o.T21[15] = 1.0f;
    o.s12 = x86_nan(ms);
    o.n_inliers = 0;
}

// ---- one correspondence under one hypothesis ---------------------------------------------------------------------------------------------
// FromCameraToImage (:491-522): the point's own image position
__host__ __device__ inline void sim3_to_image(float X, float Y, float Z, float fx, float fy, float cx, float cy, float* u, float* v) {
    const float invz = 1 / Z;
    const float x = X * invz, y = Y * invz;
    *u = fx * x + cx; *v = fy * y + cy;
}
// Project (:459-487): Rcw*P + tcw out of the rows of T, the second camera's Rcam21*P + tcam21 for camIdxs[i] == 1, the pinhole
__host__ __device__ inline void sim3_project(const float* T, const orbm_sim3_problem& P, bool second, float X, float Y, float Z, float fx, float fy,
                                             float cx, float cy, float* u, float* v) {
    float p0 = cv_gemm3(T[0], T[1], T[2], X, Y, Z, 1.0, T[3], 1.0);
    float p1 = cv_gemm3(T[4], T[5], T[6], X, Y, Z, 1.0, T[7], 1.0);
    float p2 = cv_gemm3(T[8], T[9], T[10], X, Y, Z, 1.0, T[11], 1.0);
    if (second) {
        const float c0 = cv_gemm3(P.Rcam21[0], P.Rcam21[1], P.Rcam21[2], p0, p1, p2, 1.0, P.tcam21[0], 1.0);
        const float c1 = cv_gemm3(P.Rcam21[3], P.Rcam21[4], P.Rcam21[5], p0, p1, p2, 1.0, P.tcam21[1], 1.0);
        const float c2 = cv_gemm3(P.Rcam21[6], P.Rcam21[7], P.Rcam21[8], p0, p1, p2, 1.0, P.tcam21[2], 1.0);
        p0 = c0; p1 = c1; p2 = c2;
    }
    sim3_to_image(p0, p1, p2, fx, fy, cx, cy, u, v);
}
// CheckInliers (:411-438) for correspondence i: X1 = mvX3Dc1[i], X2 = mvX3Dc2[i]; cams: bit 0 camIdx1[i] == 1, bit 1 camIdx2[i] == 1.
// dist.dot(dist) accumulates in double and is rounded to the float err.
__host__ __device__ inline bool sim3_inlier(const orbm_sim3_problem& P, const float* T12, const float* T21, const float* X1, const float* X2, int cams,
                                            float max_err1, float max_err2) {
    float u1, v1, u2, v2, pu, pv;
    sim3_to_image(X1[0], X1[1], X1[2], P.fx1, P.fy1, P.cx1, P.cy1, &u1, &v1);          // mvP1im1[i]
    sim3_to_image(X2[0], X2[1], X2[2], P.fx2, P.fy2, P.cx2, P.cy2, &u2, &v2);          // mvP2im2[i]
    sim3_project(T12, P, (cams & 2) != 0, X2[0], X2[1], X2[2], P.fx1, P.fy1, P.cx1, P.cy1, &pu, &pv);   // vP2im1[i]
    const float d10 = u1 - pu, d11 = v1 - pv;
    sim3_project(T21, P, (cams & 1) != 0, X1[0], X1[1], X1[2], P.fx2, P.fy2, P.cx2, P.cy2, &pu, &pv);   // vP1im2[i]
    const float d20 = pu - u2, d21 = pv - v2;
    const float err1 = (float)((double)d10 * (double)d10 + (double)d11 * (double)d11);
    const float err2 = (float)((double)d20 * (double)d20 + (double)d21 * (double)d21);
    return err1 < max_err1 && err2 < max_err2;
}

// ---- the kernels ------------------------------------------------------------------------------------------------------------------------
struct Sim3Dev {
    const orbm_sim3_problem* prob;     // per problem
    const int32_t* first;              // CSR of the correspondences, per problem + 1
    const int32_t* its_first;          // CSR of the hypotheses, per problem + 1
    const int32_t* mask_first;         // first mask word of every problem
    const int32_t* hyp_prob;           // per hypothesis: its problem, or -1 when the host routine takes that problem
    const int32_t* triples;            // per hypothesis: three positions inside the problem
    const float* x1; const float* y1; const float* z1; const float* x2; const float* y2; const float* z2;   // structure of arrays
    const float* e1; const float* e2; const int32_t* cams;
    int n_hyp;
    orbm_sim3_hyp* rec_dev;            // HBM: read by k_sim3_inliers
    orbm_sim3_hyp* rec_out;            // mapped pinned
    uint64_t* mask_out;                // mapped pinned
};

__global__ __launch_bounds__(SIM3_T) void k_sim3_hyp(Sim3Dev A) {
    const int g = blockIdx.x * SIM3_T + threadIdx.x;
    if (g >= A.n_hyp) return;
    const int b = A.hyp_prob[g];
    if (b < 0) return;
    const int n0 = A.first[b];
    float P1[3][3], P2[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int c = n0 + A.triples[3 * (size_t)g + i];   // (validated on the host: inside the problem)
        P1[0][i] = A.x1[c]; P1[1][i] = A.y1[c]; P1[2][i] = A.z1[c];
        P2[0][i] = A.x2[c]; P2[1][i] = A.y2[c]; P2[2][i] = A.z2[c];
    }
    orbm_sim3_hyp o;
    sim3_horn(P1, P2, A.prob[b].fix_scale != 0, ORBM_SIM3_MATH_DEVICE, o);
    A.rec_dev[g] = o;
    A.rec_out[g] = o;
}

__global__ __launch_bounds__(SIM3_T) void k_sim3_inliers(Sim3Dev A) {
    const int g = blockIdx.x;
    const int lane = threadIdx.x;
    const int b = A.hyp_prob[g];
    if (b < 0) return;
    const orbm_sim3_problem P = A.prob[b];
    const int n0 = A.first[b];
    const int n = A.first[b + 1] - n0;
    const orbm_sim3_hyp& rec = A.rec_dev[g];
    float T12[12], T21[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) { T12[k] = rec.T12[k]; T21[k] = rec.T21[k]; }
    uint64_t* words = A.mask_out + (size_t)A.mask_first[b] + (size_t)(g - A.its_first[b]) * ransac_words(n);
    const int count = ransac_mask_sweep(n, lane,
        [&](int i) {
            const int k = n0 + i;
            const float X1[3] = {A.x1[k], A.y1[k], A.z1[k]}, X2[3] = {A.x2[k], A.y2[k], A.z2[k]};
            return sim3_inlier(P, T12, T21, X1, X2, A.cams[k], A.e1[k], A.e2[k]);
        },
        [&](int c, unsigned long long word) { words[c] = word; });
    if (lane == 0) A.rec_out[g].n_inliers = count;
}

// ---- host routine -----------------------------------------------------------------------------------------------------------------------
struct Sim3In {
    const orbm_sim3_problem* problems; const int32_t* first; const float* x3dc1; const float* x3dc2; const int32_t* cam1; const int32_t* cam2;
    const float* max_err1; const float* max_err2; const int32_t* its_first; const int32_t* triples;
};

inline int sim3_cams(const Sim3In& I, int k) { return (I.cam1[k] == 1 ? 1 : 0) | (I.cam2[k] == 1 ? 2 : 0); }

// one problem: records hyp[0 .. H-1] and mask words[0 .. H*W-1]
void sim3_problem_host(const Sim3In& I, int b, int math, orbm_sim3_hyp* hyp, uint64_t* words) {
    const orbm_sim3_problem& P = I.problems[b];
    const int n0 = I.first[b], n = I.first[b + 1] - n0, h0 = I.its_first[b], H = I.its_first[b + 1] - h0;
    const int W = ransac_words(n);
    for (int h = 0; h < H; ++h) {
        float P1[3][3], P2[3][3];
        for (int i = 0; i < 3; ++i) {
            const size_t c = (size_t)n0 + I.triples[3 * (size_t)(h0 + h) + i];
            for (int r = 0; r < 3; ++r) { P1[r][i] = I.x3dc1[3 * c + r]; P2[r][i] = I.x3dc2[3 * c + r]; }
        }
        orbm_sim3_hyp& o = hyp[h];
        sim3_horn(P1, P2, P.fix_scale != 0, math, o);
        o.n_inliers = ransac_mask_sweep_host(n, words + (size_t)h * W, [&](int i) {
            const size_t k = (size_t)n0 + i;
            return sim3_inlier(P, o.T12, o.T21, I.x3dc1 + 3 * k, I.x3dc2 + 3 * k, sim3_cams(I, (int)k), I.max_err1[k], I.max_err2[k]);
        });
    }
}

// Argument checks; mask_first[b] = the first mask word of problem b, mask_first[B] = all of them.
int validate(const Sim3In& I, int B, const orbm_sim3_hyp* hyp_out, const uint64_t* mask_out, std::vector<int32_t>& mask_first) {
    MORB_ARG(I.problems != nullptr);
    if (const int rc = ransac_validate<3>(B, ORBM_SIM3_MAX_BATCH, ORBM_SIM3_MAX_ITS, I.first, I.its_first, I.triples, hyp_out, mask_out, mask_first)) return rc;
    if (I.first[B] > 0 && !(I.x3dc1 && I.x3dc2 && I.cam1 && I.cam2 && I.max_err1 && I.max_err2)) { morb::set_error("a correspondence array is NULL"); return ORB_E_ARG; }
    return ORB_OK;
}

}  // namespace

extern "C" {

double orbm_sim3_atan2(double y, double x) { return sim3_atan2(y, x); }

int orbm_sim3_ransac_host(const orbm_sim3_problem* problems, int B, const int32_t* first, const float* x3dc1, const float* x3dc2,
                          const int32_t* cam1, const int32_t* cam2, const float* max_err1, const float* max_err2,
                          const int32_t* its_first, const int32_t* triples, int order, orbm_sim3_hyp* hyp_out, uint64_t* mask_out) {
    const Sim3In I = {problems, first, x3dc1, x3dc2, cam1, cam2, max_err1, max_err2, its_first, triples};
    std::vector<int32_t> mask_first;
    int rc = validate(I, B, hyp_out, mask_out, mask_first);
    if (rc) return rc;
    if (order != ORBM_SIM3_MATH_LIBM && order != ORBM_SIM3_MATH_DEVICE) { morb::set_error("order = %d", order); return ORB_E_ARG; }
    for (int b = 0; b < B; ++b) sim3_problem_host(I, b, order, hyp_out + its_first[b], mask_out + mask_first[b]);
    return ORB_OK;
}

int orbm_sim3_ransac(orbm_matcher* m, const orbm_sim3_problem* problems, int B, const int32_t* first, const float* x3dc1,
                     const float* x3dc2, const int32_t* cam1, const int32_t* cam2, const float* max_err1, const float* max_err2,
                     const int32_t* its_first, const int32_t* triples, orbm_sim3_hyp* hyp_out, uint64_t* mask_out) {
    MORB_ARG(m != nullptr);
    const Sim3In I = {problems, first, x3dc1, x3dc2, cam1, cam2, max_err1, max_err2, its_first, triples};
    std::vector<int32_t> mask_first;
    if (const int rc = validate(I, B, hyp_out, mask_out, mask_first)) return rc;
    const int N = first[B], HT = its_first[B];
    // a problem goes to the device when it has at most ORBM_SIM3_CAP correspondences; the others to the host routine in DEVICE order
    return ransac_csr_call(m, m->sim3, B, first, its_first, mask_first, ORBM_SIM3_CAP, hyp_out, mask_out, m->last_sim3,
        [&](const std::vector<int32_t>& hyp_prob, size_t* o_mask) -> int {
            morb::StagePack pk;
            const int i_prob = pk.add(problems, (size_t)B * sizeof(orbm_sim3_problem)), i_first = pk.add(first, (size_t)(B + 1) * 4),
                      i_its = pk.add(its_first, (size_t)(B + 1) * 4), i_mf = pk.add(mask_first.data(), (size_t)(B + 1) * 4),
                      i_hp = pk.add(hyp_prob.data(), (size_t)HT * 4), i_tri = pk.add(triples, (size_t)HT * 12);
            int i_soa[8];                                      // x1 y1 z1 x2 y2 z2 e1 e2, transposed below
            for (int k = 0; k < 8; ++k) i_soa[k] = pk.add_in_place((size_t)N * 4);
            const int i_cams = pk.add_in_place((size_t)N * 4);
            *o_mask = morb::align16((size_t)HT * sizeof(orbm_sim3_hyp));
            const size_t out_bytes = *o_mask + (size_t)mask_first[B] * 8 + 16;
            int rc;
            const morb::StagePack::Block blk = pk.open(m->sim3.stage, &rc);
            if (rc || (rc = m->sim3.scratch.reserve((size_t)HT * sizeof(orbm_sim3_hyp))) || (rc = m->sim3.out.reserve(out_bytes))) return rc;
            float* soa[8];
            for (int k = 0; k < 8; ++k) soa[k] = blk.host<float>(i_soa[k]);
            int32_t* cams = blk.host<int32_t>(i_cams);
            for (int k = 0; k < N; ++k) {                      // array of structures -> structure of arrays, once per call
                soa[0][k] = x3dc1[3 * (size_t)k]; soa[1][k] = x3dc1[3 * (size_t)k + 1]; soa[2][k] = x3dc1[3 * (size_t)k + 2];
                soa[3][k] = x3dc2[3 * (size_t)k]; soa[4][k] = x3dc2[3 * (size_t)k + 1]; soa[5][k] = x3dc2[3 * (size_t)k + 2];
                soa[6][k] = max_err1[k]; soa[7][k] = max_err2[k];
                cams[k] = sim3_cams(I, k);
            }
            blk.publish();
            Sim3Dev A;
            A.prob = blk.dev<orbm_sim3_problem>(i_prob); A.first = blk.dev<int32_t>(i_first); A.its_first = blk.dev<int32_t>(i_its);
            A.mask_first = blk.dev<int32_t>(i_mf); A.hyp_prob = blk.dev<int32_t>(i_hp); A.triples = blk.dev<int32_t>(i_tri);
            A.x1 = blk.dev<float>(i_soa[0]); A.y1 = blk.dev<float>(i_soa[1]); A.z1 = blk.dev<float>(i_soa[2]);
            A.x2 = blk.dev<float>(i_soa[3]); A.y2 = blk.dev<float>(i_soa[4]); A.z2 = blk.dev<float>(i_soa[5]);
            A.e1 = blk.dev<float>(i_soa[6]); A.e2 = blk.dev<float>(i_soa[7]); A.cams = blk.dev<int32_t>(i_cams);
            A.n_hyp = HT;
            A.rec_dev = (orbm_sim3_hyp*)m->sim3.scratch.p;
            A.rec_out = (orbm_sim3_hyp*)m->sim3.out.dp;
            A.mask_out = (uint64_t*)(m->sim3.out.dp + *o_mask);
            hipLaunchKernelGGL(k_sim3_hyp, dim3((unsigned)((HT + SIM3_T - 1) / SIM3_T)), dim3(SIM3_T), 0, m->stream, A);
            hipLaunchKernelGGL(k_sim3_inliers, dim3((unsigned)HT), dim3(SIM3_T), 0, m->stream, A);
            MORB_HIP(hipGetLastError());
            return ORB_OK;
        },
        [&](int b) { sim3_problem_host(I, b, ORBM_SIM3_MATH_DEVICE, hyp_out + its_first[b], mask_out + mask_first[b]); },
        [](int) {});
}

int orbm_sim3_walk(const int32_t* counts, int H, int N, int min_inliers, int start_iteration, int n_iterations, orbm_sim3_walk_state* state) {
    if (!state || (H > 0 && !counts)) return -1;
    state->no_more = 0;
    state->iterations = start_iteration;
    if (N < min_inliers) { state->no_more = 1; return -1; }        // `if(N<mRansacMinInliers)`
    int current = 0;
    while (state->iterations < H && current < n_iterations) {
        current++;
        const int h = state->iterations++;
        const int n = counts[h];
        if (n >= state->best_inliers) {
            state->best_inliers = n;
            state->best_index = h;
            if (n > min_inliers) return h;
        }
    }
    if (state->iterations >= H) state->no_more = 1;
    return -1;
}

int orbm_sim3_iterations(double probability, int min_inliers, int max_its, int N) {
    return ransac_iterations(probability, (float)min_inliers / N, max_its, min_inliers == N);
}

}  // extern "C"
