// lba_dev.h -- what the kernels of lba.hip and its host routine share, ONE definition each: local bundle adjustment,
// Optimizer::LocalBundleAdjustment (reference src/Optimizer.cc:921-1353) from the graph on, with the parts of g2o it runs restated
// (Thirdparty/g2o/g2o/: types/types_six_dof_expmap.{h,cpp}, core/base_binary_edge.hpp, core/block_solver.hpp,
// core/optimization_algorithm_levenberg.cpp, core/sparse_optimizer.cpp).
//   lba_edge          computeError, chi2, isDepthPositive's depth and linearizeOplus of EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ
//   lba_edge_blocks   the robust / plain constructQuadraticForm of a binary edge: its blocks of Hll, Hpl, Hpp, bl, bp
//   lba_point_damp    setLambda on a landmark block, Dinv = D.inverse(), db = Dinv * db (block_solver.hpp:381-395)
//   lba_pose_oplus    oplus of a pose vertex
// (the steps over the whole graph -- the sums per vertex, the Schur entries, the landmarks' back-substitution -- are lba.hip's)
//   LbaCtl, lba_ctl_* the Levenberg controller: the statements of lm_dev.h's lm_step for a vector of unknowns, cut where g2o polls the
//                     stop flag (the host polls; tests hold both controllers to one lambda / ni / verdict sequence)
// Stated deviations (include/orbm.h): (a) the reduced system is solved by a dense LDL^T without pivoting in the natural
// order of the free poses, not by Eigen's SimplicialLDLT behind an AMD ordering; (b) the order of a point's observations is the
// caller's.  Everything g2o_dev.h marks UNPINNED is unpinned here too, eigen_inverse3 and the order inside Eigen's small products
// (taken as ascending index) included.
#pragma once
#include <cfloat>
#include <cmath>
#include <hip/hip_runtime.h>
#include "../../include/orbm.h"
#include "cv_dev.h"   // x86_nan
#include "g2o_dev.h"

constexpr int LBA_T = 256;            // lanes of a workgroup of the per-edge kernels = leaves of one chi2 partial (lm_dev.h's tree)
constexpr int LBA_EDGE_DOUBLES = 72;  // what a linearised edge leaves in HBM, structure of arrays: array k of edge e is at k * n_edges + e
enum { LBA_HPP = 0, LBA_HPL = 36, LBA_HLL = 54, LBA_BP = 63, LBA_BL = 69 };   // Hpp 6x6, Hpl 6x3, Hll 3x3 (row-major), bp 6, bl 3

struct LbaCam {                          // per problem
    SE3Quat Tc[2];                       // Tcim[cam] (:1048-1061)
    double Rc[2][9];                     // Tcim_quat.to_homogeneous_matrix().block(0,0,3,3)
    double delta[2], dsqr[2];            // RobustKernelHuber::_delta and dsqr (a FLOAT member) of a mono / stereo edge
};
__host__ __device__ inline void lba_camera(const float (*Tcim)[16], LbaCam& C) {
    for (int c = 0; c < 2; ++c) { se3_from_cv(Tcim[c], C.Tc[c]); eigen_quat_to_matrix(C.Tc[c].q, C.Rc[c]); }
    // `const float thHuberMono = sqrt(5.991)`, `thHuberStereo = sqrt(7.815)`; rk->setDelta(th)
    const float th[2] = {(float)sqrt(5.991), (float)sqrt(7.815)};
    for (int s = 0; s < 2; ++s) { C.delta[s] = (double)th[s]; C.dsqr[s] = (double)(float)(C.delta[s] * C.delta[s]); }
}

struct LbaEval { double e[3], chi2, zc, A[3][3], B[3][6]; };   // _error, chi2(), the depth, _jacobianOplusXi (point), _jacobianOplusXj (pose)

// One edge at pose T (7 doubles: q x y z w, t) and point X.  K5: fx fy cx cy bf of the edge's keyframe as the floats the reference
// assigns to the edge's double members.  JAC: also linearizeOplus (types_six_dof_expmap.cpp:103-218, :318-461).
template <bool JAC>
__host__ __device__ __forceinline__ void lba_edge(const LbaCam& C, const float* K5, const double* T7, const double* X, int cam, bool stereo,
                                                  const float* obs, double w, LbaEval& o) {
    SE3Quat T;
    T.q[0] = T7[0]; T.q[1] = T7[1]; T.q[2] = T7[2]; T.q[3] = T7[3]; T.t[0] = T7[4]; T.t[1] = T7[5]; T.t[2] = T7[6];
    const double fx = (double)K5[0], fy = (double)K5[1], cx = (double)K5[2], cy = (double)K5[3], bf = (double)K5[4];
    double p[3], pc[3];
    se3_map(T, X, p);                                    // v1->estimate().map(v2->estimate())
    se3_map(C.Tc[cam], p, pc);                           // Tcim_quat.map(...)
    o.zc = pc[2];
    if (!stereo) {
        const double proj0 = pc[0] / pc[2], proj1 = pc[1] / pc[2];            // project2d
        o.e[0] = (double)obs[0] - (proj0 * fx + cx);
        o.e[1] = (double)obs[1] - (proj1 * fy + cy);
        o.e[2] = 0.0;
        o.chi2 = o.e[0] * (w * o.e[0]) + o.e[1] * (w * o.e[1]);
    } else {
        const float invz = (float)(1.0 / pc[2]);                               // `const float invz = 1.0f/trans_xyz[2]`
        const double r0 = pc[0] * (double)invz * fx + cx;
        const double r1 = pc[1] * (double)invz * fy + cy;
        const double r2 = r0 - (double)(K5[4] * invz);                         // `bf*invz`: bf arrives as `const float&`, a float product
        o.e[0] = (double)obs[0] - r0; o.e[1] = (double)obs[1] - r1; o.e[2] = (double)obs[2] - r2;
        o.chi2 = (o.e[0] * (w * o.e[0]) + o.e[1] * (w * o.e[1])) + o.e[2] * (w * o.e[2]);
    }
    if (!JAC) return;
    double rm[9];
    eigen_quat_to_matrix(T.q, rm);                       // T.rotation().toRotationMatrix()
    const double* r = C.Rc[cam];
    const double x = p[0], y = p[1], z = p[2];
    const double xc = pc[0], yc = pc[1], zc = pc[2], zc_2 = zc * zc;
    double t1[3][3], t2[3][3];
    t1[0][0] = -fx / zc; t1[0][1] = 0; t1[0][2] = fx * xc / zc_2;
    t1[1][0] = 0; t1[1][1] = -fy / zc; t1[1][2] = fy * yc / zc_2;
    t2[0][0] = t1[0][0] * r[0] + t1[0][2] * r[6];
    t2[0][1] = t1[0][0] * r[1] + t1[0][2] * r[7];
    t2[0][2] = t1[0][0] * r[2] + t1[0][2] * r[8];
    t2[1][0] = t1[1][1] * r[3] + t1[1][2] * r[6];
    t2[1][1] = t1[1][1] * r[4] + t1[1][2] * r[7];
    t2[1][2] = t1[1][1] * r[5] + t1[1][2] * r[8];
    if (stereo) {
        const double a1 = bf / zc_2;
        t2[2][0] = t2[0][0] - a1 * r[6];
        t2[2][1] = t2[0][1] - a1 * r[7];
        t2[2][2] = t2[0][2] - a1 * r[8];
    } else { t2[2][0] = 0; t2[2][1] = 0; t2[2][2] = 0; }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (k == 2 && !stereo) {
#pragma unroll
            for (int c = 0; c < 3; ++c) o.A[2][c] = 0;
#pragma unroll
            for (int c = 0; c < 6; ++c) o.B[2][c] = 0;
            continue;
        }
        o.A[k][0] = t2[k][0] * rm[0] + t2[k][1] * rm[3] + t2[k][2] * rm[6];
        o.A[k][1] = t2[k][0] * rm[1] + t2[k][1] * rm[4] + t2[k][2] * rm[7];
        o.A[k][2] = t2[k][0] * rm[2] + t2[k][1] * rm[5] + t2[k][2] * rm[8];
        o.B[k][0] = -t2[k][1] * z + t2[k][2] * y;
        o.B[k][1] = t2[k][0] * z - t2[k][2] * x;
        o.B[k][2] = -t2[k][0] * y + t2[k][1] * x;
        o.B[k][3] = t2[k][0];
        o.B[k][4] = t2[k][1];
        o.B[k][5] = t2[k][2];
    }
}

// rho of an edge: with its Huber kernel, or without one (rho[0] = chi2, rho[1] = 1)
__host__ __device__ __forceinline__ void lba_rho(const LbaCam& C, double chi2, bool stereo, bool robust, double* rho0, double* rho1) {
    *rho0 = chi2; *rho1 = 1.;
    if (robust) g2o_huber(chi2, C.delta[stereo ? 1 : 0], C.dsqr[stereo ? 1 : 0], rho0, rho1);
}

// the sum of a product's terms in ascending index: two terms of a mono edge, three of a stereo one
#define LBA_DOT(stereo, a0, b0, a1, b1, a2, b2) ((stereo) ? ((a0) * (b0) + (a1) * (b1)) + (a2) * (b2) : (a0) * (b0) + (a1) * (b1))

// BaseBinaryEdge::constructQuadraticForm (core/base_binary_edge.hpp:55-120): the edge's own blocks, added to the vertices' and the
// solver's by the callers in active-edge order.  omega_r = -omega * _error (times rho[1] behind a kernel); with a kernel every product
// is X^T * weightedOmega * Y, without one AtO = A^T * omega is formed first and the block the edge shares is B^T * AtO^T.  out: the
// edge's slot in the structure of arrays (stride = n_edges); with_pose: the pose is free (`toNotFixed`).
__host__ __device__ __forceinline__ void lba_edge_blocks(const LbaEval& o, double w, double rho1, bool stereo, bool robust, bool with_pose,
                                                         double* out, size_t stride) {
    double omega_r[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { omega_r[k] = -(w * o.e[k]); if (robust) omega_r[k] *= rho1; }
    const double rw = robust ? w * rho1 : w;             // robustInformation: _information * rho[1]
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        out[(LBA_BL + i) * stride] = LBA_DOT(stereo, o.A[0][i], omega_r[0], o.A[1][i], omega_r[1], o.A[2][i], omega_r[2]);
#pragma unroll
        for (int j = 0; j < 3; ++j)
            out[(LBA_HLL + 3 * i + j) * stride] = LBA_DOT(stereo, o.A[0][i] * rw, o.A[0][j], o.A[1][i] * rw, o.A[1][j], o.A[2][i] * rw, o.A[2][j]);
    }
    if (!with_pose) return;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        out[(LBA_BP + r) * stride] = LBA_DOT(stereo, o.B[0][r], omega_r[0], o.B[1][r], omega_r[1], o.B[2][r], omega_r[2]);
#pragma unroll
        for (int c = 0; c < 6; ++c)
            out[(LBA_HPP + 6 * r + c) * stride] = LBA_DOT(stereo, o.B[0][r] * rw, o.B[0][c], o.B[1][r] * rw, o.B[1][c], o.B[2][r] * rw, o.B[2][c]);
#pragma unroll
        for (int c = 0; c < 3; ++c)
            out[(LBA_HPL + 3 * r + c) * stride] = robust
                ? LBA_DOT(stereo, o.B[0][r] * rw, o.A[0][c], o.B[1][r] * rw, o.A[1][c], o.B[2][r] * rw, o.A[2][c])
                : LBA_DOT(stereo, o.B[0][r], o.A[0][c] * w, o.B[1][r], o.A[1][c] * w, o.B[2][r], o.A[2][c] * w);
    }
}

// setLambda on a landmark's block, Dinv = D.inverse(), db = Dinv * db.  Hll: the undamped block (kept: restoreDiagonal is exact).
__host__ __device__ __forceinline__ void lba_point_damp(const double* Hll, const double* bl, double lambda, double* Dinv, double* db) {
    double D[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) D[k] = Hll[k];
    D[0] = D[0] + lambda; D[4] = D[4] + lambda; D[8] = D[8] + lambda;
    eigen_inverse3(D, Dinv);
#pragma unroll
    for (int r = 0; r < 3; ++r) db[r] = (Dinv[3 * r] * bl[0] + Dinv[3 * r + 1] * bl[1]) + Dinv[3 * r + 2] * bl[2];
}

// oplus of a pose vertex: exp(x) * estimate
__host__ __device__ __forceinline__ void lba_pose_oplus(const double* est7, const double* x6, int order, double* out7) {
    SE3Quat E, d, T;
    E.q[0] = est7[0]; E.q[1] = est7[1]; E.q[2] = est7[2]; E.q[3] = est7[3]; E.t[0] = est7[4]; E.t[1] = est7[5]; E.t[2] = est7[6];
    se3_exp(x6, order, d);
    se3_mul(d, E, T);
    out7[0] = T.q[0]; out7[1] = T.q[1]; out7[2] = T.q[2]; out7[3] = T.q[3]; out7[4] = T.t[0]; out7[5] = T.t[1]; out7[6] = T.t[2];
}

// ---- the controller ---------------------------------------------------------------------------------------------------------------------
// optimization_algorithm_levenberg.cpp:61-164 and the loop of SparseOptimizer::optimize (:376-414) between the passes, cut at the polls
// of the stop flag (:149, :376): the caller polls where want_trial / more say so.
struct LbaCtl {
    int order, stage, iter, max_iter, qmax, n_bad_steps, ok2, cur;   // cur: which of the two estimate buffers holds the estimate
    int want_trial, more, ok;
    double lambda, ni, current_chi, ini_chi, rho;
    orbm_pose_round round[2];
};
__host__ __device__ inline void lba_ctl_begin(LbaCtl& S, int order) {
    S.order = order; S.stage = 0; S.iter = 0; S.max_iter = 0; S.qmax = 0; S.n_bad_steps = 0; S.ok2 = 1; S.cur = 0;
    S.want_trial = 0; S.more = 0; S.ok = 1;
    S.lambda = 0; S.ni = 2; S.current_chi = 0; S.ini_chi = 0; S.rho = 0;
    for (int s = 0; s < 2; ++s) { S.round[s].iterations = 0; S.round[s].trials = 0; S.round[s].chi2 = 0; S.round[s].lambda = 0; }
}
__host__ __device__ inline void lba_ctl_begin_optimisation(LbaCtl& S, int stage, int max_iter) {
    S.stage = stage; S.iter = 0; S.max_iter = max_iter; S.ok = 1; S.more = max_iter > 0 ? 1 : 0; S.want_trial = 0;
}
// after computeActiveErrors + buildSystem at the estimate (:75-101); max_diagonal: computeLambdaInit's maximum (read at iteration 0)
__host__ __device__ inline void lba_ctl_full(LbaCtl& S, double chi, double max_diagonal) {
    S.current_chi = chi; S.ini_chi = chi;
    if (S.iter == 0) { S.lambda = 1e-5 * max_diagonal; S.ni = 2; S.n_bad_steps = 0; }
    S.qmax = 0;
}
// after a trial's computeActiveErrors (:123-149); scale: computeScale() over all of x.  Leaves want_trial = `rho<0 && qmax < 10`.
__host__ __device__ inline void lba_ctl_trial_end(LbaCtl& S, double temp_chi, double scale) {
    orbm_pose_round& R = S.round[S.stage];
    if (!S.ok2) temp_chi = DBL_MAX;
    double rho = S.current_chi - temp_chi;
    scale += 1e-3;
    rho /= scale;
    if (rho > 0 && fabs(temp_chi) <= DBL_MAX) {
        const double u = 2 * rho - 1;
        double cube;
#ifndef __HIP_DEVICE_COMPILE__
        if (S.order == ORBM_POSE_ORDER_INDEX) cube = pow(u, 3); else
#endif
        cube = u * u * u;
        double alpha = 1. - cube;
        alpha = alpha < 2. / 3. ? alpha : 2. / 3.;             // (std::min)(alpha, _goodStepUpperScale)
        const double scale_factor = 1. / 3. < alpha ? alpha : 1. / 3.;   // (std::max)(_goodStepLowerScale, alpha)
        S.lambda *= scale_factor;
        S.ni = 2;
        S.current_chi = temp_chi;
        S.cur ^= 1;                          // discardTop: the trial is the estimate
    } else {
        S.lambda *= S.ni;
        S.ni *= 2;                           // pop: the estimate stays
    }
    S.qmax++;
    R.trials++;
    S.rho = rho;
    S.want_trial = (rho < 0 && S.qmax < 10) ? 1 : 0;
}
// the trial loop is over (by its own condition or by the stop flag): solve()'s result and optimize()'s bookkeeping.  Leaves
// more = `i < iterations` and ok = `result == OK`; the caller polls the stop flag when more is set, before it reads ok.
__host__ __device__ inline void lba_ctl_iter_end(LbaCtl& S) {
    orbm_pose_round& R = S.round[S.stage];
    R.iterations++;
    bool terminate = S.qmax == 10 || S.rho == 0;
    if (!terminate) {
        if ((S.ini_chi - S.current_chi) * 1e3 < S.ini_chi) S.n_bad_steps++; else S.n_bad_steps = 0;
        if (S.n_bad_steps >= 3) terminate = true;
    }
    S.iter++;
    S.ok = terminate ? 0 : 1;
    S.more = S.iter < S.max_iter ? 1 : 0;
    S.want_trial = 0;
    R.chi2 = x86_nan(S.current_chi); R.lambda = x86_nan(S.lambda);
}
