// lba_dev.h -- what the kernels of lba.hip and its host routine share, ONE definition each: local bundle adjustment,
// Optimizer::LocalBundleAdjustment (reference src/Optimizer.cc:921-1353) from the graph on, with the parts of g2o it runs restated
// (Thirdparty/g2o/g2o/: types/types_six_dof_expmap.{h,cpp}, core/base_binary_edge.hpp, core/block_solver.hpp,
// core/optimization_algorithm_levenberg.cpp, core/sparse_optimizer.cpp).
//   lba_edge          computeError, chi2, isDepthPositive's depth and linearizeOplus of EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ
//   lba_edge_blocks   the robust / plain constructQuadraticForm of a binary edge: its blocks of Hll, Hpl, Hpp, bl, bp
//   lba_point_damp    setLambda on a landmark block, Dinv = D.inverse(), db = Dinv * db (block_solver.hpp:381-395)
//   lba_pose_oplus    oplus of a pose vertex
// (the steps over the whole graph -- the sums per vertex, the Schur entries, the landmarks' back-substitution -- are lba.hip's)
//   LbaCtl, lba_ctl_* the Levenberg controller's driver for a vector of unknowns: lm_dev.h's rules (lm_rule_full, lm_rule_trial,
//                     lm_rule_iter_end, the ones lm_step runs) cut where g2o polls the stop flag (the host polls), with what is this
//                     port's own: the stage, the choice of estimate buffer, the words for the host.  A test holds this driver and
//                     lm_step to one lambda / ni / verdict sequence.
// What is g2o's and not this port's -- the edges' Jacobian chain, the Huber constants, SE3Quat to and from seven doubles -- is g2o_dev.h's.
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
#include "lm_dev.h"

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
    g2o_huber_constants(C.delta, C.dsqr);
}

struct LbaEval { double e[3], chi2, zc, A[3][3], B[3][6]; };   // _error, chi2(), the depth, _jacobianOplusXi (point), _jacobianOplusXj (pose)

// One edge at pose T (7 doubles: q x y z w, t) and point X.  K5: fx fy cx cy bf of the edge's keyframe as the floats the reference
// assigns to the edge's double members.  JAC: also linearizeOplus (types_six_dof_expmap.cpp:103-218, :318-461).
template <bool JAC>
__host__ __device__ __forceinline__ void lba_edge(const LbaCam& C, const float* K5, const double* T7, const double* X, int cam, bool stereo,
                                                  const float* obs, double w, LbaEval& o) {
    SE3Quat T;
    se3_load7(T7, T);
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
        // the one term where this edge and pose.hip's pose_edge differ: here `bf*invz` is a FLOAT product (cam_project takes
        // `const float& bf`), there a double one with the member: two reference functions, not to be merged
        const double r2 = r0 - (double)(K5[4] * invz);
        o.e[0] = (double)obs[0] - r0; o.e[1] = (double)obs[1] - r1; o.e[2] = (double)obs[2] - r2;
        o.chi2 = (o.e[0] * (w * o.e[0]) + o.e[1] * (w * o.e[1])) + o.e[2] * (w * o.e[2]);
    }
    if (!JAC) return;
    double rm[9];
    eigen_quat_to_matrix(T.q, rm);                       // T.rotation().toRotationMatrix()
    double t2[3][3];
    g2o_cam_jacobian_rows(fx, fy, bf, C.Rc[cam], pc, stereo, t2);
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
        g2o_cam_jacobian_pose(t2[k], p, o.B[k]);
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
    se3_load7(est7, E);
    se3_exp(x6, order, d);
    se3_mul(d, E, T);
    se3_store7(T, out7);
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
// after a trial's computeActiveErrors; scale: computeScale() over all of x.  Accepting is a choice of buffer (discardTop: the trial is the
// estimate).  Leaves want_trial = `rho<0 && qmax < 10`: the caller polls the stop flag before the next trial.
__host__ __device__ inline void lba_ctl_trial_end(LbaCtl& S, double temp_chi, double scale) {
    const LmTrial t = lm_rule_trial(S, temp_chi, scale, S.round[S.stage]);
    if (t.accepted) S.cur ^= 1;
    S.rho = t.rho;
    S.want_trial = (t.rho < 0 && S.qmax < 10) ? 1 : 0;
}
// the trial loop is over (by its own condition or by the stop flag).  Leaves more = `i < iterations` and ok = `result == OK`; the caller
// polls the stop flag when more is set, before it reads ok.
__host__ __device__ inline void lba_ctl_iter_end(LbaCtl& S) {
    orbm_pose_round& R = S.round[S.stage];
    S.ok = lm_rule_iter_end(S, S.rho, R) ? 0 : 1;
    S.more = S.iter < S.max_iter ? 1 : 0;
    S.want_trial = 0;
    R.chi2 = x86_nan(S.current_chi); R.lambda = x86_nan(S.lambda);
}
