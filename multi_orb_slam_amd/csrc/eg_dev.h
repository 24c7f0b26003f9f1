// eg_dev.h -- what the kernels of essgraph.hip and its host routine share, ONE definition each: the essential graph,
// Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:1373-1677) from its graph on, with the parts of g2o it runs restated
// (Thirdparty/g2o/g2o/: types/sim3.h, types/types_seven_dof_expmap.{h,cpp}, core/base_binary_edge.hpp, core/block_solver.hpp).
//   eg_load / eg_store     a g2o::Sim3 as eight doubles: quaternion x y z w, translation, scale
//   eg_perturb             VertexSim3Expmap::oplusImpl on the unit steps of BaseBinaryEdge::linearizeOplus: the 14 perturbed estimates of
//                          a vertex and their inverses
//   eg_error / eg_slot     EdgeSim3::computeError, (C * v0 * v1.inverse()).log(), at the estimates or at one of the 28 perturbations
//   eg_chi2                _error.dot(information() * _error) with information = I, the products by the identity kept
//   eg_AtOB, eg_BtAtOt, eg_b   the blocks of constructQuadraticForm without a robust kernel, entry by entry
//   eg_diag_entry, eg_pair_entry, eg_b_entry   an entry of Hpp / b: its edges' contributions summed in active-edge order from 0.0
//   eg_oplus, eg_correct_point, eg_Tiw   the update of a vertex, step 7 and step 6 of the function
// The products by `information`, which is the identity, are ALL kept (eg_ident_row): 0 * inf and 0 * NaN are NaN, and a sum that ends on
// a -0.0 term differs from the term alone, so no product is dropped on the ground that it is by 0 or by 1.
#pragma once
#include <cfloat>
#include <cmath>
#include <hip/hip_runtime.h>
#include "../../include/orbm.h"
#include "cv_dev.h"   // x86_nan
#include "g2o_dev.h"
#include "lm_dev.h"
#include "lba_dev.h"  // LbaCtl, lba_ctl_*: the Levenberg driver for a vector of unknowns

constexpr int EG_T = 256;             // lanes of a workgroup = leaves of one partial of lm_dev.h's tree
constexpr int EG_SLOTS = 29;          // evaluations of an edge per linearisation: the estimates, 14 steps of vertex 0, 14 of vertex 1
constexpr double EG_DELTA = 1e-9;     // linearizeOplus: delta and scalar = 1 / (2 delta)
constexpr double EG_LAMBDA_INIT = 1e-16;   // solver->setUserLambdaInit(1e-16): computeLambdaInit returns it (levenberg.cpp:166-169)

// Everything a step reads and writes, as raw pointers: the host routine's vectors or the device's buffers.
struct EgView {
    int n_free, n_vertices, n_edges, n_points, fix_scale;
    int na, n_pairs;                  // active free vertices (rows of the system: 7 na), off-diagonal block pairs that have an edge
    const double* meas;               // n_edges x 8
    const int32_t* ev0; const int32_t* ev1;
    const int32_t* hidx;              // per vertex: its hessian index, -1: fixed or without an edge
    const int32_t* act;               // na: the vertex of a hessian index
    const int32_t* vfirst; const int32_t* vedge;   // per hessian index: its incident edges in edge order
    const int32_t* pairs;             // n_pairs x 2: i1 < i2, sorted
    const int32_t* pfirst; const int32_t* pedge;   // per pair: its edges in edge order
    double* est[2];                   // n_vertices x 8: the estimate and the trial (LbaCtl::cur says which is which)
    double* pert;                     // na x 28 x 8: slot 2 d + (0: +delta, 1: -delta) the perturbed estimate, 14 + the same: its inverse
    double* evals;                    // n_edges x 29 x 7
    double* J;                        // n_edges x 2 x 49: _jacobianOplusXi, _jacobianOplusXj, row-major (row: error, column: dimension)
    double* partial;                  // chi2 partials of 256 edge positions
    double* Hs; double* bs;           // 7 na x 7 na (upper triangle of blocks), 7 na
    double* diag;                     // 7 na: the undamped diagonal
    double* x; double* sterm;         // 7 na: the solver's x, the terms of computeScale
    LbaCtl* S;
};

__host__ __device__ __forceinline__ void eg_load(const double* v, Sim3Quat& T) {
    T.q[0] = v[0]; T.q[1] = v[1]; T.q[2] = v[2]; T.q[3] = v[3]; T.t[0] = v[4]; T.t[1] = v[5]; T.t[2] = v[6]; T.s = v[7];
}
__host__ __device__ __forceinline__ void eg_store(const Sim3Quat& T, double* v) {
    v[0] = T.q[0]; v[1] = T.q[1]; v[2] = T.q[2]; v[3] = T.q[3]; v[4] = T.t[0]; v[5] = T.t[1]; v[6] = T.t[2]; v[7] = T.s;
}
__host__ __device__ __forceinline__ void eg_identity(Sim3Quat& T) {   // Sim3(): r.setIdentity(), t.fill(0.), s = 1.
    T.q[0] = 0.; T.q[1] = 0.; T.q[2] = 0.; T.q[3] = 1.; T.t[0] = 0.; T.t[1] = 0.; T.t[2] = 0.; T.s = 1.;
}

// oplusImpl: `if (_fix_scale) update[6] = 0;` in the CALLER's array, Sim3 s(update), setEstimate(s * estimate())
__host__ __device__ __forceinline__ void eg_oplus(const double* est8, double* update, int fix_scale, int order, double* out8) {
    if (fix_scale) update[6] = 0;
    Sim3Quat E, d, T;
    eg_load(est8, E);
    sim3_exp(update, order, d);
    sim3_mul(d, E, T);
    eg_store(T, out8);
}
// linearizeOplus's step `slot` (dimension slot / 2, +delta for an even slot, -delta for an odd one) of one vertex: the perturbed
// estimate and its inverse.  With a fixed scale the step along dimension 6 is zeroed by oplusImpl, both signs.
__host__ __device__ __forceinline__ void eg_perturb(const double* est8, int slot, int fix_scale, int order, double* pert8, double* inv8) {
    double add[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const double step = (slot & 1) ? -EG_DELTA : EG_DELTA;
#pragma unroll
    for (int d = 0; d < 7; ++d) if (d == (slot >> 1)) add[d] = step;
    eg_oplus(est8, add, fix_scale, order, pert8);
    Sim3Quat P, I;
    eg_load(pert8, P);
    sim3_inverse(P, I);
    eg_store(I, inv8);
}
// computeError: Sim3 C(_measurement); error_ = C * v1->estimate() * v2->estimate().inverse(); _error = error_.log()
__host__ __device__ __forceinline__ int eg_error_inv(const double* meas8, const double* v0_8, const double* v1inv8, int order, double* e7) {
    Sim3Quat C, A, Bi, CA, E;
    eg_load(meas8, C); eg_load(v0_8, A); eg_load(v1inv8, Bi);
    sim3_mul(C, A, CA);
    sim3_mul(CA, Bi, E);
    return sim3_log(E, order, e7);
}
__host__ __device__ __forceinline__ int eg_error(const double* meas8, const double* v0_8, const double* v1_8, int order, double* e7) {
    Sim3Quat B, Bi;
    double inv8[8];
    eg_load(v1_8, B);
    sim3_inverse(B, Bi);
    eg_store(Bi, inv8);
    return eg_error_inv(meas8, v0_8, inv8, order, e7);
}
// slot s of edge e at the estimate buffer `buf`: 0 the estimates, 1 .. 14 vertex 0 perturbed, 15 .. 28 vertex 1.  Returns false when the
// slot belongs to a vertex without a Jacobian (fixed): nothing is evaluated.
__host__ __device__ __forceinline__ bool eg_slot(const EgView& V, int e, int s, int buf, int order, double* e7) {
    const int v0 = V.ev0[e], v1 = V.ev1[e];
    const double* M = V.meas + 8 * (size_t)e;
    const double* E0 = V.est[buf] + 8 * (size_t)v0;
    const double* E1 = V.est[buf] + 8 * (size_t)v1;
    if (s == 0) { eg_error(M, E0, E1, order, e7); return true; }
    if (s < 15) {
        const int h = V.hidx[v0];
        if (h < 0) return false;
        eg_error(M, V.pert + ((size_t)h * 28 + (s - 1)) * 8, E1, order, e7);
        return true;
    }
    const int h = V.hidx[v1];
    if (h < 0) return false;
    eg_error_inv(M, E0, V.pert + ((size_t)h * 28 + 14 + (s - 15)) * 8, order, e7);
    return true;
}

// row j of information() * v with information = Matrix<double,7,7>::Identity(): the seven products in ascending column
__host__ __device__ __forceinline__ double eg_ident_row(int j, const double* v, size_t stride) {
    double s = (j == 0 ? 1.0 : 0.0) * v[0];
#pragma unroll
    for (int k = 1; k < 7; ++k) s = s + (j == k ? 1.0 : 0.0) * v[k * stride];
    return s;
}
// chi2(): _error.dot(information() * _error)
__host__ __device__ __forceinline__ double eg_chi2(const double* e7) {
    double s = e7[0] * eg_ident_row(0, e7, 1);
#pragma unroll
    for (int j = 1; j < 7; ++j) s = s + e7[j] * eg_ident_row(j, e7, 1);
    return s;
}
// AtO = A^T * omega, entry (r, k): column r of A against column k of the identity
__host__ __device__ __forceinline__ double eg_AtO(const double* A, int r, int k) {
    double s = A[r] * (k == 0 ? 1.0 : 0.0);
#pragma unroll
    for (int j = 1; j < 7; ++j) s = s + A[7 * j + r] * (j == k ? 1.0 : 0.0);
    return s;
}
// (A^T omega) * B, entry (r, c): from->A (B = A), to->A (both B: B^T * omega * B) and _hessian
__host__ __device__ __forceinline__ double eg_AtOB(const double* A, const double* B, int r, int c) {
    double s = eg_AtO(A, r, 0) * B[c];
#pragma unroll
    for (int k = 1; k < 7; ++k) s = s + eg_AtO(A, r, k) * B[7 * k + c];
    return s;
}
// _hessianTransposed: B^T * AtO^T, entry (r, c)
__host__ __device__ __forceinline__ double eg_BtAtOt(const double* A, const double* B, int r, int c) {
    double s = B[r] * eg_AtO(A, c, 0);
#pragma unroll
    for (int k = 1; k < 7; ++k) s = s + B[7 * k + r] * eg_AtO(A, c, k);
    return s;
}
// A^T * omega_r, entry r, omega_r = -(omega * _error)
__host__ __device__ __forceinline__ double eg_b(const double* A, const double* e7, int r) {
    double s = A[r] * -eg_ident_row(0, e7, 1);
#pragma unroll
    for (int j = 1; j < 7; ++j) s = s + A[7 * j + r] * -eg_ident_row(j, e7, 1);
    return s;
}

// column d of the Jacobian of edge e by its vertex `role`: scalar * (e(+delta) - e(-delta))
__host__ __device__ __forceinline__ void eg_jacobian_column(const EgView& V, int e, int role, int d) {
    const double scalar = 1.0 / (2 * EG_DELTA);
    const double* plus = V.evals + ((size_t)e * EG_SLOTS + 1 + 14 * role + 2 * d) * 7;
    const double* minus = plus + 7;
    double* Jc = V.J + ((size_t)e * 2 + role) * 49;
#pragma unroll
    for (int r = 0; r < 7; ++r) Jc[7 * r + d] = scalar * (plus[r] - minus[r]);
}

// entry (r, c) of the diagonal block of hessian index a: from->A += AtO * A of the edges it is vertex 0 of, to->A += B^T omega B of
// those it is vertex 1 of, in active-edge order
__host__ __device__ __forceinline__ double eg_diag_entry(const EgView& V, int a, int r, int c) {
    const int v = V.act[a];
    double s = 0.0;
    for (int q = V.vfirst[a]; q < V.vfirst[a + 1]; ++q) {
        const int e = V.vedge[q];
        const double* Jv = V.J + ((size_t)e * 2 + (V.ev0[e] == v ? 0 : 1)) * 49;
        s += eg_AtOB(Jv, Jv, r, c);
    }
    return s;
}
__host__ __device__ __forceinline__ double eg_b_entry(const EgView& V, int a, int r) {
    const int v = V.act[a];
    double s = 0.0;
    for (int q = V.vfirst[a]; q < V.vfirst[a + 1]; ++q) {
        const int e = V.vedge[q];
        s += eg_b(V.J + ((size_t)e * 2 + (V.ev0[e] == v ? 0 : 1)) * 49, V.evals + (size_t)e * EG_SLOTS * 7, r);
    }
    return s;
}
// entry (r, c) of the block (i1, i2), i1 < i2: where mapHessianMemory puts it -- _hessian = AtO * B when vertex 0 has the smaller
// hessian index, _hessianTransposed = B^T * AtO^T otherwise
__host__ __device__ __forceinline__ double eg_pair_entry(const EgView& V, int p, int r, int c) {
    const int i1 = V.pairs[2 * (size_t)p];
    double s = 0.0;
    for (int q = V.pfirst[p]; q < V.pfirst[p + 1]; ++q) {
        const int e = V.pedge[q];
        const double* A = V.J + (size_t)e * 98;
        s += V.hidx[V.ev0[e]] == i1 ? eg_AtOB(A, A + 49, r, c) : eg_BtAtOt(A, A + 49, r, c);
    }
    return s;
}

// update(x) on one active vertex: oplusImpl (which zeroes x[6] of the SOLVER's vector when the scale is fixed) into the trial buffer,
// then this vertex's terms of computeScale, which therefore read the zeroed entry
__host__ __device__ __forceinline__ void eg_update_vertex(const EgView& V, int a, int order) {
    const LbaCtl& S = *V.S;
    const int v = V.act[a];
    double* x = V.x + 7 * (size_t)a;
    eg_oplus(V.est[S.cur] + 8 * (size_t)v, x, V.fix_scale, order, V.est[S.cur ^ 1] + 8 * (size_t)v);
#pragma unroll
    for (int k = 0; k < 7; ++k) V.sterm[7 * (size_t)a + k] = x[k] * (S.lambda * x[k] + V.bs[7 * (size_t)a + k]);
}

// step 7: correctedSwr.map(Srw.map(P)), Srw the INPUT estimate of the reference vertex, correctedSwr the inverse of its final one;
// without a reference vertex both are the default-constructed Sim3
__host__ __device__ __forceinline__ void eg_correct_point(const double* vertex0, const double* final_est, int ref, const float* P, float* out) {
    Sim3Quat Srw, Siw, Swr;
    if (ref < 0) { eg_identity(Srw); eg_identity(Swr); }
    else { eg_load(vertex0 + 8 * (size_t)ref, Srw); eg_load(final_est + 8 * (size_t)ref, Siw); sim3_inverse(Siw, Swr); }
    sim3_correct_point(Srw, Swr, P, out);
}
// step 6: eigR = rotation().toRotationMatrix(), eigt *= (1./s), Converter::toCvSE3
__host__ __device__ __forceinline__ void eg_Tiw(const double* est8, float* M) {
    double R[9];
    eigen_quat_to_matrix(est8, R);
    const double inv = 1. / est8[7];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) M[4 * r + c] = x86_nan((float)R[3 * r + c]);
        M[4 * r + 3] = x86_nan((float)(est8[4 + r] * inv));
    }
    M[12] = 0.0f; M[13] = 0.0f; M[14] = 0.0f; M[15] = 1.0f;
}
