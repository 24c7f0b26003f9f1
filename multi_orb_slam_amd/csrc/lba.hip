// lba.hip -- local bundle adjustment on the device (include/orbm.h, "local bundle adjustment"): Optimizer::LocalBundleAdjustment
// (reference src/Optimizer.cc:921-1353) from the graph on.  The arithmetic of one edge, of one landmark and of the controller's driver is
// lba_dev.h's, the Levenberg rules and the summation tree are lm_dev.h's, what is g2o's is g2o_dev.h's; here are the steps over the
// whole graph, ONE definition each, called by the host routine's loops and by the kernels:
//   lba_pass_edge      computeActiveErrors (+ linearizeOplus + constructQuadraticForm) of one edge, its share of activeRobustChi2
//   lba_point_sum, lba_pose_sum   a vertex's Hll / bl, Hpp / bp: its active edges in ascending edge position
//   lba_schur_entry, lba_schur_b  the reduced system: Hschur(i1, i2) -= (Bi Dinv) Bj^T over the landmarks both poses see, in ascending
//                      landmark order (a merge-join of the two poses' edge lists); bschur = b - coefficients
//   lba_ldlt_host / k_lba_solve   the dense LDL^T without pivoting (deviation (a)): every inner product sequential in ascending index
//   lba_point_update, lba_pose_update   cl = bl - B^T xp, xl = Dinv cl; oplus into the trial buffers; the terms of computeScale
//   lba_classify_edge  `chi2() > 5.991 / 7.815 || !isDepthPositive()` with the chi2 of the last computeActiveErrors
//   lba_flow           the reference's sequence around the two optimisations and g2o's optimize() loop with every poll of the stop
//                      flag, over a backend: LbaHost (loops) or LbaDevice (kernel chains, one synchronisation per Levenberg trial).
// The device: per iteration k_lba_edges<true>, k_lba_point_sum, k_lba_pose_sum, k_lba_ctl_full; per trial k_lba_point_damp,
// k_lba_schur, k_lba_solve, k_lba_update, k_lba_edges<false>, k_lba_ctl_trial, which leaves one 4-byte command word in mapped memory.  Every
// launch ends on its own: no kernel waits for another, no atomics, no order that depends on arrival.  Accepting a trial is a choice of
// buffer (LbaCtl::cur).  No libm function runs in a kernel.
// The global bundle adjustment (Optimizer::BundleAdjustment, reference src/Optimizer.cc:47-330; include/orbm.h "global bundle
// adjustment") is the same steps and backends in another sequence, ba_flow: one optimisation, the kernels on every edge or on none.
// Its backends run `global`: the reduced system over the block pairs that exist (ba_block_pairs; k_ba_schur_pairs, the rest filled with
// 0.0 once) and, for up to 6 * ORBM_BA_MAX_FREE rows, ba_ldlt_host / ba_ldlt_dev.h's blocked LDL^T across workgroups in place of
// lba_ldlt_host / k_lba_solve.  Nothing the local BA computes changes: its flow, its kernels and its caps are as they were.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <optional>
#include <vector>

#include "../../include/orbm.h"
#include "../../include/orb_debug.h"
#include "orb_common.h"
#include "matcher_internal.h"
#include "cv_dev.h"
#include "g2o_dev.h"
#include "lm_dev.h"
#include "lba_dev.h"
#include "ba_ldlt_dev.h"
#include "stage_pack.h"

namespace {

constexpr int LBA_SOLVE_T = 512;      // lanes of k_lba_solve: one per row of the reduced system (6 * ORBM_LBA_MAX_FREE = 384 rows)
constexpr int LBA_MAX_N = 6 * ORBM_LBA_MAX_FREE;
static_assert(LBA_MAX_N <= LBA_SOLVE_T, "one lane per row");
static_assert(BA_PANEL == ORBM_BA_PANEL, "the panel width the header exports");
static_assert(LBA_T == LM_T, "the chi2 partial is lm_dev.h's tree");

// Everything a step reads and writes, as raw pointers: the host routine's vectors or the device's buffers.
struct LbaView {
    int n_free, n_poses, n_points, n_edges;
    int stage;                           // 0: optimize(5), every edge behind its kernel; 1: optimize(10), kernels only on bad points' edges
    int na, nl, nx;                      // active free poses, active landmarks, 6 na + 3 nl
    // the graph
    const float* K; const int32_t* first; const int32_t* edge_pose; const int32_t* edge_point; const uint8_t* edge_cam;
    const float* obs; const float* w; const uint8_t* bad;
    // initializeOptimization(): which edges and vertices are active, hessian indices, the poses' edge lists, the points' pose-ordered lists
    const uint8_t* active;               // per edge
    const int32_t* pose_h;               // per pose: hessian index or -1
    const int32_t* point_h;              // per point: landmark index or -1
    const int32_t* pose_first;           // na + 1
    const int32_t* pose_edge;            // the active edges of an active free pose in ascending edge position
    const int32_t* srow;                 // per point at first[l]: its active edges to free poses in ascending hessian index (_HplCCS's column)
    const int32_t* nfree;                // per point: how many
    // state
    double* pose[2]; double* point[2];   // the two estimate buffers: 7 per pose, 3 per point
    double* E;                           // LBA_EDGE_DOUBLES arrays of n_edges
    double* chi2;                        // per edge: chi2() of the last computeActiveErrors that reached it
    double* Hll; double* bl; double* Dinv; double* db;     // per point: 9, 3, 9, 3
    double* Hpp; double* bp;             // per active pose: 36, 6
    double* Hs; double* bs; double* Lt; double* d;         // the reduced system (n x n, n = 6 na), its factor (Lt[k n + i] = L(i, k)), D
    double* x; double* sterm;            // g2o's x by hessian position (poses, then landmarks); x (lambda x + b) term by term
    double* partial;                     // chi2 partials, one per LBA_T edge positions
    uint8_t* flags;                      // per edge
    LbaCtl* S;
};

// ---- the steps ---------------------------------------------------------------------------------------------------------------------------
template <bool SYSTEM>
__host__ __device__ __forceinline__ double lba_pass_edge(const LbaView& V, const LbaCam& C, int e, int buf) {
    if (!V.active[e]) return 0.0;
    const int p = V.edge_pose[e], l = V.edge_point[e];
    const bool stereo = !(V.obs[3 * (size_t)e + 2] < 0);      // `mvuRight_total[i] < 0`: the mono form
    const bool robust = V.stage == 0 || V.bad[l] != 0;
    const double w = (double)V.w[e];
    LbaEval o;
    lba_edge<SYSTEM>(C, V.K + 5 * (size_t)p, V.pose[buf] + 7 * (size_t)p, V.point[buf] + 3 * (size_t)l, V.edge_cam[e], stereo, V.obs + 3 * (size_t)e, w, o);
    V.chi2[e] = o.chi2;
    double rho0, rho1;
    lba_rho(C, o.chi2, stereo, robust, &rho0, &rho1);
    if (SYSTEM) lba_edge_blocks(o, w, rho1, stereo, robust, V.pose_h[p] >= 0, V.E + e, (size_t)V.n_edges);
    return rho0;
}
// v->clearQuadraticForm(), then every active edge of the landmark adds its block: Hll[9 l ..], bl[3 l ..]
__host__ __device__ __forceinline__ void lba_point_sum(const LbaView& V, int l) {
    double H[9], b[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) H[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) b[k] = 0.0;
    const size_t ne = (size_t)V.n_edges;
    for (int e = V.first[l]; e < V.first[l + 1]; ++e) {
        if (!V.active[e]) continue;
#pragma unroll
        for (int k = 0; k < 9; ++k) H[k] = H[k] + V.E[(LBA_HLL + k) * ne + e];
#pragma unroll
        for (int k = 0; k < 3; ++k) b[k] = b[k] + V.E[(LBA_BL + k) * ne + e];
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) V.Hll[9 * (size_t)l + k] = H[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) V.bl[3 * (size_t)l + k] = b[k];
}
// entry k of active pose i: k < 36 an entry of Hpp, else of bp
__host__ __device__ __forceinline__ void lba_pose_sum(const LbaView& V, int i, int k) {
    const size_t ne = (size_t)V.n_edges;
    const size_t arr = k < 36 ? (size_t)(LBA_HPP + k) : (size_t)(LBA_BP + k - 36);
    double s = 0.0;
    for (int a = V.pose_first[i]; a < V.pose_first[i + 1]; ++a) s = s + V.E[arr * ne + V.pose_edge[a]];
    if (k < 36) V.Hpp[36 * (size_t)i + k] = s; else V.bp[6 * (size_t)i + k - 36] = s;
}
// computeLambdaInit's candidates: v > max keeps the maximum (a NaN is never taken), so the order of the vertices does not matter
__host__ __device__ __forceinline__ double lba_max_diag(const LbaView& V, int v, double m) {
    if (v < V.na) {
        for (int j = 0; j < 6; ++j) { const double a = fabs(V.Hpp[36 * (size_t)v + 7 * j]); if (a > m) m = a; }
    } else {
        const int l = v - V.na;          // a POINT index; inactive points are skipped
        if (V.point_h[l] >= 0)
            for (int j = 0; j < 3; ++j) { const double a = fabs(V.Hll[9 * (size_t)l + 4 * j]); if (a > m) m = a; }
    }
    return m;
}
__host__ __device__ __forceinline__ void lba_point_damp_at(const LbaView& V, int l, double lambda) {
    if (V.point_h[l] < 0) return;
    lba_point_damp(V.Hll + 9 * (size_t)l, V.bl + 3 * (size_t)l, lambda, V.Dinv + 9 * (size_t)l, V.db + 3 * (size_t)l);
}
// Hschur(i1, i2)(r, c), i2 >= i1: _Hschur = _Hpp with its damped diagonal, then landmark by landmark `-= BDinv * Bj^T`
__host__ __device__ __forceinline__ double lba_schur_entry(const LbaView& V, double lambda, int i1, int i2, int r, int c) {
    const size_t ne = (size_t)V.n_edges;
    double h = 0.0;
    if (i1 == i2) { double hpp = V.Hpp[36 * (size_t)i1 + 6 * r + c]; if (r == c) hpp = hpp + lambda; h = h + hpp; }
    int a = V.pose_first[i1], b = V.pose_first[i2];
    const int ae = V.pose_first[i1 + 1], be = V.pose_first[i2 + 1];
    while (a < ae && b < be) {
        const int e1 = V.pose_edge[a], e2 = V.pose_edge[b];
        const int l1 = V.edge_point[e1], l2 = V.edge_point[e2];
        if (l1 < l2) { ++a; continue; }
        if (l2 < l1) { ++b; continue; }
        const double* Di = V.Dinv + 9 * (size_t)l1;
        const double b0 = V.E[(LBA_HPL + 3 * r) * ne + e1], b1 = V.E[(LBA_HPL + 3 * r + 1) * ne + e1], b2 = V.E[(LBA_HPL + 3 * r + 2) * ne + e1];
        const double bd0 = (b0 * Di[0] + b1 * Di[3]) + b2 * Di[6];        // BDinv = Bi * Dinv
        const double bd1 = (b0 * Di[1] + b1 * Di[4]) + b2 * Di[7];
        const double bd2 = (b0 * Di[2] + b1 * Di[5]) + b2 * Di[8];
        const double s = (bd0 * V.E[(LBA_HPL + 3 * c) * ne + e2] + bd1 * V.E[(LBA_HPL + 3 * c + 1) * ne + e2]) + bd2 * V.E[(LBA_HPL + 3 * c + 2) * ne + e2];
        h = h - s;
        ++a; ++b;
    }
    return h;
}
// bschur[6 i + r] = b - coefficients, coefficients: `Bb += Bi * db` over the pose's landmarks in ascending order
__host__ __device__ __forceinline__ double lba_schur_b(const LbaView& V, int i, int r) {
    const size_t ne = (size_t)V.n_edges;
    double Bb = 0.0;
    for (int a = V.pose_first[i]; a < V.pose_first[i + 1]; ++a) {
        const int e = V.pose_edge[a];
        const double* db = V.db + 3 * (size_t)V.edge_point[e];
        Bb = Bb + ((V.E[(LBA_HPL + 3 * r) * ne + e] * db[0] + V.E[(LBA_HPL + 3 * r + 1) * ne + e] * db[1]) + V.E[(LBA_HPL + 3 * r + 2) * ne + e] * db[2]);
    }
    return V.bp[6 * (size_t)i + r] - Bb;
}
// One landmark after the poses' solve (block_solver.hpp:461-481): cl = bl, `cl += Bi^T * cp` block by block in ascending pose index with
// cp = -xp, xl = 0 + Dinv * cl -- only after a successful solve, else x stays; then the landmark's terms of computeScale and its trial
// estimate (VertexSBAPointXYZ::oplusImpl: _estimate += v) into buffer `buf`.
__host__ __device__ __forceinline__ void lba_point_update(const LbaView& V, int l, int ok2, double lambda, int buf) {
    const int h = V.point_h[l];
    if (h < 0) return;
    const size_t ne = (size_t)V.n_edges;
    double* xl = V.x + 6 * (size_t)V.na + 3 * (size_t)h;
    if (ok2) {
        double cl[3] = {V.bl[3 * (size_t)l], V.bl[3 * (size_t)l + 1], V.bl[3 * (size_t)l + 2]};
        const int s0 = V.first[l];
        for (int s = s0; s < s0 + V.nfree[l]; ++s) {
            const int e = V.srow[s];
            const double* xp = V.x + 6 * (size_t)V.pose_h[V.edge_pose[e]];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                double t = V.E[(LBA_HPL + c) * ne + e] * (-xp[0]);
#pragma unroll
                for (int k = 1; k < 6; ++k) t = t + V.E[(LBA_HPL + 3 * k + c) * ne + e] * (-xp[k]);
                cl[c] = cl[c] + t;
            }
        }
        const double* Di = V.Dinv + 9 * (size_t)l;
#pragma unroll
        for (int r = 0; r < 3; ++r) xl[r] = 0.0 + ((Di[3 * r] * cl[0] + Di[3 * r + 1] * cl[1]) + Di[3 * r + 2] * cl[2]);
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        V.sterm[6 * (size_t)V.na + 3 * (size_t)h + r] = xl[r] * (lambda * xl[r] + V.bl[3 * (size_t)l + r]);
        V.point[buf][3 * (size_t)l + r] = V.point[buf ^ 1][3 * (size_t)l + r] + xl[r];
    }
}
__host__ __device__ __forceinline__ void lba_pose_update(const LbaView& V, int p, double lambda, int order, int buf) {
    const int h = V.pose_h[p];
    if (h < 0) return;
    const double* xp = V.x + 6 * (size_t)h;
    for (int k = 0; k < 6; ++k) V.sterm[6 * (size_t)h + k] = xp[k] * (lambda * xp[k] + V.bp[6 * (size_t)h + k]);
    lba_pose_oplus(V.pose[buf ^ 1] + 7 * (size_t)p, xp, order, V.pose[buf] + 7 * (size_t)p);
}
// the tests of :1227-1262 (which = ORBM_LBA_FLAG_LEVEL1) and :1279-1309 (ORBM_LBA_FLAG_ERASE) on one edge: chi2() is the error the
// last computeActiveErrors left in the edge, isDepthPositive() is evaluated at the estimate
__host__ __device__ __forceinline__ void lba_classify_edge(const LbaView& V, const LbaCam& C, int e, int which, int buf) {
    const int p = V.edge_pose[e], l = V.edge_point[e];
    if (V.bad[l]) return;                                    // `if(pMP->isBad()) continue;`
    const bool stereo = !(V.obs[3 * (size_t)e + 2] < 0);
    LbaEval o;
    lba_edge<false>(C, V.K + 5 * (size_t)p, V.pose[buf] + 7 * (size_t)p, V.point[buf] + 3 * (size_t)l, V.edge_cam[e], stereo, V.obs + 3 * (size_t)e, (double)V.w[e], o);
    const double th = stereo ? 7.815 : 5.991;
    if (V.chi2[e] > th || !(o.zc > 0.0)) V.flags[e] = (uint8_t)(V.flags[e] | which);
}

// ---- the graph of a call -----------------------------------------------------------------------------------------------------------------
struct LbaGraph {                        // what does not change over a call, on the host
    const orbm_lba_problem* P;
    int n_edges;
    std::vector<int32_t> edge_point;
    std::vector<uint8_t> bad;            // zeros when the caller has none
    std::vector<double> pose0, point0;   // Converter::toSE3Quat(GetPose()), Converter::toVector3d(GetWorldPos())
    LbaCam C;
};
struct LbaStructure {                    // initializeOptimization(): per optimisation, on the host
    std::vector<uint8_t> active;
    std::vector<int32_t> pose_h, point_h, pose_first, pose_edge, srow, nfree;
    int na = 0, nl = 0, n_active = 0;
    std::vector<int32_t> pairs;          // (global BA) the blocks (i1 <= i2) of the reduced system that exist, sorted, two entries each
};

int lba_validate(const orbm_lba_problem* P, const orbm_lba_result* R) {
    MORB_ARG(P != nullptr && R != nullptr);
    MORB_ARG(P->n_free >= 0 && P->n_poses >= P->n_free && P->n_points >= 0 && P->first != nullptr);
    MORB_ARG(P->n_poses == 0 || (P->Tcw != nullptr && P->K != nullptr));
    MORB_ARG(P->n_points == 0 || P->points != nullptr);
    if (const int rc = morb::validate_first(P->n_points, P->first, "point")) return rc;
    const int ne = P->first[P->n_points];
    MORB_ARG(ne == 0 || (P->edge_pose && P->edge_cam && P->obs && P->inv_sigma2));
    MORB_ARG(R->pose && R->Tcw && R->point && R->point_f && R->flags);
    std::vector<int32_t> seen((size_t)std::max(P->n_poses, 1), -1);
    for (int l = 0; l < P->n_points; ++l)
        for (int e = P->first[l]; e < P->first[l + 1]; ++e) {
            const int p = P->edge_pose[e];
            if (p < 0 || p >= P->n_poses || P->edge_cam[e] > 1) { morb::set_error("edge %d: pose %d, camera %d", e, p, (int)P->edge_cam[e]); return ORB_E_ARG; }
            if (seen[p] == l) { morb::set_error("point %d has two edges to pose %d", l, p); return ORB_E_ARG; }
            seen[p] = l;
        }
    return ORB_OK;
}
void lba_graph(const orbm_lba_problem* P, LbaGraph& G, bool use_bad = true) {
    G.P = P;
    G.n_edges = P->first[P->n_points];
    G.edge_point.resize((size_t)std::max(G.n_edges, 1));
    for (int l = 0; l < P->n_points; ++l) for (int e = P->first[l]; e < P->first[l + 1]; ++e) G.edge_point[e] = l;
    G.bad.assign((size_t)std::max(P->n_points, 1), 0);
    if (P->bad && use_bad) for (int l = 0; l < P->n_points; ++l) G.bad[l] = P->bad[l] ? 1 : 0;
    G.pose0.resize(7 * (size_t)std::max(P->n_poses, 1)); G.point0.resize(3 * (size_t)std::max(P->n_points, 1));
    for (int p = 0; p < P->n_poses; ++p) {
        SE3Quat T;
        se3_from_cv(P->Tcw + 16 * (size_t)p, T);
        se3_store7(T, &G.pose0[7 * (size_t)p]);
    }
    for (size_t k = 0; k < 3 * (size_t)P->n_points; ++k) G.point0[k] = (double)P->points[k];
    lba_camera(P->Tcim, G.C);
}
// initializeOptimization(level 0): the active edges (level 0; a point is never fixed, so no edge has all its vertices fixed), the
// vertices that have one, buildIndexMapping (poses, then landmarks, each in ascending vertex id), the poses' edge lists and the
// landmarks' columns of _HplCCS (ascending pose index)
void lba_structure(const LbaGraph& G, const uint8_t* flags, LbaStructure& T) {
    const orbm_lba_problem* P = G.P;
    const int ne = G.n_edges;
    T.active.assign((size_t)std::max(ne, 1), 0);
    T.pose_h.assign((size_t)std::max(P->n_poses, 1), -1); T.point_h.assign((size_t)std::max(P->n_points, 1), -1);
    T.nfree.assign((size_t)std::max(P->n_points, 1), 0); T.srow.assign((size_t)std::max(ne, 1), 0);
    std::vector<int32_t> count((size_t)std::max(P->n_free, 1), 0);
    T.n_active = 0;
    for (int e = 0; e < ne; ++e) {
        T.active[e] = (flags[e] & ORBM_LBA_FLAG_LEVEL1) ? 0 : 1;
        if (!T.active[e]) continue;
        ++T.n_active;
        if (P->edge_pose[e] < P->n_free) ++count[P->edge_pose[e]];
    }
    T.na = 0;
    for (int p = 0; p < P->n_free; ++p) if (count[p]) T.pose_h[p] = T.na++;
    T.pose_first.assign((size_t)T.na + 1, 0);
    for (int p = 0; p < P->n_free; ++p) if (count[p]) T.pose_first[T.pose_h[p] + 1] = count[p];
    for (int i = 0; i < T.na; ++i) T.pose_first[i + 1] += T.pose_first[i];
    T.pose_edge.assign((size_t)std::max(T.pose_first[T.na], 1), 0);
    std::vector<int32_t> fill(T.pose_first.begin(), T.pose_first.end());
    T.nl = 0;
    for (int l = 0; l < P->n_points; ++l) {
        int any = 0, nf = 0;
        for (int e = P->first[l]; e < P->first[l + 1]; ++e) {
            if (!T.active[e]) continue;
            any = 1;
            const int h = T.pose_h[P->edge_pose[e]];
            if (h < 0) continue;
            T.pose_edge[fill[h]++] = e;
            T.srow[P->first[l] + nf++] = e;
        }
        if (any) T.point_h[l] = T.nl++;
        T.nfree[l] = nf;
        std::sort(T.srow.begin() + P->first[l], T.srow.begin() + P->first[l] + nf,
                  [&](int32_t a, int32_t b) { return T.pose_h[P->edge_pose[a]] < T.pose_h[P->edge_pose[b]]; });
    }
}
// The global BA's reduced system: every diagonal block, and the pairs (i1 < i2) of active free poses that share an active landmark
// (srow is a landmark's free poses in ascending hessian index).  For every other pair lba_schur_entry finds nothing to subtract from
// h = 0.0, so the block is the zeros the buffer is filled with once per optimisation.
void ba_block_pairs(const LbaGraph& G, LbaStructure& T) {
    const orbm_lba_problem* P = G.P;
    const size_t na = (size_t)T.na;
    std::vector<uint8_t> hit(std::max<size_t>(na * na, 1), 0);
    for (size_t i = 0; i < na; ++i) hit[i * na + i] = 1;
    for (int l = 0; l < P->n_points; ++l) {
        const int s0 = P->first[l], s1 = s0 + T.nfree[l];
        for (int a = s0; a < s1; ++a) {
            const size_t ha = (size_t)T.pose_h[P->edge_pose[T.srow[a]]];
            for (int b = a + 1; b < s1; ++b) hit[ha * na + (size_t)T.pose_h[P->edge_pose[T.srow[b]]]] = 1;
        }
    }
    T.pairs.clear();
    for (size_t i1 = 0; i1 < na; ++i1)
        for (size_t i2 = i1; i2 < na; ++i2) if (hit[i1 * na + i2]) { T.pairs.push_back((int32_t)i1); T.pairs.push_back((int32_t)i2); }
}

// Converter::toCvMat(SE3Quat) (g2o_dev.h's se3_to_cv), Converter::toCvMat(Vector3d)
void lba_write_result(const orbm_lba_problem* P, const double* pose, const double* point, orbm_lba_result* R) {
    for (int p = 0; p < P->n_poses; ++p) {
        const double* T = pose + 7 * (size_t)p;
        SE3Quat Q;
        se3_load7(T, Q);
        se3_to_cv(Q, R->Tcw + 16 * (size_t)p);
        for (int k = 0; k < 7; ++k) R->pose[7 * (size_t)p + k] = x86_nan(T[k]);
    }
    for (size_t k = 0; k < 3 * (size_t)P->n_points; ++k) { R->point[k] = x86_nan(point[k]); R->point_f[k] = x86_nan((float)point[k]); }
}

// ---- the sequence ------------------------------------------------------------------------------------------------------------------------
struct LbaReport { int32_t want_trial, more, ok, seq; };
// the ONE 4-byte command word the device leaves in mapped memory per trial: bit 0 want_trial, bit 1 more, bit 2 ok, bits 8 .. 31 the
// number of the step it answers (so that a word that did not arrive is an error, not an old verdict)
__host__ __device__ inline uint32_t lba_command_word(const LbaCtl& S, int seq) {
    return (uint32_t)(S.want_trial ? 1 : 0) | (uint32_t)(S.more ? 2 : 0) | (uint32_t)(S.ok ? 4 : 0) | ((uint32_t)seq << 8);
}

// Optimizer.cc:1204-1309 around g2o's optimize() (core/sparse_optimizer.cpp:354-419).  The backend supplies: begin_optimisation (returns
// the number of active vertices), iteration (solve() up to and including its first trial), trial, iter_end (the trial loop was left by
// the stop flag), classify, finish.
// g2o's optimize() loop (core/sparse_optimizer.cpp:376-414) with its two polls, after begin_optimisation: what both flows share
template <class Backend, class Poll>
int lba_optimise(Backend& B, Poll& poll, int max_iter) {
    int rc;
    LbaReport rep = {0, max_iter > 0 ? 1 : 0, 1, 0};
    // for (int i=0; i<iterations && ! terminate() && ok; i++)
    while (rep.more) {
        if (poll()) break;
        if (!rep.ok) break;
        if ((rc = B.iteration(&rep))) return rc;
        while (rep.want_trial) {                      // `while (rho<0 && qmax < 10 && ! _optimizer->terminate())`
            if (poll()) { if ((rc = B.iter_end(&rep))) return rc; break; }
            if ((rc = B.trial(&rep))) return rc;
        }
    }
    return ORB_OK;
}
template <class Backend>
int lba_flow(Backend& B, orbm_lba_stop_fn stop, void* ctx, orbm_lba_result* R) {
    int polls = 0, rc;
    auto poll = [&]() -> bool { if (!stop) return false; ++polls; return stop(ctx) != 0; };
    R->ended = ORBM_LBA_ENDED_COMPLETE; R->optimisations = 0;
    for (int s = 0; s < 2; ++s) { R->active_poses[s] = 0; R->active_points[s] = 0; R->active_edges[s] = 0; }
    R->reserved = 0;
    if (poll()) R->ended = ORBM_LBA_ENDED_STOPPED_AT_START;   // :1204 `return`
    for (int stage = 0; stage < 2 && R->ended == ORBM_LBA_ENDED_COMPLETE; ++stage) {
        int n_vertices = 0;
        if ((rc = B.begin_optimisation(stage, stage ? 10 : 5, &n_vertices, R))) return rc;
        if (n_vertices > 0) {                                 // else `_ivMap.size() == 0`: optimize() returns -1 before its loop
            R->optimisations = stage + 1;
            if ((rc = lba_optimise(B, poll, stage ? 10 : 5))) return rc;
        }
        if (stage == 0) {
            if (poll()) { R->ended = ORBM_LBA_ENDED_NO_SECOND; break; }   // :1217 bDoMore = false
            if ((rc = B.classify(ORBM_LBA_FLAG_LEVEL1))) return rc;
        }
    }
    if (R->ended != ORBM_LBA_ENDED_STOPPED_AT_START && (rc = B.classify(ORBM_LBA_FLAG_ERASE))) return rc;
    R->polls = polls;
    return B.finish(R);
}
// Optimizer::BundleAdjustment (Optimizer.cc:300-302): ONE initializeOptimization(), ONE optimize(nIterations), no test, no second
// optimisation; the reference polls nowhere, g2o where it always does.  The Huber kernels are on every edge or on none, the two forms
// lba_pass_edge has: stage 0 is "every edge behind its kernel", stage 1 with no bad point "no kernel" -- so `robust` chooses the stage,
// and the round and the active counts of that stage are the call's.
template <class Backend>
int ba_flow(Backend& B, int n_iterations, int robust, orbm_lba_stop_fn stop, void* ctx, orbm_lba_result* R) {
    int polls = 0, rc;
    auto poll = [&]() -> bool { if (!stop) return false; ++polls; return stop(ctx) != 0; };
    R->ended = ORBM_LBA_ENDED_COMPLETE; R->optimisations = 0; R->reserved = 0;
    for (int s = 0; s < 2; ++s) { R->active_poses[s] = 0; R->active_points[s] = 0; R->active_edges[s] = 0; }
    int n_vertices = 0;
    if ((rc = B.begin_optimisation(robust ? 0 : 1, n_iterations, &n_vertices, R))) return rc;
    if (n_vertices > 0) {
        R->optimisations = 1;
        if ((rc = lba_optimise(B, poll, n_iterations))) return rc;
    }
    R->polls = polls;
    return B.finish(R);
}

// chi2 partial of edge positions 256 k .. 256 k + 255 from their leaves: lm_dev.h's tree
double lba_partial_host(const double* leaf, int n) {
    double part[LBA_T], sum;
    for (int l = 0; l < LBA_T; ++l) part[l] = l < n ? leaf[l] : 0.0;
    lm_tree_host<1>(part, &sum);
    return sum;
}

// The reduced system: dense LDL^T without pivoting in the natural order (deviation (a)).  Hs: n x n row-major, its upper triangle is
// read; Lt[k n + i] = L(i, k); fails on a zero or non-finite pivot; x is written only on success.
// (the factorisation and the forward substitution, y = D^-1 L^-1 b: what the local and the global BA's routines share)
bool lba_ldlt_factor_forward(int n, const double* Hs, const double* bs, double* Lt, double* d, double* temp, double* y) {
    for (int k = 0; k < n; ++k) {
        for (int j = 0; j < k; ++j) temp[j] = d[j] * Lt[(size_t)j * n + k];
        double s = 0.0;
        for (int j = 0; j < k; ++j) s += Lt[(size_t)j * n + k] * temp[j];
        const double dk = Hs[(size_t)k * n + k] - s;
        if (!(fabs(dk) > 0) || !(fabs(dk) <= DBL_MAX)) return false;
        d[k] = dk;
        for (int i = k + 1; i < n; ++i) {
            double r = 0.0;
            for (int j = 0; j < k; ++j) r += Lt[(size_t)j * n + i] * temp[j];
            Lt[(size_t)k * n + i] = (Hs[(size_t)k * n + i] - r) / dk;
        }
    }
    for (int i = 0; i < n; ++i) { double s = 0.0; for (int j = 0; j < i; ++j) s += Lt[(size_t)j * n + i] * y[j]; y[i] = bs[i] - s; }
    for (int i = 0; i < n; ++i) y[i] = y[i] / d[i];
    return true;
}
bool lba_ldlt_host(int n, const double* Hs, const double* bs, double* Lt, double* d, double* temp, double* y, double* x) {
    if (!lba_ldlt_factor_forward(n, Hs, bs, Lt, d, temp, y)) return false;
    for (int i = n - 1; i >= 0; --i) { double s = 0.0; for (int j = i + 1; j < n; ++j) s += Lt[(size_t)i * n + j] * y[j]; y[i] = y[i] - s; }
    for (int i = 0; i < n; ++i) x[i] = y[i];
    return true;
}
// The global BA's routine, THE definition of what ba_ldlt_dev.h's kernels compute: the same factorisation and forward substitution;
// the backward substitution adds a row's terms in DESCENDING j, the far ones first, so that a blocked execution that walks the panels
// from the last to the first carries each row's sum in the order it is written here.
bool ba_ldlt_host(int n, const double* Hs, const double* bs, double* Lt, double* d, double* temp, double* y, double* x) {
    if (!lba_ldlt_factor_forward(n, Hs, bs, Lt, d, temp, y)) return false;
    for (int i = n - 1; i >= 0; --i) { double s = 0.0; for (int j = n - 1; j > i; --j) s += Lt[(size_t)i * n + j] * y[j]; y[i] = y[i] - s; }
    for (int i = 0; i < n; ++i) x[i] = y[i];
    return true;
}

// ---- host routine ------------------------------------------------------------------------------------------------------------------------
struct LbaHost {
    const LbaGraph& G;
    int order;
    bool global;                         // the global BA: the reduced system over the pairs that exist, ba_ldlt_host, sized per optimisation
    LbaStructure T;
    LbaView V;
    LbaCtl S;
    std::vector<double> pose[2], point[2], E, chi2, Hll, bl, Dinv, db, Hpp, bp, Hs, bs, Lt, d, x, sterm, temp, y, leaf;
    uint8_t* flags;

    LbaHost(const LbaGraph& g, int ord, uint8_t* fl, bool glob = false) : G(g), order(ord), global(glob), flags(fl) {
        const orbm_lba_problem* P = G.P;
        const size_t ne = (size_t)std::max(G.n_edges, 1), nl = (size_t)std::max(P->n_points, 1);
        for (int b = 0; b < 2; ++b) { pose[b] = G.pose0; point[b] = G.point0; }
        E.assign(LBA_EDGE_DOUBLES * ne, 0.0); chi2.assign(ne, 0.0);
        Hll.assign(9 * nl, 0.0); bl.assign(3 * nl, 0.0); Dinv.assign(9 * nl, 0.0); db.assign(3 * nl, 0.0);
        const size_t nf = (size_t)std::max(P->n_free, 1), n = 6 * nf;
        const size_t nn = global ? 1 : n * n;
        Hpp.assign(36 * nf, 0.0); bp.assign(6 * nf, 0.0); Hs.assign(nn, 0.0); bs.assign(n, 0.0); Lt.assign(nn, 0.0); d.assign(n, 0.0);
        temp.assign(n, 0.0); y.assign(n, 0.0);
        x.assign(n + 3 * nl, 0.0); sterm.assign(n + 3 * nl, 0.0);
        leaf.assign(ne, 0.0);
        for (int e = 0; e < G.n_edges; ++e) flags[e] = 0;
        lba_ctl_begin(S, order);
        memset(&V, 0, sizeof(V));
        V.n_free = P->n_free; V.n_poses = P->n_poses; V.n_points = P->n_points; V.n_edges = G.n_edges;
        V.K = P->K; V.first = P->first; V.edge_pose = P->edge_pose; V.edge_point = G.edge_point.data(); V.edge_cam = P->edge_cam;
        V.obs = P->obs; V.w = P->inv_sigma2; V.bad = G.bad.data();
        for (int b = 0; b < 2; ++b) { V.pose[b] = pose[b].data(); V.point[b] = point[b].data(); }
        V.E = E.data(); V.chi2 = chi2.data(); V.Hll = Hll.data(); V.bl = bl.data(); V.Dinv = Dinv.data(); V.db = db.data();
        V.Hpp = Hpp.data(); V.bp = bp.data(); V.Hs = Hs.data(); V.bs = bs.data(); V.Lt = Lt.data(); V.d = d.data();
        V.x = x.data(); V.sterm = sterm.data(); V.partial = nullptr; V.flags = flags; V.S = &S;
    }
    int begin_optimisation(int stage, int max_iter, int* n_vertices, orbm_lba_result* R) {
        lba_structure(G, flags, T);
        if (global) {
            ba_block_pairs(G, T);
            const size_t n = 6 * (size_t)T.na;
            Hs.assign(std::max<size_t>(n * n, 1), 0.0); Lt.assign(std::max<size_t>(n * n, 1), 0.0);
            V.Hs = Hs.data(); V.Lt = Lt.data();
        }
        V.stage = stage; V.na = T.na; V.nl = T.nl; V.nx = 6 * T.na + 3 * T.nl;
        V.active = T.active.data(); V.pose_h = T.pose_h.data(); V.point_h = T.point_h.data(); V.pose_first = T.pose_first.data();
        V.pose_edge = T.pose_edge.data(); V.srow = T.srow.data(); V.nfree = T.nfree.data();
        R->active_poses[stage] = T.na; R->active_points[stage] = T.nl; R->active_edges[stage] = T.n_active;
        pose[S.cur ^ 1] = pose[S.cur]; point[S.cur ^ 1] = point[S.cur];   // the trial buffer starts as the estimate (same storage: assignment copies)
        lba_ctl_begin_optimisation(S, stage, max_iter);
        *n_vertices = T.na + T.nl;
        return ORB_OK;
    }
    // activeRobustChi2 of a pass over every edge
    template <bool SYSTEM>
    double pass(int buf) {
        const int ne = G.n_edges;
        if (order == ORBM_POSE_ORDER_INDEX) {
            double chi = 0.0;
            for (int e = 0; e < ne; ++e) { if (!V.active[e]) continue; chi += lba_pass_edge<SYSTEM>(V, G.C, e, buf); }
            return chi;
        }
        for (int e = 0; e < ne; ++e) leaf[e] = lba_pass_edge<SYSTEM>(V, G.C, e, buf);
        double chi = 0.0;
        for (int k = 0; k * LBA_T < ne; ++k) chi += lba_partial_host(leaf.data() + (size_t)k * LBA_T, std::min(LBA_T, ne - k * LBA_T));
        return chi;
    }
    void report(LbaReport* rep) { rep->want_trial = S.want_trial; rep->more = S.more; rep->ok = S.ok; rep->seq++; }
    int iteration(LbaReport* rep) {
        const double chi = pass<true>(S.cur);
        for (int l = 0; l < V.n_points; ++l) if (V.point_h[l] >= 0) lba_point_sum(V, l);
        for (int i = 0; i < V.na; ++i) for (int k = 0; k < 42; ++k) lba_pose_sum(V, i, k);
        double m = 0.;
        for (int v = 0; v < V.na + V.n_points; ++v) m = lba_max_diag(V, v, m);
        lm_rule_full(S, chi, m);
        return trial(rep);
    }
    int trial(LbaReport* rep) {
        const int n = 6 * V.na, buf = S.cur ^ 1;
        for (int l = 0; l < V.n_points; ++l) lba_point_damp_at(V, l, S.lambda);
        auto block = [&](int i1, int i2) {
            for (int r = 0; r < 6; ++r) for (int c = 0; c < 6; ++c) Hs[(size_t)(6 * i1 + r) * n + 6 * i2 + c] = lba_schur_entry(V, S.lambda, i1, i2, r, c);
        };
        if (global) for (size_t q = 0; q < T.pairs.size(); q += 2) block(T.pairs[q], T.pairs[q + 1]);
        for (int i1 = 0; i1 < V.na; ++i1) {
            if (!global) for (int i2 = i1; i2 < V.na; ++i2) block(i1, i2);
            for (int r = 0; r < 6; ++r) bs[6 * i1 + r] = lba_schur_b(V, i1, r);
        }
        S.ok2 = (global ? ba_ldlt_host : lba_ldlt_host)(n, Hs.data(), bs.data(), Lt.data(), d.data(), temp.data(), y.data(), x.data()) ? 1 : 0;
        for (int l = 0; l < V.n_points; ++l) lba_point_update(V, l, S.ok2, S.lambda, buf);
        for (int p = 0; p < V.n_poses; ++p) lba_pose_update(V, p, S.lambda, order, buf);
        const double temp_chi = pass<false>(buf);
        double scale = 0.;
        for (int j = 0; j < V.nx; ++j) scale += sterm[j];
        lba_ctl_trial_end(S, temp_chi, scale);
        if (!S.want_trial) lba_ctl_iter_end(S);
        report(rep);
        return ORB_OK;
    }
    int iter_end(LbaReport* rep) { lba_ctl_iter_end(S); report(rep); return ORB_OK; }
    int classify(int which) {
        for (int e = 0; e < G.n_edges; ++e) lba_classify_edge(V, G.C, e, which, S.cur);
        return ORB_OK;
    }
    int finish(orbm_lba_result* R) {
        lba_write_result(G.P, pose[S.cur].data(), point[S.cur].data(), R);
        R->round[0] = S.round[0]; R->round[1] = S.round[1];
        return ORB_OK;
    }
};

void lba_count_flags(int ne, orbm_lba_result* R) {
    R->n_level1 = 0; R->n_erase = 0;
    for (int e = 0; e < ne; ++e) { if (R->flags[e] & ORBM_LBA_FLAG_LEVEL1) ++R->n_level1; if (R->flags[e] & ORBM_LBA_FLAG_ERASE) ++R->n_erase; }
}
int lba_host(const orbm_lba_problem* P, orbm_lba_stop_fn stop, void* ctx, int order, orbm_lba_result* R) {
    LbaGraph G;
    lba_graph(P, G);
    LbaHost H(G, order, R->flags);
    const int rc = lba_flow(H, stop, ctx, R);
    if (rc) return rc;
    lba_count_flags(G.n_edges, R);
    return ORB_OK;
}

// ---- kernels -----------------------------------------------------------------------------------------------------------------------------
// both estimate buffers, x and the per-edge chi2 at the start of a call
__global__ __launch_bounds__(LBA_T) void k_lba_init(LbaView V, const double* pose0, const double* point0, LbaCtl S0) {
    const size_t t = (size_t)blockIdx.x * LBA_T + threadIdx.x, T = (size_t)gridDim.x * LBA_T;
    for (size_t k = t; k < 7 * (size_t)V.n_poses; k += T) { V.pose[0][k] = pose0[k]; V.pose[1][k] = pose0[k]; }
    for (size_t k = t; k < 3 * (size_t)V.n_points; k += T) { V.point[0][k] = point0[k]; V.point[1][k] = point0[k]; }
    for (size_t k = t; k < 6 * (size_t)V.n_free + 3 * (size_t)V.n_points; k += T) { V.x[k] = 0.0; V.sterm[k] = 0.0; }
    for (size_t k = t; k < (size_t)V.n_edges; k += T) { V.chi2[k] = 0.0; V.flags[k] = 0; }
    if (t == 0) *V.S = S0;
}
// the trial buffer starts as the estimate; the controller's record of the optimisation
__global__ __launch_bounds__(LBA_T) void k_lba_begin_optimisation(LbaView V, int max_iter) {
    const size_t t = (size_t)blockIdx.x * LBA_T + threadIdx.x, T = (size_t)gridDim.x * LBA_T;
    const int cur = V.S->cur;
    for (size_t k = t; k < 7 * (size_t)V.n_poses; k += T) V.pose[cur ^ 1][k] = V.pose[cur][k];
    for (size_t k = t; k < 3 * (size_t)V.n_points; k += T) V.point[cur ^ 1][k] = V.point[cur][k];
    __syncthreads();
    if (t == 0) lba_ctl_begin_optimisation(*V.S, V.stage, max_iter);   // (cur is not written)
}
// one lane per edge position; the workgroup's chi2 partial through lm_dev.h's tree
template <bool SYSTEM>
__global__ __launch_bounds__(LBA_T) void k_lba_edges(LbaView V, LbaCam C) {
    __shared__ double s_part[LBA_T / 64][1];
    const int e = blockIdx.x * LBA_T + threadIdx.x;
    const int buf = SYSTEM ? V.S->cur : V.S->cur ^ 1;
    double rho0[1] = {0.0};
    if (e < V.n_edges) rho0[0] = lba_pass_edge<SYSTEM>(V, C, e, buf);
    lm_wave_sums(rho0, 0, s_part, threadIdx.x);
    __syncthreads();
    if (threadIdx.x == 0) { lm_add_waves(s_part, rho0); V.partial[blockIdx.x] = rho0[0]; }
}
__global__ __launch_bounds__(LBA_T) void k_lba_point_sum(LbaView V) {
    const int l = blockIdx.x * LBA_T + threadIdx.x;
    if (l < V.n_points && V.point_h[l] >= 0) lba_point_sum(V, l);
}
// one wave per active pose: lanes 0 .. 41 own the entries of Hpp and bp
__global__ __launch_bounds__(64) void k_lba_pose_sum(LbaView V) {
    if (threadIdx.x < 42) lba_pose_sum(V, blockIdx.x, threadIdx.x);
}
// one workgroup: the pass's chi2 (the partials in ascending order), computeLambdaInit's maximum, the controller
__global__ __launch_bounds__(LBA_T) void k_lba_ctl_full(LbaView V, int n_partials) {
    __shared__ double s_m[LBA_T];
    double m = 0.;
    for (int v = threadIdx.x; v < V.na + V.n_points; v += LBA_T) m = lba_max_diag(V, v, m);
    s_m[threadIdx.x] = m;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int l = 1; l < LBA_T; ++l) if (s_m[l] > m) m = s_m[l];
    double chi = 0.0;
    for (int k = 0; k < n_partials; ++k) chi += V.partial[k];
    lm_rule_full(*V.S, chi, m);
}
__global__ __launch_bounds__(LBA_T) void k_lba_point_damp(LbaView V) {
    const int l = blockIdx.x * LBA_T + threadIdx.x;
    if (l < V.n_points) lba_point_damp_at(V, l, V.S->lambda);
}
// one wave per block (i1, i2), i2 >= i1, of the reduced system: lanes 0 .. 35 its entries, lanes 36 .. 41 of a diagonal block bschur
__global__ __launch_bounds__(64) void k_lba_schur(LbaView V) {
    // blockIdx.x -> (i1, i2): row i1 holds na - i1 blocks
    int i1 = 0, rest = blockIdx.x;
    while (rest >= V.na - i1) { rest -= V.na - i1; ++i1; }
    const int i2 = i1 + rest, n = 6 * V.na, t = threadIdx.x;
    const double lambda = V.S->lambda;
    if (t < 36) V.Hs[(size_t)(6 * i1 + t / 6) * n + 6 * i2 + t % 6] = lba_schur_entry(V, lambda, i1, i2, t / 6, t % 6);
    else if (t < 42 && i1 == i2) V.bs[6 * i1 + t - 36] = lba_schur_b(V, i1, t - 36);
}
// (global BA) the same wave per block, for the listed pairs only; the rest of the upper triangle is k_ba_fill_zero's
__global__ __launch_bounds__(64) void k_ba_schur_pairs(LbaView V, const int32_t* pairs) {
    const int i1 = pairs[2 * (size_t)blockIdx.x], i2 = pairs[2 * (size_t)blockIdx.x + 1], n = 6 * V.na, t = threadIdx.x;
    const double lambda = V.S->lambda;
    if (t < 36) V.Hs[(size_t)(6 * i1 + t / 6) * n + 6 * i2 + t % 6] = lba_schur_entry(V, lambda, i1, i2, t / 6, t % 6);
    else if (t < 42 && i1 == i2) V.bs[6 * i1 + t - 36] = lba_schur_b(V, i1, t - 36);
}
__global__ __launch_bounds__(LBA_T) void k_ba_fill_zero(double* p, size_t count) {
    for (size_t k = (size_t)blockIdx.x * LBA_T + threadIdx.x; k < count; k += (size_t)gridDim.x * LBA_T) p[k] = 0.0;
}
// One workgroup, lane i owns row i of the reduced system: the statements of lba_ldlt_host.  Column k: temp = D L(k, .), every row at
// or below k forms its inner product in ascending j, row k's is the pivot; the forward substitution accumulates L(i, j) y(j) as y(j)
// appears (ascending j for every row); the backward one needs x(i+1 ..) complete, so the rows at work multiply and row i adds the
// products in ascending j.
__global__ __launch_bounds__(LBA_SOLVE_T) void k_lba_solve(LbaView V) {
    __shared__ double s_temp[LBA_MAX_N], s_d[LBA_MAX_N], s_y[LBA_MAX_N], s_p[LBA_MAX_N];
    __shared__ double s_dk;
    __shared__ int s_fail;
    const int n = 6 * V.na, i = threadIdx.x;
    if (i == 0) s_fail = 0;
    __syncthreads();
    for (int k = 0; k < n; ++k) {
        if (i < k) s_temp[i] = s_d[i] * V.Lt[(size_t)i * n + k];
        __syncthreads();
        double r = 0.0;
        if (i >= k && i < n) {
            double s = 0.0;
            for (int j = 0; j < k; ++j) s += V.Lt[(size_t)j * n + i] * s_temp[j];
            r = V.Hs[(size_t)k * n + i] - s;
            if (i == k) { s_dk = r; s_d[k] = r; if (!(fabs(r) > 0) || !(fabs(r) <= DBL_MAX)) s_fail = 1; }
        }
        __syncthreads();
        if (s_fail) break;
        if (i > k && i < n) V.Lt[(size_t)k * n + i] = r / s_dk;
        __syncthreads();                                   // column k of L is visible: row k + 1 reads L(k + 1, k) from lane k + 1
    }
    if (s_fail) { if (i == 0) V.S->ok2 = 0; return; }
    double s = 0.0;
    for (int j = 0; j < n; ++j) {
        if (i == j) s_y[j] = V.bs[j] - s;
        __syncthreads();
        if (i > j && i < n) s += V.Lt[(size_t)j * n + i] * s_y[j];
    }
    __syncthreads();
    if (i < n) s_y[i] = s_y[i] / s_d[i];
    __syncthreads();
    for (int r = n - 1; r >= 0; --r) {
        if (i > r && i < n) s_p[i] = V.Lt[(size_t)r * n + i] * s_y[i];
        __syncthreads();
        if (i == r) { double t = 0.0; for (int j = r + 1; j < n; ++j) t += s_p[j]; s_y[r] = s_y[r] - t; }
        __syncthreads();
    }
    if (i < n) V.x[i] = s_y[i];
    if (i == 0) V.S->ok2 = 1;
}
// the landmarks' part of the solution and every active vertex's trial estimate: lanes 0 .. n_points-1 the points, the next n_poses the poses
__global__ __launch_bounds__(LBA_T) void k_lba_update(LbaView V) {
    const int t = blockIdx.x * LBA_T + threadIdx.x;
    const LbaCtl& S = *V.S;
    if (t < V.n_points) lba_point_update(V, t, S.ok2, S.lambda, S.cur ^ 1);
    else if (t - V.n_points < V.n_poses) lba_pose_update(V, t - V.n_points, S.lambda, ORBM_POSE_ORDER_DEVICE, S.cur ^ 1);
}
// One workgroup: the trial's chi2 and computeScale (both sequential; the lanes only stage the terms in LDS), the controller's verdict,
// and the iteration's end when no trial follows; the command word for the host.
__global__ __launch_bounds__(LBA_T) void k_lba_ctl_trial(LbaView V, int n_partials, uint32_t* word, int seq) {
    __shared__ double s_buf[8 * LBA_T];
    double scale = 0.;
    for (int base = 0; base < V.nx; base += 8 * LBA_T) {
        const int m = min(8 * LBA_T, V.nx - base);
        for (int k = threadIdx.x; k < m; k += LBA_T) s_buf[k] = V.sterm[base + k];
        __syncthreads();
        if (threadIdx.x == 0) for (int k = 0; k < m; ++k) scale += s_buf[k];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    double chi = 0.0;
    for (int k = 0; k < n_partials; ++k) chi += V.partial[k];
    LbaCtl& S = *V.S;
    lba_ctl_trial_end(S, chi, scale);
    if (!S.want_trial) lba_ctl_iter_end(S);
    *word = lba_command_word(S, seq);
}
__global__ void k_lba_iter_end(LbaView V, uint32_t* word, int seq) {
    LbaCtl& S = *V.S;
    lba_ctl_iter_end(S);
    *word = lba_command_word(S, seq);
}
__global__ __launch_bounds__(LBA_T) void k_lba_classify(LbaView V, LbaCam C, int which) {
    const int e = blockIdx.x * LBA_T + threadIdx.x;
    if (e < V.n_edges) lba_classify_edge(V, C, e, which, V.S->cur);
}
// the estimates and the controller's record into mapped memory
__global__ __launch_bounds__(LBA_T) void k_lba_finish(LbaView V, double* pose_out, double* point_out, LbaCtl* ctl_out) {
    const size_t t = (size_t)blockIdx.x * LBA_T + threadIdx.x, T = (size_t)gridDim.x * LBA_T;
    const int cur = V.S->cur;
    for (size_t k = t; k < 7 * (size_t)V.n_poses; k += T) pose_out[k] = V.pose[cur][k];
    for (size_t k = t; k < 3 * (size_t)V.n_points; k += T) point_out[k] = V.point[cur][k];
    if (t == 0) *ctl_out = *V.S;
}

// ---- the device backend ------------------------------------------------------------------------------------------------------------------
inline unsigned lba_blocks(size_t n) { return (unsigned)std::max<size_t>(1, (n + LBA_T - 1) / LBA_T); }

struct LbaDevice {
    orbm_matcher* m;
    const LbaGraph& G;
    LbaStructure T;
    LbaView V;
    morb::StagePack pk;
    std::optional<morb::StagePack::Block> blk_;   // (a Block comes from open() alone)
    int i_active, i_pose_h, i_point_h, i_pose_first, i_pose_edge, i_srow, i_nfree;
    uint32_t* rep_h; uint32_t* rep_d;   // the command word, host and device alias
    LbaCtl* ctl_h; LbaCtl* ctl_d;
    uint8_t* flags_h;
    double* pose_h; double* pose_d; double* point_h; double* point_d;
    int n_partials, seq = 0, launches = 0, syncs = 0;
    // the global BA: T is the caller's (one initializeOptimization() per call, known before the buffers are laid out), the reduced
    // system has 6 T.na rows, its blocks are T.pairs, its solver ba_ldlt_dev.h's
    bool global = false;
    int i_pairs = 0;
    BaSolve A;

    LbaDevice(orbm_matcher* mm, const LbaGraph& g) : m(mm), G(g) {}
    LbaDevice(orbm_matcher* mm, const LbaGraph& g, const LbaStructure& T0) : m(mm), G(g), T(T0), global(true) {}

    int sync(LbaReport* rep) {
        MORB_HIP(hipGetLastError());
        MORB_HIP(hipStreamSynchronize(m->stream));
        ++syncs;
        if (rep) {
            const uint32_t w = *rep_h;
            if ((int)(w >> 8) != seq) { morb::set_error("local BA: the command word of step %d did not arrive", seq); return ORB_E_HIP; }
            rep->want_trial = w & 1; rep->more = (w >> 1) & 1; rep->ok = (w >> 2) & 1; rep->seq = seq;
        }
        return ORB_OK;
    }
    int open() {
        const orbm_lba_problem* P = G.P;
        const size_t ne = (size_t)std::max(G.n_edges, 1), np = (size_t)std::max(P->n_poses, 1), nl = (size_t)std::max(P->n_points, 1),
                     nf = (size_t)std::max(P->n_free, 1), n6 = 6 * nf, n = global ? 6 * (size_t)std::max(T.na, 1) : n6;
        MORB_HIP(hipSetDevice(m->device));
        // the staged block: the graph, then the index arrays of an optimisation (written in place before either)
        const int i_K = pk.add(P->K, (size_t)P->n_poses * 20), i_first = pk.add(P->first, (size_t)(P->n_points + 1) * 4),
                  i_ep = pk.add(P->edge_pose, (size_t)G.n_edges * 4), i_el = pk.add(G.edge_point.data(), (size_t)G.n_edges * 4),
                  i_ec = pk.add(P->edge_cam, (size_t)G.n_edges), i_obs = pk.add(P->obs, (size_t)G.n_edges * 12),
                  i_w = pk.add(P->inv_sigma2, (size_t)G.n_edges * 4), i_bad = pk.add(G.bad.data(), nl),
                  i_p0 = pk.add(G.pose0.data(), 7 * np * 8), i_x0 = pk.add(G.point0.data(), 3 * nl * 8);
        i_active = pk.add_in_place(ne); i_pose_h = pk.add_in_place(np * 4); i_point_h = pk.add_in_place(nl * 4);
        i_pose_first = pk.add_in_place((nf + 1) * 4); i_pose_edge = pk.add_in_place(ne * 4); i_srow = pk.add_in_place(ne * 4);
        i_nfree = pk.add_in_place(nl * 4);
        if (global) i_pairs = pk.add_in_place(std::max<size_t>(T.pairs.size(), 2) * 4);
        int rc;
        blk_.emplace(pk.open(m->lba.stage, &rc));
        if (rc) return rc;
        const morb::StagePack::Block& blk = *blk_;
        // what the kernels leave for one another, in HBM
        morb::BlockLayout L;
        const size_t o_pose0 = L.take(7 * np * 8), o_pose1 = L.take(7 * np * 8), o_pt0 = L.take(3 * nl * 8), o_pt1 = L.take(3 * nl * 8),
                     o_E = L.take((size_t)LBA_EDGE_DOUBLES * ne * 8), o_chi2 = L.take(ne * 8), o_Hll = L.take(9 * nl * 8), o_bl = L.take(3 * nl * 8),
                     o_Dinv = L.take(9 * nl * 8), o_db = L.take(3 * nl * 8), o_Hpp = L.take(36 * nf * 8), o_bp = L.take(6 * nf * 8),
                     o_Hs = L.take(n * n * 8), o_bs = L.take(n * 8), o_Lt = L.take(n * n * 8), o_d = L.take(n * 8), o_x = L.take((n6 + 3 * nl) * 8),
                     o_st = L.take((n6 + 3 * nl) * 8), o_part = L.take((size_t)lba_blocks(ne) * 8), o_S = L.take(sizeof(LbaCtl));
        const size_t o_y = global ? L.take(n * 8) : 0, o_carry = global ? L.take(n * 8) : 0, o_fail = global ? L.take(16) : 0;
        if ((rc = m->lba.scratch.reserve(L.off))) return rc;
        // what the host reads: the command word, the controller's record, the flags, the estimates (mapped pinned)
        morb::BlockLayout O;
        const size_t q_rep = O.take(64), q_ctl = O.take(sizeof(LbaCtl)), q_flags = O.take(ne), q_pose = O.take(7 * np * 8), q_point = O.take(3 * nl * 8);
        if ((rc = m->lba.out.reserve(O.off))) return rc;
        uint8_t* hp = m->lba.out.p; uint8_t* dp = m->lba.out.dp; uint8_t* sp = m->lba.scratch.p;
        rep_h = (uint32_t*)(hp + q_rep); rep_d = (uint32_t*)(dp + q_rep); ctl_h = (LbaCtl*)(hp + q_ctl); ctl_d = (LbaCtl*)(dp + q_ctl);
        flags_h = hp + q_flags; pose_h = (double*)(hp + q_pose); pose_d = (double*)(dp + q_pose);
        point_h = (double*)(hp + q_point); point_d = (double*)(dp + q_point);
        *rep_h = 0;
        memset(&V, 0, sizeof(V));
        V.n_free = P->n_free; V.n_poses = P->n_poses; V.n_points = P->n_points; V.n_edges = G.n_edges;
        V.K = blk.dev<float>(i_K); V.first = blk.dev<int32_t>(i_first); V.edge_pose = blk.dev<int32_t>(i_ep); V.edge_point = blk.dev<int32_t>(i_el);
        V.edge_cam = blk.dev<uint8_t>(i_ec); V.obs = blk.dev<float>(i_obs); V.w = blk.dev<float>(i_w); V.bad = blk.dev<uint8_t>(i_bad);
        V.active = blk.dev<uint8_t>(i_active); V.pose_h = blk.dev<int32_t>(i_pose_h); V.point_h = blk.dev<int32_t>(i_point_h);
        V.pose_first = blk.dev<int32_t>(i_pose_first); V.pose_edge = blk.dev<int32_t>(i_pose_edge); V.srow = blk.dev<int32_t>(i_srow);
        V.nfree = blk.dev<int32_t>(i_nfree);
        V.pose[0] = (double*)(sp + o_pose0); V.pose[1] = (double*)(sp + o_pose1); V.point[0] = (double*)(sp + o_pt0); V.point[1] = (double*)(sp + o_pt1);
        V.E = (double*)(sp + o_E); V.chi2 = (double*)(sp + o_chi2); V.Hll = (double*)(sp + o_Hll); V.bl = (double*)(sp + o_bl);
        V.Dinv = (double*)(sp + o_Dinv); V.db = (double*)(sp + o_db); V.Hpp = (double*)(sp + o_Hpp); V.bp = (double*)(sp + o_bp);
        V.Hs = (double*)(sp + o_Hs); V.bs = (double*)(sp + o_bs); V.Lt = (double*)(sp + o_Lt); V.d = (double*)(sp + o_d);
        V.x = (double*)(sp + o_x); V.sterm = (double*)(sp + o_st); V.partial = (double*)(sp + o_part); V.S = (LbaCtl*)(sp + o_S);
        V.flags = dp + q_flags;
        if (global) A = BaSolve{0, V.Hs, V.bs, V.Lt, V.d, (double*)(sp + o_y), (double*)(sp + o_carry), V.x, (int*)(sp + o_fail), &V.S->ok2};
        n_partials = G.n_edges > 0 ? (int)lba_blocks(ne) : 0;
        blk.publish();
        LbaCtl S0;
        lba_ctl_begin(S0, ORBM_POSE_ORDER_DEVICE);
        hipLaunchKernelGGL(k_lba_init, dim3(lba_blocks(std::max(ne, 3 * nl))), dim3(LBA_T), 0, m->stream, V, blk.dev<double>(i_p0), blk.dev<double>(i_x0), S0);
        ++launches;
        return ORB_OK;
    }
    int begin_optimisation(int stage, int max_iter, int* n_vertices, orbm_lba_result* R) {
        int rc;
        if ((rc = sync(nullptr))) return rc;                  // the flags of the first test have arrived; nothing reads the index arrays
        if (!global) lba_structure(G, flags_h, T);
        const orbm_lba_problem* P = G.P;
        const morb::StagePack::Block& blk = *blk_;
        if (global) memcpy(blk.host<int32_t>(i_pairs), T.pairs.data(), T.pairs.size() * 4);
        memcpy(blk.host<uint8_t>(i_active), T.active.data(), (size_t)G.n_edges);
        memcpy(blk.host<int32_t>(i_pose_h), T.pose_h.data(), (size_t)P->n_poses * 4);
        memcpy(blk.host<int32_t>(i_point_h), T.point_h.data(), (size_t)P->n_points * 4);
        memcpy(blk.host<int32_t>(i_pose_first), T.pose_first.data(), (size_t)(T.na + 1) * 4);
        memcpy(blk.host<int32_t>(i_pose_edge), T.pose_edge.data(), (size_t)T.pose_first[T.na] * 4);
        memcpy(blk.host<int32_t>(i_srow), T.srow.data(), (size_t)G.n_edges * 4);
        memcpy(blk.host<int32_t>(i_nfree), T.nfree.data(), (size_t)P->n_points * 4);
        blk.publish();
        V.stage = stage; V.na = T.na; V.nl = T.nl; V.nx = 6 * T.na + 3 * T.nl;
        R->active_poses[stage] = T.na; R->active_points[stage] = T.nl; R->active_edges[stage] = T.n_active;
        hipLaunchKernelGGL(k_lba_begin_optimisation, dim3(1), dim3(LBA_T), 0, m->stream, V, max_iter);
        ++launches;
        if (global) {
            A.n = 6 * T.na;
            const size_t nn = (size_t)A.n * A.n;
            hipLaunchKernelGGL(k_ba_fill_zero, dim3(std::min(lba_blocks(nn), 4096u)), dim3(LBA_T), 0, m->stream, V.Hs, nn);
            ++launches;
        }
        *n_vertices = T.na + T.nl;
        return ORB_OK;
    }
    void enqueue_trial() {
        hipStream_t st = m->stream;
        hipLaunchKernelGGL(k_lba_point_damp, dim3(lba_blocks((size_t)V.n_points)), dim3(LBA_T), 0, st, V);
        if (global) {
            if (V.na > 0) hipLaunchKernelGGL(k_ba_schur_pairs, dim3((unsigned)(T.pairs.size() / 2)), dim3(64), 0, st, V, blk_->dev<int32_t>(i_pairs));
            launches += ba_ldlt_enqueue(st, A) - 1;          // (the count below holds one solve kernel)
        } else {
            if (V.na > 0) hipLaunchKernelGGL(k_lba_schur, dim3((unsigned)(V.na * (V.na + 1) / 2)), dim3(64), 0, st, V);
            hipLaunchKernelGGL(k_lba_solve, dim3(1), dim3(LBA_SOLVE_T), 0, st, V);
        }
        hipLaunchKernelGGL(k_lba_update, dim3(lba_blocks((size_t)V.n_points + (size_t)V.n_poses)), dim3(LBA_T), 0, st, V);
        hipLaunchKernelGGL(k_lba_edges<false>, dim3(lba_blocks((size_t)V.n_edges)), dim3(LBA_T), 0, st, V, G.C);
        hipLaunchKernelGGL(k_lba_ctl_trial, dim3(1), dim3(LBA_T), 0, st, V, n_partials, rep_d, ++seq);
        launches += V.na > 0 ? 6 : 5;
    }
    int iteration(LbaReport* rep) {
        hipStream_t st = m->stream;
        hipLaunchKernelGGL(k_lba_edges<true>, dim3(lba_blocks((size_t)V.n_edges)), dim3(LBA_T), 0, st, V, G.C);
        hipLaunchKernelGGL(k_lba_point_sum, dim3(lba_blocks((size_t)V.n_points)), dim3(LBA_T), 0, st, V);
        if (V.na > 0) hipLaunchKernelGGL(k_lba_pose_sum, dim3((unsigned)V.na), dim3(64), 0, st, V);
        hipLaunchKernelGGL(k_lba_ctl_full, dim3(1), dim3(LBA_T), 0, st, V, n_partials);
        launches += V.na > 0 ? 4 : 3;
        enqueue_trial();
        return sync(rep);
    }
    int trial(LbaReport* rep) { enqueue_trial(); return sync(rep); }
    int iter_end(LbaReport* rep) {
        hipLaunchKernelGGL(k_lba_iter_end, dim3(1), dim3(1), 0, m->stream, V, rep_d, ++seq);
        ++launches;
        return sync(rep);
    }
    int classify(int which) {
        hipLaunchKernelGGL(k_lba_classify, dim3(lba_blocks((size_t)V.n_edges)), dim3(LBA_T), 0, m->stream, V, G.C, which);
        ++launches;
        return ORB_OK;
    }
    int finish(orbm_lba_result* R) {
        hipLaunchKernelGGL(k_lba_finish, dim3(lba_blocks(std::max<size_t>(7 * (size_t)V.n_poses, 3 * (size_t)V.n_points))), dim3(LBA_T), 0, m->stream,
                           V, pose_d, point_d, ctl_d);
        ++launches;
        const int rc = sync(nullptr);
        if (rc) return rc;
        lba_write_result(G.P, pose_h, point_h, R);
        memcpy(R->flags, flags_h, (size_t)G.n_edges);
        R->round[0] = ctl_h->round[0]; R->round[1] = ctl_h->round[1];
        return ORB_OK;
    }
};

// lm_step's counterpart for orbm_lba_controller_trace: a 6-vector problem whose passes are the caller's chi2 stream
struct TraceCtl : LmState<6> {
    static constexpr bool LM_TRY_INLINE = true;
    __host__ __device__ void lm_trial() {}
    __host__ __device__ void lm_accept() {}
    __host__ __device__ void lm_linearise() { cmd = LM_CMD_FULL; }
};

// ---- the global BA's calls ---------------------------------------------------------------------------------------------------------------
// The backends write an orbm_lba_result: the call keeps one whose arrays are the caller's and whose flags (never set: nothing is
// tested) are its own, and takes the stage's record from it.
struct BaCall {
    std::vector<uint8_t> flags;
    orbm_lba_result L;
    int rc;
    BaCall(const orbm_lba_problem* P, int n_iterations, const orbm_ba_result* R) : flags(1, 0) {
        memset(&L, 0, sizeof(L));
        rc = check(P, n_iterations, R);
        if (rc) return;
        flags.assign((size_t)std::max(P->first[P->n_points], 1), 0);
        L.flags = flags.data();
    }
    int check(const orbm_lba_problem* P, int n_iterations, const orbm_ba_result* R) {
        MORB_ARG(P != nullptr && R != nullptr && n_iterations >= 0);
        L.pose = R->pose; L.Tcw = R->Tcw; L.point = R->point; L.point_f = R->point_f; L.flags = flags.data();
        return lba_validate(P, &L);
    }
    void take(int robust, orbm_ba_result* R) const {
        const int s = robust ? 0 : 1;
        R->round = L.round[s]; R->optimised = L.optimisations; R->polls = L.polls;
        R->active_poses = L.active_poses[s]; R->active_points = L.active_points[s]; R->active_edges = L.active_edges[s];
        for (int k = 0; k < 3; ++k) R->reserved[k] = 0;
    }
};
int ba_host(const LbaGraph& G, int n_iterations, int robust, orbm_lba_stop_fn stop, void* ctx, int order, BaCall& call, orbm_ba_result* R) {
    LbaHost H(G, order, call.flags.data(), true);
    const int rc = ba_flow(H, n_iterations, robust, stop, ctx, &call.L);
    if (rc) return rc;
    call.take(robust, R);
    return ORB_OK;
}

}  // namespace

extern "C" {

int orbm_bundle_adjust_host(const orbm_lba_problem* problem, int n_iterations, int robust, orbm_lba_stop_fn stop, void* stop_ctx, int order,
                            orbm_ba_result* result) {
    BaCall call(problem, n_iterations, result);
    if (call.rc) return call.rc;
    if (order != ORBM_POSE_ORDER_INDEX && order != ORBM_POSE_ORDER_DEVICE) { morb::set_error("order = %d", order); return ORB_E_ARG; }
    LbaGraph G;
    lba_graph(problem, G, false);
    return ba_host(G, n_iterations, robust, stop, stop_ctx, order, call, result);
}

int orbm_bundle_adjust(orbm_matcher* m, const orbm_lba_problem* problem, int n_iterations, int robust, orbm_lba_stop_fn stop, void* stop_ctx,
                       orbm_ba_result* result) {
    MORB_ARG(m != nullptr);
    BaCall call(problem, n_iterations, result);
    int rc = call.rc;
    if (rc) return rc;
    const int ne = problem->first[problem->n_points];
    const bool beyond = problem->n_free > ORBM_BA_MAX_FREE || problem->n_poses > ORBM_BA_MAX_POSES || problem->n_points > ORBM_BA_MAX_POINTS ||
                        ne > ORBM_BA_MAX_EDGES;
    LbaGraph G;
    lba_graph(problem, G, false);
    LbaStructure T;
    if (!beyond) lba_structure(G, call.flags.data(), T);      // the call's ONE initializeOptimization(): no flag is ever set
    for (int k = 0; k < 8; ++k) m->last_ba[k] = 0;
    if (beyond || T.na == 0) {
        rc = ba_host(G, n_iterations, robust, stop, stop_ctx, ORBM_POSE_ORDER_DEVICE, call, result);
        m->last_ba[0] = beyond ? 1 : 2; m->last_ba[3] = call.L.polls;
        return rc;
    }
    ba_block_pairs(G, T);
    LbaDevice D(m, G, T);
    if ((rc = D.open())) return rc;
    rc = ba_flow(D, n_iterations, robust, stop, stop_ctx, &call.L);
    if (rc) { (void)hipStreamSynchronize(m->stream); return rc; }
    call.take(robust, result);
    m->last_ba[1] = D.launches; m->last_ba[2] = D.syncs; m->last_ba[3] = result->polls;
    m->last_ba[4] = (int)(T.pairs.size() / 2); m->last_ba[5] = T.na * (T.na + 1) / 2; m->last_ba[6] = (6 * T.na + BA_PANEL - 1) / BA_PANEL;
    return ORB_OK;
}

int orbm_ba_ldlt(int n, const double* H, const double* b, double* x) {
    MORB_ARG(n >= 0 && n <= 6 * ORBM_BA_MAX_FREE && (n == 0 || (H && b && x)));
    std::vector<double> Lt((size_t)n * n + 1), d((size_t)n + 1), temp((size_t)n + 1), y((size_t)n + 1);
    return ba_ldlt_host(n, H, b, Lt.data(), d.data(), temp.data(), y.data(), x) ? 1 : 0;
}

int orbm_ba_ldlt_device(orbm_matcher* m, int n, const double* H, const double* b, double* x) {
    MORB_ARG(m != nullptr && n >= 0 && n <= 6 * ORBM_BA_MAX_FREE && (n == 0 || (H && b && x)));
    if (n == 0) return 1;
    MORB_HIP(hipSetDevice(m->device));
    const size_t nn = (size_t)n * n * 8, nv = (size_t)n * 8;
    morb::BlockLayout L;
    const size_t o_Hs = L.take(nn), o_Lt = L.take(nn), o_bs = L.take(nv), o_d = L.take(nv), o_y = L.take(nv), o_carry = L.take(nv), o_x = L.take(nv),
                 o_flag = L.take(16);
    const int rc = m->lba.scratch.reserve(L.off);
    if (rc) return rc;
    uint8_t* sp = m->lba.scratch.p;
    int* flag = (int*)(sp + o_flag);
    const BaSolve A = {n, (double*)(sp + o_Hs), (double*)(sp + o_bs), (double*)(sp + o_Lt), (double*)(sp + o_d), (double*)(sp + o_y),
                       (double*)(sp + o_carry), (double*)(sp + o_x), flag, flag + 1};
    MORB_HIP(hipMemcpyAsync(sp + o_Hs, H, nn, hipMemcpyHostToDevice, m->stream));
    MORB_HIP(hipMemcpyAsync(sp + o_bs, b, nv, hipMemcpyHostToDevice, m->stream));
    (void)ba_ldlt_enqueue(m->stream, A);
    MORB_HIP(hipGetLastError());
    int ok[2] = {0, 0};
    MORB_HIP(hipMemcpyAsync(ok, flag, 8, hipMemcpyDeviceToHost, m->stream));
    MORB_HIP(hipStreamSynchronize(m->stream));
    if (ok[1] != 1) return 0;
    MORB_HIP(hipMemcpy(x, sp + o_x, nv, hipMemcpyDeviceToHost));
    return 1;
}

int orbm_local_ba_host(const orbm_lba_problem* problem, orbm_lba_stop_fn stop, void* stop_ctx, int order, orbm_lba_result* result) {
    const int rc = lba_validate(problem, result);
    if (rc) return rc;
    if (order != ORBM_POSE_ORDER_INDEX && order != ORBM_POSE_ORDER_DEVICE) { morb::set_error("order = %d", order); return ORB_E_ARG; }
    return lba_host(problem, stop, stop_ctx, order, result);
}

int orbm_local_ba(orbm_matcher* m, const orbm_lba_problem* problem, orbm_lba_stop_fn stop, void* stop_ctx, orbm_lba_result* result) {
    MORB_ARG(m != nullptr);
    int rc = lba_validate(problem, result);
    if (rc) return rc;
    const int ne = problem->first[problem->n_points];
    const bool beyond = problem->n_free > ORBM_LBA_MAX_FREE || problem->n_poses > ORBM_LBA_MAX_POSES || problem->n_points > ORBM_LBA_MAX_POINTS ||
                        ne > ORBM_LBA_MAX_EDGES;
    if (beyond || problem->n_free == 0) {
        rc = lba_host(problem, stop, stop_ctx, ORBM_POSE_ORDER_DEVICE, result);
        m->last_lba[0] = beyond ? 1 : 2; m->last_lba[1] = 0; m->last_lba[2] = 0; m->last_lba[3] = result->polls;
        return rc;
    }
    LbaGraph G;
    lba_graph(problem, G);
    LbaDevice D(m, G);
    if ((rc = D.open())) return rc;
    rc = lba_flow(D, stop, stop_ctx, result);
    if (rc) { (void)hipStreamSynchronize(m->stream); return rc; }
    lba_count_flags(ne, result);
    m->last_lba[0] = 0; m->last_lba[1] = D.launches; m->last_lba[2] = D.syncs; m->last_lba[3] = result->polls;
    return ORB_OK;
}

int orbm_lba_edge_eval(const float* Tcim2x16, const float* K5, const double* pose7, const double* point3, int cam, const float* obs3,
                       float inv_sigma2, double* out32) {
    MORB_ARG(Tcim2x16 && K5 && pose7 && point3 && obs3 && out32 && (cam == 0 || cam == 1));
    LbaCam C;
    lba_camera((const float (*)[16])Tcim2x16, C);
    LbaEval o;
    lba_edge<true>(C, K5, pose7, point3, cam, !(obs3[2] < 0), obs3, (double)inv_sigma2, o);
    for (int k = 0; k < 3; ++k) out32[k] = o.e[k];
    out32[3] = o.chi2; out32[4] = o.zc;
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) out32[5 + 3 * r + c] = o.A[r][c]; for (int c = 0; c < 6; ++c) out32[14 + 6 * r + c] = o.B[r][c]; }
    return ORB_OK;
}

int orbm_lba_ldlt(int n, const double* H, const double* b, double* x) {
    MORB_ARG(n >= 0 && n <= LBA_MAX_N + 6 && (n == 0 || (H && b && x)));
    std::vector<double> Lt((size_t)n * n + 1), d((size_t)n + 1), temp((size_t)n + 1), y((size_t)n + 1);
    return lba_ldlt_host(n, H, b, Lt.data(), d.data(), temp.data(), y.data(), x) ? 1 : 0;
}

int orbm_lba_controller_trace(const double* chi, int n_chi, const double* hdiag6, const double* b6, int max_iter, int order, int max_steps,
                              double* out_lba, double* out_lm) {
    MORB_ARG(chi && hdiag6 && b6 && out_lba && out_lm && n_chi >= 0 && max_iter >= 1 && max_steps >= 0);
    // The two DRIVERS of lm_dev.h's rules on one chi2 stream: the rules are one definition, so what can still drift apart is the
    // sequencing -- lm_step's commands against the local BA's cuts (want_trial / more / ok) -- and that is what the two traces hold.
    // lm_step on its record
    TraceCtl L;
    memset(&L, 0, sizeof(L));
    L.order = order; L.iter = 0; L.max_iter = max_iter; L.ok2 = 1; L.ni = 2; L.cmd = LM_CMD_FULL;
    orbm_pose_round RL = {0, 0, 0., 0.};
    double sum[TraceCtl::NSUM];
    int steps_lm = 0;
    for (int k = 0; k < n_chi && steps_lm < max_steps && L.cmd != LM_CMD_CLASSIFY; ++k) {
        for (int q = 0; q < TraceCtl::NSUM; ++q) sum[q] = 0.;
        if (L.cmd == LM_CMD_FULL) { int dgn = 0; for (int j = 0; j < 6; ++j) { sum[dgn] = hdiag6[j]; dgn += 6 - j; } for (int j = 0; j < 6; ++j) sum[TraceCtl::NH + j] = b6[j]; }
        sum[TraceCtl::CHI] = chi[k];
        lm_step(L, sum, RL);
        out_lm[3 * steps_lm] = L.lambda; out_lm[3 * steps_lm + 1] = L.ni;
        out_lm[3 * steps_lm + 2] = L.cmd == LM_CMD_CHI ? 1. : L.cmd == LM_CMD_FULL ? 2. : 3.;
        ++steps_lm;
    }
    // the local BA's driver on the same stream: the same 6x6 solve, computeScale over x
    LbaCtl S;
    lba_ctl_begin(S, order);
    lba_ctl_begin_optimisation(S, 0, max_iter);
    double x[6] = {0, 0, 0, 0, 0, 0}, A[36], temp[6];
    int transp[6], steps = 0, k = 0;
    bool full = true, done = false;
    while (k < n_chi && steps < max_steps && !done) {
        if (full) {
            double md = 0.;
            for (int j = 0; j < 6; ++j) if (fabs(hdiag6[j]) > md) md = fabs(hdiag6[j]);
            lm_rule_full(S, chi[k++], md);
        } else {
            double scale = 0.;
            for (int j = 0; j < 6; ++j) scale += x[j] * (S.lambda * x[j] + b6[j]);
            lba_ctl_trial_end(S, chi[k++], scale);
            if (!S.want_trial) lba_ctl_iter_end(S);
        }
        double verdict;
        if (full || S.want_trial) {                      // a trial follows: H + lambda, the dense solve
            for (int q = 0; q < 36; ++q) A[q] = 0.;
            for (int j = 0; j < 6; ++j) { A[7 * j] = hdiag6[j]; A[7 * j] += S.lambda; }
            S.ok2 = eigen_ldlt_solve<6>(A, b6, x, temp, transp) ? 1 : 0;
            verdict = 1.; full = false;
        } else if (S.more && S.ok) { verdict = 2.; full = true; }
        else { verdict = 3.; done = true; }
        out_lba[3 * steps] = S.lambda; out_lba[3 * steps + 1] = S.ni; out_lba[3 * steps + 2] = verdict;
        ++steps;
    }
    return steps == steps_lm ? steps : -1 - steps;
}

}  // extern "C"
