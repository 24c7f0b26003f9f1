// pose.hip -- motion-only pose optimisation on the device (include/orbm.h, "pose optimisation"): Optimizer::PoseOptimization(Frame*)
// (reference src/Optimizer.cc:352-618) and PoseOptimization(Frame*, bool bAllCams) (:620-898) from the edge list on, with the parts of
// g2o they run restated (Thirdparty/g2o/g2o/: types/types_six_dof_expmap.{h,cpp}, types/se3quat.h, types/se3_ops.hpp,
// core/base_unary_edge.hpp, core/base_edge.h, core/robust_kernel_impl.cpp, core/optimization_algorithm_levenberg.cpp,
// core/sparse_optimizer.cpp, solvers/linear_solver_dense.h) and the Eigen operators those call.
//   eigen_*, se3_*, g2o_*   the Eigen operators, g2o::SE3Quat, the Huber kernel and the Jacobian chain of the edges through Tcim, which
//                    the local bundle adjustment runs too: g2o_dev.h (UNPINNED).
//   pose_edge        one edge: error, chi2 and the Jacobian of its type, ONE statement sequence for the kernel and the host routine.
//   pose_step        the controller: everything between two passes over the edges as a resumable state machine over a PoseCtl record.
//                    The Levenberg rules and the 6x6 solve are lm_dev.h's lm_step (ONE definition, sim3opt.hip runs it too); the exp
//                    map, rounds and classification are here.  Host routine and lane 0 (on the record in LDS) call the same statements.
//   k_pose_optimize  one workgroup of 256 lanes per problem, resident for the whole call.  Per pass: every lane evaluates its edges
//                    (lane l owns l, l + 256, ...; the first eight of them stay in registers, a longer tail streams from the staged
//                    edge arrays) and sums 21 + 6 + 1 + 1 doubles over them in ascending order; lm_dev.h's summation tree (butterfly in
//                    each wave, the four waves in wave order) gives lane 0 the pass's sums, and lane 0 runs pose_step.  Two barriers
//                    per pass, no atomics, no order that depends on arrival.  The host routine walks the same tree (lm_pass_host).
// No libm function runs in the kernel: + - * / sqrt in double (the correctly rounded sequences), conversions.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/orbm.h"
#include "../../include/orb_debug.h"
#include "orb_common.h"
#include "matcher_internal.h"
#include "cv_dev.h"
#include "g2o_dev.h"
#include "lm_dev.h"
#include "stage_pack.h"

namespace {

constexpr int POSE_REG_SLOTS = 8;    // edges per lane whose constants stay in registers
// the sums of a pass (lm_dev.h): H upper triangle (21, row-major i <= j), b (6), robust chi2, outlier count
constexpr int POSE_NSUM = LmState<6>::NSUM, POSE_CHI = LmState<6>::CHI, POSE_BAD = LmState<6>::COUNT;

struct PoseCam {                         // per problem: the members of the edges that do not depend on the edge
    double fx, fy, cx, cy, bf;
    SE3Quat Tc[2];                       // Tcim[cam] (:659-666); read in the all-cameras mode only
    double Rc[2][9];                     // Tcim_quat.to_homogeneous_matrix().block(0,0,3,3)
    double delta[2], dsqr[2];            // RobustKernelHuber::_delta (double) and dsqr (a FLOAT member) of a mono / stereo edge
    int multi, n_cam0;
};
struct PoseEdge { float X[3], obs[3], inv_sigma2; int meta; };   // meta: bit 0 camera, bit 1 stereo, bit 2 slot in use

// ---- one edge ---------------------------------------------------------------------------------------------------------------------------
// computeError and chi2 of the edge's type; with want_jacobian also linearizeOplus (J: D rows of 6).  Returns chi2 = e . (Omega e) with
// Omega = Identity * (double)invSigma2.
__host__ __device__ inline double pose_edge(const PoseCam& C, const SE3Quat& T, const PoseEdge& E, double* e, bool want_jacobian, double (*J)[6]) {
    const int cam = E.meta & 1;
    const bool stereo = (E.meta & 2) != 0;
    const double Xw[3] = {(double)E.X[0], (double)E.X[1], (double)E.X[2]};
    double p[3], pc[3];
    se3_map(T, Xw, p);                                   // v1->estimate().map(Xw)
    if (C.multi) se3_map(C.Tc[cam], p, pc);              // Tcim_quat.map(...), also where it is the identity
    else { pc[0] = p[0]; pc[1] = p[1]; pc[2] = p[2]; }
    if (!stereo) {
        const double proj0 = pc[0] / pc[2], proj1 = pc[1] / pc[2];            // project2d
        e[0] = (double)E.obs[0] - (proj0 * C.fx + C.cx);
        e[1] = (double)E.obs[1] - (proj1 * C.fy + C.cy);
        e[2] = 0.0;
    } else {
        const float invz = (float)(1.0 / pc[2]);                               // `const float invz = 1.0f/trans_xyz[2]`
        const double r0 = pc[0] * (double)invz * C.fx + C.cx;
        const double r1 = pc[1] * (double)invz * C.fy + C.cy;
        // the one term where this edge (EdgeStereoSE3ProjectXYZOnlyPose::cam_project: the member bf, a double product) and lba_dev.h's
        // lba_edge (EdgeStereoSE3ProjectXYZ::cam_project: `const float& bf`, a float product) differ: two reference functions, not to be merged
        const double r2 = r0 - C.bf * (double)invz;
        e[0] = (double)E.obs[0] - r0; e[1] = (double)E.obs[1] - r1; e[2] = (double)E.obs[2] - r2;
    }
    const double w = (double)E.inv_sigma2;
    double chi2 = e[0] * (w * e[0]) + e[1] * (w * e[1]);
    if (stereo) chi2 = chi2 + e[2] * (w * e[2]);
    if (!want_jacobian) return chi2;
    if (!C.multi) {                                       // the closed expressions of the plain edges (:495-517, :883-912)
        const double x = p[0], y = p[1], invz = 1.0 / p[2], invz_2 = invz * invz;
        J[0][0] = x * y * invz_2 * C.fx;
        J[0][1] = -(1 + (x * x * invz_2)) * C.fx;
        J[0][2] = y * invz * C.fx;
        J[0][3] = -invz * C.fx;
        J[0][4] = 0;
        J[0][5] = x * invz_2 * C.fx;
        J[1][0] = (1 + y * y * invz_2) * C.fy;
        J[1][1] = -x * y * invz_2 * C.fy;
        J[1][2] = -x * invz * C.fy;
        J[1][3] = 0;
        J[1][4] = -invz * C.fy;
        J[1][5] = y * invz_2 * C.fy;
        if (stereo) {
            J[2][0] = J[0][0] - C.bf * y * invz_2;
            J[2][1] = J[0][1] + C.bf * x * invz_2;
            J[2][2] = J[0][2];
            J[2][3] = J[0][3];
            J[2][4] = 0;
            J[2][5] = J[0][5] - C.bf * invz_2;
        }
    } else {                                              // the _multi edges multiply by Rcim, the identity included (:627-696, :952-1036)
        double t2[3][3];
        g2o_cam_jacobian_rows(C.fx, C.fy, C.bf, C.Rc[cam], pc, true, t2);   // row 2 always, read below for a stereo edge only
        const int D = stereo ? 3 : 2;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (k >= D) continue;
            g2o_cam_jacobian_pose(t2[k], p, J[k]);
        }
    }
    return chi2;
}

// One ACTIVE edge's share of a pass (computeActiveErrors + activeRobustChi2, with `system` also linearizeOplus + constructQuadraticForm,
// core/base_unary_edge.hpp:44-72): acc[POSE_CHI] += rho[0]; b -= rho[1] * J^T (Omega e); H += J^T (rho[1] Omega) J.  The edge's own 6-vector
// and 6x6 are formed first (rows of J in order) and then added, as the edge adds its products to the vertex.  UNPINNED: Eigen's
// evaluation order inside the two products.
__host__ __device__ inline void pose_accumulate(const PoseCam& C, const SE3Quat& T, const PoseEdge& E, bool system, bool robust, double* acc) {
    double e[3], J[3][6];
    const bool stereo = (E.meta & 2) != 0;
    const double chi2 = pose_edge(C, T, E, e, system, J);
    double rho0 = chi2, rho1 = 1.;
    if (robust) g2o_huber(chi2, C.delta[stereo ? 1 : 0], C.dsqr[stereo ? 1 : 0], &rho0, &rho1);
    acc[POSE_CHI] += rho0;
    if (!system) return;
    const double w = (double)E.inv_sigma2, rw = rho1 * w;
    const double we[3] = {w * e[0], w * e[1], w * e[2]};
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j, ++k) {
            double h = (J[0][i] * rw) * J[0][j] + (J[1][i] * rw) * J[1][j];
            if (stereo) h = h + (J[2][i] * rw) * J[2][j];
            acc[k] += h;
        }
        double g = J[0][i] * we[0] + J[1][i] * we[1];
        if (stereo) g = g + J[2][i] * we[2];
        acc[21 + i] -= rho1 * g;
    }
}

// the classification of one edge after a round (:541-597): an outlier's error is recomputed at the estimate, an inlier keeps the error
// of the last computeActiveErrors (the pose of the last pass, which is the REJECTED trial when the round ended on one)
__host__ __device__ inline bool pose_classify(const PoseCam& C, const SE3Quat& est, const SE3Quat& last, const PoseEdge& E, bool was_outlier) {
    double e[3], J[3][6];
    const float chi2 = (float)pose_edge(C, was_outlier ? est : last, E, e, false, J);
    return (E.meta & 2) ? chi2 > 7.815f : chi2 > 5.991f;
}

// ---- the controller ---------------------------------------------------------------------------------------------------------------------
struct PoseCtl : LmState<6> {
    static constexpr bool LM_TRY_INLINE = false;
    int n, round, robust, n_bad;
    // eval: the pose of the next pass; last: of the last FULL / CHI pass.  est and last aligned: the kernel reads them with 128-bit LDS loads
    alignas(16) SE3Quat est; SE3Quat eval; alignas(16) SE3Quat last; SE3Quat start;
    orbm_pose_result res;
    // what lm_step leaves to the port
    __host__ __device__ __forceinline__ void lm_trial() {   // oplusImpl: setEstimate(SE3Quat::exp(update) * estimate())
        SE3Quat d;
        se3_exp(x, order, d);
        se3_mul(d, est, eval);
    }
    __host__ __device__ __forceinline__ void lm_accept() { est = eval; }
    __host__ __device__ __forceinline__ void lm_linearise() { eval = est; cmd = LM_CMD_FULL; }
};

__host__ __device__ inline void pose_write_estimate(PoseCtl& S) {
    se3_to_cv(S.est, S.res.Tcw);
    for (int k = 0; k < 4; ++k) S.res.q[k] = x86_nan(S.est.q[k]);
    for (int k = 0; k < 3; ++k) S.res.t[k] = x86_nan(S.est.t[k]);
}

__host__ __device__ inline void pose_begin_round(PoseCtl& S) {
    S.est = S.start;                         // vSE3->setEstimate(Converter::toSE3Quat(pFrame->mTcw))
    S.iter = 0; S.max_iter = 10;             // optimizer.optimize(its[it]), its = {10, 10, 10, 10}
    // initializeOptimization(0) finds no edge of level 0 when every edge is an outlier: optimize() returns at once
    if (S.n - S.n_bad <= 0) { S.cmd = LM_CMD_CLASSIFY; return; }
    S.lm_linearise();
}
__host__ __device__ inline void pose_begin(PoseCtl& S, const float* Tcw, int n, int order) {
    S.order = order; S.n = n; S.round = 0; S.robust = 1; S.n_bad = 0; S.ok2 = 1;
    S.lambda = 0; S.ni = 2; S.current_chi = 0; S.ini_chi = 0; S.n_bad_steps = 0; S.qmax = 0;
    for (int i = 0; i < 6; ++i) S.x[i] = 0;
    se3_from_cv(Tcw, S.start);
    S.est = S.start; S.last = S.start; S.eval = S.start;
    memset(&S.res, 0, sizeof(S.res));
    S.res.n_initial = n;
    if (n < 3) {                             // `if(nInitialCorrespondences<3) return 0;`: the pose is not touched
        for (int i = 0; i < 16; ++i) S.res.Tcw[i] = Tcw[i];
        for (int k = 0; k < 4; ++k) S.res.q[k] = x86_nan(S.start.q[k]);
        for (int k = 0; k < 3; ++k) S.res.t[k] = x86_nan(S.start.t[k]);
        S.cmd = LM_CMD_DONE;
        return;
    }
    pose_begin_round(S);
}
// Called after every pass with the pass's sums.
__host__ __device__ inline void pose_step(PoseCtl& S, const double* sum) {
    orbm_pose_round& R = S.res.round[S.round];
    if (S.cmd != LM_CMD_CLASSIFY) {          // a FULL or a CHI pass: one step of the Levenberg loop
        S.last = S.eval;
        lm_step(S, sum, R);
        return;
    }
    // LM_CMD_CLASSIFY: the round is over
    S.n_bad = (int)sum[POSE_BAD];
    S.res.n_bad = S.n_bad;
    S.res.rounds = S.round + 1;
    if (S.round == 2) S.robust = 0;          // `if(it==2) e->setRobustKernel(0)`
    if (S.n < 10 || S.round == 3) {          // `if(optimizer.edges().size()<10) break;`
        S.res.n_inliers = S.res.n_initial - S.n_bad;
        pose_write_estimate(S);
        S.cmd = LM_CMD_DONE;
        return;
    }
    S.round++;
    pose_begin_round(S);
}

// the constants of a problem (:452-456, :497-501, :653-666, :410-411)
__host__ __device__ inline void pose_camera(const orbm_pose_problem& P, PoseCam& C) {
    C.fx = (double)P.fx; C.fy = (double)P.fy; C.cx = (double)P.cx; C.cy = (double)P.cy; C.bf = (double)P.bf;
    C.multi = P.mode == ORBM_POSE_ALL_CAMS ? 1 : 0; C.n_cam0 = P.n_cam0;
    // Tcam11 = eye; Tcam21 = [Rcam12.t() | -Rcam12.t() * tcam12] in float: cv::gemm's small path (cv_dev.h cv_gemm3) over a column of
    // Rcam12, alpha = -1, no C
    float T11[16], T21[16];
    for (int i = 0; i < 16; ++i) { T11[i] = i % 5 == 0 ? 1.0f : 0.0f; T21[i] = 0.0f; }
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) T21[4 * r + c] = P.Rcam12[3 * c + r];
        T21[4 * r + 3] = cv_gemm3(P.Rcam12 + r, 3, P.tcam12, -1.0, 0.0f, 0.0);
    }
    T21[15] = 1.0f;
    se3_from_cv(T11, C.Tc[0]);
    se3_from_cv(T21, C.Tc[1]);
    eigen_quat_to_matrix(C.Tc[0].q, C.Rc[0]);
    eigen_quat_to_matrix(C.Tc[1].q, C.Rc[1]);
    g2o_huber_constants(C.delta, C.dsqr);
}

__host__ __device__ inline int pose_meta(const orbm_pose_problem& P, int feat, float uright) {
    const int cam = (P.mode == ORBM_POSE_ALL_CAMS && feat >= P.n_cam0) ? 1 : 0;
    return cam | (uright < 0 ? 0 : 2) | 4;
}

// ---- the kernel -------------------------------------------------------------------------------------------------------------------------
struct PoseDev {
    const orbm_pose_problem* prob;     // per problem
    const int32_t* first;              // CSR, per problem + 1
    const int32_t* list;               // the problems this launch works on (blockIdx.x -> problem)
    // the plain form: the caller's arrays, staged
    const int32_t* feat; const float* pos; const float* obs; const int32_t* octave;
    // the resident form (packed != NULL): feature << 16 | table row per edge; the frame's arrays and the point table in HBM
    const uint32_t* packed; const float* un_x; const float* un_y; const float* uright; const int32_t* f_octave; const orbm_point* rows;
    uint8_t* flags;                    // per edge, mapped pinned
    orbm_pose_result* res;             // per problem, mapped pinned
};

__device__ __forceinline__ PoseEdge pose_load(const PoseDev& A, const orbm_pose_problem& P, int e) {
    PoseEdge E;
    int feat, oct;
    if (A.packed) {
        const uint32_t w = A.packed[e];
        feat = (int)(w >> 16);
        const orbm_point& row = A.rows[w & 0xffffu];
        E.X[0] = row.pos[0]; E.X[1] = row.pos[1]; E.X[2] = row.pos[2];
        E.obs[0] = A.un_x[feat]; E.obs[1] = A.un_y[feat]; E.obs[2] = A.uright[feat];
        oct = A.f_octave[feat];
    } else {
        feat = A.feat[e];
        E.X[0] = A.pos[3 * (size_t)e]; E.X[1] = A.pos[3 * (size_t)e + 1]; E.X[2] = A.pos[3 * (size_t)e + 2];
        E.obs[0] = A.obs[3 * (size_t)e]; E.obs[1] = A.obs[3 * (size_t)e + 1]; E.obs[2] = A.obs[3 * (size_t)e + 2];
        oct = A.octave[e];
    }
    oct = min(max(oct, 0), ORBM_MAX_LEVELS - 1);   // (validated on the host where the host has the octaves; the table is never indexed beyond its end)
    E.inv_sigma2 = P.inv_level_sigma2[oct];
    E.meta = pose_meta(P, feat, E.obs[2]);
    return E;
}

__host__ __device__ __forceinline__ void pose_pass_edge(const PoseCam& C, const PoseCtl& S, int cmd, const PoseEdge& E, uint8_t* flag, double* acc) {
    if (cmd == LM_CMD_CLASSIFY) {
        const bool out = pose_classify(C, S.est, S.last, E, *flag != 0);
        *flag = out ? 1 : 0;
        acc[POSE_BAD] += out ? 1.0 : 0.0;
    } else if (!*flag) {
        pose_accumulate(C, S.eval, E, cmd == LM_CMD_FULL, S.robust != 0, acc);
    }
}

__global__ __launch_bounds__(LM_T) void k_pose_optimize(PoseDev A) {
    __shared__ PoseCtl S;
    __shared__ PoseCam C;
    __shared__ double s_part[LM_T / 64][POSE_NSUM];
    __shared__ uint8_t s_flag[ORBM_POSE_CAP];
    const int tid = threadIdx.x;
    const int pb = A.list[blockIdx.x];
    const orbm_pose_problem& P = A.prob[pb];
    const int e0 = A.first[pb];
    const int n = min(A.first[pb + 1] - e0, (int)ORBM_POSE_CAP);   // (a longer problem never reaches the device)
    if (tid == 0) { pose_camera(P, C); pose_begin(S, P.Tcw, n, ORBM_POSE_ORDER_DEVICE); }
    for (int e = tid; e < n; e += LM_T) s_flag[e] = 0;
    PoseEdge reg[POSE_REG_SLOTS];
#pragma unroll
    for (int s = 0; s < POSE_REG_SLOTS; ++s) {
        const int e = tid + s * LM_T;
        if (e < n) reg[s] = pose_load(A, P, e0 + e);
        else { reg[s].X[0] = reg[s].X[1] = reg[s].X[2] = 0.0f; reg[s].obs[0] = reg[s].obs[1] = reg[s].obs[2] = 0.0f; reg[s].inv_sigma2 = 0.0f; reg[s].meta = 0; }
    }
    for (;;) {
        __syncthreads();                                   // the controller's record is visible
        const int cmd = S.cmd;
        if (cmd == LM_CMD_DONE) break;
        double acc[POSE_NSUM];
#pragma unroll
        for (int k = 0; k < POSE_NSUM; ++k) acc[k] = 0.0;
        // this lane's edges in ascending order: ONE copy of the edge code; a slot's constants are selected out of the registers
        for (int s = 0, e = tid; e < n; ++s, e += LM_T) {
            PoseEdge E;
            if (s < POSE_REG_SLOTS) {
                E = reg[0];
#pragma unroll
                for (int k = 1; k < POSE_REG_SLOTS; ++k) if (s == k) E = reg[k];
            } else {
                E = pose_load(A, P, e0 + e);
            }
            pose_pass_edge(C, S, cmd, E, &s_flag[e], acc);
        }
        // lm_dev.h's lm_wave_sums, written out: as a function it costs this kernel 101 more AGPRs and 361 more copies to and from them,
        // most of them in the loop over the edges (profiles/r17/notes_lm_refactor.md).  (Skipped: exact zeros that nobody reads.)
#pragma unroll
        for (int k = 0; k < POSE_NSUM; ++k) {
            if (cmd != LM_CMD_FULL && k < POSE_CHI) continue;
            acc[k] = lm_wave_sum(acc[k]);
        }
        if ((tid & 63) == 0) {
#pragma unroll
            for (int k = 0; k < POSE_NSUM; ++k) s_part[tid >> 6][k] = acc[k];
        }
        __syncthreads();                                   // the four waves' sums are visible, every lane is done with the record
        if (tid == 0) {
            double sum[POSE_NSUM];
            lm_add_waves(s_part, sum);
            pose_step(S, sum);
        }
    }
    for (int e = tid; e < n; e += LM_T) A.flags[e0 + e] = s_flag[e];
    if (tid == 0) A.res[pb] = S.res;
}

// ---- host routine -----------------------------------------------------------------------------------------------------------------------
struct PoseEdges { const int32_t* feat; const float* pos; const float* obs; const int32_t* octave; };

PoseEdge host_edge(const orbm_pose_problem& P, const PoseEdges& G, int e) {
    PoseEdge E;
    for (int k = 0; k < 3; ++k) { E.X[k] = G.pos[3 * (size_t)e + k]; E.obs[k] = G.obs[3 * (size_t)e + k]; }
    E.inv_sigma2 = P.inv_level_sigma2[G.octave[e]];
    E.meta = pose_meta(P, G.feat[e], E.obs[2]);
    return E;
}

// one problem; edges e0 .. e0 + n - 1 of G, flags[0 .. n-1]
void pose_problem_host(const orbm_pose_problem& P, const PoseEdges& G, int e0, int n, int order, uint8_t* flags, orbm_pose_result& res) {
    PoseCam C;
    PoseCtl S;
    pose_camera(P, C);
    pose_begin(S, P.Tcw, n, order);
    for (int e = 0; e < n; ++e) flags[e] = 0;
    std::vector<PoseEdge> E((size_t)n);
    for (int e = 0; e < n; ++e) E[e] = host_edge(P, G, e0 + e);
    std::vector<double> part;
    while (S.cmd != LM_CMD_DONE) {
        double sum[POSE_NSUM];
        const int cmd = S.cmd;
        lm_pass_host<POSE_NSUM>(order, n, part, sum, [&](int e, double* acc) { pose_pass_edge(C, S, cmd, E[e], &flags[e], acc); });
        pose_step(S, sum);
    }
    res = S.res;
}

int validate(const orbm_pose_problem* problems, int B, const int32_t* first, const int32_t* feat, const float* pos, const float* obs,
             const int32_t* octave, const uint8_t* outlier_out, const orbm_pose_result* results) {
    MORB_ARG(problems && first && results);
    if (const int rc = morb::validate_csr(B, ORBM_POSE_MAX_BATCH, first)) return rc;
    for (int b = 0; b < B; ++b) {
        const orbm_pose_problem& P = problems[b];
        if (P.mode != ORBM_POSE_CAM0 && P.mode != ORBM_POSE_ALL_CAMS) { morb::set_error("problem %d: mode = %d", b, P.mode); return ORB_E_ARG; }
        if (P.n_levels < 1 || P.n_levels > ORBM_MAX_LEVELS) { morb::set_error("problem %d: n_levels = %d is outside 1..%d", b, P.n_levels, (int)ORBM_MAX_LEVELS); return ORB_E_ARG; }
    }
    const int ne = first[B];
    if (ne > 0 && !(feat && pos && obs && octave && outlier_out)) { morb::set_error("an edge array is NULL"); return ORB_E_ARG; }
    for (int b = 0; b < B; ++b)
        for (int e = first[b]; e < first[b + 1]; ++e) {
            if (octave[e] < 0 || octave[e] >= problems[b].n_levels) { morb::set_error("edge %d: octave %d is outside the %d levels of problem %d", e, octave[e], problems[b].n_levels, b); return ORB_E_ARG; }
            if (feat[e] < 0) { morb::set_error("edge %d: feature index %d", e, feat[e]); return ORB_E_ARG; }
        }
    return ORB_OK;
}

// Stages the problems, the CSR, the work list and the form's own edge arrays (plain: feat, pos, obs, octave; resident, marked by
// A.packed != NULL: the packed words); launches; leaves records and flags in m->pose.out.  flags_off: where the flags start there.
int launch(orbm_matcher* m, const orbm_pose_problem* problems, int B, const int32_t* first, const std::vector<int32_t>& list, PoseDev A,
           const void* const* edge_src, const size_t* edge_len, int n_arrays, size_t* flags_off) {
    const int ne = first[B];
    morb::StagePack pk;
    const int i_prob = pk.add(problems, (size_t)B * sizeof(orbm_pose_problem)), i_first = pk.add(first, (size_t)(B + 1) * 4),
              i_list = pk.add(list.data(), list.size() * 4);
    int i_edge[4];
    for (int k = 0; k < n_arrays; ++k) i_edge[k] = pk.add(edge_src[k], edge_len[k]);
    const size_t res_bytes = morb::align16((size_t)B * sizeof(orbm_pose_result));
    int rc;
    const morb::StagePack::Block blk = pk.open(m->pose.stage, &rc);
    if (rc || (rc = m->pose.out.reserve(res_bytes + (size_t)std::max(ne, 1)))) return rc;
    blk.publish();
    A.prob = blk.dev<orbm_pose_problem>(i_prob); A.first = blk.dev<int32_t>(i_first); A.list = blk.dev<int32_t>(i_list);
    A.res = (orbm_pose_result*)m->pose.out.dp; A.flags = m->pose.out.dp + res_bytes;
    if (A.packed) A.packed = blk.dev<uint32_t>(i_edge[0]);
    else { A.feat = blk.dev<int32_t>(i_edge[0]); A.pos = blk.dev<float>(i_edge[1]); A.obs = blk.dev<float>(i_edge[2]); A.octave = blk.dev<int32_t>(i_edge[3]); }
    *flags_off = res_bytes;
    hipLaunchKernelGGL(k_pose_optimize, dim3((unsigned)list.size()), dim3(LM_T), 0, m->stream, A);
    MORB_HIP(hipGetLastError());
    return ORB_OK;
}

}  // namespace

extern "C" {

void orbm_pose_sincos(double x, double* s, double* c) { pose_sincos(x, s, c); }

int orbm_pose_optimize_host(const orbm_pose_problem* problems, int B, const int32_t* first, const int32_t* feat, const float* pos,
                            const float* obs, const int32_t* octave, int order, uint8_t* outlier_out, orbm_pose_result* results) {
    int rc = validate(problems, B, first, feat, pos, obs, octave, outlier_out, results);
    if (rc) return rc;
    if (order != ORBM_POSE_ORDER_INDEX && order != ORBM_POSE_ORDER_DEVICE) { morb::set_error("order = %d", order); return ORB_E_ARG; }
    const PoseEdges G = {feat, pos, obs, octave};
    for (int b = 0; b < B; ++b) pose_problem_host(problems[b], G, first[b], first[b + 1] - first[b], order, outlier_out + first[b], results[b]);
    return ORB_OK;
}

int orbm_pose_optimize(orbm_matcher* m, const orbm_pose_problem* problems, int B, const int32_t* first, const int32_t* feat,
                       const float* pos, const float* obs, const int32_t* octave, uint8_t* outlier_out, orbm_pose_result* results) {
    MORB_ARG(m != nullptr);
    int rc = validate(problems, B, first, feat, pos, obs, octave, outlier_out, results);
    if (rc) return rc;
    const int ne = first[B];
    const PoseEdges G = {feat, pos, obs, octave};
    return lm_csr_call(m, m->pose, B, first, ORBM_POSE_CAP, outlier_out, results, m->last_pose,
        [&](const std::vector<int32_t>& list, size_t* flags_off) -> int {
            PoseDev A;
            memset(&A, 0, sizeof(A));
            const void* src[4] = {feat, pos, obs, octave};
            const size_t len[4] = {(size_t)ne * 4, (size_t)ne * 12, (size_t)ne * 12, (size_t)ne * 4};
            return launch(m, problems, B, first, list, A, src, len, 4, flags_off);
        },
        [&](int b) { pose_problem_host(problems[b], G, first[b], first[b + 1] - first[b], ORBM_POSE_ORDER_DEVICE, outlier_out + first[b], results[b]); });
}

int orbm_pose_optimize_resident(orbm_matcher* m, const orbm_pose_problem* problem, const orbm_frame* cur, const orbm_points* pts,
                                const int32_t* point_of_feature, uint8_t* outlier_out, orbm_pose_result* result) {
    MORB_ARG(m != nullptr && problem != nullptr && cur != nullptr && pts != nullptr && result != nullptr);
    MORB_ARG(cur->owner == m && cur->b != nullptr);
    if (cur->counts_on_device) { morb::set_error("the frame's feature count is not on the host yet (orbf_step_end)"); return ORB_E_ARG; }
    if (problem->mode != ORBM_POSE_CAM0 && problem->mode != ORBM_POSE_ALL_CAMS) { morb::set_error("mode = %d", problem->mode); return ORB_E_ARG; }
    if (problem->n_levels < 1 || problem->n_levels > ORBM_MAX_LEVELS) { morb::set_error("n_levels = %d is outside 1..%d", problem->n_levels, (int)ORBM_MAX_LEVELS); return ORB_E_ARG; }
    const int N = cur->n_total;
    MORB_ARG(N == 0 || (point_of_feature && outlier_out));
    if (N > 65536) { morb::set_error("%d features: the resident form packs the feature index into 16 bits", N); return ORB_E_CAPACITY; }
    const orbm_point* d_rows = nullptr; const orbm_point* h_rows = nullptr;
    int count = 0, rc;
    if ((rc = morb::points_view(pts, m, &d_rows, &h_rows, &count))) return rc;
    const int limit = problem->mode == ORBM_POSE_CAM0 ? std::min(N, std::max(problem->n_cam0, 0)) : N;
    std::vector<uint32_t> packed;
    std::vector<int32_t> feat;
    for (int g = 0; g < limit; ++g) {
        const int row = point_of_feature[g];
        if (row < 0) continue;
        if (row >= count) { morb::set_error("point_of_feature[%d] = %d is beyond the %d rows written", g, row, count); return ORB_E_ARG; }
        packed.push_back((uint32_t)g << 16 | (uint32_t)row);
        feat.push_back(g);
    }
    const int n = (int)feat.size();
    for (int g = 0; g < N; ++g) outlier_out[g] = 0;
    MORB_HIP(hipSetDevice(m->device));
    const int32_t first[2] = {0, n};
    if (n > ORBM_POSE_CAP) {
        // the host routine on the frame's arrays brought back (rare: more edges than the device takes)
        std::vector<float> x((size_t)N), y((size_t)N), ur((size_t)N), pos((size_t)n * 3), obs((size_t)n * 3);
        std::vector<int32_t> oct((size_t)N), eoct((size_t)n);
        MORB_HIP(hipMemcpyAsync(x.data(), cur->b->d_x.p, (size_t)N * 4, hipMemcpyDeviceToHost, m->stream));
        MORB_HIP(hipMemcpyAsync(y.data(), cur->b->d_y.p, (size_t)N * 4, hipMemcpyDeviceToHost, m->stream));
        MORB_HIP(hipMemcpyAsync(ur.data(), cur->b->d_ur.p, (size_t)N * 4, hipMemcpyDeviceToHost, m->stream));
        MORB_HIP(hipMemcpyAsync(oct.data(), cur->b->d_oct.p, (size_t)N * 4, hipMemcpyDeviceToHost, m->stream));
        MORB_HIP(hipStreamSynchronize(m->stream));
        for (int e = 0; e < n; ++e) {
            const int g = feat[e];
            const orbm_point& row = h_rows[packed[e] & 0xffffu];
            for (int k = 0; k < 3; ++k) pos[3 * (size_t)e + k] = row.pos[k];
            obs[3 * (size_t)e] = x[g]; obs[3 * (size_t)e + 1] = y[g]; obs[3 * (size_t)e + 2] = ur[g];
            eoct[e] = std::min(std::max(oct[g], 0), ORBM_MAX_LEVELS - 1);
        }
        std::vector<uint8_t> flags((size_t)n);
        const PoseEdges G = {feat.data(), pos.data(), obs.data(), eoct.data()};
        pose_problem_host(*problem, G, 0, n, ORBM_POSE_ORDER_DEVICE, flags.data(), *result);
        for (int e = 0; e < n; ++e) outlier_out[feat[e]] = flags[e];
        m->last_pose[0] = 0; m->last_pose[1] = 1;
        return ORB_OK;
    }
    PoseDev A;
    memset(&A, 0, sizeof(A));
    static const uint32_t none = 0;
    A.packed = &none;   // (marks the resident form; launch() replaces it by the staged words)
    A.un_x = cur->b->d_x.p; A.un_y = cur->b->d_y.p; A.uright = cur->b->d_ur.p; A.f_octave = cur->b->d_oct.p; A.rows = d_rows;
    const std::vector<int32_t> list(1, 0);
    const void* src[1] = {packed.data()};
    const size_t len[1] = {(size_t)n * 4};
    size_t flags_off = 0;
    if ((rc = launch(m, problem, 1, first, list, A, src, len, 1, &flags_off))) return rc;
    MORB_HIP(hipStreamSynchronize(m->stream));
    *result = *(const orbm_pose_result*)m->pose.out.p;
    for (int e = 0; e < n; ++e) outlier_out[feat[e]] = m->pose.out.p[flags_off + e];
    m->last_pose[0] = 1; m->last_pose[1] = 0;
    return ORB_OK;
}

}  // extern "C"
