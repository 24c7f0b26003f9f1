// sim3opt.hip -- Sim3 refinement on the device (include/orbm.h, "Sim3 refinement"): Optimizer::OptimizeSim3_cam1 (reference
// src/Optimizer.cc:1984-2243) from the correspondence list on, with the parts of g2o it runs restated (Thirdparty/g2o/g2o/:
// types/sim3.h, types/types_seven_dof_expmap.h, core/base_binary_edge.hpp, core/robust_kernel_impl.cpp,
// core/optimization_algorithm_levenberg.cpp, core/sparse_optimizer.cpp, solvers/linear_solver_dense.h) and the Eigen operators those call.
//   eigen_*, sim3_*, g2o_huber   the Eigen operators, g2o::Sim3 and the Huber kernel: g2o_dev.h (UNPINNED).
//   sim3opt_edge      one edge of either type: computeError, chi2, the NUMERIC linearizeOplus of BaseBinaryEdge (neither edge type
//                     has an analytic one) and the robust constructQuadraticForm, ONE statement sequence for kernel and host routine.
//   sim3opt_records   the 30 transforms a pass reads: the estimate, Sim3(+-1e-9 e_d) * estimate for d = 0..6, and the inverse of each.
//                     None depends on the edge, so the controller forms them once per pass.
//   sim3opt_step      the controller: a resumable state machine over a Sim3Ctl record.  The Levenberg bookkeeping and the 7x7 solve are
//                     lm_dev.h's lm_step (ONE definition, pose.hip runs it too); the exp map, the records and the two optimisations are
//                     here.  The host routine calls it between its passes, lane 0 calls it on the record in LDS: the same statements.
//   k_sim3_optimize   one workgroup of 256 lanes per problem, resident for the whole call.  Per pass every lane evaluates both edges
//                     of its correspondences (lane l owns l, l + 256, ... in ascending order) and sums 28 + 7 + 1 + 1 doubles;
//                     lm_dev.h's summation tree (butterfly in each wave, the four waves in wave order) gives lane 0 the pass's sums,
//                     lm_pass_host walks the same tree.  Two barriers per pass, no atomics, no order that depends on arrival.
// No libm function runs in the kernel: + - * / sqrt in double, conversions, pose_sincos and pose_exp (sincos_dev.h).
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

// the sums of a pass (lm_dev.h): H upper triangle (28, row-major i <= j), b (7), robust chi2, count of failed correspondences
constexpr int S3O_NSUM = LmState<7>::NSUM, S3O_CHI = LmState<7>::CHI, S3O_BAD = LmState<7>::COUNT;
constexpr int S3O_NREC = 30;         // 0: the estimate; 1 + 2d, 2 + 2d: Sim3(+delta e_d) * estimate, Sim3(-delta e_d) * estimate; 15 + k: inverse of k

// A compiler-only fence for the kernel (no instruction): the 30 records are loop invariant, and hoisted out of the loop over a lane's
// correspondences they alone would need 480 registers.  Behind a fence each is read from LDS where it is used.
#ifdef __HIP_DEVICE_COMPILE__
#define S3O_FENCE() asm volatile("" ::: "memory")
#else
#define S3O_FENCE() do {} while (0)
#endif

struct Sim3Cam {                         // per problem: the members of the vertex and of the robust kernels
    double K1[4], K2[4];                 // _focal_length1, _principle_point1 / ...2 as fx, fy, cx, cy
    double delta, dsqr;                  // RobustKernelHuber::_delta (the float deltaHuber as a double) and dsqr (a FLOAT member)
    double th2;                          // (double)th2 of `chi2() > th2`
};
struct Sim3Pair { float X1[3], X2[3], obs1[2], obs2[2], w1, w2; };   // w: invSigmaSquare1 / 2

// ---- one edge ---------------------------------------------------------------------------------------------------------------------------
// computeError of both edge types: obs - cam_map(project(T.map(X))).  EdgeSim3ProjectXYZ: T = the estimate, X = the point of keyframe 2,
// camera 1; EdgeInverseSim3ProjectXYZ: T = estimate().inverse(), X = the point of keyframe 1, camera 2.
__host__ __device__ inline void sim3opt_error(const Sim3Quat& T, const float* X, const float* obs, const double* K, double* e) {
    const double Xd[3] = {(double)X[0], (double)X[1], (double)X[2]};
    double p[3];
    sim3_map(T, Xd, p);
    const double proj0 = p[0] / p[2], proj1 = p[1] / p[2];                 // project
    e[0] = (double)obs[0] - (proj0 * K[0] + K[2]);
    e[1] = (double)obs[1] - (proj1 * K[1] + K[3]);
}
__host__ __device__ inline double sim3opt_chi2(const double* e, double w) { return e[0] * (w * e[0]) + e[1] * (w * e[1]); }

// One ACTIVE edge's share of a pass.  type 0: EdgeSim3ProjectXYZ (records 0 .. 14), 1: EdgeInverseSim3ProjectXYZ (15 .. 29).
// computeActiveErrors + activeRobustChi2; with `system` also BaseBinaryEdge::linearizeOplus (core/base_binary_edge.hpp:131-205: per
// dimension the error at +delta minus the error at -delta, times 1/(2 delta); the point vertex is fixed) and the robust branch of
// constructQuadraticForm (:91-113) in pose_accumulate's convention: the edge's own 7-vector and 7x7 are formed first (rows of J in
// order) and then added.  UNPINNED: Eigen's evaluation order inside the two products.
__host__ __device__ inline void sim3opt_edge(const Sim3Cam& C, const Sim3Quat* rec, const Sim3Pair& P, int type, bool system, double* acc) {
    const float* X = type ? P.X1 : P.X2;
    const float* obs = type ? P.obs2 : P.obs1;
    const double* K = type ? C.K2 : C.K1;
    const double w = (double)(type ? P.w2 : P.w1);
    const Sim3Quat* T = rec + (type ? 15 : 0);
    double e[2];
    S3O_FENCE();
    sim3opt_error(T[0], X, obs, K, e);
    const double chi2 = sim3opt_chi2(e, w);
    double rho0, rho1;
    g2o_huber(chi2, C.delta, C.dsqr, &rho0, &rho1);
    acc[S3O_CHI] += rho0;
    if (!system) return;
    const double delta = 1e-9;
    const double scalar = 1.0 / (2 * delta);
    double J[2][7];
#pragma unroll
    for (int d = 0; d < 7; ++d) {
        double ep[2], em[2];
        S3O_FENCE();
        sim3opt_error(T[1 + 2 * d], X, obs, K, ep);
        sim3opt_error(T[2 + 2 * d], X, obs, K, em);
        J[0][d] = scalar * (ep[0] - em[0]);
        J[1][d] = scalar * (ep[1] - em[1]);
    }
    const double rw = rho1 * w;
    const double we[2] = {w * e[0], w * e[1]};
    int k = 0;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
#pragma unroll
        for (int j = i; j < 7; ++j, ++k) acc[k] += (J[0][i] * rw) * J[0][j] + (J[1][i] * rw) * J[1][j];
        acc[28 + i] -= rho1 * (J[0][i] * we[0] + J[1][i] * we[1]);
    }
}
// both edges of a correspondence, e12 before e21 (the order of addEdge)
__host__ __device__ inline void sim3opt_accumulate(const Sim3Cam& C, const Sim3Quat* rec, const Sim3Pair& P, bool system, double* acc) {
    sim3opt_edge(C, rec, P, 0, system, acc);
    sim3opt_edge(C, rec, P, 1, system, acc);
}
// `e12->chi2()>th2 || e21->chi2()>th2` (:2189, :2228): _error is what the last computeActiveErrors left, the estimate of the LAST pass
// (records 0 and 15 as they stand) -- the rejected trial when the optimisation ended on one; double against (double)th2.
__host__ __device__ inline bool sim3opt_classify(const Sim3Cam& C, const Sim3Quat* rec, const Sim3Pair& P) {
    double e[2];
    sim3opt_error(rec[0], P.X2, P.obs1, C.K1, e);
    const double chi12 = sim3opt_chi2(e, (double)P.w1);
    sim3opt_error(rec[15], P.X1, P.obs2, C.K2, e);
    const double chi21 = sim3opt_chi2(e, (double)P.w2);
    return chi12 > C.th2 || chi21 > C.th2;
}

// ---- the controller ---------------------------------------------------------------------------------------------------------------------
// (Its functions are inlined by force: a call out of the kernel would save registers in scratch memory, and the kernel uses none.)
struct Sim3Ctl : LmState<7> {
    static constexpr bool LM_TRY_INLINE = true;
    int n, stage, n_bad, fix_scale;
    Sim3Quat start, est;                     // g2oS12 as it came; the vertex's estimate
    Sim3Quat rec[S3O_NREC];                  // what the next / the last pass reads; rec[0] is the estimate of that pass
    orbm_sim3opt_result res;
    // what lm_step leaves to the port (defined below, behind sim3opt_records)
    __host__ __device__ void lm_trial();
    __host__ __device__ __forceinline__ void lm_accept() { est = rec[0]; }
    __host__ __device__ void lm_linearise();
};

// rec[0] is set: its inverse, and for a FULL pass the 14 perturbed estimates of the numeric Jacobian and theirs.  oplusImpl:
// `if (_fix_scale) update[6] = 0; setEstimate(Sim3(update) * estimate())`.
__host__ __device__ __forceinline__ void sim3opt_records(Sim3Ctl& S, bool full) {
    sim3_inverse(S.rec[0], S.rec[15]);
    if (!full) return;
    const double delta = 1e-9;
    for (int d = 0; d < 7; ++d)
        for (int sg = 0; sg < 2; ++sg) {
            for (int k = 0; k < 7; ++k) S.temp[k] = 0.0;
            S.temp[d] = sg ? -delta : delta;
            if (S.fix_scale) S.temp[6] = 0;
            Sim3Quat u;
            sim3_exp(S.temp, S.order, u);
            sim3_mul(u, S.rec[0], S.rec[1 + 2 * d + sg]);
            sim3_inverse(S.rec[1 + 2 * d + sg], S.rec[16 + 2 * d + sg]);
        }
}
__host__ __device__ __forceinline__ void Sim3Ctl::lm_linearise() { rec[0] = est; sim3opt_records(*this, true); cmd = LM_CMD_FULL; }
__host__ __device__ __forceinline__ void Sim3Ctl::lm_trial() {
    if (fix_scale) x[6] = 0;                 // oplusImpl writes through the solver's x: computeScale reads the 0
    Sim3Quat d;
    sim3_exp(x, order, d);
    sim3_mul(d, est, rec[0]);
    sim3opt_records(*this, false);
}

__host__ __device__ __forceinline__ void sim3opt_write(Sim3Ctl& S, const Sim3Quat& T) {
    for (int k = 0; k < 4; ++k) S.res.q[k] = x86_nan(T.q[k]);
    for (int k = 0; k < 3; ++k) S.res.t[k] = x86_nan(T.t[k]);
    S.res.s = x86_nan(T.s);
}
// initializeOptimization() + optimize(max_iter): the estimate stays, lambda is initialised again at iteration 0
__host__ __device__ __forceinline__ void sim3opt_begin_optimisation(Sim3Ctl& S, int n_active, int max_iter) {
    S.iter = 0; S.max_iter = max_iter;
    if (n_active <= 0) { S.cmd = LM_CMD_CLASSIFY; return; }   // no active edge, no active vertex: optimize() returns at once
    S.res.optimisations = S.stage + 1;
    S.lm_linearise();
}
__host__ __device__ __forceinline__ void sim3opt_begin(Sim3Ctl& S, const orbm_sim3opt_problem& P, int n, int order) {
    S.order = order; S.n = n; S.stage = 0; S.n_bad = 0; S.ok2 = 1; S.fix_scale = P.fix_scale ? 1 : 0;
    S.lambda = 0; S.ni = 2; S.current_chi = 0; S.ini_chi = 0; S.n_bad_steps = 0; S.qmax = 0;
    for (int i = 0; i < 7; ++i) S.x[i] = 0;
    double R[9], t[3];
    for (int i = 0; i < 9; ++i) R[i] = (double)P.R[i];
    for (int i = 0; i < 3; ++i) t[i] = (double)P.t[i];
    sim3_from_matrix(R, t, (double)P.s, S.start);
    S.est = S.start; S.rec[0] = S.start;
    memset(&S.res, 0, sizeof(S.res));
    S.res.n_correspondences = n;
    sim3opt_begin_optimisation(S, n, 5);
}
// Called after every pass with the pass's sums.
__host__ __device__ __forceinline__ void sim3opt_step(Sim3Ctl& S, const double* sum) {
    orbm_pose_round& R = S.res.round[S.stage];
    if (S.cmd != LM_CMD_CLASSIFY) { lm_step(S, sum, R); return; }   // a FULL or a CHI pass: one step of the Levenberg loop
    // LM_CMD_CLASSIFY
    if (S.stage == 0) {                      // :2178-2211
        S.n_bad = (int)sum[S3O_BAD];
        S.res.n_bad = S.n_bad;
        S.res.n_more_iterations = S.n_bad > 0 ? 10 : 5;
        if (S.n - S.n_bad < 10) {            // `return 0`: g2oS12 is not touched, the removals stay
            S.res.n_inliers = 0; S.res.written = 0;
            sim3opt_write(S, S.start);
            S.cmd = LM_CMD_DONE;
            return;
        }
        S.stage = 1;
        sim3opt_begin_optimisation(S, S.n - S.n_bad, S.res.n_more_iterations);
        return;
    }
    S.res.n_inliers = S.n - S.n_bad - (int)sum[S3O_BAD];   // nIn (:2218-2235)
    S.res.written = 1;
    sim3opt_write(S, S.est);
    S.cmd = LM_CMD_DONE;
}

// the constants of a problem (:2034-2041, :2059, :2136-2138)
__host__ __device__ inline void sim3opt_camera(const orbm_sim3opt_problem& P, Sim3Cam& C) {
    for (int k = 0; k < 4; ++k) { C.K1[k] = (double)P.K1[k]; C.K2[k] = (double)P.K2[k]; }
    // `const float deltaHuber = sqrt(th2)`: the float square root (the double one rounded to float is the same number);
    // rk->setDelta(deltaHuber): _delta = the float as a double, dsqr = (float)(delta*delta)
    const float delta_huber = (float)sqrt((double)P.th2);
    C.delta = (double)delta_huber;
    C.dsqr = (double)(float)(C.delta * C.delta);
    C.th2 = (double)P.th2;
}

// one pass's share of one correspondence; flag: 0 active, 1 removed after the first optimisation, 2 failed the final test
__host__ __device__ inline void sim3opt_pass_pair(const Sim3Cam& C, const Sim3Ctl& S, int cmd, const Sim3Pair& P, uint8_t* flag, double* acc) {
    if (*flag) return;
    if (cmd == LM_CMD_CLASSIFY) {
        if (sim3opt_classify(C, S.rec, P)) { *flag = S.stage == 0 ? 1 : 2; acc[S3O_BAD] += 1.0; }
    } else {
        sim3opt_accumulate(C, S.rec, P, cmd == LM_CMD_FULL, acc);
    }
}

// ---- the kernel -------------------------------------------------------------------------------------------------------------------------
struct Sim3OptDev {
    const orbm_sim3opt_problem* prob;  // per problem
    const int32_t* first;              // CSR, per problem + 1
    const int32_t* list;               // the problems this launch works on (blockIdx.x -> problem)
    const float* x3dc1; const float* x3dc2; const float* obs1; const float* obs2; const int32_t* octave1; const int32_t* octave2;
    uint8_t* flags;                    // per correspondence, mapped pinned
    orbm_sim3opt_result* res;          // per problem, mapped pinned
};

__device__ __forceinline__ Sim3Pair sim3opt_load(const Sim3OptDev& A, const orbm_sim3opt_problem& P, int i) {
    Sim3Pair E;
    for (int k = 0; k < 3; ++k) { E.X1[k] = A.x3dc1[3 * (size_t)i + k]; E.X2[k] = A.x3dc2[3 * (size_t)i + k]; }
    for (int k = 0; k < 2; ++k) { E.obs1[k] = A.obs1[2 * (size_t)i + k]; E.obs2[k] = A.obs2[2 * (size_t)i + k]; }
    // (validated on the host; the tables are never indexed beyond their ends)
    E.w1 = P.inv_level_sigma2_1[min(max(A.octave1[i], 0), ORBM_MAX_LEVELS - 1)];
    E.w2 = P.inv_level_sigma2_2[min(max(A.octave2[i], 0), ORBM_MAX_LEVELS - 1)];
    return E;
}

__global__ __launch_bounds__(LM_T) void k_sim3_optimize(Sim3OptDev A) {
    __shared__ Sim3Ctl S;
    __shared__ Sim3Cam C;
    __shared__ double s_part[LM_T / 64][S3O_NSUM];
    __shared__ uint8_t s_flag[ORBM_SIM3OPT_CAP];
    const int tid = threadIdx.x;
    const int pb = A.list[blockIdx.x];
    const orbm_sim3opt_problem& P = A.prob[pb];
    const int e0 = A.first[pb];
    const int n = min(A.first[pb + 1] - e0, (int)ORBM_SIM3OPT_CAP);   // (a longer problem never reaches the device)
    if (tid == 0) { sim3opt_camera(P, C); sim3opt_begin(S, P, n, ORBM_POSE_ORDER_DEVICE); }
    for (int e = tid; e < n; e += LM_T) s_flag[e] = 0;
    for (;;) {
        __syncthreads();                                   // the controller's record is visible
        const int cmd = S.cmd;
        if (cmd == LM_CMD_DONE) break;
        double acc[S3O_NSUM];
#pragma unroll
        for (int k = 0; k < S3O_NSUM; ++k) acc[k] = 0.0;
        // this lane's correspondences in ascending order; their constants stream from the staged arrays
        for (int e = tid; e < n; e += LM_T) {
            if (s_flag[e]) continue;
            const Sim3Pair E = sim3opt_load(A, P, e0 + e);
            sim3opt_pass_pair(C, S, cmd, E, &s_flag[e], acc);
        }
        lm_wave_sums(acc, cmd == LM_CMD_FULL ? 0 : S3O_CHI, s_part, tid);
        __syncthreads();                                   // the four waves' sums are visible, every lane is done with the record
        if (tid == 0) {
            double sum[S3O_NSUM];
            lm_add_waves(s_part, sum);
            sim3opt_step(S, sum);
        }
    }
    for (int e = tid; e < n; e += LM_T) A.flags[e0 + e] = s_flag[e];
    if (tid == 0) A.res[pb] = S.res;
}

// ---- host routine -----------------------------------------------------------------------------------------------------------------------
struct Sim3OptPairs { const float* x3dc1; const float* x3dc2; const float* obs1; const float* obs2; const int32_t* octave1; const int32_t* octave2; };

Sim3Pair host_pair(const orbm_sim3opt_problem& P, const Sim3OptPairs& G, int i) {
    Sim3Pair E;
    for (int k = 0; k < 3; ++k) { E.X1[k] = G.x3dc1[3 * (size_t)i + k]; E.X2[k] = G.x3dc2[3 * (size_t)i + k]; }
    for (int k = 0; k < 2; ++k) { E.obs1[k] = G.obs1[2 * (size_t)i + k]; E.obs2[k] = G.obs2[2 * (size_t)i + k]; }
    E.w1 = P.inv_level_sigma2_1[G.octave1[i]];
    E.w2 = P.inv_level_sigma2_2[G.octave2[i]];
    return E;
}

// one problem; correspondences e0 .. e0 + n - 1 of G, flags[0 .. n-1]
void sim3opt_problem_host(const orbm_sim3opt_problem& P, const Sim3OptPairs& G, int e0, int n, int order, uint8_t* flags, orbm_sim3opt_result& res) {
    Sim3Cam C;
    Sim3Ctl S;
    sim3opt_camera(P, C);
    sim3opt_begin(S, P, n, order);
    for (int e = 0; e < n; ++e) flags[e] = 0;
    std::vector<Sim3Pair> E((size_t)n);
    for (int e = 0; e < n; ++e) E[e] = host_pair(P, G, e0 + e);
    std::vector<double> part;
    while (S.cmd != LM_CMD_DONE) {
        double sum[S3O_NSUM];
        const int cmd = S.cmd;
        lm_pass_host<S3O_NSUM>(order, n, part, sum, [&](int e, double* acc) { sim3opt_pass_pair(C, S, cmd, E[e], &flags[e], acc); });
        sim3opt_step(S, sum);
    }
    res = S.res;
}

int validate(const orbm_sim3opt_problem* problems, int B, const int32_t* first, const Sim3OptPairs& G, const uint8_t* flag_out,
             const orbm_sim3opt_result* results) {
    MORB_ARG(problems && first && results);
    if (const int rc = morb::validate_csr(B, ORBM_SIM3OPT_MAX_BATCH, first)) return rc;
    for (int b = 0; b < B; ++b) {
        const orbm_sim3opt_problem& P = problems[b];
        if (P.n_levels1 < 1 || P.n_levels1 > ORBM_MAX_LEVELS || P.n_levels2 < 1 || P.n_levels2 > ORBM_MAX_LEVELS) {
            morb::set_error("problem %d: n_levels = %d, %d are outside 1..%d", b, P.n_levels1, P.n_levels2, (int)ORBM_MAX_LEVELS);
            return ORB_E_ARG;
        }
    }
    const int ne = first[B];
    if (ne > 0 && !(G.x3dc1 && G.x3dc2 && G.obs1 && G.obs2 && G.octave1 && G.octave2 && flag_out)) { morb::set_error("a correspondence array is NULL"); return ORB_E_ARG; }
    for (int b = 0; b < B; ++b)
        for (int e = first[b]; e < first[b + 1]; ++e)
            if (G.octave1[e] < 0 || G.octave1[e] >= problems[b].n_levels1 || G.octave2[e] < 0 || G.octave2[e] >= problems[b].n_levels2) {
                morb::set_error("correspondence %d: octaves %d, %d are outside the %d, %d levels of problem %d", e, G.octave1[e], G.octave2[e],
                                problems[b].n_levels1, problems[b].n_levels2, b);
                return ORB_E_ARG;
            }
    return ORB_OK;
}

}  // namespace

extern "C" {

double orbm_sim3opt_exp(double x) { return pose_exp(x); }

int orbm_sim3opt_expmap(const double* update7, int order, double* out8) {
    MORB_ARG(update7 != nullptr && out8 != nullptr);
    Sim3Quat T;
    const int branch = sim3_exp(update7, order, T);
    for (int k = 0; k < 4; ++k) out8[k] = T.q[k];
    for (int k = 0; k < 3; ++k) out8[4 + k] = T.t[k];
    out8[7] = T.s;
    return branch;
}

int orbm_sim3opt_ldlt7(double* A49, const double* b7, double* x7) {
    MORB_ARG(A49 != nullptr && b7 != nullptr && x7 != nullptr);
    double temp[7];
    int transp[7];
    return eigen_ldlt_solve<7>(A49, b7, x7, temp, transp) ? 1 : 0;
}

int orbm_sim3_optimize_host(const orbm_sim3opt_problem* problems, int B, const int32_t* first, const float* x3dc1, const float* x3dc2,
                            const float* obs1, const float* obs2, const int32_t* octave1, const int32_t* octave2, int order,
                            uint8_t* flag_out, orbm_sim3opt_result* results) {
    const Sim3OptPairs G = {x3dc1, x3dc2, obs1, obs2, octave1, octave2};
    int rc = validate(problems, B, first, G, flag_out, results);
    if (rc) return rc;
    if (order != ORBM_POSE_ORDER_INDEX && order != ORBM_POSE_ORDER_DEVICE) { morb::set_error("order = %d", order); return ORB_E_ARG; }
    for (int b = 0; b < B; ++b) sim3opt_problem_host(problems[b], G, first[b], first[b + 1] - first[b], order, flag_out + first[b], results[b]);
    return ORB_OK;
}

int orbm_sim3_optimize(orbm_matcher* m, const orbm_sim3opt_problem* problems, int B, const int32_t* first, const float* x3dc1,
                       const float* x3dc2, const float* obs1, const float* obs2, const int32_t* octave1, const int32_t* octave2,
                       uint8_t* flag_out, orbm_sim3opt_result* results) {
    MORB_ARG(m != nullptr);
    const Sim3OptPairs G = {x3dc1, x3dc2, obs1, obs2, octave1, octave2};
    int rc = validate(problems, B, first, G, flag_out, results);
    if (rc) return rc;
    const int ne = first[B];
    return lm_csr_call(m, m->sim3opt, B, first, ORBM_SIM3OPT_CAP, flag_out, results, m->last_sim3opt,
        [&](const std::vector<int32_t>& list, size_t* flags_off) -> int {
            morb::StagePack pk;
            const int i_prob = pk.add(problems, (size_t)B * sizeof(orbm_sim3opt_problem)), i_first = pk.add(first, (size_t)(B + 1) * 4),
                      i_list = pk.add(list.data(), list.size() * 4);
            const int i_x1 = pk.add(x3dc1, (size_t)ne * 12), i_x2 = pk.add(x3dc2, (size_t)ne * 12), i_o1 = pk.add(obs1, (size_t)ne * 8),
                      i_o2 = pk.add(obs2, (size_t)ne * 8), i_c1 = pk.add(octave1, (size_t)ne * 4), i_c2 = pk.add(octave2, (size_t)ne * 4);
            const size_t res_bytes = morb::align16((size_t)B * sizeof(orbm_sim3opt_result));
            int rc;
            const morb::StagePack::Block blk = pk.open(m->sim3opt.stage, &rc);
            if (rc || (rc = m->sim3opt.out.reserve(res_bytes + (size_t)std::max(ne, 1)))) return rc;
            blk.publish();
            Sim3OptDev A;
            A.prob = blk.dev<orbm_sim3opt_problem>(i_prob); A.first = blk.dev<int32_t>(i_first); A.list = blk.dev<int32_t>(i_list);
            A.x3dc1 = blk.dev<float>(i_x1); A.x3dc2 = blk.dev<float>(i_x2); A.obs1 = blk.dev<float>(i_o1); A.obs2 = blk.dev<float>(i_o2);
            A.octave1 = blk.dev<int32_t>(i_c1); A.octave2 = blk.dev<int32_t>(i_c2);
            A.res = (orbm_sim3opt_result*)m->sim3opt.out.dp; A.flags = m->sim3opt.out.dp + res_bytes;
            *flags_off = res_bytes;
            hipLaunchKernelGGL(k_sim3_optimize, dim3((unsigned)list.size()), dim3(LM_T), 0, m->stream, A);
            MORB_HIP(hipGetLastError());
            return ORB_OK;
        },
        [&](int b) { sim3opt_problem_host(problems[b], G, first[b], first[b + 1] - first[b], ORBM_POSE_ORDER_DEVICE, flag_out + first[b], results[b]); });
}

}  // extern "C"
