// lm_dev.h -- what the Levenberg ports share (pose.hip: 6 unknowns, sim3opt.hip: 7, lba.hip: a vector of them), ONE definition each, for
// the kernels and the host routines.  Restated from Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp, core/sparse_optimizer.cpp
// (the loop of optimize).
//   lm_rule_full, lm_rule_trial, lm_rule_iter_end   the Levenberg rules themselves -- lambda's start, its scaling after a trial, the
//                         verdict on a trial, the end of an iteration -- over any record that has the members they touch.  Every port
//                         runs these three; its driver decides what lies between them.
//   LmState<N>, lm_step   the driver for a fixed-size vertex: the controller between two passes over the edges as far as it does not
//                         depend on the vertex (the sums into H and b, the dense solve, computeScale).  The port's record
//                         derives from LmState<N> and supplies the points where the ports differ inside an optimisation: lm_trial()
//                         (oplusImpl: exp(x) * estimate into what the next pass reads), lm_accept() (discardTop), lm_linearise() (what a
//                         FULL pass reads, at the estimate; sets cmd = LM_CMD_FULL) and the constant LM_TRY_INLINE (lm_next_trial).
//                         (The local BA's driver is lba_dev.h's lba_ctl_*: the same three calls, cut where g2o polls the stop flag.)
//   lm_wave_sum, lm_wave_sums, lm_add_waves   the kernel's summation tree: xor butterfly (1 .. 32) in each wave, the four waves in wave
//                         order.  lm_pass_host: the same tree leaf for leaf on the host (DEVICE order) or the plain loop (INDEX order).
//   lm_csr_call           the skeleton of a batched call over a CSR of problems (its checks: morb::validate_csr, stage_pack.h).
// The sums of a pass: N (N + 1) / 2 entries of H (upper triangle, row-major, i <= j), N of b, the robust chi2, a count.  Both kernels
// fill the register file (256 VGPRs, no scratch): the device functions are inlined by force, the solver's storage stays in the record.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "orb_common.h"
#include "matcher_internal.h"
#include "cv_dev.h"   // x86_nan
#include "g2o_dev.h"

constexpr int LM_T = 256;            // lanes of the workgroup = leaves of the summation tree
enum { LM_CMD_FULL = 0, LM_CMD_CHI = 1, LM_CMD_CLASSIFY = 2, LM_CMD_DONE = 3 };   // what the next pass over the edges is for

template <int N_>
struct LmState {
    enum { N = N_, NH = N_ * (N_ + 1) / 2, CHI = NH + N_, COUNT = CHI + 1, NSUM = CHI + 2 };   // the layout of a pass's sums
    int cmd, order, iter, max_iter, qmax, n_bad_steps, ok2;
    double H[NH], b[N], x[N], lambda, ni, current_chi, ini_chi;
    double A[N * N], temp[N]; int transp[N];   // the solver's working storage
};

// one trial of the Levenberg loop up to its pass (:103-121): H + lambda on the diagonal, the dense solve, update(x)
template <class Ctl>
__host__ __device__ inline void lm_try(Ctl& S) {
    constexpr int N = Ctl::N;
    int k = 0;
    for (int i = 0; i < N; ++i)
        for (int j = i; j < N; ++j, ++k) { S.A[N * i + j] = S.H[k]; S.A[N * j + i] = S.H[k]; }
    for (int i = 0; i < N; ++i) S.A[(N + 1) * i] += S.lambda;
    S.ok2 = eigen_ldlt_solve<N>(S.A, S.b, S.x, S.temp, S.transp) ? 1 : 0;
    S.lm_trial();
    S.cmd = LM_CMD_CHI;
}
// lm_step's two calls of it, as each kernel had them before the ports shared it: k_sim3_optimize inlines it, k_pose_optimize calls it
// (the measurements behind that: profiles/r17/notes_lm_refactor.md).
template <class Ctl>
__host__ __device__ __forceinline__ void lm_next_trial(Ctl& S) {
    if constexpr (Ctl::LM_TRY_INLINE) { [[clang::always_inline]] lm_try(S); } else { [[clang::noinline]] lm_try(S); }
}

// ---- the Levenberg rules of g2o ------------------------------------------------------------------------------------------------------------
// optimization_algorithm_levenberg.cpp:61-164 and the bookkeeping of SparseOptimizer::optimize's loop (core/sparse_optimizer.cpp:376-414),
// ONE definition for every port, over any record with the members order, iter, max_iter, qmax, n_bad_steps, ok2, lambda, ni,
// current_chi, ini_chi (LmState<N>, lba_dev.h's LbaCtl): templates and no base struct, so that no record's layout depends on them
// (profiles/r17/notes_lm_refactor.md).  What differs between the ports stays with their drivers: the sums, the solve, computeScale's
// sum over x, what accepting a trial means, and where g2o polls the stop flag.
// after computeActiveErrors + buildSystem at the estimate (:75-101); max_diagonal: computeLambdaInit's maximum, read at iteration 0
template <class S_>
__host__ __device__ __forceinline__ void lm_rule_full(S_& S, double chi, double max_diagonal) {
    S.current_chi = chi; S.ini_chi = chi;
    if (S.iter == 0) { S.lambda = 1e-5 * max_diagonal; S.ni = 2; S.n_bad_steps = 0; }   // computeLambdaInit: tau * the largest |diagonal|
    S.qmax = 0;
}
// after a trial's computeActiveErrors (:123-149); scale: computeScale() over all of x.  The caller does discardTop when accepted (pop
// otherwise: its estimate stays) and goes on with the next trial while `rho < 0 && qmax < 10`.
struct LmTrial { double rho; bool accepted; };
template <class S_>
__host__ __device__ __forceinline__ LmTrial lm_rule_trial(S_& S, double temp_chi, double scale, orbm_pose_round& R) {
    if (!S.ok2) temp_chi = DBL_MAX;          // the solve failed: the trial counts as rejected whatever its pass summed
    double rho = S.current_chi - temp_chi;
    scale += 1e-3;
    rho /= scale;
    S.qmax++;                                // (counted here and not behind the verdict, where g2o counts: the verdict reads neither,
    R.trials++;                              //  and so the caller's discardTop joins the accepting branch: profiles/r21/notes_lba_shared.md)
    const bool accepted = rho > 0 && fabs(temp_chi) <= DBL_MAX;
    if (accepted) {
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
    } else {
        S.lambda *= S.ni;
        S.ni *= 2;
    }
    return {rho, accepted};
}
// the trial loop is over: solve()'s result, then optimize()'s loop; rho == 0 terminates.  Returns terminate (`result != OK`); the
// caller's loop also ends at iter == max_iter.
template <class S_>
__host__ __device__ __forceinline__ bool lm_rule_iter_end(S_& S, double rho, orbm_pose_round& R) {
    R.iterations++;
    bool terminate = S.qmax == 10 || rho == 0;
    if (!terminate) {
        if ((S.ini_chi - S.current_chi) * 1e3 < S.ini_chi) S.n_bad_steps++; else S.n_bad_steps = 0;
        if (S.n_bad_steps >= 3) terminate = true;
    }
    S.iter++;
    return terminate;
}

// The driver of the rules for a fixed-size vertex.  Called after a FULL or a CHI pass with the pass's sums; R: where this optimisation's
// counters go.  Leaves cmd = LM_CMD_CHI (a trial), LM_CMD_FULL (the next iteration) or LM_CMD_CLASSIFY (optimize() returned).  lambda is
// initialised at iteration 0 of EVERY optimisation; after a rejected last trial the estimate is the last accepted one while the pass's
// transform stays the rejected one.
template <class Ctl>
__host__ __device__ __forceinline__ void lm_step(Ctl& S, const double* sum, orbm_pose_round& R) {
    constexpr int N = Ctl::N;
    if (S.cmd == LM_CMD_FULL) {              // the errors, the robust chi2 and the system at the estimate
        for (int k = 0; k < Ctl::NH; ++k) S.H[k] = sum[k];
        for (int k = 0; k < N; ++k) S.b[k] = sum[Ctl::NH + k];
        double max_diagonal = 0.;
        if (S.iter == 0) {
            int d = 0;
            for (int j = 0; j < N; ++j) { const double v = fabs(S.H[d]); if (v > max_diagonal) max_diagonal = v; d += N - j; }
        }
        lm_rule_full(S, sum[Ctl::CHI], max_diagonal);
        lm_next_trial(S);
        return;
    }
    // LM_CMD_CHI
    double scale = 0.;
    for (int j = 0; j < N; ++j) scale += S.x[j] * (S.lambda * S.x[j] + S.b[j]);
    const LmTrial t = lm_rule_trial(S, sum[Ctl::CHI], scale, R);
    if (t.accepted) S.lm_accept();           // discardTop
    if (t.rho < 0 && S.qmax < 10) { lm_next_trial(S); return; }
    if (lm_rule_iter_end(S, t.rho, R) || S.iter == S.max_iter) {
        R.chi2 = x86_nan(S.current_chi); R.lambda = x86_nan(S.lambda);
        S.cmd = LM_CMD_CLASSIFY;
    } else {
        S.lm_linearise();
    }
}

// ---- the summation tree of a pass -------------------------------------------------------------------------------------------------------
// one sum across the wave: xor butterfly, offsets 1, 2, 4, 8, 16, 32 (every lane ends with the same bits: a + b == b + a)
__device__ __forceinline__ double lm_wave_sum(double v) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}
// Every lane holds its own sums in acc: the butterfly over each, then lane 0 of each wave leaves the wave's sums in s_part.  live: the
// first sum this pass added to (0 in a FULL pass, CHI otherwise); the sums before it are skipped: they are exact zeros with or without
// the butterfly, and nobody reads them.
template <int NSUM>
__device__ __forceinline__ void lm_wave_sums(double (&acc)[NSUM], int live, double (&s_part)[LM_T / 64][NSUM], int tid) {
#pragma unroll
    for (int k = 0; k < NSUM; ++k) {
        if (k < live) continue;
        acc[k] = lm_wave_sum(acc[k]);
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < NSUM; ++k) s_part[tid >> 6][k] = acc[k];
    }
}
// after the caller's barrier, lane 0 of the workgroup: the four waves in wave order
template <int NSUM>
__device__ __forceinline__ void lm_add_waves(const double (&s_part)[LM_T / 64][NSUM], double (&sum)[NSUM]) {
#pragma unroll
    for (int k = 0; k < NSUM; ++k) sum[k] = ((s_part[0][k] + s_part[1][k]) + s_part[2][k]) + s_part[3][k];
}

// the same tree on the host over part[LM_T][NSUM], leaf l = what lane l summed: the butterfly as far as lane 0 of each wave sees it
template <int NSUM>
inline void lm_tree_host(double* part, double* sum) {
    for (int off = 1; off < 64; off <<= 1)
        for (int l = 0; l < LM_T; ++l)
            if (!(l & off) && !(l & (off - 1)))
                for (int k = 0; k < NSUM; ++k) part[(size_t)l * NSUM + k] = part[(size_t)l * NSUM + k] + part[(size_t)(l | off) * NSUM + k];
    for (int k = 0; k < NSUM; ++k)
        sum[k] = ((part[k] + part[(size_t)64 * NSUM + k]) + part[(size_t)128 * NSUM + k]) + part[(size_t)192 * NSUM + k];
}
// One pass of the host routine over edges 0 .. n-1.  edge(e, acc) adds edge e's share into acc[NSUM].  ORBM_POSE_ORDER_INDEX: one
// accumulator, the edges in index order; otherwise the kernel's tree: lane l owns l, l + 256, ... in ascending order.  part: the caller's,
// so that it is allocated once per problem.
template <int NSUM, class Edge>
inline void lm_pass_host(int order, int n, std::vector<double>& part, double* sum, Edge edge) {
    if (order == ORBM_POSE_ORDER_INDEX) {
        for (int k = 0; k < NSUM; ++k) sum[k] = 0.0;
        for (int e = 0; e < n; ++e) edge(e, sum);
        return;
    }
    part.assign((size_t)LM_T * NSUM, 0.0);
    for (int l = 0; l < LM_T && l < n; ++l)
        for (int e = l; e < n; e += LM_T) edge(e, &part[(size_t)l * NSUM]);
    lm_tree_host<NSUM>(part.data(), sum);
}

// ---- the batched call -------------------------------------------------------------------------------------------------------------------
// The problems at or under `cap` go to the device in one launch -- launch(list, &flags_off) stages and enqueues, the kernel leaves B
// records and behind them (at flags_off) the flags in port.out -- while the host routine, host(b), takes the longer ones; then records
// and flags of the device's problems are copied out.  last[0], last[1]: how many problems went to the device and to the host.
template <class Result, class Launch, class Host>
int lm_csr_call(orbm_matcher* m, PortBufs<uint8_t>& port, int B, const int32_t* first, int cap, uint8_t* flag_out, Result* results,
                int* last, Launch launch, Host host) {
    std::vector<int32_t> list;
    for (int b = 0; b < B; ++b) if (first[b + 1] - first[b] <= cap) list.push_back(b);
    size_t flags_off = 0;
    if (!list.empty()) {
        MORB_HIP(hipSetDevice(m->device));
        const int rc = launch(list, &flags_off);
        if (rc) return rc;
    }
    for (int b = 0; b < B; ++b)             // while the kernel runs
        if (first[b + 1] - first[b] > cap) host(b);
    if (!list.empty()) {
        MORB_HIP(hipStreamSynchronize(m->stream));
        const Result* R = (const Result*)port.out.p;
        for (int b : list) {
            results[b] = R[b];
            memcpy(flag_out + first[b], port.out.p + flags_off + first[b], (size_t)(first[b + 1] - first[b]));
        }
    }
    last[0] = (int)list.size(); last[1] = B - (int)list.size();
    return ORB_OK;
}
