// essgraph.hip -- the essential graph on the device (include/orbm.h, "essential graph"): Optimizer::OptimizeEssentialGraph (reference
// src/Optimizer.cc:1373-1677) from its graph on.  The statements are eg_dev.h's, ONE definition for the kernels and the host routine;
// here are the structure of a call (eg_graph: hessian indices, the CSR of every active free vertex's edges, the sorted block pairs that
// have an edge and their CSR), the sequence (eg_flow: g2o's optimize() loop without a stop flag) and its two backends:
//   EgHost     loops, in either order
//   EgDevice   per linearisation k_eg_perturb (one lane per vertex and step), k_eg_eval (one lane per edge and evaluation), k_eg_jacobian,
//              k_eg_chi<false>, k_eg_blocks (one wave per 7x7 block that exists, its b segment with a diagonal block), k_eg_ctl_full; per
//              Levenberg trial k_eg_damp, ba_ldlt_dev.h's blocked LDL^T, k_eg_update, k_eg_chi<true>, k_eg_ctl_trial, which leaves one
//              4-byte command word in mapped memory; k_eg_finish and k_eg_correct_points behind the last iteration.
// Every launch ends on its own: no kernel waits for another, no atomics, no order that depends on arrival.  Accepting a trial is a choice
// of buffer (LbaCtl::cur).  Double throughout, multiply and add separate; no libm function runs in a kernel.  Every block of the system
// without an edge is the 0.0 k_eg_fill_zero wrote once per call.
// Bounds: every kernel guards its lane against the count it was launched for; Hs is n x n with n = 7 na and every access is
// (7 i + r) * n + 7 j + c with i, j < na and r, c < 7.
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
#include "eg_dev.h"
#include "ba_ldlt_dev.h"
#include "stage_pack.h"

namespace {

static_assert(EG_T == LM_T, "the partials are lm_dev.h's tree");
static_assert(7 * ORBM_EG_MAX_FREE <= 6 * ORBM_BA_MAX_FREE, "the rows the blocked solver is sized for");

// ---- the structure of a call: initializeOptimization() -----------------------------------------------------------------------------------
struct EgGraph {
    const orbm_eg_problem* P;
    int na = 0, n_pairs = 0, active_vertices = 0;
    std::vector<int32_t> hidx, act, vfirst, vedge, pairs, pfirst, pedge;
};
void eg_graph(const orbm_eg_problem* P, EgGraph& G) {
    G.P = P;
    const int nv = P->n_vertices, ne = P->n_edges;
    std::vector<uint8_t> has(std::max(nv, 1), 0);
    for (int e = 0; e < ne; ++e) { has[P->edge_v0[e]] = 1; has[P->edge_v1[e]] = 1; }
    G.hidx.assign(std::max(nv, 1), -1);
    for (int v = 0; v < nv; ++v) {
        if (!has[v]) continue;
        ++G.active_vertices;
        if (v < P->n_free) { G.hidx[v] = G.na++; G.act.push_back(v); }
    }
    G.vfirst.assign(G.na + 1, 0);
    for (int e = 0; e < ne; ++e)
        for (int role = 0; role < 2; ++role) { const int h = G.hidx[role ? P->edge_v1[e] : P->edge_v0[e]]; if (h >= 0) ++G.vfirst[h + 1]; }
    for (int a = 0; a < G.na; ++a) G.vfirst[a + 1] += G.vfirst[a];
    G.vedge.assign(std::max(G.vfirst[G.na], 1), 0);
    std::vector<int32_t> fill(G.vfirst.begin(), G.vfirst.end());
    for (int e = 0; e < ne; ++e)
        for (int role = 0; role < 2; ++role) { const int h = G.hidx[role ? P->edge_v1[e] : P->edge_v0[e]]; if (h >= 0) G.vedge[fill[h]++] = e; }
    struct Key { int32_t i1, i2, e; };
    std::vector<Key> keys;
    for (int e = 0; e < ne; ++e) {
        const int h0 = G.hidx[P->edge_v0[e]], h1 = G.hidx[P->edge_v1[e]];
        if (h0 >= 0 && h1 >= 0) keys.push_back({std::min(h0, h1), std::max(h0, h1), e});
    }
    std::sort(keys.begin(), keys.end(), [](const Key& a, const Key& b) { return a.i1 != b.i1 ? a.i1 < b.i1 : a.i2 != b.i2 ? a.i2 < b.i2 : a.e < b.e; });
    G.pfirst.assign(1, 0);
    for (size_t k = 0; k < keys.size(); ++k) {
        if (k == 0 || keys[k].i1 != keys[k - 1].i1 || keys[k].i2 != keys[k - 1].i2) {
            if (k) G.pfirst.push_back((int32_t)k);
            G.pairs.push_back(keys[k].i1); G.pairs.push_back(keys[k].i2);
        }
        G.pedge.push_back(keys[k].e);
    }
    G.n_pairs = (int)(G.pairs.size() / 2);
    if (G.n_pairs) G.pfirst.push_back((int32_t)keys.size());
    if (G.pairs.empty()) G.pairs.assign(2, 0);
    if (G.pedge.empty()) G.pedge.assign(1, 0);
}

int eg_validate(const orbm_eg_problem* P, int n_iterations, const orbm_eg_result* R) {
    MORB_ARG(P != nullptr && R != nullptr && n_iterations >= 0);
    MORB_ARG(P->n_free >= 0 && P->n_vertices >= P->n_free && P->n_edges >= 0 && P->n_points >= 0);
    MORB_ARG(P->n_vertices == 0 || P->vertex != nullptr);
    MORB_ARG(P->n_edges == 0 || (P->measurement && P->edge_v0 && P->edge_v1));
    MORB_ARG(P->n_points == 0 || (P->points && P->point_ref));
    MORB_ARG((P->n_vertices == 0 || (R->estimate && R->Tiw)) && (P->n_points == 0 || R->point_f));
    for (int e = 0; e < P->n_edges; ++e) {
        const int a = P->edge_v0[e], b = P->edge_v1[e];
        if (a < 0 || a >= P->n_vertices || b < 0 || b >= P->n_vertices || a == b) { morb::set_error("edge %d joins vertices %d and %d", e, a, b); return ORB_E_ARG; }
    }
    for (int l = 0; l < P->n_points; ++l)
        if (P->point_ref[l] < -1 || P->point_ref[l] >= P->n_vertices) { morb::set_error("point %d refers to vertex %d", l, P->point_ref[l]); return ORB_E_ARG; }
    return ORB_OK;
}

// ---- the sequence --------------------------------------------------------------------------------------------------------------------------
struct EgReport { int32_t want_trial, more, ok; };
// the ONE 4-byte command word per trial, the local BA's: bit 0 want_trial, bit 1 more, bit 2 ok, bits 8 .. 31 the step it answers
__host__ __device__ inline uint32_t eg_command_word(const LbaCtl& S, int seq) {
    return (uint32_t)(S.want_trial ? 1 : 0) | (uint32_t)(S.more ? 2 : 0) | (uint32_t)(S.ok ? 4 : 0) | ((uint32_t)seq << 8);
}
// after computeActiveErrors + buildSystem at the estimate: lm_dev.h's rule with computeLambdaInit's user value
__host__ __device__ inline void eg_ctl_full(LbaCtl& S, double chi) {
    const bool first = S.iter == 0;
    lm_rule_full(S, chi, 0.0);
    if (first) S.lambda = EG_LAMBDA_INIT;
}
__host__ __device__ inline void eg_ctl_trial(LbaCtl& S, double chi, double scale) {
    lba_ctl_trial_end(S, chi, scale);
    if (!S.want_trial) lba_ctl_iter_end(S);
}
// initializeOptimization() and optimize(n_iterations) (core/sparse_optimizer.cpp:354-419; forceStopFlag is null), then steps 6 and 7
template <class Backend>
int eg_flow(Backend& B, const EgGraph& G, int n_iterations, orbm_eg_result* R) {
    int rc;
    R->optimised = 0; R->active_vertices = G.active_vertices; R->active_edges = G.P->n_edges; R->reserved = 0;
    if (G.na > 0) {                                       // else `_ivMap.size() == 0`: optimize() returns -1 before its loop
        R->optimised = 1;
        EgReport rep = {0, n_iterations > 0 ? 1 : 0, 1};
        while (rep.more && rep.ok) {                      // for (int i=0; i<iterations && ! terminate() && ok; i++)
            if ((rc = B.iteration(&rep))) return rc;
            while (rep.want_trial)                        // `while (rho<0 && qmax < 10 && ! _optimizer->terminate())`
                if ((rc = B.trial(&rep))) return rc;
        }
    }
    return B.finish(R);
}

// sum of v[0 .. n-1]: sequential (INDEX), or positions 256 k .. 256 k + 255 through lm_dev.h's tree, the partials in ascending k (DEVICE)
double eg_sum_host(const double* v, int n, int order) {
    double s = 0.0;
    if (order == ORBM_POSE_ORDER_INDEX) { for (int k = 0; k < n; ++k) s += v[k]; return s; }
    for (int base = 0; base < n; base += EG_T) {
        double part[EG_T], sum;
        for (int l = 0; l < EG_T; ++l) part[l] = base + l < n ? v[base + l] : 0.0;
        lm_tree_host<1>(part, &sum);
        s += sum;
    }
    return s;
}
void eg_write_result(const orbm_eg_problem* P, const double* est, orbm_eg_result* R) {
    for (int v = 0; v < P->n_vertices; ++v) {
        for (int k = 0; k < 8; ++k) R->estimate[8 * (size_t)v + k] = x86_nan(est[8 * (size_t)v + k]);
        eg_Tiw(est + 8 * (size_t)v, R->Tiw + 16 * (size_t)v);
    }
}
void eg_take_round(const LbaCtl& S, orbm_eg_result* R) { R->round = S.round[0]; }

// ---- host routine --------------------------------------------------------------------------------------------------------------------------
struct EgHost {
    const EgGraph& G;
    int order, n;
    EgView V;
    LbaCtl S;
    std::vector<double> est[2], pert, evals, J, leaf, Hs, bs, diag, x, sterm, xt;

    EgHost(const EgGraph& g, int ord, int max_iter) : G(g), order(ord), n(7 * g.na) {
        const orbm_eg_problem* P = G.P;
        const size_t ne = (size_t)std::max(P->n_edges, 1), nv = (size_t)std::max(P->n_vertices, 1), na = (size_t)std::max(G.na, 1);
        for (int b = 0; b < 2; ++b) { est[b].assign(8 * nv, 0.0); if (P->n_vertices) memcpy(est[b].data(), P->vertex, 64 * (size_t)P->n_vertices); }
        pert.assign(na * 28 * 8, 0.0); evals.assign(ne * EG_SLOTS * 7, 0.0); J.assign(ne * 98, 0.0); leaf.assign(ne, 0.0);
        Hs.assign((size_t)std::max(n, 1) * std::max(n, 1), 0.0); bs.assign(7 * na, 0.0); diag.assign(7 * na, 0.0);
        x.assign(7 * na, 0.0); sterm.assign(7 * na, 0.0); xt.assign(7 * na, 0.0);
        lba_ctl_begin(S, order);
        lba_ctl_begin_optimisation(S, 0, max_iter);
        memset(&V, 0, sizeof(V));
        V.n_free = P->n_free; V.n_vertices = P->n_vertices; V.n_edges = P->n_edges; V.n_points = P->n_points; V.fix_scale = P->fix_scale;
        V.na = G.na; V.n_pairs = G.n_pairs;
        V.meas = P->measurement; V.ev0 = P->edge_v0; V.ev1 = P->edge_v1; V.hidx = G.hidx.data(); V.act = G.act.data();
        V.vfirst = G.vfirst.data(); V.vedge = G.vedge.data(); V.pairs = G.pairs.data(); V.pfirst = G.pfirst.data(); V.pedge = G.pedge.data();
        V.est[0] = est[0].data(); V.est[1] = est[1].data(); V.pert = pert.data(); V.evals = evals.data(); V.J = J.data();
        V.Hs = Hs.data(); V.bs = bs.data(); V.diag = diag.data(); V.x = x.data(); V.sterm = sterm.data(); V.S = &S;
    }
    void report(EgReport* rep) const { rep->want_trial = S.want_trial; rep->more = S.more; rep->ok = S.ok; }
    int iteration(EgReport* rep) {
        const int ne = V.n_edges;
        for (int a = 0; a < V.na; ++a)
            for (int s = 0; s < 14; ++s)
                eg_perturb(V.est[S.cur] + 8 * (size_t)V.act[a], s, V.fix_scale, order, V.pert + ((size_t)a * 28 + s) * 8, V.pert + ((size_t)a * 28 + 14 + s) * 8);
        for (int e = 0; e < ne; ++e)
            for (int s = 0; s < EG_SLOTS; ++s) eg_slot(V, e, s, S.cur, order, V.evals + ((size_t)e * EG_SLOTS + s) * 7);
        for (int e = 0; e < ne; ++e)
            for (int role = 0; role < 2; ++role)
                if (V.hidx[role ? V.ev1[e] : V.ev0[e]] >= 0)
                    for (int d = 0; d < 7; ++d) eg_jacobian_column(V, e, role, d);
        for (int e = 0; e < ne; ++e) leaf[e] = eg_chi2(V.evals + (size_t)e * EG_SLOTS * 7);
        const double chi = eg_sum_host(leaf.data(), ne, order);
        for (int a = 0; a < V.na; ++a)
            for (int r = 0; r < 7; ++r) {
                for (int c = 0; c < 7; ++c) V.Hs[(size_t)(7 * a + r) * n + 7 * a + c] = eg_diag_entry(V, a, r, c);
                V.diag[7 * a + r] = V.Hs[(size_t)(7 * a + r) * n + 7 * a + r];
                V.bs[7 * a + r] = eg_b_entry(V, a, r);
            }
        for (int p = 0; p < V.n_pairs; ++p)
            for (int r = 0; r < 7; ++r)
                for (int c = 0; c < 7; ++c) V.Hs[(size_t)(7 * V.pairs[2 * p] + r) * n + 7 * V.pairs[2 * p + 1] + c] = eg_pair_entry(V, p, r, c);
        eg_ctl_full(S, chi);
        return trial(rep);
    }
    int trial(EgReport* rep) {
        for (int i = 0; i < n; ++i) V.Hs[(size_t)i * n + i] = V.diag[i] + S.lambda;      // setLambda
        const int ok = orbm_ba_ldlt(n, V.Hs, V.bs, xt.data());
        if (ok < 0) return ok;
        S.ok2 = ok;
        if (ok) for (int i = 0; i < n; ++i) V.x[i] = xt[i];
        for (int a = 0; a < V.na; ++a) eg_update_vertex(V, a, order);
        for (int e = 0; e < V.n_edges; ++e) {
            double e7[7];
            eg_error(V.meas + 8 * (size_t)e, V.est[S.cur ^ 1] + 8 * (size_t)V.ev0[e], V.est[S.cur ^ 1] + 8 * (size_t)V.ev1[e], order, e7);
            leaf[e] = eg_chi2(e7);
        }
        const double chi = eg_sum_host(leaf.data(), V.n_edges, order);
        const double scale = eg_sum_host(V.sterm, n, order);
        eg_ctl_trial(S, chi, scale);
        report(rep);
        return ORB_OK;
    }
    int finish(orbm_eg_result* R) {
        const orbm_eg_problem* P = G.P;
        eg_write_result(P, V.est[S.cur], R);
        for (int l = 0; l < P->n_points; ++l)
            eg_correct_point(P->vertex, V.est[S.cur], P->point_ref[l], P->points + 3 * (size_t)l, R->point_f + 3 * (size_t)l);
        eg_take_round(S, R);
        return ORB_OK;
    }
};

int eg_host(const EgGraph& G, int n_iterations, int order, orbm_eg_result* R) {
    EgHost H(G, order, n_iterations);
    return eg_flow(H, G, n_iterations, R);
}

// ---- kernels -------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EG_T) void k_eg_init(EgView V, const double* vertex0, LbaCtl S0) {
    const size_t t = (size_t)blockIdx.x * EG_T + threadIdx.x, T = (size_t)gridDim.x * EG_T;
    for (size_t k = t; k < 8 * (size_t)V.n_vertices; k += T) { V.est[0][k] = vertex0[k]; V.est[1][k] = vertex0[k]; }
    for (size_t k = t; k < 7 * (size_t)V.na; k += T) { V.x[k] = 0.0; V.sterm[k] = 0.0; }
    if (t == 0) *V.S = S0;
}
__global__ __launch_bounds__(EG_T) void k_eg_fill_zero(double* p, size_t count) {
    for (size_t k = (size_t)blockIdx.x * EG_T + threadIdx.x; k < count; k += (size_t)gridDim.x * EG_T) p[k] = 0.0;
}
// one lane per (active free vertex, step): its perturbed estimate and the inverse of it, once per linearisation
__global__ __launch_bounds__(EG_T) void k_eg_perturb(EgView V) {
    const int t = blockIdx.x * EG_T + threadIdx.x;
    if (t >= 14 * V.na) return;
    const int a = t / 14, s = t % 14;
    eg_perturb(V.est[V.S->cur] + 8 * (size_t)V.act[a], s, V.fix_scale, ORBM_POSE_ORDER_DEVICE, V.pert + ((size_t)a * 28 + s) * 8,
               V.pert + ((size_t)a * 28 + 14 + s) * 8);
}
// one lane per (edge, evaluation): two Sim3 products and a logarithm
__global__ __launch_bounds__(EG_T) void k_eg_eval(EgView V) {
    const size_t t = (size_t)blockIdx.x * EG_T + threadIdx.x;
    if (t >= (size_t)EG_SLOTS * V.n_edges) return;
    const int e = (int)(t / EG_SLOTS), s = (int)(t % EG_SLOTS);
    double e7[7];
    if (!eg_slot(V, e, s, V.S->cur, ORBM_POSE_ORDER_DEVICE, e7)) return;
    double* out = V.evals + t * 7;
#pragma unroll
    for (int k = 0; k < 7; ++k) out[k] = e7[k];
}
// one lane per (edge, vertex, column)
__global__ __launch_bounds__(EG_T) void k_eg_jacobian(EgView V) {
    const size_t t = (size_t)blockIdx.x * EG_T + threadIdx.x;
    if (t >= 14 * (size_t)V.n_edges) return;
    const int e = (int)(t / 14), role = (int)(t % 14) / 7, d = (int)(t % 7);
    if (V.hidx[role ? V.ev1[e] : V.ev0[e]] >= 0) eg_jacobian_column(V, e, role, d);
}
// one lane per edge position; the workgroup's chi2 partial through lm_dev.h's tree.  TRIAL: the errors at the trial estimates;
// otherwise the ones k_eg_eval left at the estimates
template <bool TRIAL>
__global__ __launch_bounds__(EG_T) void k_eg_chi(EgView V) {
    __shared__ double s_part[EG_T / 64][1];
    const int e = blockIdx.x * EG_T + threadIdx.x;
    double chi[1] = {0.0};
    if (e < V.n_edges) {
        if (TRIAL) {
            const int buf = V.S->cur ^ 1;
            double e7[7];
            eg_error(V.meas + 8 * (size_t)e, V.est[buf] + 8 * (size_t)V.ev0[e], V.est[buf] + 8 * (size_t)V.ev1[e], ORBM_POSE_ORDER_DEVICE, e7);
            chi[0] = eg_chi2(e7);
        } else {
            chi[0] = eg_chi2(V.evals + (size_t)e * EG_SLOTS * 7);
        }
    }
    lm_wave_sums(chi, 0, s_part, threadIdx.x);
    __syncthreads();
    if (threadIdx.x == 0) { lm_add_waves(s_part, chi); V.partial[blockIdx.x] = chi[0]; }
}
// one wave per block that exists: blockIdx.x < na the diagonal block of that hessian index (lanes 0 .. 48 its entries, 49 .. 55 its b
// segment), the others the sorted pairs
__global__ __launch_bounds__(64) void k_eg_blocks(EgView V) {
    const int t = threadIdx.x, n = 7 * V.na;
    if ((int)blockIdx.x < V.na) {
        const int a = blockIdx.x;
        if (t < 49) {
            const int r = t / 7, c = t % 7;
            const double h = eg_diag_entry(V, a, r, c);
            V.Hs[(size_t)(7 * a + r) * n + 7 * a + c] = h;
            if (r == c) V.diag[7 * a + r] = h;
        } else if (t < 56) {
            V.bs[7 * a + t - 49] = eg_b_entry(V, a, t - 49);
        }
        return;
    }
    const int p = blockIdx.x - V.na;
    if (p >= V.n_pairs || t >= 49) return;
    const int r = t / 7, c = t % 7;
    V.Hs[(size_t)(7 * V.pairs[2 * (size_t)p] + r) * n + 7 * V.pairs[2 * (size_t)p + 1] + c] = eg_pair_entry(V, p, r, c);
}
// the pass's chi2 (the partials in ascending order), the controller at the estimate
__global__ void k_eg_ctl_full(EgView V, int n_partials) {
    double chi = 0.0;
    for (int k = 0; k < n_partials; ++k) chi += V.partial[k];
    eg_ctl_full(*V.S, chi);
}
__global__ __launch_bounds__(EG_T) void k_eg_damp(EgView V) {
    const int i = blockIdx.x * EG_T + threadIdx.x, n = 7 * V.na;
    if (i < n) V.Hs[(size_t)i * n + i] = V.diag[i] + V.S->lambda;
}
__global__ __launch_bounds__(EG_T) void k_eg_update(EgView V) {
    const int a = blockIdx.x * EG_T + threadIdx.x;
    if (a < V.na) eg_update_vertex(V, a, ORBM_POSE_ORDER_DEVICE);
}
// One workgroup: the trial's chi2, computeScale through the tree (positions 256 k .. 256 k + 255 of x, the partials in ascending k), the
// controller's verdict and the iteration's end when no trial follows; the command word for the host.
__global__ __launch_bounds__(EG_T) void k_eg_ctl_trial(EgView V, int n_partials, uint32_t* word, int seq) {
    __shared__ double s_part[EG_T / 64][1];
    const int n = 7 * V.na;
    double scale = 0.0;
    for (int base = 0; base < n; base += EG_T) {
        double v[1] = {base + (int)threadIdx.x < n ? V.sterm[base + threadIdx.x] : 0.0};
        lm_wave_sums(v, 0, s_part, threadIdx.x);
        __syncthreads();
        if (threadIdx.x == 0) { lm_add_waves(s_part, v); scale += v[0]; }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    double chi = 0.0;
    for (int k = 0; k < n_partials; ++k) chi += V.partial[k];
    LbaCtl& S = *V.S;
    eg_ctl_trial(S, chi, scale);
    *word = eg_command_word(S, seq);
}
// the estimates and the controller's record into mapped memory
__global__ __launch_bounds__(EG_T) void k_eg_finish(EgView V, double* est_out, LbaCtl* ctl_out) {
    const size_t t = (size_t)blockIdx.x * EG_T + threadIdx.x, T = (size_t)gridDim.x * EG_T;
    const int cur = V.S->cur;
    for (size_t k = t; k < 8 * (size_t)V.n_vertices; k += T) est_out[k] = V.est[cur][k];
    if (t == 0) *ctl_out = *V.S;
}
// step 7, one lane per point
__global__ __launch_bounds__(EG_T) void k_eg_correct_points(EgView V, const double* vertex0, const float* points, const int32_t* point_ref, float* out) {
    const int l = blockIdx.x * EG_T + threadIdx.x;
    if (l < V.n_points) eg_correct_point(vertex0, V.est[V.S->cur], point_ref[l], points + 3 * (size_t)l, out + 3 * (size_t)l);
}

// ---- the device backend ------------------------------------------------------------------------------------------------------------------
inline unsigned eg_blocks(size_t n) { return (unsigned)std::max<size_t>(1, (n + EG_T - 1) / EG_T); }

struct EgDevice {
    orbm_matcher* m;
    const EgGraph& G;
    EgView V;
    BaSolve A;
    morb::StagePack pk;
    std::optional<morb::StagePack::Block> blk_;
    int i_vertex = 0, i_points = 0, i_ref = 0;
    uint32_t* rep_h = nullptr; uint32_t* rep_d = nullptr;
    LbaCtl* ctl_h = nullptr; LbaCtl* ctl_d = nullptr;
    double* est_h = nullptr; double* est_d = nullptr;
    float* pts_h = nullptr; float* pts_d = nullptr;
    int n_partials = 0, seq = 0, launches = 0, syncs = 0;

    EgDevice(orbm_matcher* mm, const EgGraph& g) : m(mm), G(g) {}

    int sync(EgReport* rep) {
        MORB_HIP(hipGetLastError());
        MORB_HIP(hipStreamSynchronize(m->stream));
        ++syncs;
        if (rep) {
            const uint32_t w = *rep_h;
            if ((int)(w >> 8) != seq) { morb::set_error("essential graph: the command word of step %d did not arrive", seq); return ORB_E_HIP; }
            rep->want_trial = w & 1; rep->more = (w >> 1) & 1; rep->ok = (w >> 2) & 1;
        }
        return ORB_OK;
    }
    int open(int max_iter) {
        const orbm_eg_problem* P = G.P;
        const size_t ne = (size_t)std::max(P->n_edges, 1), nv = (size_t)std::max(P->n_vertices, 1), na = (size_t)std::max(G.na, 1),
                     np = (size_t)std::max(P->n_points, 1), n = 7 * na;
        MORB_HIP(hipSetDevice(m->device));
        i_vertex = pk.add(P->vertex, (size_t)P->n_vertices * 64);
        const int i_meas = pk.add(P->measurement, (size_t)P->n_edges * 64), i_v0 = pk.add(P->edge_v0, (size_t)P->n_edges * 4),
                  i_v1 = pk.add(P->edge_v1, (size_t)P->n_edges * 4), i_hidx = pk.add(G.hidx.data(), (size_t)P->n_vertices * 4),
                  i_act = pk.add(G.act.data(), (size_t)G.na * 4), i_vfirst = pk.add(G.vfirst.data(), (size_t)(G.na + 1) * 4),
                  i_vedge = pk.add(G.vedge.data(), (size_t)G.vfirst[G.na] * 4), i_pairs = pk.add(G.pairs.data(), (size_t)G.n_pairs * 8),
                  i_pfirst = pk.add(G.pfirst.data(), (size_t)(G.n_pairs + 1) * 4), i_pedge = pk.add(G.pedge.data(), (size_t)G.pfirst[G.n_pairs] * 4);
        i_points = pk.add(P->points, (size_t)P->n_points * 12); i_ref = pk.add(P->point_ref, (size_t)P->n_points * 4);
        int rc;
        blk_.emplace(pk.open(m->lba.stage, &rc));
        if (rc) return rc;
        const morb::StagePack::Block& blk = *blk_;
        morb::BlockLayout L;
        const size_t o_e0 = L.take(64 * nv), o_e1 = L.take(64 * nv), o_pert = L.take(na * 28 * 64), o_ev = L.take(ne * EG_SLOTS * 56),
                     o_J = L.take(ne * 98 * 8), o_part = L.take((size_t)eg_blocks(ne) * 8), o_Hs = L.take(n * n * 8), o_bs = L.take(n * 8),
                     o_diag = L.take(n * 8), o_x = L.take(n * 8), o_st = L.take(n * 8), o_Lt = L.take(n * n * 8), o_d = L.take(n * 8),
                     o_y = L.take(n * 8), o_carry = L.take(n * 8), o_fail = L.take(16), o_S = L.take(sizeof(LbaCtl));
        if ((rc = m->lba.scratch.reserve(L.off))) return rc;
        morb::BlockLayout O;
        const size_t q_rep = O.take(64), q_ctl = O.take(sizeof(LbaCtl)), q_est = O.take(64 * nv), q_pts = O.take(12 * np);
        if ((rc = m->lba.out.reserve(O.off))) return rc;
        uint8_t* hp = m->lba.out.p; uint8_t* dp = m->lba.out.dp; uint8_t* sp = m->lba.scratch.p;
        rep_h = (uint32_t*)(hp + q_rep); rep_d = (uint32_t*)(dp + q_rep); ctl_h = (LbaCtl*)(hp + q_ctl); ctl_d = (LbaCtl*)(dp + q_ctl);
        est_h = (double*)(hp + q_est); est_d = (double*)(dp + q_est); pts_h = (float*)(hp + q_pts); pts_d = (float*)(dp + q_pts);
        *rep_h = 0;
        memset(&V, 0, sizeof(V));
        V.n_free = P->n_free; V.n_vertices = P->n_vertices; V.n_edges = P->n_edges; V.n_points = P->n_points; V.fix_scale = P->fix_scale;
        V.na = G.na; V.n_pairs = G.n_pairs;
        V.meas = blk.dev<double>(i_meas); V.ev0 = blk.dev<int32_t>(i_v0); V.ev1 = blk.dev<int32_t>(i_v1); V.hidx = blk.dev<int32_t>(i_hidx);
        V.act = blk.dev<int32_t>(i_act); V.vfirst = blk.dev<int32_t>(i_vfirst); V.vedge = blk.dev<int32_t>(i_vedge);
        V.pairs = blk.dev<int32_t>(i_pairs); V.pfirst = blk.dev<int32_t>(i_pfirst); V.pedge = blk.dev<int32_t>(i_pedge);
        V.est[0] = (double*)(sp + o_e0); V.est[1] = (double*)(sp + o_e1); V.pert = (double*)(sp + o_pert); V.evals = (double*)(sp + o_ev);
        V.J = (double*)(sp + o_J); V.partial = (double*)(sp + o_part); V.Hs = (double*)(sp + o_Hs); V.bs = (double*)(sp + o_bs);
        V.diag = (double*)(sp + o_diag); V.x = (double*)(sp + o_x); V.sterm = (double*)(sp + o_st); V.S = (LbaCtl*)(sp + o_S);
        A = BaSolve{7 * G.na, V.Hs, V.bs, (double*)(sp + o_Lt), (double*)(sp + o_d), (double*)(sp + o_y), (double*)(sp + o_carry), V.x,
                    (int*)(sp + o_fail), &V.S->ok2};
        n_partials = P->n_edges > 0 ? (int)eg_blocks(ne) : 0;
        blk.publish();
        LbaCtl S0;
        lba_ctl_begin(S0, ORBM_POSE_ORDER_DEVICE);
        lba_ctl_begin_optimisation(S0, 0, max_iter);
        hipStream_t st = m->stream;
        hipLaunchKernelGGL(k_eg_init, dim3(eg_blocks(8 * nv)), dim3(EG_T), 0, st, V, blk.dev<double>(i_vertex), S0);
        hipLaunchKernelGGL(k_eg_fill_zero, dim3(std::min(eg_blocks(n * n), 4096u)), dim3(EG_T), 0, st, V.Hs, n * n);
        launches += 2;
        return ORB_OK;
    }
    void enqueue_trial() {
        hipStream_t st = m->stream;
        hipLaunchKernelGGL(k_eg_damp, dim3(eg_blocks(7 * (size_t)V.na)), dim3(EG_T), 0, st, V);
        launches += ba_ldlt_enqueue(st, A);
        hipLaunchKernelGGL(k_eg_update, dim3(eg_blocks((size_t)V.na)), dim3(EG_T), 0, st, V);
        hipLaunchKernelGGL(k_eg_chi<true>, dim3(eg_blocks((size_t)V.n_edges)), dim3(EG_T), 0, st, V);
        hipLaunchKernelGGL(k_eg_ctl_trial, dim3(1), dim3(EG_T), 0, st, V, n_partials, rep_d, ++seq);
        launches += 4;
    }
    int iteration(EgReport* rep) {
        hipStream_t st = m->stream;
        hipLaunchKernelGGL(k_eg_perturb, dim3(eg_blocks(14 * (size_t)V.na)), dim3(EG_T), 0, st, V);
        hipLaunchKernelGGL(k_eg_eval, dim3(eg_blocks((size_t)EG_SLOTS * V.n_edges)), dim3(EG_T), 0, st, V);
        hipLaunchKernelGGL(k_eg_jacobian, dim3(eg_blocks(14 * (size_t)V.n_edges)), dim3(EG_T), 0, st, V);
        hipLaunchKernelGGL(k_eg_chi<false>, dim3(eg_blocks((size_t)V.n_edges)), dim3(EG_T), 0, st, V);
        hipLaunchKernelGGL(k_eg_blocks, dim3((unsigned)(V.na + V.n_pairs)), dim3(64), 0, st, V);
        hipLaunchKernelGGL(k_eg_ctl_full, dim3(1), dim3(1), 0, st, V, n_partials);
        launches += 6;
        enqueue_trial();
        return sync(rep);
    }
    int trial(EgReport* rep) { enqueue_trial(); return sync(rep); }
    int finish(orbm_eg_result* R) {
        const orbm_eg_problem* P = G.P;
        hipStream_t st = m->stream;
        hipLaunchKernelGGL(k_eg_finish, dim3(eg_blocks(8 * (size_t)V.n_vertices)), dim3(EG_T), 0, st, V, est_d, ctl_d);
        hipLaunchKernelGGL(k_eg_correct_points, dim3(eg_blocks((size_t)V.n_points)), dim3(EG_T), 0, st, V, blk_->dev<double>(i_vertex),
                           blk_->dev<float>(i_points), blk_->dev<int32_t>(i_ref), pts_d);
        launches += 2;
        const int rc = sync(nullptr);
        if (rc) return rc;
        eg_write_result(P, est_h, R);
        if (P->n_points) memcpy(R->point_f, pts_h, 12 * (size_t)P->n_points);
        eg_take_round(*ctl_h, R);
        return ORB_OK;
    }
};

}  // namespace

extern "C" {

int orbm_essential_graph_host(const orbm_eg_problem* problem, int n_iterations, int order, orbm_eg_result* result) {
    const int rc = eg_validate(problem, n_iterations, result);
    if (rc) return rc;
    if (order != ORBM_POSE_ORDER_INDEX && order != ORBM_POSE_ORDER_DEVICE) { morb::set_error("order = %d", order); return ORB_E_ARG; }
    EgGraph G;
    eg_graph(problem, G);
    return eg_host(G, n_iterations, order, result);
}

int orbm_essential_graph(orbm_matcher* m, const orbm_eg_problem* problem, int n_iterations, orbm_eg_result* result) {
    MORB_ARG(m != nullptr);
    int rc = eg_validate(problem, n_iterations, result);
    if (rc) return rc;
    const bool beyond = problem->n_free > ORBM_EG_MAX_FREE || problem->n_vertices > ORBM_EG_MAX_VERTICES || problem->n_edges > ORBM_EG_MAX_EDGES ||
                        problem->n_points > ORBM_EG_MAX_POINTS;
    EgGraph G;
    eg_graph(problem, G);
    for (int k = 0; k < 8; ++k) m->last_eg[k] = 0;
    if (beyond || G.na == 0) {
        m->last_eg[0] = beyond ? 1 : 2;
        return eg_host(G, n_iterations, ORBM_POSE_ORDER_DEVICE, result);
    }
    EgDevice D(m, G);
    if ((rc = D.open(n_iterations))) return rc;
    rc = eg_flow(D, G, n_iterations, result);
    if (rc) { (void)hipStreamSynchronize(m->stream); return rc; }
    m->last_eg[1] = D.launches; m->last_eg[2] = D.syncs; m->last_eg[4] = G.na + G.n_pairs; m->last_eg[5] = G.na * (G.na + 1) / 2;
    m->last_eg[6] = (7 * G.na + BA_PANEL - 1) / BA_PANEL;
    return ORB_OK;
}

int orbm_eg_edge_eval(const double* measurement8, const double* v0_8, const double* v1_8, int fix_scale, int order, double* out106) {
    MORB_ARG(measurement8 && v0_8 && v1_8 && out106);
    if (order != ORBM_POSE_ORDER_INDEX && order != ORBM_POSE_ORDER_DEVICE) { morb::set_error("order = %d", order); return ORB_E_ARG; }
    // a graph of this one edge between two free vertices, through the statements the routines run
    double est[16], pert[2 * 28 * 8], evals[EG_SLOTS * 7], J[98];
    const int32_t v0 = 0, v1 = 1, hidx[2] = {0, 1};
    memcpy(est, v0_8, 64); memcpy(est + 8, v1_8, 64);
    EgView V;
    memset(&V, 0, sizeof(V));
    V.n_free = 2; V.n_vertices = 2; V.n_edges = 1; V.fix_scale = fix_scale; V.na = 2;
    V.meas = measurement8; V.ev0 = &v0; V.ev1 = &v1; V.hidx = hidx; V.est[0] = est; V.est[1] = est; V.pert = pert; V.evals = evals; V.J = J;
    for (int a = 0; a < 2; ++a)
        for (int s = 0; s < 14; ++s) eg_perturb(est + 8 * a, s, fix_scale, order, pert + (a * 28 + s) * 8, pert + (a * 28 + 14 + s) * 8);
    for (int s = 0; s < EG_SLOTS; ++s) eg_slot(V, 0, s, 0, order, evals + 7 * s);
    for (int role = 0; role < 2; ++role) for (int d = 0; d < 7; ++d) eg_jacobian_column(V, 0, role, d);
    for (int k = 0; k < 7; ++k) out106[k] = evals[k];
    out106[7] = eg_chi2(evals);
    for (int k = 0; k < 98; ++k) out106[8 + k] = J[k];
    return ORB_OK;
}

int orbm_sim3_log_eval(const double* sim3_8, int order, double* out7) {
    MORB_ARG(sim3_8 && out7);
    if (order != ORBM_POSE_ORDER_INDEX && order != ORBM_POSE_ORDER_DEVICE) { morb::set_error("order = %d", order); return ORB_E_ARG; }
    Sim3Quat T;
    eg_load(sim3_8, T);
    return sim3_log(T, order, out7);
}

double orbm_pose_acos(double d) { return pose_acos(d); }
double orbm_pose_log(double x) { return pose_log(x); }

}  // extern "C"
