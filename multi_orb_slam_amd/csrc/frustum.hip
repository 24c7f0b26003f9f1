// frustum.hip -- local-map tracking on the device (include/orbm.h, "local-map tracking"): a table of map points resident in
// HBM and Tracking::SearchLocalPoints from its second loop on (reference src/Tracking.cc:1730-1768).
//   k_frustum        one lane per point: Frame::isInFrustum (src/Frame.cc:443-499), MapPoint::PredictScale
//                    (src/MapPoint.cc:602-617) and the query of SearchByProjection(F, vpMapPoints, th) (src/ORBmatcher.cc:62-157),
//                    written as one orbm_query per table row straight into the buffer k_project reads.  A point that is
//                    skipped or fails the test gets a query without a window (cam = -1): it contributes no candidates, and
//                    the query index stays the table index, so the first-come order of the resolve is the table order.
//   frustum_eval     the arithmetic itself, ONE statement sequence for the kernel and for the host (the exact fallback of the
//                    search rebuilds its queries with it; orbm_frustum_host exposes it).  No logarithm on either side: the
//                    level is the number of thresholds (orbm_level_thresholds, built from the C library's logf) the ratio
//                    exceeds.
// The search behind it is search.hip's, unchanged: k_project + the resolve kernels, host_resolve as the fallback.
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/orbm.h"
#include "orb_common.h"
#include "matcher_internal.h"
#include "cv_dev.h"

using namespace morb;

namespace {

struct FrustumView {   // orbm_view by value, the level thresholds and the scale factors included (no table in memory)
    float Rcw[9], tcw[3], Ow[3];
    float fx, fy, cx, cy, mbf;
    float min_x, max_x, min_y, max_y;
    float cos_limit, th;
    int n_levels;
    float thr[ORBM_MAX_LEVELS - 1];
    float scale[ORBM_MAX_LEVELS];
};

struct FrustumOut { float u, v, ur, view_cos, radius; int level; };

// Frame::isInFrustum + PredictScale + the window radius of SearchByProjection, operation for operation in the reference's
// number formats (this library is built without contraction and without fast-math):
//   Pc = mRcw*P + mtcw     one cv::gemm call on its small path, alpha = beta = 1 (cv_dev.h cv_gemm3)
//   cv::norm, Mat::dot     squares / products summed in double from 0.0, in index order (cv_norm3, cv_dot3)
// Returns false where the reference returns false, and for a non-finite projection.
__host__ __device__ inline bool frustum_eval(const FrustumView& V, const float* P, const float* Pn, float min_dist, float max_dist,
                                             FrustumOut& o) {
    float Pc[3];
    for (int k = 0; k < 3; ++k) Pc[k] = cv_gemm3(V.Rcw + 3 * k, 1, P, 1.0, V.tcw[k], 1.0);
    if (Pc[2] < 0.0f) return false;
    const float invz = 1.0f / Pc[2];
    const float u = V.fx * Pc[0] * invz + V.cx;
    const float v = V.fy * Pc[1] * invz + V.cy;
    if (!(fabsf(u) <= 3.402823466e+38f) || !(fabsf(v) <= 3.402823466e+38f)) return false;   // infinite or NaN
    if (u < V.min_x || u > V.max_x) return false;
    if (v < V.min_y || v > V.max_y) return false;
    const float maxDistance = 1.2f * max_dist;
    const float minDistance = 0.8f * min_dist;
    float PO[3];
    for (int k = 0; k < 3; ++k) PO[k] = P[k] - V.Ow[k];
    const float dist = (float)cv_norm3(PO);
    if (dist < minDistance || dist > maxDistance) return false;
    const float viewCos = (float)(cv_dot3(PO, Pn) / (double)dist);
    if (viewCos < V.cos_limit) return false;
    const float ratio = max_dist / dist;
    int level = 0;
    for (int k = 0; k < V.n_levels - 1; ++k) level += (ratio > V.thr[k]) ? 1 : 0;
    float r = ((double)viewCos > 0.998) ? 2.5f : 4.0f;
    if ((double)V.th != 1.0) r *= V.th;
    o.u = u; o.v = v; o.ur = u - V.mbf * invz; o.view_cos = viewCos; o.level = level;
    o.radius = r * V.scale[level];
    return true;
}

__host__ __device__ inline void frustum_records(const FrustumView& V, const orbm_point& pt, bool skipped, orbm_query& Q, orbm_track& T) {
    FrustumOut o;
    const bool in_view = !skipped && frustum_eval(V, pt.pos, pt.normal, pt.min_dist, pt.max_dist, o);
    if (in_view) {
        T.proj_x = o.u; T.proj_y = o.v; T.proj_xr = o.ur; T.view_cos = o.view_cos; T.level = o.level; T.in_view = 1;
        Q.u = o.u; Q.v = o.v; Q.radius = o.radius; Q.ur = o.ur;
        Q.min_level = o.level - 1; Q.max_level = o.level; Q.cam = 0; Q.blocks = pt.blocks ? 1 : 0; Q.angle = 0.0f;
        for (int k = 0; k < 32; ++k) Q.desc[k] = pt.desc[k];
    } else {
        T.proj_x = 0.0f; T.proj_y = 0.0f; T.proj_xr = 0.0f; T.view_cos = 0.0f; T.level = 0; T.in_view = 0;
        Q.u = 0.0f; Q.v = 0.0f; Q.radius = 0.0f; Q.ur = 0.0f;
        Q.min_level = 0; Q.max_level = 0; Q.cam = -1; Q.blocks = 0; Q.angle = 0.0f;   // cam < 0: no window, no candidates
        for (int k = 0; k < 32; ++k) Q.desc[k] = 0;
    }
}

// One lane per point.  A few dozen flops and 160 bytes per point: the launch is what it costs.  `track` is mapped pinned
// host memory (the caller reads it after the stream has been synchronised), `q` the matcher's query buffer in HBM.
// INDEXED (the resident map, localmap.hip): point i is row index[i], and it is skipped if its flag byte says bad or its mark is the
// call's epoch (k_map_mark); otherwise point i is row i and skip[i] decides.
struct FrustumIndex { const int32_t* index; const uint32_t* mark; const uint8_t* flags; uint32_t epoch; };

template <bool INDEXED>
__global__ __launch_bounds__(256) void k_frustum(FrustumView V, const orbm_point* __restrict__ pts, const uint8_t* __restrict__ skip, int n,
                                                 orbm_query* __restrict__ q, orbm_track* __restrict__ track, FrustumIndex X) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int row = i;
    bool skipped;
    if (INDEXED) {
        row = X.index[i];
        skipped = (X.flags[row] & ORBM_POINT_BAD) != 0 || X.mark[row] == X.epoch;
    } else {
        skipped = skip && skip[i] != 0;
    }
    const orbm_point pt = pts[row];
    orbm_query Q; orbm_track T;
    frustum_records(V, pt, skipped, Q, T);
    q[i] = Q;
    track[i] = T;
}

bool level_pred(float r, float lsf, int k) { return std::ceil(logf(r) / lsf) <= (float)k; }

int build_thresholds(float lsf, int n_levels, float* out) {
    if (!(lsf > 0.0f) || !(lsf <= 3.402823466e+38f)) { morb::set_error("log_scale_factor must be positive and finite"); return ORB_E_ARG; }
    for (int k = 0; k < n_levels - 1; ++k) {
        uint32_t lo = 0x00800000u, hi = 0x7f7fffffu;   // smallest normal / largest finite float: the predicate must hold at lo, fail at hi
        float flo, fhi;
        memcpy(&flo, &lo, 4); memcpy(&fhi, &hi, 4);
        if (!level_pred(flo, lsf, k) || level_pred(fhi, lsf, k)) {
            morb::set_error("level %d is not separable for log_scale_factor %g", k, (double)lsf); return ORB_E_ARG;
        }
        while (hi - lo > 1) {   // (bit patterns of positive floats are ordered like the floats)
            const uint32_t mid = lo + (hi - lo) / 2;
            float fm; memcpy(&fm, &mid, 4);
            if (level_pred(fm, lsf, k)) lo = mid; else hi = mid;
        }
        // the bisection assumes ONE flip; hold the C library's logf to that around the threshold
        const uint32_t W = 4096;
        const uint32_t a = lo - 0x00800000u > W ? lo - W : 0x00800000u, b = 0x7f7fffffu - lo > W ? lo + W : 0x7f7fffffu;
        for (uint32_t bits = a; bits <= b; ++bits) {
            float f; memcpy(&f, &bits, 4);
            if (level_pred(f, lsf, k) != (bits <= lo)) {
                morb::set_error("logf is not monotone around the level-%d threshold (log_scale_factor %g)", k, (double)lsf); return ORB_E_ARG;
            }
        }
        memcpy(&out[k], &lo, 4);
    }
    return ORB_OK;
}

int make_view(const orbm_view* v, const float* thr, FrustumView& V) {
    memcpy(V.Rcw, v->Rcw, sizeof(V.Rcw)); memcpy(V.tcw, v->tcw, sizeof(V.tcw)); memcpy(V.Ow, v->Ow, sizeof(V.Ow));
    V.fx = v->fx; V.fy = v->fy; V.cx = v->cx; V.cy = v->cy; V.mbf = v->mbf;
    V.min_x = v->min_x; V.max_x = v->max_x; V.min_y = v->min_y; V.max_y = v->max_y;
    V.cos_limit = v->viewing_cos_limit; V.th = v->th; V.n_levels = v->n_levels;
    for (int k = 0; k < ORBM_MAX_LEVELS - 1; ++k) V.thr[k] = k < v->n_levels - 1 ? thr[k] : 0.0f;
    for (int k = 0; k < ORBM_MAX_LEVELS; ++k) V.scale[k] = k < v->n_levels ? v->scale_factors[k] : 0.0f;
    return ORB_OK;
}

void frustum_host(const FrustumView& V, const orbm_point* pts, const int32_t* index, int n, const uint8_t* skip, orbm_track* track,
                  orbm_query* q, int* n_in) {
    int cnt = 0;
    for (int i = 0; i < n; ++i) {
        orbm_query Q; orbm_track T;
        frustum_records(V, pts[index ? index[i] : i], skip && skip[i] != 0, Q, T);
        cnt += T.in_view;
        if (q) q[i] = Q;
        if (track) track[i] = T;
    }
    if (n_in) *n_in = cnt;
}

int thresholds_of(FrustumScratch& p, const orbm_view* v) {
    if (p.thr_levels == v->n_levels && memcmp(&p.thr_lsf, &v->log_scale_factor, 4) == 0) return ORB_OK;
    p.thr_levels = 0;
    int rc = build_thresholds(v->log_scale_factor, v->n_levels, p.thr);
    if (rc) return rc;
    p.thr_lsf = v->log_scale_factor; p.thr_levels = v->n_levels;
    return ORB_OK;
}

// the skip flags of a source on the host: the caller's, or (resident map) the ones its routine writes into `store`
const uint8_t* host_skip_of(const LocalPointSource& S, int n, std::vector<uint8_t>& store) {
    if (!S.host_skip) return S.skip;
    store.assign((size_t)n, 0);
    S.host_skip(S.host_skip_ctx, store.data());
    return store.data();
}

struct FillCtx { const FrustumView* V; const LocalPointSource* S; int n; orbm_query* q; };
void fill_queries(void* c) {
    const FillCtx* F = (const FillCtx*)c;
    std::vector<uint8_t> store;
    const uint8_t* skip = host_skip_of(*F->S, F->n, store);
    frustum_host(*F->V, F->S->h_rows, F->S->h_index, F->n, skip, nullptr, F->q, nullptr);
}

}  // namespace

struct orbm_points {
    orbm_matcher* owner = nullptr;   // compared, never dereferenced after creation (the table may outlive the handle at thread exit)
    int device = 0;
    int capacity = 0, count = 0;
    DevBuf<orbm_point> d;            // the table
    std::vector<orbm_point> h;       // its host mirror: the exact host fallback of the search rebuilds the queries from it
    FrustumScratch s;                // what a search keeps between calls: the records k_frustum writes, host queries, level thresholds
};

int orbm_level_thresholds(float log_scale_factor, int n_levels, float* out) {
    MORB_ARG(n_levels >= 1 && n_levels <= ORBM_MAX_LEVELS && (n_levels == 1 || out));
    return build_thresholds(log_scale_factor, n_levels, out);
}

int orbm_frustum_host(const orbm_point* pts, int n, const orbm_view* view, const uint8_t* skip, orbm_track* track, orbm_query* q,
                      int* n_to_match) {
    MORB_ARG(n >= 0 && (n == 0 || pts) && view && view->n_levels >= 1 && view->n_levels <= ORBM_MAX_LEVELS && view->scale_factors);
    // the table of the calling thread's last (log_scale_factor, n_levels): built once, as the table object does for the device path
    static thread_local struct { float lsf; int levels; float thr[ORBM_MAX_LEVELS - 1]; } cache = {0.0f, 0, {0}};
    if (cache.levels != view->n_levels || memcmp(&cache.lsf, &view->log_scale_factor, 4) != 0) {
        cache.levels = 0;
        int rc = build_thresholds(view->log_scale_factor, view->n_levels, cache.thr);
        if (rc) return rc;
        cache.lsf = view->log_scale_factor; cache.levels = view->n_levels;
    }
    FrustumView V;
    make_view(view, cache.thr, V);
    frustum_host(V, pts, nullptr, n, skip, track, q, n_to_match);
    return ORB_OK;
}

int orbm_points_create(orbm_matcher* m, int capacity, orbm_points** out) {
    MORB_ARG(m && out && capacity >= 0);
    if (capacity > ORBM_MAX_POINTS) { morb::set_error("a point table holds at most %d points (asked for %d)", (int)ORBM_MAX_POINTS, capacity); return ORB_E_CAPACITY; }
    MORB_HIP(hipSetDevice(m->device));
    orbm_points* p = new orbm_points;
    p->owner = m; p->device = m->device; p->capacity = capacity;
    int rc;
    if ((rc = p->d.reserve((size_t)std::max(capacity, 1))) || (rc = p->s.h_track.reserve((size_t)std::max(capacity, 1)))) {
        p->d.release(); p->s.h_track.release(); delete p;
        return rc;
    }
    p->h.resize((size_t)capacity);
    if (capacity) memset(p->h.data(), 0, (size_t)capacity * sizeof(orbm_point));
    // rows never written read as zeros on both sides (the table's host mirror and HBM)
    if (hipMemsetAsync(p->d.p, 0, (size_t)std::max(capacity, 1) * sizeof(orbm_point), m->stream) != hipSuccess ||
        hipStreamSynchronize(m->stream) != hipSuccess) {
        morb::set_error("clearing the point table failed");
        p->d.release(); p->s.h_track.release(); delete p;
        return ORB_E_HIP;
    }
    *out = p;
    return ORB_OK;
}

void orbm_points_destroy(orbm_points* p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    p->d.release(); p->s.h_track.release();
    delete p;
}

int orbm_points_count(const orbm_points* p) { return p ? p->count : ORB_E_ARG; }

int morb::points_view(const orbm_points* p, const orbm_matcher* m, const orbm_point** d_rows, const orbm_point** h_rows, int* count) {
    MORB_ARG(p && m && p->owner == m);
    *d_rows = p->d.p; *h_rows = p->h.data(); *count = p->count;
    return ORB_OK;
}

int orbm_points_write(orbm_matcher* m, orbm_points* p, int first, int n, const orbm_point* src) {
    MORB_ARG(m && p && p->owner == m && first >= 0 && n >= 0 && (n == 0 || src));
    if ((long long)first + n > p->capacity) {
        morb::set_error("rows [%d, %d) do not fit a point table of %d", first, first + n, p->capacity); return ORB_E_CAPACITY;
    }
    if (n == 0) return ORB_OK;
    MORB_HIP(hipSetDevice(m->device));
    memcpy(p->h.data() + first, src, (size_t)n * sizeof(orbm_point));
    MORB_HIP(hipMemcpyAsync(p->d.p + first, p->h.data() + first, (size_t)n * sizeof(orbm_point), hipMemcpyHostToDevice, m->stream));
    MORB_HIP(hipStreamSynchronize(m->stream));
    p->count = std::max(p->count, first + n);
    return ORB_OK;
}

// The body both entries of the local-point search share: thresholds, k_frustum into the matcher's query buffer, project + resolve
// behind it, one synchronisation, the exact host route when the matcher asks for it or the resolve falls back.
int morb::search_local_points_body(orbm_matcher* m, const orbm_frame* cur, FrustumScratch& scr, const LocalPointSource& S, int n,
                                   const orbm_view* view, const uint8_t* occupied, float nnratio, int th_high, orbm_track* track,
                                   int32_t* match_of_feature, int* n_to_match, int* nmatches) {
    MORB_HIP(hipSetDevice(m->device));
    int rc;
    if ((rc = thresholds_of(scr, view))) return rc;
    FrustumView V;
    make_view(view, scr.thr, V);
    *n_to_match = 0; *nmatches = 0;
    const int nf = cur->n_total;
    if (n == 0) { for (int g = 0; g < nf; ++g) match_of_feature[g] = -1; return ORB_OK; }

    if ((rc = scr.h_track.reserve((size_t)n))) return rc;
    scr.hq.resize((size_t)n);
    FillCtx ctx{&V, &S, n, scr.hq.data()};
    // J.q: host records.  On the device path they are NOT written here -- nothing reads them unless the resolve falls back, and then
    // q_fill (below) writes them first.  Until then the buffer may hold an earlier call's records: do not read it here.
    SearchJob J{cur, scr.hq.data(), n, occupied, true, nnratio, th_high, 0, 64, false};
    if (m->host_resolve) {   // MORB_HOST_RESOLVE=1: everything from the host restatement, the search through host_resolve
        int cnt = 0;
        std::vector<uint8_t> store;
        const uint8_t* skip = host_skip_of(S, n, store);
        frustum_host(V, S.h_rows, S.h_index, n, skip, track, scr.hq.data(), &cnt);
        *n_to_match = cnt;
        if ((rc = search_enqueue(m, J))) return rc;
        return search_finish(m, J, match_of_feature, nmatches);
    }
    // skip flags and occupied flags through the host-written staging, read in place by the kernels
    const size_t sbytes = ((size_t)n + 255) & ~(size_t)255, obytes = occupied ? (size_t)nf : 0;
    if ((rc = m->stage_q.reserve(sbytes + obytes + 16)) || (rc = m->d_queries.reserve((size_t)n * sizeof(orbm_query)))) return rc;
    if (S.skip) memcpy(m->stage_q.p, S.skip, (size_t)n);
    if (occupied) memcpy(m->stage_q.p + sbytes, occupied, obytes);
    m->stage_q.publish();
    J.occ_dev = occupied ? m->stage_q.dp + sbytes : nullptr;
    J.q_fill = fill_queries; J.q_fill_ctx = &ctx;   // host records only if the resolve falls back
    const FrustumIndex X{S.d_index, S.d_mark, S.d_flags, S.epoch};
    if (S.d_index)
        hipLaunchKernelGGL(k_frustum<true>, dim3((n + 255) / 256), dim3(256), 0, m->stream, V, S.d_rows, (const uint8_t*)nullptr, n,
                           (orbm_query*)m->d_queries.p, scr.h_track.dp, X);
    else
        hipLaunchKernelGGL(k_frustum<false>, dim3((n + 255) / 256), dim3(256), 0, m->stream, V, S.d_rows,
                           S.skip ? (const uint8_t*)m->stage_q.dp : (const uint8_t*)nullptr, n, (orbm_query*)m->d_queries.p, scr.h_track.dp, X);
    MORB_HIP(hipGetLastError());
    if ((rc = search_enqueue(m, J, /*queries_already_on_device=*/true))) return rc;
    MORB_HIP(hipStreamSynchronize(m->stream));
    int cnt = 0;
    const orbm_track* T = scr.h_track.p;
    for (int i = 0; i < n; ++i) cnt += T[i].in_view;
    *n_to_match = cnt;
    if (track) memcpy(track, T, (size_t)n * sizeof(orbm_track));
    return search_finish(m, J, match_of_feature, nmatches);
}

int orbm_search_local_points(orbm_matcher* m, const orbm_frame* cur, const orbm_points* pts_c, int n, const orbm_view* view,
                             const uint8_t* skip, const uint8_t* occupied, float nnratio, int th_high, orbm_track* track,
                             int32_t* match_of_feature, int* n_to_match, int* nmatches) {
    orbm_points* pts = const_cast<orbm_points*>(pts_c);   // (scratch of the call lives in the table object)
    MORB_ARG(m && cur && pts && pts->owner == m && cur->owner == m && n >= 0 && view && n_to_match && nmatches &&
             (cur->n_total == 0 || match_of_feature));
    MORB_ARG(view->n_levels >= 1 && view->n_levels <= ORBM_MAX_LEVELS && view->scale_factors);
    if (n > pts->count) { morb::set_error("%d points asked for, %d written to the table", n, pts->count); return ORB_E_CAPACITY; }
    if (n > ORBM_MAX_POINTS) { morb::set_error("%d points are more than a search takes (%d)", n, (int)ORBM_MAX_POINTS); return ORB_E_CAPACITY; }
    LocalPointSource S{};
    S.d_rows = pts->d.p; S.h_rows = pts->h.data(); S.skip = skip;
    return morb::search_local_points_body(m, cur, pts->s, S, n, view, occupied, nnratio, th_high, track, match_of_feature, n_to_match, nmatches);
}
