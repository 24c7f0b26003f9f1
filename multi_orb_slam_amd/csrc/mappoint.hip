// mappoint.hip -- map-point refresh on the device (include/orbm.h, "map-point refresh"): MapPoint::ComputeDistinctiveDescriptors
// (reference src/MapPoint.cc:325-438) and MapPoint::UpdateNormalAndDepth (:480-528) for the points of a keyframe in one call.
//   k_refresh<G>     G lanes per point, 256 / G points per workgroup: G = 16 (four points per wavefront), 64 (a wavefront) and
//                    256 (the workgroup), chosen on the host by the point's observation count.  Lane l owns observation l.
//                    Descriptor job: the descriptors go to LDS, lane l computes row l of the distance matrix -- kept in LDS,
//                    transposed, for G <= 64; recomputed at every step for G = 256, where a 256 x 256 matrix has no room -- and
//                    finds the row's median as the smallest v in 0..256 with #{d <= v} > (N-1)/2 (nine bisection steps: an exact
//                    selection without a sort); the winner is the minimum of (median << 16) | l over the alive lanes.
//                    Normal / depth job: lane l computes the weighted unit vector of observation l (the f64 norm and reciprocal
//                    in parallel); lane 0 adds them up in list order, because the float sum is not associative.
//   refresh_*        the arithmetic itself, ONE statement sequence for the kernel and for the host routine
//                    (orbm_refresh_points_host; the in-call fallback for points beyond ORBM_REFRESH_CAP observations).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/orbm.h"
#include "orb_common.h"
#include "matcher_internal.h"
#include "cv_dev.h"
#include "hamming_dev.h"
#include "stage_pack.h"

using namespace morb;

namespace {

// cv::Mat normali = mWorldPos - Owi[cam]; normal = normal + normali/cv::norm(normali)   (src/MapPoint.cc:512-513)
// as host/cv_compat.h evaluates it: the difference in float; cv::norm = squares summed in double in component order, sqrt in
// double; `normali/norm` is a scaled-matrix expression with weight 1.0/norm, and the sum folds it into ONE cv::addWeighted
// with float weights: normal*1.0f + normali*(float)(1.0/norm) + 0.0f.  This computes normali*(float)(1.0/norm), the part that
// does not depend on the running sum.
__host__ __device__ inline void refresh_term(const float* pos, const float* centre, float* t) {
    float d[3];
    for (int k = 0; k < 3; ++k) d[k] = pos[k] - centre[k];
    const double nrm = cv_norm3(d);
    const float be = (float)(1.0 / nrm);
    for (int k = 0; k < 3; ++k) t[k] = d[k] * be;
}
// ... and the rest of that cv::addWeighted.  (The expression takes cv::add instead when the weight is exactly 1.0; the two give the
// same bits here: normal*1.0f is normal, and the one difference, -0 + -0, needs a running sum of -0, which `+ 0.0f` never leaves.)
__host__ __device__ inline void refresh_accumulate(float* normal, const float* t) {
    for (int k = 0; k < 3; ++k) normal[k] = normal[k] * 1.0f + t[k] + 0.0f;
}
// mNormalVector = normal/n: a scaled matrix with weight 1.0/n (cv_dev.h cv_scale); a NaN leaves as x86's (x86_nan).  const float dist = cv::norm(Pos - pRefKF->GetCameraCenter()); mfMaxDistance = dist*levelScaleFactor;
// mfMinDistance = mfMaxDistance/mvScaleFactors[nLevels-1]   (src/MapPoint.cc:517-527)
__host__ __device__ inline void refresh_finish(const float* sum, int n, const float* pos, const float* ref_centre, float level_scale,
                                               float top_scale, orbm_refresh_out& o) {
    const double inv = 1.0 / (double)n;
    for (int k = 0; k < 3; ++k) o.normal[k] = x86_nan(cv_scale(sum[k], inv));
    float d[3];
    for (int k = 0; k < 3; ++k) d[k] = pos[k] - ref_centre[k];
    const float dist = (float)cv_norm3(d);
    const float max_dist = dist * level_scale;
    o.max_dist = x86_nan(max_dist);
    o.min_dist = x86_nan(max_dist / top_scale);
}

struct RefreshDev {   // the packed inputs of a call as the kernels see them, and one class's worklist
    const int* first; const uint4* desc; const float* centre; const uint8_t* alive;
    const float* pos; const float* ref_centre; const int* ref_level; const uint8_t* what;
    const int* list; int count;   // points of this class; record w of `out` belongs to point list[w]
    orbm_refresh_out* out;
    int n_levels;
    float scale[ORBM_MAX_LEVELS];
};

// No thread leaves early: the barriers and the lane exchanges below are reached by all 256.  A slot without a point, a lane without
// an observation and a job that was not asked for carry n = 0 / zeros through the same statements.
template <int G>
__global__ __launch_bounds__(256) void k_refresh(RefreshDev A) {
    constexpr int PPB = 256 / G;                       // points per workgroup
    constexpr bool ROWS = G <= 64;                     // the distance rows fit LDS
    constexpr int RSTRIDE = G * G + (G == 16 ? 16 : 0);   // u16 per point; the pad puts a wavefront's four 16-lane groups on different banks
    __shared__ uint4 s_desc[512];                      // descriptor of thread t at [2t], [2t+1]
    __shared__ float s_term[768];                      // weighted unit vector of thread t at [3t .. 3t+2]
    __shared__ unsigned long long s_alive[4];          // per wavefront: which lanes hold an alive observation
    __shared__ unsigned s_min[4];
    __shared__ uint16_t s_row[ROWS ? PPB * RSTRIDE : 1];   // [point][j][l]: lane l reads its row with stride G, neighbours side by side

    const int tid = threadIdx.x, l = tid % G, slot = tid / G, base = slot * G;
    const int w = blockIdx.x * PPB + slot;
    const bool have = w < A.count;
    int pt = 0, o0 = 0, n = 0;
    unsigned what = 0;
    if (have) {
        pt = A.list[w];
        o0 = A.first[pt];
        n = min(A.first[pt + 1] - o0, G);              // (the host hands a point to a class that holds it; never beyond the group)
        what = A.what[pt];
    }
    const bool job_desc = (what & ORBM_REFRESH_DESCRIPTOR) != 0, job_normal = (what & ORBM_REFRESH_NORMAL_DEPTH) != 0;
    uint4 d0 = make_uint4(0, 0, 0, 0), d1 = d0;
    bool alive = false;
    float t[3] = {0.0f, 0.0f, 0.0f};
    if (l < n) {
        if (job_desc) {
            alive = A.alive[o0 + l] != 0;
            d0 = A.desc[2 * (size_t)(o0 + l)]; d1 = A.desc[2 * (size_t)(o0 + l) + 1];
        }
        if (job_normal) refresh_term(A.pos + 3 * (size_t)pt, A.centre + 3 * (size_t)(o0 + l), t);
    }
    s_desc[2 * tid] = d0; s_desc[2 * tid + 1] = d1;
    for (int k = 0; k < 3; ++k) s_term[3 * tid + k] = t[k];
    const unsigned long long ballot = __ballot(alive);
    if ((tid & 63) == 0) s_alive[tid >> 6] = ballot;
    __syncthreads();

    auto alive_at = [&](int j) -> bool { const int g = base + j; return ((s_alive[g >> 6] >> (g & 63)) & 1ull) != 0; };
    unsigned key = 0xffffffffu;
    if (alive) {
        int N = 0;
        for (int j = 0; j < n; ++j) N += alive_at(j) ? 1 : 0;
        const int rank = (N - 1) / 2;                  // (int)(0.5*(N-1)), N >= 1 here
        if (ROWS) {
            uint16_t* row = s_row + slot * RSTRIDE + l;
            for (int j = 0; j < n; ++j)
                row[j * G] = alive_at(j) ? (uint16_t)ham256(d0, d1, s_desc[2 * (base + j)], s_desc[2 * (base + j) + 1]) : (uint16_t)0xffff;
        }
        int lo = 0, hi = 256;                          // the median is the smallest v with more than `rank` distances <= v
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            int c = 0;
            if (ROWS) {
                const uint16_t* row = s_row + slot * RSTRIDE + l;
                for (int j = 0; j < n; ++j) c += ((int)row[j * G] <= mid) ? 1 : 0;   // (a dead column holds 0xffff)
            } else {
                for (int j = 0; j < n; ++j)
                    c += (alive_at(j) && ham256(d0, d1, s_desc[2 * (base + j)], s_desc[2 * (base + j) + 1]) <= mid) ? 1 : 0;
            }
            if (c > rank) hi = mid; else lo = mid + 1;
        }
        key = ((unsigned)lo << 16) | (unsigned)l;
    }
    // the first row with the least median: minimum of the keys over the point's lanes
    for (int off = (G < 64 ? G : 64) / 2; off > 0; off >>= 1) key = min(key, (unsigned)__shfl_xor((int)key, off, 64));
    if (G > 64) {
        if ((tid & 63) == 0) s_min[tid >> 6] = key;
        __syncthreads();
        key = min(min(s_min[0], s_min[1]), min(s_min[2], s_min[3]));
    }

    if (have && l == 0) {
        orbm_refresh_out o;
        memset(&o, 0, sizeof(o));
        if (job_desc) {
            if (key != 0xffffffffu) {
                const int best = (int)(key & 0xffffu);
                o.best_obs = best; o.best_median = (int)(key >> 16);
                const uint4 b0 = s_desc[2 * (base + best)], b1 = s_desc[2 * (base + best) + 1];
                memcpy(o.desc, &b0, 16); memcpy(o.desc + 16, &b1, 16);
            } else {
                o.best_obs = -1;
            }
        }
        if (job_normal && n > 0) {
            float sum[3] = {0.0f, 0.0f, 0.0f};
            for (int j = 0; j < n; ++j) refresh_accumulate(sum, s_term + 3 * (base + j));
            int level = A.ref_level[pt];
            level = min(max(level, 0), A.n_levels - 1);   // (validated on the host; the table is never indexed beyond its end)
            refresh_finish(sum, n, A.pos + 3 * (size_t)pt, A.ref_centre + 3 * (size_t)pt, A.scale[level], A.scale[A.n_levels - 1], o);
        }
        A.out[w] = o;
    }
}

// ---- host routine ------------------------------------------------------------------------------------------------------------
int popcount256(const uint8_t* a, const uint8_t* b) {
    int dist = 0;
    for (int i = 0; i < 4; i++) {
        uint64_t x, y;
        memcpy(&x, a + 8 * i, 8); memcpy(&y, b + 8 * i, 8);
        dist += __builtin_popcountll(x ^ y);
    }
    return dist;
}

struct HostScratch { std::vector<int> idx; std::vector<uint16_t> dist; };

void refresh_point_host(const orbm_refresh_in& in, int pt, HostScratch& S, orbm_refresh_out& o) {
    memset(&o, 0, sizeof(o));
    const int o0 = in.first[pt], n = in.first[pt + 1] - o0;
    const unsigned what = in.what[pt];
    if (what & ORBM_REFRESH_DESCRIPTOR) {
        S.idx.clear();
        for (int j = 0; j < n; ++j) if (in.obs_alive[o0 + j]) S.idx.push_back(j);
        const int N = (int)S.idx.size();
        o.best_obs = -1;
        if (N > 0) {
            S.dist.assign((size_t)N * N, 0);
            for (int i = 0; i < N; ++i)
                for (int j = i + 1; j < N; ++j) {
                    const int d = popcount256(in.obs_desc + 32 * (size_t)(o0 + S.idx[i]), in.obs_desc + 32 * (size_t)(o0 + S.idx[j]));
                    S.dist[(size_t)i * N + j] = (uint16_t)d; S.dist[(size_t)j * N + i] = (uint16_t)d;
                }
            const int rank = (int)(0.5 * (N - 1));
            int best_median = INT32_MAX, best = 0;
            for (int i = 0; i < N; ++i) {
                int hist[257] = {0};                   // the rank-th element of the sorted row, without the sort
                for (int j = 0; j < N; ++j) hist[S.dist[(size_t)i * N + j]]++;
                int v = 0, c = hist[0];
                while (c <= rank) c += hist[++v];
                if (v < best_median) { best_median = v; best = i; }
            }
            o.best_obs = S.idx[best]; o.best_median = best_median;
            memcpy(o.desc, in.obs_desc + 32 * (size_t)(o0 + S.idx[best]), 32);
        }
    }
    if ((what & ORBM_REFRESH_NORMAL_DEPTH) && n > 0) {
        float sum[3] = {0.0f, 0.0f, 0.0f}, t[3];
        for (int j = 0; j < n; ++j) {
            refresh_term(in.pos + 3 * (size_t)pt, in.obs_centre + 3 * (size_t)(o0 + j), t);
            refresh_accumulate(sum, t);
        }
        refresh_finish(sum, n, in.pos + 3 * (size_t)pt, in.ref_centre + 3 * (size_t)pt, in.scale_factors[in.ref_level[pt]],
                       in.scale_factors[in.n_levels - 1], o);
    }
}

int validate(const orbm_refresh_in* in, const orbm_refresh_out* out) {
    MORB_ARG(in && in->n_points >= 0 && in->n_obs >= 0 && in->first && (in->n_points == 0 || (out && in->what)));
    MORB_ARG(in->n_obs == 0 || (in->obs_desc && in->obs_centre && in->obs_alive));
    if (const int rc = validate_first(in->n_points, in->first, "point")) return rc;
    MORB_ARG(in->first[in->n_points] == in->n_obs);
    bool normals = false;
    for (int p = 0; p < in->n_points; ++p) {
        if (in->what[p] & ~(ORBM_REFRESH_DESCRIPTOR | ORBM_REFRESH_NORMAL_DEPTH)) { morb::set_error("what[%d] = %d has unknown bits", p, (int)in->what[p]); return ORB_E_ARG; }
        normals = normals || ((in->what[p] & ORBM_REFRESH_NORMAL_DEPTH) && in->first[p + 1] > in->first[p]);
    }
    if (!normals) return ORB_OK;
    MORB_ARG(in->pos && in->ref_centre && in->ref_level && in->scale_factors && in->n_levels >= 1 && in->n_levels <= ORBM_MAX_LEVELS);
    for (int p = 0; p < in->n_points; ++p)
        if ((in->what[p] & ORBM_REFRESH_NORMAL_DEPTH) && in->first[p + 1] > in->first[p] && (in->ref_level[p] < 0 || in->ref_level[p] >= in->n_levels)) {
            morb::set_error("ref_level[%d] = %d is outside the %d levels", p, in->ref_level[p], in->n_levels); return ORB_E_ARG;
        }
    return ORB_OK;
}

}  // namespace

int orbm_refresh_points_host(const orbm_refresh_in* in, orbm_refresh_out* out) {
    int rc = validate(in, out);
    if (rc) return rc;
    HostScratch S;
    for (int p = 0; p < in->n_points; ++p) refresh_point_host(*in, p, S, out[p]);
    return ORB_OK;
}

int orbm_refresh_points(orbm_matcher* m, const orbm_refresh_in* in, orbm_refresh_out* out) {
    MORB_ARG(m != nullptr);
    int rc = validate(in, out);
    if (rc) return rc;
    const int P = in->n_points, NO = in->n_obs;
    // worklist, sorted by size class so that one long point does not hold a wavefront of short ones: [16-lane | wavefront | workgroup]
    int cnt[5] = {0, 0, 0, 0, 0};   // small, wave, block, host (beyond the cap), nothing to do
    auto class_of = [&](int p) {
        const int n = in->first[p + 1] - in->first[p];
        if (n == 0 || in->what[p] == 0) return 4;
        return n <= 16 ? 0 : n <= 64 ? 1 : n <= ORBM_REFRESH_CAP ? 2 : 3;
    };
    for (int p = 0; p < P; ++p) cnt[class_of(p)]++;
    const int n_dev = cnt[0] + cnt[1] + cnt[2];
    std::vector<int32_t>& list = m->refresh_list;
    list.resize((size_t)std::max(n_dev, 1));
    int at[3] = {0, cnt[0], cnt[0] + cnt[1]};
    const int start[3] = {at[0], at[1], at[2]};
    for (int p = 0; p < P; ++p) { const int c = class_of(p); if (c < 3) list[at[c]++] = p; }

    if (n_dev > 0) {
        MORB_HIP(hipSetDevice(m->device));
        // one packed block: every array 16-byte aligned, written once by the host, read in place by the kernels
        morb::StagePack pk;
        const int i_first = pk.add(in->first, (size_t)(P + 1) * 4), i_desc = pk.add(in->obs_desc, (size_t)NO * 32),
                  i_centre = pk.add(in->obs_centre, (size_t)NO * 12), i_alive = pk.add(in->obs_alive, (size_t)NO),
                  // (the per-point arrays of the normal / depth job may be absent when no point asks for it: zeros then, never read)
                  i_pos = pk.add_or_zeros(in->pos, (size_t)P * 12), i_ref = pk.add_or_zeros(in->ref_centre, (size_t)P * 12),
                  i_level = pk.add_or_zeros(in->ref_level, (size_t)P * 4),
                  i_what = pk.add(in->what, (size_t)P), i_list = pk.add(list.data(), (size_t)n_dev * 4);
        const morb::StagePack::Block blk = pk.open(m->refresh.stage, &rc);
        if (rc || (rc = m->refresh.out.reserve((size_t)n_dev))) return rc;
        blk.publish();
        RefreshDev A;
        A.first = blk.dev<int>(i_first); A.desc = blk.dev<uint4>(i_desc); A.centre = blk.dev<float>(i_centre);
        A.alive = blk.dev<uint8_t>(i_alive); A.pos = blk.dev<float>(i_pos); A.ref_centre = blk.dev<float>(i_ref);
        A.ref_level = blk.dev<int>(i_level); A.what = blk.dev<uint8_t>(i_what);
        const bool levels = in->scale_factors && in->n_levels >= 1 && in->n_levels <= ORBM_MAX_LEVELS;
        A.n_levels = levels ? in->n_levels : 1;
        for (int k = 0; k < ORBM_MAX_LEVELS; ++k) A.scale[k] = levels && k < in->n_levels ? in->scale_factors[k] : 0.0f;
        for (int c = 0; c < 3; ++c) {
            if (!cnt[c]) continue;
            A.list = blk.dev<int>(i_list) + start[c]; A.count = cnt[c]; A.out = m->refresh.out.dp + start[c];
            if (c == 0) hipLaunchKernelGGL(k_refresh<16>, dim3((cnt[c] + 15) / 16), dim3(256), 0, m->stream, A);
            else if (c == 1) hipLaunchKernelGGL(k_refresh<64>, dim3((cnt[c] + 3) / 4), dim3(256), 0, m->stream, A);
            else hipLaunchKernelGGL(k_refresh<256>, dim3(cnt[c]), dim3(256), 0, m->stream, A);
            MORB_HIP(hipGetLastError());
        }
    }
    // while the kernels run: the points the device does not take
    HostScratch S;
    for (int p = 0; p < P; ++p) {
        const int c = class_of(p);
        if (c == 3) refresh_point_host(*in, p, S, out[p]);
        else if (c == 4) { memset(&out[p], 0, sizeof(out[p])); if (in->what[p] & ORBM_REFRESH_DESCRIPTOR) out[p].best_obs = -1; }
    }
    if (n_dev > 0) {
        MORB_HIP(hipStreamSynchronize(m->stream));
        const orbm_refresh_out* R = m->refresh.out.p;
        for (int w = 0; w < n_dev; ++w) out[list[w]] = R[w];
    }
    for (int k = 0; k < 5; ++k) m->last_refresh[k] = cnt[k];
    return ORB_OK;
}
