// localmap.hip -- the local map on the device (include/orbm.h, "the local map on the device"): a map resident in HBM under stable
// slots (one per map point, one per keyframe, one per observation) and Tracking::UpdateLocalMap's data-parallel parts over it
// (reference src/Tracking.cc:1794-1949):
//   orbm_map_vote                 keyframeCounter of UpdateLocalKeyFrames (:1838-1855): k_map_mult, k_map_vote, k_map_vote_out
//   orbm_map_local_points         UpdateLocalPoints (:1794-1824): k_map_first, k_map_count, k_map_scan, k_map_scatter
//   orbm_map_search_local_points  k_map_mark, then the body orbm_search_local_points runs (frustum.hip), reading rows[list[i]]
// and the two counting routines of the LocalMapping / LoopClosing threads over the same map:
//   orbm_map_covisibility         KFcounter / KFcounter_cam1 of KeyFrame::UpdateConnections (src/KeyFrame.cc:512-552): k_map_covis
//   orbm_map_culling_counts       nMPs / nRedundantObservations of LocalMapping::KeyFrameCulling (src/LocalMapping.cc:990-1032): k_map_cull
//   both read the chain from a point to its live records, which k_map_chain builds when a record write has made it stale
// and the two passes of LoopClosing that move map points, in place over the same map (kernels: mapcorrect_dev.h):
//   orbm_map_correct_sim3         CorrectLoop's step 4.2 (src/LoopClosing.cc:678-710): the ordered claim above, then k_map_correct_sim3
//   orbm_map_correct_rigid        the update after global BA (:953-989): k_map_stamp_last, k_map_correct_rigid
// The kernels are in localmap_dev.h.  The two host routines (orbm_local_map_vote_host, orbm_local_map_points_host) are the
// reference's loops on plain arrays: the fallback under MORB_HOST_RESOLVE=1, over the mirror, and the cross-check of the tests.
// K1, K2 and the marks are pointer logic over the covisibility graph and stay with the caller (host/LocalMap.cc).
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

#include "../../include/orbm.h"
#include "../../include/orb_debug.h"
#include "orb_common.h"
#include "matcher_internal.h"
#include "localmap_dev.h"
#include "mapcorrect_dev.h"

using namespace morb;

struct orbm_map {
    orbm_matcher* owner = nullptr;   // compared, never dereferenced after creation
    int device = 0;
    int kf_cap = 0, pt_cap = 0, obs_cap = 0, stride = 0;
    int kf_hw = 0, obs_hw = 0;       // high-water marks: one past the last keyframe / record slot in use
    // the map in HBM ...
    DevBuf<orbm_point> d_rows; DevBuf<uint8_t> d_flags; DevBuf<orbm_obs> d_obs; DevBuf<int32_t> d_kf_rows, d_kf_count;
    // ... and its host mirror
    std::vector<orbm_point> h_rows; std::vector<uint8_t> h_flags; std::vector<orbm_obs> h_obs;
    std::vector<int32_t> h_kf_rows, h_kf_count; std::vector<uint8_t> h_kf_bad;
    // per-point scratch that stays clean between calls: the frame's multiplicity (zero), the least candidate key and the skip mark
    // (both carry the epoch of the call that wrote them)
    DevBuf<int32_t> d_mult; DevBuf<unsigned long long> d_first; DevBuf<uint32_t> d_mark;
    std::vector<uint32_t> h_mark;    // host twin of d_mark (fallback only)
    uint32_t epoch = 0;
    DevBuf<int32_t> d_votes, d_block, d_list, d_total;
    PinnedBuf<int32_t> h_votes, h_list, h_total;   // what the kernels write for the host: mapped pinned
    StageBuf stage;                  // the host-written inputs of a call
    std::vector<int32_t> list;       // the last point list (host copy; the search's fallback reads it)
    int list_n = -1;                 // -1: no list
    FrustumScratch scr;
    int last[4] = {0, 0, 0, 0};
    // covisibility and culling: the record's feature, the feature bytes and camera-1 count of a keyframe, the point's n_obs ...
    DevBuf<int32_t> d_obs_feat, d_nobs, d_kf_ncam1; DevBuf<uint8_t> d_kf_feat;
    std::vector<int32_t> h_obs_feat, h_nobs, h_kf_ncam1; std::vector<uint8_t> h_kf_feat;
    // ... and the chain from a point to its live records, stale after any record write
    DevBuf<int32_t> d_head, d_next, d_cursor;
    bool index_dirty = false;
    PinnedBuf<int32_t> h_span, h_counts; PinnedBuf<orbm_covis_entry> h_entries;
    int last_cov[4] = {0, 0, 0, 0};
    // loop correction: the point's reference keyframe slot (-1: never written), the point high-water mark, the kept entries of a Sim3
    // correction and what either correction leaves for the host (mapped)
    DevBuf<int32_t> d_ref; std::vector<int32_t> h_ref;
    int pt_hw = 0;
    DevBuf<orbm_correct_entry> d_centries;
    PinnedBuf<orbm_correct_entry> h_centries; PinnedBuf<float> h_cpos; PinnedBuf<uint8_t> h_cstatus;
    std::vector<uint32_t> h_seen; uint32_t seen_epoch = 0;   // a listed slot of this call (host; the check that the slots are distinct)
    int last_cor[4] = {0, 0, 0, 0};
};

namespace {

void release_all(orbm_map* p) {
    p->d_rows.release(); p->d_flags.release(); p->d_obs.release(); p->d_kf_rows.release(); p->d_kf_count.release();
    p->d_mult.release(); p->d_first.release(); p->d_mark.release(); p->d_votes.release(); p->d_block.release(); p->d_list.release();
    p->d_obs_feat.release(); p->d_nobs.release(); p->d_kf_ncam1.release(); p->d_kf_feat.release(); p->d_head.release(); p->d_next.release();
    p->d_ref.release(); p->d_centries.release(); p->h_centries.release(); p->h_cpos.release(); p->h_cstatus.release();
    p->d_cursor.release(); p->h_span.release(); p->h_counts.release(); p->h_entries.release();
    p->d_total.release(); p->h_votes.release(); p->h_list.release(); p->h_total.release(); p->stage.release(); p->scr.h_track.release();
}

// A new epoch for the keys of k_map_first and the marks of k_map_mark; the arrays are cleared when the counter would wrap.
int next_epoch(orbm_matcher* m, orbm_map* p) {
    if (p->epoch >= 0xfffffff0u) {
        MORB_HIP(hipMemsetAsync(p->d_first.p, 0xff, (size_t)std::max(p->pt_cap, 1) * sizeof(unsigned long long), m->stream));
        MORB_HIP(hipMemsetAsync(p->d_mark.p, 0, (size_t)std::max(p->pt_cap, 1) * sizeof(uint32_t), m->stream));
        std::fill(p->h_mark.begin(), p->h_mark.end(), 0u);
        p->epoch = 0;
    }
    ++p->epoch;
    return ORB_OK;
}

int check_slots(const int32_t* s, int n, int lo, int cap, const char* what) {
    for (int i = 0; i < n; ++i)
        if (s[i] < lo || s[i] >= cap) { morb::set_error("%s %d (entry %d) is outside [%d, %d)", what, s[i], i, lo, cap); return s[i] < lo ? ORB_E_ARG : ORB_E_CAPACITY; }
    return ORB_OK;
}

inline unsigned blocks_of(long long n) { return (unsigned)((n + MAP_BLOCK - 1) / MAP_BLOCK); }

}  // namespace

int orbm_local_map_vote_host(const orbm_obs* obs, int n_obs, const uint8_t* point_flags, int n_points, const int32_t* frame_points,
                             int n_features, int n_kfs, int32_t* votes) {
    MORB_ARG(n_obs >= 0 && (n_obs == 0 || obs) && n_points >= 0 && (n_points == 0 || point_flags) && n_features >= 0 &&
             (n_features == 0 || frame_points) && n_kfs >= 0 && (n_kfs == 0 || votes));
    std::vector<int32_t> mult((size_t)n_points, 0);
    for (int f = 0; f < n_features; ++f) {
        const int p = frame_points[f];
        if (p < 0) continue;
        MORB_ARG(p < n_points);
        if (!(point_flags[p] & ORBM_POINT_BAD)) ++mult[p];
    }
    for (int k = 0; k < n_kfs; ++k) votes[k] = 0;
    for (int i = 0; i < n_obs; ++i) {
        if (obs[i].point < 0) continue;
        MORB_ARG(obs[i].point < n_points && obs[i].keyframe >= 0 && obs[i].keyframe < n_kfs);
        votes[obs[i].keyframe] += mult[obs[i].point];
    }
    return ORB_OK;
}

int orbm_local_map_points_host(const int32_t* kf_rows, const int32_t* kf_count, int n_kfs, int stride, const uint8_t* point_flags,
                               int n_points, const int32_t* local_kfs, int n_local, int32_t* list, int list_cap, int* n_list) {
    MORB_ARG(n_kfs >= 0 && stride >= 1 && (n_kfs == 0 || (kf_rows && kf_count)) && n_points >= 0 && (n_points == 0 || point_flags) &&
             n_local >= 0 && (n_local == 0 || local_kfs) && list_cap >= 0 && (list_cap == 0 || list) && n_list);
    std::vector<uint8_t> marked((size_t)n_points, 0);   // mnTrackReferenceForFrame == mCurrentFrame.mnId
    int n = 0;
    for (int j = 0; j < n_local; ++j) {
        const int kf = local_kfs[j];
        MORB_ARG(kf >= 0 && kf < n_kfs && kf_count[kf] >= 0 && kf_count[kf] <= stride);
        for (int f = 0; f < kf_count[kf]; ++f) {
            const int s = kf_rows[(size_t)kf * stride + f];
            if (s < 0) continue;
            MORB_ARG(s < n_points);
            if (marked[s]) continue;
            if (point_flags[s] & ORBM_POINT_BAD) continue;
            if (n < list_cap) list[n] = s;
            ++n;
            marked[s] = 1;
        }
    }
    *n_list = n;
    if (n > list_cap) { morb::set_error("%d local points are more than the list takes (%d)", n, list_cap); return ORB_E_CAPACITY; }
    return ORB_OK;
}

int orbm_map_create(orbm_matcher* m, int kf_capacity, int point_capacity, int obs_capacity, int features_per_keyframe, orbm_map** out) {
    MORB_ARG(m && out && kf_capacity >= 1 && point_capacity >= 0 && obs_capacity >= 0 && features_per_keyframe >= 1);
    if (kf_capacity > ORBM_MAP_MAX_KEYFRAMES || features_per_keyframe > ORBM_MAP_MAX_FEATURES) {
        morb::set_error("a resident map holds at most %d keyframes of %d features (asked for %d of %d)", (int)ORBM_MAP_MAX_KEYFRAMES,
                        (int)ORBM_MAP_MAX_FEATURES, kf_capacity, features_per_keyframe);
        return ORB_E_CAPACITY;
    }
    MORB_HIP(hipSetDevice(m->device));
    orbm_map* p = new orbm_map;
    p->owner = m; p->device = m->device;
    p->kf_cap = kf_capacity; p->pt_cap = point_capacity; p->obs_cap = obs_capacity; p->stride = features_per_keyframe;
    const size_t np = (size_t)std::max(point_capacity, 1), no = (size_t)std::max(obs_capacity, 1);
    const size_t nk = (size_t)kf_capacity, nr = nk * (size_t)features_per_keyframe;
    int rc;
    if ((rc = p->d_rows.reserve(np)) || (rc = p->d_flags.reserve(np)) || (rc = p->d_obs.reserve(no)) || (rc = p->d_kf_rows.reserve(nr)) ||
        (rc = p->d_kf_count.reserve(nk)) || (rc = p->d_mult.reserve(np)) || (rc = p->d_first.reserve(np)) || (rc = p->d_mark.reserve(np)) ||
        (rc = p->d_votes.reserve(nk)) || (rc = p->d_list.reserve(ORBM_MAX_POINTS)) || (rc = p->d_total.reserve(4)) ||
        (rc = p->h_votes.reserve(nk)) || (rc = p->h_list.reserve(ORBM_MAX_POINTS)) || (rc = p->h_total.reserve(4)) ||
        (rc = p->d_obs_feat.reserve(no)) || (rc = p->d_nobs.reserve(np)) || (rc = p->d_kf_ncam1.reserve(nk)) || (rc = p->d_kf_feat.reserve(nr)) ||
        (rc = p->d_head.reserve(np)) || (rc = p->d_next.reserve(no)) || (rc = p->d_cursor.reserve(1)) ||
        (rc = p->d_ref.reserve(np))) {
        release_all(p); delete p;
        return rc;
    }
    // empty on both sides: rows of zeros that are not bad, free records, keyframes without points, clean scratch
    hipStream_t st = m->stream;
    if (hipMemsetAsync(p->d_rows.p, 0, np * sizeof(orbm_point), st) != hipSuccess || hipMemsetAsync(p->d_flags.p, 0, np, st) != hipSuccess ||
        hipMemsetAsync(p->d_obs.p, 0xff, no * sizeof(orbm_obs), st) != hipSuccess ||
        hipMemsetAsync(p->d_kf_rows.p, 0xff, nr * sizeof(int32_t), st) != hipSuccess ||
        hipMemsetAsync(p->d_kf_count.p, 0, nk * sizeof(int32_t), st) != hipSuccess ||
        hipMemsetAsync(p->d_mult.p, 0, np * sizeof(int32_t), st) != hipSuccess ||
        hipMemsetAsync(p->d_first.p, 0xff, np * sizeof(unsigned long long), st) != hipSuccess ||
        hipMemsetAsync(p->d_mark.p, 0, np * sizeof(uint32_t), st) != hipSuccess ||
        hipMemsetAsync(p->d_obs_feat.p, 0, no * sizeof(int32_t), st) != hipSuccess || hipMemsetAsync(p->d_nobs.p, 0, np * sizeof(int32_t), st) != hipSuccess ||
        hipMemsetAsync(p->d_kf_ncam1.p, 0, nk * sizeof(int32_t), st) != hipSuccess || hipMemsetAsync(p->d_kf_feat.p, 0, nr, st) != hipSuccess ||
        hipMemsetAsync(p->d_head.p, 0xff, np * sizeof(int32_t), st) != hipSuccess ||
        hipMemsetAsync(p->d_ref.p, 0xff, np * sizeof(int32_t), st) != hipSuccess ||
        hipMemsetAsync(p->d_next.p, 0xff, no * sizeof(int32_t), st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        morb::set_error("clearing the resident map failed");
        release_all(p); delete p;
        return ORB_E_HIP;
    }
    orbm_point zero; memset(&zero, 0, sizeof(zero));
    p->h_rows.assign((size_t)point_capacity, zero); p->h_flags.assign((size_t)point_capacity, 0);
    p->h_obs.assign((size_t)obs_capacity, orbm_obs{-1, -1});
    p->h_kf_rows.assign(nr, -1); p->h_kf_count.assign(nk, 0); p->h_kf_bad.assign(nk, 0);
    p->h_mark.assign((size_t)point_capacity, 0u);
    p->h_obs_feat.assign((size_t)obs_capacity, 0); p->h_nobs.assign((size_t)point_capacity, 0); p->h_kf_ncam1.assign(nk, 0); p->h_kf_feat.assign(nr, 0);
    p->h_ref.assign((size_t)point_capacity, -1);
    *out = p;
    return ORB_OK;
}

void orbm_map_destroy(orbm_map* p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    release_all(p);
    delete p;
}

int orbm_map_keyframes(const orbm_map* p) { return p ? p->kf_hw : ORB_E_ARG; }

int orbm_map_keyframe_bad(const orbm_map* p, int kf) {
    MORB_ARG(p && kf >= 0 && kf < p->kf_cap);
    return p->h_kf_bad[(size_t)kf];
}

int orbm_debug_last_local_map(const orbm_map* p, int* out4) {
    MORB_ARG(p && out4);
    for (int k = 0; k < 4; ++k) out4[k] = p->last[k];
    return ORB_OK;
}

int orbm_map_write_points(orbm_matcher* m, orbm_map* p, const int32_t* slots, int n, const orbm_point* rows, const uint8_t* flags) {
    MORB_ARG(m && p && p->owner == m && n >= 0 && (n == 0 || (slots && rows)));
    int rc;
    if ((rc = check_slots(slots, n, 0, p->pt_cap, "point slot"))) return rc;
    if (n == 0) return ORB_OK;
    MORB_HIP(hipSetDevice(m->device));
    static_assert(sizeof(orbm_point) == 68, "orbm_point is 17 words");
    const size_t off_rows = (size_t)n * 4, off_flags = off_rows + (size_t)n * sizeof(orbm_point);
    if ((rc = p->stage.reserve(off_flags + (size_t)n + 16))) return rc;
    for (int i = 0; i < n; ++i) {
        p->h_rows[(size_t)slots[i]] = rows[i]; p->h_flags[(size_t)slots[i]] = flags ? flags[i] : 0;
        p->pt_hw = std::max(p->pt_hw, slots[i] + 1);
    }
    // staged from the mirror: a slot named twice is staged twice with its last entry, so the order of the lanes does not matter
    memcpy(p->stage.p, slots, (size_t)n * 4);
    for (int i = 0; i < n; ++i) {
        memcpy(p->stage.p + off_rows + (size_t)i * sizeof(orbm_point), &p->h_rows[(size_t)slots[i]], sizeof(orbm_point));
        p->stage.p[off_flags + (size_t)i] = p->h_flags[(size_t)slots[i]];
    }
    p->stage.publish();
    const int words = (int)(sizeof(orbm_point) / 4);
    hipLaunchKernelGGL(k_map_put_words, dim3(blocks_of((long long)n * words)), dim3(MAP_BLOCK), 0, m->stream,
                       (const uint32_t*)(p->stage.dp + off_rows), (const int32_t*)p->stage.dp, n, words, (uint32_t*)p->d_rows.p);
    hipLaunchKernelGGL(k_map_put_flags, dim3(blocks_of(n)), dim3(MAP_BLOCK), 0, m->stream, (const uint8_t*)(p->stage.dp + off_flags),
                       (const int32_t*)p->stage.dp, n, p->d_flags.p);
    MORB_HIP(hipGetLastError());
    MORB_HIP(hipStreamSynchronize(m->stream));
    return ORB_OK;
}

int orbm_map_write_observations(orbm_matcher* m, orbm_map* p, const int32_t* slots, int n, const orbm_obs* records) {
    MORB_ARG(m && p && p->owner == m && n >= 0 && (n == 0 || (slots && records)));
    int rc;
    if ((rc = check_slots(slots, n, 0, p->obs_cap, "record slot"))) return rc;
    for (int i = 0; i < n; ++i) {
        if (records[i].point < 0) continue;
        if (records[i].point >= p->pt_cap || records[i].keyframe < 0 || records[i].keyframe >= p->kf_cap) {
            morb::set_error("record %d names point %d, keyframe %d: outside the map (%d points, %d keyframes)", i, records[i].point,
                            records[i].keyframe, p->pt_cap, p->kf_cap);
            return ORB_E_CAPACITY;
        }
    }
    if (n == 0) return ORB_OK;
    MORB_HIP(hipSetDevice(m->device));
    const size_t off_rec = (size_t)n * 4;
    if ((rc = p->stage.reserve(off_rec + (size_t)n * sizeof(orbm_obs) + 16))) return rc;
    for (int i = 0; i < n; ++i) {
        orbm_obs r = records[i];
        if (r.point < 0) { r.point = -1; r.keyframe = -1; }   // one form of a free record
        else p->kf_hw = std::max(p->kf_hw, r.keyframe + 1);
        p->h_obs[(size_t)slots[i]] = r;
        p->obs_hw = std::max(p->obs_hw, slots[i] + 1);
    }
    p->index_dirty = true;   // the chain from a point to its records is rebuilt by the next counting call
    memcpy(p->stage.p, slots, (size_t)n * 4);
    for (int i = 0; i < n; ++i) memcpy(p->stage.p + off_rec + (size_t)i * sizeof(orbm_obs), &p->h_obs[(size_t)slots[i]], sizeof(orbm_obs));
    p->stage.publish();
    hipLaunchKernelGGL(k_map_put_words, dim3(blocks_of((long long)n * 2)), dim3(MAP_BLOCK), 0, m->stream,
                       (const uint32_t*)(p->stage.dp + off_rec), (const int32_t*)p->stage.dp, n, 2, (uint32_t*)p->d_obs.p);
    MORB_HIP(hipGetLastError());
    MORB_HIP(hipStreamSynchronize(m->stream));
    return ORB_OK;
}

int orbm_map_write_keyframe(orbm_matcher* m, orbm_map* p, int kf, const int32_t* point_of_feature, int n_features, int bad) {
    MORB_ARG(m && p && p->owner == m && n_features >= 0 && (n_features == 0 || point_of_feature));
    if (kf < 0 || kf >= p->kf_cap || n_features > p->stride) {
        morb::set_error("keyframe slot %d with %d features does not fit a map of %d keyframes of %d", kf, n_features, p->kf_cap, p->stride);
        return kf < 0 ? ORB_E_ARG : ORB_E_CAPACITY;
    }
    for (int f = 0; f < n_features; ++f)
        if (point_of_feature[f] >= p->pt_cap) { morb::set_error("feature %d holds point slot %d of %d", f, point_of_feature[f], p->pt_cap); return ORB_E_CAPACITY; }
    MORB_HIP(hipSetDevice(m->device));
    int32_t* row = p->h_kf_rows.data() + (size_t)kf * p->stride;
    for (int f = 0; f < n_features; ++f) row[f] = point_of_feature[f] < 0 ? -1 : point_of_feature[f];
    for (int f = n_features; f < p->stride; ++f) row[f] = -1;
    // the old row's tail is dead once the count says so: send what the new count covers, and the count
    const int n_send = std::max(n_features, 1);
    p->h_kf_count[(size_t)kf] = n_features; p->h_kf_bad[(size_t)kf] = bad ? 1 : 0;
    p->kf_hw = std::max(p->kf_hw, kf + 1);
    MORB_HIP(hipMemcpyAsync(p->d_kf_rows.p + (size_t)kf * p->stride, row, (size_t)n_send * 4, hipMemcpyHostToDevice, m->stream));
    MORB_HIP(hipMemcpyAsync(p->d_kf_count.p + kf, &p->h_kf_count[(size_t)kf], 4, hipMemcpyHostToDevice, m->stream));
    MORB_HIP(hipStreamSynchronize(m->stream));
    return ORB_OK;
}

int orbm_map_set_keyframe_bad(orbm_matcher* m, orbm_map* p, int kf, int bad) {
    MORB_ARG(m && p && p->owner == m && kf >= 0 && kf < p->kf_cap);
    p->h_kf_bad[(size_t)kf] = bad ? 1 : 0;
    p->kf_hw = std::max(p->kf_hw, kf + 1);
    return ORB_OK;
}

int orbm_map_vote(orbm_matcher* m, orbm_map* p, const int32_t* frame_points, int n_features, int32_t* votes) {
    MORB_ARG(m && p && p->owner == m && n_features >= 0 && (n_features == 0 || frame_points) && (p->kf_hw == 0 || votes));
    for (int f = 0; f < n_features; ++f)
        if (frame_points[f] >= p->pt_cap) { morb::set_error("feature %d holds point slot %d of %d", f, frame_points[f], p->pt_cap); return ORB_E_ARG; }
    const int nk = p->kf_hw;
    p->last[1] = p->obs_hw;
    if (m->host_resolve) {   // MORB_HOST_RESOLVE=1: the host routine over the mirror
        p->last[0] = 0;
        return orbm_local_map_vote_host(p->h_obs.data(), p->obs_hw, p->h_flags.data(), p->pt_cap, frame_points, n_features, nk, votes);
    }
    p->last[0] = 1;
    if (nk == 0) return ORB_OK;
    if (n_features == 0 || p->obs_hw == 0) { for (int k = 0; k < nk; ++k) votes[k] = 0; return ORB_OK; }
    MORB_HIP(hipSetDevice(m->device));
    int rc;
    if ((rc = p->stage.reserve((size_t)n_features * 4 + 16))) return rc;
    memcpy(p->stage.p, frame_points, (size_t)n_features * 4);
    p->stage.publish();
    const int32_t* d_fp = (const int32_t*)p->stage.dp;
    const unsigned g = blocks_of(std::max(n_features, nk));
    hipLaunchKernelGGL(k_map_mult, dim3(g), dim3(MAP_BLOCK), 0, m->stream, d_fp, n_features, (const uint8_t*)p->d_flags.p, p->d_mult.p,
                       p->d_votes.p, nk);
    const long long per_block = (long long)MAP_BLOCK * MAP_VOTE_PER_LANE;
    const unsigned gv = (unsigned)std::min<long long>(MAP_VOTE_MAX_BLOCKS, (p->obs_hw + per_block - 1) / per_block);
    hipLaunchKernelGGL(k_map_vote, dim3(gv), dim3(MAP_BLOCK), (size_t)nk * sizeof(int32_t), m->stream, (const orbm_obs*)p->d_obs.p, p->obs_hw,
                       (const int32_t*)p->d_mult.p, p->d_votes.p, nk);
    hipLaunchKernelGGL(k_map_vote_out, dim3(g), dim3(MAP_BLOCK), 0, m->stream, d_fp, n_features, p->d_mult.p, (const int32_t*)p->d_votes.p, nk,
                       p->h_votes.dp);
    MORB_HIP(hipGetLastError());
    MORB_HIP(hipStreamSynchronize(m->stream));
    memcpy(votes, p->h_votes.p, (size_t)nk * sizeof(int32_t));
    return ORB_OK;
}

int orbm_map_local_points(orbm_matcher* m, orbm_map* p, const int32_t* local_kfs, int n_local, int32_t* list, int* n_list) {
    MORB_ARG(m && p && p->owner == m && n_local >= 0 && (n_local == 0 || local_kfs) && list && n_list);
    if (n_local > ORBM_MAP_MAX_LOCAL) { morb::set_error("%d local keyframes are more than a call takes (%d)", n_local, (int)ORBM_MAP_MAX_LOCAL); return ORB_E_CAPACITY; }
    int rc;
    if (check_slots(local_kfs, n_local, 0, p->kf_hw, "local keyframe")) return ORB_E_ARG;
    p->list_n = -1; *n_list = 0;
    long long cand = 0; int fmax = 0;
    for (int j = 0; j < n_local; ++j) { const int c = p->h_kf_count[(size_t)local_kfs[j]]; cand += c; fmax = std::max(fmax, c); }
    p->last[2] = (int)std::min<long long>(cand, 0x7fffffff); p->last[3] = 0;
    p->list.resize(ORBM_MAX_POINTS);
    int n = 0;
    if (m->host_resolve) {   // MORB_HOST_RESOLVE=1: the host routine over the mirror (the list still goes to HBM for the search's kernels)
        p->last[0] = 0;
        rc = orbm_local_map_points_host(p->h_kf_rows.data(), p->h_kf_count.data(), p->kf_hw, p->stride, p->h_flags.data(), p->pt_cap,
                                        local_kfs, n_local, p->list.data(), ORBM_MAX_POINTS, &n);
        if (rc) return rc;
    } else {
        p->last[0] = 1;
        if (fmax > 0) {
            MORB_HIP(hipSetDevice(m->device));
            const int bpk = (fmax + MAP_BLOCK - 1) / MAP_BLOCK, nb = n_local * bpk;
            if ((rc = p->stage.reserve((size_t)n_local * 4 + 16)) || (rc = p->d_block.reserve((size_t)nb)) || (rc = next_epoch(m, p))) return rc;
            memcpy(p->stage.p, local_kfs, (size_t)n_local * 4);
            p->stage.publish();
            const int32_t* d_kfs = (const int32_t*)p->stage.dp;
            const int32_t *rows = p->d_kf_rows.p, *cnt = p->d_kf_count.p;
            const uint8_t* fl = p->d_flags.p;
            hipLaunchKernelGGL(k_map_first, dim3(nb), dim3(MAP_BLOCK), 0, m->stream, rows, cnt, d_kfs, p->stride, bpk, fl, p->d_first.p, p->epoch);
            hipLaunchKernelGGL(k_map_count, dim3(nb), dim3(MAP_BLOCK), 0, m->stream, rows, cnt, d_kfs, p->stride, bpk, fl,
                               (const unsigned long long*)p->d_first.p, p->epoch, p->d_block.p);
            hipLaunchKernelGGL(k_map_scan, dim3(1), dim3(MAP_SCAN_LANES), 0, m->stream, p->d_block.p, nb, p->d_total.p, p->h_total.dp);
            hipLaunchKernelGGL(k_map_scatter, dim3(nb), dim3(MAP_BLOCK), 0, m->stream, rows, cnt, d_kfs, p->stride, bpk, fl,
                               (const unsigned long long*)p->d_first.p, p->epoch, (const int32_t*)p->d_block.p, p->d_list.p, p->h_list.dp,
                               (int)ORBM_MAX_POINTS);
            MORB_HIP(hipGetLastError());
            MORB_HIP(hipStreamSynchronize(m->stream));
            n = p->h_total.p[0];
            if (n > ORBM_MAX_POINTS) { morb::set_error("%d local points are more than a search takes (%d)", n, (int)ORBM_MAX_POINTS); return ORB_E_CAPACITY; }
            memcpy(p->list.data(), p->h_list.p, (size_t)n * sizeof(int32_t));
        }
    }
    if (m->host_resolve && n > 0) {
        MORB_HIP(hipSetDevice(m->device));
        MORB_HIP(hipMemcpyAsync(p->d_list.p, p->list.data(), (size_t)n * 4, hipMemcpyHostToDevice, m->stream));
        MORB_HIP(hipStreamSynchronize(m->stream));
    }
    memcpy(list, p->list.data(), (size_t)n * sizeof(int32_t));
    p->list_n = n; *n_list = n; p->last[3] = n;
    return ORB_OK;
}

namespace {
struct SkipCtx { orbm_map* p; const int32_t* frame_points; int n_features; const int32_t* seen; int n_seen; };
void host_skip(void* c, uint8_t* out) {   // what k_map_mark + k_frustum<true> decide, from the mirror
    const SkipCtx* S = (const SkipCtx*)c;
    orbm_map* p = S->p;
    for (int f = 0; f < S->n_features; ++f) {
        const int s = S->frame_points[f];
        if (s >= 0 && !(p->h_flags[(size_t)s] & ORBM_POINT_BAD)) p->h_mark[(size_t)s] = p->epoch;
    }
    for (int i = 0; i < S->n_seen; ++i)
        if (S->seen[i] >= 0) p->h_mark[(size_t)S->seen[i]] = p->epoch;
    for (int i = 0; i < p->list_n; ++i) {
        const size_t s = (size_t)p->list[(size_t)i];
        out[i] = ((p->h_flags[s] & ORBM_POINT_BAD) || p->h_mark[s] == p->epoch) ? 1 : 0;
    }
}
}  // namespace

int orbm_map_search_local_points(orbm_matcher* m, const orbm_frame* cur, orbm_map* p, const orbm_view* view, const int32_t* frame_points,
                                 int n_features, const int32_t* seen, int n_seen, const uint8_t* occupied, float nnratio, int th_high,
                                 orbm_track* track, int32_t* match_of_feature, int* n_to_match, int* nmatches) {
    MORB_ARG(m && cur && p && p->owner == m && cur->owner == m && view && n_to_match && nmatches && (cur->n_total == 0 || match_of_feature));
    MORB_ARG(n_features >= 0 && (n_features == 0 || frame_points) && n_seen >= 0 && (n_seen == 0 || seen));
    MORB_ARG(view->n_levels >= 1 && view->n_levels <= ORBM_MAX_LEVELS && view->scale_factors);
    if (p->list_n < 0) { morb::set_error("no point list on the map: orbm_map_local_points comes first"); return ORB_E_ARG; }
    for (int f = 0; f < n_features; ++f) MORB_ARG(frame_points[f] < p->pt_cap);
    for (int i = 0; i < n_seen; ++i) MORB_ARG(seen[i] < p->pt_cap);
    const int n = p->list_n;
    int rc;
    MORB_HIP(hipSetDevice(m->device));
    if ((rc = next_epoch(m, p))) return rc;
    SkipCtx sc{p, frame_points, n_features, seen, n_seen};
    LocalPointSource S{};
    S.d_rows = p->d_rows.p; S.h_rows = p->h_rows.data(); S.d_index = p->d_list.p; S.h_index = p->list.data();
    S.d_mark = p->d_mark.p; S.d_flags = p->d_flags.p; S.epoch = p->epoch; S.host_skip = host_skip; S.host_skip_ctx = &sc;
    if (!m->host_resolve && n > 0 && n_features + n_seen > 0) {
        const size_t off_seen = (size_t)n_features * 4;
        if ((rc = p->stage.reserve(off_seen + (size_t)n_seen * 4 + 16))) return rc;
        if (n_features) memcpy(p->stage.p, frame_points, (size_t)n_features * 4);
        if (n_seen) memcpy(p->stage.p + off_seen, seen, (size_t)n_seen * 4);
        p->stage.publish();
        hipLaunchKernelGGL(k_map_mark, dim3(blocks_of((long long)n_features + n_seen)), dim3(MAP_BLOCK), 0, m->stream,
                           (const int32_t*)p->stage.dp, n_features, (const int32_t*)(p->stage.dp + off_seen), n_seen,
                           (const uint8_t*)p->d_flags.p, p->d_mark.p, p->epoch);
        MORB_HIP(hipGetLastError());
    }
    return morb::search_local_points_body(m, cur, p->scr, S, n, view, occupied, nnratio, th_high, track, match_of_feature, n_to_match, nmatches);
}

// ---- covisibility and culling counts

namespace {

// The live records of every point as a CSR list, for the host routines: first[p] .. first[p+1]-1 index `recs`, in record order.
int records_by_point(const orbm_obs* obs, const int32_t* obs_feature, int n_obs, int n_points, int n_kfs, int stride,
                     std::vector<int32_t>& first, std::vector<int32_t>& recs) {
    first.assign((size_t)n_points + 1, 0);
    for (int r = 0; r < n_obs; ++r) {
        if (obs[r].point < 0) continue;
        MORB_ARG(obs[r].point < n_points && obs[r].keyframe >= 0 && obs[r].keyframe < n_kfs && obs_feature[r] >= 0 && obs_feature[r] < stride);
        ++first[(size_t)obs[r].point + 1];
    }
    for (int p = 0; p < n_points; ++p) first[(size_t)p + 1] += first[(size_t)p];
    recs.resize((size_t)first[(size_t)n_points]);
    std::vector<int32_t> at(first.begin(), first.end() - 1);
    for (int r = 0; r < n_obs; ++r)
        if (obs[r].point >= 0) recs[(size_t)at[(size_t)obs[r].point]++] = r;
    return ORB_OK;
}

int check_rows(const int32_t* kf_rows, const int32_t* kf_count, int n_kfs, int stride, int n_points, const int32_t* kfs, int n) {
    for (int j = 0; j < n; ++j) {
        MORB_ARG(kfs[j] >= 0 && kfs[j] < n_kfs && kf_count[kfs[j]] >= 0 && kf_count[kfs[j]] <= stride);
        for (int i = 0; i < kf_count[kfs[j]]; ++i) MORB_ARG(kf_rows[(size_t)kfs[j] * stride + i] < n_points);
    }
    return ORB_OK;
}

// Clears the heads and links every live record below the high-water mark, when a record write has made the chains stale.
int build_index_if_dirty(orbm_matcher* m, orbm_map* p) {
    p->last_cov[1] = 0; p->last_cov[2] = p->obs_hw;
    if (!p->index_dirty) return ORB_OK;
    MORB_HIP(hipMemsetAsync(p->d_head.p, 0xff, (size_t)std::max(p->pt_cap, 1) * sizeof(int32_t), m->stream));
    if (p->obs_hw > 0)
        hipLaunchKernelGGL(k_map_chain, dim3(blocks_of(p->obs_hw)), dim3(MAP_BLOCK), 0, m->stream, (const orbm_obs*)p->d_obs.p, p->obs_hw,
                           p->d_head.p, p->d_next.p);
    MORB_HIP(hipGetLastError());
    p->index_dirty = false; p->last_cov[1] = 1;
    return ORB_OK;
}

int check_listed(const orbm_map* p, const int32_t* kfs, int n) {
    if (n > ORBM_MAP_MAX_LOCAL) { morb::set_error("%d keyframes are more than a call takes (%d)", n, (int)ORBM_MAP_MAX_LOCAL); return ORB_E_CAPACITY; }
    return check_slots(kfs, n, 0, p->kf_hw, "keyframe") ? ORB_E_ARG : ORB_OK;
}

}  // namespace

int orbm_local_map_covisibility_host(const orbm_obs* obs, const int32_t* obs_feature, int n_obs, const uint8_t* point_flags, int n_points,
                                     const int32_t* kf_rows, const int32_t* kf_count, const int32_t* kf_n_cam1, int n_kfs, int stride,
                                     const int32_t* kfs, int n, int32_t* first_out, orbm_covis_entry* entries, int entries_cap) {
    MORB_ARG(n_obs >= 0 && (n_obs == 0 || (obs && obs_feature)) && n_points >= 0 && (n_points == 0 || point_flags) && n_kfs >= 0 && stride >= 1 &&
             (n_kfs == 0 || (kf_rows && kf_count && kf_n_cam1)) && n >= 0 && (n == 0 || kfs) && first_out && entries_cap >= 0 &&
             (entries_cap == 0 || entries));
    int rc;
    if ((rc = check_rows(kf_rows, kf_count, n_kfs, stride, n_points, kfs, n))) return rc;
    std::vector<int32_t> first, recs;
    if ((rc = records_by_point(obs, obs_feature, n_obs, n_points, n_kfs, stride, first, recs))) return rc;
    std::vector<int32_t> all((size_t)n_kfs, 0), cam1((size_t)n_kfs, 0), touched;
    long long total = 0;
    first_out[0] = 0;
    for (int j = 0; j < n; ++j) {
        const int k = kfs[j];
        touched.clear();
        for (int i = 0; i < kf_count[k]; ++i) {
            const int p = kf_rows[(size_t)k * stride + i];
            if (p < 0) continue;
            if (point_flags[p] & ORBM_POINT_BAD) continue;
            for (int a = first[(size_t)p]; a < first[(size_t)p + 1]; ++a) {
                const int r = recs[(size_t)a], kf = obs[r].keyframe;
                if (kf == k) continue;
                if (all[(size_t)kf]++ == 0) touched.push_back(kf);
                if (i < kf_n_cam1[k] && obs_feature[r] < kf_n_cam1[kf]) ++cam1[(size_t)kf];
            }
        }
        std::sort(touched.begin(), touched.end());
        for (int kf : touched) {
            if (total < entries_cap) entries[total] = orbm_covis_entry{kf, all[(size_t)kf], cam1[(size_t)kf]};
            ++total;
            all[(size_t)kf] = 0; cam1[(size_t)kf] = 0;
        }
        first_out[j + 1] = (int32_t)std::min<long long>(total, 0x7fffffff);
    }
    if (total > entries_cap) { morb::set_error("%lld covisibility entries are more than the list takes (%d)", total, entries_cap); return ORB_E_CAPACITY; }
    return ORB_OK;
}

int orbm_local_map_culling_host(const orbm_obs* obs, const int32_t* obs_feature, int n_obs, const uint8_t* point_flags,
                                const int32_t* point_n_obs, int n_points, const int32_t* kf_rows, const int32_t* kf_count,
                                const uint8_t* kf_feature_bytes, int n_kfs, int stride, const int32_t* kfs, int n, int mono,
                                int32_t* counts_out) {
    MORB_ARG(n_obs >= 0 && (n_obs == 0 || (obs && obs_feature)) && n_points >= 0 && (n_points == 0 || (point_flags && point_n_obs)) &&
             n_kfs >= 0 && stride >= 1 && (n_kfs == 0 || (kf_rows && kf_count && kf_feature_bytes)) && n >= 0 && (n == 0 || (kfs && counts_out)));
    int rc;
    if ((rc = check_rows(kf_rows, kf_count, n_kfs, stride, n_points, kfs, n))) return rc;
    std::vector<int32_t> first, recs;
    if ((rc = records_by_point(obs, obs_feature, n_obs, n_points, n_kfs, stride, first, recs))) return rc;
    for (int j = 0; j < n; ++j) {
        const int k = kfs[j];
        const uint8_t* feat = kf_feature_bytes + (size_t)k * stride;
        int nMPs = 0, nRedundant = 0;
        for (int i = 0; i < kf_count[k]; ++i) {
            const int p = kf_rows[(size_t)k * stride + i];
            if (p < 0) continue;
            if (point_flags[p] & ORBM_POINT_BAD) continue;
            if (!mono && (feat[i] & ORBM_FEATURE_FAR)) continue;
            ++nMPs;
            if (point_n_obs[p] > 3) {
                const int level = feat[i] & ORBM_FEATURE_LEVEL_MASK;
                int c = 0;
                for (int a = first[(size_t)p]; a < first[(size_t)p + 1]; ++a) {
                    const int r = recs[(size_t)a], kf = obs[r].keyframe;
                    if (kf == k) continue;
                    if ((kf_feature_bytes[(size_t)kf * stride + obs_feature[r]] & ORBM_FEATURE_LEVEL_MASK) <= level + 1) ++c;
                }
                if (c >= 3) ++nRedundant;
            }
        }
        counts_out[2 * j] = nMPs; counts_out[2 * j + 1] = nRedundant;
    }
    return ORB_OK;
}

int orbm_debug_last_covisibility(const orbm_map* p, int* out4) {
    MORB_ARG(p && out4);
    for (int k = 0; k < 4; ++k) out4[k] = p->last_cov[k];
    return ORB_OK;
}

int orbm_map_write_observation_features(orbm_matcher* m, orbm_map* p, const int32_t* slots, int n, const int32_t* feature) {
    MORB_ARG(m && p && p->owner == m && n >= 0 && (n == 0 || (slots && feature)));
    int rc;
    if ((rc = check_slots(slots, n, 0, p->obs_cap, "record slot")) || (rc = check_slots(feature, n, 0, p->stride, "feature index"))) return rc;
    if (n == 0) return ORB_OK;
    MORB_HIP(hipSetDevice(m->device));
    const size_t off_val = (size_t)n * 4;
    if ((rc = p->stage.reserve(off_val + (size_t)n * 4 + 16))) return rc;
    for (int i = 0; i < n; ++i) p->h_obs_feat[(size_t)slots[i]] = feature[i];
    memcpy(p->stage.p, slots, (size_t)n * 4);   // (staged from the mirror, as the records are: a slot named twice takes its last entry)
    for (int i = 0; i < n; ++i) memcpy(p->stage.p + off_val + (size_t)i * 4, &p->h_obs_feat[(size_t)slots[i]], 4);
    p->stage.publish();
    hipLaunchKernelGGL(k_map_put_words, dim3(blocks_of(n)), dim3(MAP_BLOCK), 0, m->stream, (const uint32_t*)(p->stage.dp + off_val),
                       (const int32_t*)p->stage.dp, n, 1, (uint32_t*)p->d_obs_feat.p);
    MORB_HIP(hipGetLastError());
    MORB_HIP(hipStreamSynchronize(m->stream));
    return ORB_OK;
}

int orbm_map_write_point_nobs(orbm_matcher* m, orbm_map* p, const int32_t* slots, int n, const int32_t* n_obs) {
    MORB_ARG(m && p && p->owner == m && n >= 0 && (n == 0 || (slots && n_obs)));
    int rc;
    if ((rc = check_slots(slots, n, 0, p->pt_cap, "point slot"))) return rc;
    if (n == 0) return ORB_OK;
    MORB_HIP(hipSetDevice(m->device));
    const size_t off_val = (size_t)n * 4;
    if ((rc = p->stage.reserve(off_val + (size_t)n * 4 + 16))) return rc;
    for (int i = 0; i < n; ++i) p->h_nobs[(size_t)slots[i]] = n_obs[i];
    memcpy(p->stage.p, slots, (size_t)n * 4);
    for (int i = 0; i < n; ++i) memcpy(p->stage.p + off_val + (size_t)i * 4, &p->h_nobs[(size_t)slots[i]], 4);
    p->stage.publish();
    hipLaunchKernelGGL(k_map_put_words, dim3(blocks_of(n)), dim3(MAP_BLOCK), 0, m->stream, (const uint32_t*)(p->stage.dp + off_val),
                       (const int32_t*)p->stage.dp, n, 1, (uint32_t*)p->d_nobs.p);
    MORB_HIP(hipGetLastError());
    MORB_HIP(hipStreamSynchronize(m->stream));
    return ORB_OK;
}

int orbm_map_write_keyframe_features(orbm_matcher* m, orbm_map* p, int kf, const uint8_t* feature_bytes, int n_features, int n_cam1) {
    MORB_ARG(m && p && p->owner == m && n_features >= 0 && (n_features == 0 || feature_bytes) && n_cam1 >= 0);
    if (kf < 0 || kf >= p->kf_cap || n_features > p->stride || n_cam1 > p->stride) {
        morb::set_error("keyframe slot %d with %d features, %d of camera 1, does not fit a map of %d keyframes of %d", kf, n_features, n_cam1,
                        p->kf_cap, p->stride);
        return kf < 0 ? ORB_E_ARG : ORB_E_CAPACITY;
    }
    MORB_HIP(hipSetDevice(m->device));
    uint8_t* row = p->h_kf_feat.data() + (size_t)kf * p->stride;
    if (n_features) memcpy(row, feature_bytes, (size_t)n_features);
    memset(row + n_features, 0, (size_t)(p->stride - n_features));
    p->h_kf_ncam1[(size_t)kf] = n_cam1;
    // the whole row travels: a record of another keyframe's point may name any feature of this one
    MORB_HIP(hipMemcpyAsync(p->d_kf_feat.p + (size_t)kf * p->stride, row, (size_t)p->stride, hipMemcpyHostToDevice, m->stream));
    MORB_HIP(hipMemcpyAsync(p->d_kf_ncam1.p + kf, &p->h_kf_ncam1[(size_t)kf], 4, hipMemcpyHostToDevice, m->stream));
    MORB_HIP(hipStreamSynchronize(m->stream));
    return ORB_OK;
}

int orbm_map_covisibility(orbm_matcher* m, orbm_map* p, const int32_t* kfs, int n, int32_t* first_out, orbm_covis_entry* entries,
                          int entries_cap) {
    MORB_ARG(m && p && p->owner == m && n >= 0 && (n == 0 || kfs) && first_out && entries_cap >= 0 && (entries_cap == 0 || entries));
    int rc;
    if ((rc = check_listed(p, kfs, n))) return rc;
    p->last_cov[3] = n;
    if (m->host_resolve) {   // MORB_HOST_RESOLVE=1: the host routine over the mirror
        p->last_cov[0] = 0; p->last_cov[1] = 0; p->last_cov[2] = p->obs_hw;
        std::vector<orbm_covis_entry> tmp((size_t)std::max(entries_cap, 1));
        rc = orbm_local_map_covisibility_host(p->h_obs.data(), p->h_obs_feat.data(), p->obs_hw, p->h_flags.data(), p->pt_cap, p->h_kf_rows.data(),
                                              p->h_kf_count.data(), p->h_kf_ncam1.data(), p->kf_hw, p->stride, kfs, n, first_out, tmp.data(),
                                              entries_cap);
        if (rc == ORB_E_CAPACITY) { const int32_t need = first_out[n]; for (int j = 0; j < n; ++j) first_out[j] = 0; first_out[n] = need; }
        if (rc == ORB_OK && first_out[n] > 0) memcpy(entries, tmp.data(), (size_t)first_out[n] * sizeof(orbm_covis_entry));
        return rc;
    }
    p->last_cov[0] = 1;
    MORB_HIP(hipSetDevice(m->device));
    if ((rc = build_index_if_dirty(m, p))) return rc;
    first_out[0] = 0;
    if (n == 0) { MORB_HIP(hipStreamSynchronize(m->stream)); return ORB_OK; }
    if ((rc = p->stage.reserve((size_t)n * 4 + 16)) || (rc = p->h_span.reserve((size_t)n * 2)) ||
        (rc = p->h_entries.reserve((size_t)std::max(entries_cap, 1)))) return rc;
    memcpy(p->stage.p, kfs, (size_t)n * 4);
    p->stage.publish();
    MORB_HIP(hipMemsetAsync(p->d_cursor.p, 0, sizeof(int32_t), m->stream));
    const int nk = p->kf_hw;
    hipLaunchKernelGGL(k_map_covis, dim3(n), dim3(MAP_BLOCK), ((size_t)nk + MAP_BLOCK / 64 + 1) * sizeof(int32_t), m->stream,
                       (const int32_t*)p->stage.dp, (const int32_t*)p->d_kf_rows.p, (const int32_t*)p->d_kf_count.p,
                       (const int32_t*)p->d_kf_ncam1.p, p->stride, (const uint8_t*)p->d_flags.p, (const orbm_obs*)p->d_obs.p,
                       (const int32_t*)p->d_obs_feat.p, (const int32_t*)p->d_head.p, (const int32_t*)p->d_next.p, nk, p->d_cursor.p,
                       p->h_span.dp, p->h_entries.dp, entries_cap);
    MORB_HIP(hipGetLastError());
    MORB_HIP(hipStreamSynchronize(m->stream));
    long long total = 0;
    for (int j = 0; j < n; ++j) total += p->h_span.p[2 * j + 1];
    if (total > entries_cap) {
        for (int j = 0; j < n; ++j) first_out[j] = 0;
        first_out[n] = (int32_t)std::min<long long>(total, 0x7fffffff);
        morb::set_error("%lld covisibility entries are more than the list takes (%d)", total, entries_cap);
        return ORB_E_CAPACITY;
    }
    // the workgroups took their spans in the order they arrived: laid out here in the order of kfs
    for (int j = 0; j < n; ++j) {
        const int start = p->h_span.p[2 * j], cnt = p->h_span.p[2 * j + 1];
        if (cnt) memcpy(entries + first_out[j], p->h_entries.p + start, (size_t)cnt * sizeof(orbm_covis_entry));
        first_out[j + 1] = first_out[j] + cnt;
    }
    return ORB_OK;
}

int orbm_map_culling_counts(orbm_matcher* m, orbm_map* p, const int32_t* kfs, int n, int mono, int32_t* counts_out) {
    MORB_ARG(m && p && p->owner == m && n >= 0 && (n == 0 || (kfs && counts_out)));
    int rc;
    if ((rc = check_listed(p, kfs, n))) return rc;
    p->last_cov[3] = n;
    if (m->host_resolve) {   // MORB_HOST_RESOLVE=1: the host routine over the mirror
        p->last_cov[0] = 0; p->last_cov[1] = 0; p->last_cov[2] = p->obs_hw;
        return orbm_local_map_culling_host(p->h_obs.data(), p->h_obs_feat.data(), p->obs_hw, p->h_flags.data(), p->h_nobs.data(), p->pt_cap,
                                           p->h_kf_rows.data(), p->h_kf_count.data(), p->h_kf_feat.data(), p->kf_hw, p->stride, kfs, n, mono,
                                           counts_out);
    }
    p->last_cov[0] = 1;
    MORB_HIP(hipSetDevice(m->device));
    if ((rc = build_index_if_dirty(m, p))) return rc;
    if (n == 0) { MORB_HIP(hipStreamSynchronize(m->stream)); return ORB_OK; }
    if ((rc = p->stage.reserve((size_t)n * 4 + 16)) || (rc = p->h_counts.reserve((size_t)n * 2))) return rc;
    memcpy(p->stage.p, kfs, (size_t)n * 4);
    p->stage.publish();
    hipLaunchKernelGGL(k_map_cull, dim3(n), dim3(MAP_BLOCK), 0, m->stream, (const int32_t*)p->stage.dp, (const int32_t*)p->d_kf_rows.p,
                       (const int32_t*)p->d_kf_count.p, (const uint8_t*)p->d_kf_feat.p, p->stride, (const uint8_t*)p->d_flags.p,
                       (const int32_t*)p->d_nobs.p, (const orbm_obs*)p->d_obs.p, (const int32_t*)p->d_obs_feat.p, (const int32_t*)p->d_head.p,
                       (const int32_t*)p->d_next.p, mono ? 1 : 0, p->h_counts.dp);
    MORB_HIP(hipGetLastError());
    MORB_HIP(hipStreamSynchronize(m->stream));
    memcpy(counts_out, p->h_counts.p, (size_t)n * 2 * sizeof(int32_t));
    return ORB_OK;
}

// ---- loop correction over the resident map (kernels: mapcorrect_dev.h)

namespace {

constexpr int POS_STRIDE_ROWS = (int)(sizeof(orbm_point) / sizeof(float));   // the mirror's rows as a strided array of positions
static_assert(offsetof(orbm_point, pos) == 0 && sizeof(orbm_point) % sizeof(float) == 0, "a row begins with its position");

inline size_t pad8(size_t n) { return (n + 7) & ~(size_t)7; }

// The positions of the listed slots from the mirror into their rows in HBM (a slot named twice is staged twice with the same bytes).
// Enqueues only: the caller synchronises.
int put_positions(orbm_matcher* m, orbm_map* p, const int32_t* slots, int n) {
    if (n == 0) return ORB_OK;
    int rc;
    const size_t off_pos = pad8((size_t)n * 4);
    if ((rc = p->stage.reserve(off_pos + (size_t)n * 12 + 16))) return rc;
    memcpy(p->stage.p, slots, (size_t)n * 4);
    for (int i = 0; i < n; ++i) memcpy(p->stage.p + off_pos + (size_t)i * 12, p->h_rows[(size_t)slots[i]].pos, 12);
    p->stage.publish();
    hipLaunchKernelGGL(k_map_put_positions, dim3(blocks_of((long long)n * 3)), dim3(MAP_BLOCK), 0, m->stream,
                       (const float*)(p->stage.dp + off_pos), (const int32_t*)p->stage.dp, n, p->d_rows.p);
    MORB_HIP(hipGetLastError());
    return ORB_OK;
}

int check_sim3_args(const int32_t* kfs, int n, const double* before, const double* after, const int32_t* already, int n_already,
                    const orbm_correct_entry* entries, const float* pos_out, int cap, const int* n_out, const float* Tiw_out) {
    MORB_ARG(n >= 0 && (n == 0 || (kfs && before && after && Tiw_out)) && n_already >= 0 && (n_already == 0 || already) && cap >= 0 &&
             (cap == 0 || (entries && pos_out)) && n_out);
    if (n > ORBM_MAP_MAX_LOCAL) { morb::set_error("%d keyframes are more than a call takes (%d)", n, (int)ORBM_MAP_MAX_LOCAL); return ORB_E_CAPACITY; }
    return ORB_OK;
}

int check_rigid_args(int n, const uint8_t* kf_corrected, const float* Tcw_before, const float* Twc_after, int n_kfs,
                     const int32_t* gba_slots, const float* gba_pos, int n_gba, int n_points) {
    MORB_ARG(n >= 0 && n_kfs >= 0 && (n_kfs == 0 || (kf_corrected && Tcw_before && Twc_after)) && n_gba >= 0 &&
             (n_gba == 0 || (gba_slots && gba_pos)));
    if (n_kfs > ORBM_MAP_MAX_KEYFRAMES) { morb::set_error("%d keyframes are more than a map holds (%d)", n_kfs, (int)ORBM_MAP_MAX_KEYFRAMES); return ORB_E_CAPACITY; }
    for (int g = 0; g < n_gba; ++g) MORB_ARG(gba_slots[g] < n_points);
    return ORB_OK;
}

// rows 0-2 of mTcwBefGBA, then rows 0-2 of GetPoseInverse(), per keyframe
void rigid_table(const float* Tcw_before, const float* Twc_after, int n_kfs, float* table) {
    for (int r = 0; r < n_kfs; ++r) {
        memcpy(table + (size_t)MAP_RIGID_TABLE * r, Tcw_before + 12 * (size_t)r, 48);
        memcpy(table + (size_t)MAP_RIGID_TABLE * r + 12, Twc_after + 12 * (size_t)r, 48);
    }
}

}  // namespace

int orbm_local_map_correct_sim3_host(const int32_t* kf_rows, const int32_t* kf_count, int n_kfs, int stride, const uint8_t* point_flags,
                                     float* pos, int pos_stride, int n_points, const int32_t* kfs, int n, const double* sim3_before,
                                     const double* sim3_after, const int32_t* already, int n_already, orbm_correct_entry* entries,
                                     float* pos_out, int cap, int* n_out, float* Tiw_out) {
    MORB_ARG(n_kfs >= 0 && stride >= 1 && (n_kfs == 0 || (kf_rows && kf_count)) && n_points >= 0 && (n_points == 0 || (point_flags && pos)) &&
             pos_stride >= 3);
    int rc;
    if ((rc = check_sim3_args(kfs, n, sim3_before, sim3_after, already, n_already, entries, pos_out, cap, n_out, Tiw_out))) return rc;
    *n_out = 0;
    std::vector<uint8_t> marked((size_t)n_points, 0);   // mnCorrectedByKF == mpCurrentKF->mnId
    for (int i = 0; i < n_already; ++i) {
        if (already[i] < 0) continue;
        MORB_ARG(already[i] < n_points);
        marked[(size_t)already[i]] = 1;
    }
    std::vector<orbm_correct_entry> kept;
    for (int j = 0; j < n; ++j) {
        const int kf = kfs[j];
        MORB_ARG(kf >= 0 && kf < n_kfs && kf_count[kf] >= 0 && kf_count[kf] <= stride);
        for (int f = 0; f < kf_count[kf]; ++f) {
            const int s = kf_rows[(size_t)kf * stride + f];
            if (s < 0) continue;                              // :692
            MORB_ARG(s < n_points);
            if (point_flags[s] & ORBM_POINT_BAD) continue;    // :694
            if (marked[(size_t)s]) continue;                  // :696
            kept.push_back(orbm_correct_entry{s, j});
            marked[(size_t)s] = 1;                            // :707
        }
    }
    *n_out = (int)std::min<size_t>(kept.size(), 0x7fffffff);
    if (kept.size() > (size_t)cap) {
        morb::set_error("%zu corrected points are more than the list takes (%d)", kept.size(), cap);
        return ORB_E_CAPACITY;
    }
    std::vector<double> table((size_t)n * MAP_SIM3_TABLE);
    for (int j = 0; j < n; ++j) {
        map_sim3_table_entry(sim3_before + 8 * (size_t)j, sim3_after + 8 * (size_t)j, table.data() + (size_t)MAP_SIM3_TABLE * j);
        eg_Tiw(sim3_after + 8 * (size_t)j, Tiw_out + 16 * (size_t)j);   // :714-720
    }
    for (size_t i = 0; i < kept.size(); ++i) {
        float* P = pos + (size_t)pos_stride * (size_t)kept[i].point;
        float w[3];
        map_correct_sim3_point(table.data() + (size_t)MAP_SIM3_TABLE * (size_t)kept[i].position, P, w);
        for (int k = 0; k < 3; ++k) { P[k] = w[k]; pos_out[3 * i + k] = w[k]; }
        entries[i] = kept[i];
    }
    return ORB_OK;
}

int orbm_local_map_correct_rigid_host(float* pos, int pos_stride, const uint8_t* point_flags, const int32_t* point_ref, int n_points,
                                      const int32_t* slots, int n, const uint8_t* kf_corrected, const float* Tcw_before,
                                      const float* Twc_after, int n_kfs, const int32_t* gba_slots, const float* gba_pos, int n_gba,
                                      uint8_t* status, float* pos_out) {
    MORB_ARG(n_points >= 0 && (n_points == 0 || (pos && point_flags && point_ref)) && pos_stride >= 3);
    int rc;
    if ((rc = check_rigid_args(n, kf_corrected, Tcw_before, Twc_after, n_kfs, gba_slots, gba_pos, n_gba, n_points))) return rc;
    if (!slots) MORB_ARG(n <= n_points);
    std::vector<int32_t> given((size_t)n_points, -1);   // mnBAGlobalForKF == nLoopKF: the last entry that names the point
    for (int g = 0; g < n_gba; ++g)
        if (gba_slots[g] >= 0) given[(size_t)gba_slots[g]] = g;
    std::vector<uint8_t> listed(slots ? (size_t)n_points : 0, 0);
    for (int i = 0; i < n && slots; ++i) {
        MORB_ARG(slots[i] >= 0 && slots[i] < n_points && !listed[(size_t)slots[i]]);
        listed[(size_t)slots[i]] = 1;
    }
    float T[MAP_RIGID_TABLE];
    for (int i = 0; i < n; ++i) {
        const int s = slots ? slots[i] : i;
        float* P = pos + (size_t)pos_stride * (size_t)s;
        int st = 0;
        if (!(point_flags[s] & ORBM_POINT_BAD)) {                          // :961
            if (given[(size_t)s] >= 0) {                                   // :964-967
                memcpy(P, gba_pos + 3 * (size_t)given[(size_t)s], 12);
                st = 1;
            } else {
                const int r = point_ref[s];
                if (r >= 0 && r < n_kfs && kf_corrected[r]) {              // :974
                    float w[3];
                    rigid_table(Tcw_before + 12 * (size_t)r, Twc_after + 12 * (size_t)r, 1, T);
                    map_correct_rigid_point(T, P, w);                      // :978-987
                    for (int k = 0; k < 3; ++k) P[k] = w[k];
                    st = 2;
                }
            }
        }
        if (status) status[i] = (uint8_t)st;
        if (pos_out) memcpy(pos_out + 3 * (size_t)i, P, 12);
    }
    return ORB_OK;
}

int orbm_map_points(const orbm_map* p) { return p ? p->pt_hw : ORB_E_ARG; }

int orbm_debug_last_correction(const orbm_map* p, int* out4) {
    MORB_ARG(p && out4);
    for (int k = 0; k < 4; ++k) out4[k] = p->last_cor[k];
    return ORB_OK;
}

int orbm_debug_map_read_points(orbm_matcher* m, orbm_map* p, const int32_t* slots, int n, orbm_point* rows) {
    MORB_ARG(m && p && p->owner == m && n >= 0 && (n == 0 || (slots && rows)));
    int rc;
    if ((rc = check_slots(slots, n, 0, p->pt_cap, "point slot"))) return rc;
    if (n == 0) return ORB_OK;
    MORB_HIP(hipSetDevice(m->device));
    const int lo = *std::min_element(slots, slots + n), hi = *std::max_element(slots, slots + n);
    std::vector<orbm_point> span((size_t)(hi - lo + 1));
    MORB_HIP(hipMemcpyAsync(span.data(), p->d_rows.p + lo, span.size() * sizeof(orbm_point), hipMemcpyDeviceToHost, m->stream));
    MORB_HIP(hipStreamSynchronize(m->stream));
    for (int i = 0; i < n; ++i) rows[i] = span[(size_t)(slots[i] - lo)];
    return ORB_OK;
}

int orbm_map_write_positions(orbm_matcher* m, orbm_map* p, const int32_t* slots, int n, const float* pos3) {
    MORB_ARG(m && p && p->owner == m && n >= 0 && (n == 0 || (slots && pos3)));
    int rc;
    if ((rc = check_slots(slots, n, 0, p->pt_cap, "point slot"))) return rc;
    if (n == 0) return ORB_OK;
    MORB_HIP(hipSetDevice(m->device));
    for (int i = 0; i < n; ++i) {
        memcpy(p->h_rows[(size_t)slots[i]].pos, pos3 + 3 * (size_t)i, 12);
        p->pt_hw = std::max(p->pt_hw, slots[i] + 1);
    }
    if ((rc = put_positions(m, p, slots, n))) return rc;   // (staged from the mirror: a slot named twice takes its last entry)
    MORB_HIP(hipStreamSynchronize(m->stream));
    return ORB_OK;
}

int orbm_map_write_point_ref(orbm_matcher* m, orbm_map* p, const int32_t* slots, int n, const int32_t* ref_kf) {
    MORB_ARG(m && p && p->owner == m && n >= 0 && (n == 0 || (slots && ref_kf)));
    int rc;
    if ((rc = check_slots(slots, n, 0, p->pt_cap, "point slot"))) return rc;
    if (n == 0) return ORB_OK;
    MORB_HIP(hipSetDevice(m->device));
    const size_t off_val = (size_t)n * 4;
    if ((rc = p->stage.reserve(off_val + (size_t)n * 4 + 16))) return rc;
    for (int i = 0; i < n; ++i) { p->h_ref[(size_t)slots[i]] = ref_kf[i]; p->pt_hw = std::max(p->pt_hw, slots[i] + 1); }
    memcpy(p->stage.p, slots, (size_t)n * 4);
    for (int i = 0; i < n; ++i) memcpy(p->stage.p + off_val + (size_t)i * 4, &p->h_ref[(size_t)slots[i]], 4);
    p->stage.publish();
    hipLaunchKernelGGL(k_map_put_words, dim3(blocks_of(n)), dim3(MAP_BLOCK), 0, m->stream, (const uint32_t*)(p->stage.dp + off_val),
                       (const int32_t*)p->stage.dp, n, 1, (uint32_t*)p->d_ref.p);
    MORB_HIP(hipGetLastError());
    MORB_HIP(hipStreamSynchronize(m->stream));
    return ORB_OK;
}

int orbm_map_correct_sim3(orbm_matcher* m, orbm_map* p, const int32_t* kfs, int n, const double* sim3_before, const double* sim3_after,
                          const int32_t* already, int n_already, orbm_correct_entry* entries, float* pos_out, int cap, int* n_out,
                          float* Tiw_out) {
    MORB_ARG(m && p && p->owner == m);
    int rc;
    if ((rc = check_sim3_args(kfs, n, sim3_before, sim3_after, already, n_already, entries, pos_out, cap, n_out, Tiw_out))) return rc;
    *n_out = 0;
    if (check_slots(kfs, n, 0, p->kf_hw, "keyframe")) return ORB_E_ARG;
    for (int i = 0; i < n_already; ++i) MORB_ARG(already[i] < p->pt_cap);
    long long cand = 0; int fmax = 0;
    for (int j = 0; j < n; ++j) { const int c = p->h_kf_count[(size_t)kfs[j]]; cand += c; fmax = std::max(fmax, c); }
    p->last_cor[1] = (int)std::min<long long>(cand, 0x7fffffff); p->last_cor[2] = 0; p->last_cor[3] = n;
    MORB_HIP(hipSetDevice(m->device));
    if (m->host_resolve) {   // MORB_HOST_RESOLVE=1: the host routine over the mirror, the new positions then sent to their rows
        p->last_cor[0] = 0;
        rc = orbm_local_map_correct_sim3_host(p->h_kf_rows.data(), p->h_kf_count.data(), p->kf_hw, p->stride, p->h_flags.data(),
                                              p->pt_cap ? p->h_rows[0].pos : nullptr, POS_STRIDE_ROWS, p->pt_cap, kfs, n, sim3_before,
                                              sim3_after, already, n_already, entries, pos_out, cap, n_out, Tiw_out);
        if (rc) return rc;
        p->last_cor[2] = *n_out;
        std::vector<int32_t> moved((size_t)*n_out);
        for (int i = 0; i < *n_out; ++i) moved[(size_t)i] = entries[i].point;
        if ((rc = put_positions(m, p, moved.data(), *n_out))) return rc;
        MORB_HIP(hipStreamSynchronize(m->stream));
        return ORB_OK;
    }
    p->last_cor[0] = 1;
    for (int j = 0; j < n; ++j) eg_Tiw(sim3_after + 8 * (size_t)j, Tiw_out + 16 * (size_t)j);   // :714-720
    if (fmax == 0) return ORB_OK;
    const int bpk = (fmax + MAP_BLOCK - 1) / MAP_BLOCK, nb = n * bpk;
    const int n_launch = (int)std::min<long long>(cap, cand);
    const size_t off_table = pad8((size_t)n * 4), off_already = off_table + (size_t)n * MAP_SIM3_TABLE * sizeof(double);
    if ((rc = p->stage.reserve(off_already + (size_t)n_already * 4 + 16)) || (rc = p->d_block.reserve((size_t)nb)) ||
        (rc = p->d_centries.reserve((size_t)std::max(n_launch, 1))) || (rc = p->h_centries.reserve((size_t)std::max(n_launch, 1))) ||
        (rc = p->h_cpos.reserve((size_t)std::max(n_launch, 1) * 3))) return rc;
    // two epochs: the claim's, and a NEWER one for the points already corrected -- a newer key is smaller than every key of the claim
    uint32_t e_claim, e_skip;
    do {
        if ((rc = next_epoch(m, p))) return rc;
        e_claim = p->epoch;
        if ((rc = next_epoch(m, p))) return rc;
        e_skip = p->epoch;
    } while (e_skip < e_claim);   // (the counter wrapped in between: both again)
    memcpy(p->stage.p, kfs, (size_t)n * 4);
    {
        double entry[MAP_SIM3_TABLE];
        for (int j = 0; j < n; ++j) {
            map_sim3_table_entry(sim3_before + 8 * (size_t)j, sim3_after + 8 * (size_t)j, entry);
            memcpy(p->stage.p + off_table + (size_t)j * sizeof(entry), entry, sizeof(entry));
        }
    }
    if (n_already) memcpy(p->stage.p + off_already, already, (size_t)n_already * 4);
    p->stage.publish();
    const int32_t* d_kfs = (const int32_t*)p->stage.dp;
    const int32_t *rows = p->d_kf_rows.p, *cnt = p->d_kf_count.p;
    const uint8_t* fl = p->d_flags.p;
    if (n_already)
        hipLaunchKernelGGL(k_map_stamp, dim3(blocks_of(n_already)), dim3(MAP_BLOCK), 0, m->stream, (const int32_t*)(p->stage.dp + off_already),
                           n_already, p->d_first.p, map_key(e_skip, 0));
    hipLaunchKernelGGL(k_map_first, dim3(nb), dim3(MAP_BLOCK), 0, m->stream, rows, cnt, d_kfs, p->stride, bpk, fl, p->d_first.p, e_claim);
    hipLaunchKernelGGL(k_map_count, dim3(nb), dim3(MAP_BLOCK), 0, m->stream, rows, cnt, d_kfs, p->stride, bpk, fl,
                       (const unsigned long long*)p->d_first.p, e_claim, p->d_block.p);
    hipLaunchKernelGGL(k_map_scan, dim3(1), dim3(MAP_SCAN_LANES), 0, m->stream, p->d_block.p, nb, p->d_total.p, p->h_total.dp);
    hipLaunchKernelGGL(k_map_correct_scatter, dim3(nb), dim3(MAP_BLOCK), 0, m->stream, rows, cnt, d_kfs, p->stride, bpk, fl,
                       (const unsigned long long*)p->d_first.p, e_claim, (const int32_t*)p->d_block.p, (const int32_t*)p->d_total.p,
                       p->d_centries.p, p->h_centries.dp, n_launch);
    if (n_launch > 0)
        hipLaunchKernelGGL(k_map_correct_sim3, dim3(blocks_of(n_launch)), dim3(MAP_BLOCK), 0, m->stream,
                           (const orbm_correct_entry*)p->d_centries.p, n_launch, (const int32_t*)p->d_total.p, n_launch,
                           (const double*)(p->stage.dp + off_table), p->d_rows.p, p->h_cpos.dp);
    MORB_HIP(hipGetLastError());
    MORB_HIP(hipStreamSynchronize(m->stream));
    const int total = p->h_total.p[0];
    *n_out = total;
    if (total > cap) {   // (beyond n_launch <= cap neither kernel wrote anything)
        morb::set_error("%d corrected points are more than the list takes (%d)", total, cap);
        return ORB_E_CAPACITY;
    }
    p->last_cor[2] = total;
    for (int i = 0; i < total; ++i) {
        entries[i] = p->h_centries.p[i];
        memcpy(pos_out + 3 * (size_t)i, p->h_cpos.p + 3 * (size_t)i, 12);
        memcpy(p->h_rows[(size_t)entries[i].point].pos, p->h_cpos.p + 3 * (size_t)i, 12);
    }
    return ORB_OK;
}

int orbm_map_correct_rigid(orbm_matcher* m, orbm_map* p, const int32_t* slots, int n, const uint8_t* kf_corrected,
                           const float* Tcw_before, const float* Twc_after, int n_kfs, const int32_t* gba_slots, const float* gba_pos,
                           int n_gba, uint8_t* status, float* pos_out) {
    MORB_ARG(m && p && p->owner == m);
    int rc;
    if ((rc = check_rigid_args(n, kf_corrected, Tcw_before, Twc_after, n_kfs, gba_slots, gba_pos, n_gba, p->pt_cap))) return rc;
    if (!slots) {
        if (n != p->pt_hw) { morb::set_error("slots == NULL covers the %d point slots below the high-water mark, not %d", p->pt_hw, n); return ORB_E_ARG; }
    } else {
        if ((rc = check_slots(slots, n, 0, p->pt_cap, "point slot"))) return rc;
        if (p->seen_epoch == 0xffffffffu) { std::fill(p->h_seen.begin(), p->h_seen.end(), 0u); p->seen_epoch = 0; }
        p->h_seen.resize((size_t)p->pt_cap, 0u);
        ++p->seen_epoch;
        for (int i = 0; i < n; ++i) {
            if (p->h_seen[(size_t)slots[i]] == p->seen_epoch) { morb::set_error("point slot %d is listed twice (entry %d)", slots[i], i); return ORB_E_ARG; }
            p->h_seen[(size_t)slots[i]] = p->seen_epoch;
        }
    }
    p->last_cor[1] = n; p->last_cor[2] = 0; p->last_cor[3] = n_kfs;
    MORB_HIP(hipSetDevice(m->device));
    if (m->host_resolve) {   // MORB_HOST_RESOLVE=1: the host routine over the mirror, the changed positions then sent to their rows
        p->last_cor[0] = 0;
        std::vector<uint8_t> st((size_t)std::max(n, 1));
        rc = orbm_local_map_correct_rigid_host(p->pt_cap ? p->h_rows[0].pos : nullptr, POS_STRIDE_ROWS, p->h_flags.data(), p->h_ref.data(),
                                               p->pt_cap, slots, n, kf_corrected, Tcw_before, Twc_after, n_kfs, gba_slots, gba_pos, n_gba,
                                               st.data(), pos_out);
        if (rc) return rc;
        std::vector<int32_t> moved;
        for (int i = 0; i < n; ++i)
            if (st[(size_t)i]) moved.push_back(slots ? slots[i] : i);
        p->last_cor[2] = (int)moved.size();
        if (status) memcpy(status, st.data(), (size_t)n);
        if ((rc = put_positions(m, p, moved.data(), (int)moved.size()))) return rc;
        MORB_HIP(hipStreamSynchronize(m->stream));
        return ORB_OK;
    }
    p->last_cor[0] = 1;
    if (n == 0) return ORB_OK;
    const size_t off_flag = pad8(slots ? (size_t)n * 4 : 0), off_table = off_flag + pad8((size_t)n_kfs);
    const size_t off_gslots = off_table + pad8((size_t)n_kfs * MAP_RIGID_TABLE * sizeof(float)), off_gpos = off_gslots + pad8((size_t)n_gba * 4);
    if ((rc = p->stage.reserve(off_gpos + (size_t)n_gba * 12 + 16)) || (rc = p->h_cstatus.reserve((size_t)n)) ||
        (rc = p->h_cpos.reserve((size_t)n * 3)) || (rc = next_epoch(m, p))) return rc;
    if (slots) memcpy(p->stage.p, slots, (size_t)n * 4);
    if (n_kfs) {
        memcpy(p->stage.p + off_flag, kf_corrected, (size_t)n_kfs);
        rigid_table(Tcw_before, Twc_after, n_kfs, (float*)(p->stage.p + off_table));
    }
    if (n_gba) {
        memcpy(p->stage.p + off_gslots, gba_slots, (size_t)n_gba * 4);
        memcpy(p->stage.p + off_gpos, gba_pos, (size_t)n_gba * 12);
    }
    p->stage.publish();
    if (n_gba)
        hipLaunchKernelGGL(k_map_stamp_last, dim3(blocks_of(n_gba)), dim3(MAP_BLOCK), 0, m->stream, (const int32_t*)(p->stage.dp + off_gslots),
                           n_gba, p->d_first.p, p->epoch);
    hipLaunchKernelGGL(k_map_correct_rigid, dim3(std::min<unsigned>(blocks_of(n), MAP_RIGID_MAX_BLOCKS)), dim3(MAP_BLOCK), 0, m->stream,
                       slots ? (const int32_t*)p->stage.dp : (const int32_t*)nullptr, n, p->d_rows.p, (const uint8_t*)p->d_flags.p,
                       (const int32_t*)p->d_ref.p, (const uint8_t*)(p->stage.dp + off_flag), (const float*)(p->stage.dp + off_table), n_kfs,
                       (const unsigned long long*)p->d_first.p, p->epoch, (const float*)(p->stage.dp + off_gpos), p->h_cstatus.dp,
                       p->h_cpos.dp);
    MORB_HIP(hipGetLastError());
    MORB_HIP(hipStreamSynchronize(m->stream));
    int changed = 0;
    for (int i = 0; i < n; ++i) {
        float* P = p->h_rows[(size_t)(slots ? slots[i] : i)].pos;
        if (p->h_cstatus.p[i]) { memcpy(P, p->h_cpos.p + 3 * (size_t)i, 12); ++changed; }
        if (pos_out) memcpy(pos_out + 3 * (size_t)i, P, 12);
    }
    if (status) memcpy(status, p->h_cstatus.p, (size_t)n);
    p->last_cor[2] = changed;
    return ORB_OK;
}
