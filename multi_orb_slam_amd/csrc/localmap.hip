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
// The six writers of a column by slot are one sequence (write_slots: k_map_put_words, k_map_put_flags).
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
#include "stage_pack.h"
#include "localmap_dev.h"
#include "mapcorrect_dev.h"

using namespace morb;

namespace {

// What sizes a buffer of the map when the map is created: its capacities, the longest point list, a few words.  ON_DEMAND: nothing
// then; the calls that use the buffer reserve it.  FEW is four words: the totals of the scan use them, and the one-word cursor of
// k_map_covis is sized by it too (three words of room it does not use) rather than by a domain of its own.
enum Domain { ON_DEMAND, POINTS, RECORDS, KEYFRAMES, FEATURES /* keyframes x stride */, LIST, FEW, N_DOMAINS };

// Every buffer of a map enters orbm_map::all where it is declared.  orbm_map_create and orbm_map_destroy walk that list and nothing
// else, so a buffer is named once: a column cannot be reserved and not cleared, cleared and not mirrored, or left out of the release.
struct MapBuffer {
    virtual int create(const size_t* count, hipStream_t st) = 0;   // count[Domain]; enqueues, the caller synchronises
    virtual void release() = 0;
};
using MapBuffers = std::vector<MapBuffer*>;

// A persistent column: count[D] entries in HBM (d; at least one, so a map of no points still has pointers to pass) and in the host
// mirror (h), both holding FILL in every byte until written -- 0x00: zero, 0xff: -1, {-1, -1} for a record.
enum { HBM = 1, MIRROR = 2 };
template <typename T, Domain D, int FILL, int SIDES = HBM | MIRROR>
struct Column final : MapBuffer {
    DevBuf<T> d;
    std::vector<T> h;
    explicit Column(MapBuffers& all) { all.push_back(this); }
    int clear(hipStream_t st) {   // back to the initial state, on both sides
        if (SIDES & HBM) MORB_HIP(hipMemsetAsync(d.p, FILL, d.cap * sizeof(T), st));
        T v; memset(&v, FILL, sizeof(v));
        std::fill(h.begin(), h.end(), v);
        return ORB_OK;
    }
    int create(const size_t* count, hipStream_t st) override {
        int rc = ORB_OK;
        if ((SIDES & HBM) && (rc = d.reserve(std::max<size_t>(count[D], 1)))) return rc;
        if (SIDES & MIRROR) h.resize(count[D]);
        if (clear(st)) { morb::set_error("clearing the resident map failed"); return ORB_E_HIP; }
        return ORB_OK;
    }
    void release() override { d.release(); }
};

// Per-call scratch and the mapped buffers the kernels write for the host: a DevBuf / PinnedBuf / StageBuf as it is, sized at creation
// where D says so, released with the map.
template <typename B, Domain D = ON_DEMAND>
struct Owned final : B, MapBuffer {
    explicit Owned(MapBuffers& all) { all.push_back(this); }
    int create(const size_t* count, hipStream_t) override {
        if constexpr (D != ON_DEMAND) return B::reserve(count[D]);
        return ORB_OK;
    }
    void release() override { B::release(); }
};

struct SearchScratch : FrustumScratch { void release() { h_track.release(); } };

}  // namespace

struct orbm_map {
    MapBuffers all;                  // every Column and Owned below, in the order declared
    orbm_matcher* owner = nullptr;   // compared, never dereferenced after creation
    int device = 0;
    int kf_cap = 0, pt_cap = 0, obs_cap = 0, stride = 0;
    int kf_hw = 0, obs_hw = 0;       // high-water marks: one past the last keyframe / record slot in use
    // the map: point rows and their flag bytes, observation records, mvpMapPoints of every keyframe as point slots and its length,
    // the keyframe's bad flag (host only)
    Column<orbm_point, POINTS, 0x00> rows{all};
    Column<uint8_t, POINTS, 0x00> flags{all};
    Column<orbm_obs, RECORDS, 0xff> obs{all};
    Column<int32_t, FEATURES, 0xff> kf_rows{all};
    Column<int32_t, KEYFRAMES, 0x00> kf_count{all};
    Column<uint8_t, KEYFRAMES, 0x00, MIRROR> kf_bad{all};
    // per-point scratch that stays clean between calls: the frame's multiplicity (zero), the least candidate key and the skip mark
    // (both carry the epoch of the call that wrote them; the mark's host twin serves the fallback only)
    Column<int32_t, POINTS, 0x00, HBM> mult{all};
    Column<unsigned long long, POINTS, 0xff, HBM> first{all};
    Column<uint32_t, POINTS, 0x00> mark{all};
    uint32_t epoch = 0;
    Owned<DevBuf<int32_t>, KEYFRAMES> d_votes{all};
    Owned<DevBuf<int32_t>, LIST> d_list{all};
    Owned<DevBuf<int32_t>, FEW> d_total{all};
    Owned<DevBuf<int32_t>> d_block{all};
    Owned<PinnedBuf<int32_t>, KEYFRAMES> h_votes{all};   // what the kernels write for the host: mapped pinned
    Owned<PinnedBuf<int32_t>, LIST> h_list{all};
    Owned<PinnedBuf<int32_t>, FEW> h_total{all};
    Owned<StageBuf> stage{all};      // the host-written inputs of a call
    std::vector<int32_t> list;       // the last point list (host copy; the search's fallback reads it)
    int list_n = -1;                 // -1: no list
    Owned<SearchScratch> scr{all};
    int last[4] = {0, 0, 0, 0};
    // covisibility and culling: the record's feature, the point's n_obs, the camera-1 count and the feature bytes of a keyframe ...
    Column<int32_t, RECORDS, 0x00> obs_feat{all};
    Column<int32_t, POINTS, 0x00> nobs{all};
    Column<int32_t, KEYFRAMES, 0x00> kf_ncam1{all};
    Column<uint8_t, FEATURES, 0x00> kf_feat{all};
    // ... and the chain from a point to its live records, stale after any record write
    Column<int32_t, POINTS, 0xff, HBM> head{all};
    Column<int32_t, RECORDS, 0xff, HBM> next{all};
    Owned<DevBuf<int32_t>, FEW> d_cursor{all};
    bool index_dirty = false;
    Owned<PinnedBuf<int32_t>> h_span{all}, h_counts{all};
    Owned<PinnedBuf<orbm_covis_entry>> h_entries{all};
    int last_cov[4] = {0, 0, 0, 0};
    // loop correction: the point's reference keyframe slot (-1: never written), the point high-water mark, the kept entries of a Sim3
    // correction and what either correction leaves for the host (mapped)
    Column<int32_t, POINTS, 0xff> ref{all};
    int pt_hw = 0;
    Owned<DevBuf<orbm_correct_entry>> d_centries{all};
    Owned<PinnedBuf<orbm_correct_entry>> h_centries{all};
    Owned<PinnedBuf<float>> h_cpos{all};
    Owned<PinnedBuf<uint8_t>> h_cstatus{all};
    std::vector<uint32_t> h_seen; uint32_t seen_epoch = 0;   // a listed slot of this call (host; the check that the slots are distinct)
    int last_cor[4] = {0, 0, 0, 0};
};

namespace {

// A new epoch for the keys of k_map_first and the marks of k_map_mark; the arrays are cleared when the counter would wrap.
int next_epoch(orbm_matcher* m, orbm_map* p) {
    if (p->epoch >= 0xfffffff0u) {
        int rc;
        if ((rc = p->first.clear(m->stream)) || (rc = p->mark.clear(m->stream))) return rc;
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

int copy_last(const orbm_map* p, int (orbm_map::*last)[4], int* out4) {   // the three orbm_debug_last_* of a map
    MORB_ARG(p && out4);
    for (int k = 0; k < 4; ++k) out4[k] = (p->*last)[k];
    return ORB_OK;
}

inline unsigned blocks_of(long long n) { return (unsigned)((n + MAP_BLOCK - 1) / MAP_BLOCK); }

// What one writer asks of write_slots beyond its column, slots and values.
struct SlotWrite {
    const char* what;                // the slots' name in an error
    int* hw = nullptr;               // the high-water mark the write raises (one past the greatest slot), if any
    bool with_flags = false;         // orbm_map_write_points: the rows' flag bytes ride along (k_map_put_flags) ...
    const uint8_t* flags = nullptr;  // ... from here, or zeros
    int offset = 0;                  // the entry's first word in its row
};
struct NoCheck { int operator()() const { return ORB_OK; } };
struct AsGiven { void operator()(int, void*) const {} };

// The one way a column is written by slot: n entries of `words` 32-bit words into words [offset, offset + words) of rows slots[i] of
// `col`, in HBM and in the mirror, in this order --
//   1  validate: the slots against the column's capacity, then check_values()
//   2  reserve the stage: up to here a refused call has changed nothing
//   3  write the mirror, entry by entry: values[i] (values == NULL: the mirror holds the entries already), then settle(i, the
//      mirror's entry) for what a writer changes beside the bytes, and *hw raised past the slot
//   4  stage the slots, and the values FROM THE MIRROR: a slot named twice is staged twice with its last entry, so the order in which
//      the lanes store does not matter
//   5  publish, 6  launch k_map_put_words, and synchronise.
// `words` is a constant so that the copies have a fixed size: the stage is write-combined memory, and a copy whose length is known only
// at run time made orbm_map_write_points a quarter slower (profiles/r29/notes_resident_map.md, first set).
// Who raises what:  orbm_map_write_points, _positions, _point_ref raise pt_hw;  _point_nobs raises nothing ("The resident
// map's columns");  _observations raises obs_hw and, in its settle, kf_hw for a live record;  _observation_features and the host
// routes of the corrections (put_positions) raise nothing.
template <int words, typename T, Domain D, int FILL, typename Check = NoCheck, typename Settle = AsGiven>
int write_slots(orbm_matcher* m, orbm_map* p, Column<T, D, FILL>& col, const int32_t* slots, int n, const void* values, const SlotWrite& w,
                Check check_values = Check(), Settle settle = Settle()) {
    static_assert(sizeof(T) % 4 == 0, "a column of 32-bit words");
    int rc;
    if ((rc = check_slots(slots, n, 0, (int)col.h.size(), w.what)) || (rc = check_values())) return rc;
    if (n == 0) return ORB_OK;
    MORB_HIP(hipSetDevice(m->device));
    StagePack pk;
    const int i_slots = pk.add(slots, (size_t)n * 4), i_values = pk.add_in_place((size_t)n * words * 4);
    const int i_flags = pk.add_in_place(w.with_flags ? (size_t)n : 0);
    const StagePack::Block blk = pk.open(p->stage, &rc);
    if (rc) return rc;
    uint8_t* mirror = (uint8_t*)col.h.data() + (size_t)w.offset * 4;
    for (int i = 0; i < n; ++i) {
        uint8_t* entry = mirror + (size_t)slots[i] * sizeof(T);
        if (values) memcpy(entry, (const uint8_t*)values + (size_t)i * words * 4, (size_t)words * 4);
        settle(i, entry);
        if (w.with_flags) p->flags.h[(size_t)slots[i]] = w.flags ? w.flags[i] : 0;
        if (w.hw) *w.hw = std::max(*w.hw, slots[i] + 1);
    }
    uint8_t* staged = blk.host<uint8_t>(i_values); uint8_t* fl = blk.host<uint8_t>(i_flags);
    for (int i = 0; i < n; ++i) {
        memcpy(staged + (size_t)i * words * 4, mirror + (size_t)slots[i] * sizeof(T), (size_t)words * 4);
        if (w.with_flags) fl[i] = p->flags.h[(size_t)slots[i]];
    }
    blk.publish();
    hipLaunchKernelGGL(k_map_put_words, dim3(blocks_of((long long)n * words)), dim3(MAP_BLOCK), 0, m->stream, blk.dev<uint32_t>(i_values),
                       blk.dev<int32_t>(i_slots), n, words, (int)(sizeof(T) / 4), w.offset, (uint32_t*)col.d.p);
    if (w.with_flags)
        hipLaunchKernelGGL(k_map_put_flags, dim3(blocks_of(n)), dim3(MAP_BLOCK), 0, m->stream, blk.dev<uint8_t>(i_flags),
                           blk.dev<int32_t>(i_slots), n, p->flags.d.p);
    MORB_HIP(hipGetLastError());
    MORB_HIP(hipStreamSynchronize(m->stream));
    return ORB_OK;
}

// One caller array of slots as the whole staged block of a call: copied, published, *dev its device address.
int stage_slots(orbm_map* p, const int32_t* v, int n, const int32_t** dev) {
    int rc;
    StagePack pk;
    const int i = pk.add(v, (size_t)n * 4);
    const StagePack::Block blk = pk.open(p->stage, &rc);
    if (rc) return rc;
    blk.publish();
    *dev = blk.dev<int32_t>(i);
    return ORB_OK;
}

// The ordered claim over a list of keyframe slots (UpdateLocalPoints' and CorrectLoop's "the first keyframe that holds a point takes
// it"): block b covers the features [256 (b % bpk), +256) of listed keyframe b / bpk.  The shape comes from the mirror's row lengths.
// reserve() goes with the caller's other reserves, before anything is enqueued; enqueue() leaves the least key of every point in
// `first` and the exclusive prefix sums of the kept candidates in d_block, their total in d_total / h_total, for the scatter of the
// caller (k_map_scatter, k_map_correct_scatter) to place them.
struct Claim {
    long long cand = 0;              // row entries of the listed keyframes
    int fmax = 0, bpk = 0, nb = 0;   // the longest row, blocks per keyframe, blocks
    Claim(const orbm_map* p, const int32_t* kfs, int n) {
        for (int j = 0; j < n; ++j) { const int c = p->kf_count.h[(size_t)kfs[j]]; cand += c; fmax = std::max(fmax, c); }
        bpk = (fmax + MAP_BLOCK - 1) / MAP_BLOCK; nb = n * bpk;
    }
    int reserve(orbm_map* p) const { return p->d_block.reserve((size_t)nb); }
    void enqueue(orbm_matcher* m, orbm_map* p, const int32_t* d_kfs, uint32_t epoch) const {
        hipLaunchKernelGGL(k_map_first, dim3(nb), dim3(MAP_BLOCK), 0, m->stream, (const int32_t*)p->kf_rows.d.p, (const int32_t*)p->kf_count.d.p,
                           d_kfs, p->stride, bpk, (const uint8_t*)p->flags.d.p, p->first.d.p, epoch);
        hipLaunchKernelGGL(k_map_count, dim3(nb), dim3(MAP_BLOCK), 0, m->stream, (const int32_t*)p->kf_rows.d.p, (const int32_t*)p->kf_count.d.p,
                           d_kfs, p->stride, bpk, (const uint8_t*)p->flags.d.p, (const unsigned long long*)p->first.d.p, epoch, p->d_block.p);
        hipLaunchKernelGGL(k_map_scan, dim3(1), dim3(MAP_SCAN_LANES), 0, m->stream, p->d_block.p, nb, p->d_total.p, p->h_total.dp);
    }
};

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
    size_t count[N_DOMAINS] = {};
    count[POINTS] = (size_t)point_capacity; count[RECORDS] = (size_t)obs_capacity; count[KEYFRAMES] = (size_t)kf_capacity;
    count[FEATURES] = (size_t)kf_capacity * (size_t)features_per_keyframe; count[LIST] = ORBM_MAX_POINTS; count[FEW] = 4;
    // empty on both sides: rows of zeros that are not bad, free records, keyframes without points, clean scratch
    int rc = ORB_OK;
    for (MapBuffer* b : p->all)
        if ((rc = b->create(count, m->stream))) break;
    if (!rc && hipStreamSynchronize(m->stream) != hipSuccess) { morb::set_error("clearing the resident map failed"); rc = ORB_E_HIP; }
    if (rc) { orbm_map_destroy(p); return rc; }
    *out = p;
    return ORB_OK;
}

void orbm_map_destroy(orbm_map* p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    for (MapBuffer* b : p->all) b->release();
    delete p;
}

int orbm_map_keyframes(const orbm_map* p) { return p ? p->kf_hw : ORB_E_ARG; }

int orbm_map_keyframe_bad(const orbm_map* p, int kf) {
    MORB_ARG(p && kf >= 0 && kf < p->kf_cap);
    return p->kf_bad.h[(size_t)kf];
}

int orbm_debug_last_local_map(const orbm_map* p, int* out4) { return copy_last(p, &orbm_map::last, out4); }

int orbm_map_write_points(orbm_matcher* m, orbm_map* p, const int32_t* slots, int n, const orbm_point* rows, const uint8_t* flags) {
    MORB_ARG(m && p && p->owner == m && n >= 0 && (n == 0 || (slots && rows)));
    static_assert(sizeof(orbm_point) == 68, "orbm_point is 17 words");
    SlotWrite w{"point slot", &p->pt_hw};
    w.with_flags = true; w.flags = flags;
    return write_slots<17>(m, p, p->rows, slots, n, rows, w);
}

int orbm_map_write_observations(orbm_matcher* m, orbm_map* p, const int32_t* slots, int n, const orbm_obs* records) {
    MORB_ARG(m && p && p->owner == m && n >= 0 && (n == 0 || (slots && records)));
    auto check_records = [&]() {
        for (int i = 0; i < n; ++i) {
            if (records[i].point < 0) continue;
            if (records[i].point >= p->pt_cap || records[i].keyframe < 0 || records[i].keyframe >= p->kf_cap) {
                morb::set_error("record %d names point %d, keyframe %d: outside the map (%d points, %d keyframes)", i, records[i].point,
                                records[i].keyframe, p->pt_cap, p->kf_cap);
                return (int)ORB_E_CAPACITY;
            }
        }
        return (int)ORB_OK;
    };
    auto settle = [&](int i, void* entry) {
        if (records[i].point < 0) memset(entry, 0xff, sizeof(orbm_obs));   // one form of a free record: {-1, -1}
        else p->kf_hw = std::max(p->kf_hw, records[i].keyframe + 1);
        p->index_dirty = true;   // the chain from a point to its records is rebuilt by the next counting call
    };
    return write_slots<2>(m, p, p->obs, slots, n, records, SlotWrite{"record slot", &p->obs_hw}, check_records, settle);
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
    int32_t* row = p->kf_rows.h.data() + (size_t)kf * p->stride;
    for (int f = 0; f < n_features; ++f) row[f] = point_of_feature[f] < 0 ? -1 : point_of_feature[f];
    for (int f = n_features; f < p->stride; ++f) row[f] = -1;
    // the old row's tail is dead once the count says so: send what the new count covers, and the count
    const int n_send = std::max(n_features, 1);
    p->kf_count.h[(size_t)kf] = n_features; p->kf_bad.h[(size_t)kf] = bad ? 1 : 0;
    p->kf_hw = std::max(p->kf_hw, kf + 1);
    MORB_HIP(hipMemcpyAsync(p->kf_rows.d.p + (size_t)kf * p->stride, row, (size_t)n_send * 4, hipMemcpyHostToDevice, m->stream));
    MORB_HIP(hipMemcpyAsync(p->kf_count.d.p + kf, &p->kf_count.h[(size_t)kf], 4, hipMemcpyHostToDevice, m->stream));
    MORB_HIP(hipStreamSynchronize(m->stream));
    return ORB_OK;
}

int orbm_map_set_keyframe_bad(orbm_matcher* m, orbm_map* p, int kf, int bad) {
    MORB_ARG(m && p && p->owner == m && kf >= 0 && kf < p->kf_cap);
    p->kf_bad.h[(size_t)kf] = bad ? 1 : 0;
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
        return orbm_local_map_vote_host(p->obs.h.data(), p->obs_hw, p->flags.h.data(), p->pt_cap, frame_points, n_features, nk, votes);
    }
    p->last[0] = 1;
    if (nk == 0) return ORB_OK;
    if (n_features == 0 || p->obs_hw == 0) { for (int k = 0; k < nk; ++k) votes[k] = 0; return ORB_OK; }
    MORB_HIP(hipSetDevice(m->device));
    int rc;
    const int32_t* d_fp;
    if ((rc = stage_slots(p, frame_points, n_features, &d_fp))) return rc;
    const unsigned g = blocks_of(std::max(n_features, nk));
    hipLaunchKernelGGL(k_map_mult, dim3(g), dim3(MAP_BLOCK), 0, m->stream, d_fp, n_features, (const uint8_t*)p->flags.d.p, p->mult.d.p,
                       p->d_votes.p, nk);
    const long long per_block = (long long)MAP_BLOCK * MAP_VOTE_PER_LANE;
    const unsigned gv = (unsigned)std::min<long long>(MAP_VOTE_MAX_BLOCKS, (p->obs_hw + per_block - 1) / per_block);
    hipLaunchKernelGGL(k_map_vote, dim3(gv), dim3(MAP_BLOCK), (size_t)nk * sizeof(int32_t), m->stream, (const orbm_obs*)p->obs.d.p, p->obs_hw,
                       (const int32_t*)p->mult.d.p, p->d_votes.p, nk);
    hipLaunchKernelGGL(k_map_vote_out, dim3(g), dim3(MAP_BLOCK), 0, m->stream, d_fp, n_features, p->mult.d.p, (const int32_t*)p->d_votes.p, nk,
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
    const Claim claim(p, local_kfs, n_local);
    p->last[2] = (int)std::min<long long>(claim.cand, 0x7fffffff); p->last[3] = 0;
    p->list.resize(ORBM_MAX_POINTS);
    int n = 0;
    if (m->host_resolve) {   // MORB_HOST_RESOLVE=1: the host routine over the mirror (the list still goes to HBM for the search's kernels)
        p->last[0] = 0;
        rc = orbm_local_map_points_host(p->kf_rows.h.data(), p->kf_count.h.data(), p->kf_hw, p->stride, p->flags.h.data(), p->pt_cap,
                                        local_kfs, n_local, p->list.data(), ORBM_MAX_POINTS, &n);
        if (rc) return rc;
    } else {
        p->last[0] = 1;
        if (claim.fmax > 0) {
            MORB_HIP(hipSetDevice(m->device));
            const int32_t* d_kfs;
            if ((rc = stage_slots(p, local_kfs, n_local, &d_kfs)) || (rc = claim.reserve(p)) || (rc = next_epoch(m, p))) return rc;
            claim.enqueue(m, p, d_kfs, p->epoch);
            hipLaunchKernelGGL(k_map_scatter, dim3(claim.nb), dim3(MAP_BLOCK), 0, m->stream, (const int32_t*)p->kf_rows.d.p,
                               (const int32_t*)p->kf_count.d.p, d_kfs, p->stride, claim.bpk, (const uint8_t*)p->flags.d.p,
                               (const unsigned long long*)p->first.d.p, p->epoch, (const int32_t*)p->d_block.p, p->d_list.p, p->h_list.dp,
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
        if (s >= 0 && !(p->flags.h[(size_t)s] & ORBM_POINT_BAD)) p->mark.h[(size_t)s] = p->epoch;
    }
    for (int i = 0; i < S->n_seen; ++i)
        if (S->seen[i] >= 0) p->mark.h[(size_t)S->seen[i]] = p->epoch;
    for (int i = 0; i < p->list_n; ++i) {
        const size_t s = (size_t)p->list[(size_t)i];
        out[i] = ((p->flags.h[s] & ORBM_POINT_BAD) || p->mark.h[s] == p->epoch) ? 1 : 0;
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
    S.d_rows = p->rows.d.p; S.h_rows = p->rows.h.data(); S.d_index = p->d_list.p; S.h_index = p->list.data();
    S.d_mark = p->mark.d.p; S.d_flags = p->flags.d.p; S.epoch = p->epoch; S.host_skip = host_skip; S.host_skip_ctx = &sc;
    if (!m->host_resolve && n > 0 && n_features + n_seen > 0) {
        StagePack pk;
        const int i_fp = pk.add(frame_points, (size_t)n_features * 4), i_seen = pk.add(seen, (size_t)n_seen * 4);
        const StagePack::Block blk = pk.open(p->stage, &rc);
        if (rc) return rc;
        blk.publish();
        hipLaunchKernelGGL(k_map_mark, dim3(blocks_of((long long)n_features + n_seen)), dim3(MAP_BLOCK), 0, m->stream,
                           blk.dev<int32_t>(i_fp), n_features, blk.dev<int32_t>(i_seen), n_seen, (const uint8_t*)p->flags.d.p, p->mark.d.p,
                           p->epoch);
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
    int rc;
    if ((rc = p->head.clear(m->stream))) return rc;
    if (p->obs_hw > 0)
        hipLaunchKernelGGL(k_map_chain, dim3(blocks_of(p->obs_hw)), dim3(MAP_BLOCK), 0, m->stream, (const orbm_obs*)p->obs.d.p, p->obs_hw,
                           p->head.d.p, p->next.d.p);
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

int orbm_debug_last_covisibility(const orbm_map* p, int* out4) { return copy_last(p, &orbm_map::last_cov, out4); }

int orbm_map_write_observation_features(orbm_matcher* m, orbm_map* p, const int32_t* slots, int n, const int32_t* feature) {
    MORB_ARG(m && p && p->owner == m && n >= 0 && (n == 0 || (slots && feature)));
    return write_slots<1>(m, p, p->obs_feat, slots, n, feature, SlotWrite{"record slot"},
                          [&]() { return check_slots(feature, n, 0, p->stride, "feature index"); });
}

int orbm_map_write_point_nobs(orbm_matcher* m, orbm_map* p, const int32_t* slots, int n, const int32_t* n_obs) {
    MORB_ARG(m && p && p->owner == m && n >= 0 && (n == 0 || (slots && n_obs)));
    return write_slots<1>(m, p, p->nobs, slots, n, n_obs, SlotWrite{"point slot"});
}

int orbm_map_write_keyframe_features(orbm_matcher* m, orbm_map* p, int kf, const uint8_t* feature_bytes, int n_features, int n_cam1) {
    MORB_ARG(m && p && p->owner == m && n_features >= 0 && (n_features == 0 || feature_bytes) && n_cam1 >= 0);
    if (kf < 0 || kf >= p->kf_cap || n_features > p->stride || n_cam1 > p->stride) {
        morb::set_error("keyframe slot %d with %d features, %d of camera 1, does not fit a map of %d keyframes of %d", kf, n_features, n_cam1,
                        p->kf_cap, p->stride);
        return kf < 0 ? ORB_E_ARG : ORB_E_CAPACITY;
    }
    MORB_HIP(hipSetDevice(m->device));
    uint8_t* row = p->kf_feat.h.data() + (size_t)kf * p->stride;
    if (n_features) memcpy(row, feature_bytes, (size_t)n_features);
    memset(row + n_features, 0, (size_t)(p->stride - n_features));
    p->kf_ncam1.h[(size_t)kf] = n_cam1;
    // the whole row travels: a record of another keyframe's point may name any feature of this one
    MORB_HIP(hipMemcpyAsync(p->kf_feat.d.p + (size_t)kf * p->stride, row, (size_t)p->stride, hipMemcpyHostToDevice, m->stream));
    MORB_HIP(hipMemcpyAsync(p->kf_ncam1.d.p + kf, &p->kf_ncam1.h[(size_t)kf], 4, hipMemcpyHostToDevice, m->stream));
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
        rc = orbm_local_map_covisibility_host(p->obs.h.data(), p->obs_feat.h.data(), p->obs_hw, p->flags.h.data(), p->pt_cap, p->kf_rows.h.data(),
                                              p->kf_count.h.data(), p->kf_ncam1.h.data(), p->kf_hw, p->stride, kfs, n, first_out, tmp.data(),
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
    const int32_t* d_kfs;
    if ((rc = stage_slots(p, kfs, n, &d_kfs)) || (rc = p->h_span.reserve((size_t)n * 2)) ||
        (rc = p->h_entries.reserve((size_t)std::max(entries_cap, 1)))) return rc;
    MORB_HIP(hipMemsetAsync(p->d_cursor.p, 0, sizeof(int32_t), m->stream));
    const int nk = p->kf_hw;
    hipLaunchKernelGGL(k_map_covis, dim3(n), dim3(MAP_BLOCK), ((size_t)nk + MAP_BLOCK / 64 + 1) * sizeof(int32_t), m->stream,
                       d_kfs, (const int32_t*)p->kf_rows.d.p, (const int32_t*)p->kf_count.d.p,
                       (const int32_t*)p->kf_ncam1.d.p, p->stride, (const uint8_t*)p->flags.d.p, (const orbm_obs*)p->obs.d.p,
                       (const int32_t*)p->obs_feat.d.p, (const int32_t*)p->head.d.p, (const int32_t*)p->next.d.p, nk, p->d_cursor.p,
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
        return orbm_local_map_culling_host(p->obs.h.data(), p->obs_feat.h.data(), p->obs_hw, p->flags.h.data(), p->nobs.h.data(), p->pt_cap,
                                           p->kf_rows.h.data(), p->kf_count.h.data(), p->kf_feat.h.data(), p->kf_hw, p->stride, kfs, n, mono,
                                           counts_out);
    }
    p->last_cov[0] = 1;
    MORB_HIP(hipSetDevice(m->device));
    if ((rc = build_index_if_dirty(m, p))) return rc;
    if (n == 0) { MORB_HIP(hipStreamSynchronize(m->stream)); return ORB_OK; }
    const int32_t* d_kfs;
    if ((rc = stage_slots(p, kfs, n, &d_kfs)) || (rc = p->h_counts.reserve((size_t)n * 2))) return rc;
    hipLaunchKernelGGL(k_map_cull, dim3(n), dim3(MAP_BLOCK), 0, m->stream, d_kfs, (const int32_t*)p->kf_rows.d.p,
                       (const int32_t*)p->kf_count.d.p, (const uint8_t*)p->kf_feat.d.p, p->stride, (const uint8_t*)p->flags.d.p,
                       (const int32_t*)p->nobs.d.p, (const orbm_obs*)p->obs.d.p, (const int32_t*)p->obs_feat.d.p, (const int32_t*)p->head.d.p,
                       (const int32_t*)p->next.d.p, mono ? 1 : 0, p->h_counts.dp);
    MORB_HIP(hipGetLastError());
    MORB_HIP(hipStreamSynchronize(m->stream));
    memcpy(counts_out, p->h_counts.p, (size_t)n * 2 * sizeof(int32_t));
    return ORB_OK;
}

// ---- loop correction over the resident map (kernels: mapcorrect_dev.h)

namespace {

constexpr int POS_STRIDE_ROWS = (int)(sizeof(orbm_point) / sizeof(float));   // the mirror's rows as a strided array of positions
static_assert(offsetof(orbm_point, pos) == 0 && sizeof(orbm_point) % sizeof(float) == 0, "a row begins with its position");

// The positions of the listed slots as the mirror holds them into their rows in HBM, and the stream synchronised (an empty list
// included): how the host routes of both corrections end, once the host routine has moved the mirror's points.
int put_positions(orbm_matcher* m, orbm_map* p, const int32_t* slots, int n) {
    if (n == 0) { MORB_HIP(hipStreamSynchronize(m->stream)); return ORB_OK; }
    return write_slots<3>(m, p, p->rows, slots, n, nullptr, SlotWrite{"point slot"});
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

int orbm_debug_last_correction(const orbm_map* p, int* out4) { return copy_last(p, &orbm_map::last_cor, out4); }

int orbm_debug_map_read_points(orbm_matcher* m, orbm_map* p, const int32_t* slots, int n, orbm_point* rows) {
    MORB_ARG(m && p && p->owner == m && n >= 0 && (n == 0 || (slots && rows)));
    int rc;
    if ((rc = check_slots(slots, n, 0, p->pt_cap, "point slot"))) return rc;
    if (n == 0) return ORB_OK;
    MORB_HIP(hipSetDevice(m->device));
    const int lo = *std::min_element(slots, slots + n), hi = *std::max_element(slots, slots + n);
    std::vector<orbm_point> span((size_t)(hi - lo + 1));
    MORB_HIP(hipMemcpyAsync(span.data(), p->rows.d.p + lo, span.size() * sizeof(orbm_point), hipMemcpyDeviceToHost, m->stream));
    MORB_HIP(hipStreamSynchronize(m->stream));
    for (int i = 0; i < n; ++i) rows[i] = span[(size_t)(slots[i] - lo)];
    return ORB_OK;
}

int orbm_map_write_positions(orbm_matcher* m, orbm_map* p, const int32_t* slots, int n, const float* pos3) {
    MORB_ARG(m && p && p->owner == m && n >= 0 && (n == 0 || (slots && pos3)));
    return write_slots<3>(m, p, p->rows, slots, n, pos3, SlotWrite{"point slot", &p->pt_hw});
}

int orbm_map_write_point_ref(orbm_matcher* m, orbm_map* p, const int32_t* slots, int n, const int32_t* ref_kf) {
    MORB_ARG(m && p && p->owner == m && n >= 0 && (n == 0 || (slots && ref_kf)));
    return write_slots<1>(m, p, p->ref, slots, n, ref_kf, SlotWrite{"point slot", &p->pt_hw});
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
    const Claim claim(p, kfs, n);
    p->last_cor[1] = (int)std::min<long long>(claim.cand, 0x7fffffff); p->last_cor[2] = 0; p->last_cor[3] = n;
    MORB_HIP(hipSetDevice(m->device));
    if (m->host_resolve) {   // MORB_HOST_RESOLVE=1: the host routine over the mirror, the new positions then sent to their rows
        p->last_cor[0] = 0;
        rc = orbm_local_map_correct_sim3_host(p->kf_rows.h.data(), p->kf_count.h.data(), p->kf_hw, p->stride, p->flags.h.data(),
                                              p->pt_cap ? p->rows.h[0].pos : nullptr, POS_STRIDE_ROWS, p->pt_cap, kfs, n, sim3_before,
                                              sim3_after, already, n_already, entries, pos_out, cap, n_out, Tiw_out);
        if (rc) return rc;
        p->last_cor[2] = *n_out;
        std::vector<int32_t> moved((size_t)*n_out);
        for (int i = 0; i < *n_out; ++i) moved[(size_t)i] = entries[i].point;
        return put_positions(m, p, moved.data(), *n_out);
    }
    p->last_cor[0] = 1;
    for (int j = 0; j < n; ++j) eg_Tiw(sim3_after + 8 * (size_t)j, Tiw_out + 16 * (size_t)j);   // :714-720
    if (claim.fmax == 0) return ORB_OK;
    const int n_launch = (int)std::min<long long>(cap, claim.cand);
    StagePack pk;
    const int i_kfs = pk.add(kfs, (size_t)n * 4), i_table = pk.add_in_place((size_t)n * MAP_SIM3_TABLE * sizeof(double));
    const int i_already = pk.add(already, (size_t)n_already * 4);
    const StagePack::Block blk = pk.open(p->stage, &rc);
    if (rc || (rc = claim.reserve(p)) || (rc = p->d_centries.reserve((size_t)std::max(n_launch, 1))) ||
        (rc = p->h_centries.reserve((size_t)std::max(n_launch, 1))) || (rc = p->h_cpos.reserve((size_t)std::max(n_launch, 1) * 3))) return rc;
    // two epochs: the claim's, and a NEWER one for the points already corrected -- a newer key is smaller than every key of the claim
    uint32_t e_claim, e_skip;
    do {
        if ((rc = next_epoch(m, p))) return rc;
        e_claim = p->epoch;
        if ((rc = next_epoch(m, p))) return rc;
        e_skip = p->epoch;
    } while (e_skip < e_claim);   // (the counter wrapped in between: both again)
    double entry[MAP_SIM3_TABLE];   // (built here, not in the stage: the host only ever stores to that memory)
    for (int j = 0; j < n; ++j) {
        map_sim3_table_entry(sim3_before + 8 * (size_t)j, sim3_after + 8 * (size_t)j, entry);
        memcpy(blk.host<double>(i_table) + (size_t)MAP_SIM3_TABLE * j, entry, sizeof(entry));
    }
    blk.publish();
    const int32_t* d_kfs = blk.dev<int32_t>(i_kfs);
    if (n_already)
        hipLaunchKernelGGL(k_map_stamp, dim3(blocks_of(n_already)), dim3(MAP_BLOCK), 0, m->stream, blk.dev<int32_t>(i_already), n_already,
                           p->first.d.p, map_key(e_skip, 0));
    claim.enqueue(m, p, d_kfs, e_claim);
    hipLaunchKernelGGL(k_map_correct_scatter, dim3(claim.nb), dim3(MAP_BLOCK), 0, m->stream, (const int32_t*)p->kf_rows.d.p,
                       (const int32_t*)p->kf_count.d.p, d_kfs, p->stride, claim.bpk, (const uint8_t*)p->flags.d.p,
                       (const unsigned long long*)p->first.d.p, e_claim, (const int32_t*)p->d_block.p, (const int32_t*)p->d_total.p,
                       p->d_centries.p, p->h_centries.dp, n_launch);
    if (n_launch > 0)
        hipLaunchKernelGGL(k_map_correct_sim3, dim3(blocks_of(n_launch)), dim3(MAP_BLOCK), 0, m->stream,
                           (const orbm_correct_entry*)p->d_centries.p, n_launch, (const int32_t*)p->d_total.p, n_launch,
                           blk.dev<double>(i_table), p->rows.d.p, p->h_cpos.dp);
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
        memcpy(p->rows.h[(size_t)entries[i].point].pos, p->h_cpos.p + 3 * (size_t)i, 12);
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
        rc = orbm_local_map_correct_rigid_host(p->pt_cap ? p->rows.h[0].pos : nullptr, POS_STRIDE_ROWS, p->flags.h.data(), p->ref.h.data(),
                                               p->pt_cap, slots, n, kf_corrected, Tcw_before, Twc_after, n_kfs, gba_slots, gba_pos, n_gba,
                                               st.data(), pos_out);
        if (rc) return rc;
        std::vector<int32_t> moved;
        for (int i = 0; i < n; ++i)
            if (st[(size_t)i]) moved.push_back(slots ? slots[i] : i);
        p->last_cor[2] = (int)moved.size();
        if (status) memcpy(status, st.data(), (size_t)n);
        return put_positions(m, p, moved.data(), (int)moved.size());
    }
    p->last_cor[0] = 1;
    if (n == 0) return ORB_OK;
    StagePack pk;
    const int i_slots = pk.add(slots, slots ? (size_t)n * 4 : 0), i_flag = pk.add(kf_corrected, (size_t)n_kfs);
    const int i_table = pk.add_in_place((size_t)n_kfs * MAP_RIGID_TABLE * sizeof(float));
    const int i_gslots = pk.add(gba_slots, (size_t)n_gba * 4), i_gpos = pk.add(gba_pos, (size_t)n_gba * 12);
    const StagePack::Block blk = pk.open(p->stage, &rc);
    if (rc || (rc = p->h_cstatus.reserve((size_t)n)) || (rc = p->h_cpos.reserve((size_t)n * 3)) || (rc = next_epoch(m, p))) return rc;
    rigid_table(Tcw_before, Twc_after, n_kfs, blk.host<float>(i_table));
    blk.publish();
    if (n_gba)
        hipLaunchKernelGGL(k_map_stamp_last, dim3(blocks_of(n_gba)), dim3(MAP_BLOCK), 0, m->stream, blk.dev<int32_t>(i_gslots), n_gba,
                           p->first.d.p, p->epoch);
    hipLaunchKernelGGL(k_map_correct_rigid, dim3(std::min<unsigned>(blocks_of(n), MAP_RIGID_MAX_BLOCKS)), dim3(MAP_BLOCK), 0, m->stream,
                       slots ? blk.dev<int32_t>(i_slots) : (const int32_t*)nullptr, n, p->rows.d.p, (const uint8_t*)p->flags.d.p,
                       (const int32_t*)p->ref.d.p, blk.dev<uint8_t>(i_flag), blk.dev<float>(i_table), n_kfs,
                       (const unsigned long long*)p->first.d.p, p->epoch, blk.dev<float>(i_gpos), p->h_cstatus.dp, p->h_cpos.dp);
    MORB_HIP(hipGetLastError());
    MORB_HIP(hipStreamSynchronize(m->stream));
    int changed = 0;
    for (int i = 0; i < n; ++i) {
        float* P = p->rows.h[(size_t)(slots ? slots[i] : i)].pos;
        if (p->h_cstatus.p[i]) { memcpy(P, p->h_cpos.p + 3 * (size_t)i, 12); ++changed; }
        if (pos_out) memcpy(pos_out + 3 * (size_t)i, P, 12);
    }
    if (status) memcpy(status, p->h_cstatus.p, (size_t)n);
    p->last_cor[2] = changed;
    return ORB_OK;
}
