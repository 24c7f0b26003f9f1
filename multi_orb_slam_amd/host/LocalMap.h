// LocalMap.h -- Tracking::UpdateLocalMap (reference src/Tracking.cc:1794-1949) over a map that stays resident under stable slots,
// and Tracking::SearchLocalPoints (:1702-1770) over the list it leaves on the device.
//
// The reference counts the keyframe votes by copying pMP->GetObservations() for every feature of the frame, builds the point list by
// copying GetMapPointMatches() of every local keyframe, and host/LocalMapSearch.cc then packs every local point and compares it with
// the previous frame's table.  Here a ResidentMap holds every map point, keyframe and observation under a slot of its own
// (include/orbm.h: orbm_map); the threads that change the map say so (Touch), the tracking thread sends what changed (Flush), and
// per frame only the frame's own point slots and the local keyframes' slots travel: the votes are one stream over the observation
// records (orbm_map_vote), the point list a gather over the local keyframes' rows (orbm_map_local_points), the search reads the points
// through that list (orbm_map_search_local_points).  K1 in std::map order and the K2 walk with its marks are pointer logic over the
// covisibility graph: they stay here, statement by statement.  INTEGRATION.md shows the lines this replaces and lists every statement
// of the reference that needs a Touch.
#ifndef LOCALMAP_H
#define LOCALMAP_H

#include <cstdint>
#include <map>
#include <mutex>
#include <unordered_map>
#include <vector>
#include "../../include/orbm.h"
#include "ORBmatcher.h"

namespace ORB_SLAM2 {

class ResidentMap {
public:
    struct Capacity { int keyframes = 4096, points = 1 << 20, observations = 1 << 22, features_per_keyframe = 4096; };

    // matcher != NULL: the map lives in HBM on the handle of the thread that makes the first Flush (the tracking thread), created
    // there.  matcher == NULL: host-only -- no device is needed, UpdateLocalMap runs over the mirror through the library's two host
    // routines (orbm_local_map_vote_host, orbm_local_map_points_host); SearchLocalPoints needs the device.
    explicit ResidentMap(ORBmatcher* matcher);                 // the default capacities
    ResidentMap(ORBmatcher* matcher, const Capacity& capacity);
    ~ResidentMap();
    ResidentMap(const ResidentMap&) = delete;
    ResidentMap& operator=(const ResidentMap&) = delete;

    // The object changed (or is new): queue it.  Any thread; the objects are read later, by Flush, on the tracking thread, under
    // whatever lock the integration holds there (the reference's accessors take the objects' own mutexes).
    void Touch(MapPoint* pMP);
    void Touch(KeyFrame* pKF);
    // Tracking thread: re-reads every queued object -- a point's row bytes, flag and observations, a keyframe's point matches and flag
    // -- and sends what differs from the mirror, compared by bytes (the rule host/resident.h states), in one call per kind.  Returns
    // the number of rows, records and keyframes sent, or -1 after a failed device call (reported on stderr).
    int Flush();
    // Walks the whole host map, compares it with the mirror and returns the number of differences: an object without a slot, a row,
    // a flag, an observation set or a keyframe row that is not what the mirror holds.  0 after a Flush that followed every Touch the
    // integration owes; for tests and for integrators who forgot one.
    int Audit(const std::vector<KeyFrame*>& vpKeyFrames, const std::vector<MapPoint*>& vpMapPoints);

    bool HostOnly() const { return mpMatcher == nullptr; }
    // inspection (tests / bench): what the last Flush sent
    // (rows, records, keyframes: as ever.  The facts the covisibility and culling counts read beyond them (host/Covisibility.h):
    // record_features the records whose feature index was sent, point_nobs the points whose Observations() was, keyframe_features
    // the keyframes whose level / far bytes and camera-1 count were.  Flush's return value stays the sum of the first three.)
    // point_refs: the points whose reference keyframe slot was sent (host/LoopCorrection.h reads it on the device).
    struct FlushStats { int rows = 0, records = 0, keyframes = 0, record_features = 0, point_nobs = 0, keyframe_features = 0, point_refs = 0; };
    FlushStats LastFlush() const { return mLastFlush; }
    // inspection: orbm_debug_last_covisibility of the device map (all zero for a host-only map)
    void LastCovisibility(int out4[4]) const;
    // inspection: orbm_debug_last_correction of the device map (all zero for a host-only map)
    void LastCorrection(int out4[4]) const;

private:
    friend void UpdateLocalMap(ResidentMap&, Frame&, std::vector<KeyFrame*>&, std::vector<MapPoint*>&, KeyFrame*&);
    friend int SearchLocalPoints(ORBmatcher&, ResidentMap&, Frame&, std::vector<MapPoint*>&, float, int*);
    friend void CovisibilityCounts(ResidentMap&, const std::vector<KeyFrame*>&, std::vector<std::map<KeyFrame*, int> >&,
                                   std::vector<std::map<KeyFrame*, int> >&);
    friend void KeyFrameCulling(ResidentMap&, KeyFrame*, bool);
    friend struct LoopCorrectionAccess;   // CorrectLoopMap and UpdateMapAfterGlobalBA (host/LoopCorrection.cc)

    struct PointEntry { int slot; std::map<KeyFrame*, int> records; };   // the record slot of each observation the mirror holds
    int SlotOf(MapPoint* pMP);      // assigned on first sight; -1 when the map is full (reported)
    int SlotOf(KeyFrame* pKF);
    bool EnsureDevice();
    int Vote(const std::vector<int32_t>& frame_points, std::vector<int32_t>& votes);
    int LocalPoints(const std::vector<int32_t>& local_kfs, std::vector<int32_t>& list);
    // the slots of keyframes the map has been told of (one it has not is read now, as a Touch would have it); false after a failure
    bool SlotsOfSent(const std::vector<KeyFrame*>& vpKFs, size_t begin, size_t end, std::vector<int32_t>& slots);
    int Covisibility(const std::vector<int32_t>& kfs, std::vector<int32_t>& first, std::vector<orbm_covis_entry>& entries);
    int CullingCounts(const std::vector<int32_t>& kfs, bool mono, std::vector<int32_t>& counts);
    // the two corrections, on the device or over the mirror; either way the mirror's positions are the new ones afterwards
    int CorrectSim3(const std::vector<int32_t>& kfs, const std::vector<double>& before, const std::vector<double>& after,
                    const std::vector<int32_t>& already, std::vector<orbm_correct_entry>& entries, std::vector<float>& pos, std::vector<float>& Tiw);
    int CorrectRigid(const std::vector<int32_t>& slots, const std::vector<uint8_t>& kf_corrected, const std::vector<float>& Tcw_before,
                     const std::vector<float>& Twc_after, const std::vector<int32_t>& gba_slots, const std::vector<float>& gba_pos,
                     std::vector<uint8_t>& status, std::vector<float>& pos);

    // Everything that touches the device object or the slot tables runs under this: Flush, Audit, the calls of the tracking thread and
    // those of the LocalMapping / LoopClosing threads (an orbm_map is bound to one handle, and one call uses it at a time).
    std::recursive_mutex mMutexMap;

    ORBmatcher* mpMatcher;
    Capacity mCap;
    orbm_matcher* mpHandle = nullptr;
    orbm_map* mpMap = nullptr;
    bool mbFailed = false;

    std::mutex mMutexQueue;
    std::vector<MapPoint*> mvQueuedPoints;
    std::vector<KeyFrame*> mvQueuedKeyFrames;

    // slot tables and free lists
    std::unordered_map<MapPoint*, PointEntry> mPoints;
    std::unordered_map<KeyFrame*, int> mKeyFrames;
    std::vector<MapPoint*> mvPointOfSlot;
    std::vector<KeyFrame*> mvKeyFrameOfSlot;
    std::vector<int32_t> mvFreeRecords;
    // the mirror: what the device holds (device mode) / all there is (host-only), as the plain arrays of the host routines
    std::vector<orbm_point> mvRows;
    std::vector<uint8_t> mvFlags, mvKeyFrameBad, mvKeyFrameSent;
    std::vector<orbm_obs> mvRecords;
    std::vector<int32_t> mvKeyFrameRows, mvKeyFrameCount;   // mvKeyFrameRows[slot * features_per_keyframe + f]
    std::vector<int32_t> mvRecordFeature, mvPointNObs, mvKeyFrameNCam1;   // per record, per point slot, per keyframe slot
    std::vector<int32_t> mvPointRef;                        // per point slot: the keyframe slot of GetReferenceKeyFrame(), -1: none
    std::vector<uint8_t> mvKeyFrameFeatures;                // [slot * features_per_keyframe + f]: level | ORBM_FEATURE_FAR
    // the last point list (slots), what SearchLocalPoints searches
    std::vector<int32_t> mvList;
    FlushStats mLastFlush;
    // scratch
    std::vector<int32_t> mvFramePoints, mvVotes, mvLocalSlots, mvSeen, mvMatch;
    std::vector<uint8_t> mvSkip, mvOccupied;
    std::vector<orbm_track> mvTrack;
};

// Tracking::UpdateLocalMap's two halves (src/Tracking.cc:1832-1949, then :1794-1824) for the frame F, with the reference's observable
// effects: F.mvpMapPoints loses its bad points; vpLocalKeyFrames is K1 (ascending pointer order, bad keyframes dropped) followed by
// what the K2 walk adds; pReferenceKF and F.mpReferenceKF are the keyframe with the most votes (the first in pointer order on a tie);
// every mnTrackReferenceForFrame the reference writes is written; vpLocalMapPoints is the point list.  As in the reference, a frame
// whose points cast no vote leaves vpLocalKeyFrames and the reference keyframe as they are (:1857), and the point list is then
// rebuilt from that unchanged keyframe list.
// One deviation (include/orbm.h, orbm_map_local_points): a point whose mnTrackReferenceForFrame already is F.mnId when the call
// begins is listed all the same; the reference would leave it out (a second call for the same frame yields an empty list there).
// A failed device call, more than ORBM_MAP_MAX_LOCAL local keyframes or more than ORBM_MAX_POINTS local points are reported on
// stderr and leave an empty point list.
void UpdateLocalMap(ResidentMap& map, Frame& F, std::vector<KeyFrame*>& vpLocalKeyFrames, std::vector<MapPoint*>& vpLocalMapPoints,
                    KeyFrame*& pReferenceKF);

// SearchLocalPoints of host/LocalMapSearch.h with the same observable effects, over the list the last UpdateLocalMap left on the
// device: vpLocalMapPoints must be the vector that call filled.  No point is packed and none compared per frame: a point's row
// travels when Flush finds it changed.
int SearchLocalPoints(ORBmatcher& matcher, ResidentMap& map, Frame& F, std::vector<MapPoint*>& vpLocalMapPoints, float th,
                      int* nToMatch = nullptr);

}  // namespace ORB_SLAM2

#endif
