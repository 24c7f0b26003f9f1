// NewMapPoints.h -- the loop over the matched pairs in LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:388-669) for all
// pairs of one neighbour in one call: parallax test, linear triangulation or stereo unprojection, depth, reprojection and scale gates.
//
// The reference runs the loop body once per pair, about thirty cv::Mat temporaries each, for up to fifteen neighbours of every new
// keyframe.  TriangulateMatches below replaces the body up to, but not including, `new MapPoint`: it flattens the two keyframes, hands
// the pairs to orbv_triangulate_pairs (include/orbv.h; one lane per pair) and returns, per pair, the verdict and x3D.  The caller keeps
// its `new MapPoint` / AddObservation / AddMapPoint lines and hands the new points to RefreshMapPoints (host/MapPointRefresh.h).
// INTEGRATION.md shows the lines it replaces.
//
// CreateNewPointsOfKeyFrame replaces the neighbour loop itself (:315-690 up to `new MapPoint`): the baseline tests and istrian of every
// neighbour, then SearchForTriangulation and the pair loop of ALL neighbours in one device call with one synchronisation
// (orbv_create_new_points_keyframe), out of keyframes that stay resident in HBM (ResidentKeyFrames).  Between two neighbours the
// reference gives the accepted features of the current keyframe their map point (AddMapPoint, :682) and the next search skips them; the
// device keeps that bit itself.
// ONE DEVIATION from the reference: it abandons the remaining neighbours when CheckNewKeyFrames() turns true between two of them (:318).
// One enqueue cannot do that: the caller checks before the call and gets all neighbours.  A caller who needs the abort keeps its loop
// and calls TriangulateMatches per neighbour.
#ifndef NEWMAPPOINTS_H
#define NEWMAPPOINTS_H

#include <cstddef>
#include <utility>
#include <vector>
#include "ORBmatcher.h"

namespace ORB_SLAM2 {

struct TriangulatedPair {
    bool accepted = false;   // the pair reached `new MapPoint`
    int outcome = 0;         // ORBV_TRI_* (include/orbv.h): which exit of the loop body the pair took
    cv::Mat x3D;             // 3x1 CV_32F; empty when no point was computed
};

// vMatchedIndices: what SearchForTriangulation filled; istrian: the per-camera baseline verdict of :338-341.  out[ikp] belongs to
// vMatchedIndices[ikp].  Batches of fewer than TRIANGULATE_HOST_BELOW pairs are computed by the library's host routine (the same
// statements, no launch).  Returns false -- reported as every search of ORBmatcher reports a failure, out left empty -- when the
// library refuses the call.
bool TriangulateMatches(ORBmatcher& matcher, KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<std::pair<size_t, size_t> >& vMatchedIndices,
                        const std::vector<bool>& istrian, std::vector<TriangulatedPair>& out);

// The keyframes of the calling thread that are resident in HBM for the BoW-gated searches and the triangulation stage: KeyFrame* ->
// orbv_keyframe*.  An entry is created with orbv_keyframe_create + orbv_keyframe_set_geometry from the members SearchForTriangulation
// and TriangulateMatches flatten (descriptors, angles, FeatureVector, keypoints, right coordinates, depths).  The poses are NOT cached:
// they travel with every call.  Nothing is taken on trust: an entry is reused only while the keyframe's feature count and mnId are the
// ones it was built from (an address can be reused by another keyframe).  Bounded, least recently used out first; Forget(pKF) belongs
// where the integration calls KeyFrame::SetBadFlag.  One instance per thread (OfThread), as the matcher's device state is.
class ResidentKeyFrames {
public:
    explicit ResidentKeyFrames(size_t capacity = 40) : mCapacity(capacity) {}
    ~ResidentKeyFrames() { Clear(); }
    ResidentKeyFrames(const ResidentKeyFrames&) = delete;
    ResidentKeyFrames& operator=(const ResidentKeyFrames&) = delete;
    static ResidentKeyFrames& OfThread();
    // The resident form of pKF, created when there is none or the one there was built from another keyframe.  An entry used in this
    // call is the most recent one, so up to Capacity() keyframes obtained in a row stay valid together.  ok (may be NULL) reports
    // failure; without a device (dry run) the return value is NULL on success too.
    orbv_keyframe* Get(ORBmatcher& matcher, KeyFrame* pKF, bool* ok = nullptr);
    void Forget(KeyFrame* pKF);
    void Clear();
    void Reserve(size_t capacity) { if (capacity > mCapacity) mCapacity = capacity; }
    size_t Capacity() const { return mCapacity; }
    size_t Size() const { return mEntries.size(); }
    bool Holds(KeyFrame* pKF) const;
    unsigned long Created() const { return mCreated; }
    unsigned long Reused() const { return mReused; }
    unsigned long Evicted() const { return mEvicted; }
    // test hook: flatten and keep the books, create nothing on the device (a process without a device can check both)
    bool mbDryRun = false;

private:
    struct Entry { KeyFrame* pKF; unsigned long id; size_t n; orbv_keyframe* handle; unsigned long stamp; };
    std::vector<Entry> mEntries;
    size_t mCapacity;
    unsigned long mClock = 0, mCreated = 0, mReused = 0, mEvicted = 0;
};

// One neighbour that passed the baseline tests (:323-351), in the order of vpNeighKFs.
struct NewPointsRoundPlan {
    KeyFrame* pKF2 = nullptr;
    float baseline = 0, baseline_cam2 = 0;
    std::vector<bool> istrian;
};
// :315-351 statement by statement, the search and the pair loop left out: the two baselines with cv::norm, the `continue` when both
// are below pKF2->mb, istrian.  In this fork the monocular branch never sets istrian, so :351 skips every neighbour whatever
// ComputeSceneMedianDepth returns: under bMonocular no neighbour is planned.
void PlanNewPointsRounds(KeyFrame* pKF1, const std::vector<KeyFrame*>& vpNeighKFs, bool bMonocular, std::vector<NewPointsRoundPlan>& rounds);

struct NeighbourPoints {
    KeyFrame* pKF2 = nullptr;
    std::vector<std::pair<size_t, size_t> > vMatchedIndices;   // what SearchForTriangulation fills for this neighbour
    std::vector<TriangulatedPair> pairs;                        // pairs[ikp] belongs to vMatchedIndices[ikp]
};
// The neighbour loop of CreateNewMapPoints for pKF1 = mpCurrentKeyFrame up to `new MapPoint`: out holds, in the order of vpNeighKFs,
// the neighbours that were not skipped.  The caller walks out[k].pairs and keeps `new MapPoint` ... mlpRecentAddedMapPoints.push_back
// for the accepted ones -- a feature of pKF1 is accepted for at most one neighbour, as in the reference.  Uses the matcher's
// mbCheckOrientation and TH_LOW.  Returns false -- reported as every search of ORBmatcher reports a failure, out left empty -- when the
// library refuses the call or there is no device.
bool CreateNewPointsOfKeyFrame(ORBmatcher& matcher, KeyFrame* pKF1, const std::vector<KeyFrame*>& vpNeighKFs, bool bMonocular,
                               std::vector<NeighbourPoints>& out);

// The batch size below which the host routine is used.  UNMEASURED placeholder until tools/triangulate_bench.py has run.
extern const int TRIANGULATE_HOST_BELOW;

}  // namespace ORB_SLAM2

#endif
