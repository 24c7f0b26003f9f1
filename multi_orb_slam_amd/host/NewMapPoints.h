// NewMapPoints.h -- the loop over the matched pairs in LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:388-669) for all
// pairs of one neighbour in one call: parallax test, linear triangulation or stereo unprojection, depth, reprojection and scale gates.
//
// The reference runs the loop body once per pair, about thirty cv::Mat temporaries each, for up to fifteen neighbours of every new
// keyframe.  TriangulateMatches below replaces the body up to, but not including, `new MapPoint`: it flattens the two keyframes, hands
// the pairs to orbv_triangulate_pairs (include/orbv.h; one lane per pair) and returns, per pair, the verdict and x3D.  The caller keeps
// its `new MapPoint` / AddObservation / AddMapPoint lines and hands the new points to RefreshMapPoints (host/MapPointRefresh.h).
// INTEGRATION.md shows the lines it replaces.
#ifndef NEWMAPPOINTS_H
#define NEWMAPPOINTS_H

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

// The batch size below which the host routine is used.  UNMEASURED placeholder until tools/triangulate_bench.py has run.
extern const int TRIANGULATE_HOST_BELOW;

}  // namespace ORB_SLAM2

#endif
