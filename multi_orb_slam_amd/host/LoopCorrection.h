// LoopCorrection.h -- the two passes of LoopClosing that move map points, over the resident map (host/LocalMap.h):
// LoopClosing::CorrectLoop's propagation of the loop's Sim3 (reference src/LoopClosing.cc:645-727) and the map update behind a global
// bundle adjustment (LoopClosing::RunGlobalBundleAdjustment, :925-989).
//
// The reference moves every point through a cv::Mat and two Eigen maps, one point at a time.  After either pass only the 12 position
// bytes of a corrected point's row differ from what the resident map holds, so the rows are corrected where they lie
// (include/orbm.h: orbm_map_correct_sim3, orbm_map_correct_rigid; the host routines for a map without a device) and no row crosses the
// bus for its position.  What is pointer logic -- the pose propagation of step 4.1, the spanning-tree walk -- stays the reference's,
// statement by statement.  INTEGRATION.md shows the lines these replace.
#ifndef LOOPCORRECTION_H
#define LOOPCORRECTION_H

#include <vector>
#include "LocalMap.h"
#include "LoopClosing.h"
#include "g2o_compat.h"

namespace ORB_SLAM2 {

class Map;

// The drop-in for src/LoopClosing.cc:645-727 with mpCurrentKF = pCurrentKF, mvpCurrentConnectedKFs = vpConnected and mg2oScw =
// g2oScw; CorrectedSim3 arrives holding the current keyframe's entry (:631) and leaves, like NonCorrectedSim3, as the reference fills it.
// Step 4.1 runs on the host (Tiw*Twc is a 4x4 cv::gemm on its small path).  Then ONE orbm_map_correct_sim3 call claims and moves the
// points of all keyframes in CorrectedSim3's iteration order, and keyframe by keyframe in that order: SetWorldPos, mnCorrectedByKF and
// mnCorrectedReference for the points that keyframe claimed; one RefreshMapPoints(those points, REFRESH_NORMAL_DEPTH); SetPose;
// UpdateConnections.
// Two facts this order rests on:
//   * UpdateNormalAndDepth of a point corrected under keyframe j reads the camera centres of ALL its observers, and in the reference
//     the keyframes before j in CorrectedSim3's order have their corrected pose by then, those from j on their old one.  So the
//     refresh is one batch PER KEYFRAME, between the SetPose of the keyframe before and this keyframe's own; batched across
//     keyframes it would see other centres and give other normals.
//   * The refresh also sums the observations in std::map<KeyFrame*> order, which the records of the resident map do not keep.  That
//     is why it is not folded into the correction kernel.
// The refreshed points are Touched -- their normal and distance band did change -- and the next Flush sends those rows.  The position
// needs no Touch: the call has written it into the map on both sides.
// A failed call is reported on stderr and leaves the points and poses as they were (the Sim3 maps filled).
void CorrectLoopMap(ResidentMap& map, ORBmatcher& matcher, KeyFrame* pCurrentKF, const std::vector<KeyFrame*>& vpConnected,
                    const g2o::Sim3& g2oScw, LoopClosing::KeyFrameAndPose& CorrectedSim3, LoopClosing::KeyFrameAndPose& NonCorrectedSim3);

// The drop-in for src/LoopClosing.cc:925-989.  Step 1, the walk down the spanning tree from mvpKeyFrameOrigins (mTcwGBA of the children,
// mTcwBefGBA, SetPose), stays on the host as written.  Step 2 is one orbm_map_correct_rigid call over the points of the map, then
// SetWorldPos for every point it changed.  The update changes positions only (the reference calls no UpdateNormalAndDepth here), so
// nothing is Touched for it and nothing is Flushed afterwards: the map Audits clean.  A keyframe that the walk did not reach has no
// mTcwBefGBA; a point whose reference is such a keyframe stays (the reference would read an empty matrix).
void UpdateMapAfterGlobalBA(ResidentMap& map, Map* pMap, unsigned long nLoopKF);

// The number of points below which a correction would run through the library's host routine inside the same call.  UNMEASURED
// placeholder until tools/loop_correction_bench.py has found where the device call and the host routine cross: 0, every call of a map
// with a device goes to the device.
extern const int CORRECT_HOST_BELOW;

}  // namespace ORB_SLAM2

#endif
