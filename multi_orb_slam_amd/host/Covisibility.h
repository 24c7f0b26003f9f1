// Covisibility.h -- the two counting routines of the LocalMapping and LoopClosing threads over the resident map (host/LocalMap.h):
// the counters of KeyFrame::UpdateConnections (reference src/KeyFrame.cc:512-552) and LocalMapping::KeyFrameCulling
// (src/LocalMapping.cc:966-1038).
//
// The reference copies pMP->GetObservations() -- a std::map -- for every point of the keyframe, twice in UpdateConnections, and for
// every point of every covisible keyframe in KeyFrameCulling.  Here the resident map already holds every observation as a record
// under a slot; it learns the feature index of a record, a level / far byte per feature, the camera-1 feature count of a keyframe
// and n_obs of a point (ResidentMap::Flush sends them with everything else), and one call counts for all the keyframes asked about
// (include/orbm.h: orbm_map_covisibility, orbm_map_culling_counts; the host routines for a map without a device).  What is pointer
// logic over private members -- the rest of UpdateConnections, KeyFrame::SetBadFlag -- stays the reference's.  INTEGRATION.md shows the
// lines these replace and lists every statement of the reference that owes the map a Touch.
#ifndef COVISIBILITY_H
#define COVISIBILITY_H

#include <map>
#include <vector>
#include "LocalMap.h"

namespace ORB_SLAM2 {

// KFcounter and KFcounter_cam1 exactly as src/KeyFrame.cc:512-552 leave them for pKF (no entry of value 0): the drop-in for those
// lines inside the member function.  The maps are cleared first; a failed call is reported on stderr and leaves them empty.
void CovisibilityCounts(ResidentMap& map, KeyFrame* pKF, std::map<KeyFrame*, int>& KFcounter, std::map<KeyFrame*, int>& KFcounter_cam1);
// The same for every keyframe of vpKFs in one call (LoopClosing::CorrectLoop's loop over the connected keyframes): entry i belongs to
// vpKFs[i].  The counters of one keyframe do not depend on the AddConnection calls of another, so they may all be taken first.
void CovisibilityCounts(ResidentMap& map, const std::vector<KeyFrame*>& vpKFs, std::vector<std::map<KeyFrame*, int> >& vKFcounter,
                        std::vector<std::map<KeyFrame*, int> >& vKFcounter_cam1);

// The body of LocalMapping::KeyFrameCulling for mpCurrentKeyFrame = pCurrentKF and mbMonocular = bMonocular, with the reference's
// verdicts keyframe by keyframe: one counting call covers all of GetVectorCovisibleKeyFrames() (mnId == 0 skipped); the test
// nRedundantObservations > 0.90 * nMPs runs in double, in the reference's order; after a SetBadFlag() that made the keyframe bad the
// keyframe, its points and the observers of those points that turned bad are Touched, the map is Flushed and the keyframes not yet
// judged are counted again -- a culled keyframe changes the map the later ones are judged on.  A SetBadFlag() that was refused
// (mbNotErase) changes nothing and costs no call.
void KeyFrameCulling(ResidentMap& map, KeyFrame* pCurrentKF, bool bMonocular);

}  // namespace ORB_SLAM2

#endif
