// MapPointRefresh.h -- MapPoint::ComputeDistinctiveDescriptors + MapPoint::UpdateNormalAndDepth (reference src/MapPoint.cc:325-438,
// :480-528) for a batch of map points in one device call.
//
// The reference calls the pair for every point of every new keyframe (src/LocalMapping.cc:199-201, :685-687, :784-785;
// src/Tracking.cc:740-743, :786-788, :1600-1601, :1664-1665; src/LoopClosing.cc:709, :748) and UpdateNormalAndDepth alone after every
// bundle adjustment (src/Optimizer.cc:320, :1346, :1675), one point at a time: a std::map copy, a vector of cv::Mat rows and an allocation
// plus std::sort per observation.  RefreshMapPoints below has the same observable effects on every non-bad point of the vector --
// mDescriptor, mNormalVector, mfMinDistance, mfMaxDistance -- with the all-pairs Hamming work, the medians and the normals of the whole
// batch computed in one call of orbm_refresh_points (include/orbm.h).  INTEGRATION.md shows the loops it replaces.
#ifndef MAPPOINTREFRESH_H
#define MAPPOINTREFRESH_H

#include <vector>
#include "ORBmatcher.h"

namespace ORB_SLAM2 {

enum { REFRESH_DESCRIPTOR = 1, REFRESH_NORMAL_DEPTH = 2, REFRESH_BOTH = 3 };

// what: REFRESH_DESCRIPTOR = ComputeDistinctiveDescriptors, REFRESH_NORMAL_DEPTH = UpdateNormalAndDepth, REFRESH_BOTH = the pair, for every
// point of the vector that is not NULL and not bad.  A point may appear more than once (it is refreshed once).  Batches of fewer than
// REFRESH_HOST_BELOW points are computed by the library's host routine (the same statements, no launch); a failed device call is
// reported as every search of ORBmatcher reports it and leaves the points as they were.
void RefreshMapPoints(ORBmatcher& matcher, const std::vector<MapPoint*>& vpMapPoints, int what = REFRESH_BOTH);

// The batch size below which the host routine is used.  UNMEASURED placeholder until tools/map_points_bench.py has run.
extern const int REFRESH_HOST_BELOW;

// inspection (tests / bench): points of the calling thread's last call by path, as orbm_debug_last_refresh reports them, or all
// zero but [3] = the batch size when the host routine took the whole batch
void RefreshStats(int* out5);

}  // namespace ORB_SLAM2

#endif
