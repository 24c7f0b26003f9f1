// LocalMapSearch.h -- Tracking::SearchLocalPoints (reference src/Tracking.cc:1702-1770) with its second half on the device.
//
// The reference projects every local map point into the frame on the host (Frame::isInFrustum), then searches the visible ones
// (ORBmatcher::SearchByProjection(F, vpLocalMapPoints, th)).  SearchLocalPoints below has the same observable effects -- loop 1 over
// F.mvpMapPoints, the six tracking scratch fields and IncreaseVisible of the local points, F.mvpMapPoints filled by the search --
// but the points live in a table in HBM (include/orbm.h: orbm_points), one per calling thread, of which only the rows whose
// packed bytes changed since the previous call are sent again; the frustum test, the scale prediction, the query records and
// the search run on the device in one call (orbm_search_local_points).  INTEGRATION.md shows the three lines it replaces.
#ifndef LOCALMAPSEARCH_H
#define LOCALMAPSEARCH_H

#include <vector>
#include "ORBmatcher.h"

namespace ORB_SLAM2 {

// th: SearchByProjection's th (1, 3 or 5 in the reference).  Returns the number of matches; *nToMatch (may be NULL) receives the
// number of local points in view.  A failed device call reports 0 matches, as every search of ORBmatcher does.
int SearchLocalPoints(ORBmatcher& matcher, Frame& F, std::vector<MapPoint*>& vpLocalMapPoints, float th, int* nToMatch = nullptr);

// inspection (tests / bench): rows of the calling thread's point table sent to the device by its last call / held by the table
void LocalPointsStats(int* rows_written, int* rows_total);

}  // namespace ORB_SLAM2

#endif
