// point_row.h -- internal to libmorb_host.so: a MapPoint as the 68-byte row the device reads (include/orbm.h: orbm_point), packed in
// one place for host/LocalMapSearch.cc (the per-thread point table) and host/LocalMap.cc (the resident map).
#pragma once
#include <cstring>
#include "../../include/orbm.h"
#include "slam_types.h"

namespace ORB_SLAM2 {

// The raw distance bounds of a MapPoint.  They are protected in the reference's class (include/MapPoint.h:152-153), whose
// accessors hand out 0.8f * min and 1.2f * max only; a build against the reference's headers adds the two accessors named
// here to MapPoint.
#ifdef MORB_USE_REFERENCE_TYPES
inline float raw_min_distance(MapPoint* p) { return p->GetMinDistance(); }
inline float raw_max_distance(MapPoint* p) { return p->GetMaxDistance(); }
#else
inline float raw_min_distance(MapPoint* p) { return p->mfMinDistance; }
inline float raw_max_distance(MapPoint* p) { return p->mfMaxDistance; }
#endif

inline void pack_point_row(MapPoint* pMP, orbm_point& r) {
    std::memset(&r, 0, sizeof(r));
    const cv::Mat P = pMP->GetWorldPos(), Pn = pMP->GetNormal(), d = pMP->GetDescriptor();
    for (int k = 0; k < 3; ++k) { r.pos[k] = P.at<float>(k); r.normal[k] = Pn.at<float>(k); }
    r.min_dist = raw_min_distance(pMP); r.max_dist = raw_max_distance(pMP);
    r.blocks = pMP->Observations() > 0 ? 1 : 0;
    std::memcpy(r.desc, d.ptr(0), 32);
}

}  // namespace ORB_SLAM2
