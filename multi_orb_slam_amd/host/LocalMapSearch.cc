// LocalMapSearch.cc -- see LocalMapSearch.h.
#include "LocalMapSearch.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include "../../include/orbm.h"
#include "point_row.h"

namespace ORB_SLAM2 {

namespace {

// The point table belongs to the calling THREAD, like the matcher handle it was created on (ORBmatcher.cc: ThreadState).  `rows`
// is what the table holds, byte for byte: a row is sent again only if its 68 packed bytes differ -- compared, not inferred from
// pointers or ids (the rule host/resident.h states for descriptors).
struct LocalTable {
    orbm_matcher* owner = nullptr;
    orbm_points* table = nullptr;
    int capacity = 0;
    std::vector<orbm_point> rows, fresh;
    std::vector<uint8_t> skip, occupied;
    std::vector<orbm_track> track;
    std::vector<int32_t> match;
    int last_written = 0;
    ~LocalTable() { orbm_points_destroy(table); }
};
thread_local LocalTable tls_table;

int report(const char* what, int rc) {
    std::fprintf(stderr, "SearchLocalPoints: %s failed (%d): %s -- search reports 0 matches\n", what, rc, orb_last_error());
    return 0;
}

}  // namespace

void LocalPointsStats(int* rows_written, int* rows_total) {
    if (rows_written) *rows_written = tls_table.last_written;
    if (rows_total) *rows_total = (int)tls_table.rows.size();
}

int SearchLocalPoints(ORBmatcher& matcher, Frame& F, std::vector<MapPoint*>& vpLocalMapPoints, float th, int* nToMatch) {
    if (nToMatch) *nToMatch = 0;
    // points the frame already holds are not searched again (src/Tracking.cc:1708-1728)
    for (MapPoint*& pMP : F.mvpMapPoints) {
        if (!pMP) continue;
        if (pMP->isBad()) { pMP = static_cast<MapPoint*>(NULL); continue; }
        pMP->IncreaseVisible();
        pMP->mnLastFrameSeen = F.mnId;
        pMP->mbTrackInView = false;
    }
    const int n = (int)vpLocalMapPoints.size();
    if (n == 0) return 0;
    if (n > ORBM_MAX_POINTS) { std::fprintf(stderr, "SearchLocalPoints: %d local points exceed the table's limit of %d -- search reports 0 matches\n", n, (int)ORBM_MAX_POINTS); return 0; }

    ORBmatcher::LocalSearchContext C;
    if (!matcher.GetLocalSearchContext(F, &C)) return 0;
    // (a table never reads through its owner after creation -- orbm_points keeps its own device id -- so it may be destroyed after
    //  the thread's matcher handle, whatever the order of the two thread-local destructors)
    LocalTable& T = tls_table;
    int rc;
    if (T.owner != C.handle || n > T.capacity) {           // first use, or the local map outgrew the table: a new one, every row sent
        orbm_points_destroy(T.table); T.table = nullptr; T.rows.clear(); T.capacity = 0;
        const int cap = std::min<int>(ORBM_MAX_POINTS, std::max(n + n / 2, 4096));
        if ((rc = orbm_points_create(C.handle, cap, &T.table))) { T.table = nullptr; return report("orbm_points_create", rc); }
        T.owner = C.handle; T.capacity = cap;
    }
    // pack; which points take no part (src/Tracking.cc:1740-1743)
    T.fresh.resize((size_t)n); T.skip.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        MapPoint* pMP = vpLocalMapPoints[i];
        T.skip[i] = (pMP->mnLastFrameSeen == F.mnId || pMP->isBad()) ? 1 : 0;
        pack_point_row(pMP, T.fresh[i]);
    }
    // send the runs of rows that changed (runs less than 32 unchanged rows apart go out as one)
    const int known = (int)T.rows.size();
    T.rows.resize((size_t)std::max(known, n));
    T.last_written = 0;
    int run_first = -1, run_last = -1;
    auto flush = [&]() -> int {
        if (run_first < 0) return 0;
        const int cnt = run_last - run_first + 1;
        const int r = orbm_points_write(C.handle, T.table, run_first, cnt, T.fresh.data() + run_first);
        if (!r) { std::memcpy(T.rows.data() + run_first, T.fresh.data() + run_first, (size_t)cnt * sizeof(orbm_point)); T.last_written += cnt; }
        run_first = run_last = -1;
        return r;
    };
    for (int i = 0; i < n; ++i) {
        const bool changed = i >= known || std::memcmp(&T.rows[i], &T.fresh[i], sizeof(orbm_point)) != 0;
        if (!changed) continue;
        if (run_first >= 0 && i - run_last > 32 && (rc = flush())) return report("orbm_points_write", rc);
        if (run_first < 0) run_first = i;
        run_last = i;
    }
    if ((rc = flush())) return report("orbm_points_write", rc);

    // the frame members isInFrustum reads.  mRcw, mtcw and mOw are private in the reference (include/Frame.h:263-282): rotation and
    // translation are taken from mTcw -- the very floats UpdatePoseMatrices copies -- and the centre from GetCameraCenter()
    orbm_view V;
    const cv::Mat Ow = F.GetCameraCenter();
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) V.Rcw[3 * i + j] = F.mTcw.at<float>(i, j);
        V.tcw[i] = F.mTcw.at<float>(i, 3);
        V.Ow[i] = Ow.at<float>(i);
    }
    V.fx = F.fx; V.fy = F.fy; V.cx = F.cx; V.cy = F.cy; V.mbf = F.mbf;
    V.min_x = F.mnMinX; V.max_x = F.mnMaxX; V.min_y = F.mnMinY; V.max_y = F.mnMaxY;
    V.viewing_cos_limit = 0.5f;                            // src/Tracking.cc:1746
    V.th = th;
    V.log_scale_factor = F.mfLogScaleFactor; V.n_levels = F.mnScaleLevels; V.scale_factors = F.mvScaleFactors.data();

    T.occupied.resize((size_t)std::max(F.N, 1));
    for (int g = 0; g < F.N; ++g)
        T.occupied[g] = (F.mvpMapPoints[g] && F.mvpMapPoints[g]->Observations() > 0) ? 1 : 0;   // src/ORBmatcher.cc:107-109
    T.track.resize((size_t)n); T.match.resize((size_t)std::max(F.N, 1));
    int in_view = 0, nmatches = 0;
    rc = orbm_search_local_points(C.handle, C.frame, T.table, n, &V, T.skip.data(), T.occupied.data(), C.nnratio, ORBmatcher::TH_HIGH,
                                  T.track.data(), T.match.data(), &in_view, &nmatches);
    if (rc) return report("orbm_search_local_points", rc);
    // what isInFrustum leaves in the points it was called for (src/Frame.cc:445, :491-496; src/Tracking.cc:1746-1750)
    for (int i = 0; i < n; ++i) {
        if (T.skip[i]) continue;
        MapPoint* pMP = vpLocalMapPoints[i];
        const orbm_track& t = T.track[i];
        pMP->mbTrackInView = t.in_view != 0;
        if (!t.in_view) continue;
        pMP->mTrackProjX = t.proj_x; pMP->mTrackProjY = t.proj_y; pMP->mTrackProjXR = t.proj_xr;
        pMP->mnTrackScaleLevel = t.level; pMP->mTrackViewCos = t.view_cos;
        pMP->IncreaseVisible();
    }
    if (nToMatch) *nToMatch = in_view;
    for (int g = 0; g < F.N; ++g)
        if (T.match[g] >= 0) F.mvpMapPoints[g] = vpLocalMapPoints[T.match[g]];                 // src/ORBmatcher.cc:143
    return nmatches;
}

}  // namespace ORB_SLAM2
