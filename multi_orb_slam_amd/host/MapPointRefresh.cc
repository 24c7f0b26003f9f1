// MapPointRefresh.cc -- see MapPointRefresh.h.
#include "MapPointRefresh.h"

#include <cstdio>
#include <cstring>
#include <map>
#include <unordered_map>
#include <unordered_set>
#include "../../include/orbm.h"
#include "../../include/orb_debug.h"

namespace ORB_SLAM2 {

// UNMEASURED: see MapPointRefresh.h
const int REFRESH_HOST_BELOW = 16;

namespace {

// Everything below goes through public members of the reference's classes but two: the results are written through
// MapPoint::SetDistinctiveDescriptor(const cv::Mat&) and MapPoint::SetNormalAndDepth(const cv::Mat&, float, float), which a build against
// the reference's headers adds to MapPoint (mDescriptor, mNormalVector and the two distances are protected there, include/MapPoint.h:134-153;
// INTEGRATION.md).  The stand-in of slam_types.h has them under the same names.
struct Centres { float c[2][3]; };

struct Scratch {   // per calling thread, like the matcher handle
    std::vector<MapPoint*> pts;
    std::vector<int32_t> first, ref_level;
    std::vector<uint8_t> desc, alive, what;
    std::vector<float> centre, pos, ref_centre;
    std::vector<orbm_refresh_out> out;
    int stats[5] = {0, 0, 0, 0, 0};
};
thread_local Scratch tls_scratch;

}  // namespace

void RefreshStats(int* out5) { for (int k = 0; k < 5; ++k) out5[k] = tls_scratch.stats[k]; }

void RefreshMapPoints(ORBmatcher& matcher, const std::vector<MapPoint*>& vpMapPoints, int what) {
    what &= REFRESH_BOTH;
    Scratch& S = tls_scratch;
    for (int k = 0; k < 5; ++k) S.stats[k] = 0;
    if (!what) return;
    S.pts.clear(); S.first.assign(1, 0); S.ref_level.clear(); S.desc.clear(); S.alive.clear(); S.what.clear();
    S.centre.clear(); S.pos.clear(); S.ref_centre.clear();
    std::unordered_map<KeyFrame*, Centres> centres;      // GetCameraCenter() / GetCameraCenter_cam2() once per keyframe of the batch
    std::unordered_set<MapPoint*> seen;
    const std::vector<float>* scale_factors = nullptr;
    int n_levels = 0;
    bool same_pyramid = true;
    auto centre_of = [&](KeyFrame* pKF) -> const Centres& {
        auto it = centres.find(pKF);
        if (it != centres.end()) return it->second;
        Centres C;
        const cv::Mat c1 = pKF->GetCameraCenter(), c2 = pKF->GetCameraCenter_cam2();
        for (int k = 0; k < 3; ++k) { C.c[0][k] = c1.at<float>(k); C.c[1][k] = c2.at<float>(k); }
        return centres.emplace(pKF, C).first->second;
    };
    for (MapPoint* pMP : vpMapPoints) {
        if (!pMP || pMP->isBad() || !seen.insert(pMP).second) continue;          // `if(mbBad) return;` (src/MapPoint.cc:334, :488)
        const std::map<KeyFrame*, size_t> observations = pMP->GetObservations();
        if (observations.empty()) continue;                                       // :341, :496
        const cv::Mat Pos = pMP->GetWorldPos();
        for (std::map<KeyFrame*, size_t>::const_iterator mit = observations.begin(), mend = observations.end(); mit != mend; ++mit) {
            KeyFrame* pKF = mit->first;
            const size_t l = mit->second;
            const int cam = pKF->keypoint_to_cam.find(l)->second;                 // :355, :505
            const bool alive = !pKF->isBad();                                     // :352 -- ComputeDistinctiveDescriptors only
            const size_t at = S.desc.size();
            S.desc.resize(at + 32, 0);
            if ((what & REFRESH_DESCRIPTOR) && alive) {
                const int descIdx = pKF->cont_idx_to_local_cam_idx.find(l)->second;   // :356
                const cv::Mat d = pKF->GetDescriptor(cam, descIdx);                   // :358
                std::memcpy(&S.desc[at], d.ptr(0), 32);
            }
            S.alive.push_back(alive ? 1 : 0);
            const Centres& C = centre_of(pKF);                                    // Owi[cam], :507-512
            for (int k = 0; k < 3; ++k) S.centre.push_back(C.c[cam ? 1 : 0][k]);
        }
        // pRefKF->mvKeysUn_total[observations[pRefKF]].octave (:519): operator[] on the copy -- index 0 when the reference keyframe
        // does not observe the point
        KeyFrame* pRefKF = pMP->GetReferenceKeyFrame();
        int level = 0;
        if (what & REFRESH_NORMAL_DEPTH) {
            const std::map<KeyFrame*, size_t>::const_iterator rit = observations.find(pRefKF);
            const size_t ridx = rit != observations.end() ? rit->second : 0;
            level = pRefKF->mvKeysUn_total[ridx].octave;
            const cv::Mat Or = pRefKF->GetCameraCenter();                         // camera 1, whatever camera observed (:517)
            for (int k = 0; k < 3; ++k) S.ref_centre.push_back(Or.at<float>(k));
            if (!scale_factors) { scale_factors = &pRefKF->mvScaleFactors; n_levels = pRefKF->mnScaleLevels; }
            else if (pRefKF->mnScaleLevels != n_levels || pRefKF->mvScaleFactors != *scale_factors) same_pyramid = false;
        } else {
            for (int k = 0; k < 3; ++k) S.ref_centre.push_back(0.0f);
        }
        for (int k = 0; k < 3; ++k) S.pos.push_back(Pos.at<float>(k));
        S.ref_level.push_back(level);
        S.what.push_back((uint8_t)what);
        S.first.push_back((int32_t)S.alive.size());
        S.pts.push_back(pMP);
    }
    const int P = (int)S.pts.size();
    if (P == 0) return;
    if (!same_pyramid) {
        // the reference reads the scale table of every point's own reference keyframe; one ORBextractor configuration per system
        // makes them all equal, and the batch carries one table
        std::fprintf(stderr, "RefreshMapPoints: the reference keyframes of the batch have different scale pyramids -- points left as they were\n");
        return;
    }
    orbm_refresh_in in;
    std::memset(&in, 0, sizeof(in));
    in.n_points = P; in.n_obs = (int32_t)S.alive.size();
    in.first = S.first.data(); in.obs_desc = S.desc.data(); in.obs_centre = S.centre.data(); in.obs_alive = S.alive.data();
    in.pos = S.pos.data(); in.ref_centre = S.ref_centre.data(); in.ref_level = S.ref_level.data(); in.what = S.what.data();
    in.scale_factors = scale_factors ? scale_factors->data() : nullptr; in.n_levels = n_levels;
    S.out.resize((size_t)P);
    int rc;
    if (P < REFRESH_HOST_BELOW) {                       // a single MapPoint::Replace does not pay a launch
        rc = orbm_refresh_points_host(&in, S.out.data());
        S.stats[3] = P;
    } else {
        orbm_matcher* h = matcher.GetDeviceHandle();
        if (!h) return;                                 // (reported by the matcher)
        rc = orbm_refresh_points(h, &in, S.out.data());
        if (!rc) orbm_debug_last_refresh(h, S.stats);
    }
    if (rc) {
        std::fprintf(stderr, "RefreshMapPoints: orbm_refresh_points failed (%d): %s -- points left as they were\n", rc, orb_last_error());
        return;
    }
    for (int i = 0; i < P; ++i) {
        const orbm_refresh_out& o = S.out[i];
        if ((what & REFRESH_DESCRIPTOR) && o.best_obs >= 0) {     // `if(vDescriptors.empty()) return;` otherwise (:366)
            cv::Mat d(1, 32, CV_8U);
            std::memcpy(d.ptr(0), o.desc, 32);
            S.pts[i]->SetDistinctiveDescriptor(d);                // mDescriptor = vDescriptors[BestIdx].clone()   (:428)
        }
        if (what & REFRESH_NORMAL_DEPTH) {
            cv::Mat n(3, 1, CV_32F);
            for (int k = 0; k < 3; ++k) n.at<float>(k) = o.normal[k];
            S.pts[i]->SetNormalAndDepth(n, o.min_dist, o.max_dist);   // :525-527
        }
    }
}

}  // namespace ORB_SLAM2
