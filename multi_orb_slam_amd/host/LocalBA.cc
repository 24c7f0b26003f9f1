// LocalBA.cc -- Optimizer::LocalBundleAdjustment (host/Optimizer.h; reference src/Optimizer.cc:921-1353) over orbm_local_ba
// (include/orbm.h).  Steps 1-4 (the local keyframes, the local map points, the fixed cameras, with the mnBALocalForKF / mnBAFixedForKF
// marks) and 12-13 (the erasures, SetPose, SetWorldPos, UpdateNormalAndDepth under pMap->mMutexMapUpdate) are the reference's statement by
// statement; the g2o graph between them is the arrays of one call.  What differs from the reference is the call's (include/orbm.h):
// the dense solver of the reduced system, and the order of a point's observations, which is by mnId here and by heap address there; the
// points are handed over in ascending vertex id, so the edges are summed in that order and not in that of lLocalMapPoints.
#include "Optimizer.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <list>
#include <map>
#include <mutex>
#include <vector>
#include "../../include/orbm.h"
#include "slam_types.h"
#ifdef MORB_USE_REFERENCE_TYPES
#include "Map.h"
#endif
#include "MapPointRefresh.h"
#include "ba_rig.h"

namespace ORB_SLAM2 {

// tools/local_ba_bench.py on an MI355X (profiles/r20/local_ba_bench.json): 2 228 edges take the host routine 5.6 ms and the device call
// 5.9 ms, 9 057 edges 29.7 against 18.4 ms
const int LBA_HOST_BELOW = 2500;

namespace {
int read_stop_flag(void* p) { return *static_cast<bool*>(p) ? 1 : 0; }
}

void Optimizer::LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, Map* pMap) {
    // Local KeyFrames: First Breath Search from Current Keyframe (:930-953)
    std::list<KeyFrame*> lLocalKeyFrames;
    lLocalKeyFrames.push_back(pKF);
    pKF->mnBALocalForKF = pKF->mnId;
    const std::vector<KeyFrame*> vNeighKFs = pKF->GetVectorCovisibleKeyFrames();
    for (int i = 0, iend = vNeighKFs.size(); i < iend; i++) {
        KeyFrame* pKFi = vNeighKFs[i];
        pKFi->mnBALocalForKF = pKF->mnId;
        if (!pKFi->isBad()) lLocalKeyFrames.push_back(pKFi);
    }
    // Local MapPoints seen in Local KeyFrames (:955-974)
    std::list<MapPoint*> lLocalMapPoints;
    for (std::list<KeyFrame*>::iterator lit = lLocalKeyFrames.begin(), lend = lLocalKeyFrames.end(); lit != lend; lit++) {
        std::vector<MapPoint*> vpMPs = (*lit)->GetMapPointMatches();
        for (std::vector<MapPoint*>::iterator vit = vpMPs.begin(), vend = vpMPs.end(); vit != vend; vit++) {
            MapPoint* pMP = *vit;
            if (pMP)
                if (!pMP->isBad())
                    if (pMP->mnBALocalForKF != pKF->mnId) {
                        lLocalMapPoints.push_back(pMP);
                        pMP->mnBALocalForKF = pKF->mnId;
                    }
        }
    }
    // Fixed Keyframes. Keyframes that see Local MapPoints but that are not Local Keyframes (:976-996)
    std::list<KeyFrame*> lFixedCameras;
    for (std::list<MapPoint*>::iterator lit = lLocalMapPoints.begin(), lend = lLocalMapPoints.end(); lit != lend; lit++) {
        std::map<KeyFrame*, size_t> observations = (*lit)->GetObservations();
        for (std::map<KeyFrame*, size_t>::iterator mit = observations.begin(), mend = observations.end(); mit != mend; mit++) {
            KeyFrame* pKFi = mit->first;
            if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) {
                pKFi->mnBAFixedForKF = pKF->mnId;
                if (!pKFi->isBad()) lFixedCameras.push_back(pKFi);
            }
        }
    }

    // The vertices: the local keyframes except mnId == 0 in ascending mnId (g2o's VertexIDCompare order) are the free poses; keyframe 0
    // and the fixed cameras follow (setFixed(true), :1027, :1041)
    std::vector<KeyFrame*> vpPoses;
    for (KeyFrame* k : lLocalKeyFrames) if (k->mnId != 0) vpPoses.push_back(k);
    std::sort(vpPoses.begin(), vpPoses.end(), [](KeyFrame* a, KeyFrame* b) { return a->mnId < b->mnId; });
    const int n_free = (int)vpPoses.size();
    for (KeyFrame* k : lLocalKeyFrames) if (k->mnId == 0) vpPoses.push_back(k);
    for (KeyFrame* k : lFixedCameras) vpPoses.push_back(k);
    std::map<KeyFrame*, int> pose_of;
    for (size_t p = 0; p < vpPoses.size(); ++p) pose_of[vpPoses[p]] = (int)p;
    std::vector<float> Tcw(16 * std::max<size_t>(vpPoses.size(), 1)), K(5 * std::max<size_t>(vpPoses.size(), 1));
    for (size_t p = 0; p < vpPoses.size(); ++p) {
        const cv::Mat T = vpPoses[p]->GetPose();
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) Tcw[16 * p + 4 * r + c] = T.at<float>(r, c);
        K[5 * p] = vpPoses[p]->fx; K[5 * p + 1] = vpPoses[p]->fy; K[5 * p + 2] = vpPoses[p]->cx; K[5 * p + 3] = vpPoses[p]->cy;
        K[5 * p + 4] = vpPoses[p]->mbf;
    }

    // Tcam11, Tcam21 (:1048-1061)
    orbm_lba_problem P;
    std::memset(&P, 0, sizeof(P));
    FillTcim(pKF->mRcam12, pKF->mtcam12, P.Tcim);

    // The points in ascending vertex id (mnId + maxKFid + 1), each with its observations as edges (:1092-1202), ordered by mnId
    std::vector<MapPoint*> vpPoints(lLocalMapPoints.begin(), lLocalMapPoints.end());
    std::sort(vpPoints.begin(), vpPoints.end(), [](MapPoint* a, MapPoint* b) { return a->mnId < b->mnId; });
    std::vector<float> points(3 * std::max<size_t>(vpPoints.size(), 1)), obs, inv_sigma2;
    std::vector<int32_t> first(1, 0), edge_pose;
    std::vector<uint8_t> edge_cam;
    std::vector<KeyFrame*> vpEdgeKF;
    std::vector<MapPoint*> vpEdgeMP;
    for (size_t l = 0; l < vpPoints.size(); ++l) {
        MapPoint* pMP = vpPoints[l];
        const cv::Mat X = pMP->GetWorldPos();
        for (int k = 0; k < 3; ++k) points[3 * l + k] = X.at<float>(k);
        const std::map<KeyFrame*, size_t> observations = pMP->GetObservations();
        std::vector<std::pair<KeyFrame*, size_t> > vObs(observations.begin(), observations.end());
        std::sort(vObs.begin(), vObs.end(), [](const std::pair<KeyFrame*, size_t>& a, const std::pair<KeyFrame*, size_t>& b) { return a.first->mnId < b.first->mnId; });
        for (size_t o = 0; o < vObs.size(); ++o) {
            KeyFrame* pKFi = vObs[o].first;
            const size_t idx = vObs[o].second;
            const int cam = pKFi->keypoint_to_cam.find(idx)->second;
            if (pKFi->isBad()) continue;
            std::map<KeyFrame*, int>::const_iterator pit = pose_of.find(pKFi);
            if (pit == pose_of.end()) continue;            // (every observer that is not bad is a local or a fixed keyframe)
            const cv::KeyPoint& kpUn = pKFi->mvKeysUn_total[idx];
            const float kp_ur = pKFi->mvuRight_total[idx];
            edge_pose.push_back(pit->second); edge_cam.push_back((uint8_t)(cam ? 1 : 0));
            obs.push_back(kpUn.pt.x); obs.push_back(kpUn.pt.y); obs.push_back(kp_ur);
            inv_sigma2.push_back(pKFi->mvInvLevelSigma2[kpUn.octave]);
            vpEdgeKF.push_back(pKFi); vpEdgeMP.push_back(pMP);
        }
        first.push_back((int32_t)edge_pose.size());
    }
    const size_t ne = edge_pose.size();
    P.n_free = n_free; P.n_poses = (int32_t)vpPoses.size(); P.n_points = (int32_t)vpPoints.size();
    P.Tcw = Tcw.data(); P.K = K.data(); P.points = points.data(); P.bad = nullptr; P.first = first.data();
    P.edge_pose = edge_pose.data(); P.edge_cam = edge_cam.data(); P.obs = obs.data(); P.inv_sigma2 = inv_sigma2.data();
    std::vector<double> pose_out(7 * std::max<size_t>(vpPoses.size(), 1)), point_out(3 * std::max<size_t>(vpPoints.size(), 1));
    std::vector<float> Tcw_out(16 * std::max<size_t>(vpPoses.size(), 1)), point_f(3 * std::max<size_t>(vpPoints.size(), 1));
    std::vector<uint8_t> flags(std::max<size_t>(ne, 1), 0);
    orbm_lba_result R;
    std::memset(&R, 0, sizeof(R));
    R.pose = pose_out.data(); R.Tcw = Tcw_out.data(); R.point = point_out.data(); R.point_f = point_f.data(); R.flags = flags.data();

    // :1204-1271 -- the poll at :1204, both optimisations and the test between them, the poll at :1217, the final test
    orbm_lba_stop_fn stop = pbStopFlag ? read_stop_flag : nullptr;
    ORBmatcher matcher(0.6f, false);                       // (the handle underneath is the calling thread's)
    int rc;
    if ((int)ne < LBA_HOST_BELOW || n_free == 0) {
        rc = orbm_local_ba_host(&P, stop, pbStopFlag, ORBM_POSE_ORDER_DEVICE, &R);
    } else {
        orbm_matcher* h = matcher.GetDeviceHandle();
        if (!h) return;                                    // (reported by the matcher)
        rc = orbm_local_ba(h, &P, stop, pbStopFlag, &R);
    }
    if (rc != ORB_OK) { std::fprintf(stderr, "LocalBundleAdjustment: %s -- nothing optimised\n", orb_last_error()); return; }
    if (R.ended == ORBM_LBA_ENDED_STOPPED_AT_START) return;   // :1204-1206

    // Check inlier observations (:1273-1309): the mono edges in insertion order, then the stereo ones
    std::vector<std::pair<KeyFrame*, MapPoint*> > vToErase;
    vToErase.reserve(ne);
    for (int stereo = 0; stereo < 2; ++stereo)
        for (size_t e = 0; e < ne; ++e) {
            if ((obs[3 * e + 2] < 0 ? 0 : 1) != stereo) continue;
            if (vpEdgeMP[e]->isBad()) continue;
            if (flags[e] & ORBM_LBA_FLAG_ERASE) vToErase.push_back(std::make_pair(vpEdgeKF[e], vpEdgeMP[e]));
        }

    // Get Map Mutex (:1311-1347)
    std::unique_lock<decltype(pMap->mMutexMapUpdate)> lock(pMap->mMutexMapUpdate);   // (std::mutex in the reference: `unique_lock<mutex>`)
    if (!vToErase.empty()) {
        for (size_t i = 0; i < vToErase.size(); i++) {
            KeyFrame* pKFi = vToErase[i].first;
            MapPoint* pMPi = vToErase[i].second;
            pKFi->EraseMapPointMatch(pMPi);
            pMPi->EraseObservation(pKFi);
        }
    }
    // Recover optimized data: Keyframes
    for (std::list<KeyFrame*>::iterator lit = lLocalKeyFrames.begin(), lend = lLocalKeyFrames.end(); lit != lend; lit++) {
        KeyFrame* pKFl = *lit;
        const float* T = Tcw_out.data() + 16 * (size_t)pose_of[pKFl];
        cv::Mat M(4, 4, CV_32F);
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) M.at<float>(r, c) = T[4 * r + c];
        pKFl->SetPose(M);
    }
    // Points: SetWorldPos in the reference's order; UpdateNormalAndDepth of all of them in one batched call
    std::map<MapPoint*, size_t> point_of;
    for (size_t l = 0; l < vpPoints.size(); ++l) point_of[vpPoints[l]] = l;
    std::vector<MapPoint*> vpRefresh;
    vpRefresh.reserve(vpPoints.size());
    for (std::list<MapPoint*>::iterator lit = lLocalMapPoints.begin(), lend = lLocalMapPoints.end(); lit != lend; lit++) {
        MapPoint* pMP = *lit;
        const float* X = point_f.data() + 3 * point_of[pMP];
        cv::Mat Pos(3, 1, CV_32F);
        for (int k = 0; k < 3; ++k) Pos.at<float>(k) = X[k];
        pMP->SetWorldPos(Pos);
        vpRefresh.push_back(pMP);
    }
    RefreshMapPoints(matcher, vpRefresh, REFRESH_NORMAL_DEPTH);
}

}  // namespace ORB_SLAM2
