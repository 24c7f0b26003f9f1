// GlobalBA.cc -- Optimizer::BundleAdjustment and Optimizer::GlobalBundleAdjustemnt (host/Optimizer.h; reference src/Optimizer.cc:47-330)
// over orbm_bundle_adjust (include/orbm.h).  The filtering of the keyframes, points and observations (:102-276) and the recovery
// (:282-328) are the reference's statement by statement; the g2o graph between them is the arrays of one call.  What differs from the
// reference is the call's (include/orbm.h: the dense solver of the reduced system) and the order in which the graph is handed over: the
// points in ascending mnId (their vertex ids mnId + maxKFid + 1 ascend with it) and a point's observations in ascending keyframe mnId,
// where std::map<KeyFrame*, size_t> orders them by heap address.  An observing keyframe that is neither bad nor past maxKFid but is not
// in vpKFs has no vertex in the reference (optimizer.vertex() returns NULL there); its observation is dropped here.
#include "Optimizer.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>
#include "../../include/orbm.h"
#include "slam_types.h"
#ifdef MORB_USE_REFERENCE_TYPES
#include "Map.h"
#endif
#include "MapPointRefresh.h"
#include "ba_rig.h"

namespace ORB_SLAM2 {

// tools/global_ba_bench.py on an MI355X (profiles/r21/global_ba_bench.json): at 1 007 edges (10 free keyframes), the smallest world
// measured, the device call already takes 4.3 ms against the host routine's 5.3 ms, at 2 002 edges 5.9 against 10.7 ms.  The crossing
// lies below the smallest world measured; 1 000 is that bound, not a crossing found from both sides.
const int GBA_HOST_BELOW = 1000;

namespace {
int read_stop_flag(void* p) { return *static_cast<bool*>(p) ? 1 : 0; }
}

void Optimizer::GlobalBundleAdjustemnt(Map* pMap, int nIterations, bool* pbStopFlag, const unsigned long nLoopKF, const bool bRobust,
                                       cv::Mat mCalibMatrix) {
    std::vector<KeyFrame*> vpKFs = pMap->GetAllKeyFrames();
    std::vector<MapPoint*> vpMP = pMap->GetAllMapPoints();
    BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust, mCalibMatrix);
}

void Optimizer::BundleAdjustment(const std::vector<KeyFrame*>& vpKFs, const std::vector<MapPoint*>& vpMP, int nIterations, bool* pbStopFlag,
                                 const unsigned long nLoopKF, const bool bRobust, cv::Mat CalibMatrix) {
    std::vector<bool> vbNotIncludedMP;
    vbNotIncludedMP.resize(vpMP.size());

    // Set KeyFrame vertices (:102-120): every keyframe that is not bad; fixed iff mnId == 0.  The free poses in ascending mnId
    // (g2o's VertexIDCompare order) come first.
    long unsigned int maxKFid = 0;
    std::vector<KeyFrame*> vpPoses;
    for (size_t i = 0; i < vpKFs.size(); i++) {
        KeyFrame* pKF = vpKFs[i];
        if (pKF->isBad()) continue;
        if (pKF->mnId != 0) vpPoses.push_back(pKF);
        if (pKF->mnId > maxKFid) maxKFid = pKF->mnId;
    }
    std::sort(vpPoses.begin(), vpPoses.end(), [](KeyFrame* a, KeyFrame* b) { return a->mnId < b->mnId; });
    const int n_free = (int)vpPoses.size();
    for (size_t i = 0; i < vpKFs.size(); i++) if (!vpKFs[i]->isBad() && vpKFs[i]->mnId == 0) vpPoses.push_back(vpKFs[i]);
    std::map<KeyFrame*, int> pose_of;
    for (size_t p = 0; p < vpPoses.size(); ++p) pose_of[vpPoses[p]] = (int)p;
    std::vector<float> Tcw(16 * std::max<size_t>(vpPoses.size(), 1)), K(5 * std::max<size_t>(vpPoses.size(), 1));
    for (size_t p = 0; p < vpPoses.size(); ++p) {
        const cv::Mat T = vpPoses[p]->GetPose();
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) Tcw[16 * p + 4 * r + c] = T.at<float>(r, c);
        K[5 * p] = vpPoses[p]->fx; K[5 * p + 1] = vpPoses[p]->fy; K[5 * p + 2] = vpPoses[p]->cx; K[5 * p + 3] = vpPoses[p]->cy;
        K[5 * p + 4] = vpPoses[p]->mbf;
    }

    // Tcam11, Tcam21 (:122-136): rows 0..2 of CalibMatrix hold Rcam12, row 3 holds tcam12
    cv::Mat Rcam12(3, 3, CV_32F), tcam12 = cv::Mat::zeros(3, 1, CV_32F);
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) Rcam12.at<float>(r, c) = CalibMatrix.at<float>(r, c); tcam12.at<float>(r, 0) = CalibMatrix.at<float>(3, r); }
    orbm_lba_problem P;
    std::memset(&P, 0, sizeof(P));
    FillTcim(Rcam12, tcam12, P.Tcim);

    // Set MapPoint vertices and their edges (:148-276); a point without an edge is removed again
    std::vector<size_t> order;
    for (size_t i = 0; i < vpMP.size(); i++) if (!vpMP[i]->isBad()) order.push_back(i);
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return vpMP[a]->mnId < vpMP[b]->mnId; });
    std::vector<float> points, obs, inv_sigma2;
    std::vector<int32_t> first(1, 0), edge_pose;
    std::vector<uint8_t> edge_cam;
    std::vector<int> row_of(vpMP.size(), -1);
    for (size_t q = 0; q < order.size(); ++q) {
        MapPoint* pMP = vpMP[order[q]];
        const std::map<KeyFrame*, size_t> observations = pMP->GetObservations();
        std::vector<std::pair<KeyFrame*, size_t> > vObs(observations.begin(), observations.end());
        std::sort(vObs.begin(), vObs.end(), [](const std::pair<KeyFrame*, size_t>& a, const std::pair<KeyFrame*, size_t>& b) { return a.first->mnId < b.first->mnId; });
        int nEdges = 0;
        for (size_t o = 0; o < vObs.size(); ++o) {
            KeyFrame* pKF = vObs[o].first;
            if (pKF->isBad() || pKF->mnId > maxKFid) continue;
            std::map<KeyFrame*, int>::const_iterator pit = pose_of.find(pKF);
            if (pit == pose_of.end()) continue;
            nEdges++;
            const size_t idx = vObs[o].second;
            const cv::KeyPoint& kpUn = pKF->mvKeysUn_total[idx];
            const int cam = pKF->keypoint_to_cam.find(idx)->second;
            edge_pose.push_back(pit->second); edge_cam.push_back((uint8_t)(cam ? 1 : 0));
            obs.push_back(kpUn.pt.x); obs.push_back(kpUn.pt.y); obs.push_back(pKF->mvuRight_total[idx]);   // (< 0: the mono edge)
            inv_sigma2.push_back(pKF->mvInvLevelSigma2[kpUn.octave]);
        }
        if (nEdges == 0) { vbNotIncludedMP[order[q]] = true; continue; }
        vbNotIncludedMP[order[q]] = false;
        row_of[order[q]] = (int)(first.size() - 1);
        const cv::Mat X = pMP->GetWorldPos();
        for (int k = 0; k < 3; ++k) points.push_back(X.at<float>(k));
        first.push_back((int32_t)edge_pose.size());
    }
    const size_t ne = edge_pose.size(), np = first.size() - 1;
    if (points.empty()) points.resize(3);
    P.n_free = n_free; P.n_poses = (int32_t)vpPoses.size(); P.n_points = (int32_t)np;
    P.Tcw = Tcw.data(); P.K = K.data(); P.points = points.data(); P.bad = nullptr; P.first = first.data();
    P.edge_pose = edge_pose.data(); P.edge_cam = edge_cam.data(); P.obs = obs.data(); P.inv_sigma2 = inv_sigma2.data();
    std::vector<double> pose_out(7 * std::max<size_t>(vpPoses.size(), 1)), point_out(3 * std::max<size_t>(np, 1));
    std::vector<float> Tcw_out(16 * std::max<size_t>(vpPoses.size(), 1)), point_f(3 * std::max<size_t>(np, 1));
    orbm_ba_result R;
    std::memset(&R, 0, sizeof(R));
    R.pose = pose_out.data(); R.Tcw = Tcw_out.data(); R.point = point_out.data(); R.point_f = point_f.data();

    // Optimize! (:278-280)
    orbm_lba_stop_fn stop = pbStopFlag ? read_stop_flag : nullptr;
    ORBmatcher matcher(0.6f, false);                       // (the handle underneath is the calling thread's)
    int rc;
    if ((int)ne < GBA_HOST_BELOW || n_free == 0) {
        rc = orbm_bundle_adjust_host(&P, nIterations, bRobust ? 1 : 0, stop, pbStopFlag, ORBM_POSE_ORDER_DEVICE, &R);
    } else {
        orbm_matcher* h = matcher.GetDeviceHandle();
        if (!h) return;                                    // (reported by the matcher)
        rc = orbm_bundle_adjust(h, &P, nIterations, bRobust ? 1 : 0, stop, pbStopFlag, &R);
    }
    if (rc != ORB_OK) { std::fprintf(stderr, "BundleAdjustment: %s -- nothing optimised\n", orb_last_error()); return; }

    // Recover optimized data: Keyframes (:284-302)
    for (size_t i = 0; i < vpKFs.size(); i++) {
        KeyFrame* pKF = vpKFs[i];
        if (pKF->isBad()) continue;
        const float* T = Tcw_out.data() + 16 * (size_t)pose_of[pKF];
        cv::Mat M(4, 4, CV_32F);
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) M.at<float>(r, c) = T[4 * r + c];
        if (nLoopKF == 0) {
            pKF->SetPose(M);
        } else {
            M.copyTo(pKF->mTcwGBA);
            pKF->mnBAGlobalForKF = nLoopKF;
        }
    }
    // Points (:304-328): SetWorldPos in vpMP's order; UpdateNormalAndDepth of all of them in one batched call
    std::vector<MapPoint*> vpRefresh;
    for (size_t i = 0; i < vpMP.size(); i++) {
        if (vbNotIncludedMP[i]) continue;
        MapPoint* pMP = vpMP[i];
        if (pMP->isBad()) continue;
        const float* X = point_f.data() + 3 * (size_t)row_of[i];
        cv::Mat Pos(3, 1, CV_32F);
        for (int k = 0; k < 3; ++k) Pos.at<float>(k) = X[k];
        if (nLoopKF == 0) {
            pMP->SetWorldPos(Pos);
            vpRefresh.push_back(pMP);
        } else {
            Pos.copyTo(pMP->mPosGBA);
            pMP->mnBAGlobalForKF = nLoopKF;
        }
    }
    if (!vpRefresh.empty()) RefreshMapPoints(matcher, vpRefresh, REFRESH_NORMAL_DEPTH);
}

}  // namespace ORB_SLAM2
