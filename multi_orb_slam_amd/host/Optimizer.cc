// Optimizer.cc -- see Optimizer.h.
#include "Optimizer.h"

#include <cstdio>
#include <cstring>
#include "../../include/orbm.h"

namespace ORB_SLAM2 {

// UNMEASURED: see Optimizer.h
const int POSE_HOST_BELOW = 16;

namespace {

struct Flat {   // the problems of one call and their edges, CSR
    std::vector<orbm_pose_problem> prob;
    std::vector<int32_t> first, feat, octave;
    std::vector<float> pos, obs;
    std::vector<uint8_t> outlier;
    std::vector<orbm_pose_result> res;
};
thread_local Flat tls_flat;

// src/Optimizer.cc:371-516 / :641-793 without the g2o objects: one edge per feature with a map point
bool flatten(Frame* pFrame, bool bAllCams, Flat& F) {
    orbm_pose_problem P;
    std::memset(&P, 0, sizeof(P));
    if (pFrame->mTcw.empty()) return false;
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) P.Tcw[4 * r + c] = pFrame->mTcw.at<float>(r, c);
    P.fx = pFrame->fx; P.fy = pFrame->fy; P.cx = pFrame->cx; P.cy = pFrame->cy; P.bf = pFrame->mbf;
    for (int k = 0; k < 9; ++k) P.Rcam12[k] = k % 4 == 0 ? 1.0f : 0.0f;
    if (bAllCams) {
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) P.Rcam12[3 * r + c] = pFrame->mRcam12.at<float>(r, c);
            P.tcam12[r] = pFrame->mtcam12.at<float>(r);
        }
    }
    const int L = (int)pFrame->mvInvLevelSigma2.size();
    if (L < 1 || L > ORBM_MAX_LEVELS) return false;
    for (int k = 0; k < L; ++k) P.inv_level_sigma2[k] = pFrame->mvInvLevelSigma2[k];
    P.n_levels = L;
    P.mode = bAllCams ? ORBM_POSE_ALL_CAMS : ORBM_POSE_CAM0;
    P.n_cam0 = pFrame->N;
    F.prob.push_back(P);
    const int N = bAllCams ? pFrame->N_total : pFrame->N;                      // :671 / :398
    for (int i = 0; i < N; i++) {
        MapPoint* pMP = pFrame->mvpMapPoints[i];
        if (!pMP) continue;
        pFrame->mvbOutlier[i] = false;                                         // :431, :471
        const cv::KeyPoint& kpUn = bAllCams ? pFrame->mvKeysUn_total[i] : pFrame->mvKeysUn[i];
        const float kp_ur = bAllCams ? pFrame->mvuRight_total[i] : pFrame->mvuRight[i];
        const cv::Mat Xw = pMP->GetWorldPos();
        F.feat.push_back(i); F.octave.push_back(kpUn.octave);
        F.obs.push_back(kpUn.pt.x); F.obs.push_back(kpUn.pt.y); F.obs.push_back(kp_ur);
        for (int k = 0; k < 3; ++k) F.pos.push_back(Xw.at<float>(k));
    }
    F.first.push_back((int32_t)F.feat.size());
    return true;
}

bool run(const std::vector<Frame*>& frames, bool bAllCams, std::vector<int>& inliers) {
    Flat& F = tls_flat;
    F.prob.clear(); F.feat.clear(); F.octave.clear(); F.pos.clear(); F.obs.clear();
    F.first.assign(1, 0);
    const int B = (int)frames.size();
    for (Frame* f : frames)
        if (!flatten(f, bAllCams, F)) { std::fprintf(stderr, "PoseOptimization: the frame has no pose or no level table -- nothing optimised\n"); return false; }
    const int ne = F.first[B];
    F.outlier.assign((size_t)(ne > 0 ? ne : 1), 0); F.res.resize((size_t)B);
    int rc;
    if (B == 1 && ne < POSE_HOST_BELOW) {
        rc = orbm_pose_optimize_host(F.prob.data(), B, F.first.data(), F.feat.data(), F.pos.data(), F.obs.data(), F.octave.data(),
                                     ORBM_POSE_ORDER_DEVICE, F.outlier.data(), F.res.data());
    } else {
        ORBmatcher matcher(0.6f, false);                                       // (the handle underneath is the calling thread's)
        orbm_matcher* h = matcher.GetDeviceHandle();
        if (!h) return false;                                                  // (reported by the matcher)
        rc = orbm_pose_optimize(h, F.prob.data(), B, F.first.data(), F.feat.data(), F.pos.data(), F.obs.data(), F.octave.data(),
                                F.outlier.data(), F.res.data());
    }
    if (rc) {
        std::fprintf(stderr, "PoseOptimization: the call failed (%d): %s -- nothing optimised\n", rc, orb_last_error());
        return false;
    }
    inliers.resize((size_t)B);
    for (int b = 0; b < B; ++b) {
        Frame* pFrame = frames[b];
        const orbm_pose_result& R = F.res[b];
        inliers[b] = R.n_inliers;
        if (R.n_initial < 3) continue;                                         // `return 0` before anything else is written (:519)
        for (int e = F.first[b]; e < F.first[b + 1]; ++e) pFrame->mvbOutlier[F.feat[e]] = F.outlier[e] != 0;
        cv::Mat pose(4, 4, CV_32F);                                            // Converter::toCvMat(SE3quat_recov)
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) pose.at<float>(r, c) = R.Tcw[4 * r + c];
        pFrame->SetPose(pose);
    }
    return true;
}

}  // namespace

int Optimizer::PoseOptimization(Frame* pFrame) {
    std::vector<int> n;
    return run(std::vector<Frame*>(1, pFrame), false, n) ? n[0] : 0;
}

int Optimizer::PoseOptimization(Frame* pFrame, bool bAllCams) {
    // (the reference's second overload is the all-cameras form whatever the flag says: :620-898 never reads bAllCams)
    (void)bAllCams;
    std::vector<int> n;
    return run(std::vector<Frame*>(1, pFrame), true, n) ? n[0] : 0;
}

bool Optimizer::PoseOptimizationBatch(const std::vector<Frame*>& vpFrames, bool bAllCams, std::vector<int>& vnInliers) {
    vnInliers.clear();
    if (vpFrames.empty()) return true;
    if ((int)vpFrames.size() > ORBM_POSE_MAX_BATCH) { std::fprintf(stderr, "PoseOptimizationBatch: %d frames, at most %d\n", (int)vpFrames.size(), (int)ORBM_POSE_MAX_BATCH); return false; }
    return run(vpFrames, bAllCams, vnInliers);
}

}  // namespace ORB_SLAM2
