// Optimizer.cc -- see Optimizer.h.
#include "g2o_compat.h"
#include "Optimizer.h"

#include <cstdio>
#include <cstring>
#include "../../include/orbm.h"
#include "slam_types.h"

namespace ORB_SLAM2 {

// UNMEASURED: see Optimizer.h
const int POSE_HOST_BELOW = 16;
// tools/sim3opt_bench.py on an MI355X (profiles/r14/sim3opt_bench.json): one problem of 200 correspondences takes the host routine 352 us and
// the device call 641 us, one of 500 takes 618 against 560 us
const int SIM3OPT_HOST_BELOW = 450;

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

// ---- OptimizeSim3_cam1 ----------------------------------------------------------------------------------------------------------------
namespace {

struct FlatSim3 {   // the problems of one call and their correspondences, CSR
    std::vector<orbm_sim3opt_problem> prob;
    std::vector<int32_t> first, octave1, octave2;
    std::vector<float> x1, x2, obs1, obs2;
    std::vector<size_t> index;               // vnIndexEdge
    std::vector<uint8_t> flag;
    std::vector<orbm_sim3opt_result> res;
};
thread_local FlatSim3 tls_sim3;

bool level_table(const std::vector<float>& v, float* out, int32_t* n) {
    if (v.empty() || (int)v.size() > ORBM_MAX_LEVELS) return false;
    for (size_t k = 0; k < v.size(); ++k) out[k] = v[k];
    *n = (int32_t)v.size();
    return true;
}

// src/Optimizer.cc:2003-2167 without the g2o objects
bool flatten_sim3(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*>& vpMatches1, const g2o::Sim3& g2oS12, const float th2,
                  const bool bFixScale, FlatSim3& F) {
    orbm_sim3opt_problem P;
    std::memset(&P, 0, sizeof(P));
    // Calibration
    const cv::Mat& K1 = pKF1->mK;
    const cv::Mat& K2 = pKF2->mK;
    P.K1[0] = K1.at<float>(0, 0); P.K1[1] = K1.at<float>(1, 1); P.K1[2] = K1.at<float>(0, 2); P.K1[3] = K1.at<float>(1, 2);
    P.K2[0] = K2.at<float>(0, 0); P.K2[1] = K2.at<float>(1, 1); P.K2[2] = K2.at<float>(0, 2); P.K2[3] = K2.at<float>(1, 2);
    if (!level_table(pKF1->mvInvLevelSigma2, P.inv_level_sigma2_1, &P.n_levels1) || !level_table(pKF2->mvInvLevelSigma2, P.inv_level_sigma2_2, &P.n_levels2))
        return false;
    const auto R = g2oS12.rotation().toRotationMatrix();
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) P.R[3 * r + c] = (float)R(r, c);
        P.t[r] = (float)g2oS12.translation()[r];
    }
    P.s = (float)g2oS12.scale();
    P.th2 = th2;
    P.fix_scale = bFixScale ? 1 : 0;
    F.prob.push_back(P);

    // Camera poses
    const cv::Mat R1w = pKF1->GetRotation();
    const cv::Mat t1w = pKF1->GetTranslation();
    const cv::Mat R2w = pKF2->GetRotation();
    const cv::Mat t2w = pKF2->GetTranslation();

    const int N = vpMatches1.size();
    const std::vector<MapPoint*> vpMapPoints1 = pKF1->GetMapPointMatches_cam1();
    for (int i = 0; i < N; i++) {
        if (!vpMatches1[i])
            continue;

        MapPoint* pMP1 = vpMapPoints1[i];
        MapPoint* pMP2 = vpMatches1[i];

        const int i2 = pMP2->GetIndexInKeyFrame_cam1(pKF2);

        if (pMP1 && pMP2) {
            if (!pMP1->isBad() && !pMP2->isBad() && i2 >= 0) {
                cv::Mat P3D1w = pMP1->GetWorldPos();
                cv::Mat P3D1c = R1w * P3D1w + t1w;
                cv::Mat P3D2w = pMP2->GetWorldPos();
                cv::Mat P3D2c = R2w * P3D2w + t2w;
                for (int k = 0; k < 3; ++k) { F.x1.push_back(P3D1c.at<float>(k)); F.x2.push_back(P3D2c.at<float>(k)); }
            } else
                continue;
        } else
            continue;

        const cv::KeyPoint& kpUn1 = pKF1->mvKeysUn[i];
        const cv::KeyPoint& kpUn2 = pKF2->mvKeysUn[i2];
        F.obs1.push_back(kpUn1.pt.x); F.obs1.push_back(kpUn1.pt.y);
        F.obs2.push_back(kpUn2.pt.x); F.obs2.push_back(kpUn2.pt.y);
        F.octave1.push_back(kpUn1.octave); F.octave2.push_back(kpUn2.octave);
        F.index.push_back((size_t)i);
    }
    F.first.push_back((int32_t)F.index.size());
    return true;
}

bool run_sim3(KeyFrame* pKF1, const std::vector<KeyFrame*>& vpKF2, std::vector<std::vector<MapPoint*> >& vvpMatches1, std::vector<g2o::Sim3>& vS12,
              const float th2, const bool bFixScale, std::vector<int>& inliers) {
    FlatSim3& F = tls_sim3;
    F.prob.clear(); F.octave1.clear(); F.octave2.clear(); F.x1.clear(); F.x2.clear(); F.obs1.clear(); F.obs2.clear(); F.index.clear();
    F.first.assign(1, 0);
    const int B = (int)vpKF2.size();
    for (int b = 0; b < B; ++b)
        if (!flatten_sim3(pKF1, vpKF2[b], vvpMatches1[b], vS12[b], th2, bFixScale, F)) {
            std::fprintf(stderr, "OptimizeSim3_cam1: a keyframe has no level table -- nothing optimised\n");
            return false;
        }
    const int ne = F.first[B];
    F.flag.assign((size_t)(ne > 0 ? ne : 1), 0); F.res.resize((size_t)B);
    int rc;
    if (B == 1 && ne < SIM3OPT_HOST_BELOW) {
        rc = orbm_sim3_optimize_host(F.prob.data(), B, F.first.data(), F.x1.data(), F.x2.data(), F.obs1.data(), F.obs2.data(), F.octave1.data(),
                                     F.octave2.data(), ORBM_POSE_ORDER_DEVICE, F.flag.data(), F.res.data());
    } else {
        ORBmatcher matcher(0.6f, false);                                       // (the handle underneath is the calling thread's)
        orbm_matcher* h = matcher.GetDeviceHandle();
        if (!h) return false;                                                  // (reported by the matcher)
        rc = orbm_sim3_optimize(h, F.prob.data(), B, F.first.data(), F.x1.data(), F.x2.data(), F.obs1.data(), F.obs2.data(), F.octave1.data(),
                                F.octave2.data(), F.flag.data(), F.res.data());
    }
    if (rc) {
        std::fprintf(stderr, "OptimizeSim3_cam1: the call failed (%d): %s -- nothing optimised\n", rc, orb_last_error());
        return false;
    }
    inliers.resize((size_t)B);
    for (int b = 0; b < B; ++b) {
        const orbm_sim3opt_result& R = F.res[b];
        inliers[b] = R.n_inliers;
        for (int e = F.first[b]; e < F.first[b + 1]; ++e)
            if (F.flag[e]) vvpMatches1[b][F.index[e]] = static_cast<MapPoint*>(NULL);
        if (!R.written) continue;                                              // `return 0` (:2210-2211): g2oS12 stays
        g2o::Quaterniond q(R.q[3], R.q[0], R.q[1], R.q[2]);
        vS12[b] = g2o::Sim3(q, g2o::Vector3d(R.t[0], R.t[1], R.t[2]), R.s);
    }
    return true;
}

}  // namespace

int Optimizer::OptimizeSim3_cam1(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches1, g2o::Sim3& g2oS12, const float th2,
                                 const bool bFixScale) {
    std::vector<std::vector<MapPoint*> > matches(1);
    matches[0].swap(vpMatches1);
    std::vector<g2o::Sim3> s12(1, g2oS12);
    std::vector<int> n;
    const bool ok = run_sim3(pKF1, std::vector<KeyFrame*>(1, pKF2), matches, s12, th2, bFixScale, n);
    vpMatches1.swap(matches[0]);
    if (!ok) return 0;
    g2oS12 = s12[0];
    return n[0];
}

bool Optimizer::OptimizeSim3Batch(KeyFrame* pKF1, const std::vector<KeyFrame*>& vpKF2, std::vector<std::vector<MapPoint*> >& vvpMatches1,
                                  std::vector<g2o::Sim3>& vg2oS12, const float th2, const bool bFixScale, std::vector<int>& vnInliers) {
    vnInliers.clear();
    if (vpKF2.empty()) return true;
    if (vpKF2.size() != vvpMatches1.size() || vpKF2.size() != vg2oS12.size()) { std::fprintf(stderr, "OptimizeSim3Batch: the three vectors differ in length\n"); return false; }
    if ((int)vpKF2.size() > ORBM_SIM3OPT_MAX_BATCH) { std::fprintf(stderr, "OptimizeSim3Batch: %d candidates, at most %d\n", (int)vpKF2.size(), (int)ORBM_SIM3OPT_MAX_BATCH); return false; }
    return run_sim3(pKF1, vpKF2, vvpMatches1, vg2oS12, th2, bFixScale, vnInliers);
}

}  // namespace ORB_SLAM2
