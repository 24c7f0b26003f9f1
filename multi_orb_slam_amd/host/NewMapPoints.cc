// NewMapPoints.cc -- see NewMapPoints.h.
#include "NewMapPoints.h"

#include <cstdio>
#include <cstring>
#include "../../include/orbv.h"

namespace ORB_SLAM2 {

// UNMEASURED: see NewMapPoints.h
const int TRIANGULATE_HOST_BELOW = 16;

namespace {

// One keyframe as orbv_tri_keyframe reads it.  Everything goes through public members of the reference's KeyFrame: the pose getters,
// GetPoseInverse() for Twc (protected there), the intrinsics, mRcam12 / mtcam12, the keypoint vectors and the two level tables.
struct Flat {
    orbv_tri_keyframe k;
    std::vector<float> x, y, xd, yd, uright, depth, cos_stereo;
    std::vector<int32_t> octave, cam_of;
};

void copy34(const cv::Mat& R, const cv::Mat& t, float* dst) {
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) dst[4 * r + c] = R.at<float>(r, c);
        dst[4 * r + 3] = t.at<float>(r);
    }
}

void flatten(KeyFrame* pKF, Flat& F) {
    std::memset(&F.k, 0, sizeof(F.k));
    copy34(pKF->GetRotation(), pKF->GetTranslation(), F.k.Tcw[0]);
    copy34(pKF->GetRotation_cam2(), pKF->GetTranslation_cam2(), F.k.Tcw[1]);
    const cv::Mat Ow = pKF->GetCameraCenter(), Ow2 = pKF->GetCameraCenter_cam2();
    for (int c = 0; c < 3; ++c) { F.k.centre[0][c] = Ow.at<float>(c); F.k.centre[1][c] = Ow2.at<float>(c); }
    const cv::Mat Twc = pKF->GetPoseInverse();
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) F.k.Twc[4 * r + c] = Twc.at<float>(r, c);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) F.k.Rcam12[3 * r + c] = pKF->mRcam12.at<float>(r, c);
        F.k.tcam12[r] = pKF->mtcam12.at<float>(r);
    }
    F.k.fx = pKF->fx; F.k.fy = pKF->fy; F.k.cx = pKF->cx; F.k.cy = pKF->cy; F.k.invfx = pKF->invfx; F.k.invfy = pKF->invfy; F.k.mbf = pKF->mbf;
    F.k.n_levels = (int)pKF->mvScaleFactors.size();
    F.k.scale_factors = pKF->mvScaleFactors.data(); F.k.level_sigma2 = pKF->mvLevelSigma2.data();
    const int n = (int)pKF->mvKeysUn_total.size();
    F.k.n = n; F.k.n_cam1 = pKF->N;
    F.x.resize(n); F.y.resize(n); F.xd.resize(n); F.yd.resize(n); F.uright.resize(n); F.depth.resize(n); F.cos_stereo.resize(n);
    F.octave.resize(n); F.cam_of.resize(n);
    for (int i = 0; i < n; ++i) {
        const cv::KeyPoint& un = pKF->mvKeysUn_total[i];
        const cv::KeyPoint& kp = pKF->mvKeys_total[i];
        F.x[i] = un.pt.x; F.y[i] = un.pt.y; F.octave[i] = un.octave;
        F.xd[i] = kp.pt.x; F.yd[i] = kp.pt.y;
        F.uright[i] = pKF->mvuRight_total[i]; F.depth[i] = pKF->mvDepth_total[i];
        F.cam_of[i] = pKF->keypoint_to_cam.find(i)->second;                    // :410
    }
    orbv_cos_stereo(pKF->mb, F.depth.data(), n, F.cos_stereo.data());          // :447, :449 -- read where uright >= 0 only
    F.k.x = F.x.data(); F.k.y = F.y.data(); F.k.xd = F.xd.data(); F.k.yd = F.yd.data(); F.k.octave = F.octave.data();
    F.k.uright = F.uright.data(); F.k.depth = F.depth.data(); F.k.cos_stereo = F.cos_stereo.data(); F.k.cam_of = F.cam_of.data();
}

struct Scratch {   // per calling thread, like the matcher handle
    Flat f1, f2;
    std::vector<int32_t> pairs;
    std::vector<orbv_tri_out> rec;
};
thread_local Scratch tls_scratch;

}  // namespace

bool TriangulateMatches(ORBmatcher& matcher, KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<std::pair<size_t, size_t> >& vMatchedIndices,
                        const std::vector<bool>& istrian, std::vector<TriangulatedPair>& out) {
    out.clear();
    const int n = (int)vMatchedIndices.size();
    if (n == 0) return true;
    Scratch& S = tls_scratch;
    flatten(pKF1, S.f1); flatten(pKF2, S.f2);
    S.pairs.resize(2 * (size_t)n); S.rec.resize((size_t)n);
    for (int i = 0; i < n; ++i) { S.pairs[2 * i] = (int32_t)vMatchedIndices[i].first; S.pairs[2 * i + 1] = (int32_t)vMatchedIndices[i].second; }
    const uint8_t enabled[2] = {(uint8_t)(istrian.size() > 0 && istrian[0]), (uint8_t)(istrian.size() > 1 && istrian[1])};
    const float ratioFactor = 1.5f * pKF1->mfScaleFactor;                      // :308
    int rc;
    if (n < TRIANGULATE_HOST_BELOW) {
        rc = orbv_triangulate_pairs_host(&S.f1.k, &S.f2.k, enabled, S.pairs.data(), n, ratioFactor, S.rec.data());
    } else {
        orbv_workspace* w = matcher.GetBowWorkspace();
        if (!w) return false;                                                   // (reported by the matcher)
        rc = orbv_triangulate_pairs(w, &S.f1.k, &S.f2.k, enabled, S.pairs.data(), n, ratioFactor, S.rec.data());
    }
    if (rc) {
        std::fprintf(stderr, "TriangulateMatches: the triangulation call failed (%d): %s -- no points created\n", rc, orb_last_error());
        return false;
    }
    out.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        const orbv_tri_out& o = S.rec[i];
        out[i].outcome = o.outcome;
        out[i].accepted = o.outcome == ORBV_TRI_ACCEPTED;
        if (o.path != ORBV_TRI_PATH_NONE) {
            out[i].x3D = cv::Mat(3, 1, CV_32F);
            for (int k = 0; k < 3; ++k) out[i].x3D.at<float>(k) = o.x3D[k];
        }
    }
    return true;
}

}  // namespace ORB_SLAM2
