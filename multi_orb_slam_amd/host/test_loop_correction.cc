// test_loop_correction.cc -- driver of CorrectLoopMap / UpdateMapAfterGlobalBA (host/LoopCorrection.h) for
// tests/test_loop_correction_class.py.
//
//   test_loop_correction host     no device: seeded stand-in maps and hand-built cases, every one built twice from the same draws.  On one
//                                 twin runs a transcription of the reference on the stand-in types -- LoopClosing::CorrectLoop's steps
//                                 4.1-4.4 (src/LoopClosing.cc:645-727) with MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:480-528) per
//                                 point, and the map update behind a global BA (:925-989) --, on the other the two drop-ins over a
//                                 host-only ResidentMap.  Compared per point: position, normal, distance band, mnCorrectedByKF,
//                                 mnCorrectedReference; per keyframe: the pose, mTcwBefGBA, the connections; the two Sim3 maps.  After
//                                 UpdateMapAfterGlobalBA: Audit() == 0 and nothing for a Flush to send.  (Every keyframe of these worlds
//                                 claims fewer points than REFRESH_HOST_BELOW, so the refresh too needs no device.)
//   test_loop_correction device   the same cases and larger ones with the ResidentMap on the device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>
#include <memory>
#include <string>
#include <vector>
#include "../../include/orbm.h"
#include "LoopCorrection.h"
#include "MapPointRefresh.h"

using namespace ORB_SLAM2;

namespace {

struct Rng {   // (one generator for both twins of a world)
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 1) {}
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    int below(int n) { return (int)(next() % (uint32_t)n); }
    bool chance(int percent) { return below(100) < percent; }
    float real(float lo, float hi) { return lo + (hi - lo) * (float)(next() & 0xffffff) / 16777216.0f; }
};

struct World {
    int nk = 0, np = 0, nf = 0;
    std::unique_ptr<KeyFrame[]> kfs;      // contiguous: pointer order is index order, in both twins
    std::unique_ptr<MapPoint[]> pts;
    Map map;
    std::vector<KeyFrame*> connected;     // mvpCurrentConnectedKFs (the current keyframe among them)
    int current = 0;
    g2o::Sim3 Scw;
    unsigned long nLoopKF = 7;
    std::vector<KeyFrame*> all_kfs() { std::vector<KeyFrame*> v; for (int k = 0; k < nk; ++k) v.push_back(&kfs[k]); return v; }
    std::vector<MapPoint*> all_pts() { std::vector<MapPoint*> v; for (int p = 0; p < np; ++p) v.push_back(&pts[p]); return v; }
};

cv::Mat random_pose(Rng& r, float spread) {   // a rotation about a random axis built from a quaternion, a translation within `spread`
    float q[4]; float n = 0;
    for (float& c : q) { c = r.real(-1.f, 1.f); n += c * c; }
    n = std::sqrt(n); if (n < 1e-3f) { q[3] = 1.f; n = 1.f; }
    const float x = q[0] / n, y = q[1] / n, z = q[2] / n, w = q[3] / n;
    cv::Mat T = cv::Mat::eye(4, 4, CV_32F);
    const float R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                        2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) T.at<float>(i, j) = R[3 * i + j]; T.at<float>(i, 3) = r.real(-spread, spread); }
    return T;
}

void alloc(World& w, int nk, int np, int nf) {
    w.nk = nk; w.np = np; w.nf = nf;
    w.kfs.reset(new KeyFrame[nk]); w.pts.reset(new MapPoint[np]);
    for (int k = 0; k < nk; ++k) {
        KeyFrame& kf = w.kfs[k];
        kf.mnId = k; kf.N = nf * 2 / 3; kf.N_total = nf; kf.mThDepth = 10.f;
        kf.mvpMapPoints.assign((size_t)nf, nullptr);
        kf.mvKeysUn_total.assign((size_t)nf, cv::KeyPoint()); kf.mvDepth_total.assign((size_t)nf, 1.f); kf.mvuRight_total.assign((size_t)nf, -1.f);
        kf.mnScaleLevels = 8; kf.mvScaleFactors.assign(8, 1.f);
        for (int l = 1; l < 8; ++l) kf.mvScaleFactors[(size_t)l] = kf.mvScaleFactors[(size_t)l - 1] * 1.2f;
        for (int f = 0; f < nf; ++f) { kf.keypoint_to_cam[(size_t)f] = 0; kf.cont_idx_to_local_cam_idx[(size_t)f] = f; }
        w.map.mvpKeyFrames.push_back(&kf);
    }
    for (int p = 0; p < np; ++p) {
        MapPoint& mp = w.pts[p];
        mp.mnId = p; mp.nObs = 0;
        mp.mWorldPos = cv::Mat(3, 1, CV_32F); mp.mNormalVector = cv::Mat(3, 1, CV_32F); mp.mDescriptor = cv::Mat(1, 32, CV_8U);
        for (int k = 0; k < 3; ++k) mp.mNormalVector.at<float>(k) = 0.5f;
        for (int k = 0; k < 32; ++k) mp.mDescriptor.ptr(0)[k] = (uint8_t)(p + k);
        mp.mfMinDistance = 1.f; mp.mfMaxDistance = 9.f;
        w.map.mvpMapPoints.push_back(&mp);
    }
}

void observe(World& w, int p, int k, int idx) {
    MapPoint& mp = w.pts[p]; KeyFrame& kf = w.kfs[k];
    if (mp.mObservations.count(&kf) || kf.mvpMapPoints[(size_t)idx]) return;
    mp.mObservations[&kf] = (size_t)idx; mp.nObs += 1;
    kf.mvpMapPoints[(size_t)idx] = &mp;
    if (!mp.mpRefKF) mp.mpRefKF = &kf;
}

// nk keyframes of nf features on a chain of parents, np points seen by about `observers` keyframes each.  The connected keyframes of
// the loop are the last `n_conn`; the current keyframe is the middle one of them, so that keyframes lie before and after it in
// CorrectedSim3's (pointer) order.  Global BA has "optimised" most keyframes and points (mTcwGBA, mPosGBA, the marks).
void build(World& w, uint64_t seed, int nk, int np, int nf, int observers, int n_conn, bool scale_one) {
    Rng r(seed);
    alloc(w, nk, np, nf);
    for (int k = 0; k < nk; ++k) {
        KeyFrame& kf = w.kfs[k];
        kf.Tcw = random_pose(r, 3.f); kf.Tcw_cam2 = kf.Tcw.clone();
        for (int f = 0; f < nf; ++f) kf.mvKeysUn_total[(size_t)f].octave = r.below(8);
        if (k > 0) { kf.mpParent = &w.kfs[r.below(k)]; kf.mpParent->mspChildrens.insert(&kf); kf.mbFirstConnection = false; }
        if (k == 0 || r.chance(75)) { kf.mnBAGlobalForKF = w.nLoopKF; kf.mTcwGBA = random_pose(r, 3.f); }
    }
    w.map.mvpKeyFrameOrigins.push_back(&w.kfs[0]);
    for (int p = 0; p < np; ++p) {
        MapPoint& mp = w.pts[p];
        for (int k = 0; k < 3; ++k) mp.mWorldPos.at<float>(k) = r.real(-8.f, 8.f);
        mp.mbBad = r.chance(6);
        const int n = std::max(1, observers - 2 + r.below(5));
        for (int o = 0; o < n; ++o) observe(w, p, r.below(nk), r.below(nf));
        if (mp.mObservations.empty()) mp.mbBad = true;       // every feature drawn was taken: no observation, no reference keyframe (the
                                                             // reference has no such point alive: :972 would read a NULL pRefKF)
        if (r.chance(60)) { mp.mnBAGlobalForKF = w.nLoopKF; mp.mPosGBA = cv::Mat(3, 1, CV_32F); for (int k = 0; k < 3; ++k) mp.mPosGBA.at<float>(k) = r.real(-8.f, 8.f); }
    }
    // a point observed by a connected keyframe BEFORE and one AFTER its claimant: claimed by the second connected keyframe (its first
    // free feature), seen by the first and the last too
    for (int k = 0; k < nk; k += 3)                           // a row with the same point twice
        for (int f = 0; f + 1 < nf; ++f)
            if (w.kfs[k].mvpMapPoints[(size_t)f] && !w.kfs[k].mvpMapPoints[(size_t)f + 1]) { w.kfs[k].mvpMapPoints[(size_t)f + 1] = w.kfs[k].mvpMapPoints[(size_t)f]; break; }
    n_conn = std::min(n_conn, nk);
    for (int k = nk - n_conn; k < nk; ++k) w.connected.push_back(&w.kfs[k]);
    w.current = nk - n_conn + n_conn / 2;
    // a point observed by a connected keyframe BEFORE and one AFTER its claimant: point 0 is seen by the first, the second and the last
    // connected keyframe, and the first no longer holds it in its row (the observation stays) -- the second one claims it.  Point 1 is
    // bad: it stays where it is in both passes.
    if (n_conn >= 3 && np >= 2) {
        MapPoint& mp = w.pts[0];
        mp.mbBad = false;
        const int ks[3] = {nk - n_conn, nk - n_conn + 1, nk - 1};
        for (int k : ks)
            for (int f = 0; f < nf && !mp.mObservations.count(&w.kfs[k]); ++f) observe(w, 0, k, f);
        KeyFrame& first = w.kfs[ks[0]];
        for (auto& held : first.mvpMapPoints) if (held == &mp) held = nullptr;
        w.pts[1].mbBad = true;
    }
    const cv::Mat Tcw = random_pose(r, 3.f);
    g2o::Matrix3d R; for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) R(i, j) = (double)Tcw.at<float>(i, j);
    w.Scw = g2o::Sim3(R, g2o::Vector3d(Tcw.at<float>(0, 3), Tcw.at<float>(1, 3), Tcw.at<float>(2, 3)), scale_one ? 1.0 : 1.0 + 0.01 * (double)r.below(30));
}

// ---- the reference, transcribed onto the stand-in types ------------------------------------------------------------------------------
void ref_update_normal_and_depth(MapPoint* pMP) {   // src/MapPoint.cc:480-528
    std::map<KeyFrame*, size_t> observations = pMP->mObservations;
    KeyFrame* pRefKF = pMP->mpRefKF;
    if (pMP->mbBad) return;
    cv::Mat Pos = pMP->mWorldPos.clone();
    if (observations.empty()) return;
    cv::Mat normal = cv::Mat::zeros(3, 1, CV_32F);
    int n = 0;
    for (auto& ob : observations) {
        KeyFrame* pKF = ob.first;
        const int cam = pKF->keypoint_to_cam.find(ob.second)->second;
        std::vector<cv::Mat> Owi = {pKF->GetCameraCenter(), pKF->GetCameraCenter_cam2()};
        cv::Mat normali = pMP->mWorldPos - Owi[cam];
        normal = normal + normali / cv::norm(normali);
        n++;
    }
    cv::Mat PC = Pos - pRefKF->GetCameraCenter();
    const float dist = cv::norm(PC);
    const int level = pRefKF->mvKeysUn_total[observations[pRefKF]].octave;
    const float levelScaleFactor = pRefKF->mvScaleFactors[level];
    const int nLevels = pRefKF->mnScaleLevels;
    pMP->mfMaxDistance = dist * levelScaleFactor;
    pMP->mfMinDistance = pMP->mfMaxDistance / pRefKF->mvScaleFactors[nLevels - 1];
    pMP->mNormalVector = normal / n;
}

g2o::Sim3 ref_sim3(const cv::Mat& T) {   // Converter::toMatrix3d, toVector3d, g2o::Sim3(R, t, 1.0)
    g2o::Matrix3d R; for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) R(i, j) = (double)T.at<float>(i, j);
    return g2o::Sim3(R, g2o::Vector3d((double)T.at<float>(0, 3), (double)T.at<float>(1, 3), (double)T.at<float>(2, 3)), 1.0);
}

void ref_correct_loop(World& w, LoopClosing::KeyFrameAndPose& CorrectedSim3, LoopClosing::KeyFrameAndPose& NonCorrectedSim3) {   // src/LoopClosing.cc:631-727
    KeyFrame* mpCurrentKF = &w.kfs[w.current];
    CorrectedSim3[mpCurrentKF] = w.Scw;
    cv::Mat Twc = mpCurrentKF->GetPoseInverse();
    for (KeyFrame* pKFi : w.connected) {
        cv::Mat Tiw = pKFi->GetPose();
        if (pKFi != mpCurrentKF) {
            cv::Mat Tic = Tiw * Twc;
            g2o::Sim3 g2oSic = ref_sim3(Tic);
            g2o::Sim3 g2oCorrectedSiw = g2oSic * w.Scw;
            CorrectedSim3[pKFi] = g2oCorrectedSiw;
        }
        NonCorrectedSim3[pKFi] = ref_sim3(Tiw);
    }
    for (auto mit = CorrectedSim3.begin(), mend = CorrectedSim3.end(); mit != mend; mit++) {
        KeyFrame* pKFi = mit->first;
        g2o::Sim3 g2oCorrectedSiw = mit->second;
        g2o::Sim3 g2oCorrectedSwi = g2oCorrectedSiw.inverse();
        g2o::Sim3 g2oSiw = NonCorrectedSim3[pKFi];
        std::vector<MapPoint*> vpMPsi = pKFi->GetMapPointMatches();
        for (size_t iMP = 0, endMPi = vpMPsi.size(); iMP < endMPi; iMP++) {
            MapPoint* pMPi = vpMPsi[iMP];
            if (!pMPi) continue;
            if (pMPi->isBad()) continue;
            if (pMPi->mnCorrectedByKF == mpCurrentKF->mnId) continue;
            cv::Mat P3Dw = pMPi->GetWorldPos();
            g2o::Vector3d eigP3Dw((double)P3Dw.at<float>(0), (double)P3Dw.at<float>(1), (double)P3Dw.at<float>(2));
            g2o::Vector3d eigCorrectedP3Dw = g2oCorrectedSwi.map(g2oSiw.map(eigP3Dw));
            cv::Mat cvCorrectedP3Dw(3, 1, CV_32F);
            for (int k = 0; k < 3; ++k) cvCorrectedP3Dw.at<float>(k) = (float)eigCorrectedP3Dw[k];
            pMPi->SetWorldPos(cvCorrectedP3Dw);
            pMPi->mnCorrectedByKF = mpCurrentKF->mnId;
            pMPi->mnCorrectedReference = pKFi->mnId;
            ref_update_normal_and_depth(pMPi);
        }
        g2o::Matrix3d eigR = g2oCorrectedSiw.rotation().toRotationMatrix();
        g2o::Vector3d eigt = g2oCorrectedSiw.translation();
        double s = g2oCorrectedSiw.scale();
        for (int k = 0; k < 3; ++k) eigt[k] *= (1. / s);
        cv::Mat correctedTiw = cv::Mat::eye(4, 4, CV_32F);
        for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) correctedTiw.at<float>(i, j) = (float)eigR(i, j); correctedTiw.at<float>(i, 3) = (float)eigt[i]; }
        pKFi->SetPose(correctedTiw);
        pKFi->UpdateConnections();
    }
}

void ref_after_global_ba(World& w) {   // src/LoopClosing.cc:925-989
    Map* mpMap = &w.map; const unsigned long nLoopKF = w.nLoopKF;
    std::list<KeyFrame*> lpKFtoCheck(mpMap->mvpKeyFrameOrigins.begin(), mpMap->mvpKeyFrameOrigins.end());
    while (!lpKFtoCheck.empty()) {
        KeyFrame* pKF = lpKFtoCheck.front();
        const std::set<KeyFrame*> sChilds = pKF->GetChilds();
        cv::Mat Twc = pKF->GetPoseInverse();
        for (std::set<KeyFrame*>::const_iterator sit = sChilds.begin(); sit != sChilds.end(); sit++) {
            KeyFrame* pChild = *sit;
            if (pChild->mnBAGlobalForKF != nLoopKF) {
                cv::Mat Tchildc = pChild->GetPose() * Twc;
                pChild->mTcwGBA = Tchildc * pKF->mTcwGBA;
                pChild->mnBAGlobalForKF = nLoopKF;
            }
            lpKFtoCheck.push_back(pChild);
        }
        pKF->mTcwBefGBA = pKF->GetPose();
        pKF->SetPose(pKF->mTcwGBA);
        lpKFtoCheck.pop_front();
    }
    const std::vector<MapPoint*> vpMPs = mpMap->GetAllMapPoints();
    for (size_t i = 0; i < vpMPs.size(); i++) {
        MapPoint* pMP = vpMPs[i];
        if (pMP->isBad()) continue;
        if (pMP->mnBAGlobalForKF == nLoopKF) pMP->SetWorldPos(pMP->mPosGBA);
        else {
            KeyFrame* pRefKF = pMP->GetReferenceKeyFrame();
            if (pRefKF->mnBAGlobalForKF != nLoopKF) continue;
            cv::Mat Rcw = pRefKF->mTcwBefGBA.rowRange(0, 3).colRange(0, 3);
            cv::Mat tcw = pRefKF->mTcwBefGBA.rowRange(0, 3).col(3);
            cv::Mat Xc = Rcw * pMP->GetWorldPos() + tcw;
            cv::Mat Twc = pRefKF->GetPoseInverse();
            cv::Mat Rwc = Twc.rowRange(0, 3).colRange(0, 3);
            cv::Mat twc = Twc.rowRange(0, 3).col(3);
            pMP->SetWorldPos(Rwc * Xc + twc);
        }
    }
}

// ---- comparison
bool same_mat(const cv::Mat& a, const cv::Mat& b) {
    if (a.empty() || b.empty()) return a.empty() == b.empty();
    if (a.rows != b.rows || a.cols != b.cols) return false;
    for (int i = 0; i < a.rows; ++i) for (int j = 0; j < a.cols; ++j) if (std::memcmp(&a.at<float>(i, j), &b.at<float>(i, j), 4) != 0) return false;
    return true;
}
bool same_sim3(const g2o::Sim3& a, const g2o::Sim3& b) {
    return std::memcmp(a.rotation().coeffs(), b.rotation().coeffs(), 32) == 0 && std::memcmp(&a.translation()[0], &b.translation()[0], 24) == 0 && a.scale() == b.scale();
}
int idx_of(World& w, KeyFrame* k) { return k ? (int)(k - w.kfs.get()) : -1; }

int compare(World& a, World& b, const char* what) {
    int diff = 0, moved = 0;
    for (int p = 0; p < a.np; ++p) {
        MapPoint &x = a.pts[p], &y = b.pts[p];
        if (!same_mat(x.mWorldPos, y.mWorldPos) || !same_mat(x.mNormalVector, y.mNormalVector) || std::memcmp(&x.mfMinDistance, &y.mfMinDistance, 4) ||
            std::memcmp(&x.mfMaxDistance, &y.mfMaxDistance, 4) || x.mnCorrectedByKF != y.mnCorrectedByKF || x.mnCorrectedReference != y.mnCorrectedReference) {
            if (++diff <= 5) std::printf("FAIL %s: point %d differs\n", what, p);
        }
    }
    for (int k = 0; k < a.nk; ++k) {
        KeyFrame &x = a.kfs[k], &y = b.kfs[k];
        bool same = same_mat(x.Tcw, y.Tcw) && same_mat(x.mTcwBefGBA, y.mTcwBefGBA) && same_mat(x.mTcwGBA, y.mTcwGBA) && x.mnBAGlobalForKF == y.mnBAGlobalForKF &&
                    x.mvOrderedWeights == y.mvOrderedWeights && x.mvpOrderedConnectedKeyFrames.size() == y.mvpOrderedConnectedKeyFrames.size();
        for (size_t i = 0; same && i < x.mvpOrderedConnectedKeyFrames.size(); ++i)
            same = idx_of(a, x.mvpOrderedConnectedKeyFrames[i]) == idx_of(b, y.mvpOrderedConnectedKeyFrames[i]);
        if (!same && ++diff <= 5) std::printf("FAIL %s: keyframe %d differs\n", what, k);
    }
    (void)moved;
    return diff;
}

ResidentMap::Capacity capacity_for(const World& w) {
    ResidentMap::Capacity c;
    c.keyframes = w.nk + 2; c.points = w.np + 8; c.observations = w.np * 12 + 64; c.features_per_keyframe = w.nf;
    return c;
}

typedef void (*Maker)(World&);

int loop_case(ORBmatcher* device, const char* name, Maker make) {
    World a, b;
    make(a); make(b);
    ORBmatcher host_matcher(0.8f, true);
    ORBmatcher& matcher = device ? *device : host_matcher;
    std::vector<float> before;
    for (int p = 0; p < a.np; ++p) for (int k = 0; k < 3; ++k) before.push_back(a.pts[p].mWorldPos.at<float>(k));
    LoopClosing::KeyFrameAndPose refC, refN, gotC, gotN;
    ref_correct_loop(a, refC, refN);
    ResidentMap R(device, capacity_for(b));
    for (KeyFrame* k : b.all_kfs()) R.Touch(k);
    for (MapPoint* p : b.all_pts()) R.Touch(p);
    if (R.Flush() < 0) { std::printf("FAIL %s: Flush\n", name); return 1; }
    gotC[&b.kfs[b.current]] = b.Scw;
    CorrectLoopMap(R, matcher, &b.kfs[b.current], b.connected, b.Scw, gotC, gotN);
    int diff = compare(a, b, name);
    if (refC.size() != gotC.size() || refN.size() != gotN.size()) { std::printf("FAIL %s: the Sim3 maps differ in size\n", name); ++diff; }
    else {
        auto x = refC.begin(); auto y = gotC.begin();
        for (; x != refC.end(); ++x, ++y) if (idx_of(a, x->first) != idx_of(b, y->first) || !same_sim3(x->second, y->second)) { std::printf("FAIL %s: CorrectedSim3 differs\n", name); ++diff; break; }
        auto u = refN.begin(); auto v = gotN.begin();
        for (; u != refN.end(); ++u, ++v) if (idx_of(a, u->first) != idx_of(b, v->first) || !same_sim3(u->second, v->second)) { std::printf("FAIL %s: NonCorrectedSim3 differs\n", name); ++diff; break; }
    }
    // what the case must hold: corrected points, and one seen by connected keyframes before and after its claimant
    int corrected = 0, straddled = 0, max_batch = 0;
    std::map<unsigned long, int> batch;
    for (int p = 0; p < a.np; ++p) {
        MapPoint& mp = a.pts[p];
        if (mp.mnCorrectedByKF != a.kfs[a.current].mnId || mp.mbBad) continue;
        ++corrected; max_batch = std::max(max_batch, ++batch[mp.mnCorrectedReference]);
        bool lower = false, higher = false;
        for (auto& ob : mp.mObservations) {
            if (!refC.count(ob.first)) continue;
            if (ob.first->mnId < mp.mnCorrectedReference) lower = true;
            if (ob.first->mnId > mp.mnCorrectedReference) higher = true;
        }
        straddled += lower && higher;
    }
    // the refreshed rows were Touched, the positions were written by the call: after one Flush the map agrees with the host
    const int sent = R.Flush();
    const int audit = R.Audit(b.all_kfs(), b.all_pts());
    if (audit) { std::printf("FAIL %s: Audit %d\n", name, audit); ++diff; }
    int cor[4]; R.LastCorrection(cor);
    std::printf("loop %s: %d keyframes, %d points corrected (largest batch %d), %d seen before and after their claimant, flush %d, device %d, %d differ\n", name,
                (int)refC.size(), corrected, max_batch, straddled, sent, cor[0], diff);
    if (corrected == 0 || straddled == 0) { std::printf("FAIL %s: the case holds no such point\n", name); ++diff; }
    if (!device && max_batch >= REFRESH_HOST_BELOW) { std::printf("FAIL %s: a batch of %d needs the device\n", name, max_batch); ++diff; }
    if (device && cor[0] != 1) { std::printf("FAIL %s: the call did not run on the device\n", name); ++diff; }
    return diff;
}

int gba_case(ORBmatcher* device, const char* name, Maker make) {
    World a, b;
    make(a); make(b);
    ref_after_global_ba(a);
    ResidentMap R(device, capacity_for(b));
    for (KeyFrame* k : b.all_kfs()) R.Touch(k);
    for (MapPoint* p : b.all_pts()) R.Touch(p);
    if (R.Flush() < 0) { std::printf("FAIL %s: Flush\n", name); return 1; }
    std::vector<float> before;
    for (int p = 0; p < b.np; ++p) for (int k = 0; k < 3; ++k) before.push_back(b.pts[p].mWorldPos.at<float>(k));
    UpdateMapAfterGlobalBA(R, &b.map, b.nLoopKF);
    int diff = compare(a, b, name);
    int given = 0, moved = 0, still = 0;
    for (int p = 0; p < b.np; ++p) {
        MapPoint& mp = b.pts[p];
        bool same = true;
        for (int k = 0; k < 3; ++k) same = same && std::memcmp(&before[3 * (size_t)p + k], &mp.mWorldPos.at<float>(k), 4) == 0;
        if (same) ++still; else if (mp.mnBAGlobalForKF == b.nLoopKF) ++given; else ++moved;
    }
    const int audit = R.Audit(b.all_kfs(), b.all_pts());
    const int sent = R.Flush();
    const ResidentMap::FlushStats fs = R.LastFlush();
    if (audit != 0 || sent != 0 || fs.rows != 0) { std::printf("FAIL %s: Audit %d, Flush %d (rows %d)\n", name, audit, sent, fs.rows); ++diff; }
    int cor[4]; R.LastCorrection(cor);
    std::printf("gba %s: %d points: %d took mPosGBA, %d moved through their reference, %d stayed; audit %d, rows flushed %d, device %d, %d differ\n", name, b.np,
                given, moved, still, audit, fs.rows, cor[0], diff);
    if (given == 0 || moved == 0 || still == 0) { std::printf("FAIL %s: a class of point is missing\n", name); ++diff; }
    if (device && cor[0] != 1) { std::printf("FAIL %s: the call did not run on the device\n", name); ++diff; }
    return diff;
}

// small: every keyframe claims fewer points than REFRESH_HOST_BELOW (no device needed).  large: device batches.
void small_scaled(World& w) { build(w, 1, 9, 30, 24, 3, 5, false); }
void small_fixed(World& w) { build(w, 2, 8, 26, 20, 3, 4, true); }
void large_scaled(World& w) { build(w, 3, 30, 4000, 400, 5, 12, false); }
void large_fixed(World& w) { build(w, 4, 40, 9000, 600, 6, 20, true); }
// hand-built: three connected keyframes 1, 2, 3 (current: 2) and point 0 claimed by keyframe 2 while keyframes 1 and 3 see it too
void hand_straddle(World& w) {
    build(w, 5, 4, 6, 8, 1, 3, false);
    for (int k = 0; k < 4; ++k) for (auto& p : w.kfs[k].mvpMapPoints) p = nullptr;
    for (int p = 0; p < 6; ++p) { w.pts[p].mObservations.clear(); w.pts[p].nObs = 0; w.pts[p].mpRefKF = nullptr; w.pts[p].mbBad = false; }
    observe(w, 0, 2, 0); observe(w, 0, 1, 1); observe(w, 0, 3, 1);     // reference keyframe 2; keyframe 1 lists it at feature 1 ...
    w.kfs[1].mvpMapPoints[1] = nullptr;                                // ... but no longer holds it: keyframe 2 claims it
    observe(w, 1, 1, 0); observe(w, 2, 3, 0); observe(w, 3, 0, 0); observe(w, 4, 2, 3); observe(w, 5, 3, 4);
    w.pts[4].mbBad = true;
}

int run_cases(ORBmatcher* device) {
    int f = 0;
    f += loop_case(device, "hand straddle", hand_straddle);
    f += loop_case(device, "small scaled", small_scaled);
    f += loop_case(device, "small fixed scale", small_fixed);
    f += gba_case(device, "small scaled", small_scaled);
    f += gba_case(device, "small fixed scale", small_fixed);
    if (device) {
        f += loop_case(device, "large scaled", large_scaled);
        f += loop_case(device, "large fixed scale", large_fixed);
        f += gba_case(device, "large scaled", large_scaled);
        f += gba_case(device, "large fixed scale", large_fixed);
    }
    return f;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "host") {
        const int f = run_cases(nullptr);
        if (f == 0) std::printf("loop correction host ok\n");
        return f ? 1 : 0;
    }
    if (mode == "device") {
        ORBmatcher matcher(0.8f, true);
        const int f = run_cases(&matcher);
        if (f == 0) std::printf("loop correction device ok\n");
        return f ? 1 : 0;
    }
    std::fprintf(stderr, "usage: test_loop_correction host | device\n");
    return 2;
}
