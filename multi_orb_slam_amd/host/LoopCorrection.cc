// LoopCorrection.cc -- see LoopCorrection.h.
#include "LoopCorrection.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <list>
#include <mutex>
#include <set>
#include "../../include/orbm.h"
#include "slam_types.h"
#ifdef MORB_USE_REFERENCE_TYPES
#include "Map.h"
#endif
#include "MapPointRefresh.h"

namespace ORB_SLAM2 {

// UNMEASURED: see LoopCorrection.h
const int CORRECT_HOST_BELOW = 0;

namespace {
void report(const char* who, const char* what, int rc) { std::fprintf(stderr, "%s: %s failed (%d): %s\n", who, what, rc, orb_last_error()); }

// Converter::toMatrix3d / toVector3d of a float pose, g2o::Sim3(R, t, 1.0)
g2o::Sim3 sim3_of(const cv::Mat& T) {
    g2o::Matrix3d R;
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R(r, c) = (double)T.at<float>(r, c);
    const g2o::Vector3d t((double)T.at<float>(0, 3), (double)T.at<float>(1, 3), (double)T.at<float>(2, 3));
    return g2o::Sim3(R, t, 1.0);
}
void push8(std::vector<double>& v, const g2o::Sim3& S) {
    const g2o::Quaterniond& q = S.rotation();
    v.push_back(q.x()); v.push_back(q.y()); v.push_back(q.z()); v.push_back(q.w());
    for (int k = 0; k < 3; ++k) v.push_back(S.translation()[k]);
    v.push_back(S.scale());
}
cv::Mat point_of(const float* p) {
    cv::Mat P(3, 1, CV_32F);
    for (int k = 0; k < 3; ++k) P.at<float>(k) = p[k];
    return P;
}
}  // namespace

int ResidentMap::CorrectSim3(const std::vector<int32_t>& kfs, const std::vector<double>& before, const std::vector<double>& after,
                             const std::vector<int32_t>& already, std::vector<orbm_correct_entry>& entries, std::vector<float>& pos,
                             std::vector<float>& Tiw) {
    std::lock_guard<std::recursive_mutex> lock_map(mMutexMap);
    const int n = (int)kfs.size();
    Tiw.assign((size_t)std::max(n, 1) * 16, 0.f);
    int cap = 0;
    for (int k : kfs) cap += mvKeyFrameCount[(size_t)k];       // every candidate kept: the list cannot be longer
    entries.resize((size_t)std::max(cap, 1)); pos.resize((size_t)std::max(cap, 1) * 3);
    int kept = 0, rc;
    if (mpMap) {
        rc = orbm_map_correct_sim3(mpHandle, mpMap, kfs.data(), n, before.data(), after.data(), already.data(), (int)already.size(),
                                   entries.data(), pos.data(), cap, &kept, Tiw.data());
        if (rc) { report("CorrectLoopMap", "orbm_map_correct_sim3", rc); return rc; }
        for (int i = 0; i < kept; ++i) std::memcpy(mvRows[(size_t)entries[(size_t)i].point].pos, &pos[3 * (size_t)i], 12);
    } else {
        rc = orbm_local_map_correct_sim3_host(mvKeyFrameRows.data(), mvKeyFrameCount.data(), (int)mvKeyFrameOfSlot.size(), mCap.features_per_keyframe,
                                              mvFlags.data(), mvRows.empty() ? nullptr : mvRows[0].pos, (int)(sizeof(orbm_point) / sizeof(float)),
                                              (int)mvRows.size(), kfs.data(), n, before.data(), after.data(), already.data(), (int)already.size(),
                                              entries.data(), pos.data(), cap, &kept, Tiw.data());
        if (rc) { report("CorrectLoopMap", "orbm_local_map_correct_sim3_host", rc); return rc; }
    }
    entries.resize((size_t)kept); pos.resize((size_t)kept * 3);
    return 0;
}

int ResidentMap::CorrectRigid(const std::vector<int32_t>& slots, const std::vector<uint8_t>& kf_corrected, const std::vector<float>& Tcw_before,
                              const std::vector<float>& Twc_after, const std::vector<int32_t>& gba_slots, const std::vector<float>& gba_pos,
                              std::vector<uint8_t>& status, std::vector<float>& pos) {
    std::lock_guard<std::recursive_mutex> lock_map(mMutexMap);
    const int n = (int)slots.size(), n_kfs = (int)kf_corrected.size(), n_gba = (int)gba_slots.size();
    status.assign((size_t)std::max(n, 1), 0); pos.assign((size_t)std::max(n, 1) * 3, 0.f);
    int rc;
    if (mpMap) {
        rc = orbm_map_correct_rigid(mpHandle, mpMap, slots.data(), n, kf_corrected.data(), Tcw_before.data(), Twc_after.data(), n_kfs,
                                    gba_slots.data(), gba_pos.data(), n_gba, status.data(), pos.data());
        if (rc) { report("UpdateMapAfterGlobalBA", "orbm_map_correct_rigid", rc); return rc; }
        for (int i = 0; i < n; ++i)
            if (status[(size_t)i]) std::memcpy(mvRows[(size_t)slots[(size_t)i]].pos, &pos[3 * (size_t)i], 12);
    } else {
        rc = orbm_local_map_correct_rigid_host(mvRows.empty() ? nullptr : mvRows[0].pos, (int)(sizeof(orbm_point) / sizeof(float)), mvFlags.data(),
                                               mvPointRef.data(), (int)mvRows.size(), slots.data(), n, kf_corrected.data(), Tcw_before.data(),
                                               Twc_after.data(), n_kfs, gba_slots.data(), gba_pos.data(), n_gba, status.data(), pos.data());
        if (rc) { report("UpdateMapAfterGlobalBA", "orbm_local_map_correct_rigid_host", rc); return rc; }
    }
    return 0;
}

struct LoopCorrectionAccess {
    static void CorrectLoop(ResidentMap& R, ORBmatcher& matcher, KeyFrame* mpCurrentKF, const std::vector<KeyFrame*>& mvpCurrentConnectedKFs,
                            const g2o::Sim3& mg2oScw, LoopClosing::KeyFrameAndPose& CorrectedSim3, LoopClosing::KeyFrameAndPose& NonCorrectedSim3);
    static void AfterGlobalBA(ResidentMap& R, Map* mpMap, unsigned long nLoopKF);
};

void LoopCorrectionAccess::CorrectLoop(ResidentMap& R, ORBmatcher& matcher, KeyFrame* mpCurrentKF,
                                       const std::vector<KeyFrame*>& mvpCurrentConnectedKFs, const g2o::Sim3& mg2oScw,
                                       LoopClosing::KeyFrameAndPose& CorrectedSim3, LoopClosing::KeyFrameAndPose& NonCorrectedSim3) {
    std::lock_guard<std::recursive_mutex> lock_map(R.mMutexMap);
    cv::Mat Twc = mpCurrentKF->GetPoseInverse();

    // step 4.1 (:645-673), as written
    for (std::vector<KeyFrame*>::const_iterator vit = mvpCurrentConnectedKFs.begin(), vend = mvpCurrentConnectedKFs.end(); vit != vend; vit++) {
        KeyFrame* pKFi = *vit;
        cv::Mat Tiw = pKFi->GetPose();
        if (pKFi != mpCurrentKF) {
            cv::Mat Tic = Tiw * Twc;
            g2o::Sim3 g2oSic = sim3_of(Tic);
            g2o::Sim3 g2oCorrectedSiw = g2oSic * mg2oScw;
            CorrectedSim3[pKFi] = g2oCorrectedSiw;
        }
        NonCorrectedSim3[pKFi] = sim3_of(Tiw);
    }

    // steps 4.2 and 4.3 (:678-727): one call for the claim and the arithmetic, in CorrectedSim3's iteration order
    std::vector<KeyFrame*> vpKFs;
    std::vector<double> before, after;
    for (LoopClosing::KeyFrameAndPose::iterator mit = CorrectedSim3.begin(), mend = CorrectedSim3.end(); mit != mend; mit++) {
        vpKFs.push_back(mit->first);
        push8(after, mit->second);
        push8(before, NonCorrectedSim3[mit->first]);
    }
    if (vpKFs.size() > (size_t)ORBM_MAP_MAX_LOCAL) {
        std::fprintf(stderr, "CorrectLoopMap: %d keyframes are more than a call takes (%d)\n", (int)vpKFs.size(), (int)ORBM_MAP_MAX_LOCAL);
        return;
    }
    if (R.Flush() < 0) return;
    std::vector<int32_t> slots, already;
    if (!R.SlotsOfSent(vpKFs, 0, vpKFs.size(), slots)) return;
    for (KeyFrame* pKFi : vpKFs) {                              // the marks an earlier correction left (:696)
        const std::vector<MapPoint*> vpMPsi = pKFi->GetMapPointMatches();
        for (MapPoint* pMPi : vpMPsi)
            if (pMPi && pMPi->mnCorrectedByKF == mpCurrentKF->mnId) { auto it = R.mPoints.find(pMPi); if (it != R.mPoints.end()) already.push_back(it->second.slot); }
    }
    std::vector<orbm_correct_entry> entries; std::vector<float> pos, Tiw;
    if (R.CorrectSim3(slots, before, after, already, entries, pos, Tiw)) return;

    size_t at = 0;
    std::vector<MapPoint*> claimed;
    for (size_t j = 0; j < vpKFs.size(); ++j) {
        KeyFrame* pKFi = vpKFs[j];
        claimed.clear();
        for (; at < entries.size() && entries[at].position == (int32_t)j; ++at) {
            MapPoint* pMPi = R.mvPointOfSlot[(size_t)entries[at].point];
            pMPi->SetWorldPos(point_of(&pos[3 * at]));
            pMPi->mnCorrectedByKF = mpCurrentKF->mnId;
            pMPi->mnCorrectedReference = pKFi->mnId;
            claimed.push_back(pMPi);
        }
        RefreshMapPoints(matcher, claimed, REFRESH_NORMAL_DEPTH);   // UpdateNormalAndDepth of this keyframe's points, the poses as they are NOW
        for (MapPoint* pMPi : claimed) R.Touch(pMPi);

        cv::Mat correctedTiw(4, 4, CV_32F);
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) correctedTiw.at<float>(r, c) = Tiw[16 * j + 4 * (size_t)r + (size_t)c];
        pKFi->SetPose(correctedTiw);
        pKFi->UpdateConnections();
    }
}

void LoopCorrectionAccess::AfterGlobalBA(ResidentMap& R, Map* mpMap, unsigned long nLoopKF) {
    std::lock_guard<std::recursive_mutex> lock_map(R.mMutexMap);
    // Correct keyframes starting at map first keyframe (:927-951), as written
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

    // Correct MapPoints (:955-989): one call
    const std::vector<MapPoint*> vpMPs = mpMap->GetAllMapPoints();
    for (MapPoint* pMP : vpMPs)
        if (pMP && !R.mPoints.count(pMP)) R.Touch(pMP);         // a point the map was never told of is read now (Audit counts such points)
    if (R.Flush() < 0) return;
    const size_t n_kfs = R.mvKeyFrameOfSlot.size();
    std::vector<uint8_t> kf_corrected(n_kfs, 0);
    std::vector<float> Tcw_before(n_kfs * 12, 0.f), Twc_after(n_kfs * 12, 0.f);
    for (size_t r = 0; r < n_kfs; ++r) {
        KeyFrame* pRefKF = R.mvKeyFrameOfSlot[r];
        if (pRefKF->mnBAGlobalForKF != nLoopKF || pRefKF->mTcwBefGBA.empty()) continue;
        kf_corrected[r] = 1;
        const cv::Mat Twc = pRefKF->GetPoseInverse();
        for (int i = 0; i < 3; ++i)
            for (int c = 0; c < 4; ++c) { Tcw_before[12 * r + 4 * (size_t)i + (size_t)c] = pRefKF->mTcwBefGBA.at<float>(i, c); Twc_after[12 * r + 4 * (size_t)i + (size_t)c] = Twc.at<float>(i, c); }
    }
    std::vector<int32_t> slots, gba_slots; std::vector<float> gba_pos; std::vector<MapPoint*> listed;
    for (MapPoint* pMP : vpMPs) {
        if (!pMP) continue;
        const int slot = R.mPoints[pMP].slot;
        slots.push_back(slot); listed.push_back(pMP);
        if (pMP->mnBAGlobalForKF == nLoopKF) { gba_slots.push_back(slot); for (int k = 0; k < 3; ++k) gba_pos.push_back(pMP->mPosGBA.at<float>(k)); }
    }
    std::vector<uint8_t> status; std::vector<float> pos;
    if (R.CorrectRigid(slots, kf_corrected, Tcw_before, Twc_after, gba_slots, gba_pos, status, pos)) return;
    for (size_t i = 0; i < listed.size(); ++i)
        if (status[i]) listed[i]->SetWorldPos(point_of(&pos[3 * i]));
}

void CorrectLoopMap(ResidentMap& map, ORBmatcher& matcher, KeyFrame* pCurrentKF, const std::vector<KeyFrame*>& vpConnected,
                    const g2o::Sim3& g2oScw, LoopClosing::KeyFrameAndPose& CorrectedSim3, LoopClosing::KeyFrameAndPose& NonCorrectedSim3) {
    LoopCorrectionAccess::CorrectLoop(map, matcher, pCurrentKF, vpConnected, g2oScw, CorrectedSim3, NonCorrectedSim3);
}

void UpdateMapAfterGlobalBA(ResidentMap& map, Map* pMap, unsigned long nLoopKF) { LoopCorrectionAccess::AfterGlobalBA(map, pMap, nLoopKF); }

}  // namespace ORB_SLAM2
