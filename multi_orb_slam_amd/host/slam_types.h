// slam_types.h -- minimal stand-ins for the reference's Frame (include/Frame.h:155-261), KeyFrame (include/KeyFrame.h:218-248)
// and MapPoint (include/MapPoint.h) carrying the members ORBmatcher's searches read or write, under the reference's names
// and with the reference's container types for everything the wrapper iterates or indexes (std::unordered_map<size_t,int>
// for the two index maps, std::vector<cv::Mat> for the per-camera descriptors, DBoW2's map-derived vectors).  What is NOT the
// reference's: the image bounds and the ids are per-object here and static members there (same spelling at the point of use),
// nNextId is an atomic accessor, MapPoint keeps its observations in a std::map<KeyFrame*,size_t> without the mutexes.
// A real integration compiles the wrapper against the reference's own headers instead: define MORB_USE_REFERENCE_TYPES and put
// the reference's include/ (and its root, for Thirdparty/DBoW2) on the include path; tests/test_reference_headers.py holds
// that build (-fsyntax-only, reference headers used in place) to zero errors on every CPU run.
#pragma once
#ifndef MORB_USE_REFERENCE_TYPES
#include <algorithm>
#include <atomic>
#include <cmath>
#include <map>
#include <mutex>
#include <set>
#include <unordered_map>
#include <vector>
#include "cv_compat.h"
#include "ORBVocabulary.h"

#define FRAME_GRID_ROWS 48
#define FRAME_GRID_COLS 64

namespace ORB_SLAM2 {

class KeyFrame;
class Frame;

// A record of the calls host/LocalBA.cc makes on the map, for its driver (host/test_local_ba.cc): off unless the driver hands in a
// vector.  One entry per call: what was called and the mnIds it was called on.
struct CallLogEntry { const char* what; long unsigned int a, b; };
inline std::vector<CallLogEntry>*& CallLog() { static std::vector<CallLogEntry>* log = nullptr; return log; }
inline void LogCall(const char* what, long unsigned int a = 0, long unsigned int b = 0) { if (CallLog()) CallLog()->push_back({what, a, b}); }

class MapPoint {
public:
    cv::Mat GetWorldPos() { return mWorldPos; }
    cv::Mat GetDescriptor() { return mDescriptor; }
    int Observations() { return nObs; }
    bool isBad() { return mbBad; }
    // tracking scratch written by Frame::isInFrustum (src/Frame.cc:443-499)
    float mTrackProjX = 0, mTrackProjY = 0, mTrackProjXR = 0;
    bool mbTrackInView = false;
    int mnTrackScaleLevel = 0;
    float mTrackViewCos = 1.f;
    // bookkeeping of Tracking::SearchLocalPoints (src/Tracking.cc:1702-1770; include/MapPoint.h, src/MapPoint.cc:IncreaseVisible)
    long unsigned int mnLastFrameSeen = 0;
    // the mark of Tracking::UpdateLocalPoints (src/Tracking.cc:1812-1817; include/MapPoint.h:106), read and written by host/LocalMap.cc
    long unsigned int mnTrackReferenceForFrame = 0;
    void IncreaseVisible(int n = 1) { mnVisible += n; }
    int mnVisible = 1;

    // members the remaining projection searches read (src/MapPoint.cc:559-617)
    cv::Mat GetNormal() { return mNormalVector; }
    float GetMinDistanceInvariance() { return 0.8f * mfMinDistance; }
    float GetMaxDistanceInvariance() { return 1.2f * mfMaxDistance; }
    template <class FrameOrKeyFrame> int PredictScale(const float& currentDist, FrameOrKeyFrame* pF) {
        const float ratio = mfMaxDistance / currentDist;
        int nScale = (int)std::ceil(std::log(ratio) / pF->mfLogScaleFactor);
        if (nScale < 0) nScale = 0;
        else if (nScale >= pF->mnScaleLevels) nScale = pF->mnScaleLevels - 1;
        return nScale;
    }
    bool IsInKeyFrame(KeyFrame* pKF) { return mObservations.count(pKF) != 0; }
    int GetIndexInKeyFrame(KeyFrame* pKF) { auto it = mObservations.find(pKF); return it != mObservations.end() ? (int)it->second : -1; }
    int GetIndexInKeyFrame_cam1(KeyFrame* pKF) { auto it = mObservations.find(pKF); return it != mObservations.end() ? (int)it->second : -1; }
    void AddObservation(KeyFrame* pKF, size_t idx) { if (mObservations.count(pKF)) return; mObservations[pKF] = idx; nObs++; }
    void Replace(MapPoint* pMP) { if (pMP == this) return; mpReplaced = pMP; mbBad = true; }
    // members host/MapPointRefresh.cc reads (include/MapPoint.h:50-52) and the two writers an integration adds for it
    std::map<KeyFrame*, size_t> GetObservations() { return mObservations; }
    KeyFrame* GetReferenceKeyFrame() { return mpRefKF; }
    void SetDistinctiveDescriptor(const cv::Mat& d) { mDescriptor = d.clone(); }
    void SetNormalAndDepth(const cv::Mat& normal, float minDistance, float maxDistance) {
        LogCall("SetNormalAndDepth", mnId);
        mNormalVector = normal.clone(); mfMinDistance = minDistance; mfMaxDistance = maxDistance;
    }
    KeyFrame* mpRefKF = nullptr;
    // members host/LocalBA.cc reads or writes (include/MapPoint.h:  mnId, mnBALocalForKF, SetWorldPos, EraseObservation; the stand-in's
    // EraseObservation drops the observation and moves the reference keyframe on, without SetBadFlag)
    long unsigned int mnId = 0, mnBALocalForKF = 0;
    void SetWorldPos(const cv::Mat& Pos) { LogCall("SetWorldPos", mnId); mWorldPos = Pos.clone(); }
    void EraseObservation(KeyFrame* pKF);   // (defined behind KeyFrame: it logs the keyframe's mnId)
    void EraseObservationImpl(KeyFrame* pKF) {
        if (!mObservations.count(pKF)) return;
        mObservations.erase(pKF); nObs--;
        if (mpRefKF == pKF) mpRefKF = mObservations.empty() ? nullptr : mObservations.begin()->first;
    }

    // members host/Covisibility.cc and its driver read (include/MapPoint.h; src/MapPoint.cc:138-209): the camera-1 observations -- here
    // computed from mObservations by the rule AddObservation files them under (idx < pKF->N) --, and the reference's EraseObservation
    // as KeyFrame::SetBadFlag needs it: the counter drops by 2 for a stereo feature, and a point left with two observations or fewer
    // goes bad and lets go of every keyframe that holds it (MapPoint::SetBadFlag).  Both are defined behind KeyFrame.
    std::map<KeyFrame*, size_t> GetObservations_cam1();
    void EraseObservationOfBadKeyFrame(KeyFrame* pKF);

    // members host/GlobalBA.cc writes when the adjustment belongs to a loop (include/MapPoint.h: mPosGBA, mnBAGlobalForKF)
    cv::Mat mPosGBA;
    long unsigned int mnBAGlobalForKF = 0;
    // members host/EssentialGraph.cc reads (include/MapPoint.h:115-116: written by LoopClosing::CorrectLoop)
    long unsigned int mnCorrectedByKF = 0, mnCorrectedReference = 0;

    cv::Mat mWorldPos;    // 3x1 CV_32F
    cv::Mat mDescriptor;  // 1x32 CV_8U
    cv::Mat mNormalVector;  // 3x1 CV_32F
    float mfMinDistance = 0, mfMaxDistance = 0;
    std::map<KeyFrame*, size_t> mObservations;
    MapPoint* mpReplaced = nullptr;
    int nObs = 1;
    bool mbBad = false;
};

class Frame {
public:
    // identity (include/Frame.h: `static long unsigned int nNextId; long unsigned int mnId;`, assigned in the constructors,
    // src/Frame.cc:257; copies keep it)
    // (atomic here: the stand-in's test driver constructs frames on several threads; the reference's tracking thread is alone)
    static std::atomic<long unsigned int>& NextId() { static std::atomic<long unsigned int> n{0}; return n; }
    long unsigned int mnId = NextId()++;
    // multi-camera "_total" view (src/Frame.cc:191-239): global index g, cam-major
    int N = 0, N_cam2 = 0, N_total = 0;
    std::vector<cv::KeyPoint> mvKeys_total, mvKeysUn_total, mvKeysUn;
    std::vector<float> mvuRight_total, mvuRight, mvDepth_total;
    std::vector<cv::Mat> mDescriptors_total;  // per camera, N_c x 32
    cv::Mat mDescriptors;                     // camera 1
    std::unordered_map<size_t, int> keypoint_to_cam, cont_idx_to_local_cam_idx;   // include/Frame.h:256,261 / include/KeyFrame.h:243,248
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<bool> mvbOutlier;
    std::vector<float> mvScaleFactors;
    cv::Mat mTcw;  // 4x4 CV_32F
    float fx = 0, fy = 0, cx = 0, cy = 0, mb = 0, mbf = 0;
    float mnMinX = 0, mnMaxX = 0, mnMinY = 0, mnMaxY = 0;  // static members in the reference
    DBoW2::BowVector mBowVec;       // all cameras (include/Frame.h:185-187)
    DBoW2::FeatureVector mFeatVec;
    DBoW2::BowVector mBowVec_cam1;  // camera 1 only (include/Frame.h:186,188)
    DBoW2::FeatureVector mFeatVec_cam1;
    std::vector<cv::KeyPoint> mvKeys;   // camera 1, distorted
    float mfLogScaleFactor = 0; int mnScaleLevels = 0;
    // members host/Optimizer.cc reads (include/Frame.h:226-227, :243)
    std::vector<float> mvInvLevelSigma2, mvLevelSigma2;   // (mvLevelSigma2: include/Frame.h:242, read by host/PnPsolver.cc)
    cv::Mat mRcam12, mtcam12;                 // 3x3, 3x1 CV_32F
    KeyFrame* mpReferenceKF = nullptr;        // include/Frame.h:234, written by Tracking::UpdateLocalKeyFrames (src/Tracking.cc:1947)

    // pose members (include/Frame.h:82-99, src/Frame.cc:420-499)
    void SetPose(cv::Mat Tcw) { mTcw = Tcw.clone(); UpdatePoseMatrices(); }
    void UpdatePoseMatrices() {
        mRcw = mTcw.rowRange(0, 3).colRange(0, 3);
        mRwc = mRcw.t();
        mtcw = mTcw.rowRange(0, 3).col(3);
        mOw = -mRcw.t() * mtcw;
    }
    cv::Mat GetCameraCenter() { return mOw.clone(); }
    // Frame::isInFrustum (src/Frame.cc:443-499), camera 1: the same tests in the same order on the same cv::Mat expressions --
    // cv_compat.h evaluates them as OpenCV does (R*P + t is ONE small-path gemm; norm and dot accumulate in double) -- and the same
    // six scratch fields written on success.  This is the checker of the device form (csrc/frustum.hip).
    // One deviation: a projection that is not finite (depth exactly 0) is out of view.
    bool isInFrustum(MapPoint* pMP, float viewingCosLimit) {
        pMP->mbTrackInView = false;
        const cv::Mat world = pMP->GetWorldPos();
        const cv::Mat cam = mRcw * world + mtcw;
        const float depth = cam.at<float>(2);
        if (depth < 0.0f) return false;
        const float inv_depth = 1.0f / depth;
        const float u = fx * cam.at<float>(0) * inv_depth + cx, v = fy * cam.at<float>(1) * inv_depth + cy;
        if (!std::isfinite(u) || !std::isfinite(v)) return false;
        if (u < mnMinX || u > mnMaxX || v < mnMinY || v > mnMaxY) return false;
        const cv::Mat ray = world - mOw;
        const float range = cv::norm(ray);
        if (range < pMP->GetMinDistanceInvariance() || range > pMP->GetMaxDistanceInvariance()) return false;
        const float cosine = ray.dot(pMP->GetNormal()) / range;   // (double / float, rounded once)
        if (cosine < viewingCosLimit) return false;
        pMP->mnTrackScaleLevel = pMP->PredictScale(range, this);
        pMP->mTrackProjX = u; pMP->mTrackProjY = v; pMP->mTrackProjXR = u - mbf * inv_depth;
        pMP->mTrackViewCos = cosine;
        pMP->mbTrackInView = true;
        return true;
    }

private:
    cv::Mat mRcw, mtcw, mRwc, mOw;   // private in the reference too (include/Frame.h:263-282): read them through mTcw / GetCameraCenter()
};

// KeyFrame members the BoW-gated searches read (include/KeyFrame.h:53-59, :104-113, :218-219 and the Frame copies of
// src/KeyFrame.cc:31-80).  Poses are world -> camera, one per camera of the rig.
class KeyFrame {
public:
    // identity (include/KeyFrame.h: `static long unsigned int nNextId; long unsigned int mnId;`)
    static std::atomic<long unsigned int>& NextId() { static std::atomic<long unsigned int> n{0}; return n; }
    long unsigned int mnId = NextId()++;
    std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
    MapPoint* GetMapPoint(const size_t& idx) { return mvpMapPoints[idx]; }
    cv::Mat GetDescriptor(const int& cam, const size_t& idx) const { return mDescriptors_total[cam].row((int)idx); }
    cv::Mat GetRotation() { return Tcw.rowRange(0, 3).colRange(0, 3).clone(); }
    cv::Mat GetTranslation() { return Tcw.rowRange(0, 3).col(3).clone(); }
    cv::Mat GetRotation_cam2() { return Tcw_cam2.rowRange(0, 3).colRange(0, 3).clone(); }
    cv::Mat GetTranslation_cam2() { return Tcw_cam2.rowRange(0, 3).col(3).clone(); }
    cv::Mat GetCameraCenter() { return -(GetRotation().t() * GetTranslation()); }
    cv::Mat GetCameraCenter_cam2() { return -(GetRotation_cam2().t() * GetTranslation_cam2()); }
    bool isBad() { return mbBad; }
    bool mbBad = false;

    std::vector<cv::KeyPoint> mvKeysUn_total;
    std::vector<float> mvuRight_total;
    std::vector<cv::Mat> mDescriptors_total;
    std::unordered_map<size_t, int> keypoint_to_cam, cont_idx_to_local_cam_idx;   // include/Frame.h:256,261 / include/KeyFrame.h:243,248
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<float> mvScaleFactors, mvLevelSigma2;
    DBoW2::BowVector mBowVec, mBowVec_cam1;
    DBoW2::FeatureVector mFeatVec, mFeatVec_cam1;
    cv::Mat mK;                      // 3x3 CV_32F
    float fx = 0, fy = 0, cx = 0, cy = 0;
    cv::Mat Tcw, Tcw_cam2;           // 4x4 CV_32F

    // members host/NewMapPoints.cc reads (include/KeyFrame.h:52, :186-211, :226; src/KeyFrame.cc SetPose for Twc = [Rwc | Ow])
    cv::Mat GetPoseInverse() {
        cv::Mat Twc = cv::Mat::eye(4, 4, CV_32F);
        const cv::Mat Rwc = GetRotation().t(), Ow = GetCameraCenter();
        for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) Twc.at<float>(r, c) = Rwc.at<float>(r, c); Twc.at<float>(r, 3) = Ow.at<float>(r); }
        return Twc;
    }
    float invfx = 0, invfy = 0, mb = 0, mfScaleFactor = 0;
    cv::Mat mRcam12, mtcam12;                        // 3x3, 3x1 CV_32F
    std::vector<cv::KeyPoint> mvKeys_total;          // distorted (what UnprojectStereo reads)
    std::vector<float> mvDepth_total;

    // members the remaining projection searches read
    std::vector<MapPoint*> GetMapPointMatches_cam1() { return std::vector<MapPoint*>(mvpMapPoints.begin(), mvpMapPoints.begin() + N); }
    void AddMapPoint(MapPoint* pMP, const size_t& idx) { mvpMapPoints[idx] = pMP; }
    std::set<MapPoint*> GetMapPoints() { std::set<MapPoint*> s; for (MapPoint* p : mvpMapPoints) if (p && !p->isBad()) s.insert(p); return s; }
    bool IsInImage(const float& x, const float& y) const { return (x >= mnMinX && x < mnMaxX && y >= mnMinY && y < mnMaxY); }
    int N = 0, N_cam2 = 0, N_total = 0;
    std::vector<cv::KeyPoint> mvKeysUn;   // camera 1
    std::vector<float> mvuRight;
    cv::Mat mDescriptors;                 // camera 1
    std::vector<float> mvInvLevelSigma2;
    float mbf = 0, mfLogScaleFactor = 0; int mnScaleLevels = 0;
    float mnMinX = 0, mnMaxX = 0, mnMinY = 0, mnMaxY = 0;

    // members KeyFrameDatabase reads or writes (include/KeyFrame.h:73-79, :172-178).  The reference's constructor initialises the two ids
    // and the two counts to 0 (src/KeyFrame.cc:35) and leaves the two scores uninitialised: 0 here.
    long unsigned int mnLoopQuery = 0;
    int mnLoopWords = 0;
    float mLoopScore = 0;
    long unsigned int mnRelocQuery = 0;
    int mnRelocWords = 0;
    float mRelocScore = 0;
    std::set<KeyFrame*> GetConnectedKeyFrames() { return mConnectedKeyFrames; }
    std::set<KeyFrame*> GetConnectedKeyFrames_cam1() { return mConnectedKeyFrames_cam1; }
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N) { return FirstN(mvpOrderedConnectedKeyFrames, N); }
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames_cam1(const int& N) { return FirstN(mvpOrderedConnectedKeyFrames_cam1, N); }
    // the covisibility graph itself is not modelled: plain containers the caller fills (ordered: best covisibility first)
    std::set<KeyFrame*> mConnectedKeyFrames, mConnectedKeyFrames_cam1;
    std::vector<KeyFrame*> mvpOrderedConnectedKeyFrames, mvpOrderedConnectedKeyFrames_cam1;
    // members host/LocalBA.cc reads or writes (include/KeyFrame.h: GetVectorCovisibleKeyFrames, GetPose, SetPose, EraseMapPointMatch,
    // mnBALocalForKF, mnBAFixedForKF)
    std::vector<KeyFrame*> GetVectorCovisibleKeyFrames() { return mvpOrderedConnectedKeyFrames; }
    cv::Mat GetPose() { return Tcw.clone(); }
    void SetPose(const cv::Mat& Tcw_) { LogCall("SetPose", mnId); Tcw = Tcw_.clone(); }
    void EraseMapPointMatch(MapPoint* pMP) { LogCall("EraseMapPointMatch", mnId, pMP->mnId); const int idx = pMP->GetIndexInKeyFrame(this); if (idx >= 0) mvpMapPoints[idx] = nullptr; }
    long unsigned int mnBALocalForKF = 0, mnBAFixedForKF = 0;
    // members host/GlobalBA.cc writes when the adjustment belongs to a loop (include/KeyFrame.h: mTcwGBA, mnBAGlobalForKF)
    cv::Mat mTcwGBA;
    long unsigned int mnBAGlobalForKF = 0;
    // member host/LoopCorrection.cc writes and reads (include/KeyFrame.h: mTcwBefGBA, set by LoopClosing::RunGlobalBundleAdjustment)
    cv::Mat mTcwBefGBA;
    // KeyFrame::UpdateConnections (src/KeyFrame.cc:486-668), which LoopClosing::CorrectLoop calls per keyframe: defined behind MapPoint's
    // late members.  Two statements of the reference cannot run on a keyframe without a camera-1 counter (pKFmax_cam1 is NULL at :618,
    // front() of an empty vector at :660): they are skipped there.
    void UpdateConnections();
    // members host/EssentialGraph.cc reads (include/KeyFrame.h:82-96; src/KeyFrame.cc:331-364): the spanning tree, the loop edges and
    // the camera-1 covisibility weights are plain containers the caller fills (mvOrderedWeights_cam1 descending, beside
    // mvpOrderedConnectedKeyFrames_cam1)
    KeyFrame* GetParent() { return mpParent; }
    std::set<KeyFrame*> GetChilds() { return mspChildrens; }
    // the mark of Tracking::UpdateLocalKeyFrames (src/Tracking.cc:1885-1937; include/KeyFrame.h:164), read and written by host/LocalMap.cc
    long unsigned int mnTrackReferenceForFrame = 0;
    bool hasChild(KeyFrame* pKF) { return mspChildrens.count(pKF) != 0; }
    std::set<KeyFrame*> GetLoopEdges() { return mspLoopEdges; }
    int GetWeight_cam1(KeyFrame* pKF) { auto it = mConnectedKeyFrameWeights_cam1.find(pKF); return it != mConnectedKeyFrameWeights_cam1.end() ? it->second : 0; }
    std::vector<KeyFrame*> GetCovisiblesByWeight_cam1(const int& w) {
        if (mvpOrderedConnectedKeyFrames_cam1.empty()) return std::vector<KeyFrame*>();
        size_t n = 0;                                     // upper_bound(..., w, weightComp): the first weight with w > weight
        while (n < mvOrderedWeights_cam1.size() && !(w > mvOrderedWeights_cam1[n])) ++n;
        if (n == mvOrderedWeights_cam1.size()) return std::vector<KeyFrame*>();
        return std::vector<KeyFrame*>(mvpOrderedConnectedKeyFrames_cam1.begin(), mvpOrderedConnectedKeyFrames_cam1.begin() + n);
    }
    KeyFrame* mpParent = nullptr;
    std::set<KeyFrame*> mspChildrens, mspLoopEdges;
    std::map<KeyFrame*, int> mConnectedKeyFrameWeights_cam1;
    std::vector<int> mvOrderedWeights_cam1;
    static std::vector<KeyFrame*> FirstN(const std::vector<KeyFrame*>& v, int N) {   // src/KeyFrame.cc GetBestCovisibilityKeyFrames
        return (int)v.size() < N ? v : std::vector<KeyFrame*>(v.begin(), v.begin() + N);
    }

    // members host/Covisibility.cc and its driver read or write (include/KeyFrame.h; src/KeyFrame.cc:176-263, :486-668, :670-700,
    // :760-886): the weights of the covisibility graph and what keeps them ordered, the rest of UpdateConnections' state, and
    // SetBadFlag without the re-parenting of the children (the spanning tree is not what the culling reads) and without the map and
    // the keyframe database.
    float mThDepth = 0;
    bool mbFirstConnection = true, mbNotErase = false, mbToBeErased = false;
    std::map<KeyFrame*, int> mConnectedKeyFrameWeights;
    std::vector<int> mvOrderedWeights;
    static void OrderByWeight(const std::map<KeyFrame*, int>& weights, std::vector<KeyFrame*>& kfs, std::vector<int>& ws) {
        std::vector<std::pair<int, KeyFrame*> > vPairs;   // src/KeyFrame.cc:226-241: ascending sort, then pushed to the front
        for (const auto& kv : weights) vPairs.push_back(std::make_pair(kv.second, kv.first));
        std::sort(vPairs.begin(), vPairs.end());
        kfs.clear(); ws.clear();
        for (size_t i = vPairs.size(); i-- > 0;) { kfs.push_back(vPairs[i].second); ws.push_back(vPairs[i].first); }
    }
    void UpdateBestCovisibles() { OrderByWeight(mConnectedKeyFrameWeights, mvpOrderedConnectedKeyFrames, mvOrderedWeights); }
    void UpdateBestCovisibles_cam1() { OrderByWeight(mConnectedKeyFrameWeights_cam1, mvpOrderedConnectedKeyFrames_cam1, mvOrderedWeights_cam1); }
    void AddConnection(KeyFrame* pKF, const int& weight) {
        LogCall("AddConnection", mnId, pKF->mnId);
        auto it = mConnectedKeyFrameWeights.find(pKF);
        if (it != mConnectedKeyFrameWeights.end() && it->second == weight) return;
        mConnectedKeyFrameWeights[pKF] = weight;
        UpdateBestCovisibles();
    }
    void AddConnection_cam1(KeyFrame* pKF, const int& weight) {
        LogCall("AddConnection_cam1", mnId, pKF->mnId);
        auto it = mConnectedKeyFrameWeights_cam1.find(pKF);
        if (it != mConnectedKeyFrameWeights_cam1.end() && it->second == weight) return;
        mConnectedKeyFrameWeights_cam1[pKF] = weight;
        UpdateBestCovisibles_cam1();
    }
    void EraseConnection(KeyFrame* pKF) { if (mConnectedKeyFrameWeights.erase(pKF)) UpdateBestCovisibles(); }
    void AddChild(KeyFrame* pKF) { mspChildrens.insert(pKF); }
    void EraseChild(KeyFrame* pKF) { mspChildrens.erase(pKF); }
    void SetNotErase() { mbNotErase = true; }
    void SetBadFlag() {
        LogCall("SetBadFlag", mnId);
        if (mnId == 0) return;
        if (mbNotErase) { mbToBeErased = true; return; }
        for (auto& kv : mConnectedKeyFrameWeights) kv.first->EraseConnection(this);
        for (size_t i = 0; i < mvpMapPoints.size(); i++)
            if (mvpMapPoints[i]) mvpMapPoints[i]->EraseObservationOfBadKeyFrame(this);
        mConnectedKeyFrameWeights.clear();
        mvpOrderedConnectedKeyFrames.clear();
        mvpOrderedConnectedKeyFrames_cam1.clear();
        if (mpParent) mpParent->EraseChild(this);
        mbBad = true;
    }
};

inline void MapPoint::EraseObservation(KeyFrame* pKF) { LogCall("EraseObservation", mnId, pKF->mnId); EraseObservationImpl(pKF); }

inline std::map<KeyFrame*, size_t> MapPoint::GetObservations_cam1() {
    std::map<KeyFrame*, size_t> cam1;
    for (const auto& ob : mObservations)
        if ((int)ob.second < ob.first->N) cam1.insert(ob);
    return cam1;
}

inline void MapPoint::EraseObservationOfBadKeyFrame(KeyFrame* pKF) {   // src/MapPoint.cc:167-199, then :225-247 when it goes bad
    auto it = mObservations.find(pKF);
    if (it == mObservations.end()) return;
    const size_t idx = it->second;
    nObs -= (idx < pKF->mvuRight_total.size() && pKF->mvuRight_total[idx] >= 0) ? 2 : 1;
    mObservations.erase(it);
    if (mpRefKF == pKF) mpRefKF = mObservations.empty() ? nullptr : mObservations.begin()->first;
    if (nObs > 2) return;
    mbBad = true;
    const std::map<KeyFrame*, size_t> obs = mObservations;
    mObservations.clear();
    for (const auto& ob : obs)
        if (ob.second < ob.first->mvpMapPoints.size()) ob.first->mvpMapPoints[ob.second] = nullptr;   // EraseMapPointMatch(idx)
}

inline void KeyFrame::UpdateConnections() {
    LogCall("UpdateConnections", mnId);
    std::map<KeyFrame*, int> KFcounter, KFcounter_cam1;
    for (size_t i = 0; i < mvpMapPoints.size(); ++i) {               // :512-552
        MapPoint* pMP = mvpMapPoints[i];
        if (!pMP || pMP->isBad()) continue;
        for (const auto& ob : pMP->mObservations) {
            if (ob.first->mnId == mnId) continue;
            KFcounter[ob.first]++;
            if ((int)i < N && (int)ob.second < ob.first->N) KFcounter_cam1[ob.first]++;
        }
    }
    if (KFcounter.empty()) return;                                   // :554-667
    int nmax = 0, nmax_cam1 = 0;
    KeyFrame *pKFmax = nullptr, *pKFmax_cam1 = nullptr;
    const int th = 15;
    std::vector<std::pair<int, KeyFrame*> > vPairs, vPairs_cam1;
    for (auto& kv : KFcounter) {
        if (kv.second > nmax) { nmax = kv.second; pKFmax = kv.first; }
        if (kv.second >= th) { vPairs.push_back(std::make_pair(kv.second, kv.first)); kv.first->AddConnection(this, kv.second); }
    }
    for (auto& kv : KFcounter_cam1) {
        if (kv.second > nmax_cam1) { nmax_cam1 = kv.second; pKFmax_cam1 = kv.first; }
        if (kv.second >= th) { vPairs_cam1.push_back(std::make_pair(kv.second, kv.first)); kv.first->AddConnection_cam1(this, kv.second); }
    }
    if (vPairs.empty()) { vPairs.push_back(std::make_pair(nmax, pKFmax)); pKFmax->AddConnection(this, nmax); }
    if (vPairs_cam1.empty() && pKFmax_cam1) { vPairs_cam1.push_back(std::make_pair(nmax_cam1, pKFmax_cam1)); pKFmax_cam1->AddConnection_cam1(this, nmax_cam1); }
    std::sort(vPairs.begin(), vPairs.end());
    std::sort(vPairs_cam1.begin(), vPairs_cam1.end());
    mConnectedKeyFrameWeights = KFcounter; mConnectedKeyFrameWeights_cam1 = KFcounter_cam1;
    mvpOrderedConnectedKeyFrames.clear(); mvOrderedWeights.clear(); mvpOrderedConnectedKeyFrames_cam1.clear(); mvOrderedWeights_cam1.clear();
    for (size_t i = vPairs.size(); i-- > 0;) { mvpOrderedConnectedKeyFrames.push_back(vPairs[i].second); mvOrderedWeights.push_back(vPairs[i].first); }
    for (size_t i = vPairs_cam1.size(); i-- > 0;) { mvpOrderedConnectedKeyFrames_cam1.push_back(vPairs_cam1[i].second); mvOrderedWeights_cam1.push_back(vPairs_cam1[i].first); }
    if (mbFirstConnection && mnId != 0 && !mvpOrderedConnectedKeyFrames_cam1.empty()) {
        mpParent = mvpOrderedConnectedKeyFrames_cam1.front();
        mpParent->AddChild(this);
        mbFirstConnection = false;
    }
}

// Map: what host/LocalBA.cc takes of it (include/Map.h).  The stand-in's mutex is a std::mutex that records when it is taken and given back.
struct LoggedMutex {
    void lock() { m.lock(); LogCall("lock"); }
    void unlock() { LogCall("unlock"); m.unlock(); }
    bool try_lock() { if (!m.try_lock()) return false; LogCall("lock"); return true; }
    std::mutex m;
};
class Map {
public:
    LoggedMutex mMutexMapUpdate;
    // what host/GlobalBA.cc takes of it (include/Map.h; the reference keeps sets ordered by address, the stand-in what the caller filled)
    std::vector<KeyFrame*> GetAllKeyFrames() { return mvpKeyFrames; }
    std::vector<MapPoint*> GetAllMapPoints() { return mvpMapPoints; }
    std::vector<KeyFrame*> mvpKeyFrames;
    std::vector<MapPoint*> mvpMapPoints;
    // what host/EssentialGraph.cc takes of it (include/Map.h:58)
    long unsigned int GetMaxKFid() { return mnMaxKFid; }
    long unsigned int mnMaxKFid = 0;
    // what host/LoopCorrection.cc takes of it (include/Map.h: mvpKeyFrameOrigins)
    std::vector<KeyFrame*> mvpKeyFrameOrigins;
};

}  // namespace ORB_SLAM2
#else
#include "Frame.h"
#include "KeyFrame.h"
#include "MapPoint.h"
#endif
