// LocalMap.cc -- see LocalMap.h.
#include "LocalMap.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <functional>
#include <set>
#include "../../include/orbm.h"
#include "../../include/orb_debug.h"
#include "point_row.h"

namespace ORB_SLAM2 {

namespace {
void report(const char* who, const char* what, int rc) {
    std::fprintf(stderr, "%s: %s failed (%d): %s\n", who, what, rc, orb_last_error());
}

// out[f], f < stride: the level of feature f in the low five bits, ORBM_FEATURE_FAR where the reference's statement
// `mvDepth_total[f] > mThDepth || mvDepth_total[f] < 0` holds; zero from the n-th feature on and where the keyframe's vectors end.
void keyframe_feature_bytes(KeyFrame* pKF, size_t n, int stride, std::vector<uint8_t>& out) {
    out.assign((size_t)stride, 0);
    for (size_t f = 0; f < n && f < (size_t)stride; ++f) {
        uint8_t b = 0;
        if (f < pKF->mvKeysUn_total.size()) b = (uint8_t)(pKF->mvKeysUn_total[f].octave & ORBM_FEATURE_LEVEL_MASK);
        if (f < pKF->mvDepth_total.size() && (pKF->mvDepth_total[f] > pKF->mThDepth || pKF->mvDepth_total[f] < 0)) b |= ORBM_FEATURE_FAR;
        out[f] = b;
    }
}
}  // namespace

ResidentMap::ResidentMap(ORBmatcher* matcher) : ResidentMap(matcher, Capacity()) {}

ResidentMap::ResidentMap(ORBmatcher* matcher, const Capacity& capacity) : mpMatcher(matcher), mCap(capacity) {
    mCap.keyframes = std::max(1, std::min<int>(mCap.keyframes, ORBM_MAP_MAX_KEYFRAMES));
    mCap.features_per_keyframe = std::max(1, std::min<int>(mCap.features_per_keyframe, ORBM_MAP_MAX_FEATURES));
    mCap.points = std::max(0, mCap.points); mCap.observations = std::max(0, mCap.observations);
}

ResidentMap::~ResidentMap() { orbm_map_destroy(mpMap); }

void ResidentMap::Touch(MapPoint* pMP) {
    if (!pMP) return;
    std::lock_guard<std::mutex> lock(mMutexQueue);
    mvQueuedPoints.push_back(pMP);
}

void ResidentMap::Touch(KeyFrame* pKF) {
    if (!pKF) return;
    std::lock_guard<std::mutex> lock(mMutexQueue);
    mvQueuedKeyFrames.push_back(pKF);
}

int ResidentMap::SlotOf(MapPoint* pMP) {
    auto it = mPoints.find(pMP);
    if (it != mPoints.end()) return it->second.slot;
    const int slot = (int)mvPointOfSlot.size();
    if (slot >= mCap.points) { std::fprintf(stderr, "ResidentMap: more than %d map points\n", mCap.points); mbFailed = true; return -1; }
    mvPointOfSlot.push_back(pMP);
    orbm_point zero; std::memset(&zero, 0, sizeof(zero));
    mvRows.push_back(zero); mvFlags.push_back(0); mvPointNObs.push_back(0); mvPointRef.push_back(-1);   // what an unwritten slot holds on the device
    mPoints[pMP] = PointEntry{slot, {}};
    return slot;
}

int ResidentMap::SlotOf(KeyFrame* pKF) {
    auto it = mKeyFrames.find(pKF);
    if (it != mKeyFrames.end()) return it->second;
    const int slot = (int)mvKeyFrameOfSlot.size();
    if (slot >= mCap.keyframes) { std::fprintf(stderr, "ResidentMap: more than %d keyframes\n", mCap.keyframes); mbFailed = true; return -1; }
    mvKeyFrameOfSlot.push_back(pKF);
    mvKeyFrameRows.resize((size_t)(slot + 1) * mCap.features_per_keyframe, -1);
    mvKeyFrameFeatures.resize((size_t)(slot + 1) * mCap.features_per_keyframe, 0);
    mvKeyFrameCount.push_back(0); mvKeyFrameBad.push_back(0); mvKeyFrameSent.push_back(0); mvKeyFrameNCam1.push_back(0);
    mKeyFrames[pKF] = slot;
    return slot;
}

bool ResidentMap::EnsureDevice() {
    if (!mpMatcher) return true;
    if (mpMap) return true;
    mpHandle = mpMatcher->GetDeviceHandle();
    if (!mpHandle) return false;
    const int rc = orbm_map_create(mpHandle, mCap.keyframes, mCap.points, mCap.observations, mCap.features_per_keyframe, &mpMap);
    if (rc) { mpMap = nullptr; report("ResidentMap", "orbm_map_create", rc); return false; }
    return true;
}

void ResidentMap::LastCovisibility(int out4[4]) const {
    for (int k = 0; k < 4; ++k) out4[k] = 0;
    if (mpMap) (void)orbm_debug_last_covisibility(mpMap, out4);
}

void ResidentMap::LastCorrection(int out4[4]) const {
    for (int k = 0; k < 4; ++k) out4[k] = 0;
    if (mpMap) (void)orbm_debug_last_correction(mpMap, out4);
}

int ResidentMap::Flush() {
    std::lock_guard<std::recursive_mutex> lock_map(mMutexMap);
    mLastFlush = FlushStats();
    if (mbFailed) return -1;                                   // a map that outgrew its capacity or lost a device call stays loud
    std::vector<MapPoint*> points; std::vector<KeyFrame*> keyframes;
    {
        std::lock_guard<std::mutex> lock(mMutexQueue);
        points.swap(mvQueuedPoints); keyframes.swap(mvQueuedKeyFrames);
    }
    if (!EnsureDevice()) return -1;
    if (points.empty() && keyframes.empty()) return 0;
    // an object queued twice is read once
    std::sort(points.begin(), points.end(), std::less<MapPoint*>()); points.erase(std::unique(points.begin(), points.end()), points.end());
    std::sort(keyframes.begin(), keyframes.end(), std::less<KeyFrame*>()); keyframes.erase(std::unique(keyframes.begin(), keyframes.end()), keyframes.end());

    std::vector<int32_t> row_slots, rec_slots; std::vector<orbm_point> rows; std::vector<uint8_t> flags; std::vector<orbm_obs> recs;
    std::vector<int32_t> nobs_slots, nobs, feat_slots, feats, ref_slots, refs;
    for (MapPoint* pMP : points) {
        const int slot = SlotOf(pMP);
        if (slot < 0) return -1;
        KeyFrame* pRefKF = pMP->GetReferenceKeyFrame();        // (what the update after global BA carries the point through)
        const int ref = pRefKF ? SlotOf(pRefKF) : -1;
        if (pRefKF && ref < 0) return -1;
        if (ref != mvPointRef[(size_t)slot]) { mvPointRef[(size_t)slot] = ref; ref_slots.push_back(slot); refs.push_back(ref); }
        const int n_obs = pMP->Observations();                 // (the reference's counter, mirrored as a value)
        if (n_obs != mvPointNObs[(size_t)slot]) { mvPointNObs[(size_t)slot] = n_obs; nobs_slots.push_back(slot); nobs.push_back(n_obs); }
        orbm_point row; pack_point_row(pMP, row);
        const uint8_t flag = pMP->isBad() ? ORBM_POINT_BAD : 0;
        if (std::memcmp(&row, &mvRows[(size_t)slot], sizeof(row)) != 0 || flag != mvFlags[(size_t)slot]) {
            mvRows[(size_t)slot] = row; mvFlags[(size_t)slot] = flag;
            row_slots.push_back(slot); rows.push_back(row); flags.push_back(flag);
        }
        // the observations against the records the mirror holds for the point: both are ordered by keyframe pointer
        const std::map<KeyFrame*, size_t> now = pMP->GetObservations();
        std::map<KeyFrame*, int>& held = mPoints[pMP].records;
        for (auto it = held.begin(); it != held.end();) {
            if (now.count(it->first)) { ++it; continue; }
            mvRecords[(size_t)it->second] = orbm_obs{-1, -1};
            rec_slots.push_back(it->second); recs.push_back(orbm_obs{-1, -1});
            mvFreeRecords.push_back(it->second);
            it = held.erase(it);
        }
        for (const auto& ob : now) {
            // the feature index of the observation in its keyframe, of a record the mirror holds already and of a new one alike
            const int feature = (int)std::min<size_t>(ob.second, (size_t)mCap.features_per_keyframe - 1);
            auto h = held.find(ob.first);
            if (h != held.end()) {
                if (mvRecordFeature[(size_t)h->second] != feature) { mvRecordFeature[(size_t)h->second] = feature; feat_slots.push_back(h->second); feats.push_back(feature); }
                continue;
            }
            const int kf = SlotOf(ob.first);
            if (kf < 0) return -1;
            int rec;
            if (!mvFreeRecords.empty()) { rec = mvFreeRecords.back(); mvFreeRecords.pop_back(); }
            else {
                rec = (int)mvRecords.size();
                if (rec >= mCap.observations) { std::fprintf(stderr, "ResidentMap: more than %d observations\n", mCap.observations); mbFailed = true; return -1; }
                mvRecords.push_back(orbm_obs{-1, -1}); mvRecordFeature.push_back(0);
            }
            if (mvRecordFeature[(size_t)rec] != feature) { mvRecordFeature[(size_t)rec] = feature; feat_slots.push_back(rec); feats.push_back(feature); }
            mvRecords[(size_t)rec] = orbm_obs{slot, kf};
            // a record slot freed and taken again in this Flush: the later entry is the one both sides keep (orbm_map_write_observations
            // stages from its mirror, which holds the last entry of a slot)
            rec_slots.push_back(rec); recs.push_back(orbm_obs{slot, kf});
            held[ob.first] = rec;
        }
    }
    struct KfSend { int slot, n; };
    std::vector<KfSend> kf_send;
    std::vector<int> kf_feat_send;
    std::vector<int32_t> row;
    std::vector<uint8_t> feat_row;
    for (KeyFrame* pKF : keyframes) {
        const int slot = SlotOf(pKF);
        if (slot < 0) return -1;
        const std::vector<MapPoint*> vpMPs = pKF->GetMapPointMatches();
        if ((int)vpMPs.size() > mCap.features_per_keyframe) {
            std::fprintf(stderr, "ResidentMap: a keyframe of %d features does not fit rows of %d\n", (int)vpMPs.size(), mCap.features_per_keyframe);
            mbFailed = true; return -1;
        }
        // a byte per feature: the level, and the far test of LocalMapping::KeyFrameCulling evaluated here, in float, as the reference
        // states it (src/LocalMapping.cc:999).  A keyframe whose key or depth vector is shorter than its matches: level 0, not far.
        keyframe_feature_bytes(pKF, vpMPs.size(), mCap.features_per_keyframe, feat_row);
        const int n_cam1 = std::max(0, std::min(pKF->N, mCap.features_per_keyframe));
        uint8_t* held_feat = mvKeyFrameFeatures.data() + (size_t)slot * mCap.features_per_keyframe;
        if (n_cam1 != mvKeyFrameNCam1[(size_t)slot] || std::memcmp(held_feat, feat_row.data(), feat_row.size()) != 0) {
            std::memcpy(held_feat, feat_row.data(), feat_row.size());
            mvKeyFrameNCam1[(size_t)slot] = n_cam1;
            kf_feat_send.push_back(slot);
        }
        row.assign((size_t)mCap.features_per_keyframe, -1);
        for (size_t f = 0; f < vpMPs.size(); ++f)
            if (vpMPs[f]) { row[f] = SlotOf(vpMPs[f]); if (row[f] < 0) return -1; }
        const uint8_t bad = pKF->isBad() ? 1 : 0;
        int32_t* held = mvKeyFrameRows.data() + (size_t)slot * mCap.features_per_keyframe;
        const bool same_row = mvKeyFrameCount[(size_t)slot] == (int)vpMPs.size() && std::memcmp(held, row.data(), row.size() * sizeof(int32_t)) == 0;
        if (same_row && bad == mvKeyFrameBad[(size_t)slot] && mvKeyFrameSent[(size_t)slot]) continue;   // (the first Flush of a keyframe tells the device of its slot)
        mvKeyFrameSent[(size_t)slot] = 1;
        std::memcpy(held, row.data(), row.size() * sizeof(int32_t));
        mvKeyFrameCount[(size_t)slot] = (int)vpMPs.size(); mvKeyFrameBad[(size_t)slot] = bad;
        kf_send.push_back(KfSend{slot, (int)vpMPs.size()});
    }
    mLastFlush.rows = (int)row_slots.size(); mLastFlush.records = (int)rec_slots.size(); mLastFlush.keyframes = (int)kf_send.size();
    mLastFlush.record_features = (int)feat_slots.size(); mLastFlush.point_nobs = (int)nobs_slots.size(); mLastFlush.keyframe_features = (int)kf_feat_send.size();
    mLastFlush.point_refs = (int)ref_slots.size();
    if (mpMap) {
        // a device call that fails leaves the map loud: reported once, and every later Flush returns -1
        auto sent = [this](const char* call, int rc) {
            if (rc) { report("ResidentMap::Flush", call, rc); mbFailed = true; }
            return rc == 0;
        };
        if (!sent("orbm_map_write_point_ref", orbm_map_write_point_ref(mpHandle, mpMap, ref_slots.data(), (int)ref_slots.size(), refs.data()))) return -1;
        if (!sent("orbm_map_write_point_nobs", orbm_map_write_point_nobs(mpHandle, mpMap, nobs_slots.data(), (int)nobs_slots.size(), nobs.data()))) return -1;
        if (!sent("orbm_map_write_observation_features",
                  orbm_map_write_observation_features(mpHandle, mpMap, feat_slots.data(), (int)feat_slots.size(), feats.data()))) return -1;
        for (int slot : kf_feat_send)
            if (!sent("orbm_map_write_keyframe_features",
                      orbm_map_write_keyframe_features(mpHandle, mpMap, slot, mvKeyFrameFeatures.data() + (size_t)slot * mCap.features_per_keyframe,
                                                       mCap.features_per_keyframe, mvKeyFrameNCam1[(size_t)slot]))) return -1;
        if (!sent("orbm_map_write_points", orbm_map_write_points(mpHandle, mpMap, row_slots.data(), (int)row_slots.size(), rows.data(), flags.data()))) return -1;
        if (!sent("orbm_map_write_observations", orbm_map_write_observations(mpHandle, mpMap, rec_slots.data(), (int)rec_slots.size(), recs.data()))) return -1;
        for (const KfSend& k : kf_send)
            if (!sent("orbm_map_write_keyframe", orbm_map_write_keyframe(mpHandle, mpMap, k.slot, mvKeyFrameRows.data() + (size_t)k.slot * mCap.features_per_keyframe,
                                                                         k.n, mvKeyFrameBad[(size_t)k.slot]))) return -1;
    }
    return mLastFlush.rows + mLastFlush.records + mLastFlush.keyframes;
}

int ResidentMap::Audit(const std::vector<KeyFrame*>& vpKeyFrames, const std::vector<MapPoint*>& vpMapPoints) {
    std::lock_guard<std::recursive_mutex> lock_map(mMutexMap);
    int differences = 0;
    std::vector<uint8_t> feat_row;
    for (MapPoint* pMP : vpMapPoints) {
        if (!pMP) continue;
        auto it = mPoints.find(pMP);
        if (it == mPoints.end()) { ++differences; continue; }
        const int slot = it->second.slot;
        orbm_point row; pack_point_row(pMP, row);
        if (std::memcmp(&row, &mvRows[(size_t)slot], sizeof(row)) != 0) ++differences;
        if ((pMP->isBad() ? ORBM_POINT_BAD : 0) != mvFlags[(size_t)slot]) ++differences;
        if (pMP->Observations() != mvPointNObs[(size_t)slot]) ++differences;
        {
            KeyFrame* pRefKF = pMP->GetReferenceKeyFrame();
            auto r = pRefKF ? mKeyFrames.find(pRefKF) : mKeyFrames.end();
            if ((pRefKF ? (r == mKeyFrames.end() ? -2 : r->second) : -1) != mvPointRef[(size_t)slot]) ++differences;
        }
        const std::map<KeyFrame*, size_t> now = pMP->GetObservations();
        const std::map<KeyFrame*, int>& held = it->second.records;
        bool same = now.size() == held.size();
        for (auto a = now.begin(); same && a != now.end(); ++a) {
            auto h = held.find(a->first);
            same = h != held.end() && mvRecords[(size_t)h->second].point == slot && mKeyFrames.count(a->first) &&
                   mvRecords[(size_t)h->second].keyframe == mKeyFrames[a->first] &&
                   mvRecordFeature[(size_t)h->second] == (int)std::min<size_t>(a->second, (size_t)mCap.features_per_keyframe - 1);
        }
        if (!same) ++differences;
    }
    for (KeyFrame* pKF : vpKeyFrames) {
        if (!pKF) continue;
        auto it = mKeyFrames.find(pKF);
        if (it == mKeyFrames.end()) { ++differences; continue; }
        const int slot = it->second;
        if ((pKF->isBad() ? 1 : 0) != mvKeyFrameBad[(size_t)slot]) ++differences;
        const std::vector<MapPoint*> vpMPs = pKF->GetMapPointMatches();
        bool same = (int)vpMPs.size() == mvKeyFrameCount[(size_t)slot];
        const int32_t* held = mvKeyFrameRows.data() + (size_t)slot * mCap.features_per_keyframe;
        for (size_t f = 0; same && f < vpMPs.size(); ++f) {
            int want = -1;
            if (vpMPs[f]) { auto p = mPoints.find(vpMPs[f]); want = p == mPoints.end() ? -2 : p->second.slot; }
            same = held[f] == want;
        }
        if (!same) ++differences;
        keyframe_feature_bytes(pKF, vpMPs.size(), mCap.features_per_keyframe, feat_row);
        if (std::max(0, std::min(pKF->N, mCap.features_per_keyframe)) != mvKeyFrameNCam1[(size_t)slot] ||
            std::memcmp(mvKeyFrameFeatures.data() + (size_t)slot * mCap.features_per_keyframe, feat_row.data(), feat_row.size()) != 0) ++differences;
    }
    return differences;
}

int ResidentMap::Vote(const std::vector<int32_t>& frame_points, std::vector<int32_t>& votes) {
    std::lock_guard<std::recursive_mutex> lock_map(mMutexMap);
    const int n_kfs = (int)mvKeyFrameOfSlot.size();
    votes.assign((size_t)std::max(n_kfs, 1), 0);
    if (mpMap) {
        // (the device's high-water mark may lie below the slots handed out: a keyframe that has a slot but was never written or named)
        const int rc = orbm_map_vote(mpHandle, mpMap, frame_points.data(), (int)frame_points.size(), votes.data());
        if (rc) report("UpdateLocalMap", "orbm_map_vote", rc);
        return rc;
    }
    const int rc = orbm_local_map_vote_host(mvRecords.data(), (int)mvRecords.size(), mvFlags.data(), (int)mvFlags.size(), frame_points.data(),
                                            (int)frame_points.size(), n_kfs, votes.data());
    if (rc) report("UpdateLocalMap", "orbm_local_map_vote_host", rc);
    return rc;
}

bool ResidentMap::SlotsOfSent(const std::vector<KeyFrame*>& vpKFs, size_t begin, size_t end, std::vector<int32_t>& slots) {
    slots.clear();
    bool fresh = false;
    for (size_t i = begin; i < end; ++i) {
        const int slot = SlotOf(vpKFs[i]);
        if (slot < 0) return false;
        slots.push_back(slot);
        if (!mvKeyFrameSent[(size_t)slot]) { Touch(vpKFs[i]); fresh = true; }   // (Audit counts such keyframes)
    }
    return !fresh || Flush() >= 0;
}

int ResidentMap::Covisibility(const std::vector<int32_t>& kfs, std::vector<int32_t>& first, std::vector<orbm_covis_entry>& entries) {
    std::lock_guard<std::recursive_mutex> lock_map(mMutexMap);
    const int n = (int)kfs.size();
    first.assign((size_t)n + 1, 0);
    if (entries.size() < 1024) entries.resize(1024);
    for (int attempt = 0; attempt < 2; ++attempt) {            // a list too short says how long it must be: asked again once
        int rc;
        if (mpMap) rc = orbm_map_covisibility(mpHandle, mpMap, kfs.data(), n, first.data(), entries.data(), (int)entries.size());
        else rc = orbm_local_map_covisibility_host(mvRecords.data(), mvRecordFeature.data(), (int)mvRecords.size(), mvFlags.data(), (int)mvFlags.size(),
                                                   mvKeyFrameRows.data(), mvKeyFrameCount.data(), mvKeyFrameNCam1.data(), (int)mvKeyFrameOfSlot.size(),
                                                   mCap.features_per_keyframe, kfs.data(), n, first.data(), entries.data(), (int)entries.size());
        if (rc == ORB_E_CAPACITY && attempt == 0 && first[(size_t)n] > (int)entries.size()) { entries.resize((size_t)first[(size_t)n]); continue; }
        if (rc) report("CovisibilityCounts", mpMap ? "orbm_map_covisibility" : "orbm_local_map_covisibility_host", rc);
        return rc;
    }
    return ORB_E_CAPACITY;
}

int ResidentMap::CullingCounts(const std::vector<int32_t>& kfs, bool mono, std::vector<int32_t>& counts) {
    std::lock_guard<std::recursive_mutex> lock_map(mMutexMap);
    const int n = (int)kfs.size();
    counts.assign((size_t)std::max(n, 1) * 2, 0);
    int rc;
    if (mpMap) rc = orbm_map_culling_counts(mpHandle, mpMap, kfs.data(), n, mono ? 1 : 0, counts.data());
    else rc = orbm_local_map_culling_host(mvRecords.data(), mvRecordFeature.data(), (int)mvRecords.size(), mvFlags.data(), mvPointNObs.data(),
                                          (int)mvFlags.size(), mvKeyFrameRows.data(), mvKeyFrameCount.data(), mvKeyFrameFeatures.data(),
                                          (int)mvKeyFrameOfSlot.size(), mCap.features_per_keyframe, kfs.data(), n, mono ? 1 : 0, counts.data());
    if (rc) report("KeyFrameCulling", mpMap ? "orbm_map_culling_counts" : "orbm_local_map_culling_host", rc);
    return rc;
}

int ResidentMap::LocalPoints(const std::vector<int32_t>& local_kfs, std::vector<int32_t>& list) {
    std::lock_guard<std::recursive_mutex> lock_map(mMutexMap);
    list.assign(ORBM_MAX_POINTS, 0);
    int n = 0, rc;
    if (mpMap) {
        rc = orbm_map_local_points(mpHandle, mpMap, local_kfs.data(), (int)local_kfs.size(), list.data(), &n);
        if (rc) report("UpdateLocalMap", "orbm_map_local_points", rc);
    } else {
        rc = orbm_local_map_points_host(mvKeyFrameRows.data(), mvKeyFrameCount.data(), (int)mvKeyFrameOfSlot.size(), mCap.features_per_keyframe,
                                        mvFlags.data(), (int)mvFlags.size(), local_kfs.data(), (int)local_kfs.size(), list.data(),
                                        ORBM_MAX_POINTS, &n);
        if (rc) report("UpdateLocalMap", "orbm_local_map_points_host", rc);
    }
    list.resize(rc ? 0 : (size_t)n);
    return rc;
}

void UpdateLocalMap(ResidentMap& R, Frame& F, std::vector<KeyFrame*>& vpLocalKeyFrames, std::vector<MapPoint*>& vpLocalMapPoints,
                    KeyFrame*& pReferenceKF) {
    std::lock_guard<std::recursive_mutex> lock_map(R.mMutexMap);
    const bool flushed = R.Flush() >= 0;

    // ---- UpdateLocalKeyFrames (src/Tracking.cc:1832-1949)
    // Each map point votes for the keyframes in which it has been observed (:1838-1855): the frame's points as slots
    std::vector<int32_t>& fp = R.mvFramePoints;
    fp.assign(F.mvpMapPoints.size(), -1);
    for (size_t i = 0; i < F.mvpMapPoints.size(); ++i) {
        MapPoint* pMP = F.mvpMapPoints[i];
        if (!pMP) continue;
        if (!pMP->isBad()) fp[i] = R.SlotOf(pMP);             // (a point the map never saw gets an empty slot: it casts no vote, and Audit counts it)
        else F.mvpMapPoints[i] = static_cast<MapPoint*>(NULL);
    }
    vpLocalMapPoints.clear();                                  // (:1797; done here so that every failure below leaves an empty list)
    R.mvList.clear();
    if (!flushed || R.Vote(fp, R.mvVotes)) return;

    std::vector<KeyFrame*> voted;                              // keyframeCounter's keys, in std::map order: ascending pointer
    for (size_t k = 0; k < R.mvKeyFrameOfSlot.size(); ++k)
        if (R.mvVotes[k] > 0) voted.push_back(R.mvKeyFrameOfSlot[k]);
    std::sort(voted.begin(), voted.end(), std::less<KeyFrame*>());

    if (!voted.empty()) {                                      // (:1857: otherwise the keyframes stay as they are)
        int max = 0;
        KeyFrame* pKFmax = static_cast<KeyFrame*>(NULL);
        vpLocalKeyFrames.clear();
        vpLocalKeyFrames.reserve(3 * voted.size());

        // K1: all keyframes that observe a map point of the frame; which of them shares most points (:1871-1886)
        for (KeyFrame* pKF : voted) {
            if (pKF->isBad()) continue;
            const int votes = R.mvVotes[(size_t)R.mKeyFrames[pKF]];
            if (votes > max) { max = votes; pKFmax = pKF; }
            vpLocalKeyFrames.push_back(pKF);
            pKF->mnTrackReferenceForFrame = F.mnId;
        }

        // K2: neighbours of K1 in the covisibility graph (:1892-1942).  The walk covers K1 only: the end is taken before it starts.
        const size_t nK1 = vpLocalKeyFrames.size();
        for (size_t i = 0; i < nK1; ++i) {
            // Limit the number of keyframes
            if (vpLocalKeyFrames.size() > 80) break;

            KeyFrame* pKF = vpLocalKeyFrames[i];

            const std::vector<KeyFrame*> vNeighs = pKF->GetBestCovisibilityKeyFrames(10);
            for (std::vector<KeyFrame*>::const_iterator itNeighKF = vNeighs.begin(), itEndNeighKF = vNeighs.end(); itNeighKF != itEndNeighKF; itNeighKF++) {
                KeyFrame* pNeighKF = *itNeighKF;
                if (!pNeighKF->isBad()) {
                    if (pNeighKF->mnTrackReferenceForFrame != F.mnId) {
                        vpLocalKeyFrames.push_back(pNeighKF);
                        pNeighKF->mnTrackReferenceForFrame = F.mnId;
                        break;
                    }
                }
            }

            const std::set<KeyFrame*> spChilds = pKF->GetChilds();
            for (std::set<KeyFrame*>::const_iterator sit = spChilds.begin(), send = spChilds.end(); sit != send; sit++) {
                KeyFrame* pChildKF = *sit;
                if (!pChildKF->isBad()) {
                    if (pChildKF->mnTrackReferenceForFrame != F.mnId) {
                        vpLocalKeyFrames.push_back(pChildKF);
                        pChildKF->mnTrackReferenceForFrame = F.mnId;
                        break;
                    }
                }
            }

            KeyFrame* pParent = pKF->GetParent();
            if (pParent) {
                if (pParent->mnTrackReferenceForFrame != F.mnId) {
                    vpLocalKeyFrames.push_back(pParent);
                    pParent->mnTrackReferenceForFrame = F.mnId;
                    break;                                     // leaves the OUTER loop, as :1938 does
                }
            }
        }

        if (pKFmax) {
            pReferenceKF = pKFmax;
            F.mpReferenceKF = pReferenceKF;
        }
    }

    // ---- UpdateLocalPoints (:1794-1824) over the rows of the local keyframes
    if (vpLocalKeyFrames.size() > (size_t)ORBM_MAP_MAX_LOCAL) {
        std::fprintf(stderr, "UpdateLocalMap: %d local keyframes are more than a call takes (%d)\n", (int)vpLocalKeyFrames.size(), (int)ORBM_MAP_MAX_LOCAL);
        return;
    }
    std::vector<int32_t>& local = R.mvLocalSlots;
    local.clear();
    bool fresh = false;
    for (KeyFrame* pKF : vpLocalKeyFrames) {
        const int slot = R.SlotOf(pKF);
        if (slot < 0) return;
        local.push_back(slot);
        // a keyframe the map has never been told of: its row is read now, as a Touch would have it (Audit counts such keyframes)
        if (!R.mvKeyFrameSent[(size_t)slot]) { R.Touch(pKF); fresh = true; }
    }
    if (fresh && R.Flush() < 0) return;
    if (R.LocalPoints(local, R.mvList)) { R.mvList.clear(); return; }
    vpLocalMapPoints.reserve(R.mvList.size());
    for (int32_t slot : R.mvList) {
        MapPoint* pMP = R.mvPointOfSlot[(size_t)slot];
        vpLocalMapPoints.push_back(pMP);
        pMP->mnTrackReferenceForFrame = F.mnId;
    }
}

int SearchLocalPoints(ORBmatcher& matcher, ResidentMap& R, Frame& F, std::vector<MapPoint*>& vpLocalMapPoints, float th, int* nToMatch) {
    static const char* who = "SearchLocalPoints";
    std::lock_guard<std::recursive_mutex> lock_map(R.mMutexMap);
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
    if (!R.mpMap) { std::fprintf(stderr, "%s: the resident map is not on a device -- search reports 0 matches\n", who); return 0; }
    if (n != (int)R.mvList.size()) {
        std::fprintf(stderr, "%s: %d local points handed in, the list of the last UpdateLocalMap has %d -- search reports 0 matches\n", who, n, (int)R.mvList.size());
        return 0;
    }
    ORBmatcher::LocalSearchContext C;
    if (!matcher.GetLocalSearchContext(F, &C)) return 0;
    if (C.handle != R.mpHandle) { std::fprintf(stderr, "%s: the resident map belongs to another thread's handle -- search reports 0 matches\n", who); return 0; }
    if (R.Flush() < 0) return 0;                               // (what the mapping thread touched since UpdateLocalMap)

    // which points take no part (:1740-1743): one integer compare and one flag per point, no packing.  They travel as the `seen`
    // list; the frame's own points are among them (loop 1 stamped them), so frame_points stays empty.
    R.mvSkip.assign((size_t)n, 0); R.mvSeen.clear();
    for (int i = 0; i < n; ++i) {
        MapPoint* pMP = vpLocalMapPoints[i];
        if (pMP->mnLastFrameSeen == F.mnId || pMP->isBad()) { R.mvSkip[(size_t)i] = 1; R.mvSeen.push_back(R.mvList[(size_t)i]); }
    }

    orbm_view V;
    const cv::Mat Ow = F.GetCameraCenter();
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) V.Rcw[3 * i + j] = F.mTcw.at<float>(i, j);
        V.tcw[i] = F.mTcw.at<float>(i, 3);
        V.Ow[i] = Ow.at<float>(i);
    }
    V.fx = F.fx; V.fy = F.fy; V.cx = F.cx; V.cy = F.cy; V.mbf = F.mbf;
    V.min_x = F.mnMinX; V.max_x = F.mnMaxX; V.min_y = F.mnMinY; V.max_y = F.mnMaxY;
    V.viewing_cos_limit = 0.5f;                                // src/Tracking.cc:1746
    V.th = th;
    V.log_scale_factor = F.mfLogScaleFactor; V.n_levels = F.mnScaleLevels; V.scale_factors = F.mvScaleFactors.data();

    R.mvOccupied.resize((size_t)std::max(F.N, 1));
    for (int g = 0; g < F.N; ++g)
        R.mvOccupied[(size_t)g] = (F.mvpMapPoints[g] && F.mvpMapPoints[g]->Observations() > 0) ? 1 : 0;   // src/ORBmatcher.cc:107-109
    R.mvTrack.resize((size_t)n); R.mvMatch.resize((size_t)std::max(F.N, 1));
    int in_view = 0, nmatches = 0;
    const int rc = orbm_map_search_local_points(C.handle, C.frame, R.mpMap, &V, nullptr, 0, R.mvSeen.data(), (int)R.mvSeen.size(),
                                                R.mvOccupied.data(), C.nnratio, ORBmatcher::TH_HIGH, R.mvTrack.data(), R.mvMatch.data(),
                                                &in_view, &nmatches);
    if (rc) { report(who, "orbm_map_search_local_points", rc); std::fprintf(stderr, "%s: search reports 0 matches\n", who); return 0; }
    // what isInFrustum leaves in the points it was called for (src/Frame.cc:445, :491-496; src/Tracking.cc:1746-1750)
    for (int i = 0; i < n; ++i) {
        if (R.mvSkip[(size_t)i]) continue;
        MapPoint* pMP = vpLocalMapPoints[i];
        const orbm_track& t = R.mvTrack[(size_t)i];
        pMP->mbTrackInView = t.in_view != 0;
        if (!t.in_view) continue;
        pMP->mTrackProjX = t.proj_x; pMP->mTrackProjY = t.proj_y; pMP->mTrackProjXR = t.proj_xr;
        pMP->mnTrackScaleLevel = t.level; pMP->mTrackViewCos = t.view_cos;
        pMP->IncreaseVisible();
    }
    if (nToMatch) *nToMatch = in_view;
    for (int g = 0; g < F.N; ++g)
        if (R.mvMatch[(size_t)g] >= 0) F.mvpMapPoints[g] = vpLocalMapPoints[(size_t)R.mvMatch[(size_t)g]];   // src/ORBmatcher.cc:143
    return nmatches;
}

}  // namespace ORB_SLAM2
