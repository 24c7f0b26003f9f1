// Covisibility.cc -- see Covisibility.h.
#include "Covisibility.h"

#include <algorithm>
#include <cstdio>

namespace ORB_SLAM2 {

void CovisibilityCounts(ResidentMap& R, const std::vector<KeyFrame*>& vpKFs, std::vector<std::map<KeyFrame*, int> >& vKFcounter,
                        std::vector<std::map<KeyFrame*, int> >& vKFcounter_cam1) {
    std::lock_guard<std::recursive_mutex> lock_map(R.mMutexMap);
    vKFcounter.assign(vpKFs.size(), std::map<KeyFrame*, int>());
    vKFcounter_cam1.assign(vpKFs.size(), std::map<KeyFrame*, int>());
    if (R.Flush() < 0) return;
    std::vector<int32_t> slots, first;
    std::vector<orbm_covis_entry> entries;
    for (size_t begin = 0; begin < vpKFs.size(); begin += ORBM_MAP_MAX_LOCAL) {   // (a call takes ORBM_MAP_MAX_LOCAL keyframes)
        const size_t end = std::min(vpKFs.size(), begin + (size_t)ORBM_MAP_MAX_LOCAL);
        if (!R.SlotsOfSent(vpKFs, begin, end, slots) || R.Covisibility(slots, first, entries)) {
            for (size_t i = 0; i < vpKFs.size(); ++i) { vKFcounter[i].clear(); vKFcounter_cam1[i].clear(); }
            return;
        }
        for (size_t j = 0; j < slots.size(); ++j)
            for (int e = first[j]; e < first[j + 1]; ++e) {
                KeyFrame* pKFi = R.mvKeyFrameOfSlot[(size_t)entries[(size_t)e].keyframe];
                vKFcounter[begin + j][pKFi] = entries[(size_t)e].all;
                if (entries[(size_t)e].cam1 > 0) vKFcounter_cam1[begin + j][pKFi] = entries[(size_t)e].cam1;
            }
    }
}

void CovisibilityCounts(ResidentMap& R, KeyFrame* pKF, std::map<KeyFrame*, int>& KFcounter, std::map<KeyFrame*, int>& KFcounter_cam1) {
    std::vector<std::map<KeyFrame*, int> > all, cam1;
    CovisibilityCounts(R, std::vector<KeyFrame*>(1, pKF), all, cam1);
    KFcounter.swap(all[0]); KFcounter_cam1.swap(cam1[0]);
}

void KeyFrameCulling(ResidentMap& R, KeyFrame* pCurrentKF, bool bMonocular) {
    std::lock_guard<std::recursive_mutex> lock_map(R.mMutexMap);
    // Check redundant keyframes (only local keyframes): the reference's list, taken once (src/LocalMapping.cc:974)
    const std::vector<KeyFrame*> vpLocalKeyFrames = pCurrentKF->GetVectorCovisibleKeyFrames();
    std::vector<KeyFrame*> todo;
    for (KeyFrame* pKF : vpLocalKeyFrames)
        if (pKF->mnId != 0) todo.push_back(pKF);

    std::vector<int32_t> slots, counts;
    size_t at = 0;
    while (at < todo.size()) {
        // the counts of the keyframes not judged yet, on the map as it is now
        if (R.Flush() < 0) return;
        const size_t end = std::min(todo.size(), at + (size_t)ORBM_MAP_MAX_LOCAL);
        if (!R.SlotsOfSent(todo, at, end, slots) || R.CullingCounts(slots, bMonocular, counts)) return;
        const size_t begin = at;
        bool changed = false;
        for (; at < end && !changed; ++at) {
            KeyFrame* pKF = todo[at];
            const int nMPs = counts[2 * (at - begin)], nRedundantObservations = counts[2 * (at - begin) + 1];
            if (!(nRedundantObservations > 0.90 * nMPs)) continue;
            // what SetBadFlag is about to change, gathered before it does: the keyframe's points and who observes them
            const std::vector<MapPoint*> vpMapPoints = pKF->GetMapPointMatches();
            std::vector<std::map<KeyFrame*, size_t> > observers(vpMapPoints.size());
            for (size_t i = 0; i < vpMapPoints.size(); ++i)
                if (vpMapPoints[i]) observers[i] = vpMapPoints[i]->GetObservations();
            pKF->SetBadFlag();
            if (!pKF->isBad()) continue;                       // refused (mbNotErase): nothing changed
            R.Touch(pKF);
            for (size_t i = 0; i < vpMapPoints.size(); ++i) {
                MapPoint* pMP = vpMapPoints[i];
                if (!pMP) continue;
                R.Touch(pMP);                                  // it lost an observation
                if (pMP->isBad())                              // ... and went bad over it: every keyframe that held it let go of it
                    for (const auto& ob : observers[i]) R.Touch(ob.first);
            }
            changed = true;
        }
    }
    (void)R.Flush();                                           // (what the last culled keyframe changed)
}

}  // namespace ORB_SLAM2
