// KeyFrameDatabase.h -- drop-in for the reference's include/KeyFrameDatabase.h:42-61 (same public member functions): place recognition
// for loop closing and relocalisation.  The two inverted files (all cameras / camera 1) are two resident databases in HBM here
// (include/orbv.h, orbv_db_*): the walk over the query's words is one k_db_query pass that returns the keyframes sharing a word with the
// query in the reference's order, with the shared-word counts and the L1 scores; what follows (word threshold, scores, covisibility groups,
// the retained best: src/KeyFrameDatabase.cc:157-254, :305-401, :449-542) is one host routine for the three Detect methods, with the
// reference's number types at every step.  mMutex is held around every use of the handles (a database handle serves one caller at a time);
// clear(), which the reference leaves unlocked, takes it too.  Without a device the constructor throws std::runtime_error: there is no
// host path.
#ifndef KEYFRAMEDATABASE_H
#define KEYFRAMEDATABASE_H

#include <map>
#include <mutex>
#include <set>
#include <vector>

#ifdef MORB_USE_REFERENCE_TYPES
#include "KeyFrame.h"
#include "Frame.h"
#include "ORBVocabulary.h"
#else
#include "slam_types.h"
#endif

struct orbv_database;

namespace ORB_SLAM2 {

class KeyFrame;
class Frame;

class KeyFrameDatabase {
public:
    KeyFrameDatabase(const ORBVocabulary& voc);
    ~KeyFrameDatabase();
    KeyFrameDatabase(const KeyFrameDatabase&) = delete;
    KeyFrameDatabase& operator=(const KeyFrameDatabase&) = delete;

    void add(KeyFrame* pKF);
    void add_cam1(KeyFrame* pKF);
    void erase(KeyFrame* pKF);
    void clear();
    std::vector<KeyFrame*> DetectLoopCandidates(KeyFrame* pKF, float minScore);
    std::vector<KeyFrame*> DetectLoopCandidates_cam1(KeyFrame* pKF, float minScore);
    std::vector<KeyFrame*> DetectRelocalizationCandidates(Frame* F);

protected:
    struct Rules;   // where loop detection and relocalisation differ (KeyFrameDatabase.cc)
    std::vector<KeyFrame*> Detect(const Rules& rules, bool cam1, long unsigned int asker, const DBoW2::BowVector& words,
                                  const std::set<KeyFrame*>& connected, float minScore);
    void Add(KeyFrame* pKF, bool cam1);

    const ORBVocabulary* mpVoc;
    // one database per inverted file of the reference (key = mnId) and the way back from a key to its keyframe
    orbv_database* mpDb = nullptr;
    orbv_database* mpDb_cam1 = nullptr;
    std::map<long unsigned int, KeyFrame*> mKeyFrames, mKeyFrames_cam1;
    std::mutex mMutex;
};

}  // namespace ORB_SLAM2

#endif
