// KeyFrameDatabase.cc -- see KeyFrameDatabase.h.  Line numbers refer to the reference's src/KeyFrameDatabase.cc.
#include "KeyFrameDatabase.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include "../../include/orbv.h"

#include "resident.h"

namespace ORB_SLAM2 {

// Loop detection and relocalisation are one procedure over different scratch fields of KeyFrame, apart from three rules.
struct KeyFrameDatabase::Rules {
    long unsigned int KeyFrame::*asked_by;   // id of the query that last listed the keyframe
    int KeyFrame::*shared;                   // words shared with that query
    float KeyFrame::*score;                  // L1 score against that query, when it was computed
    bool skip_connected;      // loop: a keyframe connected to the asker is counted to 1, neither marked nor listed (:146)
    bool min_score_applies;   // loop: only scores >= minScore go on (:190) and no group total below minScore raises the bar (:199);
                              // relocalisation: every score goes on (:479), the bar starts at 0 (:487)
    bool neighbour_needs_words;   // loop: a marked neighbour joins a group only above the word threshold (:216); relocalisation: marked is enough (:505)
};

namespace {

[[noreturn]] void fail(const char* what, int rc) {
    std::fprintf(stderr, "KeyFrameDatabase::%s failed (%d): %s\n", what, rc, orb_last_error());
    std::abort();   // there is no host path to fall back to
}

void flatten(const DBoW2::BowVector& v, std::vector<uint32_t>& id, std::vector<double>& val) {
    id.clear(); val.clear();
    id.reserve(v.size()); val.reserve(v.size());
    for (const auto& word : v) { id.push_back(word.first); val.push_back(word.second); }
}

}  // namespace

KeyFrameDatabase::KeyFrameDatabase(const ORBVocabulary& voc) : mpVoc(&voc) {
    const int words = voc.size() ? (int)voc.size() : 1;
    int rc = orbv_db_create(words, host_device(), &mpDb);
    if (!rc) rc = orbv_db_create(words, host_device(), &mpDb_cam1);
    if (rc) {   // fail once, here, and not at the first add or query
        const std::string why = std::string("KeyFrameDatabase: no database on the device: ") + orb_last_error();
        orbv_db_destroy(mpDb);
        throw std::runtime_error(why);
    }
}

KeyFrameDatabase::~KeyFrameDatabase() { orbv_db_destroy(mpDb); orbv_db_destroy(mpDb_cam1); }

void KeyFrameDatabase::Add(KeyFrame* pKF, bool cam1) {
    std::unique_lock<std::mutex> lock(mMutex);
    std::map<long unsigned int, KeyFrame*>& known = cam1 ? mKeyFrames_cam1 : mKeyFrames;
    if (known.count(pKF->mnId)) {
        // the reference pushes the keyframe onto its lists a second time and counts its words twice from then on; here: refused
        static bool told = false;
        if (!told) { told = true; std::fprintf(stderr, "KeyFrameDatabase::add: keyframe %lu is already in the database; ignored\n", pKF->mnId); }
        return;
    }
    std::vector<uint32_t> id; std::vector<double> val;
    flatten(cam1 ? pKF->mBowVec_cam1 : pKF->mBowVec, id, val);
    const int rc = orbv_db_add(cam1 ? mpDb_cam1 : mpDb, pKF->mnId, id.data(), val.data(), (int)id.size());
    if (rc) fail(cam1 ? "add_cam1" : "add", rc);
    known[pKF->mnId] = pKF;
}

void KeyFrameDatabase::add(KeyFrame* pKF) { Add(pKF, false); }         // :41-48
void KeyFrameDatabase::add_cam1(KeyFrame* pKF) { Add(pKF, true); }     // :51-57

void KeyFrameDatabase::erase(KeyFrame* pKF) {                          // :63-97: out of both files
    std::unique_lock<std::mutex> lock(mMutex);
    int rc = orbv_db_erase(mpDb, pKF->mnId);
    if (!rc) rc = orbv_db_erase(mpDb_cam1, pKF->mnId);
    if (rc) fail("erase", rc);
    mKeyFrames.erase(pKF->mnId); mKeyFrames_cam1.erase(pKF->mnId);
}

void KeyFrameDatabase::clear() {                                       // :99-105
    std::unique_lock<std::mutex> lock(mMutex);
    int rc = orbv_db_clear(mpDb);
    if (!rc) rc = orbv_db_clear(mpDb_cam1);
    if (rc) fail("clear", rc);
    mKeyFrames.clear(); mKeyFrames_cam1.clear();
}

std::vector<KeyFrame*> KeyFrameDatabase::DetectLoopCandidates(KeyFrame* pKF, float minScore) {
    static const Rules loop = {&KeyFrame::mnLoopQuery, &KeyFrame::mnLoopWords, &KeyFrame::mLoopScore, true, true, true};
    return Detect(loop, false, pKF->mnId, pKF->mBowVec, pKF->GetConnectedKeyFrames(), minScore);
}

std::vector<KeyFrame*> KeyFrameDatabase::DetectLoopCandidates_cam1(KeyFrame* pKF, float minScore) {
    static const Rules loop = {&KeyFrame::mnLoopQuery, &KeyFrame::mnLoopWords, &KeyFrame::mLoopScore, true, true, true};
    return Detect(loop, true, pKF->mnId, pKF->mBowVec_cam1, pKF->GetConnectedKeyFrames_cam1(), minScore);
}

std::vector<KeyFrame*> KeyFrameDatabase::DetectRelocalizationCandidates(Frame* F) {
    static const Rules reloc = {&KeyFrame::mnRelocQuery, &KeyFrame::mnRelocWords, &KeyFrame::mRelocScore, false, false, false};
    return Detect(reloc, true, F->mnId, F->mBowVec_cam1, std::set<KeyFrame*>(), 0.f);
}

std::vector<KeyFrame*> KeyFrameDatabase::Detect(const Rules& rules, bool cam1, long unsigned int asker, const DBoW2::BowVector& words,
                                                const std::set<KeyFrame*>& connected, float minScore) {
    struct Listed { KeyFrame* kf; double l1; };
    std::vector<Listed> listed;   // the reference's list of keyframes sharing words, in its order, with the L1 score of each
    {
        std::unique_lock<std::mutex> lock(mMutex);
        orbv_database* db = cam1 ? mpDb_cam1 : mpDb;
        const std::map<long unsigned int, KeyFrame*>& known = cam1 ? mKeyFrames_cam1 : mKeyFrames;
        std::vector<uint32_t> id; std::vector<double> val;
        flatten(words, id, val);
        const int capacity = orbv_db_count(db);
        std::vector<uint64_t> key(capacity);
        std::vector<int32_t> common(capacity);
        std::vector<double> l1(capacity);
        const uint32_t* pid = id.data(); const double* pval = val.data();
        const int n = (int)id.size();
        int hits = 0;
        const int rc = orbv_db_query(db, 1, &pid, &pval, &n, capacity, key.data(), common.data(), l1.data(), &hits);
        if (rc) fail("Detect*Candidates", rc);
        // What the word-by-word walk (:132-153, :429-446) leaves in a keyframe it meets `common` times, the first rule that applies:
        for (int i = 0; i < hits; ++i) {
            KeyFrame* kf = known.at((long unsigned int)key[i]);
            if (kf->*rules.asked_by == asker) kf->*rules.shared += common[i];                        // carries this id already: counted on top
            else if (rules.skip_connected && connected.count(kf)) kf->*rules.shared = 1;            // restarts at every meeting, never marked
            else { kf->*rules.asked_by = asker; kf->*rules.shared = common[i]; listed.push_back(Listed{kf, l1[i]}); }
        }
    }
    if (listed.empty()) return {};

    int most = 0;
    for (const Listed& c : listed) most = std::max(most, c.kf->*rules.shared);
    const int word_floor = most * 0.8f;   // int = int * float, as the reference computes it (:171, :461)

    struct Scored { float value; KeyFrame* kf; };
    std::vector<Scored> scored;
    for (const Listed& c : listed) {
        if (!(c.kf->*rules.shared > word_floor)) continue;
        const float s = (float)c.l1;      // the reference keeps the score as a float from here on
        c.kf->*rules.score = s;
        if (!rules.min_score_applies || s >= minScore) scored.push_back(Scored{s, c.kf});
    }
    if (scored.empty()) return {};

    // one group per scored keyframe: itself and those of its ten best covisible keyframes that this query marked
    std::vector<Scored> groups;   // (total of the group, its best member)
    float bar = rules.min_score_applies ? minScore : 0.f;
    for (const Scored& seed : scored) {
        const std::vector<KeyFrame*> near = cam1 ? seed.kf->GetBestCovisibilityKeyFrames_cam1(10) : seed.kf->GetBestCovisibilityKeyFrames(10);
        float total = seed.value, top = seed.value;
        KeyFrame* top_kf = seed.kf;
        for (KeyFrame* other : near) {
            if (other->*rules.asked_by != asker) continue;
            if (rules.neighbour_needs_words && !(other->*rules.shared > word_floor)) continue;
            total += other->*rules.score;   // whatever it holds: relocalisation may meet a score of an earlier query here (:508)
            if (other->*rules.score > top) { top = other->*rules.score; top_kf = other; }
        }
        groups.push_back(Scored{total, top_kf});
        if (total > bar) bar = total;
    }

    const float keep_above = 0.75f * bar;
    std::vector<KeyFrame*> out;
    for (const Scored& g : groups)
        if (g.value > keep_above && std::find(out.begin(), out.end(), g.kf) == out.end()) out.push_back(g.kf);
    return out;
}

}  // namespace ORB_SLAM2
