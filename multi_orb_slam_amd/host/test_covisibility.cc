// test_covisibility.cc -- driver of CovisibilityCounts / KeyFrameCulling (host/Covisibility.h) for tests/test_covisibility_class.py and
// tools/covisibility_bench.py.
//
//   test_covisibility host      no device: seeded stand-in maps and hand-built cases, every one built twice from the same draws.  On
//                               one twin runs a transcription of the reference on the stand-in types, std::map copies included --
//                               KeyFrame::UpdateConnections whole (src/KeyFrame.cc:486-668), LocalMapping::KeyFrameCulling
//                               (src/LocalMapping.cc:966-1038) --, on the other CovisibilityCounts followed by the transcribed rest of
//                               UpdateConnections, and KeyFrameCulling, over a host-only ResidentMap.  Compared: the weights, both
//                               ordered vectors and their weights, the parent, mbFirstConnection, the AddConnection / SetBadFlag calls
//                               in order; after the culling every keyframe's and point's flags, counters, observations and matches.
//                               Audit == 0 after every case.  The ninety-percent rule at 9 of 10, 10 of 10 and 0 of 0.
//   test_covisibility device    the same with the ResidentMap on the device.
//   test_covisibility time KEYFRAMES POINTS OBSERVERS LISTED SECONDS
//                               a seeded map of that size (OBSERVERS keyframes per point on average); the counters of LISTED keyframes
//                               and the culling counts of LISTED keyframes through the class and through the transcribed loops,
//                               alternated in one process, five pairs, SECONDS per leg; one JSON line per leg.
// Two statements of the reference cannot run on a keyframe without a camera-1 counter (pKFmax_cam1 is NULL at src/KeyFrame.cc:618,
// front() of an empty vector at :660); the transcribed rest skips them there, on both twins alike.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>
#include <memory>
#include <string>
#include <vector>
#include "../../include/orbm.h"
#include "Covisibility.h"

using namespace ORB_SLAM2;

namespace {

struct Rng {   // (one generator for both twins of a world: the twins are built from the same draws)
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 1) {}
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    int below(int n) { return (int)(next() % (uint32_t)n); }
    bool chance(int percent) { return below(100) < percent; }
};

struct World {
    int nk = 0, np = 0, nf = 0;
    std::unique_ptr<KeyFrame[]> kfs;      // contiguous: pointer order is index order, in both twins
    std::unique_ptr<MapPoint[]> pts;
    std::vector<CallLogEntry> log;
    std::vector<KeyFrame*> all_kfs() { std::vector<KeyFrame*> v; for (int k = 0; k < nk; ++k) v.push_back(&kfs[k]); return v; }
    std::vector<MapPoint*> all_pts() { std::vector<MapPoint*> v; for (int p = 0; p < np; ++p) v.push_back(&pts[p]); return v; }
};

void alloc(World& w, int nk, int np, int nf, int n_cam1) {
    w.nk = nk; w.np = np; w.nf = nf;
    w.kfs.reset(new KeyFrame[nk]); w.pts.reset(new MapPoint[np]);
    for (int k = 0; k < nk; ++k) {
        KeyFrame& kf = w.kfs[k];
        kf.mnId = k; kf.N = n_cam1; kf.N_total = nf; kf.mThDepth = 10.f;
        kf.mvpMapPoints.assign((size_t)nf, nullptr);
        kf.mvKeysUn_total.assign((size_t)nf, cv::KeyPoint()); kf.mvDepth_total.assign((size_t)nf, 1.f); kf.mvuRight_total.assign((size_t)nf, -1.f);
        for (int f = 0; f < nf; ++f) kf.mvKeysUn_total[(size_t)f].octave = 0;
    }
    for (int p = 0; p < np; ++p) {
        MapPoint& mp = w.pts[p];
        mp.mnId = p; mp.nObs = 0;
        mp.mWorldPos = cv::Mat(3, 1, CV_32F); mp.mNormalVector = cv::Mat(3, 1, CV_32F); mp.mDescriptor = cv::Mat(1, 32, CV_8U);
        for (int k = 0; k < 3; ++k) { mp.mWorldPos.at<float>(k) = (float)(p % 7 + k); mp.mNormalVector.at<float>(k) = 0.5f; }
        for (int k = 0; k < 32; ++k) mp.mDescriptor.ptr(0)[k] = (uint8_t)(p + k);
    }
}

// MapPoint::AddObservation with the reference's counter (src/MapPoint.cc:138-165) and KeyFrame::AddMapPoint
void observe(World& w, int p, int k, int idx) {
    MapPoint& mp = w.pts[p]; KeyFrame& kf = w.kfs[k];
    if (mp.mObservations.count(&kf)) return;
    mp.mObservations[&kf] = (size_t)idx;
    mp.nObs += kf.mvuRight_total[(size_t)idx] >= 0 ? 2 : 1;
    kf.mvpMapPoints[(size_t)idx] = &mp;
    if (!mp.mpRefKF) mp.mpRefKF = &kf;
}

// A seeded map: nk keyframes of nf features, the first n_cam1 of camera 1; np points seen by about `observers` keyframes each.
void build(World& w, uint64_t seed, int nk, int np, int nf, int observers, int max_level) {
    Rng r(seed);
    alloc(w, nk, np, nf, nf * 2 / 3);
    for (int k = 0; k < nk; ++k) {
        KeyFrame& kf = w.kfs[k];
        if (r.chance(15)) kf.N = r.chance(50) ? 0 : nf;      // a keyframe without camera-1 features, one with nothing else
        for (int f = 0; f < nf; ++f) {
            kf.mvKeysUn_total[(size_t)f].octave = r.below(max_level + 1);
            kf.mvDepth_total[(size_t)f] = r.chance(15) ? 12.f : (r.chance(5) ? -1.f : 1.f + (float)r.below(8));   // far, invalid, close
            kf.mvuRight_total[(size_t)f] = r.chance(40) ? 5.f : -1.f;                                              // stereo features count 2
        }
        if (k > 0 && r.chance(80)) { kf.mpParent = &w.kfs[r.below(k)]; kf.mpParent->mspChildrens.insert(&kf); kf.mbFirstConnection = false; }
        if (r.chance(10)) kf.mbNotErase = true;
    }
    for (int p = 0; p < np; ++p) {
        w.pts[p].mbBad = r.chance(6);
        const int n = std::max(0, observers - 2 + r.below(5));
        for (int o = 0; o < n; ++o) {
            const int k = r.below(nk), idx = r.below(nf);
            if (w.kfs[k].mvpMapPoints[(size_t)idx]) continue;
            observe(w, p, k, idx);
        }
    }
    for (int k = 0; k < nk; k += 3)                            // a keyframe row with the same point twice, one with a point that does not know of it
        for (int f = 0; f + 2 < nf; ++f)
            if (w.kfs[k].mvpMapPoints[(size_t)f] && !w.kfs[k].mvpMapPoints[(size_t)f + 1] && !w.kfs[k].mvpMapPoints[(size_t)f + 2]) {
                w.kfs[k].mvpMapPoints[(size_t)f + 1] = w.kfs[k].mvpMapPoints[(size_t)f];
                w.kfs[k].mvpMapPoints[(size_t)f + 2] = &w.pts[r.below(np)];
                break;
            }
}

// ---- the reference, transcribed onto the stand-in types ------------------------------------------------------------------------------
// src/KeyFrame.cc:512-552: the two counters, with their std::map copies
void ref_counters(KeyFrame* self, std::map<KeyFrame*, int>& KFcounter, std::map<KeyFrame*, int>& KFcounter_cam1) {
    std::vector<MapPoint*> vpMP = self->mvpMapPoints;
    std::vector<MapPoint*> vpMP_cam1;
    vpMP_cam1.resize((size_t)self->N);
    for (int i = 0; i < self->N; i++) vpMP_cam1[(size_t)i] = self->mvpMapPoints[(size_t)i];
    for (std::vector<MapPoint*>::iterator vit = vpMP.begin(), vend = vpMP.end(); vit != vend; vit++) {
        MapPoint* pMP = *vit;
        if (!pMP) continue;
        if (pMP->isBad()) continue;
        std::map<KeyFrame*, size_t> observations = pMP->GetObservations();
        for (std::map<KeyFrame*, size_t>::iterator mit = observations.begin(), mend = observations.end(); mit != mend; mit++) {
            if (mit->first->mnId == self->mnId) continue;
            KFcounter[mit->first]++;
        }
    }
    for (std::vector<MapPoint*>::iterator vit = vpMP_cam1.begin(), vend = vpMP_cam1.end(); vit != vend; vit++) {
        MapPoint* pMP_cam1 = *vit;
        if (!pMP_cam1) continue;
        if (pMP_cam1->isBad()) continue;
        std::map<KeyFrame*, size_t> observations_cam1 = pMP_cam1->GetObservations_cam1();
        for (std::map<KeyFrame*, size_t>::iterator mit = observations_cam1.begin(), mend = observations_cam1.end(); mit != mend; mit++) {
            if (mit->first->mnId == self->mnId) continue;
            KFcounter_cam1[mit->first]++;
        }
    }
}

// src/KeyFrame.cc:554-667: everything behind the counters, for both twins
void rest_of_update_connections(KeyFrame* self, std::map<KeyFrame*, int>& KFcounter, std::map<KeyFrame*, int>& KFcounter_cam1) {
    if (KFcounter.empty()) return;
    int nmax = 0; KeyFrame* pKFmax = NULL;
    int nmax_cam1 = 0; KeyFrame* pKFmax_cam1 = NULL;
    int th = 15;
    std::vector<std::pair<int, KeyFrame*> > vPairs, vPairs_cam1;
    vPairs.reserve(KFcounter.size()); vPairs_cam1.reserve(KFcounter_cam1.size());
    for (std::map<KeyFrame*, int>::iterator mit = KFcounter.begin(), mend = KFcounter.end(); mit != mend; mit++) {
        if (mit->second > nmax) { nmax = mit->second; pKFmax = mit->first; }
        if (mit->second >= th) { vPairs.push_back(std::make_pair(mit->second, mit->first)); (mit->first)->AddConnection(self, mit->second); }
    }
    for (std::map<KeyFrame*, int>::iterator mit = KFcounter_cam1.begin(), mend = KFcounter_cam1.end(); mit != mend; mit++) {
        if (mit->second > nmax_cam1) { nmax_cam1 = mit->second; pKFmax_cam1 = mit->first; }
        if (mit->second >= th) { vPairs_cam1.push_back(std::make_pair(mit->second, mit->first)); (mit->first)->AddConnection_cam1(self, mit->second); }
    }
    if (vPairs.empty()) { vPairs.push_back(std::make_pair(nmax, pKFmax)); pKFmax->AddConnection(self, nmax); }
    if (vPairs_cam1.empty() && pKFmax_cam1) { vPairs_cam1.push_back(std::make_pair(nmax_cam1, pKFmax_cam1)); pKFmax_cam1->AddConnection_cam1(self, nmax_cam1); }
    std::sort(vPairs.begin(), vPairs.end());
    std::sort(vPairs_cam1.begin(), vPairs_cam1.end());
    std::list<KeyFrame*> lKFs, lKFs_cam1; std::list<int> lWs, lWs_cam1;
    for (size_t i = 0; i < vPairs.size(); i++) { lKFs.push_front(vPairs[i].second); lWs.push_front(vPairs[i].first); }
    for (size_t i = 0; i < vPairs_cam1.size(); i++) { lKFs_cam1.push_front(vPairs_cam1[i].second); lWs_cam1.push_front(vPairs_cam1[i].first); }
    self->mConnectedKeyFrameWeights = KFcounter;
    self->mvpOrderedConnectedKeyFrames = std::vector<KeyFrame*>(lKFs.begin(), lKFs.end());
    self->mvOrderedWeights = std::vector<int>(lWs.begin(), lWs.end());
    self->mConnectedKeyFrameWeights_cam1 = KFcounter_cam1;
    self->mvpOrderedConnectedKeyFrames_cam1 = std::vector<KeyFrame*>(lKFs_cam1.begin(), lKFs_cam1.end());
    self->mvOrderedWeights_cam1 = std::vector<int>(lWs_cam1.begin(), lWs_cam1.end());
    if (self->mbFirstConnection && self->mnId != 0 && !self->mvpOrderedConnectedKeyFrames_cam1.empty()) {
        self->mpParent = self->mvpOrderedConnectedKeyFrames_cam1.front();
        self->mpParent->AddChild(self);
        self->mbFirstConnection = false;
    }
}

void ref_update_connections(KeyFrame* self) {
    std::map<KeyFrame*, int> KFcounter, KFcounter_cam1;
    ref_counters(self, KFcounter, KFcounter_cam1);
    rest_of_update_connections(self, KFcounter, KFcounter_cam1);
}

void class_update_connections(ResidentMap& R, KeyFrame* self) {
    std::map<KeyFrame*, int> KFcounter, KFcounter_cam1;
    CovisibilityCounts(R, self, KFcounter, KFcounter_cam1);
    rest_of_update_connections(self, KFcounter, KFcounter_cam1);
}

// src/LocalMapping.cc:983-1032 for one keyframe, with its std::map copies -> nMPs, nRedundantObservations
void ref_culling_counts(KeyFrame* pKF, bool mbMonocular, int& nMPs, int& nRedundantObservations) {
    const std::vector<MapPoint*> vpMapPoints = pKF->GetMapPointMatches();
    int nObs = 3;
    const int thObs = nObs;
    nRedundantObservations = 0; nMPs = 0;
    for (size_t i = 0, iend = vpMapPoints.size(); i < iend; i++) {
        MapPoint* pMP = vpMapPoints[i];
        if (pMP) {
            if (!pMP->isBad()) {
                if (!mbMonocular) {
                    if (pKF->mvDepth_total[i] > pKF->mThDepth || pKF->mvDepth_total[i] < 0) continue;
                }
                nMPs++;
                if (pMP->Observations() > thObs) {
                    const int& scaleLevel = pKF->mvKeysUn_total[i].octave;
                    const std::map<KeyFrame*, size_t> observations = pMP->GetObservations();
                    int nObs = 0;
                    for (std::map<KeyFrame*, size_t>::const_iterator mit = observations.begin(), mend = observations.end(); mit != mend; mit++) {
                        KeyFrame* pKFi = mit->first;
                        if (pKFi == pKF) continue;
                        const int& scaleLeveli = pKFi->mvKeysUn_total[mit->second].octave;
                        if (scaleLeveli <= scaleLevel + 1) {
                            nObs++;
                            if (nObs >= thObs) break;
                        }
                    }
                    if (nObs >= thObs) nRedundantObservations++;
                }
            }
        }
    }
}

void ref_keyframe_culling(KeyFrame* mpCurrentKeyFrame, bool mbMonocular) {   // src/LocalMapping.cc:966-1038
    std::vector<KeyFrame*> vpLocalKeyFrames = mpCurrentKeyFrame->GetVectorCovisibleKeyFrames();
    for (std::vector<KeyFrame*>::iterator vit = vpLocalKeyFrames.begin(), vend = vpLocalKeyFrames.end(); vit != vend; vit++) {
        KeyFrame* pKF = *vit;
        if (pKF->mnId == 0) continue;
        int nMPs, nRedundantObservations;
        ref_culling_counts(pKF, mbMonocular, nMPs, nRedundantObservations);
        if (nRedundantObservations > 0.90 * nMPs) pKF->SetBadFlag();
    }
}

// ---- comparison ----------------------------------------------------------------------------------------------------------------------
int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); ++fails; } } while (0)

int idx_of(World& w, KeyFrame* k) { return k ? (int)(k - w.kfs.get()) : -1; }
int idx_of(World& w, MapPoint* p) { return p ? (int)(p - w.pts.get()) : -1; }

std::string state_of(World& w) {   // everything the two routines may change, by index
    std::string s;
    char buf[64];
    auto put = [&](const char* tag, long v) { std::snprintf(buf, sizeof buf, "%s%ld ", tag, v); s += buf; };
    for (int k = 0; k < w.nk; ++k) {
        KeyFrame& kf = w.kfs[k];
        put("\nK", k); put("b", kf.mbBad); put("e", kf.mbToBeErased); put("f", kf.mbFirstConnection); put("p", idx_of(w, kf.mpParent));
        s += "w:"; for (auto& kv : kf.mConnectedKeyFrameWeights) { put("", idx_of(w, kv.first)); put("=", kv.second); }
        s += "o:"; for (KeyFrame* o : kf.mvpOrderedConnectedKeyFrames) put("", idx_of(w, o));
        s += "ow:"; for (int v : kf.mvOrderedWeights) put("", v);
        s += "w1:"; for (auto& kv : kf.mConnectedKeyFrameWeights_cam1) { put("", idx_of(w, kv.first)); put("=", kv.second); }
        s += "o1:"; for (KeyFrame* o : kf.mvpOrderedConnectedKeyFrames_cam1) put("", idx_of(w, o));
        s += "ow1:"; for (int v : kf.mvOrderedWeights_cam1) put("", v);
        s += "c:"; for (KeyFrame* o : kf.mspChildrens) put("", idx_of(w, o));
        s += "m:"; for (MapPoint* p : kf.mvpMapPoints) put("", idx_of(w, p));
    }
    for (int p = 0; p < w.np; ++p) {
        MapPoint& mp = w.pts[p];
        put("\nP", p); put("b", mp.mbBad); put("n", mp.nObs); put("r", idx_of(w, mp.mpRefKF));
        for (auto& ob : mp.mObservations) { put("", idx_of(w, ob.first)); put("@", (long)ob.second); }
    }
    s += "\nlog:";
    for (const CallLogEntry& e : w.log) { s += e.what; put(" ", (long)e.a); put(",", (long)e.b); }
    return s;
}

bool same_state(World& a, World& b, const char* what) {
    const std::string sa = state_of(a), sb = state_of(b);
    if (sa == sb) return true;
    size_t at = 0; while (at < sa.size() && at < sb.size() && sa[at] == sb[at]) ++at;
    const size_t from = at > 60 ? at - 60 : 0;
    std::printf("FAIL %s: the twins differ near\n  reference: ...%s\n  class:     ...%s\n", what, sa.substr(from, 140).c_str(), sb.substr(from, 140).c_str());
    ++fails;
    return false;
}

void touch_all(World& w, ResidentMap& R) { for (int k = 0; k < w.nk; ++k) R.Touch(&w.kfs[k]); for (int p = 0; p < w.np; ++p) R.Touch(&w.pts[p]); }

int audit(World& w, ResidentMap& R) { R.Flush(); return R.Audit(w.all_kfs(), w.all_pts()); }

ResidentMap::Capacity capacity_for(int nk, int np, int nf) {
    ResidentMap::Capacity c; c.keyframes = nk + 2; c.points = np + 2; c.observations = np * 12 + 16; c.features_per_keyframe = nf;
    return c;
}

// UpdateConnections for the keyframes of `order`, one by one, then all counters in one call against the one-by-one counters
int connections_case(ORBmatcher* matcher, const char* name, void (*make)(World&), const std::vector<int>& order) {
    World A, B;
    make(A); make(B);
    ResidentMap R(matcher, capacity_for(B.nk, B.np, B.nf));
    touch_all(B, R);
    CHECK(audit(B, R) == 0, "%s: Audit after the first Flush", name);
    // all the counters in one call, against the transcribed loops on the twin, before anything changes
    std::vector<KeyFrame*> listed; for (int k : order) listed.push_back(&B.kfs[k]);
    std::vector<std::map<KeyFrame*, int> > all, cam1;
    CovisibilityCounts(R, listed, all, cam1);
    long entries = 0;
    for (size_t j = 0; j < order.size(); ++j) {
        std::map<KeyFrame*, int> ra, r1;
        ref_counters(&A.kfs[order[j]], ra, r1);
        bool same = ra.size() == all[j].size() && r1.size() == cam1[j].size();
        for (auto& kv : ra) same = same && all[j].count(&B.kfs[idx_of(A, kv.first)]) && all[j][&B.kfs[idx_of(A, kv.first)]] == kv.second;
        for (auto& kv : r1) same = same && cam1[j].count(&B.kfs[idx_of(A, kv.first)]) && cam1[j][&B.kfs[idx_of(A, kv.first)]] == kv.second;
        for (auto& kv : all[j]) same = same && kv.second > 0;
        for (auto& kv : cam1[j]) same = same && kv.second > 0;
        CHECK(same, "%s: the counters of keyframe %d in the batched call", name, order[j]);
        entries += (long)ra.size();
    }
    CallLog() = &A.log; for (int k : order) ref_update_connections(&A.kfs[k]);
    CallLog() = &B.log; for (int k : order) class_update_connections(R, &B.kfs[k]);
    CallLog() = nullptr;
    same_state(A, B, name);
    CHECK(audit(B, R) == 0, "%s: Audit after UpdateConnections", name);
    std::printf("connections %s: %d keyframes updated, %ld counter entries, %d calls logged\n", name, (int)order.size(), entries, (int)A.log.size());
    return (int)A.log.size();
}

// KeyFrameCulling for keyframe `current` whose covisible list is `listed` -> the number of keyframes culled
int culling_case(ORBmatcher* matcher, const char* name, void (*make)(World&), int current, const std::vector<int>& listed, bool mono, int expect_culled = -1) {
    World A, B;
    make(A); make(B);
    for (World* w : {&A, &B}) { w->kfs[current].mvpOrderedConnectedKeyFrames.clear(); for (int k : listed) w->kfs[current].mvpOrderedConnectedKeyFrames.push_back(&w->kfs[k]); }
    ResidentMap R(matcher, capacity_for(B.nk, B.np, B.nf));
    touch_all(B, R);
    CHECK(audit(B, R) == 0, "%s: Audit after the first Flush", name);
    CallLog() = &A.log; ref_keyframe_culling(&A.kfs[current], mono);
    CallLog() = &B.log; KeyFrameCulling(R, &B.kfs[current], mono);
    CallLog() = nullptr;
    same_state(A, B, name);
    CHECK(audit(B, R) == 0, "%s: Audit after KeyFrameCulling", name);
    int culled = 0, refused = 0, tried = 0, bad_points = 0;
    for (int k : listed) { culled += A.kfs[k].mbBad && k != 0; refused += A.kfs[k].mbToBeErased; }
    for (const CallLogEntry& e : A.log) tried += std::strcmp(e.what, "SetBadFlag") == 0;
    for (int p = 0; p < A.np; ++p) bad_points += A.pts[p].mbBad;
    std::printf("culling %s: %d listed, %d SetBadFlag calls, %d refused, %d bad points afterwards\n", name, (int)listed.size(), tried, refused, bad_points);
    if (expect_culled >= 0) CHECK(tried - refused == expect_culled, "%s: %d keyframes culled, %d expected", name, tried - refused, expect_culled);
    return tried - refused;
}

// ---- worlds ---------------------------------------------------------------------------------------------------------------------------
void seeded_sparse(World& w) { build(w, 1, 30, 400, 96, 4, 7); }
void seeded_dense(World& w) { build(w, 2, 14, 300, 160, 7, 2); }
void seeded_wide(World& w) { build(w, 3, 60, 1500, 200, 6, 3); }
void seeded_redundant(World& w) { build(w, 4, 10, 200, 400, 9, 1); }   // most points seen by six keyframes at levels 0 and 1: keyframes go one after another
void seeded_redundant2(World& w) { build(w, 6, 12, 260, 400, 8, 1); }

// point p sits at feature p of every keyframe of sets[p]; mono features, level 0, close: nObs is the number of observers
void hand(World& w, int nk, const std::vector<std::vector<int> >& sets) {
    alloc(w, nk, (int)sets.size(), (int)sets.size(), (int)sets.size());
    for (size_t p = 0; p < sets.size(); ++p) for (int k : sets[p]) observe(w, (int)p, k, (int)p);
    for (int k = 1; k < nk; ++k) { w.kfs[k].mpParent = &w.kfs[0]; w.kfs[0].mspChildrens.insert(&w.kfs[k]); w.kfs[k].mbFirstConnection = false; }
}
std::vector<std::vector<int> > repeat(int n, const std::vector<int>& set) { return std::vector<std::vector<int> >((size_t)n, set); }

// keyframe 1 is the current one and lists 0 (skipped: mnId 0), 2, 3, 4.
void hand_none(World& w) { hand(w, 8, repeat(10, {2, 3, 4})); }                               // three observers: nObs 3, never examined
void hand_one(World& w) { auto s = repeat(10, {2, 5, 6, 7}); for (auto& x : repeat(10, {3, 4, 5})) s.push_back(x); hand(w, 8, s); }
void hand_two(World& w) { hand(w, 8, repeat(10, {2, 3, 0, 5, 6, 7})); }                       // 2 goes, five observers stay: 3 goes too; then 4 is empty
void hand_first_changes_second(World& w) { hand(w, 8, repeat(10, {2, 3, 6, 7})); }            // 2 goes, nObs drops to 3: 3 stays
void hand_not_erase(World& w) { hand(w, 8, repeat(10, {2, 3, 6, 7})); w.kfs[2].mbNotErase = true; }   // 2 is refused, nothing changed: 3 goes
void hand_points_go_bad(World& w) {   // 2 goes (20 of 22); points 20 and 21 drop to two observers, go bad and leave 3 empty; 4 goes (20 of 20)
    auto s = repeat(20, {2, 4, 5, 6, 7}); for (auto& x : repeat(2, {2, 3, 4})) s.push_back(x);
    hand(w, 8, s);
}
// the ninety-percent rule: keyframe 2 holds ten counted points, `red` of them seen by three others
template <int RED> void hand_ratio(World& w) {
    std::vector<std::vector<int> > s = repeat(RED, {2, 5, 6, 7});
    for (auto& x : repeat(10 - RED, {2, 5, 6})) s.push_back(x);
    hand(w, 8, s);
}
void hand_empty(World& w) { hand(w, 8, repeat(4, {5, 6, 7})); }                                // keyframe 2 holds nothing: 0 > 0.9 * 0 is false

int run_cases(ORBmatcher* matcher) {
    std::vector<int> every30, every14, some60;
    for (int k = 0; k < 30; ++k) every30.push_back(k);
    for (int k = 13; k >= 0; --k) every14.push_back(k);
    for (int k = 0; k < 60; k += 2) some60.push_back(k);
    int calls = 0;
    calls += connections_case(matcher, "sparse", seeded_sparse, every30);
    calls += connections_case(matcher, "dense", seeded_dense, every14);
    calls += connections_case(matcher, "wide", seeded_wide, some60);
    CHECK(calls > 100, "the seeded maps made %d AddConnection calls", calls);
    connections_case(matcher, "no observers", hand_empty, {2, 1});   // empty counters: UpdateConnections returns at once
    connections_case(matcher, "hand", hand_one, {2, 3, 5});

    int culled = 0;
    for (bool mono : {false, true}) {
        culled += culling_case(matcher, mono ? "sparse mono" : "sparse", seeded_sparse, 1, {0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12}, mono);
        culled += culling_case(matcher, mono ? "dense mono" : "dense", seeded_dense, 1, {0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13}, mono);
        culled += culling_case(matcher, mono ? "wide mono" : "wide", seeded_wide, 1, {5, 9, 2, 0, 30, 31, 32, 33, 34, 40, 41, 42, 50, 59}, mono);
        culled += culling_case(matcher, mono ? "redundant mono" : "redundant", seeded_redundant, 1, {0, 2, 3, 4, 5, 6, 7, 8, 9}, mono);
        culled += culling_case(matcher, mono ? "redundant2 mono" : "redundant2", seeded_redundant2, 1, {11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 0}, mono);
    }
    CHECK(culled >= 4, "the seeded maps culled %d keyframes", culled);
    culling_case(matcher, "none", hand_none, 1, {0, 2, 3, 4}, false, 0);
    culling_case(matcher, "one", hand_one, 1, {0, 2, 3, 4}, false, 1);
    culling_case(matcher, "two consecutive", hand_two, 1, {0, 2, 3, 4}, false, 2);
    culling_case(matcher, "first changes second", hand_first_changes_second, 1, {0, 2, 3, 4}, false, 1);
    culling_case(matcher, "not erase", hand_not_erase, 1, {0, 2, 3, 4}, false, 1);
    culling_case(matcher, "points go bad", hand_points_go_bad, 1, {0, 2, 3, 4}, false, 2);
    culling_case(matcher, "9 of 10", hand_ratio<9>, 1, {2}, false, 0);
    culling_case(matcher, "10 of 10", hand_ratio<10>, 1, {2}, false, 1);
    culling_case(matcher, "0 of 0", hand_empty, 1, {2}, false, 0);
    culling_case(matcher, "empty list", hand_one, 1, {}, false, 0);
    return fails;
}

int time_mode(int nk, int np, int observers, int n_listed, double seconds) {
    ORBmatcher matcher(0.8f, true);
    World w;
    const int nf = std::max(64, std::min<int>(ORBM_MAP_MAX_FEATURES, (int)((long long)np * observers * 4 / nk)));   // rows four times as long as they fill: few draws meet a taken feature
    build(w, 5, nk, np, nf, observers, 3);
    ResidentMap::Capacity c; c.keyframes = nk; c.points = np; c.observations = np * (observers + 3); c.features_per_keyframe = nf;
    ResidentMap R(&matcher, c);
    touch_all(w, R);
    if (R.Flush() < 0) return 1;
    long records = 0; for (int p = 0; p < np; ++p) records += (long)w.pts[p].mObservations.size();
    std::vector<KeyFrame*> listed; for (int j = 0; j < n_listed; ++j) listed.push_back(&w.kfs[1 + (j * 7) % (nk - 1)]);
    // the culling legs must leave the map as it is: every SetBadFlag is refused, so a leg is the counting and the verdicts alone
    for (int k = 0; k < nk; ++k) w.kfs[k].mbNotErase = true;
    w.kfs[0].mvpOrderedConnectedKeyFrames = listed;
    auto verdicts = [&] { long s = 0; for (KeyFrame* k : listed) { s += k->mbToBeErased; k->mbToBeErased = false; } return s; };
    std::vector<std::map<KeyFrame*, int> > all, cam1;
    auto leg = [&](const char* what, const char* route, int pair, auto&& body) {
        const auto t0 = std::chrono::steady_clock::now();
        int calls = 0; double el = 0; long sum = 0;
        do { sum += body(); ++calls; el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); } while (el < seconds);
        std::printf("{\"what\": \"%s\", \"route\": \"%s\", \"pair\": %d, \"keyframes\": %d, \"points\": %d, \"records\": %ld, \"listed\": %d, \"calls\": %d, \"ms_per_call\": %.4f, \"checksum\": %ld}\n",
                    what, route, pair, nk, np, records, n_listed, calls, 1e3 * el / calls, sum / calls);
    };
    for (int pair = 0; pair < 5; ++pair) {
        leg("covisibility", "class", pair, [&] { CovisibilityCounts(R, listed, all, cam1); long s = 0; for (auto& m : all) s += (long)m.size(); return s; });
        leg("covisibility", "transcription", pair, [&] { long s = 0; for (KeyFrame* k : listed) { std::map<KeyFrame*, int> a, b; ref_counters(k, a, b); s += (long)a.size(); } return s; });
        leg("culling", "class", pair, [&] { KeyFrameCulling(R, &w.kfs[0], false); return verdicts(); });
        leg("culling", "transcription", pair, [&] { ref_keyframe_culling(&w.kfs[0], false); return verdicts(); });
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "host") {
        const int f = run_cases(nullptr);
        if (f == 0) std::printf("covisibility host ok\n");
        return f ? 1 : 0;
    }
    if (mode == "device") {
        ORBmatcher matcher(0.8f, true);
        const int f = run_cases(&matcher);
        if (f == 0) std::printf("covisibility device ok\n");
        return f ? 1 : 0;
    }
    if (mode == "time" && argc == 7) return time_mode(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), std::atof(argv[6]));
    std::fprintf(stderr, "usage: test_covisibility host | device | time KEYFRAMES POINTS OBSERVERS LISTED SECONDS\n");
    return 2;
}
