// test_local_map.cc -- driver of ResidentMap / UpdateLocalMap / SearchLocalPoints (host/LocalMap.h) for tests/test_local_map_class.py
// and tools/local_map_bench.py.
//
//   test_local_map host                  no device: seeded stand-in maps (keyframes with point matches, a covisibility graph and a spanning
//                                        tree, points with observations, bad objects), three frames each with mutations and their Touch
//                                        calls in between; UpdateLocalMap over a host-only ResidentMap against a transcription of the
//                                        reference (src/Tracking.cc:1794-1949) on a twin of the map: vpLocalKeyFrames, vpLocalMapPoints,
//                                        the reference keyframe, F.mvpMapPoints and every mnTrackReferenceForFrame.  Then the hand-built
//                                        cases (more than 80 K1 keyframes, a tie for the most votes, a parent that ends the walk early --
//                                        and a transcription WITHOUT the outer break, which must differ there --, neighbour lists whose
//                                        first nine or ten entries are marked or bad, no votes at all) and Audit.
//   test_local_map device                the same with a third twin whose ResidentMap lives on the device: it must equal the host-only one.
//   test_local_map search WORLD.bin      a world of tests/frustum_worlds.py (layout: host/test_local_points.cc): its points spread over
//                                        keyframes of 2 000; UpdateLocalMap + SearchLocalPoints over the resident map against the
//                                        transcription + the existing SearchLocalPoints(matcher, F, points, th), on two frames.
//   test_local_map time WORLD.bin SECONDS  those two routes alternated in one process, five pairs, SECONDS per leg; one JSON line per leg.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "../../include/orbm.h"
#include "LocalMap.h"
#include "LocalMapSearch.h"

using namespace ORB_SLAM2;

namespace {

struct Rng {   // (one generator for every twin of a world: the twins are built from the same draws)
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 1) {}
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    int below(int n) { return (int)(next() % (uint32_t)n); }
    bool chance(int percent) { return below(100) < percent; }
    float unit() { return (float)(next() & 0xffff) / 65536.0f; }
};

struct World {
    int nk = 0, np = 0, nf = 0;
    std::unique_ptr<KeyFrame[]> kfs;      // contiguous: pointer order is index order, in every twin
    std::unique_ptr<MapPoint[]> pts;
    Frame F;
    std::vector<KeyFrame*> local; std::vector<MapPoint*> lpts; KeyFrame* ref = nullptr;
    std::vector<KeyFrame*> all_kfs() { std::vector<KeyFrame*> v; for (int k = 0; k < nk; ++k) v.push_back(&kfs[k]); return v; }
    std::vector<MapPoint*> all_pts() { std::vector<MapPoint*> v; for (int p = 0; p < np; ++p) v.push_back(&pts[p]); return v; }
};

void fill_point(MapPoint& mp, Rng& r) {
    mp.mWorldPos = cv::Mat(3, 1, CV_32F); mp.mNormalVector = cv::Mat(3, 1, CV_32F); mp.mDescriptor = cv::Mat(1, 32, CV_8U);
    for (int k = 0; k < 3; ++k) { mp.mWorldPos.at<float>(k) = r.unit() * 10.f; mp.mNormalVector.at<float>(k) = r.unit(); }
    for (int k = 0; k < 32; ++k) mp.mDescriptor.ptr(0)[k] = (uint8_t)r.next();
    mp.mfMinDistance = 1.f + r.unit(); mp.mfMaxDistance = 10.f + r.unit(); mp.nObs = 0;
}

void alloc(World& w, int nk, int np, int nf) {
    w.nk = nk; w.np = np; w.nf = nf;
    w.kfs.reset(new KeyFrame[nk]); w.pts.reset(new MapPoint[np]);
    for (int k = 0; k < nk; ++k) { w.kfs[k].mnId = k; w.kfs[k].N_total = nf; w.kfs[k].mvpMapPoints.assign((size_t)nf, nullptr); }
    w.F.mvpMapPoints.clear(); w.F.N_total = 0;
}

void observe(World& w, int p, int k, int idx) { w.pts[p].AddObservation(&w.kfs[k], (size_t)idx); w.kfs[k].mvpMapPoints[(size_t)idx] = &w.pts[p]; }

void build(World& w, uint64_t seed, int nk, int np, int nf) {
    Rng r(seed);
    alloc(w, nk, np, nf);
    for (int p = 0; p < np; ++p) { fill_point(w.pts[p], r); w.pts[p].mnId = p; w.pts[p].mbBad = r.chance(8); }
    for (int k = 0; k < nk; ++k) w.kfs[k].mbBad = r.chance(10);
    for (int p = 0; p < np; ++p) {
        const int n_obs = p % 17 == 5 ? 0 : 1 + r.below(8);   // (some points nobody observes)
        for (int o = 0; o < n_obs; ++o) {
            const int k = r.below(nk), idx = r.below(nf);
            if (w.kfs[k].mvpMapPoints[(size_t)idx] || w.pts[p].IsInKeyFrame(&w.kfs[k])) continue;
            observe(w, p, k, idx);
        }
    }
    for (int k = 0; k < nk; k += 3)                            // a keyframe row with the same point twice
        for (int f = 0; f + 1 < nf; ++f)
            if (w.kfs[k].mvpMapPoints[(size_t)f] && !w.kfs[k].mvpMapPoints[(size_t)f + 1]) { w.kfs[k].mvpMapPoints[(size_t)f + 1] = w.kfs[k].mvpMapPoints[(size_t)f]; break; }
    for (int k = 0; k < nk; ++k) {                             // the graph: ordered neighbours, children, a parent
        KeyFrame& kf = w.kfs[k];
        for (int j = 0, n = r.below(14); j < n; ++j) { const int o = r.below(nk); if (o != k) kf.mvpOrderedConnectedKeyFrames.push_back(&w.kfs[o]); }
        for (int j = 0, n = r.below(3); j < n; ++j) { const int o = r.below(nk); if (o != k) kf.mspChildrens.insert(&w.kfs[o]); }
        if (k > 0 && r.chance(70)) kf.mpParent = &w.kfs[r.below(k)];
    }
}

void set_frame(World& w, uint64_t seed, long unsigned int id, int n_features) {
    Rng r(seed);
    w.F.mnId = id; w.F.N_total = n_features;
    w.F.mvpMapPoints.assign((size_t)n_features, nullptr);
    for (int i = 0; i < n_features; ++i) if (r.chance(60)) w.F.mvpMapPoints[(size_t)i] = &w.pts[r.below(w.np)];
    if (n_features >= 2) w.F.mvpMapPoints[(size_t)n_features - 1] = w.F.mvpMapPoints[0];   // a point at two features
}

// what the mapping and loop-closing threads do between two frames; `R` (may be NULL) is told of every object that changed
void mutate(World& w, uint64_t seed, ResidentMap* R) {
    Rng r(seed);
    auto tp = [&](MapPoint* p) { if (R) R->Touch(p); };
    auto tk = [&](KeyFrame* k) { if (R) R->Touch(k); };
    for (int i = 0; i < w.np / 20 + 1; ++i) { MapPoint& p = w.pts[r.below(w.np)]; p.mbBad = true; tp(&p); }                                   // SetBadFlag
    for (int i = 0; i < w.np / 20 + 1; ++i) { MapPoint& p = w.pts[r.below(w.np)]; p.mWorldPos.at<float>(1) += 0.5f; tp(&p); }                // SetWorldPos
    for (int i = 0; i < w.np / 10 + 1; ++i) {                                                                                                  // EraseObservation + EraseMapPointMatch
        MapPoint& p = w.pts[r.below(w.np)];
        if (p.mObservations.empty()) continue;
        KeyFrame* k = p.mObservations.begin()->first; const size_t idx = p.mObservations.begin()->second;
        p.EraseObservationImpl(k); if (k->mvpMapPoints[idx] == &p) k->mvpMapPoints[idx] = nullptr;
        tp(&p); tk(k);
    }
    for (int i = 0; i < w.np / 10 + 1; ++i) {                                                                                                  // AddObservation + AddMapPoint
        const int p = r.below(w.np), k = r.below(w.nk), idx = r.below(w.nf);
        if (w.kfs[k].mvpMapPoints[(size_t)idx] || w.pts[p].IsInKeyFrame(&w.kfs[k])) continue;
        observe(w, p, k, idx); tp(&w.pts[p]); tk(&w.kfs[k]);
    }
    { KeyFrame& k = w.kfs[r.below(w.nk)]; k.mbBad = true; tk(&k); }                                                                            // KeyFrame::SetBadFlag
}

// ---- the reference, transcribed onto the stand-in types (src/Tracking.cc:1832-1949, :1794-1824) -------------------------------------
void ref_update_local_keyframes(World& w, bool outer_break = true) {
    Frame& mCurrentFrame = w.F; std::vector<KeyFrame*>& mvpLocalKeyFrames = w.local;
    std::map<KeyFrame*, int> keyframeCounter;
    for (int i = 0; i < mCurrentFrame.N_total; i++) {
        if (mCurrentFrame.mvpMapPoints[i]) {
            MapPoint* pMP = mCurrentFrame.mvpMapPoints[i];
            if (!pMP->isBad()) {
                const std::map<KeyFrame*, size_t> observations = pMP->GetObservations();
                for (std::map<KeyFrame*, size_t>::const_iterator it = observations.begin(), itend = observations.end(); it != itend; it++)
                    keyframeCounter[it->first]++;
            } else {
                mCurrentFrame.mvpMapPoints[i] = NULL;
            }
        }
    }
    if (keyframeCounter.empty()) return;
    int max = 0;
    KeyFrame* pKFmax = static_cast<KeyFrame*>(NULL);
    mvpLocalKeyFrames.clear();
    mvpLocalKeyFrames.reserve(3 * keyframeCounter.size());
    for (std::map<KeyFrame*, int>::const_iterator it = keyframeCounter.begin(), itEnd = keyframeCounter.end(); it != itEnd; it++) {
        KeyFrame* pKF = it->first;
        if (pKF->isBad()) continue;
        if (it->second > max) { max = it->second; pKFmax = pKF; }
        mvpLocalKeyFrames.push_back(it->first);
        pKF->mnTrackReferenceForFrame = mCurrentFrame.mnId;
    }
    for (std::vector<KeyFrame*>::const_iterator itKF = mvpLocalKeyFrames.begin(), itEndKF = mvpLocalKeyFrames.end(); itKF != itEndKF; itKF++) {
        if (mvpLocalKeyFrames.size() > 80) break;
        KeyFrame* pKF = *itKF;
        const std::vector<KeyFrame*> vNeighs = pKF->GetBestCovisibilityKeyFrames(10);
        for (std::vector<KeyFrame*>::const_iterator itNeighKF = vNeighs.begin(), itEndNeighKF = vNeighs.end(); itNeighKF != itEndNeighKF; itNeighKF++) {
            KeyFrame* pNeighKF = *itNeighKF;
            if (!pNeighKF->isBad()) {
                if (pNeighKF->mnTrackReferenceForFrame != mCurrentFrame.mnId) {
                    mvpLocalKeyFrames.push_back(pNeighKF);
                    pNeighKF->mnTrackReferenceForFrame = mCurrentFrame.mnId;
                    break;
                }
            }
        }
        const std::set<KeyFrame*> spChilds = pKF->GetChilds();
        for (std::set<KeyFrame*>::const_iterator sit = spChilds.begin(), send = spChilds.end(); sit != send; sit++) {
            KeyFrame* pChildKF = *sit;
            if (!pChildKF->isBad()) {
                if (pChildKF->mnTrackReferenceForFrame != mCurrentFrame.mnId) {
                    mvpLocalKeyFrames.push_back(pChildKF);
                    pChildKF->mnTrackReferenceForFrame = mCurrentFrame.mnId;
                    break;
                }
            }
        }
        KeyFrame* pParent = pKF->GetParent();
        if (pParent) {
            if (pParent->mnTrackReferenceForFrame != mCurrentFrame.mnId) {
                mvpLocalKeyFrames.push_back(pParent);
                pParent->mnTrackReferenceForFrame = mCurrentFrame.mnId;
                if (outer_break) break;
            }
        }
    }
    if (pKFmax) { w.ref = pKFmax; mCurrentFrame.mpReferenceKF = w.ref; }
}

void ref_update_local_points(World& w) {
    w.lpts.clear();
    for (std::vector<KeyFrame*>::const_iterator itKF = w.local.begin(), itEndKF = w.local.end(); itKF != itEndKF; itKF++) {
        KeyFrame* pKF = *itKF;
        const std::vector<MapPoint*> vpMPs = pKF->GetMapPointMatches();
        for (std::vector<MapPoint*>::const_iterator itMP = vpMPs.begin(), itEndMP = vpMPs.end(); itMP != itEndMP; itMP++) {
            MapPoint* pMP = *itMP;
            if (!pMP) continue;
            if (pMP->mnTrackReferenceForFrame == w.F.mnId) continue;
            if (!pMP->isBad()) { w.lpts.push_back(pMP); pMP->mnTrackReferenceForFrame = w.F.mnId; }
        }
    }
}

void ref_update_local_map(World& w, bool outer_break = true) { ref_update_local_keyframes(w, outer_break); ref_update_local_points(w); }

// everything UpdateLocalMap may change, twin against twin, by index
int compare(World& a, World& b, const char* what) {
    int bad = 0;
    auto ik = [](World& w, KeyFrame* k) { return k ? (long)(k - w.kfs.get()) : -1L; };
    auto ip = [](World& w, MapPoint* p) { return p ? (long)(p - w.pts.get()) : -1L; };
    if (a.local.size() != b.local.size()) { fprintf(stderr, "%s: %zu / %zu local keyframes\n", what, a.local.size(), b.local.size()); ++bad; }
    else for (size_t i = 0; i < a.local.size(); ++i)
        if (ik(a, a.local[i]) != ik(b, b.local[i]) && bad++ < 10) fprintf(stderr, "%s: local keyframe %zu is %ld / %ld\n", what, i, ik(a, a.local[i]), ik(b, b.local[i]));
    if (a.lpts.size() != b.lpts.size()) { fprintf(stderr, "%s: %zu / %zu local points\n", what, a.lpts.size(), b.lpts.size()); ++bad; }
    else for (size_t i = 0; i < a.lpts.size(); ++i)
        if (ip(a, a.lpts[i]) != ip(b, b.lpts[i]) && bad++ < 10) fprintf(stderr, "%s: local point %zu is %ld / %ld\n", what, i, ip(a, a.lpts[i]), ip(b, b.lpts[i]));
    if (ik(a, a.ref) != ik(b, b.ref) || ik(a, a.F.mpReferenceKF) != ik(b, b.F.mpReferenceKF)) { fprintf(stderr, "%s: reference keyframe %ld / %ld\n", what, ik(a, a.ref), ik(b, b.ref)); ++bad; }
    for (int k = 0; k < a.nk; ++k)
        if (a.kfs[k].mnTrackReferenceForFrame != b.kfs[k].mnTrackReferenceForFrame && bad++ < 10) fprintf(stderr, "%s: mark of keyframe %d is %lu / %lu\n", what, k, a.kfs[k].mnTrackReferenceForFrame, b.kfs[k].mnTrackReferenceForFrame);
    for (int p = 0; p < a.np; ++p)
        if (a.pts[p].mnTrackReferenceForFrame != b.pts[p].mnTrackReferenceForFrame && bad++ < 10) fprintf(stderr, "%s: mark of point %d is %lu / %lu\n", what, p, a.pts[p].mnTrackReferenceForFrame, b.pts[p].mnTrackReferenceForFrame);
    for (size_t g = 0; g < a.F.mvpMapPoints.size(); ++g)
        if (ip(a, a.F.mvpMapPoints[g]) != ip(b, b.F.mvpMapPoints[g]) && bad++ < 10) fprintf(stderr, "%s: feature %zu holds point %ld / %ld\n", what, g, ip(a, a.F.mvpMapPoints[g]), ip(b, b.F.mvpMapPoints[g]));
    return bad;
}

ResidentMap::Capacity small_capacity(int nf) { ResidentMap::Capacity c; c.keyframes = 512; c.points = 20000; c.observations = 200000; c.features_per_keyframe = nf; return c; }

struct Routes {   // the twins of one world: T the transcription, H a host-only resident map, D (device mode) one on the device
    World T, H, D;
    std::unique_ptr<ResidentMap> RH, RD;
    bool device;
    Routes(ORBmatcher* m, int nf) : device(m != nullptr) {
        RH.reset(new ResidentMap(nullptr, small_capacity(nf)));
        if (m) RD.reset(new ResidentMap(m, small_capacity(nf)));
    }
    template <class Fn> void each(Fn fn) { fn(T, (ResidentMap*)nullptr); fn(H, RH.get()); if (device) fn(D, RD.get()); }
    void touch_all() {
        each([](World& w, ResidentMap* R) { if (!R) return; for (int k = 0; k < w.nk; ++k) R->Touch(&w.kfs[k]); for (int p = 0; p < w.np; ++p) R->Touch(&w.pts[p]); });
    }
    int step(const char* what, bool outer_break = true) {
        ref_update_local_map(T, outer_break);
        UpdateLocalMap(*RH, H.F, H.local, H.lpts, H.ref);
        int bad = compare(T, H, what);
        if (device) {
            UpdateLocalMap(*RD, D.F, D.local, D.lpts, D.ref);
            bad += compare(H, D, (std::string(what) + " (device against host-only)").c_str());
        }
        return bad;
    }
};

int run_random(ORBmatcher* m, uint64_t seed, int nk, int np, int nf, int n_frame) {
    Routes R(m, nf);
    R.each([&](World& w, ResidentMap*) { build(w, seed, nk, np, nf); });
    R.touch_all();
    int bad = 0; size_t kept = 0, kfs = 0;
    for (int t = 0; t < 3; ++t) {
        R.each([&](World& w, ResidentMap*) { set_frame(w, seed * 10 + t, 100 + t, n_frame); });
        char what[64]; snprintf(what, sizeof what, "world %d frame %d", (int)seed, t);
        bad += R.step(what);
        kept += R.T.lpts.size(); kfs += R.T.local.size();
        bad += R.RH->Audit(R.H.all_kfs(), R.H.all_pts());
        R.each([&](World& w, ResidentMap* rm) { mutate(w, seed * 100 + t, rm); });
    }
    if (kept == 0 || kfs == 0) { fprintf(stderr, "world %d: nothing was listed\n", (int)seed); ++bad; }
    printf("world %d: %d keyframes, %d points, 3 frames -> %zu local keyframes, %zu local points in all\n", (int)seed, nk, np, kfs, kept);
    return bad;
}

// ---- hand-built cases ------------------------------------------------------------------------------------------------------------------
void plain(World& w, int nk, int np, int nf) {
    alloc(w, nk, np, nf);
    Rng r(7);
    for (int p = 0; p < np; ++p) { fill_point(w.pts[p], r); w.pts[p].mnId = p; }
}
void frame_of(World& w, std::initializer_list<int> points, long unsigned int id) {
    w.F.mnId = id; w.F.mvpMapPoints.clear();
    for (int p : points) w.F.mvpMapPoints.push_back(p < 0 ? nullptr : &w.pts[p]);
    w.F.N_total = (int)w.F.mvpMapPoints.size();
}
std::vector<long> indices(World& w) { std::vector<long> v; for (KeyFrame* k : w.local) v.push_back((long)(k - w.kfs.get())); return v; }
bool expect(World& w, std::vector<long> local, long ref, const char* what) {
    const std::vector<long> got = indices(w);
    const long r = w.ref ? (long)(w.ref - w.kfs.get()) : -1;
    if (got == local && r == ref) return true;
    fprintf(stderr, "%s: local keyframes", what); for (long k : got) fprintf(stderr, " %ld", k);
    fprintf(stderr, " (reference %ld), expected", r); for (long k : local) fprintf(stderr, " %ld", k);
    fprintf(stderr, " (reference %ld)\n", ref);
    return false;
}

int run_cases(ORBmatcher* m) {
    int bad = 0;
    {   // more than 80 K1 keyframes: K2 never starts
        Routes R(m, 4);
        R.each([](World& w, ResidentMap*) {
            plain(w, 100, 3, 4);
            for (int k = 0; k < 90; ++k) { observe(w, 0, k, 0); w.kfs[k].mvpOrderedConnectedKeyFrames.push_back(&w.kfs[95]); w.kfs[k].mpParent = &w.kfs[96]; }
            observe(w, 1, 95, 1);
            frame_of(w, {0, -1, 2}, 5);
        });
        R.touch_all();
        bad += R.step("more than 80 K1 keyframes");
        std::vector<long> k1; for (long k = 0; k < 90; ++k) k1.push_back(k);
        bad += !expect(R.H, k1, 0, "more than 80 K1 keyframes");
        if (R.H.lpts.size() != 1) { fprintf(stderr, "more than 80 K1 keyframes: %zu local points\n", R.H.lpts.size()); ++bad; }
    }
    {   // a tie for the most votes: the strict > keeps the first in pointer order; a bad keyframe with more votes does not count
        Routes R(m, 4);
        R.each([](World& w, ResidentMap*) {
            plain(w, 8, 6, 4);
            for (int p = 0; p < 3; ++p) { observe(w, p, 5, p); observe(w, p, 2, p); observe(w, p, 6, p); }
            observe(w, 3, 6, 3); w.kfs[6].mbBad = true;
            observe(w, 4, 1, 0);
            frame_of(w, {0, 1, 2, 3, 4}, 5);
        });
        R.touch_all();
        bad += R.step("tie");
        bad += !expect(R.H, {1, 2, 5}, 2, "tie");
    }
    {   // a parent that ends the walk early: the break in the parent branch leaves the OUTER loop
        Routes R(m, 4), N(nullptr, 4);
        auto make = [](World& w, ResidentMap*) {
            plain(w, 8, 3, 4);
            observe(w, 0, 1, 0); observe(w, 0, 2, 0); observe(w, 1, 2, 1);
            w.kfs[1].mvpOrderedConnectedKeyFrames = {&w.kfs[4]}; w.kfs[1].mpParent = &w.kfs[7];
            w.kfs[2].mvpOrderedConnectedKeyFrames = {&w.kfs[5]}; w.kfs[2].mspChildrens = {&w.kfs[6]};
            frame_of(w, {0, 1}, 5);
        };
        R.each(make); N.each(make);
        R.touch_all();
        bad += R.step("parent ends the walk");
        bad += !expect(R.H, {1, 2, 4, 7}, 2, "parent ends the walk");
        ref_update_local_map(N.T, /*outer_break=*/false);      // the walk as it would be without the outer break: a different list
        bad += !expect(N.T, {1, 2, 4, 7, 5, 6}, 2, "parent ends the walk, transcription without the outer break");
        if (indices(N.T) == indices(R.H)) { fprintf(stderr, "the outer break decides nothing in its own case\n"); ++bad; }
    }
    for (int variant = 0; variant < 2; ++variant) {   // a neighbour list whose first nine (variant 1: ten) entries are marked or bad
        Routes R(m, 4);
        R.each([variant](World& w, ResidentMap*) {
            plain(w, 20, 3, 4);
            for (int k = 1; k <= 5; ++k) observe(w, 0, k, 0);                     // K1 = 1 .. 5
            for (int k = 6; k <= 9; ++k) w.kfs[k].mbBad = true;
            std::vector<KeyFrame*>& nb = w.kfs[1].mvpOrderedConnectedKeyFrames;
            for (int k : {2, 6, 3, 7, 4, 8, 5, 9, 2}) nb.push_back(&w.kfs[k]);  // nine entries: marked (in K1) or bad
            nb.push_back(&w.kfs[variant ? 3 : 12]);                               // the tenth: good and unmarked, or marked as well
            nb.push_back(&w.kfs[13]);                                             // the eleventh is never looked at
            frame_of(w, {0}, 5);
        });
        R.touch_all();
        bad += R.step("nine marked or bad neighbours");
        bad += !expect(R.H, variant ? std::vector<long>{1, 2, 3, 4, 5} : std::vector<long>{1, 2, 3, 4, 5, 12}, 1, "nine marked or bad neighbours");
    }
    {   // no votes at all: the keyframes and the reference stay, the point list is rebuilt from them
        Routes R(m, 4);
        R.each([](World& w, ResidentMap*) {
            plain(w, 6, 5, 4);
            observe(w, 0, 1, 0); observe(w, 1, 3, 0); observe(w, 2, 3, 1);
            w.pts[4].mbBad = true;
            frame_of(w, {0}, 5);
        });
        R.touch_all();
        bad += R.step("votes");
        bad += !expect(R.H, {1}, 1, "votes");
        R.each([](World& w, ResidentMap*) { w.local = {&w.kfs[3], &w.kfs[1]}; frame_of(w, {-1, 4, 3, -1}, 6); });   // a bad point, an unobserved one
        bad += R.step("no votes at all");
        bad += !expect(R.H, {3, 1}, 1, "no votes at all");
        if (R.H.lpts.size() != 3 || R.H.F.mvpMapPoints[1] != nullptr) { fprintf(stderr, "no votes at all: %zu local points\n", R.H.lpts.size()); ++bad; }
        R.each([](World& w, ResidentMap*) { frame_of(w, {}, 7); });                                                    // an empty frame
        bad += R.step("empty frame");
    }
    return bad;
}

int run_audit(ORBmatcher* m) {
    int bad = 0;
    World w; build(w, 3, 30, 400, 40);
    ResidentMap R(m, small_capacity(40));
    const std::vector<KeyFrame*> kfs = w.all_kfs(); const std::vector<MapPoint*> pts = w.all_pts();
    auto want = [&](bool zero, const char* what) {
        const int d = R.Audit(kfs, pts);
        if ((d == 0) != zero) { fprintf(stderr, "audit %s: %d differences\n", what, d); ++bad; }
    };
    want(false, "before anything was touched");
    for (KeyFrame* k : kfs) R.Touch(k);
    for (MapPoint* p : pts) R.Touch(p);
    if (R.Flush() <= 0) { fprintf(stderr, "the first Flush sent nothing\n"); ++bad; }
    want(true, "after the first Flush");
    if (R.Flush() != 0) { fprintf(stderr, "a Flush with nothing queued sent something\n"); ++bad; }
    for (MapPoint* p : pts) R.Touch(p);                          // touched, unchanged: nothing travels
    if (R.Flush() != 0) { fprintf(stderr, "unchanged objects were sent again\n"); ++bad; }
    // one mutation of each kind without its Touch, then with it
    MapPoint* moved = pts[3]; moved->mWorldPos.at<float>(0) += 1.f;
    want(false, "after SetWorldPos without a Touch"); R.Touch(moved); R.Flush(); want(true, "after its Touch");
    if (R.LastFlush().rows != 1 || R.LastFlush().records != 0) { fprintf(stderr, "one moved point sent %d rows, %d records\n", R.LastFlush().rows, R.LastFlush().records); ++bad; }
    MapPoint* gone = pts[4]; gone->mbBad = true;
    want(false, "after SetBadFlag without a Touch"); R.Touch(gone); R.Flush(); want(true, "after its Touch");
    MapPoint* seen = nullptr; for (MapPoint* p : pts) if (!p->mObservations.empty()) { seen = p; break; }
    KeyFrame* by = seen->mObservations.begin()->first; const size_t idx = seen->mObservations.begin()->second;
    seen->EraseObservationImpl(by); by->mvpMapPoints[idx] = nullptr;
    want(false, "after EraseObservation without a Touch"); R.Touch(seen); R.Flush();
    want(false, "with the keyframe's Touch still owed"); R.Touch(by); R.Flush(); want(true, "after both");
    seen->AddObservation(by, idx); by->mvpMapPoints[idx] = seen;
    want(false, "after AddObservation without a Touch"); R.Touch(seen); R.Touch(by); R.Flush(); want(true, "after its Touches");
    if (R.LastFlush().records != 1 || R.LastFlush().keyframes != 1) { fprintf(stderr, "one observation sent %d records, %d keyframes\n", R.LastFlush().records, R.LastFlush().keyframes); ++bad; }
    kfs[2]->mbBad = !kfs[2]->mbBad;
    want(false, "after KeyFrame::SetBadFlag without a Touch"); R.Touch(kfs[2]); R.Flush(); want(true, "after its Touch");
    return bad;
}

int run_all(bool device) {
    std::unique_ptr<ORBmatcher> m;
    if (device) m.reset(new ORBmatcher(0.8f));
    const unsigned long fails = ORBmatcher::FailureCount();
    int bad = 0;
    bad += run_random(m.get(), 1, 40, 600, 64, 200);
    bad += run_random(m.get(), 2, 120, 3000, 300, 1000);
    bad += run_random(m.get(), 3, 5, 30, 8, 12);
    bad += run_cases(m.get());
    bad += run_audit(m.get());
    if (ORBmatcher::FailureCount() != fails) { fprintf(stderr, "a device call failed: %s\n", ORBmatcher::LastError()); return 3; }
    if (bad) { fprintf(stderr, "%d differences\n", bad); return 1; }
    printf("local_map %s ok\n", device ? "device" : "host");
    return 0;
}

// ---- a searchable world (tests/frustum_worlds.py; layout in host/test_local_points.cc) ---------------------------------------------
struct SearchWorld {
    Frame F;
    std::vector<MapPoint> pts; std::vector<MapPoint*> vp;
    std::unique_ptr<KeyFrame[]> kfs; int nk = 0;
    std::vector<std::pair<int, int>> pre;
    float th = 3;
    std::vector<KeyFrame*> local; std::vector<MapPoint*> lpts; KeyFrame* ref = nullptr;
    void place() { F.mvpMapPoints.assign(F.N_total, nullptr); for (auto& p : pre) F.mvpMapPoints[p.first] = &pts[p.second]; }
};

bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
template <class T> bool rdv(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return rd(f, v.data(), n * sizeof(T)); }

bool load(const char* path, SearchWorld& w) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return false; }
    int32_t h[5];
    if (!rd(f, h, sizeof h) || h[0] != 0x4C505731 || h[1] < 0 || h[2] < 0 || h[3] < 0 || h[4] < 0) { fprintf(stderr, "bad header\n"); fclose(f); return false; }
    Frame& F = w.F;
    F.N = h[1]; F.N_cam2 = h[2]; F.N_total = F.N + F.N_cam2;
    const int n = F.N_total, npts = h[3], npre = h[4];
    std::vector<float> x, y, ang, ur; std::vector<int32_t> oct;
    bool ok = rdv(f, x, n) && rdv(f, y, n) && rdv(f, ang, n) && rdv(f, ur, n) && rdv(f, oct, n);
    F.mvKeys_total.resize(n); F.mvKeysUn_total.resize(n); F.mvuRight_total = ur;
    for (int g = 0; ok && g < n; ++g) {
        cv::KeyPoint k; k.pt.x = x[g]; k.pt.y = y[g]; k.angle = ang[g]; k.octave = oct[g];
        F.mvKeys_total[g] = k; F.mvKeysUn_total[g] = k;
        F.keypoint_to_cam[g] = g < F.N ? 0 : 1;
        F.cont_idx_to_local_cam_idx[g] = g < F.N ? g : g - F.N;
    }
    F.mvKeysUn.assign(F.mvKeysUn_total.begin(), F.mvKeysUn_total.begin() + F.N);
    F.mvKeys = F.mvKeysUn;
    F.mvuRight.assign(ur.begin(), ur.begin() + F.N);
    F.mDescriptors_total.resize(2);
    for (int c = 0; ok && c < 2; ++c) {
        const int nc = c == 0 ? F.N : F.N_cam2;
        F.mDescriptors_total[c].create(nc > 0 ? nc : 1, 32, CV_8U);
        ok = rd(f, F.mDescriptors_total[c].ptr(0), (size_t)nc * 32);
    }
    F.mDescriptors = F.mDescriptors_total[0];
    F.mvbOutlier.assign(n, false);
    float T[16], c[11];
    ok = ok && rdv(f, F.mvScaleFactors, 8) && rd(f, T, sizeof T) && rd(f, c, sizeof c);
    if (!ok) { fclose(f); return false; }
    cv::Mat Tcw = cv::Mat::eye(4, 4, CV_32F);
    for (int i = 0; i < 16; ++i) Tcw.at<float>(i / 4, i % 4) = T[i];
    F.SetPose(Tcw);
    F.fx = c[0]; F.fy = c[1]; F.cx = c[2]; F.cy = c[3]; F.mbf = c[4]; F.mb = F.mbf / F.fx;
    F.mnMinX = c[5]; F.mnMinY = c[6]; F.mnMaxX = c[7]; F.mnMaxY = c[8];
    F.mfLogScaleFactor = c[9]; F.mnScaleLevels = 8; w.th = c[10];
    w.pts.resize(npts); w.vp.resize(npts);
    for (int i = 0; i < npts; ++i) {
        orbm_point p; int32_t bad;
        if (!rd(f, &p, sizeof p) || !rd(f, &bad, 4)) { fclose(f); return false; }
        MapPoint& mp = w.pts[i];
        mp.mWorldPos = cv::Mat(3, 1, CV_32F); mp.mNormalVector = cv::Mat(3, 1, CV_32F); mp.mDescriptor = cv::Mat(1, 32, CV_8U);
        for (int k = 0; k < 3; ++k) { mp.mWorldPos.at<float>(k) = p.pos[k]; mp.mNormalVector.at<float>(k) = p.normal[k]; }
        mp.mfMinDistance = p.min_dist; mp.mfMaxDistance = p.max_dist; mp.nObs = p.blocks ? 1 : 0; mp.mbBad = bad != 0; mp.mnId = i;
        std::memcpy(mp.mDescriptor.ptr(0), p.desc, 32);
        mp.mnLastFrameSeen = (long unsigned int)-1; mp.mnTrackReferenceForFrame = (long unsigned int)-1;
        w.vp[i] = &mp;
    }
    w.pre.resize(npre);
    for (auto& p : w.pre) {
        int32_t a[2];
        if (!rd(f, a, 8) || a[0] < 0 || a[0] >= n || a[1] < 0 || a[1] >= npts) { fclose(f); return false; }
        p = {a[0], a[1]};
    }
    fclose(f);
    // the points spread over keyframes of 2 000, each observed by its keyframe (a point that `blocks` by one more, so that the packed
    // row keeps its Observations() > 0 and the others keep 0: AddObservation counts)
    const int per = 2000;
    w.nk = (npts + per - 1) / per;
    w.kfs.reset(new KeyFrame[w.nk > 0 ? w.nk : 1]);
    for (int k = 0; k < w.nk; ++k) {
        KeyFrame& kf = w.kfs[k];
        kf.mnId = k; kf.mnTrackReferenceForFrame = (long unsigned int)-1;
        const int lo = k * per, hi = std::min(npts, lo + per);
        kf.N_total = hi - lo; kf.mvpMapPoints.assign((size_t)(hi - lo), nullptr);
        for (int i = lo; i < hi; ++i) {
            kf.mvpMapPoints[(size_t)(i - lo)] = &w.pts[i];
            const int before = w.pts[i].nObs;
            w.pts[i].AddObservation(&kf, (size_t)(i - lo));
            w.pts[i].nObs = before;                              // (Observations() stays what the world file says: it decides `blocks`)
        }
    }
    w.place();
    return true;
}

int ref_update_local_map(SearchWorld& w) {   // the transcription, on this world's members
    std::map<KeyFrame*, int> keyframeCounter;
    for (int i = 0; i < w.F.N_total; i++) {
        if (w.F.mvpMapPoints[i]) {
            MapPoint* pMP = w.F.mvpMapPoints[i];
            if (!pMP->isBad()) {
                const std::map<KeyFrame*, size_t> observations = pMP->GetObservations();
                for (std::map<KeyFrame*, size_t>::const_iterator it = observations.begin(), itend = observations.end(); it != itend; it++) keyframeCounter[it->first]++;
            } else w.F.mvpMapPoints[i] = NULL;
        }
    }
    if (!keyframeCounter.empty()) {
        int max = 0; KeyFrame* pKFmax = NULL;
        w.local.clear(); w.local.reserve(3 * keyframeCounter.size());
        for (std::map<KeyFrame*, int>::const_iterator it = keyframeCounter.begin(); it != keyframeCounter.end(); it++) {
            KeyFrame* pKF = it->first;
            if (pKF->isBad()) continue;
            if (it->second > max) { max = it->second; pKFmax = pKF; }
            w.local.push_back(it->first); pKF->mnTrackReferenceForFrame = w.F.mnId;
        }
        // (these keyframes have no neighbours, children or parents: K2 adds nothing)
        if (pKFmax) { w.ref = pKFmax; w.F.mpReferenceKF = pKFmax; }
    }
    w.lpts.clear();
    for (KeyFrame* pKF : w.local) {
        const std::vector<MapPoint*> vpMPs = pKF->GetMapPointMatches();
        for (MapPoint* pMP : vpMPs) {
            if (!pMP) continue;
            if (pMP->mnTrackReferenceForFrame == w.F.mnId) continue;
            if (!pMP->isBad()) { w.lpts.push_back(pMP); pMP->mnTrackReferenceForFrame = w.F.mnId; }
        }
    }
    return (int)w.lpts.size();
}

int compare_search(const SearchWorld& a, const SearchWorld& b, const char* what) {
    int bad = 0;
    for (size_t i = 0; i < a.pts.size(); ++i) {
        const MapPoint& p = a.pts[i]; const MapPoint& q = b.pts[i];
        bool same = p.mbTrackInView == q.mbTrackInView && p.mnVisible == q.mnVisible && p.mnLastFrameSeen == q.mnLastFrameSeen &&
                    p.mnTrackReferenceForFrame == q.mnTrackReferenceForFrame;
        if (p.mbTrackInView && q.mbTrackInView)
            same = same && std::memcmp(&p.mTrackProjX, &q.mTrackProjX, 4) == 0 && std::memcmp(&p.mTrackProjY, &q.mTrackProjY, 4) == 0 &&
                   std::memcmp(&p.mTrackProjXR, &q.mTrackProjXR, 4) == 0 && std::memcmp(&p.mTrackViewCos, &q.mTrackViewCos, 4) == 0 &&
                   p.mnTrackScaleLevel == q.mnTrackScaleLevel;
        if (!same && bad++ < 10) fprintf(stderr, "%s: point %zu differs: in view %d/%d visible %d/%d\n", what, i, (int)p.mbTrackInView, (int)q.mbTrackInView, p.mnVisible, q.mnVisible);
    }
    for (int g = 0; g < a.F.N_total; ++g) {
        const long ia = a.F.mvpMapPoints[g] ? (long)(a.F.mvpMapPoints[g] - a.pts.data()) : -1;
        const long ib = b.F.mvpMapPoints[g] ? (long)(b.F.mvpMapPoints[g] - b.pts.data()) : -1;
        if (ia != ib && bad++ < 10) fprintf(stderr, "%s: feature %d holds point %ld / %ld\n", what, g, ia, ib);
    }
    if (a.lpts.size() != b.lpts.size()) { fprintf(stderr, "%s: %zu / %zu local points\n", what, a.lpts.size(), b.lpts.size()); ++bad; }
    else for (size_t i = 0; i < a.lpts.size(); ++i)
        if ((a.lpts[i] - a.pts.data()) != (b.lpts[i] - b.pts.data()) && bad++ < 10) fprintf(stderr, "%s: local point %zu differs\n", what, i);
    return bad;
}

ResidentMap::Capacity search_capacity(const SearchWorld& w) {
    ResidentMap::Capacity c; c.keyframes = 64; c.points = (int)w.pts.size() + 16; c.observations = (int)w.pts.size() + 16; c.features_per_keyframe = 2000;
    return c;
}
void touch_all(SearchWorld& w, ResidentMap& R) { for (int k = 0; k < w.nk; ++k) R.Touch(&w.kfs[k]); for (MapPoint& p : w.pts) R.Touch(&p); }

int run_search(const char* world) {
    SearchWorld A, B;
    if (!load(world, A) || !load(world, B)) return 2;
    B.F.mnId = A.F.mnId;
    ORBmatcher ma(0.8f), mb(0.8f);
    ResidentMap R(&ma, search_capacity(A));
    touch_all(A, R);
    const unsigned long fails = ORBmatcher::FailureCount();
    int bad = 0, na = 0, nb = 0, ra = 0, rb = 0;
    for (int frame = 0; frame < 2; ++frame) {
        if (frame == 1) {   // a second frame: a new id, the first frame's matches stay in F.mvpMapPoints, some points moved or gone bad
            const long unsigned int second_id = A.F.mnId + 1000;
            for (SearchWorld* W : {&A, &B}) {
                W->F.mnId = second_id;
                for (size_t i = 0; i < W->pts.size(); ++i) {
                    if (i % 50 == 7) W->pts[i].mWorldPos.at<float>(0) += 0.01f;
                    if (i % 97 == 3) W->pts[i].mDescriptor.ptr(0)[5] ^= 0x10;
                }
                for (size_t i = 11; i < W->pts.size() && i < 14; ++i) W->pts[i].mbBad = true;
            }
            for (MapPoint& p : A.pts) R.Touch(&p);   // (every point touched: Flush sends the rows whose bytes changed)
        }
        UpdateLocalMap(R, A.F, A.local, A.lpts, A.ref);
        ra = SearchLocalPoints(ma, R, A.F, A.lpts, A.th, &na);
        ref_update_local_map(B);
        rb = SearchLocalPoints(mb, B.F, B.lpts, B.th, &nb);
        if (ORBmatcher::FailureCount() != fails) { fprintf(stderr, "a device call failed: %s\n", ORBmatcher::LastError()); return 3; }
        bad += compare_search(A, B, frame ? "second frame" : "first frame");
        if (ra != rb || na != nb) { fprintf(stderr, "frame %d: counts differ: matches %d / %d, in view %d / %d\n", frame, ra, rb, na, nb); ++bad; }
        if (frame == 1) {
            int changed = 0;
            for (size_t i = 0; i < A.pts.size(); ++i) changed += (i % 50 == 7 || i % 97 == 3 || (i >= 11 && i < 14)) ? 1 : 0;
            // (UpdateLocalMap's Flush sent them; the one inside SearchLocalPoints found nothing queued)
            if (ra <= 0 || A.lpts.empty()) { fprintf(stderr, "second frame: nothing matched\n"); ++bad; }
            printf("second frame: %d rows changed\n", changed);
        }
    }
    if (bad) return 1;
    printf("local_map search ok: %zu points in %d keyframes, %zu listed, %d in view, %d matches\n", A.pts.size(), A.nk, A.lpts.size(), na, ra);
    return 0;
}

int run_time(const char* world, double seconds) {
    SearchWorld A, B;
    if (!load(world, A) || !load(world, B)) return 2;
    ORBmatcher ma(0.8f), mb(0.8f);
    ResidentMap R(&ma, search_capacity(A));
    touch_all(A, R);
    using clk = std::chrono::steady_clock;
    long unsigned int id = 1000;
    for (int pair = -1; pair < 5; ++pair)          // (pair -1: warm-up, not reported)
        for (int leg = 0; leg < 2; ++leg) {
            SearchWorld& W = leg ? B : A;
            const double budget = pair < 0 ? 0.2 : seconds;
            long calls = 0; int nm = 0, nin = 0; double el = 0;
            const clk::time_point t0 = clk::now();
            do {
                W.place(); W.F.mnId = ++id;                      // a new frame id per call: the marks of the call before do not count
                if (leg) { ref_update_local_map(W); nm = SearchLocalPoints(mb, W.F, W.lpts, W.th, &nin); }
                else { UpdateLocalMap(R, W.F, W.local, W.lpts, W.ref); nm = SearchLocalPoints(ma, R, W.F, W.lpts, W.th, &nin); }
                ++calls;
                el = std::chrono::duration<double>(clk::now() - t0).count();
            } while (el < budget);
            if (pair >= 0)
                printf("{\"leg\": \"%s\", \"pair\": %d, \"calls\": %ld, \"us_per_call\": %.2f, \"local_points\": %zu, \"in_view\": %d, \"matches\": %d}\n",
                       leg ? "reference_update_then_point_table_search" : "resident_map_update_and_search", pair, calls, el * 1e6 / calls, W.lpts.size(), nin, nm);
        }
    return ORBmatcher::FailureCount() ? 3 : 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "host") return run_all(false);
    if (mode == "device") return run_all(true);
    if (mode == "search" && argc >= 3) return run_search(argv[2]);
    if (mode == "time" && argc >= 4) return run_time(argv[2], std::atof(argv[3]));
    fprintf(stderr, "usage: test_local_map host | device | search WORLD.bin | time WORLD.bin SECONDS\n");
    return 2;
}
