// test_refresh.cc -- driver of RefreshMapPoints (host/MapPointRefresh.h) for tests/test_gpu_map_points.py and tools/map_points_bench.py.
//
//   test_refresh check                  a small map built here (two-camera keyframes, a tenth of them bad, bad points, points without
//                                       observations, a point whose reference keyframe does not observe it, long points around the
//                                       device's size classes and beyond its cap): RefreshMapPoints with each job mask on one copy, the
//                                       two reference functions restated per point with cv_compat.h types on another; mDescriptor,
//                                       mNormalVector and the two distances of every point are compared as bytes.
//   test_refresh time [POINTS SECONDS]  the two alternated in one process, five pairs, SECONDS per leg; one JSON line per leg
//   test_refresh world WORLD OUT WHAT   a map read from a file (one keyframe per observation, so that any centre can be asked for),
//                                       RefreshMapPoints(WHAT) on it; OUT receives what every point holds afterwards
//
// WORLD (little endian): int32 P, n_obs, n_levels; float scale[n_levels]; int32 first[P+1]; int32 ref_obs[P] (the observation whose keyframe
// is the point's reference keyframe, or -1: a keyframe that does not observe the point); uint8 desc[n_obs*32]; float centre[n_obs*3];
// uint8 alive[n_obs]; float pos[P*3], ref_centre[P*3]; int32 ref_level[P]; uint8 bad[P].
// OUT: P x {uint8 desc[32]; float normal[3], min_dist, max_dist}.  Before the call every point holds 0xAB bytes, (7, 8, 9), 11, 12.
#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <numeric>
#include <string>
#include <vector>
#include "MapPointRefresh.h"

using namespace ORB_SLAM2;

namespace {

struct Rng {   // splitmix64
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed) {}
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    double uni() { return (double)(next() >> 11) / 9007199254740992.0; }
    int below(int n) { return (int)(next() % (uint64_t)n); }
};

// ---- the two reference functions, restated per point on the stand-in types (src/MapPoint.cc:325-438, :480-528) ---------------------
void ComputeDistinctiveDescriptors(MapPoint* pMP) {
    if (pMP->isBad()) return;
    std::map<KeyFrame*, size_t> observations = pMP->mObservations;
    if (observations.empty()) return;
    std::vector<cv::Mat> vDescriptors;
    for (auto& ob : observations) {
        KeyFrame* pKF = ob.first;
        if (pKF->isBad()) continue;
        const int cam = pKF->keypoint_to_cam.find(ob.second)->second;
        const int descIdx = pKF->cont_idx_to_local_cam_idx.find(ob.second)->second;
        vDescriptors.push_back(pKF->GetDescriptor(cam, descIdx));
    }
    if (vDescriptors.empty()) return;
    const size_t N = vDescriptors.size();
    std::vector<std::vector<float>> Distances(N, std::vector<float>(N, 0.0f));
    for (size_t i = 0; i < N; i++)
        for (size_t j = i + 1; j < N; j++) {
            const int d = ORBmatcher::DescriptorDistance(vDescriptors[i], vDescriptors[j]);
            Distances[i][j] = d; Distances[j][i] = d;
        }
    int BestMedian = INT_MAX, BestIdx = 0;
    for (size_t i = 0; i < N; i++) {
        std::vector<int> vDists(Distances[i].begin(), Distances[i].end());
        std::sort(vDists.begin(), vDists.end());
        const int median = vDists[0.5 * (N - 1)];
        if (median < BestMedian) { BestMedian = median; BestIdx = i; }
    }
    pMP->mDescriptor = vDescriptors[BestIdx].clone();
}

void UpdateNormalAndDepth(MapPoint* pMP) {
    if (pMP->isBad()) return;
    std::map<KeyFrame*, size_t> observations = pMP->mObservations;
    KeyFrame* pRefKF = pMP->mpRefKF;
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

// ---- maps -------------------------------------------------------------------------------------------------------------------
struct Map {
    std::vector<KeyFrame> kfs;      // one block: pointer order is index order, which is the iteration order of std::map<KeyFrame*, size_t>
    std::deque<MapPoint> pts;
    std::vector<MapPoint*> vp;
};

cv::Mat pose_with_centre(const float* c) {   // identity rotation: the camera centre -(R.t()*t) is exactly c
    cv::Mat T = cv::Mat::eye(4, 4, CV_32F);
    for (int k = 0; k < 3; ++k) T.at<float>(k, 3) = -c[k];
    return T;
}

std::vector<float> pyramid(int n_levels) {
    std::vector<float> s(n_levels, 1.0f);
    for (int k = 1; k < n_levels; ++k) s[k] = s[k - 1] * 1.2f;
    return s;
}

void prefill(MapPoint& mp) {
    mp.mDescriptor = cv::Mat(1, 32, CV_8U); std::memset(mp.mDescriptor.ptr(0), 0xAB, 32);
    mp.mNormalVector = cv::Mat(3, 1, CV_32F);
    mp.mNormalVector.at<float>(0) = 7; mp.mNormalVector.at<float>(1) = 8; mp.mNormalVector.at<float>(2) = 9;
    mp.mfMinDistance = 11; mp.mfMaxDistance = 12;
}

// a general rigid pose (rotation about a random axis), so that GetCameraCenter() is real pose algebra
cv::Mat random_pose(Rng& r) {
    double ax[3] = {r.uni() - 0.5, r.uni() - 0.5, r.uni() - 0.5};
    const double nn = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]) + 1e-9;
    for (double& a : ax) a /= nn;
    const double th = (r.uni() - 0.5) * 2.0, c = std::cos(th), s = std::sin(th);
    const double R[9] = {c + ax[0] * ax[0] * (1 - c), ax[0] * ax[1] * (1 - c) - ax[2] * s, ax[0] * ax[2] * (1 - c) + ax[1] * s,
                         ax[1] * ax[0] * (1 - c) + ax[2] * s, c + ax[1] * ax[1] * (1 - c), ax[1] * ax[2] * (1 - c) - ax[0] * s,
                         ax[2] * ax[0] * (1 - c) - ax[1] * s, ax[2] * ax[1] * (1 - c) + ax[0] * s, c + ax[2] * ax[2] * (1 - c)};
    cv::Mat T = cv::Mat::eye(4, 4, CV_32F);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) T.at<float>(i, j) = (float)R[3 * i + j];
        T.at<float>(i, 3) = (float)((r.uni() - 0.5) * 40.0);
    }
    return T;
}

// n_kf two-camera keyframes of `feat` features per camera, n_pts points with 1 + geometric(0.12) observations (capped by n_kf), the
// descriptor of an observation = the point's base with up to 39 bits flipped
void build_map(Map& M, int n_kf, int n_pts, int feat, uint64_t seed, const std::vector<int>& forced_counts) {
    Rng r(seed);
    const std::vector<float> scale = pyramid(8);
    M.kfs.resize(n_kf);
    std::vector<int> used(n_kf, 0);
    for (KeyFrame& kf : M.kfs) {
        kf.Tcw = random_pose(r); kf.Tcw_cam2 = random_pose(r);
        kf.mvScaleFactors = scale; kf.mnScaleLevels = 8;
        kf.N = feat; kf.N_cam2 = feat; kf.N_total = 2 * feat;
        kf.mvKeysUn_total.resize(2 * feat);
        for (cv::KeyPoint& k : kf.mvKeysUn_total) k.octave = r.below(8);
        kf.mDescriptors_total.resize(2);
        for (int c = 0; c < 2; ++c) {
            kf.mDescriptors_total[c].create(feat, 32, CV_8U);
            for (int i = 0; i < feat * 32; ++i) kf.mDescriptors_total[c].ptr(0)[i] = (uint8_t)r.next();
        }
        for (int g = 0; g < 2 * feat; ++g) { kf.keypoint_to_cam[g] = g < feat ? 0 : 1; kf.cont_idx_to_local_cam_idx[g] = g < feat ? g : g - feat; }
        kf.mbBad = r.uni() < 0.1;
    }
    for (int p = 0; p < n_pts; ++p) {
        M.pts.emplace_back();
        MapPoint& mp = M.pts.back();
        mp.nObs = 0;
        mp.mWorldPos = cv::Mat(3, 1, CV_32F);
        for (int k = 0; k < 3; ++k) mp.mWorldPos.at<float>(k) = (float)((r.uni() - 0.5) * 40.0);
        prefill(mp);
        int n = 1;
        while (r.uni() >= 0.12 && n < 300) ++n;
        if (p < (int)forced_counts.size()) n = forced_counts[p];
        n = std::min(n, n_kf);
        uint8_t base[32];
        for (uint8_t& b : base) b = (uint8_t)r.next();
        // n distinct keyframes: a random start and stride through the array
        const int start = r.below(n_kf);
        int stride = 1 + r.below(n_kf - 1);
        while (std::gcd(stride, n_kf) != 1) ++stride;
        KeyFrame* first_kf = nullptr;
        for (int j = 0; j < n; ++j) {
            KeyFrame& kf = M.kfs[(start + (long long)j * stride) % n_kf];
            const int idx = used[&kf - M.kfs.data()]++;
            if (idx >= kf.N_total) continue;                                   // the keyframe is full
            const int cam = kf.keypoint_to_cam[idx], loc = kf.cont_idx_to_local_cam_idx[idx];
            uint8_t* d = kf.mDescriptors_total[cam].ptr(loc);
            std::memcpy(d, base, 32);
            for (int f = r.below(40); f > 0; --f) { const int bit = r.below(256); d[bit >> 3] ^= (uint8_t)(1u << (bit & 7)); }
            mp.AddObservation(&kf, (size_t)idx);
            if (!first_kf || r.uni() < 0.3) first_kf = &kf;
        }
        mp.mpRefKF = first_kf ? first_kf : &M.kfs[r.below(n_kf)];
        if (p % 17 == 5) mp.mpRefKF = &M.kfs[r.below(n_kf)];                  // most likely not an observer: observations[pRefKF] inserts 0
        if (p % 23 == 7) mp.mbBad = true;
        M.vp.push_back(&mp);
    }
    M.vp.push_back(nullptr);                       // a hole, and a point twice
    if (n_pts > 3) M.vp.push_back(M.vp[3]);
}

bool same_point(MapPoint& a, MapPoint& b, int i, const char* what) {
    const bool ok = std::memcmp(a.mDescriptor.ptr(0), b.mDescriptor.ptr(0), 32) == 0 &&
                    std::memcmp(a.mNormalVector.ptr(0), b.mNormalVector.ptr(0), 12) == 0 &&
                    std::memcmp(&a.mfMinDistance, &b.mfMinDistance, 4) == 0 && std::memcmp(&a.mfMaxDistance, &b.mfMaxDistance, 4) == 0;
    if (!ok)
        std::fprintf(stderr, "%s: point %d (%d observations) differs: normal (%g %g %g) vs (%g %g %g), distances %g %g vs %g %g, descriptors %s\n", what, i,
                     (int)a.mObservations.size(), a.mNormalVector.at<float>(0), a.mNormalVector.at<float>(1), a.mNormalVector.at<float>(2),
                     b.mNormalVector.at<float>(0), b.mNormalVector.at<float>(1), b.mNormalVector.at<float>(2), a.mfMinDistance, a.mfMaxDistance,
                     b.mfMinDistance, b.mfMaxDistance, std::memcmp(a.mDescriptor.ptr(0), b.mDescriptor.ptr(0), 32) ? "differ" : "equal");
    return ok;
}

int run_check() {
    const std::vector<int> forced = {0, 1, 2, 3, 16, 17, 64, 65, 256, 257, 300};
    int fails = 0;
    for (int what = 1; what <= 3; ++what) {
        for (int n_pts : {3000, 9}) {              // a device batch and one below REFRESH_HOST_BELOW
            Map A, B;
            build_map(A, 400, n_pts, 40, 1234 + n_pts, forced);
            build_map(B, 400, n_pts, 40, 1234 + n_pts, forced);
            ORBmatcher matcher(0.6f, true);
            RefreshMapPoints(matcher, A.vp, what);
            int st[5]; RefreshStats(st);
            if (ORBmatcher::FailureCount()) { std::fprintf(stderr, "device failure: %s\n", ORBmatcher::LastError()); return 1; }
            for (MapPoint* p : B.vp) {
                if (!p) continue;
                if (what & REFRESH_DESCRIPTOR) ComputeDistinctiveDescriptors(p);
                if (what & REFRESH_NORMAL_DEPTH) UpdateNormalAndDepth(p);
            }
            int changed = 0;
            for (int i = 0; i < n_pts; ++i) {
                if (!same_point(A.pts[i], B.pts[i], i, "check")) ++fails;
                MapPoint fresh; prefill(fresh);
                if (std::memcmp(B.pts[i].mDescriptor.ptr(0), fresh.mDescriptor.ptr(0), 32) || B.pts[i].mfMaxDistance != 12.0f) ++changed;
            }
            std::printf("what %d, %d points: paths {%d %d %d %d %d}, %d points refreshed, %d differ\n", what, n_pts, st[0], st[1], st[2], st[3], st[4], changed, fails);
            if (changed < n_pts / 2) { std::fprintf(stderr, "too few points were refreshed\n"); return 1; }
            if (n_pts >= REFRESH_HOST_BELOW && (st[0] == 0 || st[1] == 0 || st[2] == 0 || st[3] == 0)) { std::fprintf(stderr, "a path was not taken\n"); return 1; }
            if (n_pts < REFRESH_HOST_BELOW && (st[0] || st[1] || st[2])) { std::fprintf(stderr, "a small batch went to the device\n"); return 1; }
        }
    }
    if (fails) return 1;
    std::printf("refresh check ok\n");
    return 0;
}

int run_time(int n_pts, double seconds) {
    Map A, B;
    build_map(A, 400, n_pts, 2 + n_pts / 20, 99, {});
    build_map(B, 400, n_pts, 2 + n_pts / 20, 99, {});
    ORBmatcher matcher(0.6f, true);
    RefreshMapPoints(matcher, A.vp, REFRESH_BOTH);     // warm: handle, scratch
    if (ORBmatcher::FailureCount()) { std::fprintf(stderr, "device failure: %s\n", ORBmatcher::LastError()); return 1; }
    for (int pair = 0; pair < 5; ++pair)
        for (int leg = 0; leg < 2; ++leg) {
            const auto t0 = std::chrono::steady_clock::now();
            long calls = 0; double el = 0;
            do {
                if (leg == 0) RefreshMapPoints(matcher, A.vp, REFRESH_BOTH);
                else for (MapPoint* p : B.vp) { if (!p) continue; ComputeDistinctiveDescriptors(p); UpdateNormalAndDepth(p); }
                ++calls;
                el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            } while (el < seconds);
            std::printf("{\"leg\": \"%s\", \"pair\": %d, \"points\": %d, \"calls\": %ld, \"us_per_call\": %.2f}\n", leg == 0 ? "class" : "per_point", pair, n_pts, calls, 1e6 * el / calls);
        }
    for (int i = 0; i < n_pts; ++i) if (!same_point(A.pts[i], B.pts[i], i, "time")) return 1;
    return 0;
}

bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
template <class T> bool rdv(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return rd(f, v.data(), n * sizeof(T)); }

int run_world(const char* wpath, const char* opath, int what) {
    FILE* f = std::fopen(wpath, "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", wpath); return 1; }
    int32_t h[3];
    if (!rd(f, h, sizeof h) || h[0] < 0 || h[1] < 0 || h[2] < 1 || h[2] > 32) { std::fprintf(stderr, "bad header\n"); std::fclose(f); return 1; }
    const int P = h[0], NO = h[1], L = h[2];
    std::vector<float> scale, centre, pos, refc; std::vector<int32_t> first, ref_obs, ref_level; std::vector<uint8_t> desc, alive, bad;
    const bool ok = rdv(f, scale, L) && rdv(f, first, (size_t)P + 1) && rdv(f, ref_obs, P) && rdv(f, desc, (size_t)NO * 32) && rdv(f, centre, (size_t)NO * 3) &&
                    rdv(f, alive, NO) && rdv(f, pos, (size_t)P * 3) && rdv(f, refc, (size_t)P * 3) && rdv(f, ref_level, P) && rdv(f, bad, P);
    std::fclose(f);
    if (!ok) { std::fprintf(stderr, "short file\n"); return 1; }
    // keyframe o makes observation o; keyframe NO + p is the reference keyframe of a point whose reference does not observe it.
    // Observation o is feature o % 3 of its keyframe, seen by camera o % 2 as row (o / 2) % 2 of that camera's descriptors.
    Map M;
    M.kfs.resize((size_t)NO + P);
    Rng r(5);
    for (int o = 0; o < NO + P; ++o) {
        KeyFrame& kf = M.kfs[o];
        kf.mvScaleFactors = scale; kf.mnScaleLevels = L;
        kf.N = 2; kf.N_cam2 = 2; kf.N_total = 3;
        kf.mvKeysUn_total.resize(3);
        for (cv::KeyPoint& k : kf.mvKeysUn_total) k.octave = L + 5;            // (never a valid level: whatever is read must have been set below)
        kf.mDescriptors_total.resize(2);
        for (int c = 0; c < 2; ++c) {
            kf.mDescriptors_total[c].create(2, 32, CV_8U);
            for (int i = 0; i < 64; ++i) kf.mDescriptors_total[c].ptr(0)[i] = (uint8_t)r.next();
        }
        float junk[3] = {(float)(r.uni() * 50), (float)(r.uni() * 50), (float)(r.uni() * 50)};
        const int g = o % 3, cam = o % 2, loc = (o / 2) % 2;
        if (o < NO) {
            kf.keypoint_to_cam[g] = cam; kf.cont_idx_to_local_cam_idx[g] = loc;
            std::memcpy(kf.mDescriptors_total[cam].ptr(loc), &desc[(size_t)o * 32], 32);
            kf.Tcw = pose_with_centre(cam == 0 ? &centre[(size_t)o * 3] : junk);
            kf.Tcw_cam2 = pose_with_centre(cam == 1 ? &centre[(size_t)o * 3] : junk);
            kf.mbBad = alive[o] == 0;
        } else {
            kf.keypoint_to_cam[0] = 0; kf.cont_idx_to_local_cam_idx[0] = 0;
            kf.Tcw = pose_with_centre(&refc[(size_t)(o - NO) * 3]); kf.Tcw_cam2 = pose_with_centre(junk);
            kf.mvKeysUn_total[0].octave = ref_level[o - NO];                   // observations[pRefKF] inserts index 0
        }
    }
    for (int p = 0; p < P; ++p) {
        M.pts.emplace_back();
        MapPoint& mp = M.pts.back();
        mp.nObs = 0;
        mp.mWorldPos = cv::Mat(3, 1, CV_32F);
        for (int k = 0; k < 3; ++k) mp.mWorldPos.at<float>(k) = pos[(size_t)p * 3 + k];
        prefill(mp);
        for (int o = first[p]; o < first[p + 1]; ++o) mp.AddObservation(&M.kfs[o], (size_t)(o % 3));
        if (ref_obs[p] >= 0) {
            const int o = ref_obs[p];
            if (o < first[p] || o >= first[p + 1] || o % 2 != 0) { std::fprintf(stderr, "ref_obs[%d] must be a camera-1 observation of the point\n", p); return 1; }
            mp.mpRefKF = &M.kfs[o];
            M.kfs[o].mvKeysUn_total[o % 3].octave = ref_level[p];
        } else {
            mp.mpRefKF = &M.kfs[(size_t)NO + p];
        }
        mp.mbBad = bad[p] != 0;
        M.vp.push_back(&mp);
    }
    ORBmatcher matcher(0.6f, true);
    RefreshMapPoints(matcher, M.vp, what);
    if (ORBmatcher::FailureCount()) { std::fprintf(stderr, "device failure: %s\n", ORBmatcher::LastError()); return 1; }
    int st[5]; RefreshStats(st);
    FILE* o = std::fopen(opath, "wb");
    if (!o) { std::fprintf(stderr, "cannot write %s\n", opath); return 1; }
    for (int p = 0; p < P; ++p) {
        MapPoint& mp = M.pts[p];
        std::fwrite(mp.mDescriptor.ptr(0), 1, 32, o); std::fwrite(mp.mNormalVector.ptr(0), 4, 3, o);
        std::fwrite(&mp.mfMinDistance, 4, 1, o); std::fwrite(&mp.mfMaxDistance, 4, 1, o);
    }
    std::fclose(o);
    std::printf("refresh world ok: %d points, %d observations, paths {%d %d %d %d %d}\n", P, NO, st[0], st[1], st[2], st[3], st[4]);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "check") return run_check();
    if (mode == "time") return run_time(argc > 2 ? std::atoi(argv[2]) : 1500, argc > 3 ? std::atof(argv[3]) : 1.0);
    if (mode == "world" && argc == 5) return run_world(argv[2], argv[3], std::atoi(argv[4]));
    std::fprintf(stderr, "usage: test_refresh check | time [POINTS SECONDS] | world WORLD OUT WHAT\n");
    return 2;
}
