// test_new_points_keyframe.cc -- driver of CreateNewPointsOfKeyFrame and ResidentKeyFrames (host/NewMapPoints.h) on stand-in keyframes
// read from a text file (tests/test_new_points_keyframe_class.py writes it from a world of tests/new_points_worlds.py and compares what
// comes back with the CPU reference chain).
//   test_new_points_keyframe FILE          the call, twice (the second one out of the resident keyframes), then Forget
//   test_new_points_keyframe FILE host     what needs no device: the flattening, the baselines and the books of the cache (dry run)
// FILE: "K monocular", then 1 + K keyframes (the current one first) -- "n N", Tcw (12 floats), Tcw_cam2 (12), "fx fy cx cy invfx invfy mbf
// mb scaleFactor", "nlevels", the scale factors, the level sigma2, mRcam12 (9), mtcam12 (3), n lines "x y xd yd octave uright depth cam
// angle hasMapPoint descriptor(64 hex digits)", "nnodes", nnodes lines "nodeId count idx..." -- floats as the hexadecimal of their bits.
// Output: per keyframe "kf i" + the camera centres and Twc the class read (bits); per planned neighbour "round k neighbour j baseline
// baseline_cam2 istrian0 istrian1" (bits); per call "call c rounds R", per neighbour "neighbour j pairs P" and P lines "idx1 idx2 outcome
// accepted x y z" (bits, or - - -), "cache created reused evicted size"; at last the Forget / eviction lines.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include "NewMapPoints.h"
#include "slam_types.h"

using namespace ORB_SLAM2;

static float rdf(std::istream& in) { std::string s; in >> s; const uint32_t u = (uint32_t)std::stoul(s, nullptr, 16); float f; std::memcpy(&f, &u, 4); return f; }
static unsigned bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

static cv::Mat pose(std::istream& in) {
    cv::Mat T = cv::Mat::eye(4, 4, CV_32F);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) T.at<float>(r, c) = rdf(in);
    return T;
}

static MapPoint g_some_point;

static bool read_keyframe(std::istream& in, KeyFrame& K) {
    int n = 0, N = 0;
    in >> n >> N;
    if (!in.good() || n < 0 || N < 0 || N > n) return false;
    K.N = N; K.N_cam2 = n - N; K.N_total = n;
    K.Tcw = pose(in); K.Tcw_cam2 = pose(in);
    K.fx = rdf(in); K.fy = rdf(in); K.cx = rdf(in); K.cy = rdf(in); K.invfx = rdf(in); K.invfy = rdf(in); K.mbf = rdf(in); K.mb = rdf(in);
    K.mfScaleFactor = rdf(in);
    K.mK = cv::Mat::eye(3, 3, CV_32F);
    K.mK.at<float>(0, 0) = K.fx; K.mK.at<float>(1, 1) = K.fy; K.mK.at<float>(0, 2) = K.cx; K.mK.at<float>(1, 2) = K.cy;
    int L = 0; in >> L;
    if (!in.good() || L < 1 || L > 64) return false;
    K.mnScaleLevels = L; K.mvScaleFactors.resize(L); K.mvLevelSigma2.resize(L);
    for (int k = 0; k < L; ++k) K.mvScaleFactors[k] = rdf(in);
    for (int k = 0; k < L; ++k) K.mvLevelSigma2[k] = rdf(in);
    K.mRcam12 = cv::Mat(3, 3, CV_32F); K.mtcam12 = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) K.mRcam12.at<float>(r, c) = rdf(in);
    for (int r = 0; r < 3; ++r) K.mtcam12.at<float>(r) = rdf(in);
    K.mvKeysUn_total.resize(n); K.mvKeys_total.resize(n); K.mvuRight_total.resize(n); K.mvDepth_total.resize(n); K.mvpMapPoints.assign(n, nullptr);
    K.mDescriptors_total.resize(2);
    K.mDescriptors_total[0].create(N > 0 ? N : 1, 32, CV_8U); K.mDescriptors_total[1].create(n - N > 0 ? n - N : 1, 32, CV_8U);
    for (int i = 0; i < n; ++i) {
        K.mvKeysUn_total[i].pt.x = rdf(in); K.mvKeysUn_total[i].pt.y = rdf(in);
        K.mvKeys_total[i].pt.x = rdf(in); K.mvKeys_total[i].pt.y = rdf(in);
        int octave; in >> octave;
        K.mvKeysUn_total[i].octave = K.mvKeys_total[i].octave = octave;
        K.mvuRight_total[i] = rdf(in); K.mvDepth_total[i] = rdf(in);
        int cam; in >> cam;
        if (cam != (i < N ? 0 : 1)) return false;                       // the reference numbers camera-1 features first
        K.keypoint_to_cam[(size_t)i] = cam;
        K.cont_idx_to_local_cam_idx[(size_t)i] = i < N ? i : i - N;
        K.mvKeysUn_total[i].angle = K.mvKeys_total[i].angle = rdf(in);
        int has; in >> has;
        if (has) K.mvpMapPoints[i] = &g_some_point;
        std::string hex; in >> hex;
        if (hex.size() != 64) return false;
        unsigned char* row = K.mDescriptors_total[cam].ptr(i < N ? i : i - N);
        for (int b = 0; b < 32; ++b) row[b] = (unsigned char)std::stoul(hex.substr(2 * (size_t)b, 2), nullptr, 16);
    }
    int nodes = 0; in >> nodes;
    if (!in.good() || nodes < 0) return false;
    for (int k = 0; k < nodes; ++k) {
        unsigned id; int count; in >> id >> count;
        if (!in.good() || count < 0) return false;
        std::vector<unsigned int>& v = K.mFeatVec[id];
        for (int j = 0; j < count; ++j) { unsigned idx; in >> idx; if (idx >= (unsigned)n) return false; v.push_back(idx); }
    }
    return !in.fail();
}

static void print_read(int i, KeyFrame& K) {
    const cv::Mat c1 = K.GetCameraCenter(), c2 = K.GetCameraCenter_cam2(), Twc = K.GetPoseInverse();
    std::printf("kf %d", i);
    for (int k = 0; k < 3; ++k) std::printf(" %08x", bits(c1.at<float>(k)));
    for (int k = 0; k < 3; ++k) std::printf(" %08x", bits(c2.at<float>(k)));
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) std::printf(" %08x", bits(Twc.at<float>(r, c)));
    std::printf("\n");
}

static void print_cache(const ResidentKeyFrames& C) {
    std::printf("cache created %lu reused %lu evicted %lu size %zu\n", C.Created(), C.Reused(), C.Evicted(), C.Size());
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: test_new_points_keyframe FILE [host]\n"); return 2; }
    const bool host_only = argc > 2 && std::strcmp(argv[2], "host") == 0;
    std::ifstream in(argv[1]);
    if (!in.good()) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int K = 0, mono = 0;
    in >> K >> mono;
    if (!in.good() || K < 0 || K > 64) { std::fprintf(stderr, "bad header\n"); return 2; }
    std::vector<std::unique_ptr<KeyFrame> > kfs;
    for (int i = 0; i <= K; ++i) {
        kfs.emplace_back(new KeyFrame());
        if (!read_keyframe(in, *kfs.back())) { std::fprintf(stderr, "short or malformed file (keyframe %d)\n", i); return 2; }
    }
    KeyFrame* cur = kfs[0].get();
    std::vector<KeyFrame*> neigh;
    for (int i = 1; i <= K; ++i) neigh.push_back(kfs[(size_t)i].get());
    auto index_of = [&](KeyFrame* p) { for (int i = 0; i <= K; ++i) if (kfs[(size_t)i].get() == p) return i; return -1; };
    for (int i = 0; i <= K; ++i) print_read(i, *kfs[(size_t)i]);

    std::vector<NewPointsRoundPlan> plan;
    PlanNewPointsRounds(cur, neigh, mono != 0, plan);
    for (size_t k = 0; k < plan.size(); ++k)
        std::printf("round %zu neighbour %d %08x %08x %d %d\n", k, index_of(plan[k].pKF2), bits(plan[k].baseline), bits(plan[k].baseline_cam2),
                    (int)plan[k].istrian[0], (int)plan[k].istrian[1]);

    ORBmatcher matcher(0.6f, true);
    if (host_only) {
        // the books of the cache with nothing on the device: every keyframe is flattened as the resident form needs it
        ResidentKeyFrames C(3);
        C.mbDryRun = true;
        bool ok = true, all = true;
        for (int pass = 0; pass < 2; ++pass) {
            for (int i = 0; i <= K && i < 3; ++i) { C.Get(matcher, kfs[(size_t)i].get(), &ok); all = all && ok; }
            print_cache(C);                                               // pass 0: created, pass 1: reused
        }
        for (int i = 3; i <= K; ++i) { C.Get(matcher, kfs[(size_t)i].get(), &ok); all = all && ok; }
        print_cache(C);                                                   // beyond the capacity: the least recently used leave
        std::printf("holds");
        for (int i = 0; i <= K; ++i) std::printf(" %d", (int)C.Holds(kfs[(size_t)i].get()));
        std::printf("\n");
        KeyFrame* last = kfs[(size_t)K].get();
        C.Forget(last);
        std::printf("forget holds %d size %zu\n", (int)C.Holds(last), C.Size());
        KeyFrame* kept = kfs[(size_t)(K > 0 ? K - 1 : 0)].get();
        if (C.Holds(kept)) {
            kept->mnId += 1000;                                           // another keyframe at the same address: not taken on trust
            C.Get(matcher, kept, &ok); all = all && ok;
            kept->mvKeysUn_total.pop_back(); kept->mvKeys_total.pop_back();   // ... or the same one with another feature count
            kept->mvuRight_total.pop_back(); kept->mvDepth_total.pop_back();
            for (auto& e : kept->mFeatVec) { std::vector<unsigned int> v; for (unsigned idx : e.second) if (idx < kept->mvKeysUn_total.size()) v.push_back(idx); e.second = v; }
            C.Get(matcher, kept, &ok); all = all && ok;
        }
        print_cache(C);
        std::printf("dry run %s\n", all ? "ok" : "FAILED");
        return all ? 0 : 1;
    }

    ResidentKeyFrames& C = ResidentKeyFrames::OfThread();
    for (int call = 0; call < 2; ++call) {
        std::vector<NeighbourPoints> out;
        if (!CreateNewPointsOfKeyFrame(matcher, cur, neigh, mono != 0, out)) { std::fprintf(stderr, "CreateNewPointsOfKeyFrame failed\n"); return 1; }
        std::printf("call %d rounds %zu\n", call, out.size());
        for (const NeighbourPoints& N : out) {
            std::printf("neighbour %d pairs %zu\n", index_of(N.pKF2), N.pairs.size());
            for (size_t i = 0; i < N.pairs.size(); ++i) {
                const TriangulatedPair& p = N.pairs[i];
                std::printf("%zu %zu %d %d", N.vMatchedIndices[i].first, N.vMatchedIndices[i].second, p.outcome, (int)p.accepted);
                if (p.x3D.empty()) std::printf(" - - -\n");
                else std::printf(" %08x %08x %08x\n", bits(p.x3D.at<float>(0)), bits(p.x3D.at<float>(1)), bits(p.x3D.at<float>(2)));
            }
        }
        print_cache(C);
    }
    if (!plan.empty()) {
        KeyFrame* p = plan[0].pKF2;
        const int before = (int)C.Holds(p);
        C.Forget(p);
        std::printf("forget held %d holds %d size %zu\n", before, (int)C.Holds(p), C.Size());
    }
    C.Clear();
    return 0;
}
