// test_sim3opt.cc -- driver of Optimizer::OptimizeSim3_cam1 / OptimizeSim3Batch (host/Optimizer.h) on stand-in keyframes and map points
// read from a text file (tests/test_sim3_optimize_class.py writes it from worlds of tests/sim3opt_worlds.py and compares what comes
// back with the library's host routine).
//   test_sim3opt FILE [batch]
// FILE: "ncases", then per case "th2 fix_scale", the start as "R (9) t (3) s" -- g2o::Sim3(Matrix3d, Vector3d, double) is built from
// them as LoopClosing::ComputeSim3 builds gScm --, two keyframes "Tcw (16) fx fy cx cy nlevels invSigma2... nfeatures" + per feature
// "x y octave", then "N" and per entry of vpMatches1 "has1 bad1 X Y Z has2 bad2 idx2 X Y Z": keyframe 1's map point at that feature and
// the matched point (has = 0: null; idx2 = the matched point's index in keyframe 2 or -1).  Floats travel as the hexadecimal of their
// bits.  With `batch` keyframe 1 of the FIRST case (and its map points) is the current keyframe of every candidate.
// Output per case: "ret q (4) t (3) s matches": the return value, g2oS12 afterwards (doubles, hexadecimal), vpMatches1 as 0 / 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fstream>
#include <string>
#include "g2o_compat.h"
#include "Optimizer.h"
#include "slam_types.h"

using namespace ORB_SLAM2;

static float rdf(std::istream& in) { std::string s; in >> s; const uint32_t u = (uint32_t)std::stoul(s, nullptr, 16); float f; std::memcpy(&f, &u, 4); return f; }
static unsigned long long bits(double d) { unsigned long long u; std::memcpy(&u, &d, 8); return u; }

static void read_keyframe(std::istream& in, KeyFrame& K) {
    K.Tcw = cv::Mat(4, 4, CV_32F);
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) K.Tcw.at<float>(r, c) = rdf(in);
    K.mK = cv::Mat::eye(3, 3, CV_32F);
    K.fx = rdf(in); K.fy = rdf(in); K.cx = rdf(in); K.cy = rdf(in);
    K.mK.at<float>(0, 0) = K.fx; K.mK.at<float>(1, 1) = K.fy; K.mK.at<float>(0, 2) = K.cx; K.mK.at<float>(1, 2) = K.cy;
    int L; in >> L;
    K.mvInvLevelSigma2.resize(L);
    for (int k = 0; k < L; ++k) K.mvInvLevelSigma2[k] = rdf(in);
    int n; in >> n;
    K.N = K.N_total = n;
    K.mvKeysUn.resize(n); K.mvpMapPoints.assign(n, nullptr);
    for (int i = 0; i < n; ++i) { K.mvKeysUn[i].pt.x = rdf(in); K.mvKeysUn[i].pt.y = rdf(in); in >> K.mvKeysUn[i].octave; }
}

static MapPoint* read_point(std::istream& in, KeyFrame* K, int idx, int has, int bad, std::deque<MapPoint>& points) {
    const float X = rdf(in), Y = rdf(in), Z = rdf(in);
    if (!has) return nullptr;
    points.emplace_back();
    MapPoint& P = points.back();
    P.mWorldPos = cv::Mat(3, 1, CV_32F);
    P.mWorldPos.at<float>(0) = X; P.mWorldPos.at<float>(1) = Y; P.mWorldPos.at<float>(2) = Z;
    P.mbBad = bad != 0;
    if (idx >= 0) P.AddObservation(K, (size_t)idx);
    return &P;
}

struct Case {
    float th2 = 0;
    int fix_scale = 0;
    g2o::Sim3 s12;
    KeyFrame kf1, kf2;
    std::vector<MapPoint*> points1, matches1;
};

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: test_sim3opt FILE [batch]\n"); return 2; }
    const bool batch = argc > 2 && !std::strcmp(argv[2], "batch");
    std::ifstream in(argv[1]);
    if (!in.good()) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int ncases;
    in >> ncases;
    std::deque<Case> cases((size_t)ncases);
    std::deque<MapPoint> points;
    for (Case& C : cases) {
        C.th2 = rdf(in);
        in >> C.fix_scale;
        g2o::Matrix3d R;
        g2o::Vector3d t;
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R(r, c) = (double)rdf(in);   // Converter::toMatrix3d
        for (int r = 0; r < 3; ++r) t[r] = (double)rdf(in);                                     // Converter::toVector3d
        const double s = (double)rdf(in);
        C.s12 = g2o::Sim3(R, t, s);
        read_keyframe(in, C.kf1);
        read_keyframe(in, C.kf2);
        int N; in >> N;
        C.matches1.assign((size_t)N, nullptr);
        for (int i = 0; i < N; ++i) {
            int has1, bad1, has2, bad2, idx2;
            in >> has1 >> bad1;
            C.kf1.mvpMapPoints[i] = read_point(in, &C.kf1, i, has1, bad1, points);
            in >> has2 >> bad2 >> idx2;
            C.matches1[i] = read_point(in, &C.kf2, idx2, has2, bad2, points);
        }
    }
    if (!in.good()) { std::fprintf(stderr, "short file\n"); return 2; }
    std::vector<int> ret((size_t)ncases, 0);
    if (batch) {
        std::vector<KeyFrame*> kf2;
        std::vector<std::vector<MapPoint*> > matches;
        std::vector<g2o::Sim3> s12;
        for (Case& C : cases) { kf2.push_back(&C.kf2); matches.push_back(C.matches1); s12.push_back(C.s12); }
        if (!Optimizer::OptimizeSim3Batch(&cases[0].kf1, kf2, matches, s12, cases[0].th2, cases[0].fix_scale != 0, ret)) {
            std::fprintf(stderr, "OptimizeSim3Batch failed: %s\n", ORBmatcher::LastError());
            return 1;
        }
        for (int b = 0; b < ncases; ++b) { cases[b].matches1 = matches[b]; cases[b].s12 = s12[b]; }
    } else {
        for (int b = 0; b < ncases; ++b) {
            Case& C = cases[b];
            ret[b] = Optimizer::OptimizeSim3_cam1(&C.kf1, &C.kf2, C.matches1, C.s12, C.th2, C.fix_scale != 0);
        }
    }
    for (int b = 0; b < ncases; ++b) {
        const Case& C = cases[b];
        std::printf("%d", ret[b]);
        const g2o::Quaterniond& q = C.s12.rotation();
        std::printf(" %016llx %016llx %016llx %016llx", bits(q.x()), bits(q.y()), bits(q.z()), bits(q.w()));
        for (int k = 0; k < 3; ++k) std::printf(" %016llx", bits(C.s12.translation()[k]));
        std::printf(" %016llx ", bits(C.s12.scale()));
        for (MapPoint* p : C.matches1) std::putchar(p ? '1' : '0');
        if (C.matches1.empty()) std::putchar('-');
        std::printf("\n");
    }
    if (ORBmatcher::FailureCount()) { std::fprintf(stderr, "a call failed: %s\n", ORBmatcher::LastError()); return 1; }
    return 0;
}
