// test_sim3.cc -- driver of Sim3Solver (host/Sim3Solver.h) on stand-in keyframes and map points read from a text file
// (tests/test_sim3_solver_class.py writes it from worlds of tests/sim3_worlds.py and compares what comes back with the model).
//   test_sim3 FILE
// FILE: "nsolvers seed mode" (mode 0: every solver prepares itself on its first iterate; 1: Sim3Solver::Prepare over all of them, null
// entries included, in one call), then per solver "present" and, if 1: "fix_scale min_inliers max_its protocol" (protocol 0:
// iterate(5, ...) until bNoMore; 1: find), CalibMatrix (4x3, 12 floats), two keyframes "Tcw (16) fx fy cx cy nlevels sigma2...
// nfeatures" + per feature "octave cam", then "mN1" and per entry "has1 bad1 idx1 X Y Z has2 bad2 idx2 X Y Z": keyframe 1's map point at
// that feature and vpMatched12's (has = 0: null; idx = the point's index in its keyframe or -1).  Floats travel as the hexadecimal of
// their bits.  srand(seed) is called once before anything is drawn.
// Output per solver: "null", or "triples H a b c ...", one line per call "call T12|- bNoMore nInliers vbInliers", and
// "best R t s|-" from the three getters.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fstream>
#include <string>
#include "Sim3Solver.h"
#include "slam_types.h"

using namespace ORB_SLAM2;

static float rdf(std::istream& in) { std::string s; in >> s; const uint32_t u = (uint32_t)std::stoul(s, nullptr, 16); float f; std::memcpy(&f, &u, 4); return f; }
static unsigned bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

static void read_keyframe(std::istream& in, KeyFrame& K) {
    K.Tcw = cv::Mat(4, 4, CV_32F);
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) K.Tcw.at<float>(r, c) = rdf(in);
    K.mK = cv::Mat::eye(3, 3, CV_32F);
    K.fx = rdf(in); K.fy = rdf(in); K.cx = rdf(in); K.cy = rdf(in);
    K.mK.at<float>(0, 0) = K.fx; K.mK.at<float>(1, 1) = K.fy; K.mK.at<float>(0, 2) = K.cx; K.mK.at<float>(1, 2) = K.cy;
    int L; in >> L;
    K.mvLevelSigma2.resize(L);
    for (int k = 0; k < L; ++k) K.mvLevelSigma2[k] = rdf(in);
    int n; in >> n;
    K.N = K.N_total = n;
    K.mvKeysUn.resize(n); K.mvpMapPoints.assign(n, nullptr);
    for (int i = 0; i < n; ++i) { int cam; in >> K.mvKeysUn[i].octave >> cam; K.keypoint_to_cam[(size_t)i] = cam; }
}

static MapPoint* read_point(std::istream& in, KeyFrame* K, std::deque<MapPoint>& points) {
    int has, bad, idx;
    in >> has >> bad >> idx;
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
    bool present = false;
    int fix_scale = 0, min_inliers = 0, max_its = 0, protocol = 0;
    cv::Mat calib;
    KeyFrame kf1, kf2;
    std::vector<MapPoint*> matched12;
    Sim3Solver* solver = nullptr;
};

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: test_sim3 FILE\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in.good()) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int nsolvers, seed, mode;
    in >> nsolvers >> seed >> mode;
    std::deque<Case> cases((size_t)nsolvers);
    std::deque<MapPoint> points;
    for (Case& C : cases) {
        int present; in >> present;
        C.present = present != 0;
        if (!C.present) continue;
        in >> C.fix_scale >> C.min_inliers >> C.max_its >> C.protocol;
        C.calib = cv::Mat(4, 3, CV_32F);
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 3; ++c) C.calib.at<float>(r, c) = rdf(in);
        read_keyframe(in, C.kf1);
        read_keyframe(in, C.kf2);
        int mN1; in >> mN1;
        C.matched12.assign((size_t)mN1, nullptr);
        for (int i = 0; i < mN1; ++i) {
            C.kf1.mvpMapPoints[i] = read_point(in, &C.kf1, points);
            C.matched12[i] = read_point(in, &C.kf2, points);
        }
    }
    if (!in.good()) { std::fprintf(stderr, "short file\n"); return 2; }
    srand((unsigned)seed);
    std::vector<Sim3Solver*> solvers;
    for (Case& C : cases) {
        if (C.present) {
            C.solver = new Sim3Solver(&C.kf1, &C.kf2, C.matched12, C.calib, C.fix_scale != 0);
            C.solver->SetRansacParameters(0.99, C.min_inliers, C.max_its);
        }
        solvers.push_back(C.solver);
    }
    if (mode == 1 && !Sim3Solver::Prepare(solvers)) { std::fprintf(stderr, "Prepare failed: %s\n", ORBmatcher::LastError()); return 1; }
    for (Case& C : cases) {
        if (!C.solver) { std::printf("null\n"); continue; }
        std::string lines;
        int calls = 0;
        for (;;) {
            std::vector<bool> vbInliers;
            int nInliers = -1;
            bool bNoMore = C.protocol == 1;
            const cv::Mat T = C.protocol == 1 ? C.solver->find(vbInliers, nInliers) : C.solver->iterate(5, bNoMore, vbInliers, nInliers);
            char buf[64];
            lines += "call";
            if (T.empty()) lines += " -";
            else for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) { std::snprintf(buf, sizeof buf, " %08x", bits(T.at<float>(r, c))); lines += buf; }
            std::snprintf(buf, sizeof buf, " %d %d ", bNoMore ? 1 : 0, nInliers);
            lines += buf;
            for (size_t i = 0; i < vbInliers.size(); ++i) lines += vbInliers[i] ? '1' : '0';
            if (vbInliers.empty()) lines += '-';
            lines += "\n";
            if (bNoMore || ++calls >= 400) break;
        }
        // (the triples exist from the first iterate on)
        const std::vector<int32_t>& t = C.solver->DrawnTriples();
        std::printf("triples %d", (int)(t.size() / 3));
        for (int32_t v : t) std::printf(" %d", v);
        std::printf("\n%s", lines.c_str());
        const cv::Mat R = C.solver->GetEstimatedRotation(), tr = C.solver->GetEstimatedTranslation();
        if (R.empty()) std::printf("best -\n");
        else {
            std::printf("best");
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) std::printf(" %08x", bits(R.at<float>(r, c)));
            for (int r = 0; r < 3; ++r) std::printf(" %08x", bits(tr.at<float>(r)));
            std::printf(" %08x\n", bits(C.solver->GetEstimatedScale()));
        }
    }
    if (ORBmatcher::FailureCount()) { std::fprintf(stderr, "a call failed: %s\n", ORBmatcher::LastError()); return 1; }
    for (Sim3Solver* s : solvers) delete s;
    return 0;
}
