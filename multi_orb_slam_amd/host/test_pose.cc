// test_pose.cc -- driver of Optimizer::PoseOptimization (host/Optimizer.h) on stand-in frames read from a text file
// (tests/test_pose_optimization_class.py writes it from worlds of tests/pose_worlds.py and compares what comes back with the model).
//   test_pose FILE [batch]
// FILE: "nframes allcams", then per frame "N N_total", mTcw (16 floats), "fx fy cx cy mbf", mRcam12 (9), mtcam12 (3), "nlevels", the
// inverse level sigma2, then N_total lines "x y octave uright has_point X Y Z".  Floats travel as the hexadecimal of their bits.
// Output per frame: "ret", the pose after the call (16 floats, bits), then mvbOutlier as one string of 0 / 1.
// With `batch` the frames go through PoseOptimizationBatch in one call, otherwise through the reference's signature one by one.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <deque>
#include "Optimizer.h"
#include "slam_types.h"

using namespace ORB_SLAM2;

static float rdf(std::istream& in) { std::string s; in >> s; const uint32_t u = (uint32_t)std::stoul(s, nullptr, 16); float f; std::memcpy(&f, &u, 4); return f; }
static unsigned bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

static void read_frame(std::istream& in, Frame& F, std::deque<MapPoint>& points) {
    int N, Nt;
    in >> N >> Nt;
    F.N = N; F.N_total = Nt; F.N_cam2 = Nt - N;
    cv::Mat T(4, 4, CV_32F);
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) T.at<float>(r, c) = rdf(in);
    F.SetPose(T);
    F.fx = rdf(in); F.fy = rdf(in); F.cx = rdf(in); F.cy = rdf(in); F.mbf = rdf(in);
    F.mRcam12 = cv::Mat(3, 3, CV_32F); F.mtcam12 = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) F.mRcam12.at<float>(r, c) = rdf(in);
    for (int r = 0; r < 3; ++r) F.mtcam12.at<float>(r) = rdf(in);
    int L; in >> L;
    F.mvInvLevelSigma2.resize(L);
    for (int k = 0; k < L; ++k) F.mvInvLevelSigma2[k] = rdf(in);
    F.mvKeysUn_total.resize(Nt); F.mvuRight_total.resize(Nt); F.mvpMapPoints.assign(Nt, nullptr); F.mvbOutlier.assign(Nt, true);
    for (int i = 0; i < Nt; ++i) {
        F.mvKeysUn_total[i].pt.x = rdf(in); F.mvKeysUn_total[i].pt.y = rdf(in);
        in >> F.mvKeysUn_total[i].octave;
        F.mvuRight_total[i] = rdf(in);
        int has; in >> has;
        const float X = rdf(in), Y = rdf(in), Z = rdf(in);
        if (has) {
            points.emplace_back();
            points.back().mWorldPos = cv::Mat(3, 1, CV_32F);
            points.back().mWorldPos.at<float>(0) = X; points.back().mWorldPos.at<float>(1) = Y; points.back().mWorldPos.at<float>(2) = Z;
            F.mvpMapPoints[i] = &points.back();
        }
    }
    F.mvKeysUn.assign(F.mvKeysUn_total.begin(), F.mvKeysUn_total.begin() + N);
    F.mvuRight.assign(F.mvuRight_total.begin(), F.mvuRight_total.begin() + N);
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: test_pose FILE [batch]\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in.good()) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    const bool batch = argc > 2 && std::strcmp(argv[2], "batch") == 0;
    int nframes, allcams;
    in >> nframes >> allcams;
    std::deque<Frame> frames((size_t)nframes);
    std::deque<MapPoint> points;
    for (Frame& F : frames) read_frame(in, F, points);
    if (!in.good()) { std::fprintf(stderr, "short file\n"); return 2; }
    std::vector<int> ret((size_t)nframes);
    if (batch) {
        std::vector<Frame*> v;
        for (Frame& F : frames) v.push_back(&F);
        if (!Optimizer::PoseOptimizationBatch(v, allcams != 0, ret)) { std::fprintf(stderr, "PoseOptimizationBatch failed\n"); return 1; }
    } else {
        int k = 0;
        for (Frame& F : frames) ret[k++] = allcams ? Optimizer::PoseOptimization(&F, true) : Optimizer::PoseOptimization(&F);
        if (ORBmatcher::FailureCount()) { std::fprintf(stderr, "a call failed: %s\n", ORBmatcher::LastError()); return 1; }
    }
    int k = 0;
    for (Frame& F : frames) {
        std::printf("%d", ret[k++]);
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) std::printf(" %08x", bits(F.mTcw.at<float>(r, c)));
        std::string s;
        for (size_t i = 0; i < F.mvbOutlier.size(); ++i) s += F.mvbOutlier[i] ? '1' : '0';
        std::printf(" %s\n", s.c_str());
    }
    return 0;
}
