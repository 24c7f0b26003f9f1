// test_new_points.cc -- driver of TriangulateMatches (host/NewMapPoints.h) on stand-in keyframes read from a text file
// (tests/test_new_map_points_class.py writes it from a world of tests/triangulate_worlds.py and compares what comes back with the model).
//   test_new_points FILE
// FILE: "npairs istrian0 istrian1", then two keyframes -- "n N", Tcw (12 floats), Tcw_cam2 (12), "fx fy cx cy invfx invfy mbf mb
// scaleFactor", "nlevels", the scale factors, the level sigma2, mRcam12 (9), mtcam12 (3), n lines "x y xd yd octave uright depth cam" --
// then npairs lines "idx1 idx2".  Floats travel as the hexadecimal of their bits.
// Output: the camera centres and Twc the class read from each keyframe (bits), then per pair "outcome accepted x y z" (bits, or - - -).
#include <cstdio>
#include <cstring>
#include <fstream>
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

static void read_keyframe(std::istream& in, KeyFrame& K) {
    int n, N;
    in >> n >> N;
    K.N = N; K.N_cam2 = n - N; K.N_total = n;
    K.Tcw = pose(in); K.Tcw_cam2 = pose(in);
    K.fx = rdf(in); K.fy = rdf(in); K.cx = rdf(in); K.cy = rdf(in); K.invfx = rdf(in); K.invfy = rdf(in); K.mbf = rdf(in); K.mb = rdf(in);
    K.mfScaleFactor = rdf(in);
    int L; in >> L;
    K.mnScaleLevels = L; K.mvScaleFactors.resize(L); K.mvLevelSigma2.resize(L);
    for (int k = 0; k < L; ++k) K.mvScaleFactors[k] = rdf(in);
    for (int k = 0; k < L; ++k) K.mvLevelSigma2[k] = rdf(in);
    K.mRcam12 = cv::Mat(3, 3, CV_32F); K.mtcam12 = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) K.mRcam12.at<float>(r, c) = rdf(in);
    for (int r = 0; r < 3; ++r) K.mtcam12.at<float>(r) = rdf(in);
    K.mvKeysUn_total.resize(n); K.mvKeys_total.resize(n); K.mvuRight_total.resize(n); K.mvDepth_total.resize(n);
    for (int i = 0; i < n; ++i) {
        K.mvKeysUn_total[i].pt.x = rdf(in); K.mvKeysUn_total[i].pt.y = rdf(in);
        K.mvKeys_total[i].pt.x = rdf(in); K.mvKeys_total[i].pt.y = rdf(in);
        int octave; in >> octave;
        K.mvKeysUn_total[i].octave = K.mvKeys_total[i].octave = octave;
        K.mvuRight_total[i] = rdf(in); K.mvDepth_total[i] = rdf(in);
        int cam; in >> cam;
        K.keypoint_to_cam[(size_t)i] = cam;
    }
}

static void print_read(const char* name, KeyFrame& K) {
    const cv::Mat c1 = K.GetCameraCenter(), c2 = K.GetCameraCenter_cam2(), Twc = K.GetPoseInverse();
    std::printf("%s", name);
    for (int k = 0; k < 3; ++k) std::printf(" %08x", bits(c1.at<float>(k)));
    for (int k = 0; k < 3; ++k) std::printf(" %08x", bits(c2.at<float>(k)));
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) std::printf(" %08x", bits(Twc.at<float>(r, c)));
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: test_new_points FILE\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in.good()) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int npairs, e0, e1;
    in >> npairs >> e0 >> e1;
    KeyFrame K1, K2;
    read_keyframe(in, K1); read_keyframe(in, K2);
    std::vector<std::pair<size_t, size_t> > pairs((size_t)npairs);
    for (int i = 0; i < npairs; ++i) in >> pairs[i].first >> pairs[i].second;
    if (!in.good()) { std::fprintf(stderr, "short file\n"); return 2; }
    std::vector<bool> istrian(2); istrian[0] = e0 != 0; istrian[1] = e1 != 0;
    ORBmatcher matcher(0.6f, false);
    std::vector<TriangulatedPair> out;
    if (!TriangulateMatches(matcher, &K1, &K2, pairs, istrian, out)) { std::fprintf(stderr, "TriangulateMatches failed\n"); return 1; }
    print_read("kf1", K1); print_read("kf2", K2);
    for (size_t i = 0; i < out.size(); ++i) {
        if (out[i].x3D.empty()) std::printf("%d %d - - -\n", out[i].outcome, (int)out[i].accepted);
        else std::printf("%d %d %08x %08x %08x\n", out[i].outcome, (int)out[i].accepted, bits(out[i].x3D.at<float>(0)), bits(out[i].x3D.at<float>(1)), bits(out[i].x3D.at<float>(2)));
    }
    return 0;
}
