// test_global_ba.cc -- driver of Optimizer::GlobalBundleAdjustemnt / BundleAdjustment (host/Optimizer.h, host/GlobalBA.cc) on a stand-in
// map read from a text file (tests/test_global_ba_class.py writes it from a world of tests/gba_worlds.py and compares what comes back
// with its transcription of the filtering and the recovery around the library's call).
//   test_global_ba FILE ITERATIONS ROBUST
// FILE: the format of test_local_ba.cc; its third number is nLoopKF here (0: the results go to SetPose / SetWorldPos, otherwise to
// mTcwGBA / mPosGBA / mnBAGlobalForKF).  CalibMatrix is built from the file's mRcam12 (rows 0..2) and mtcam12 (row 3).
// Output: per keyframe "KF mnId mnBAGlobalForKF", its pose and its mTcwGBA (16 floats each, bits; zeros where mTcwGBA is empty); per
// point "MP mnId mnBAGlobalForKF", its position and its mPosGBA (3 floats each); then the calls the function made on the map, in order.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fstream>
#include <string>
#include "Optimizer.h"
#include "slam_types.h"

using namespace ORB_SLAM2;

static float rdf(std::istream& in) { std::string s; in >> s; const uint32_t u = (uint32_t)std::stoul(s, nullptr, 16); float f; std::memcpy(&f, &u, 4); return f; }
static unsigned bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static void print_mat(const cv::Mat& M, int rows, int cols) {
    for (int r = 0; r < rows; ++r) for (int c = 0; c < cols; ++c) std::printf(" %08x", M.empty() ? 0u : bits(M.at<float>(r, c)));
}

int main(int argc, char** argv) {
    if (argc < 4) { std::fprintf(stderr, "usage: test_global_ba FILE ITERATIONS ROBUST\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in.good()) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    const int iterations = std::atoi(argv[2]);
    const bool robust = std::atoi(argv[3]) != 0;
    int nkf, npt, loop_kf, stop;
    in >> nkf >> npt >> loop_kf >> stop;
    cv::Mat Calib = cv::Mat::zeros(4, 3, CV_32F);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) Calib.at<float>(r, c) = rdf(in);
    for (int r = 0; r < 3; ++r) Calib.at<float>(3, r) = rdf(in);
    int L; in >> L;
    std::vector<float> inv_sigma2(L), scale(L);
    for (int k = 0; k < L; ++k) inv_sigma2[k] = rdf(in);
    for (int k = 0; k < L; ++k) scale[k] = rdf(in);
    std::deque<KeyFrame> kfs((size_t)nkf);
    std::deque<MapPoint> mps((size_t)npt);
    std::vector<std::vector<int> > feat_point((size_t)nkf);
    for (int i = 0; i < nkf; ++i) {
        KeyFrame& K = kfs[i];
        int bad; in >> K.mnId >> bad; K.mbBad = bad != 0;
        K.fx = rdf(in); K.fy = rdf(in); K.cx = rdf(in); K.cy = rdf(in); K.mbf = rdf(in);
        K.Tcw = cv::Mat(4, 4, CV_32F);
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) K.Tcw.at<float>(r, c) = rdf(in);
        K.Tcw_cam2 = K.Tcw.clone();
        K.mvInvLevelSigma2 = inv_sigma2; K.mvScaleFactors = scale; K.mnScaleLevels = L;
        int nc; in >> nc;
        for (int k = 0, skip; k < nc; ++k) in >> skip;     // (the covisibility list of the local BA's format: not used here)
        int nf; in >> nf;
        K.N_total = nf; K.N = nf;
        K.mvKeysUn_total.resize(nf); K.mvuRight_total.resize(nf); K.mvpMapPoints.assign(nf, nullptr); feat_point[i].resize(nf);
        for (int f = 0; f < nf; ++f) {
            K.mvKeysUn_total[f].pt.x = rdf(in); K.mvKeysUn_total[f].pt.y = rdf(in);
            in >> K.mvKeysUn_total[f].octave;
            K.mvuRight_total[f] = rdf(in);
            int cam; in >> cam >> feat_point[i][f];
            K.keypoint_to_cam[(size_t)f] = cam; K.cont_idx_to_local_cam_idx[(size_t)f] = f;
        }
    }
    for (int l = 0; l < npt; ++l) {
        MapPoint& M = mps[l];
        int bad, ref; in >> M.mnId >> bad; M.mbBad = bad != 0;
        M.mWorldPos = cv::Mat(3, 1, CV_32F);
        for (int k = 0; k < 3; ++k) M.mWorldPos.at<float>(k) = rdf(in);
        in >> ref; M.mpRefKF = &kfs[ref];
        M.mNormalVector = cv::Mat::zeros(3, 1, CV_32F);
        M.nObs = 0;
    }
    if (!in.good()) { std::fprintf(stderr, "the file ends early\n"); return 2; }
    for (int i = 0; i < nkf; ++i)
        for (size_t f = 0; f < feat_point[i].size(); ++f)
            if (feat_point[i][f] >= 0) { kfs[i].mvpMapPoints[f] = &mps[feat_point[i][f]]; mps[feat_point[i][f]].AddObservation(&kfs[i], f); }

    Map map;
    for (int i = 0; i < nkf; ++i) map.mvpKeyFrames.push_back(&kfs[i]);
    for (int l = 0; l < npt; ++l) map.mvpMapPoints.push_back(&mps[l]);
    bool flag = stop > 0;
    std::vector<CallLogEntry> log;
    CallLog() = &log;
    Optimizer::GlobalBundleAdjustemnt(&map, iterations, stop < 0 ? nullptr : &flag, (unsigned long)loop_kf, robust, Calib);
    CallLog() = nullptr;

    for (int i = 0; i < nkf; ++i) {
        KeyFrame& K = kfs[i];
        std::printf("KF %lu %lu", K.mnId, K.mnBAGlobalForKF);
        print_mat(K.Tcw, 4, 4); print_mat(K.mTcwGBA, 4, 4);
        std::printf("\n");
    }
    for (int l = 0; l < npt; ++l) {
        MapPoint& M = mps[l];
        std::printf("MP %lu %lu", M.mnId, M.mnBAGlobalForKF);
        print_mat(M.mWorldPos, 3, 1); print_mat(M.mPosGBA, 3, 1);
        std::printf("\n");
    }
    for (const CallLogEntry& c : log) std::printf("CALL %s %lu %lu\n", c.what, c.a, c.b);
    return 0;
}
