// test_local_ba.cc -- driver of Optimizer::LocalBundleAdjustment (host/Optimizer.h, host/LocalBA.cc) on a stand-in map read from a text
// file (tests/test_local_ba_class.py writes it from a world of tests/lba_worlds.py and compares what comes back with its transcription of
// steps 1-4 and 12-13 around the library's call).
//   test_local_ba FILE
// FILE: "nkf npt current stop" (stop: -1 no flag, 0 / 1 the flag's value), mRcam12 (9), mtcam12 (3), "nlevels", the inverse level
// sigma2, the scale factors; per keyframe "mnId bad", "fx fy cx cy mbf", Tcw (16), "ncov" and the covisible keyframes (indices, best
// first), "nfeat" and per feature "x y octave uright cam point" (point: an index or -1); per point "mnId bad X Y Z ref" (ref: the index of
// its reference keyframe).  Floats travel as the hexadecimal of their bits.
// Output: per keyframe "KF mnId mnBALocalForKF mnBAFixedForKF", its pose (16 floats, bits) and its map-point matches (indices, -1 none);
// per point "MP mnId mnBALocalForKF", its position (3 floats, bits) and the mnIds of the keyframes that still observe it; then the calls
// the function made on the map, in order: "CALL what mnId mnId" for lock, EraseMapPointMatch (keyframe, point), EraseObservation (point,
// keyframe), SetPose, SetWorldPos, SetNormalAndDepth, unlock.
#include <cstdio>
#include <cstring>
#include <deque>
#include <fstream>
#include <map>
#include <string>
#include "Optimizer.h"
#include "slam_types.h"

using namespace ORB_SLAM2;

static float rdf(std::istream& in) { std::string s; in >> s; const uint32_t u = (uint32_t)std::stoul(s, nullptr, 16); float f; std::memcpy(&f, &u, 4); return f; }
static unsigned bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: test_local_ba FILE\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in.good()) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int nkf, npt, current, stop;
    in >> nkf >> npt >> current >> stop;
    cv::Mat Rcam12(3, 3, CV_32F), tcam12(3, 1, CV_32F);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) Rcam12.at<float>(r, c) = rdf(in);
    for (int r = 0; r < 3; ++r) tcam12.at<float>(r) = rdf(in);
    int L; in >> L;
    std::vector<float> inv_sigma2(L), scale(L);
    for (int k = 0; k < L; ++k) inv_sigma2[k] = rdf(in);
    for (int k = 0; k < L; ++k) scale[k] = rdf(in);
    std::deque<KeyFrame> kfs((size_t)nkf);
    std::deque<MapPoint> mps((size_t)npt);
    std::vector<std::vector<int> > cov((size_t)nkf), feat_point((size_t)nkf);
    for (int i = 0; i < nkf; ++i) {
        KeyFrame& K = kfs[i];
        int bad; in >> K.mnId >> bad; K.mbBad = bad != 0;
        K.fx = rdf(in); K.fy = rdf(in); K.cx = rdf(in); K.cy = rdf(in); K.mbf = rdf(in);
        K.Tcw = cv::Mat(4, 4, CV_32F);
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) K.Tcw.at<float>(r, c) = rdf(in);
        K.Tcw_cam2 = K.Tcw.clone();
        K.mRcam12 = Rcam12.clone(); K.mtcam12 = tcam12.clone();
        K.mvInvLevelSigma2 = inv_sigma2; K.mvScaleFactors = scale; K.mnScaleLevels = L;
        int nc; in >> nc; cov[i].resize(nc);
        for (int k = 0; k < nc; ++k) in >> cov[i][k];
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
    for (int i = 0; i < nkf; ++i) for (int k : cov[i]) kfs[i].mvpOrderedConnectedKeyFrames.push_back(&kfs[k]);
    std::map<MapPoint*, int> index_of;
    for (int l = 0; l < npt; ++l) {
        MapPoint& M = mps[l];
        int bad, ref; in >> M.mnId >> bad; M.mbBad = bad != 0;
        M.mWorldPos = cv::Mat(3, 1, CV_32F);
        for (int k = 0; k < 3; ++k) M.mWorldPos.at<float>(k) = rdf(in);
        in >> ref; M.mpRefKF = &kfs[ref];
        M.mNormalVector = cv::Mat::zeros(3, 1, CV_32F);
        M.nObs = 0;
        index_of[&M] = l;
    }
    if (!in.good()) { std::fprintf(stderr, "the file ends early\n"); return 2; }
    for (int i = 0; i < nkf; ++i)
        for (size_t f = 0; f < feat_point[i].size(); ++f)
            if (feat_point[i][f] >= 0) { kfs[i].mvpMapPoints[f] = &mps[feat_point[i][f]]; mps[feat_point[i][f]].AddObservation(&kfs[i], f); }

    Map map;
    bool flag = stop > 0;
    std::vector<CallLogEntry> log;
    CallLog() = &log;
    Optimizer::LocalBundleAdjustment(&kfs[current], stop < 0 ? nullptr : &flag, &map);
    CallLog() = nullptr;

    for (int i = 0; i < nkf; ++i) {
        KeyFrame& K = kfs[i];
        std::printf("KF %lu %lu %lu", K.mnId, K.mnBALocalForKF, K.mnBAFixedForKF);
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) std::printf(" %08x", bits(K.Tcw.at<float>(r, c)));
        for (MapPoint* p : K.mvpMapPoints) std::printf(" %d", p ? index_of[p] : -1);
        std::printf("\n");
    }
    for (int l = 0; l < npt; ++l) {
        MapPoint& M = mps[l];
        std::printf("MP %lu %lu", M.mnId, M.mnBALocalForKF);
        for (int k = 0; k < 3; ++k) std::printf(" %08x", bits(M.mWorldPos.at<float>(k)));
        for (const auto& o : M.mObservations) std::printf(" %lu", o.first->mnId);   // (sorted by the test: the map's order is addresses)
        std::printf("\n");
    }
    for (const CallLogEntry& c : log) std::printf("CALL %s %lu %lu\n", c.what, c.a, c.b);
    return 0;
}
