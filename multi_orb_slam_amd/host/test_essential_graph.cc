// test_essential_graph.cc -- driver of Optimizer::OptimizeEssentialGraph (host/Optimizer.h, host/EssentialGraph.cc) on a stand-in map
// read from two text files (tests/test_essential_graph_class.py writes them and compares what comes back with its transcription of
// steps 2-4 and 6-7 around the library's call).
//   test_essential_graph MAP GRAPH
// MAP: the format of test_local_ba.cc (keyframes with features, points with their reference keyframe).  GRAPH:
//   loop current fix_scale max_kf_id                       (keyframe positions in MAP; Map::GetMaxKFid())
//   per keyframe: parent (-1: none), n children..., n loop edges..., n (covisible weight)... in descending weight (camera 1)
//   n, then n x (keyframe, 8 doubles as bits): CorrectedSim3;  the same: NonCorrectedSim3
//   n, then n x (keyframe, m, m keyframes): LoopConnections
//   per point: mnCorrectedByKF mnCorrectedReference
// The keyframes live in ONE vector, so the order of their heap addresses -- which the function follows when it iterates
// LoopConnections and the sets -- is their order in MAP.
// Output: per keyframe "KF mnId" and its pose (16 floats, bits); per point "MP mnId" and its position (3 floats); then the calls the
// function made on the map, in order.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include "Optimizer.h"
#include "slam_types.h"

using namespace ORB_SLAM2;

static float rdf(std::istream& in) { std::string s; in >> s; const uint32_t u = (uint32_t)std::stoul(s, nullptr, 16); float f; std::memcpy(&f, &u, 4); return f; }
static double rdd(std::istream& in) { std::string s; in >> s; const uint64_t u = (uint64_t)std::stoull(s, nullptr, 16); double d; std::memcpy(&d, &u, 8); return d; }
static unsigned bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static void print_mat(const cv::Mat& M, int rows, int cols) {
    for (int r = 0; r < rows; ++r) for (int c = 0; c < cols; ++c) std::printf(" %08x", M.empty() ? 0u : bits(M.at<float>(r, c)));
}
static g2o::Sim3 rd_sim3(std::istream& in) {
    double v[8];
    for (int k = 0; k < 8; ++k) v[k] = rdd(in);
    return g2o::Sim3(g2o::Quaterniond(v[3], v[0], v[1], v[2]), g2o::Vector3d(v[4], v[5], v[6]), v[7]);
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: test_essential_graph MAP GRAPH\n"); return 2; }
    std::ifstream in(argv[1]), gr(argv[2]);
    if (!in.good() || !gr.good()) { std::fprintf(stderr, "cannot open %s or %s\n", argv[1], argv[2]); return 2; }
    int nkf, npt, unused_current, unused_stop;
    in >> nkf >> npt >> unused_current >> unused_stop;
    for (int k = 0; k < 12; ++k) (void)rdf(in);             // (mRcam12, mtcam12 of the local BA's format: not used here)
    int L; in >> L;
    std::vector<float> inv_sigma2(L), scale(L);
    for (int k = 0; k < L; ++k) inv_sigma2[k] = rdf(in);
    for (int k = 0; k < L; ++k) scale[k] = rdf(in);
    std::vector<KeyFrame> kfs((size_t)nkf);
    std::vector<MapPoint> mps((size_t)npt);
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
        for (int k = 0, skip; k < nc; ++k) in >> skip;
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
    if (!in.good()) { std::fprintf(stderr, "the map file ends early\n"); return 2; }
    for (int i = 0; i < nkf; ++i)
        for (size_t f = 0; f < feat_point[i].size(); ++f)
            if (feat_point[i][f] >= 0) { kfs[i].mvpMapPoints[f] = &mps[feat_point[i][f]]; mps[feat_point[i][f]].AddObservation(&kfs[i], f); }

    int loop, current, fix_scale;
    Map map;
    gr >> loop >> current >> fix_scale >> map.mnMaxKFid;
    for (int i = 0; i < nkf; ++i) {
        KeyFrame& K = kfs[i];
        int parent, n;
        gr >> parent; K.mpParent = parent < 0 ? nullptr : &kfs[parent];
        gr >> n; for (int k = 0, c; k < n; ++k) { gr >> c; K.mspChildrens.insert(&kfs[c]); }
        gr >> n; for (int k = 0, c; k < n; ++k) { gr >> c; K.mspLoopEdges.insert(&kfs[c]); }
        gr >> n;
        for (int k = 0, c, w; k < n; ++k) {
            gr >> c >> w;
            K.mvpOrderedConnectedKeyFrames_cam1.push_back(&kfs[c]); K.mvOrderedWeights_cam1.push_back(w); K.mConnectedKeyFrameWeights_cam1[&kfs[c]] = w;
        }
    }
    LoopClosing::KeyFrameAndPose Corrected, NonCorrected;
    for (LoopClosing::KeyFrameAndPose* poses : {&Corrected, &NonCorrected}) {
        int n; gr >> n;
        for (int k = 0, c; k < n; ++k) { gr >> c; (*poses)[&kfs[c]] = rd_sim3(gr); }
    }
    std::map<KeyFrame*, std::set<KeyFrame*> > LoopConnections;
    {
        int n; gr >> n;
        for (int k = 0, c, m; k < n; ++k) { gr >> c >> m; std::set<KeyFrame*>& s = LoopConnections[&kfs[c]]; for (int q = 0, d; q < m; ++q) { gr >> d; s.insert(&kfs[d]); } }
    }
    for (int l = 0; l < npt; ++l) gr >> mps[l].mnCorrectedByKF >> mps[l].mnCorrectedReference;
    if (!gr.good()) { std::fprintf(stderr, "the graph file ends early\n"); return 2; }

    for (int i = 0; i < nkf; ++i) map.mvpKeyFrames.push_back(&kfs[i]);
    for (int l = 0; l < npt; ++l) map.mvpMapPoints.push_back(&mps[l]);
    std::vector<CallLogEntry> log;
    CallLog() = &log;
    Optimizer::OptimizeEssentialGraph(&map, &kfs[loop], &kfs[current], NonCorrected, Corrected, LoopConnections, fix_scale != 0);
    CallLog() = nullptr;

    for (int i = 0; i < nkf; ++i) { std::printf("KF %lu", kfs[i].mnId); print_mat(kfs[i].Tcw, 4, 4); std::printf("\n"); }
    for (int l = 0; l < npt; ++l) { std::printf("MP %lu", mps[l].mnId); print_mat(mps[l].mWorldPos, 3, 1); std::printf("\n"); }
    for (const CallLogEntry& c : log) std::printf("CALL %s %lu %lu\n", c.what, c.a, c.b);
    return 0;
}
