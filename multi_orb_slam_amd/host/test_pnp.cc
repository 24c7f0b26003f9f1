// test_pnp.cc -- driver of PnPsolver (host/PnPsolver.h) on stand-in frames and map points read from a text file
// (tests/test_pnp_solver_class.py writes it from worlds of tests/pnp_worlds.py and compares what comes back with the model).
//   test_pnp FILE
// FILE: "nsolvers seed mode" (mode 0: every solver prepares itself on its first iterate; 1: PnPsolver::Prepare over all of them, null
// entries included, in one call), then per solver "present" and, if 1: "protocol extra" (protocol 0: iterate(5, ...) until bNoMore,
// then `extra` calls more -- they run past mRansacMaxIts; 1: find, then `extra` more), the frame "fx fy cx cy nlevels sigma2...
// nfeatures" + per feature "octave x y" (mvKeysUn), then per feature "has bad X Y Z": vpMapPointMatches (has = 0: null).  Floats travel
// as the hexadecimal of their bits.  srand(seed) is called once before anything is drawn.
// Output: "host_below PNP_HOST_BELOW", then per solver: "null", or "quads H a b c d ..." (everything drawn, continuation blocks included) and one line per call
// "call Tcw|- bNoMore nInliers vbInliers".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fstream>
#include <string>
#include "PnPsolver.h"
#include "slam_types.h"

using namespace ORB_SLAM2;

static float rdf(std::istream& in) { std::string s; in >> s; const uint32_t u = (uint32_t)std::stoul(s, nullptr, 16); float f; std::memcpy(&f, &u, 4); return f; }
static unsigned bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

struct Case {
    bool present = false;
    int protocol = 0, extra = 0;
    Frame frame;
    std::vector<MapPoint*> matches;
    PnPsolver* solver = nullptr;
};

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: test_pnp FILE\n"); return 2; }
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
        in >> C.protocol >> C.extra;
        Frame& F = C.frame;
        F.fx = rdf(in); F.fy = rdf(in); F.cx = rdf(in); F.cy = rdf(in);
        int L; in >> L;
        F.mvLevelSigma2.resize(L);
        for (int k = 0; k < L; ++k) F.mvLevelSigma2[k] = rdf(in);
        int n; in >> n;
        F.N = F.N_total = n;
        F.mvKeysUn.resize(n); F.mvpMapPoints.assign(n, nullptr);
        for (int i = 0; i < n; ++i) { in >> F.mvKeysUn[i].octave; F.mvKeysUn[i].pt.x = rdf(in); F.mvKeysUn[i].pt.y = rdf(in); }
        C.matches.assign((size_t)n, nullptr);
        for (int i = 0; i < n; ++i) {
            int has, bad; in >> has >> bad;
            const float X = rdf(in), Y = rdf(in), Z = rdf(in);
            if (!has) continue;
            points.emplace_back();
            MapPoint& P = points.back();
            P.mWorldPos = cv::Mat(3, 1, CV_32F);
            P.mWorldPos.at<float>(0) = X; P.mWorldPos.at<float>(1) = Y; P.mWorldPos.at<float>(2) = Z;
            P.mbBad = bad != 0;
            C.matches[i] = &P;
        }
    }
    if (!in.good()) { std::fprintf(stderr, "short file\n"); return 2; }
    std::printf("host_below %ld\n", PNP_HOST_BELOW);
    srand((unsigned)seed);
    std::vector<PnPsolver*> solvers;
    for (Case& C : cases) {
        if (C.present) {
            C.solver = new PnPsolver(C.frame, C.matches);
            C.solver->SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991);      // as Tracking::Relocalization sets them
        }
        solvers.push_back(C.solver);
    }
    if (mode == 1 && !PnPsolver::Prepare(solvers)) { std::fprintf(stderr, "Prepare failed: %s\n", ORBmatcher::LastError()); return 1; }
    for (Case& C : cases) {
        if (!C.solver) { std::printf("null\n"); continue; }
        std::string lines;
        int calls = 0, after = -1;
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
            if (after < 0 && bNoMore) after = 0;
            else if (after >= 0) ++after;
            if ((after >= 0 && after >= C.extra) || ++calls >= 400) break;
        }
        const std::vector<int32_t>& q = C.solver->DrawnQuads();
        std::printf("quads %d", (int)(q.size() / 4));
        for (int32_t v : q) std::printf(" %d", v);
        std::printf("\n%s", lines.c_str());
    }
    if (ORBmatcher::FailureCount()) { std::fprintf(stderr, "a call failed: %s\n", ORBmatcher::LastError()); return 1; }
    for (PnPsolver* s : solvers) delete s;
    return 0;
}
