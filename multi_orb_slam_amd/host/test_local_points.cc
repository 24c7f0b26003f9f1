// test_local_points.cc -- driver of SearchLocalPoints (host/LocalMapSearch.h) for tests/test_gpu_local_points.py and
// tools/local_points_bench.py.
//
//   test_local_points check WORLD.bin OUT.bin   Tracking::SearchLocalPoints twice on two copies of the world: through the class
//                                               (the point table in HBM, frustum test + search in one device call) and through the
//                                               host restatement (Frame::isInFrustum per point on the host, then the existing
//                                               ORBmatcher::SearchByProjection(F, points, th)).  Every scratch field, mnVisible,
//                                               mnLastFrameSeen, F.mvpMapPoints and both counts are compared; then the class runs a
//                                               second frame on a slightly changed map (only the changed rows may be sent).  OUT.bin
//                                               receives the class path's results of the first call for the caller's own checks.
//   test_local_points time  WORLD.bin SECONDS   the two alternated in one process, five pairs, SECONDS per leg, the table resident
//                                               and unchanged between calls; one JSON line per leg: calls, microseconds per call
//
// WORLD.bin (little endian): int32 magic, N (camera 1), N2 (camera 2), npts, npre; float x[n], y[n], angle[n], uright[n]; int32 octave[n];
// uint8 desc1[N*32], desc2[N2*32]; float scale[8], Tcw[16], fx, fy, cx, cy, mbf, minX, minY, maxX, maxY, logScaleFactor, th;
// npts x {orbm_point (68 bytes), int32 bad}; npre x {int32 feature, int32 point}: what F.mvpMapPoints holds before the call.
// OUT.bin: int32 nToMatch, nmatches; npts x {int32 inView, float projX, projY, projXR, viewCos, int32 level, int32 mnVisible};
// N x int32 point index in F.mvpMapPoints (-1: none).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/orbm.h"
#include "LocalMapSearch.h"

using namespace ORB_SLAM2;

namespace {

struct World {
    Frame F;
    std::vector<MapPoint> pts;
    std::vector<MapPoint*> vp;
    std::vector<std::pair<int, int>> pre;
    float th = 3;
    void place() {   // F.mvpMapPoints as before a call
        F.mvpMapPoints.assign(F.N_total, nullptr);
        for (auto& p : pre) F.mvpMapPoints[p.first] = &pts[p.second];
    }
};

bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
template <class T> bool rdv(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return rd(f, v.data(), n * sizeof(T)); }

bool load(const char* path, World& w) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return false; }
    int32_t h[5];
    if (!rd(f, h, sizeof h) || h[0] != 0x4C505731 || h[1] < 0 || h[2] < 0 || h[3] < 0 || h[4] < 0) { fprintf(stderr, "bad header\n"); fclose(f); return false; }
    Frame& F = w.F;
    F.N = h[1]; F.N_cam2 = h[2]; F.N_total = F.N + F.N_cam2;
    const int n = F.N_total, npts = h[3], npre = h[4];
    std::vector<float> x, y, ang, ur; std::vector<int32_t> oct;
    bool ok = rdv(f, x, n) && rdv(f, y, n) && rdv(f, ang, n) && rdv(f, ur, n) && rdv(f, oct, n);
    F.mvKeys_total.resize(n); F.mvKeysUn_total.resize(n); F.mvuRight_total = ur;
    for (int g = 0; ok && g < n; ++g) {
        cv::KeyPoint k; k.pt.x = x[g]; k.pt.y = y[g]; k.angle = ang[g]; k.octave = oct[g];
        F.mvKeys_total[g] = k; F.mvKeysUn_total[g] = k;
        F.keypoint_to_cam[g] = g < F.N ? 0 : 1;
        F.cont_idx_to_local_cam_idx[g] = g < F.N ? g : g - F.N;
    }
    F.mvKeysUn.assign(F.mvKeysUn_total.begin(), F.mvKeysUn_total.begin() + F.N);
    F.mvKeys = F.mvKeysUn;
    F.mvuRight.assign(ur.begin(), ur.begin() + F.N);
    F.mDescriptors_total.resize(2);
    for (int c = 0; ok && c < 2; ++c) {
        const int nc = c == 0 ? F.N : F.N_cam2;
        F.mDescriptors_total[c].create(nc > 0 ? nc : 1, 32, CV_8U);
        ok = rd(f, F.mDescriptors_total[c].ptr(0), (size_t)nc * 32);
    }
    F.mDescriptors = F.mDescriptors_total[0];
    F.mvbOutlier.assign(n, false);
    float T[16], c[11];
    ok = ok && rdv(f, F.mvScaleFactors, 8) && rd(f, T, sizeof T) && rd(f, c, sizeof c);
    if (!ok) { fclose(f); return false; }
    cv::Mat Tcw = cv::Mat::eye(4, 4, CV_32F);
    for (int i = 0; i < 16; ++i) Tcw.at<float>(i / 4, i % 4) = T[i];
    F.SetPose(Tcw);
    F.fx = c[0]; F.fy = c[1]; F.cx = c[2]; F.cy = c[3]; F.mbf = c[4]; F.mb = F.mbf / F.fx;
    F.mnMinX = c[5]; F.mnMinY = c[6]; F.mnMaxX = c[7]; F.mnMaxY = c[8];
    F.mfLogScaleFactor = c[9]; F.mnScaleLevels = 8; w.th = c[10];
    w.pts.resize(npts); w.vp.resize(npts);
    for (int i = 0; i < npts; ++i) {
        orbm_point p; int32_t bad;
        if (!rd(f, &p, sizeof p) || !rd(f, &bad, 4)) { fclose(f); return false; }
        MapPoint& mp = w.pts[i];
        mp.mWorldPos = cv::Mat(3, 1, CV_32F); mp.mNormalVector = cv::Mat(3, 1, CV_32F); mp.mDescriptor = cv::Mat(1, 32, CV_8U);
        for (int k = 0; k < 3; ++k) { mp.mWorldPos.at<float>(k) = p.pos[k]; mp.mNormalVector.at<float>(k) = p.normal[k]; }
        mp.mfMinDistance = p.min_dist; mp.mfMaxDistance = p.max_dist; mp.nObs = p.blocks ? 2 : 0; mp.mbBad = bad != 0;
        std::memcpy(mp.mDescriptor.ptr(0), p.desc, 32);
        mp.mnLastFrameSeen = (long unsigned int)-1;
        w.vp[i] = &mp;
    }
    w.pre.resize(npre);
    for (auto& p : w.pre) {
        int32_t a[2];
        if (!rd(f, a, 8) || a[0] < 0 || a[0] >= n || a[1] < 0 || a[1] >= npts) { fclose(f); return false; }
        p = {a[0], a[1]};
    }
    fclose(f);
    w.place();
    return true;
}

// Tracking::SearchLocalPoints (src/Tracking.cc:1702-1770) as the reference runs it: everything before the search on the host
int host_search_local_points(ORBmatcher& matcher, Frame& F, std::vector<MapPoint*>& local, float th, int* nToMatch) {
    for (MapPoint*& pMP : F.mvpMapPoints) {
        if (!pMP) continue;
        if (pMP->isBad()) { pMP = nullptr; continue; }
        pMP->IncreaseVisible(); pMP->mnLastFrameSeen = F.mnId; pMP->mbTrackInView = false;
    }
    int n = 0;
    for (MapPoint* pMP : local) {
        if (pMP->mnLastFrameSeen == F.mnId || pMP->isBad()) continue;
        if (F.isInFrustum(pMP, 0.5)) { pMP->IncreaseVisible(); ++n; }
    }
    *nToMatch = n;
    return n > 0 ? matcher.SearchByProjection(F, local, th) : 0;
}

int compare(const World& a, const World& b, const char* what) {
    int bad = 0;
    for (size_t i = 0; i < a.pts.size(); ++i) {
        const MapPoint& p = a.pts[i]; const MapPoint& q = b.pts[i];
        bool same = p.mbTrackInView == q.mbTrackInView && p.mnVisible == q.mnVisible && p.mnLastFrameSeen == q.mnLastFrameSeen;
        if (p.mbTrackInView && q.mbTrackInView)
            same = same && std::memcmp(&p.mTrackProjX, &q.mTrackProjX, 4) == 0 && std::memcmp(&p.mTrackProjY, &q.mTrackProjY, 4) == 0 &&
                   std::memcmp(&p.mTrackProjXR, &q.mTrackProjXR, 4) == 0 && std::memcmp(&p.mTrackViewCos, &q.mTrackViewCos, 4) == 0 &&
                   p.mnTrackScaleLevel == q.mnTrackScaleLevel;
        if (!same && bad++ < 10)
            fprintf(stderr, "%s: point %zu differs: in view %d/%d visible %d/%d u %.9g/%.9g v %.9g/%.9g level %d/%d cos %.9g/%.9g\n", what, i, (int)p.mbTrackInView,
                    (int)q.mbTrackInView, p.mnVisible, q.mnVisible, p.mTrackProjX, q.mTrackProjX, p.mTrackProjY, q.mTrackProjY, p.mnTrackScaleLevel,
                    q.mnTrackScaleLevel, p.mTrackViewCos, q.mTrackViewCos);
    }
    for (int g = 0; g < a.F.N_total; ++g) {
        const long ia = a.F.mvpMapPoints[g] ? (long)(a.F.mvpMapPoints[g] - a.pts.data()) : -1;
        const long ib = b.F.mvpMapPoints[g] ? (long)(b.F.mvpMapPoints[g] - b.pts.data()) : -1;
        if (ia != ib && bad++ < 10) fprintf(stderr, "%s: feature %d holds point %ld / %ld\n", what, g, ia, ib);
    }
    return bad;
}

int run_check(const char* world, const char* out) {
    World A, B;
    if (!load(world, A) || !load(world, B)) return 2;
    B.F.mnId = A.F.mnId;
    ORBmatcher ma(0.8f), mb(0.8f);
    int na = 0, nb = 0;
    const unsigned long fails = ORBmatcher::FailureCount();
    const int ra = SearchLocalPoints(ma, A.F, A.vp, A.th, &na);
    const int rb = host_search_local_points(mb, B.F, B.vp, B.th, &nb);
    if (ORBmatcher::FailureCount() != fails) { fprintf(stderr, "a device call failed: %s\n", ORBmatcher::LastError()); return 3; }
    int bad = compare(A, B, "first frame");
    if (ra != rb || na != nb) { fprintf(stderr, "counts differ: matches %d / %d, in view %d / %d\n", ra, rb, na, nb); ++bad; }
    int written = 0, total = 0;
    LocalPointsStats(&written, &total);
    if (written != (int)A.pts.size()) { fprintf(stderr, "first call sent %d rows of %zu\n", written, A.pts.size()); ++bad; }
    FILE* f = fopen(out, "wb");
    if (!f) return 2;
    fwrite(&na, 4, 1, f); fwrite(&ra, 4, 1, f);
    for (const MapPoint& p : A.pts) {
        const int32_t iv = p.mbTrackInView, lv = p.mnTrackScaleLevel, vis = p.mnVisible;
        fwrite(&iv, 4, 1, f); fwrite(&p.mTrackProjX, 4, 1, f); fwrite(&p.mTrackProjY, 4, 1, f); fwrite(&p.mTrackProjXR, 4, 1, f);
        fwrite(&p.mTrackViewCos, 4, 1, f); fwrite(&lv, 4, 1, f); fwrite(&vis, 4, 1, f);
    }
    for (int g = 0; g < A.F.N; ++g) {
        const int32_t idx = A.F.mvpMapPoints[g] ? (int32_t)(A.F.mvpMapPoints[g] - A.pts.data()) : -1;
        fwrite(&idx, 4, 1, f);
    }
    fclose(f);
    // a second frame: a new id, the matches of the first frame stay in F.mvpMapPoints (loop 1 takes them out of the search), every
    // 50th point moved a little, every 97th with a new descriptor bit, three points gone bad.  Only the changed rows may be sent.
    int changed = 0;
    const long unsigned int second_id = A.F.mnId + 1000;
    for (World* W : {&A, &B}) {
        W->F.mnId = second_id;
        changed = 0;
        for (size_t i = 0; i < W->pts.size(); ++i) {
            bool ch = false;
            if (i % 50 == 7) { W->pts[i].mWorldPos.at<float>(0) += 0.01f; ch = true; }
            if (i % 97 == 3) { W->pts[i].mDescriptor.ptr(0)[5] ^= 0x10; ch = true; }
            changed += ch;
        }
        for (size_t i = 11; i < W->pts.size() && i < 14; ++i) W->pts[i].mbBad = true;
    }
    const int ra2 = SearchLocalPoints(ma, A.F, A.vp, A.th, &na);
    const int rb2 = host_search_local_points(mb, B.F, B.vp, B.th, &nb);
    if (ORBmatcher::FailureCount() != fails) { fprintf(stderr, "a device call failed: %s\n", ORBmatcher::LastError()); return 3; }
    bad += compare(A, B, "second frame");
    if (ra2 != rb2 || na != nb) { fprintf(stderr, "second frame: counts differ: matches %d / %d, in view %d / %d\n", ra2, rb2, na, nb); ++bad; }
    LocalPointsStats(&written, &total);
    // (runs less than 32 rows apart go out as one: at most 32 unchanged rows ride along with every changed one)
    if (written < changed || written > changed * 33) { fprintf(stderr, "second call sent %d rows for %d changed ones\n", written, changed); ++bad; }
    if (bad) return 1;
    printf("local_points check ok: %zu points, %d in view, %d matches; second frame %d in view, %d matches, %d of %d rows sent for %d changed\n",
           A.pts.size(), nb, ra, na, ra2, written, total, changed);
    return 0;
}

int run_time(const char* world, double seconds) {
    World A, B;
    if (!load(world, A) || !load(world, B)) return 2;
    ORBmatcher ma(0.8f), mb(0.8f);
    using clk = std::chrono::steady_clock;
    for (int pair = -1; pair < 5; ++pair)          // (pair -1: warm-up, not reported)
        for (int leg = 0; leg < 2; ++leg) {
            World& W = leg ? B : A;
            const double budget = pair < 0 ? 0.2 : seconds;
            long calls = 0; int nm = 0, nin = 0;
            const clk::time_point t0 = clk::now();
            double el = 0;
            do {
                W.place();
                nm = leg ? host_search_local_points(mb, W.F, W.vp, W.th, &nin) : SearchLocalPoints(ma, W.F, W.vp, W.th, &nin);
                ++calls;
                el = std::chrono::duration<double>(clk::now() - t0).count();
            } while (el < budget);
            if (pair >= 0)
                printf("{\"leg\": \"%s\", \"pair\": %d, \"calls\": %ld, \"us_per_call\": %.2f, \"in_view\": %d, \"matches\": %d}\n",
                       leg ? "host_frustum_then_search" : "search_local_points", pair, calls, el * 1e6 / calls, nin, nm);
        }
    return ORBmatcher::FailureCount() ? 3 : 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "check" && argc >= 4) return run_check(argv[2], argv[3]);
    if (mode == "time" && argc >= 4) return run_time(argv[2], std::atof(argv[3]));
    fprintf(stderr, "usage: test_local_points check WORLD.bin OUT.bin | time WORLD.bin SECONDS\n");
    return 2;
}
