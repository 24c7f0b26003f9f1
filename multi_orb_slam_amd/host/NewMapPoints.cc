// NewMapPoints.cc -- see NewMapPoints.h.
#include "NewMapPoints.h"

#include <cstdio>
#include <cstring>
#include "../../include/orbv.h"

namespace ORB_SLAM2 {

// UNMEASURED: see NewMapPoints.h
const int TRIANGULATE_HOST_BELOW = 16;

namespace {

// One keyframe as orbv_tri_keyframe reads it.  Everything goes through public members of the reference's KeyFrame: the pose getters,
// GetPoseInverse() for Twc (protected there), the intrinsics, mRcam12 / mtcam12, the keypoint vectors and the two level tables.
struct Flat {
    orbv_tri_keyframe k;
    std::vector<float> x, y, xd, yd, uright, depth, cos_stereo;
    std::vector<int32_t> octave, cam_of;
};

void copy34(const cv::Mat& R, const cv::Mat& t, float* dst) {
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) dst[4 * r + c] = R.at<float>(r, c);
        dst[4 * r + 3] = t.at<float>(r);
    }
}

// poses, intrinsics and level tables: all the resident calls read of an orbv_tri_keyframe
void flatten_constants(KeyFrame* pKF, orbv_tri_keyframe& k) {
    std::memset(&k, 0, sizeof(k));
    copy34(pKF->GetRotation(), pKF->GetTranslation(), k.Tcw[0]);
    copy34(pKF->GetRotation_cam2(), pKF->GetTranslation_cam2(), k.Tcw[1]);
    const cv::Mat Ow = pKF->GetCameraCenter(), Ow2 = pKF->GetCameraCenter_cam2();
    for (int c = 0; c < 3; ++c) { k.centre[0][c] = Ow.at<float>(c); k.centre[1][c] = Ow2.at<float>(c); }
    const cv::Mat Twc = pKF->GetPoseInverse();
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) k.Twc[4 * r + c] = Twc.at<float>(r, c);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) k.Rcam12[3 * r + c] = pKF->mRcam12.at<float>(r, c);
        k.tcam12[r] = pKF->mtcam12.at<float>(r);
    }
    k.fx = pKF->fx; k.fy = pKF->fy; k.cx = pKF->cx; k.cy = pKF->cy; k.invfx = pKF->invfx; k.invfy = pKF->invfy; k.mbf = pKF->mbf;
    k.n_levels = (int)pKF->mvScaleFactors.size();
    k.scale_factors = pKF->mvScaleFactors.data(); k.level_sigma2 = pKF->mvLevelSigma2.data();
    k.n = (int)pKF->mvKeysUn_total.size(); k.n_cam1 = pKF->N;
}

void flatten(KeyFrame* pKF, Flat& F) {
    flatten_constants(pKF, F.k);
    const int n = F.k.n;
    F.x.resize(n); F.y.resize(n); F.xd.resize(n); F.yd.resize(n); F.uright.resize(n); F.depth.resize(n); F.cos_stereo.resize(n);
    F.octave.resize(n); F.cam_of.resize(n);
    for (int i = 0; i < n; ++i) {
        const cv::KeyPoint& un = pKF->mvKeysUn_total[i];
        const cv::KeyPoint& kp = pKF->mvKeys_total[i];
        F.x[i] = un.pt.x; F.y[i] = un.pt.y; F.octave[i] = un.octave;
        F.xd[i] = kp.pt.x; F.yd[i] = kp.pt.y;
        F.uright[i] = pKF->mvuRight_total[i]; F.depth[i] = pKF->mvDepth_total[i];
        F.cam_of[i] = pKF->keypoint_to_cam.find(i)->second;                    // :410
    }
    orbv_cos_stereo(pKF->mb, F.depth.data(), n, F.cos_stereo.data());          // :447, :449 -- read where uright >= 0 only
    F.k.x = F.x.data(); F.k.y = F.y.data(); F.k.xd = F.xd.data(); F.k.yd = F.yd.data(); F.k.octave = F.octave.data();
    F.k.uright = F.uright.data(); F.k.depth = F.depth.data(); F.k.cos_stereo = F.cos_stereo.data(); F.k.cam_of = F.cam_of.data();
}

struct Scratch {   // per calling thread, like the matcher handle
    Flat f1, f2;
    std::vector<int32_t> pairs;
    std::vector<orbv_tri_out> rec;
    // CreateNewPointsOfKeyFrame
    std::vector<orbv_new_points_round> rounds;
    std::vector<std::vector<uint8_t> > flags;   // [0]: the current keyframe's, [1 + k]: round k's neighbour's
    std::vector<int32_t> match;
    std::vector<int> counts;
};
thread_local Scratch tls_scratch;


void to_pair(const orbv_tri_out& o, TriangulatedPair& t) {
    t.outcome = o.outcome;
    t.accepted = o.outcome == ORBV_TRI_ACCEPTED;
    if (o.path != ORBV_TRI_PATH_NONE) {
        t.x3D = cv::Mat(3, 1, CV_32F);
        for (int k = 0; k < 3; ++k) t.x3D.at<float>(k) = o.x3D[k];
    }
}

// bit 0: no MapPoint yet (!pKF->GetMapPoint(i), host/ORBmatcher.cc SearchForTriangulation with bOnlyStereo = false); bit 1: stereo
void map_point_flags(KeyFrame* pKF, std::vector<uint8_t>& f) {
    const size_t n = pKF->mvKeysUn_total.size();
    f.resize(n);
    for (size_t i = 0; i < n; ++i) f[i] = (uint8_t)((pKF->GetMapPoint(i) ? 0 : 1) | (pKF->mvuRight_total[i] >= 0 ? 2 : 0));
}

}  // namespace

bool TriangulateMatches(ORBmatcher& matcher, KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<std::pair<size_t, size_t> >& vMatchedIndices,
                        const std::vector<bool>& istrian, std::vector<TriangulatedPair>& out) {
    out.clear();
    const int n = (int)vMatchedIndices.size();
    if (n == 0) return true;
    Scratch& S = tls_scratch;
    flatten(pKF1, S.f1); flatten(pKF2, S.f2);
    S.pairs.resize(2 * (size_t)n); S.rec.resize((size_t)n);
    for (int i = 0; i < n; ++i) { S.pairs[2 * i] = (int32_t)vMatchedIndices[i].first; S.pairs[2 * i + 1] = (int32_t)vMatchedIndices[i].second; }
    const uint8_t enabled[2] = {(uint8_t)(istrian.size() > 0 && istrian[0]), (uint8_t)(istrian.size() > 1 && istrian[1])};
    const float ratioFactor = 1.5f * pKF1->mfScaleFactor;                      // :308
    int rc;
    if (n < TRIANGULATE_HOST_BELOW) {
        rc = orbv_triangulate_pairs_host(&S.f1.k, &S.f2.k, enabled, S.pairs.data(), n, ratioFactor, S.rec.data());
    } else {
        orbv_workspace* w = matcher.GetBowWorkspace();
        if (!w) return false;                                                   // (reported by the matcher)
        rc = orbv_triangulate_pairs(w, &S.f1.k, &S.f2.k, enabled, S.pairs.data(), n, ratioFactor, S.rec.data());
    }
    if (rc) {
        std::fprintf(stderr, "TriangulateMatches: the triangulation call failed (%d): %s -- no points created\n", rc, orb_last_error());
        return false;
    }
    out.resize((size_t)n);
    for (int i = 0; i < n; ++i) to_pair(S.rec[i], out[i]);
    return true;
}

ResidentKeyFrames& ResidentKeyFrames::OfThread() {
    thread_local ResidentKeyFrames cache;
    return cache;
}

bool ResidentKeyFrames::Holds(KeyFrame* pKF) const {
    for (const Entry& e : mEntries) if (e.pKF == pKF) return true;
    return false;
}

void ResidentKeyFrames::Forget(KeyFrame* pKF) {
    for (size_t i = 0; i < mEntries.size(); ++i)
        if (mEntries[i].pKF == pKF) {
            orbv_keyframe_destroy(mEntries[i].handle);
            mEntries.erase(mEntries.begin() + (std::ptrdiff_t)i);
            return;
        }
}

void ResidentKeyFrames::Clear() {
    for (Entry& e : mEntries) orbv_keyframe_destroy(e.handle);
    mEntries.clear();
}

orbv_keyframe* ResidentKeyFrames::Get(ORBmatcher& matcher, KeyFrame* pKF, bool* ok) {
    if (ok) *ok = true;
    const size_t n = pKF->mvKeysUn_total.size();
    for (size_t i = 0; i < mEntries.size(); ++i) {
        Entry& e = mEntries[i];
        if (e.pKF != pKF) continue;
        if (e.id == pKF->mnId && e.n == n) { e.stamp = ++mClock; ++mReused; return e.handle; }
        Forget(pKF);   // the address belongs to another keyframe now
        break;
    }
    orbv_workspace* w = mbDryRun ? nullptr : matcher.GetBowWorkspace();
    if (!w && !mbDryRun) { if (ok) *ok = false; return nullptr; }                // (reported by the matcher)
    orbv_keyframe* handle = nullptr;
    Flat& F = tls_scratch.f2;
    flatten(pKF, F);
    int rc = ORBmatcher::CreateResidentKeyFrame(w, pKF, &handle);
    if (!rc && handle) rc = orbv_keyframe_set_geometry(w, handle, F.uright.data(), F.depth.data(), F.cos_stereo.data(), F.xd.data(), F.yd.data());
    if (rc) {
        std::fprintf(stderr, "ResidentKeyFrames: keyframe %lu could not be made resident (%d): %s\n", pKF->mnId, rc, orb_last_error());
        orbv_keyframe_destroy(handle);
        if (ok) *ok = false;
        return nullptr;
    }
    if (mCapacity == 0) mCapacity = 1;
    while (mEntries.size() >= mCapacity) {                                       // least recently used out first
        size_t victim = 0;
        for (size_t i = 1; i < mEntries.size(); ++i) if (mEntries[i].stamp < mEntries[victim].stamp) victim = i;
        orbv_keyframe_destroy(mEntries[victim].handle);
        mEntries.erase(mEntries.begin() + (std::ptrdiff_t)victim);
        ++mEvicted;
    }
    mEntries.push_back(Entry{pKF, pKF->mnId, n, handle, ++mClock});
    ++mCreated;
    return handle;
}

void PlanNewPointsRounds(KeyFrame* pKF1, const std::vector<KeyFrame*>& vpNeighKFs, bool bMonocular, std::vector<NewPointsRoundPlan>& rounds) {
    rounds.clear();
    cv::Mat Ow1 = pKF1->GetCameraCenter();                                       // :298
    cv::Mat Ow1_cam2 = pKF1->GetCameraCenter_cam2();                             // :299
    for (size_t i = 0; i < vpNeighKFs.size(); i++) {                             // :315  (:318: see the deviation in NewMapPoints.h)
        KeyFrame* pKF2 = vpNeighKFs[i];
        cv::Mat Ow2 = pKF2->GetCameraCenter();
        cv::Mat Ow2_cam2 = pKF2->GetCameraCenter_cam2();
        cv::Mat vBaseline = Ow2 - Ow1;
        cv::Mat vBaseline_cam2 = Ow2_cam2 - Ow1_cam2;
        const float baseline = cv::norm(vBaseline);
        const float baseline_cam2 = cv::norm(vBaseline_cam2);
        std::vector<bool> istrian(2, false);
        if (!bMonocular) {
            if (baseline < pKF2->mb && baseline_cam2 < pKF2->mb) continue;       // :338
            if (baseline >= pKF2->mb) istrian[0] = true;
            if (baseline_cam2 >= pKF2->mb) istrian[1] = true;
        }
        // (monocular, :343-350: a `continue` on baseline / ComputeSceneMedianDepth(2) < 0.01 that leaves istrian untouched either way)
        if (!istrian[0] && !istrian[1]) continue;                                // :351
        NewPointsRoundPlan r;
        r.pKF2 = pKF2; r.baseline = baseline; r.baseline_cam2 = baseline_cam2; r.istrian = istrian;
        rounds.push_back(r);
    }
}

bool CreateNewPointsOfKeyFrame(ORBmatcher& matcher, KeyFrame* pKF1, const std::vector<KeyFrame*>& vpNeighKFs, bool bMonocular,
                               std::vector<NeighbourPoints>& out) {
    out.clear();
    std::vector<NewPointsRoundPlan> plan;
    PlanNewPointsRounds(pKF1, vpNeighKFs, bMonocular, plan);
    const int K = (int)plan.size();
    if (K == 0) return true;
    if (K > ORBV_MAX_ROUNDS) {
        std::fprintf(stderr, "CreateNewPointsOfKeyFrame: %d neighbours, the library takes %d -- no points created\n", K, (int)ORBV_MAX_ROUNDS);
        return false;
    }
    orbv_workspace* w = matcher.GetBowWorkspace();
    if (!w) return false;                                                        // (reported by the matcher)
    ResidentKeyFrames& cache = ResidentKeyFrames::OfThread();
    cache.Reserve((size_t)K + 1);                                                // the keyframes of one call stay resident together
    Scratch& S = tls_scratch;
    bool ok = true;
    const orbv_keyframe* a = cache.Get(matcher, pKF1, &ok);
    if (!ok) return false;
    const int n = (int)pKF1->mvKeysUn_total.size();
    S.rounds.assign((size_t)K, orbv_new_points_round());
    S.flags.resize((size_t)K + 1);
    map_point_flags(pKF1, S.flags[0]);
    const float ratioFactor = 1.5f * pKF1->mfScaleFactor;                        // :308
    orbv_tri_keyframe k1;
    flatten_constants(pKF1, k1);
    for (int k = 0; k < K; ++k) {
        orbv_new_points_round& r = S.rounds[(size_t)k];
        KeyFrame* pKF2 = plan[(size_t)k].pKF2;
        r.b = cache.Get(matcher, pKF2, &ok);
        if (!ok) return false;
        map_point_flags(pKF2, S.flags[(size_t)k + 1]);
        r.flags_b = S.flags[(size_t)k + 1].data();
        matcher.TriangulationGeometry(pKF1, pKF2, &r.t);
        r.geometry.kf1 = k1;
        flatten_constants(pKF2, r.geometry.kf2);
        r.geometry.cam_enabled[0] = plan[(size_t)k].istrian[0]; r.geometry.cam_enabled[1] = plan[(size_t)k].istrian[1];
        r.geometry.ratio_factor = ratioFactor;
    }
    S.match.resize((size_t)K * n + 1); S.rec.resize((size_t)K * n + 1); S.counts.assign(2 * (size_t)K, 0);
    const int rc = orbv_create_new_points_keyframe(w, a, S.flags[0].data(), S.rounds.data(), K, ORBmatcher::TH_LOW, matcher.ChecksOrientation() ? 1 : 0,
                                                   S.match.data(), S.rec.data(), S.counts.data(), S.counts.data() + K);
    if (rc) {
        std::fprintf(stderr, "CreateNewPointsOfKeyFrame: the call failed (%d): %s -- no points created\n", rc, orb_last_error());
        return false;
    }
    out.resize((size_t)K);
    for (int k = 0; k < K; ++k) {
        NeighbourPoints& N = out[(size_t)k];
        N.pKF2 = plan[(size_t)k].pKF2;
        N.vMatchedIndices.reserve((size_t)S.counts[(size_t)k]); N.pairs.reserve((size_t)S.counts[(size_t)k]);
        for (int i = 0; i < n; ++i) {
            const int32_t j = S.match[(size_t)k * n + i];
            if (j < 0) continue;
            N.vMatchedIndices.push_back(std::make_pair((size_t)i, (size_t)j));   // ascending idx1, as SearchForTriangulation fills it
            N.pairs.push_back(TriangulatedPair());
            to_pair(S.rec[(size_t)k * n + i], N.pairs.back());
        }
    }
    return true;
}

}  // namespace ORB_SLAM2
