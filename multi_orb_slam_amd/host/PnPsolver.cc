// PnPsolver.cc -- see PnPsolver.h.
#include "PnPsolver.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "ransac_draw.h"
#include "slam_types.h"

namespace ORB_SLAM2 {

// UNMEASURED placeholder: see PnPsolver.h
const long PNP_HOST_BELOW = 3000;

// src/PnPsolver.cc:71-114, statement by statement; cv::Point2f / cv::Point3f are flat float vectors
PnPsolver::PnPsolver(const Frame& F, const std::vector<MapPoint*>& vpMapPointMatches)
    : N(0), mnTakenBest(-1), mbPrepared(false), mbFailed(false), mnBlockStart(0) {
    mvpMapPointMatches = vpMapPointMatches;
    mvP2D.reserve(2 * F.mvpMapPoints.size());
    mvSigma2.reserve(F.mvpMapPoints.size());
    mvP3Dw.reserve(3 * F.mvpMapPoints.size());
    mvKeyPointIndices.reserve(F.mvpMapPoints.size());
    mvAllIndices.reserve(F.mvpMapPoints.size());

    int idx = 0;
    for (size_t i = 0, iend = vpMapPointMatches.size(); i < iend; i++) {
        MapPoint* pMP = vpMapPointMatches[i];

        if (pMP) {
            if (!pMP->isBad()) {
                const cv::KeyPoint& kp = F.mvKeysUn[i];

                mvP2D.push_back(kp.pt.x);
                mvP2D.push_back(kp.pt.y);
                mvSigma2.push_back(F.mvLevelSigma2[kp.octave]);

                cv::Mat Pos = pMP->GetWorldPos();
                mvP3Dw.push_back(Pos.at<float>(0));
                mvP3Dw.push_back(Pos.at<float>(1));
                mvP3Dw.push_back(Pos.at<float>(2));

                mvKeyPointIndices.push_back(i);
                mvAllIndices.push_back(idx);

                idx++;
            }
        }
    }

    // Set camera calibration parameters
    fu = F.fx;
    fv = F.fy;
    uc = F.cx;
    vc = F.cy;

    std::memset(&mState, 0, sizeof(mState));
    SetRansacParameters();
}

PnPsolver::~PnPsolver() {}

// src/PnPsolver.cc:126-162; the arithmetic is the library's (orbm_pnp_parameters)
void PnPsolver::SetRansacParameters(double probability, int minInliers, int maxIterations, int minSet, float epsilon, float th2) {
    mRansacProb = probability;
    mRansacMinSet = minSet;
    mRansacTh = th2;

    N = mvP2D.size() / 2;  // number of correspondences

    int32_t out2[2];
    orbm_pnp_parameters(probability, minInliers, maxIterations, minSet, epsilon, N, out2, &mRansacEpsilon);
    mRansacMaxIts = out2[0];
    mRansacMinInliers = out2[1];

    mvMaxError.resize(mvSigma2.size());
    for (size_t i = 0; i < mvSigma2.size(); i++)
        mvMaxError[i] = mvSigma2[i] * th2;

    // what was drawn and evaluated belonged to the parameters before (the reference keeps mnIterations and mnBestInliers: so does this)
    mbPrepared = false; mbFailed = false;
    mnBlockStart = mState.iterations;
    mvQuads.clear(); mvCounts.clear(); mvRecHyp.clear(); mvRecInliers.clear(); mvHyp.clear(); mvMasks.clear(); mvRefined.clear(); mvRefinedMasks.clear();
    if (mState.best_hyp < 0 || mState.best_inliers == 0) { mState.best_hyp = -1; mState.best_record = -1; }
}

// nHyp[k] more iterations of todo[k]: drawn (:194-207), evaluated in one call with best_start = mnBestInliers, kept as the solver's block
bool PnPsolver::Evaluate(const std::vector<PnPsolver*>& todo, const std::vector<int>& nHyp) {
    bool ok = true;
    for (size_t b0 = 0; b0 < todo.size(); b0 += ORBM_PNP_MAX_BATCH) {
        const int B = (int)std::min(todo.size() - b0, (size_t)ORBM_PNP_MAX_BATCH);
        std::vector<orbm_pnp_problem> prob((size_t)B);
        std::vector<int32_t> first(1, 0), its_first(1, 0), quads;
        std::vector<float> p3, p2, me;
        std::vector<size_t> vAvailableIndices;
        long work = 0;
        size_t words = 0, rwords = 0;
        int extra = 0;
        for (int b = 0; b < B; ++b) {
            PnPsolver& S = *todo[b0 + b];
            const int H = S.N >= 4 ? std::min(nHyp[b0 + b], (int)ORBM_PNP_MAX_ITS) : 0;
            const size_t q0 = S.mvQuads.size();
            for (int it = 0; it < H; ++it) RansacDrawSet(vAvailableIndices, S.N, 4, S.mvQuads);   // (mRansacMinSet: EPnP's minimal set is four here as in every caller of the reference)
            quads.insert(quads.end(), S.mvQuads.begin() + q0, S.mvQuads.end());
            orbm_pnp_problem& P = prob[b];
            P.fu = S.fu; P.fv = S.fv; P.uc = S.uc; P.vc = S.vc;
            P.min_inliers = S.mRansacMinInliers;
            P.best_start = S.mState.best_inliers;
            p3.insert(p3.end(), S.mvP3Dw.begin(), S.mvP3Dw.end()); p2.insert(p2.end(), S.mvP2D.begin(), S.mvP2D.end());
            me.insert(me.end(), S.mvMaxError.begin(), S.mvMaxError.end());
            first.push_back(first.back() + S.N); its_first.push_back(its_first.back() + H);
            const size_t W = (size_t)(S.N + 63) / 64;
            work += (long)H * S.N;
            words += (size_t)H * W;
            rwords += (size_t)ORBM_PNP_MAX_RECORDS * W;
            extra += std::max(0, std::min(H, S.N) - (int)ORBM_PNP_MAX_RECORDS);
        }
        size_t xwords = 0;
        for (int b = 0; b < B; ++b) {
            const PnPsolver& S = *todo[b0 + b];
            xwords += (size_t)std::max(0, std::min(its_first[b + 1] - its_first[b], S.N) - (int)ORBM_PNP_MAX_RECORDS) * ((size_t)(S.N + 63) / 64);
        }
        std::vector<orbm_pnp_hyp> hyp((size_t)std::max(its_first[B], 1));
        std::vector<uint64_t> masks(std::max(words, (size_t)1)), rmasks(std::max(rwords + xwords, (size_t)1));
        std::vector<int32_t> nrec((size_t)B, 0);
        std::vector<orbm_pnp_refined> refined((size_t)B * ORBM_PNP_MAX_RECORDS + (size_t)extra);
        int rc;
        if (work < PNP_HOST_BELOW) {
            rc = orbm_pnp_ransac_host(prob.data(), B, first.data(), p3.data(), p2.data(), me.data(), its_first.data(), quads.data(), hyp.data(),
                                      masks.data(), nrec.data(), refined.data(), rmasks.data(), extra);
        } else {
            ORBmatcher matcher(0.6f, false);                                   // (the handle underneath is the calling thread's)
            orbm_matcher* h = matcher.GetDeviceHandle();
            rc = h ? orbm_pnp_ransac(h, prob.data(), B, first.data(), p3.data(), p2.data(), me.data(), its_first.data(), quads.data(), hyp.data(),
                                     masks.data(), nrec.data(), refined.data(), rmasks.data(), extra)
                   : -1;
        }
        if (rc) std::fprintf(stderr, "PnPsolver: the call failed (%d): %s -- the solvers report bNoMore\n", rc, orb_last_error());
        size_t w0 = 0, rw0 = 0, xr = (size_t)B * ORBM_PNP_MAX_RECORDS, xw = rwords;
        for (int b = 0; b < B; ++b) {
            PnPsolver& S = *todo[b0 + b];
            const int H = its_first[b + 1] - its_first[b];
            const size_t W = (size_t)(S.N + 63) / 64;
            S.mbPrepared = true; S.mbFailed = rc != 0;
            S.mnBlockStart = S.mState.iterations;
            S.mState.best_record = -1;
            S.mvCounts.clear(); S.mvRecHyp.clear(); S.mvRecInliers.clear(); S.mvRefined.clear(); S.mvRefinedMasks.clear();
            if (!rc) {
                S.mvHyp.assign(hyp.begin() + its_first[b], hyp.begin() + its_first[b + 1]);
                S.mvMasks.assign(masks.begin() + w0, masks.begin() + w0 + (size_t)H * W);
                S.mvCounts.resize((size_t)H);
                for (int h = 0; h < H; ++h) S.mvCounts[h] = S.mvHyp[h].n_inliers;
                const int nr = nrec[b], nd = std::min(nr, (int)ORBM_PNP_MAX_RECORDS);
                for (int r = 0; r < nr; ++r) {                 // the slots first, the appended records behind
                    const bool ex = r >= nd;
                    const orbm_pnp_refined& R = ex ? refined[xr + (size_t)(r - nd)] : refined[(size_t)b * ORBM_PNP_MAX_RECORDS + r];
                    const uint64_t* rw = ex ? rmasks.data() + xw + (size_t)(r - nd) * W : rmasks.data() + rw0 + (size_t)r * W;
                    S.mvRefined.push_back(R);
                    S.mvRefinedMasks.insert(S.mvRefinedMasks.end(), rw, rw + W);
                    S.mvRecHyp.push_back(R.hyp);
                    S.mvRecInliers.push_back(R.n_inliers);
                }
                xr += (size_t)(nr - nd); xw += (size_t)(nr - nd) * W;
            }
            w0 += (size_t)H * W; rw0 += (size_t)ORBM_PNP_MAX_RECORDS * W;
        }
        ok = ok && !rc;
    }
    return ok;
}

bool PnPsolver::Prepare(const std::vector<PnPsolver*>& vpSolvers) {
    std::vector<PnPsolver*> todo;
    std::vector<int> nHyp;
    for (PnPsolver* p : vpSolvers)
        if (p && !p->mbPrepared) {
            todo.push_back(p);
            nHyp.push_back(p->N < p->mRansacMinInliers ? 0 : std::max(0, p->mRansacMaxIts - p->mState.iterations));   // (the reference returns before it draws)
        }
    return Evaluate(todo, nHyp);
}

// `mvbBestInliers = mvbInliersi; mBestTcw = ...` (:218-230) and what Refine() (:266-311) computed from it, copied out of the block
void PnPsolver::TakeBest() {
    if (mState.best_hyp == mnTakenBest || mState.best_record < 0) return;
    const int h = mState.best_hyp - mnBlockStart, r = mState.best_record;
    const size_t W = (size_t)(N + 63) / 64;
    mBestHyp = mvHyp[h];
    mBestMask.assign(mvMasks.begin() + (size_t)h * W, mvMasks.begin() + (size_t)(h + 1) * W);
    mBestRefined = mvRefined[r];
    mBestRefinedMask.assign(mvRefinedMasks.begin() + (size_t)r * W, mvRefinedMasks.begin() + (size_t)(r + 1) * W);
    mnTakenBest = mState.best_hyp;
}

// `Rcw.convertTo(Rcw,CV_32F); tcw.convertTo(tcw,CV_32F); eye(4,4); copyTo` (:223-229, :300-306)
cv::Mat PnPsolver::Pose(const double* R, const double* t) const {
    cv::Mat Tcw = cv::Mat::eye(4, 4, CV_32F);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) Tcw.at<float>(r, c) = (float)R[3 * r + c];
        Tcw.at<float>(r, 3) = (float)t[r];
    }
    return Tcw;
}

void PnPsolver::Spread(const uint64_t* words, std::vector<bool>& vbInliers) const {
    vbInliers = std::vector<bool>(mvpMapPointMatches.size(), false);
    for (int i = 0; i < N; i++)
        if ((words[i >> 6] >> (i & 63)) & 1) vbInliers[mvKeyPointIndices[i]] = true;
}

// src/PnPsolver.cc:171-264 over the iterations evaluated ahead
cv::Mat PnPsolver::iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
    bNoMore = false;
    vbInliers.clear();
    nInliers = 0;

    if (N < mRansacMinInliers) {
        bNoMore = true;
        return cv::Mat();
    }
    if (!mbPrepared) Prepare(std::vector<PnPsolver*>(1, this));
    mState.exhausted = 0;
    int answer = -1;
    for (;;) {
        if (mbFailed) break;
        answer = orbm_pnp_walk(mvCounts.data(), (int)mvCounts.size(), mnBlockStart, mvRecHyp.data(), mvRecInliers.data(), (int)mvRecHyp.size(), N,
                               mRansacMinInliers, mRansacMaxIts, nIterations, &mState);
        if (answer < 0) { mbFailed = true; break; }
        TakeBest();
        if (!mState.exhausted) break;
        // beyond the evaluated iterations: a continuation block of nIterations hypotheses, the best so far carried along
        Evaluate(std::vector<PnPsolver*>(1, this), std::vector<int>(1, std::max(1, nIterations)));
    }
    if (mbFailed) {
        bNoMore = true;
        return cv::Mat();
    }
    bNoMore = mState.no_more != 0;
    if (answer == ORBM_PNP_WALK_REFINED) {
        nInliers = mBestRefined.n_inliers;
        Spread(mBestRefinedMask.data(), vbInliers);
        return Pose(mBestRefined.R, mBestRefined.t);
    }
    if (answer == ORBM_PNP_WALK_BEST) {
        nInliers = mState.best_inliers;
        Spread(mBestMask.data(), vbInliers);
        return Pose(mBestHyp.R, mBestHyp.t);
    }
    return cv::Mat();
}

cv::Mat PnPsolver::find(std::vector<bool>& vbInliers, int& nInliers) {
    bool bFlag;
    return iterate(mRansacMaxIts, bFlag, vbInliers, nInliers);
}

}  // namespace ORB_SLAM2
