// Sim3Solver.cc -- see Sim3Solver.h.
#include "Sim3Solver.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "ransac_draw.h"
#include "slam_types.h"

namespace ORB_SLAM2 {

// UNMEASURED placeholder: see Sim3Solver.h
const long SIM3_HOST_BELOW = 4096;

// src/Sim3Solver.cc:38-153, statement by statement; the per-correspondence cv::Mat vectors are flat float vectors
Sim3Solver::Sim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*>& vpMatched12, const cv::Mat CalibMatrix, const bool bFixScale)
    : mnIterations(0), mnBestInliers(0), mnBestIndex(-1), mBestScale(0), mbFixScale(bFixScale), mbPrepared(false), mbFailed(false) {
    mpKF1 = pKF1;
    mpKF2 = pKF2;

    std::vector<MapPoint*> vpKeyFrameMP1 = pKF1->GetMapPointMatches();

    mN1 = vpMatched12.size();

    mvpMapPoints1.reserve(mN1);
    mvpMapPoints2.reserve(mN1);
    mvpMatches12 = vpMatched12;
    mvnIndices1.reserve(mN1);
    mvX3Dc1.reserve(3 * (size_t)mN1);
    mvX3Dc2.reserve(3 * (size_t)mN1);

    cv::Mat Rcw1 = pKF1->GetRotation();
    cv::Mat tcw1 = pKF1->GetTranslation();
    cv::Mat Rcw2 = pKF2->GetRotation();
    cv::Mat tcw2 = pKF2->GetTranslation();

    const cv::Mat Rcam12 = CalibMatrix.rowRange(0, 3).colRange(0, 3);
    cv::Mat tcam12 = cv::Mat_<float>(3, 1);
    tcam12.at<float>(0, 0) = CalibMatrix.at<float>(3, 0);
    tcam12.at<float>(1, 0) = CalibMatrix.at<float>(3, 1);
    tcam12.at<float>(2, 0) = CalibMatrix.at<float>(3, 2);
    mRcam21 = Rcam12.t();
    mtcam21 = -mRcam21 * tcam12;

    for (int i1 = 0; i1 < mN1; i1++) {
        if (vpMatched12[i1]) {
            MapPoint* pMP1 = vpKeyFrameMP1[i1];
            MapPoint* pMP2 = vpMatched12[i1];

            if (!pMP1)
                continue;

            if (pMP1->isBad() || pMP2->isBad())
                continue;

            int indexKF1 = pMP1->GetIndexInKeyFrame_cam1(pKF1);
            int indexKF2 = pMP2->GetIndexInKeyFrame_cam1(pKF2);

            if (indexKF1 < 0 || indexKF2 < 0)
                continue;

            const cv::KeyPoint& kp1 = pKF1->mvKeysUn[indexKF1];
            const cv::KeyPoint& kp2 = pKF2->mvKeysUn[indexKF2];

            const float sigmaSquare1 = pKF1->mvLevelSigma2[kp1.octave];
            const float sigmaSquare2 = pKF2->mvLevelSigma2[kp2.octave];

            mvnMaxError1.push_back(9.210 * sigmaSquare1);      // (a std::vector<size_t> in the reference too: the product is truncated)
            mvnMaxError2.push_back(9.210 * sigmaSquare2);

            mvpMapPoints1.push_back(pMP1);
            mvpMapPoints2.push_back(pMP2);
            mvnIndices1.push_back(i1);

            int cam1 = pKF1->keypoint_to_cam.find(indexKF1)->second;
            cv::Mat X3D1w = pMP1->GetWorldPos();
            cv::Mat x3dc1 = Rcw1 * X3D1w + tcw1;
            for (int k = 0; k < 3; ++k) mvX3Dc1.push_back(x3dc1.at<float>(k));
            camIdx1.push_back(cam1);

            int cam2 = pKF2->keypoint_to_cam.find(indexKF2)->second;
            cv::Mat X3D2w = pMP2->GetWorldPos();
            cv::Mat x3dc2 = Rcw2 * X3D2w + tcw2;
            for (int k = 0; k < 3; ++k) mvX3Dc2.push_back(x3dc2.at<float>(k));
            camIdx2.push_back(cam2);
        }
    }

    mK1 = pKF1->mK;
    mK2 = pKF2->mK;

    // FromCameraToImage(mvX3Dc1, mvP1im1, mK1, camIdx1) / (mvX3Dc2, ...): computed by the library from the points (include/orbm.h)

    SetRansacParameters();
}

// src/Sim3Solver.cc:156-182; the arithmetic is the library's (orbm_sim3_iterations)
void Sim3Solver::SetRansacParameters(double probability, int minInliers, int maxIterations) {
    mRansacProb = probability;
    mRansacMinInliers = minInliers;
    N = mvpMapPoints1.size();
    mRansacMaxIts = orbm_sim3_iterations(probability, minInliers, maxIterations, N);
    mnIterations = 0;
    // what was drawn and evaluated belonged to the parameters before
    mbPrepared = false; mbFailed = false;
    mvTriples.clear(); mvCounts.clear(); mvHyp.clear(); mvMasks.clear();
}

// the triples of all mRansacMaxIts iterations (:211-231): vAvailableIndices = mvAllIndices, three times take one and move the back into its place
void Sim3Solver::Draw() {
    mvTriples.clear();
    if (N < mRansacMinInliers || N < 3) return;      // (the reference returns before it draws; with fewer than three it has nothing to draw from)
    std::vector<size_t> vAvailableIndices;
    mvTriples.reserve(3 * (size_t)mRansacMaxIts);
    for (int it = 0; it < mRansacMaxIts; ++it) {
        RansacDrawSet(vAvailableIndices, N, 3, mvTriples);
    }
}

bool Sim3Solver::Prepare(const std::vector<Sim3Solver*>& vpSolvers) {
    std::vector<Sim3Solver*> todo;
    for (Sim3Solver* p : vpSolvers)
        if (p && !p->mbPrepared) todo.push_back(p);
    bool ok = true;
    for (size_t b0 = 0; b0 < todo.size(); b0 += ORBM_SIM3_MAX_BATCH) {
        const int B = (int)std::min(todo.size() - b0, (size_t)ORBM_SIM3_MAX_BATCH);
        std::vector<orbm_sim3_problem> prob((size_t)B);
        std::vector<int32_t> first(1, 0), its_first(1, 0), cam1, cam2, triples;
        std::vector<float> x1, x2, e1, e2;
        long work = 0;
        size_t words = 0;
        for (int b = 0; b < B; ++b) {
            Sim3Solver& S = *todo[b0 + b];
            S.Draw();
            orbm_sim3_problem& P = prob[b];
            std::memset(&P, 0, sizeof(P));
            P.fx1 = S.mK1.at<float>(0, 0); P.fy1 = S.mK1.at<float>(1, 1); P.cx1 = S.mK1.at<float>(0, 2); P.cy1 = S.mK1.at<float>(1, 2);
            P.fx2 = S.mK2.at<float>(0, 0); P.fy2 = S.mK2.at<float>(1, 1); P.cx2 = S.mK2.at<float>(0, 2); P.cy2 = S.mK2.at<float>(1, 2);
            for (int r = 0; r < 3; ++r) {
                for (int c = 0; c < 3; ++c) P.Rcam21[3 * r + c] = S.mRcam21.at<float>(r, c);
                P.tcam21[r] = S.mtcam21.at<float>(r);
            }
            P.fix_scale = S.mbFixScale ? 1 : 0;
            x1.insert(x1.end(), S.mvX3Dc1.begin(), S.mvX3Dc1.end()); x2.insert(x2.end(), S.mvX3Dc2.begin(), S.mvX3Dc2.end());
            cam1.insert(cam1.end(), S.camIdx1.begin(), S.camIdx1.end()); cam2.insert(cam2.end(), S.camIdx2.begin(), S.camIdx2.end());
            for (int i = 0; i < S.N; ++i) { e1.push_back((float)S.mvnMaxError1[i]); e2.push_back((float)S.mvnMaxError2[i]); }   // `err1<mvnMaxError1[i]`: size_t -> float
            triples.insert(triples.end(), S.mvTriples.begin(), S.mvTriples.end());
            const int H = (int)(S.mvTriples.size() / 3);
            first.push_back(first.back() + S.N); its_first.push_back(its_first.back() + H);
            work += (long)H * S.N;
            words += (size_t)H * ((S.N + 63) / 64);
        }
        std::vector<orbm_sim3_hyp> hyp((size_t)std::max(its_first[B], 1));
        std::vector<uint64_t> masks(std::max(words, (size_t)1));
        int rc;
        if (work < SIM3_HOST_BELOW) {
            rc = orbm_sim3_ransac_host(prob.data(), B, first.data(), x1.data(), x2.data(), cam1.data(), cam2.data(), e1.data(), e2.data(),
                                       its_first.data(), triples.data(), ORBM_SIM3_MATH_DEVICE, hyp.data(), masks.data());
        } else {
            ORBmatcher matcher(0.6f, false);                                   // (the handle underneath is the calling thread's)
            orbm_matcher* h = matcher.GetDeviceHandle();
            rc = h ? orbm_sim3_ransac(h, prob.data(), B, first.data(), x1.data(), x2.data(), cam1.data(), cam2.data(), e1.data(), e2.data(),
                                      its_first.data(), triples.data(), hyp.data(), masks.data())
                   : -1;
        }
        if (rc) std::fprintf(stderr, "Sim3Solver::Prepare: the call failed (%d): %s -- the solvers report bNoMore\n", rc, orb_last_error());
        size_t w0 = 0;
        for (int b = 0; b < B; ++b) {
            Sim3Solver& S = *todo[b0 + b];
            const int H = its_first[b + 1] - its_first[b];
            const size_t nw = (size_t)H * ((S.N + 63) / 64);
            S.mbPrepared = true; S.mbFailed = rc != 0;
            if (!rc) {
                S.mvHyp.assign(hyp.begin() + its_first[b], hyp.begin() + its_first[b + 1]);
                S.mvMasks.assign(masks.begin() + w0, masks.begin() + w0 + nw);
                S.mvCounts.resize((size_t)H);
                for (int h = 0; h < H; ++h) S.mvCounts[h] = S.mvHyp[h].n_inliers;
            }
            w0 += nw;
        }
        ok = ok && !rc;
    }
    return ok;
}

// mBestT12 = mT12i.clone() ... of iteration h (:241-246)
void Sim3Solver::SetBest(int h) {
    const orbm_sim3_hyp& R = mvHyp[h];
    mBestT12 = cv::Mat(4, 4, CV_32F);
    mBestRotation = cv::Mat(3, 3, CV_32F);
    mBestTranslation = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) mBestT12.at<float>(r, c) = R.T12[4 * r + c];
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) mBestRotation.at<float>(r, c) = R.R12[3 * r + c]; mBestTranslation.at<float>(r) = R.t12[r]; }
    mBestScale = R.s12;
    mnBestIndex = h;
}

// src/Sim3Solver.cc:186-263 over the counts evaluated ahead
cv::Mat Sim3Solver::iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
    bNoMore = false;
    vbInliers = std::vector<bool>(mN1, false);
    nInliers = 0;

    if (N < mRansacMinInliers) {
        bNoMore = true;
        return cv::Mat();
    }
    if (!mbPrepared) Prepare(std::vector<Sim3Solver*>(1, this));
    if (mbFailed) {
        bNoMore = true;
        return cv::Mat();
    }
    orbm_sim3_walk_state st = {mnIterations, mnBestInliers, mnBestIndex, 0};
    const int H = (int)mvCounts.size();
    const int h = orbm_sim3_walk(mvCounts.data(), H, N, mRansacMinInliers, mnIterations, nIterations, &st);
    mnIterations = st.iterations;
    mnBestInliers = st.best_inliers;
    if (st.best_index != mnBestIndex) SetBest(st.best_index);
    bNoMore = st.no_more != 0;
    if (h < 0) return cv::Mat();
    nInliers = mvCounts[h];
    const int W = (N + 63) / 64;
    for (int i = 0; i < N; i++)
        if ((mvMasks[(size_t)h * W + (i >> 6)] >> (i & 63)) & 1) vbInliers[mvnIndices1[i]] = true;
    return mBestT12;
}

cv::Mat Sim3Solver::find(std::vector<bool>& vbInliers12, int& nInliers) {
    bool bFlag;
    return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
}

cv::Mat Sim3Solver::GetEstimatedRotation() { return mBestRotation.clone(); }

cv::Mat Sim3Solver::GetEstimatedTranslation() { return mBestTranslation.clone(); }

float Sim3Solver::GetEstimatedScale() { return mBestScale; }

}  // namespace ORB_SLAM2
