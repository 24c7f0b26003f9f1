// Sim3Solver.h -- Sim3Solver (reference include/Sim3Solver.h, src/Sim3Solver.cc), the RANSAC between SearchByBoW and SearchBySim3 of
// LoopClosing::ComputeSim3, on the device.
//
// The reference runs up to 300 iterations per loop candidate, five at a time, alternating between candidates; each is a three-point
// Horn alignment and a reprojection of every correspondence in both directions, every vector its own cv::Mat.  No iteration depends on
// another.  This class keeps the reference's signatures and the constructor's filtering statement by statement, draws the triples of
// ALL mRansacMaxIts iterations when it is prepared (DUtils::Random::RandomInt's arithmetic on rand(), the take-and-swap procedure),
// evaluates them in one orbm_sim3_ransac call (include/orbm.h) and turns `iterate` into a scan over the inlier counts
// (orbm_sim3_walk): given the same triples the results are the reference's.  What differs is where rand() is consumed: the reference
// draws lazily, interleaved between candidates, and stops at the first success; this class draws everything up front, so the position
// in the global rand() stream afterwards is not the reference's.
#ifndef SIM3SOLVER_H
#define SIM3SOLVER_H

#include <cstdint>
#include <vector>
#include "ORBmatcher.h"
#include "../../include/orbm.h"

namespace ORB_SLAM2 {

class Sim3Solver {
public:
    Sim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*>& vpMatched12, const cv::Mat CalibMatrix, const bool bFixScale = true);

    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300);

    cv::Mat find(std::vector<bool>& vbInliers12, int& nInliers);

    cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers);

    cv::Mat GetEstimatedRotation();
    cv::Mat GetEstimatedTranslation();
    float GetEstimatedScale();

    // This repository's own: draws the triples of every solver in the vector (null entries are skipped, a solver already prepared is left
    // alone) and evaluates all hypotheses of all of them in ONE orbm_sim3_ransac call (ORBM_SIM3_MAX_BATCH solvers per call; a longer
    // vector takes one call per 64).  In LoopClosing::ComputeSim3 it goes between the loop that constructs the solvers and the loop that
    // iterates them.  A solver that was never prepared prepares itself on its first iterate.  Returns false -- reported as every search
    // of ORBmatcher reports a failure -- when the library refuses the call; such a solver answers bNoMore with the empty matrix.
    static bool Prepare(const std::vector<Sim3Solver*>& vpSolvers);

    // (inspection, for the tests) the triples drawn at preparation, three positions per iteration
    const std::vector<int32_t>& DrawnTriples() const { return mvTriples; }

protected:
    void Draw();
    void SetBest(int h);

    KeyFrame* mpKF1;
    KeyFrame* mpKF2;
    std::vector<float> mvX3Dc1, mvX3Dc2;        // three floats per correspondence
    std::vector<MapPoint*> mvpMapPoints1, mvpMapPoints2, mvpMatches12;
    std::vector<size_t> mvnIndices1;
    std::vector<size_t> mvnMaxError1, mvnMaxError2;
    std::vector<int32_t> camIdx1, camIdx2;
    cv::Mat mRcam21, mtcam21, mK1, mK2;
    int N, mN1;

    // Current Ransac State
    int mnIterations, mnBestInliers, mnBestIndex;
    cv::Mat mBestT12, mBestRotation, mBestTranslation;
    float mBestScale;
    bool mbFixScale;
    double mRansacProb;
    int mRansacMinInliers, mRansacMaxIts;

    // every iteration, evaluated ahead
    bool mbPrepared, mbFailed;
    std::vector<int32_t> mvTriples, mvCounts;
    std::vector<orbm_sim3_hyp> mvHyp;
    std::vector<uint64_t> mvMasks;
};

// hypotheses x correspondences of a Prepare call below which the library's host routine computes it (the same statements in the
// device's order, no launch).  UNMEASURED placeholder until tools/sim3_bench.py has run on a device.
extern const long SIM3_HOST_BELOW;

}  // namespace ORB_SLAM2

#endif
