// PnPsolver.h -- PnPsolver (reference include/PnPsolver.h, src/PnPsolver.cc), the EPnP RANSAC between SearchByBoW_cam1 and
// Optimizer::PoseOptimization of Tracking::Relocalization, on the device.
//
// The reference runs up to mRansacMaxIts iterations per candidate keyframe, five at a time, alternating between candidates; each is a
// four-point EPnP, CheckInliers over every correspondence and -- whenever the count reaches mRansacMinInliers -- Refine() on the best
// mask.  No iteration depends on another.  This class keeps the reference's public signatures and the constructor's filtering
// statement by statement, draws the quadruples of ALL mRansacMaxIts iterations when it is prepared (ransac_draw.h), evaluates them in
// one orbm_pnp_ransac call (include/orbm.h) and turns `iterate` into orbm_pnp_walk over the counts and the refined records: given the
// same quadruples the results are the reference's.  An iterate that needs iterations beyond the evaluated ones (a call after a
// success, past mRansacMaxIts) draws and evaluates a continuation block with best_start = mnBestInliers and carries the best record
// along.  What differs is where rand() is consumed: everything is drawn up front, so the position in the global rand() stream
// afterwards is not the reference's.
#ifndef PNPSOLVER_H
#define PNPSOLVER_H

#include <cstdint>
#include <vector>
#include "ORBmatcher.h"
#include "../../include/orbm.h"

namespace ORB_SLAM2 {

class PnPsolver {
public:
    PnPsolver(const Frame& F, const std::vector<MapPoint*>& vpMapPointMatches);
    ~PnPsolver();

    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4,
                             float th2 = 5.991);

    cv::Mat find(std::vector<bool>& vbInliers, int& nInliers);

    cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers);

    // This repository's own: draws the quadruples of all mRansacMaxIts iterations of every solver in the vector (null entries are
    // skipped, a solver already prepared is left alone) and evaluates them in ONE orbm_pnp_ransac call (ORBM_PNP_MAX_BATCH solvers per
    // call).  In Tracking::Relocalization it goes between the loop that constructs the solvers and the loop that iterates them.  A
    // solver that was never prepared prepares itself on its first iterate.  Returns false when the library refuses the call; such a
    // solver answers bNoMore with the empty matrix.
    static bool Prepare(const std::vector<PnPsolver*>& vpSolvers);

    // (inspection, for the tests) every quadruple drawn so far, four positions per iteration, continuation blocks included
    const std::vector<int32_t>& DrawnQuads() const { return mvQuads; }

private:
    static bool Evaluate(const std::vector<PnPsolver*>& todo, const std::vector<int>& nHyp);
    void TakeBest();
    cv::Mat Pose(const double* R, const double* t) const;
    void Spread(const uint64_t* words, std::vector<bool>& vbInliers) const;

    std::vector<MapPoint*> mvpMapPointMatches;
    std::vector<float> mvP2D;                  // two floats per correspondence (cv::Point2f)
    std::vector<float> mvSigma2;
    std::vector<float> mvP3Dw;                 // three floats per correspondence (cv::Point3f)
    std::vector<size_t> mvKeyPointIndices;
    std::vector<size_t> mvAllIndices;
    std::vector<float> mvMaxError;
    double uc, vc, fu, fv;
    int N;

    double mRansacProb;
    int mRansacMinInliers, mRansacMaxIts;
    float mRansacEpsilon, mRansacTh;
    int mRansacMinSet;

    // the state of `iterate` (mnIterations, mnBestInliers, ...) as orbm_pnp_walk keeps it
    orbm_pnp_walk_state mState;
    int mnTakenBest;                           // the iteration mBestHyp / mBestMask / mBestRefined were copied for
    orbm_pnp_hyp mBestHyp;
    orbm_pnp_refined mBestRefined;
    std::vector<uint64_t> mBestMask, mBestRefinedMask;

    // the block of iterations evaluated ahead
    bool mbPrepared, mbFailed;
    int mnBlockStart;
    std::vector<int32_t> mvQuads, mvCounts, mvRecHyp, mvRecInliers;
    std::vector<orbm_pnp_hyp> mvHyp;
    std::vector<uint64_t> mvMasks, mvRefinedMasks;
    std::vector<orbm_pnp_refined> mvRefined;
};

// hypotheses x correspondences of an evaluation below which the library's host routine computes it (the same statements, no launch).
// UNMEASURED placeholder until tools/pnp_bench.py has run on a device.
extern const long PNP_HOST_BELOW;

}  // namespace ORB_SLAM2

#endif
