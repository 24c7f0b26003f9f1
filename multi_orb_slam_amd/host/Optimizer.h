// Optimizer.h -- Optimizer::PoseOptimization (reference include/Optimizer.h:47-48, src/Optimizer.cc:352-898), the motion-only
// optimisation the tracking thread runs after every search, on the device.
//
// The reference builds a g2o graph per call (one `new` per edge and per robust kernel) around a single 6-dof vertex.  The two statics
// below keep its signatures and replace the body: they fill the edge arrays from the frame (mvpMapPoints, mvKeysUn[_total],
// mvuRight[_total], mvInvLevelSigma2), hand them to orbm_pose_optimize (include/orbm.h: one workgroup carries the problem through all
// four rounds), write mvbOutlier and call SetPose.  This translation unit, host/LocalBA.cc (LocalBundleAdjustment) and host/GlobalBA.cc
// (BundleAdjustment, GlobalBundleAdjustemnt; both below) and host/EssentialGraph.cc (OptimizeEssentialGraph, below) replace the
// reference's: only OptimizeSim3 (all cameras), commented out at its one call site, stays with g2o.
// INTEGRATION.md shows the swap.
//
// Optimizer::OptimizeSim3_cam1 (reference include/Optimizer.h:62-63, src/Optimizer.cc:1984-2243), the refinement LoopClosing::ComputeSim3
// runs between SearchBySim3 and the acceptance of a loop, likewise: the reference's filtering of vpMatches1 statement by statement, the
// camera-frame points as it computes them, then orbm_sim3_optimize (one workgroup carries the problem through both optimisations and both
// chi-square tests).  g2o::Sim3 is the reference's own type inside the reference build and host/g2o_compat.h's stand-in here.
#ifndef OPTIMIZER_H
#define OPTIMIZER_H

#include <map>
#include <set>
#include <vector>
#include "ORBmatcher.h"
#ifndef MORB_USE_REFERENCE_TYPES
#include "LoopClosing.h"   // (host/LoopClosing.h: the stand-in of LoopClosing::KeyFrameAndPose)
#endif

namespace g2o { struct Sim3; }   // (the reference's Thirdparty/g2o/g2o/types/sim3.h, or host/g2o_compat.h)

namespace ORB_SLAM2 {

class KeyFrame;
class MapPoint;
class Map;

class Optimizer {
public:
    int static PoseOptimization(Frame* pFrame);
    int static PoseOptimization(Frame* pFrame, bool bAllCams);

    // This repository's own: the frames of Tracking::Relocalization's candidate loop (src/Tracking.cc:2083-2121 runs PoseOptimization
    // once per surviving candidate) in ONE batched call, at most ORBM_POSE_MAX_BATCH frames.  vnInliers[i] is what
    // PoseOptimization(vpFrames[i][, bAllCams]) would have returned; every frame's mvbOutlier and pose are written the same way.
    // Returns false -- reported as every search of ORBmatcher reports a failure, nothing written -- when the library refuses the call.
    bool static PoseOptimizationBatch(const std::vector<Frame*>& vpFrames, bool bAllCams, std::vector<int>& vnInliers);

    // Returns nIn; nulls vpMatches1[idx] of every correspondence either chi-square test rejected; writes g2oS12 only where the reference
    // does (not on `return 0` after the first test).  The start reaches the library as the float rotation matrix, translation and scale
    // g2o::Sim3(Matrix3d, Vector3d, double) was built from in ComputeSim3 (rotation().toRotationMatrix() rounded to float: exact for a
    // g2oS12 made from float matrices up to the rounding of that round trip).
    int static OptimizeSim3_cam1(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches1, g2o::Sim3& g2oS12, const float th2,
                                 const bool bFixScale);

    // This repository's own: the candidates of one loop (ComputeSim3 runs OptimizeSim3_cam1 once per candidate whose RANSAC succeeded and
    // takes the first with nInliers >= 20) in ONE batched call, at most ORBM_SIM3OPT_MAX_BATCH.  pKF1 is the current keyframe of all;
    // vnInliers[i], vvpMatches1[i] and vg2oS12[i] end as OptimizeSim3_cam1(pKF1, vpKF2[i], vvpMatches1[i], vg2oS12[i], th2, bFixScale)
    // leaves them.  Returns false, nothing written, when the library refuses the call.
    bool static OptimizeSim3Batch(KeyFrame* pKF1, const std::vector<KeyFrame*>& vpKF2, std::vector<std::vector<MapPoint*> >& vvpMatches1,
                                  std::vector<g2o::Sim3>& vg2oS12, const float th2, const bool bFixScale, std::vector<int>& vnInliers);

    // The local bundle adjustment of the mapping thread (reference include/Optimizer.h, src/Optimizer.cc:921-1353), defined in
    // host/LocalBA.cc: steps 1-4 and 12-13 are the reference's, the g2o graph between them is one orbm_local_ba call (include/orbm.h
    // lists what differs: the dense solver of the reduced system, the order of a point's observations and of the points).  *pbStopFlag
    // is read exactly where the reference and g2o read it.
    void static LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, Map* pMap);

    // The bundle adjustment over a whole map that follows a closed loop (LoopClosing::RunGlobalBundleAdjustment: 10 iterations, no
    // kernels) and the map's initialisation (reference include/Optimizer.h:40-45, src/Optimizer.cc:47-330), defined in host/GlobalBA.cc:
    // the filtering of keyframes, points and observations and the recovery (SetPose / SetWorldPos / UpdateNormalAndDepth, or mTcwGBA /
    // mPosGBA / mnBAGlobalForKF when nLoopKF != 0) are the reference's statement by statement, the g2o graph between them is one
    // orbm_bundle_adjust call (include/orbm.h lists what differs: the dense solver of the reduced system; here also the order of the
    // points, ascending mnId, and of a point's observations, ascending keyframe mnId, not heap addresses).  *pbStopFlag is read exactly
    // where g2o reads it.  No map mutex is taken: the reference takes none here.
    void static BundleAdjustment(const std::vector<KeyFrame*>& vpKFs, const std::vector<MapPoint*>& vpMP, int nIterations = 5,
                                 bool* pbStopFlag = NULL, const unsigned long nLoopKF = 0, const bool bRobust = true,
                                 cv::Mat CalibMatrix = cv::Mat::eye(4, 4, CV_32F));
    void static GlobalBundleAdjustemnt(Map* pMap, int nIterations = 5, bool* pbStopFlag = NULL, const unsigned long nLoopKF = 0,
                                       const bool bRobust = true, cv::Mat mCalibMatrix = cv::Mat::eye(4, 4, CV_32F));

    // The pose graph LoopClosing::CorrectLoop optimises between OptimizeSim3_cam1 and the global bundle adjustment (reference
    // include/Optimizer.h:51-55, src/Optimizer.cc:1373-1677), defined in host/EssentialGraph.cc: steps 2-4 (the vertices from
    // CorrectedSim3 or the keyframe's own pose, the loop edges with the minFeat = 100 test and its exception for the current-loop
    // pair, sInsertedEdges, the spanning-tree, loop and covisibility edges, every measurement Sjw * Swi in double, the edges in
    // insertion order) are the reference's statement by statement, the g2o graph between them and step 6 is one
    // orbm_essential_graph call (include/orbm.h lists what differs: the dense solver), then SetPose in vpKFs' order under
    // mMutexMapUpdate, SetWorldPos in vpMPs' order and UpdateNormalAndDepth through the batched RefreshMapPoints.  Two stated
    // deviations, because the reference dereferences a NULL vertex in both: an edge with an end that has no vertex (a bad keyframe) is
    // not added, and a bad keyframe of vpKFs gets no SetPose.  Iterating LoopConnections, its sets and GetLoopEdges() follows heap
    // addresses, as in the reference.  Declared where LoopClosing::KeyFrameAndPose is known: host/LoopClosing.h's stand-in, or the
    // reference's LoopClosing.h included before this header.
#if !defined(MORB_USE_REFERENCE_TYPES) || defined(LOOPCLOSING_H)
    void static OptimizeEssentialGraph(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const LoopClosing::KeyFrameAndPose& NonCorrectedSim3,
                                       const LoopClosing::KeyFrameAndPose& CorrectedSim3,
                                       const std::map<KeyFrame*, std::set<KeyFrame*> >& LoopConnections, const bool& bFixScale);
#endif
};

// The edge count below which a single call is computed by the library's host routine (the same statements in the kernel's order, no
// launch).  UNMEASURED placeholder until tools/pose_bench.py has run on a device.
extern const int POSE_HOST_BELOW;
// The same for OptimizeSim3_cam1, in correspondences: where tools/sim3opt_bench.py found the two to cross for a single problem
// (profiles/r14/notes_sim3opt.md; a batched call always takes the device).
extern const int SIM3OPT_HOST_BELOW;
// The same for LocalBundleAdjustment, in edges: where tools/local_ba_bench.py found the two to cross (profiles/r20/notes_local_ba.md).
extern const int LBA_HOST_BELOW;
// The same for BundleAdjustment, in edges: the smallest world tools/global_ba_bench.py measured, where the device already wins; the
// crossing lies below it (profiles/r21/notes_global_ba.md).
extern const int GBA_HOST_BELOW;
// The same for OptimizeEssentialGraph, in edges: between the two worlds of tools/essential_graph_bench.py that bracket the crossing
// (profiles/r22/notes_essential_graph.md).
extern const int EG_HOST_BELOW;

}  // namespace ORB_SLAM2

#endif
