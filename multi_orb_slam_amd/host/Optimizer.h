// Optimizer.h -- Optimizer::PoseOptimization (reference include/Optimizer.h:47-48, src/Optimizer.cc:352-898), the motion-only
// optimisation the tracking thread runs after every search, on the device.
//
// The reference builds a g2o graph per call (one `new` per edge and per robust kernel) around a single 6-dof vertex.  The two statics
// below keep its signatures and replace the body: they fill the edge arrays from the frame (mvpMapPoints, mvKeysUn[_total],
// mvuRight[_total], mvInvLevelSigma2), hand them to orbm_pose_optimize (include/orbm.h: one workgroup carries the problem through all
// four rounds), write mvbOutlier and call SetPose.  Only this translation unit replaces the reference's: bundle adjustment, the
// essential graph and Sim3 stay with g2o.  INTEGRATION.md shows the swap.
#ifndef OPTIMIZER_H
#define OPTIMIZER_H

#include <vector>
#include "ORBmatcher.h"

namespace ORB_SLAM2 {

class Optimizer {
public:
    int static PoseOptimization(Frame* pFrame);
    int static PoseOptimization(Frame* pFrame, bool bAllCams);

    // This repository's own: the frames of Tracking::Relocalization's candidate loop (src/Tracking.cc:2083-2121 runs PoseOptimization
    // once per surviving candidate) in ONE batched call, at most ORBM_POSE_MAX_BATCH frames.  vnInliers[i] is what
    // PoseOptimization(vpFrames[i][, bAllCams]) would have returned; every frame's mvbOutlier and pose are written the same way.
    // Returns false -- reported as every search of ORBmatcher reports a failure, nothing written -- when the library refuses the call.
    bool static PoseOptimizationBatch(const std::vector<Frame*>& vpFrames, bool bAllCams, std::vector<int>& vnInliers);
};

// The edge count below which a single call is computed by the library's host routine (the same statements in the kernel's order, no
// launch).  UNMEASURED placeholder until tools/pose_bench.py has run on a device.
extern const int POSE_HOST_BELOW;

}  // namespace ORB_SLAM2

#endif
