// LoopClosing.h -- a stand-in for the one type Optimizer::OptimizeEssentialGraph takes from the reference's LoopClosing
// (include/LoopClosing.h:49-50): `typedef map<KeyFrame*, g2o::Sim3, std::less<KeyFrame*>, Eigen::aligned_allocator<...> > KeyFrameAndPose`.
// The host library links no Eigen, so the allocator is the default one here; the function only finds and iterates.  Inside the
// reference build the reference's own header is on the include path in place of this file.
#ifndef LOOPCLOSING_H
#define LOOPCLOSING_H

#include <functional>
#include <map>
#include "g2o_compat.h"

namespace ORB_SLAM2 {

class KeyFrame;

class LoopClosing {
public:
    typedef std::map<KeyFrame*, g2o::Sim3, std::less<KeyFrame*> > KeyFrameAndPose;
};

}  // namespace ORB_SLAM2

#endif
