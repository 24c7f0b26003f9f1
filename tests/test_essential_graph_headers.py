"""host/EssentialGraph.cc must compile against the reference's own headers (`-fsyntax-only -DMORB_USE_REFERENCE_TYPES`), in the arrangement
INTEGRATION.md describes for it: our ORBextractor.h / ORBmatcher.h / ORBVocabulary.h / Optimizer.h in place of the reference's four,
MapPointRefresh.h and g2o_compat.h added, KeyFrame.h, MapPoint.h and Map.h the reference's, used in place.  Everything the function reads
or writes of a KeyFrame, a MapPoint and the Map is public there (isBad, mnId, GetRotation, GetTranslation, GetParent, hasChild,
GetLoopEdges, GetWeight_cam1, GetCovisiblesByWeight_cam1, SetPose, mnCorrectedByKF, mnCorrectedReference, GetReferenceKeyFrame,
GetWorldPos / SetWorldPos, GetAllKeyFrames, GetAllMapPoints, GetMaxKFid, mMutexMapUpdate): no member is added.  LoopClosing.h is
host/LoopClosing.h here: the reference's includes g2o's types and through them Eigen, which this image does not have, so of that header
only the typedef KeyFrameAndPose is held (its Eigen::aligned_allocator is the default allocator in the stand-in).  The tree is made of
symbolic links into the reference checkout (nothing of the reference is kept here).  Skipped where the reference checkout is absent."""
import os

import pytest

from helpers import BASE_ADDED, BASE_REPLACED, reference_tree, syntax_only

REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include")), reason="reference checkout not present")


@needs_ref
def test_essential_graph_compiles_against_the_reference_headers(tmp_path):
    tree = reference_tree(tmp_path, replaced=BASE_REPLACED + ("Optimizer.h", "LoopClosing.h"), added=BASE_ADDED + ("MapPointRefresh.h", "g2o_compat.h"))
    text = open(os.path.join(tree, "Optimizer.h")).read()
    assert "OptimizeEssentialGraph(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const LoopClosing::KeyFrameAndPose& NonCorrectedSim3" in text
    rc, errors = syntax_only("EssentialGraph.cc", tree)
    assert rc == 0 and not errors, "\n".join(errors[:20])
