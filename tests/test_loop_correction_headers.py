"""host/LoopCorrection.cc must compile against the reference's own KeyFrame.h, MapPoint.h and Map.h (`-fsyntax-only
-DMORB_USE_REFERENCE_TYPES`), in the arrangement INTEGRATION.md describes, as tests/test_covisibility_headers.py does for the counting
routines.  LoopClosing.h is host/LoopClosing.h here, as for the essential graph: the reference's includes g2o's types and through them
Eigen, which this image does not have, so of that header only the typedef KeyFrameAndPose is held, and g2o::Sim3 is g2o_compat.h's.
MapPoint.h receives the accessors and the two writers RefreshMapPoints needs.  The tree is made of symbolic links into the reference
checkout; nothing of the reference is kept here.  Skipped where the reference checkout is absent."""
import os

import pytest

from helpers import BASE_ADDED, BASE_REPLACED, reference_tree, syntax_only

REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include")), reason="reference checkout not present")
ADDED_MEMBERS = ("    float GetMinDistance();\n    float GetMaxDistance();\n    void SetDistinctiveDescriptor(const cv::Mat& d);\n"
                 "    void SetNormalAndDepth(const cv::Mat& normal, float minDistance, float maxDistance);\n")


@needs_ref
def test_loop_correction_compiles_against_the_reference_headers(tmp_path):
    tree = reference_tree(tmp_path, replaced=BASE_REPLACED + ("LoopClosing.h",),
                          added=BASE_ADDED + ("LocalMap.h", "LocalMapSearch.h", "point_row.h", "LoopCorrection.h", "MapPointRefresh.h", "g2o_compat.h"),
                          mappoint_patch=("float GetMaxDistanceInvariance();\n", ADDED_MEMBERS))
    rc, errors = syntax_only("LoopCorrection.cc", tree)
    assert rc == 0 and not errors, "\n".join(errors[:20])
