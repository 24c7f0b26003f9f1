"""host/GlobalBA.cc must compile against the reference's own headers (`-fsyntax-only -DMORB_USE_REFERENCE_TYPES`), in the arrangement
INTEGRATION.md describes for it: our ORBextractor.h / ORBmatcher.h / ORBVocabulary.h / Optimizer.h in place of the reference's four,
MapPointRefresh.h and ba_rig.h added, everything else -- KeyFrame.h, MapPoint.h and Map.h among them -- the reference's, used in place.
Everything the two functions read or write of a KeyFrame, a MapPoint and the Map is public there (isBad, mnId, GetPose / SetPose,
GetObservations, the keypoint vectors and index map, GetWorldPos / SetWorldPos, mTcwGBA, mPosGBA, mnBAGlobalForKF, GetAllKeyFrames,
GetAllMapPoints): no member is added.  The tree is made of symbolic links into the reference checkout (nothing of the reference is kept
here).  Skipped where the reference checkout is absent."""
import os

import pytest

from helpers import BASE_ADDED, BASE_REPLACED, reference_tree, syntax_only

REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include")), reason="reference checkout not present")


@needs_ref
def test_global_ba_compiles_against_the_reference_headers(tmp_path):
    tree = reference_tree(tmp_path, replaced=BASE_REPLACED + ("Optimizer.h",), added=BASE_ADDED + ("MapPointRefresh.h", "ba_rig.h"))
    text = open(os.path.join(tree, "Optimizer.h")).read()
    assert "GlobalBundleAdjustemnt" in text and "BundleAdjustment(const std::vector<KeyFrame*>& vpKFs" in text
    rc, errors = syntax_only("GlobalBA.cc", tree)
    assert rc == 0 and not errors, "\n".join(errors[:20])
