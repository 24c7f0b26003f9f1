"""host/Sim3Solver.cc must compile against the reference's own headers (`-fsyntax-only -DMORB_USE_REFERENCE_TYPES`), in the arrangement
INTEGRATION.md describes for it: our ORBextractor.h / ORBmatcher.h / ORBVocabulary.h / Sim3Solver.h in place of the reference's four,
everything else -- KeyFrame.h and MapPoint.h among them -- the reference's, used in place.  Everything the constructor reads of a
KeyFrame or a MapPoint is public there (GetMapPointMatches, GetRotation, GetTranslation, mvKeysUn, mvLevelSigma2, keypoint_to_cam, mK,
isBad, GetIndexInKeyFrame_cam1, GetWorldPos): no member is added.  The tree is made of symbolic links into the reference checkout
(nothing of the reference is kept here).  Skipped where the reference checkout is absent."""
import os

import pytest

from helpers import BASE_REPLACED, reference_tree, syntax_only

REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include")), reason="reference checkout not present")


@needs_ref
def test_sim3_solver_compiles_against_the_reference_headers(tmp_path):
    rc, errors = syntax_only("Sim3Solver.cc", reference_tree(tmp_path, replaced=BASE_REPLACED + ("Sim3Solver.h",)))
    assert rc == 0 and not errors, "\n".join(errors[:20])
