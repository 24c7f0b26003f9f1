"""host/Optimizer.cc with OptimizeSim3_cam1 must compile against the reference's own headers (`-fsyntax-only
-DMORB_USE_REFERENCE_TYPES`), in the arrangement INTEGRATION.md describes for it: our ORBextractor.h / ORBmatcher.h / ORBVocabulary.h /
Optimizer.h in place of the reference's four, everything else -- KeyFrame.h and MapPoint.h among them -- the reference's, used in place.
Everything the drop-in reads of a KeyFrame or a MapPoint is public there (mK, GetRotation, GetTranslation, GetMapPointMatches_cam1,
mvKeysUn, mvInvLevelSigma2, isBad, GetIndexInKeyFrame_cam1, GetWorldPos): no member is added.  g2o::Sim3 is host/g2o_compat.h's stand-in
here (the test needs no Eigen); inside the reference build HAVE_G2O selects the reference's header.  Skipped where the reference
checkout is absent."""
import os

import pytest

from helpers import BASE_ADDED, BASE_REPLACED, reference_tree, syntax_only

REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include")), reason="reference checkout not present")


@needs_ref
def test_optimize_sim3_compiles_against_the_reference_headers(tmp_path):
    tree = reference_tree(tmp_path, replaced=BASE_REPLACED + ("Optimizer.h",), added=BASE_ADDED + ("g2o_compat.h",))
    assert "OptimizeSim3_cam1" in open(os.path.join(tree, "Optimizer.h")).read()
    rc, errors = syntax_only("Optimizer.cc", tree)
    assert rc == 0 and not errors, "\n".join(errors[:20])
