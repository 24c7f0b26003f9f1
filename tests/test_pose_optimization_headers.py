"""host/Optimizer.cc must compile against the reference's own headers (`-fsyntax-only -DMORB_USE_REFERENCE_TYPES`), in the arrangement
INTEGRATION.md describes for it: our ORBextractor.h / ORBmatcher.h / ORBVocabulary.h / Optimizer.h in place of the reference's four,
everything else the reference's.  Everything the drop-in reads or writes of a Frame is public there (mTcw, the intrinsics, mRcam12 /
mtcam12, mvInvLevelSigma2, the keypoint and map-point vectors, mvbOutlier, SetPose): no member is added.  The tree is made of symbolic
links into the reference checkout (nothing of the reference is kept here).  Skipped where the reference checkout is absent."""
import os

import pytest

from helpers import BASE_REPLACED, reference_tree, syntax_only

REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include")), reason="reference checkout not present")


@needs_ref
def test_optimizer_compiles_against_the_reference_headers(tmp_path):
    rc, errors = syntax_only("Optimizer.cc", reference_tree(tmp_path, replaced=BASE_REPLACED + ("Optimizer.h",)))
    assert rc == 0 and not errors, "\n".join(errors[:20])
