"""host/NewMapPoints.cc must compile against the reference's own headers (`-fsyntax-only -DMORB_USE_REFERENCE_TYPES`), in the arrangement
INTEGRATION.md describes for it: our ORBextractor.h / ORBmatcher.h / ORBVocabulary.h in place of the reference's three, everything else
the reference's.  Everything the drop-in reads of a KeyFrame is public there (the pose getters, GetPoseInverse, the intrinsics, mRcam12 /
mtcam12, the keypoint vectors, the index map, the level tables): no member is added.  The tree is made of symbolic links into the
reference checkout (nothing of the reference is kept here).  Skipped where the reference checkout is absent."""
import os

import pytest

from helpers import BASE_ADDED, reference_tree, syntax_only

REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include")), reason="reference checkout not present")


@needs_ref
def test_new_map_points_compiles_against_the_reference_headers(tmp_path):
    rc, errors = syntax_only("NewMapPoints.cc", reference_tree(tmp_path, added=BASE_ADDED + ("NewMapPoints.h",)))
    assert rc == 0 and not errors, "\n".join(errors[:20])
