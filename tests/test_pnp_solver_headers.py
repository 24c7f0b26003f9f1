"""host/PnPsolver.cc must compile against the reference's own headers (`-fsyntax-only -DMORB_USE_REFERENCE_TYPES`), in the arrangement
INTEGRATION.md describes for it: our ORBextractor.h / ORBmatcher.h / ORBVocabulary.h / PnPsolver.h in place of the reference's four,
everything else -- Frame.h and MapPoint.h among them -- the reference's, used in place.  Everything the constructor reads of a Frame or
a MapPoint is public there (mvpMapPoints, mvKeysUn, mvLevelSigma2, fx, fy, cx, cy, isBad, GetWorldPos): no member is added.  The tree
is made of symbolic links into the reference checkout (nothing of the reference is kept here).  Skipped where the reference checkout is
absent."""
import os

import pytest

from helpers import BASE_REPLACED, reference_tree, syntax_only

REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include")), reason="reference checkout not present")


@needs_ref
def test_pnp_solver_compiles_against_the_reference_headers(tmp_path):
    rc, errors = syntax_only("PnPsolver.cc", reference_tree(tmp_path, replaced=BASE_REPLACED + ("PnPsolver.h",)))
    assert rc == 0 and not errors, "\n".join(errors[:20])
