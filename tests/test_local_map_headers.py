"""host/LocalMap.cc must compile against the reference's own Frame.h, KeyFrame.h and MapPoint.h (`-fsyntax-only
-DMORB_USE_REFERENCE_TYPES`), in the arrangement INTEGRATION.md describes: our ORBextractor.h / ORBmatcher.h / ORBVocabulary.h in place
of the reference's three, and the reference's MapPoint.h with the two accessors the integration adds for the packed row
(GetMinDistance / GetMaxDistance).  The tree is made of symbolic links into the reference checkout; nothing of the reference is kept
here.  Skipped where the reference checkout is absent."""
import os

import pytest

from helpers import BASE_ADDED, reference_tree, syntax_only

REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include")), reason="reference checkout not present")
ACCESSORS = "    float GetMinDistance();\n    float GetMaxDistance();\n"


@needs_ref
def test_local_map_compiles_against_the_reference_headers(tmp_path):
    tree = reference_tree(tmp_path, added=BASE_ADDED + ("LocalMap.h", "LocalMapSearch.h", "point_row.h"),
                          mappoint_patch=("float GetMaxDistanceInvariance();\n", ACCESSORS))
    rc, errors = syntax_only("LocalMap.cc", tree)
    assert rc == 0 and not errors, "\n".join(errors[:20])
