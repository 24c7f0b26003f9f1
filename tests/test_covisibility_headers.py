"""host/Covisibility.cc (and host/LocalMap.cc, whose Flush now reads the features' levels and depths, N and mThDepth) must compile
against the reference's own KeyFrame.h, MapPoint.h and Map.h (`-fsyntax-only -DMORB_USE_REFERENCE_TYPES`), in the arrangement
INTEGRATION.md describes, as tests/test_local_map_headers.py does for the local map.  The tree is made of symbolic links into the
reference checkout; nothing of the reference is kept here.  Skipped where the reference checkout is absent."""
import os

import pytest

from helpers import BASE_ADDED, reference_tree, syntax_only

REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include")), reason="reference checkout not present")
ACCESSORS = "    float GetMinDistance();\n    float GetMaxDistance();\n"


@needs_ref
@pytest.mark.parametrize("source", ["Covisibility.cc", "LocalMap.cc"])
def test_covisibility_compiles_against_the_reference_headers(tmp_path, source):
    tree = reference_tree(tmp_path, added=BASE_ADDED + ("LocalMap.h", "LocalMapSearch.h", "point_row.h", "Covisibility.h"),
                          mappoint_patch=("float GetMaxDistanceInvariance();\n", ACCESSORS))
    rc, errors = syntax_only(source, tree)
    assert rc == 0 and not errors, "\n".join(errors[:20])
