"""host/LocalMapSearch.cc must compile against the reference's own headers (`-fsyntax-only -DMORB_USE_REFERENCE_TYPES`), in the
arrangement INTEGRATION.md describes for it: our ORBextractor.h / ORBmatcher.h / ORBVocabulary.h in place of the reference's three,
and the reference's MapPoint.h with the two accessors the integration adds (GetMinDistance / GetMaxDistance: the raw bounds are
protected there).  The tree is made of symbolic links into the reference checkout; the patched MapPoint.h is written into the
temporary directory at test time (nothing of the reference is kept here).  Skipped where the reference checkout is absent."""
import os

import pytest

from helpers import BASE_ADDED, reference_tree, syntax_only

REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include")), reason="reference checkout not present")
ACCESSORS = "    float GetMinDistance();\n    float GetMaxDistance();\n"


def _tree(tmp_path, with_accessors):
    return reference_tree(tmp_path, added=BASE_ADDED + ("LocalMapSearch.h",), mappoint_patch=("float GetMaxDistanceInvariance();\n", ACCESSORS) if with_accessors else None)


@needs_ref
def test_local_map_search_compiles_against_the_reference_headers_with_the_two_accessors(tmp_path):
    rc, errors = syntax_only("LocalMapSearch.cc", _tree(tmp_path, True))
    assert rc == 0 and not errors, "\n".join(errors[:20])


@needs_ref
def test_the_two_accessors_are_all_it_needs_of_the_integration(tmp_path):
    """Against the untouched MapPoint.h the only errors are the two missing accessors: nothing else of the reference's classes is
    reached through a private or absent member."""
    rc, errors = syntax_only("LocalMapSearch.cc", _tree(tmp_path, False))
    assert rc != 0 and errors
    assert all("GetMinDistance" in e or "GetMaxDistance" in e for e in errors), "\n".join(errors[:20])
