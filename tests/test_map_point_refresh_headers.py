"""host/MapPointRefresh.cc must compile against the reference's own headers (`-fsyntax-only -DMORB_USE_REFERENCE_TYPES`), in the
arrangement INTEGRATION.md describes for it: our ORBextractor.h / ORBmatcher.h / ORBVocabulary.h in place of the reference's three,
and the reference's MapPoint.h with the two writers the integration adds (SetDistinctiveDescriptor / SetNormalAndDepth: the members
they fill are protected there).  The tree is made of symbolic links into the reference checkout; the patched MapPoint.h is written
into the temporary directory at test time (nothing of the reference is kept here).  Skipped where the reference checkout is absent."""
import os

import pytest

from helpers import BASE_ADDED, reference_tree, syntax_only

REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include")), reason="reference checkout not present")
ACCESSORS = ("    void SetDistinctiveDescriptor(const cv::Mat &d);\n"
             "    void SetNormalAndDepth(const cv::Mat &normal, float minDistance, float maxDistance);\n")


def _tree(tmp_path, with_accessors):
    return reference_tree(tmp_path, added=BASE_ADDED + ("MapPointRefresh.h",), mappoint_patch=("void UpdateNormalAndDepth();\n", ACCESSORS) if with_accessors else None)


@needs_ref
def test_map_point_refresh_compiles_against_the_reference_headers_with_the_two_writers(tmp_path):
    rc, errors = syntax_only("MapPointRefresh.cc", _tree(tmp_path, True))
    assert rc == 0 and not errors, "\n".join(errors[:20])


@needs_ref
def test_the_two_writers_are_all_it_needs_of_the_integration(tmp_path):
    """Against the untouched MapPoint.h the only errors are the two missing writers: everything it reads of the reference's classes
    is public there (GetObservations, GetReferenceKeyFrame, GetWorldPos, isBad; the keyframe's index maps, descriptors, centres,
    keypoints and scale table)."""
    rc, errors = syntax_only("MapPointRefresh.cc", _tree(tmp_path, False))
    assert rc != 0 and errors
    assert all("SetDistinctiveDescriptor" in e or "SetNormalAndDepth" in e for e in errors), "\n".join(errors[:20])
