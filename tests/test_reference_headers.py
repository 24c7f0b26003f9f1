"""The drop-in must compile against the reference's OWN headers: `-fsyntax-only -DMORB_USE_REFERENCE_TYPES` over
the three host sources with /root/reference/include used IN PLACE (nothing of the reference is copied; OpenCV, which this image
lacks, is stood in for by host/cv_compat.h through the include shim host/cv_shim/).  Two arrangements:

  A. the reference tree untouched: its Frame.h / KeyFrame.h / MapPoint.h pull in its own ORBextractor.h and ORBVocabulary.h;
     our ORBmatcher.cc / ORBextractor.cc / ORBVocabulary.cc must compile beside them;
  B. the integration INTEGRATION.md describes: our ORBextractor.h, ORBmatcher.h and ORBVocabulary.h take the place of the
     reference's three (a directory of symbolic links: the reference's headers where they lie, ours for those three), and besides
     our sources the reference's own consumers of the classes that need nothing but OpenCV core -- src/KeyFrameDatabase.cc
     (ORBVocabulary::score / size), src/MapPoint.cc (ORBmatcher::DescriptorDistance), src/Map.cc -- must compile UNCHANGED.
     (Frame.cc / KeyFrame.cc / Tracking.cc need Eigen and Pangolin, which are absent: not attempted, not faked.)

The compile checks are skipped where the reference checkout is absent (the GPU box); the container types of the stand-ins are
checked everywhere."""
import os

import pytest

from helpers import reference_tree, syntax_only

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "multi_orb_slam_amd", "host")
REF = "/root/reference"
OURS = ["ORBmatcher.cc", "ORBextractor.cc", "ORBVocabulary.cc"]

HAVE_REF = os.path.isdir(os.path.join(REF, "include"))
needs_ref = pytest.mark.skipif(not HAVE_REF, reason="reference checkout not present")


@needs_ref
@pytest.mark.parametrize("src", OURS)
def test_host_sources_compile_against_the_reference_headers_in_place(src):
    rc, errors = syntax_only(os.path.join(HOST, src),
                              [HOST, os.path.join(HOST, "cv_shim"), os.path.join(REF, "include"), REF, os.path.join(ROOT, "include")])
    assert rc == 0 and not errors, "\n".join(errors[:20])


@needs_ref
@pytest.mark.parametrize("src", OURS + ["ref:src/KeyFrameDatabase.cc", "ref:src/MapPoint.cc", "ref:src/Map.cc"])
def test_replaced_headers_serve_our_sources_and_the_reference_consumers(tmp_path, src):
    inc = reference_tree(tmp_path)       # ours take the place of the reference's three
    path = os.path.join(REF, src[4:]) if src.startswith("ref:") else os.path.join(HOST, src)
    rc, errors = syntax_only(path, [inc, os.path.join(HOST, "cv_shim"), REF, os.path.join(ROOT, "include")])
    assert rc == 0 and not errors, "\n".join(errors[:20])


def test_stand_in_types_are_the_reference_types():
    """slam_types.h must declare the two index maps with the reference's container type (include/Frame.h:256,261,
    include/KeyFrame.h:243,248: std::unordered_map<size_t, int>); the reference's headers are read too where they are present."""
    import re
    want = re.compile(r"std::unordered_map<size_t,\s*int>\s+keypoint_to_cam")
    for hdr in ("Frame.h", "KeyFrame.h") if HAVE_REF else ():
        assert want.search(open(os.path.join(REF, "include", hdr)).read()), hdr
    assert len(want.findall(open(os.path.join(HOST, "slam_types.h")).read())) == 2
