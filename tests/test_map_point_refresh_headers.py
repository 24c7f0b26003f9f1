"""host/MapPointRefresh.cc must compile against the reference's own headers (`-fsyntax-only -DMORB_USE_REFERENCE_TYPES`), in the
arrangement INTEGRATION.md describes for it: our ORBextractor.h / ORBmatcher.h / ORBVocabulary.h in place of the reference's three,
and the reference's MapPoint.h with the two writers the integration adds (SetDistinctiveDescriptor / SetNormalAndDepth: the members
they fill are protected there).  The tree is made of symbolic links into the reference checkout; the patched MapPoint.h is written
into the temporary directory at test time (nothing of the reference is kept here).  Skipped where the reference checkout is absent."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "multi_orb_slam_amd", "host")
REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include")), reason="reference checkout not present")
ACCESSORS = ("    void SetDistinctiveDescriptor(const cv::Mat &d);\n"
             "    void SetNormalAndDepth(const cv::Mat &normal, float minDistance, float maxDistance);\n")


def _tree(tmp_path, with_accessors):
    inc = tmp_path / "include"
    inc.mkdir()
    for name in os.listdir(os.path.join(REF, "include")):
        os.symlink(os.path.join(REF, "include", name), inc / name)
    for name in ("ORBextractor.h", "ORBmatcher.h", "ORBVocabulary.h"):
        os.unlink(inc / name)
        os.symlink(os.path.join(HOST, name), inc / name)
    for name in ("cv_compat.h", "slam_types.h", "MapPointRefresh.h"):
        os.symlink(os.path.join(HOST, name), inc / name)
    if with_accessors:
        text = open(os.path.join(REF, "include", "MapPoint.h")).read()
        anchor = "void UpdateNormalAndDepth();\n"
        assert text.count(anchor) == 1
        os.unlink(inc / "MapPoint.h")
        (inc / "MapPoint.h").write_text(text.replace(anchor, anchor + ACCESSORS))
    return str(inc)


def _syntax_only(inc):
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-ffp-contract=off", "-DMORB_USE_REFERENCE_TYPES", "-I", inc, "-I", os.path.join(HOST, "cv_shim"),
           "-I", REF, "-I", os.path.join(ROOT, "include"), os.path.join(HOST, "MapPointRefresh.cc")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    return p.returncode, [ln for ln in p.stderr.splitlines() if "error" in ln]


@needs_ref
def test_map_point_refresh_compiles_against_the_reference_headers_with_the_two_writers(tmp_path):
    rc, errors = _syntax_only(_tree(tmp_path, True))
    assert rc == 0 and not errors, "\n".join(errors[:20])


@needs_ref
def test_the_two_writers_are_all_it_needs_of_the_integration(tmp_path):
    """Against the untouched MapPoint.h the only errors are the two missing writers: everything it reads of the reference's classes
    is public there (GetObservations, GetReferenceKeyFrame, GetWorldPos, isBad; the keyframe's index maps, descriptors, centres,
    keypoints and scale table)."""
    rc, errors = _syntax_only(_tree(tmp_path, False))
    assert rc != 0 and errors
    assert all("SetDistinctiveDescriptor" in e or "SetNormalAndDepth" in e for e in errors), "\n".join(errors[:20])
