"""host/LocalMapSearch.cc must compile against the reference's own headers (`-fsyntax-only -DMORB_USE_REFERENCE_TYPES`), in the
arrangement INTEGRATION.md describes for it: our ORBextractor.h / ORBmatcher.h / ORBVocabulary.h in place of the reference's three,
and the reference's MapPoint.h with the two accessors the integration adds (GetMinDistance / GetMaxDistance: the raw bounds are
protected there).  The tree is made of symbolic links into the reference checkout; the patched MapPoint.h is written into the
temporary directory at test time (nothing of the reference is kept here).  Skipped where the reference checkout is absent."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "multi_orb_slam_amd", "host")
REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include")), reason="reference checkout not present")
ACCESSORS = "    float GetMinDistance();\n    float GetMaxDistance();\n"


def _tree(tmp_path, with_accessors):
    inc = tmp_path / "include"
    inc.mkdir()
    for name in os.listdir(os.path.join(REF, "include")):
        os.symlink(os.path.join(REF, "include", name), inc / name)
    for name in ("ORBextractor.h", "ORBmatcher.h", "ORBVocabulary.h"):
        os.unlink(inc / name)
        os.symlink(os.path.join(HOST, name), inc / name)
    for name in ("cv_compat.h", "slam_types.h", "LocalMapSearch.h"):
        os.symlink(os.path.join(HOST, name), inc / name)
    if with_accessors:
        text = open(os.path.join(REF, "include", "MapPoint.h")).read()
        anchor = "float GetMaxDistanceInvariance();\n"
        assert text.count(anchor) == 1
        os.unlink(inc / "MapPoint.h")
        (inc / "MapPoint.h").write_text(text.replace(anchor, anchor + ACCESSORS))
    return str(inc)


def _syntax_only(inc):
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-ffp-contract=off", "-DMORB_USE_REFERENCE_TYPES", "-I", inc, "-I", os.path.join(HOST, "cv_shim"),
           "-I", REF, "-I", os.path.join(ROOT, "include"), os.path.join(HOST, "LocalMapSearch.cc")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    return p.returncode, [ln for ln in p.stderr.splitlines() if "error" in ln]


@needs_ref
def test_local_map_search_compiles_against_the_reference_headers_with_the_two_accessors(tmp_path):
    rc, errors = _syntax_only(_tree(tmp_path, True))
    assert rc == 0 and not errors, "\n".join(errors[:20])


@needs_ref
def test_the_two_accessors_are_all_it_needs_of_the_integration(tmp_path):
    """Against the untouched MapPoint.h the only errors are the two missing accessors: nothing else of the reference's classes is
    reached through a private or absent member."""
    rc, errors = _syntax_only(_tree(tmp_path, False))
    assert rc != 0 and errors
    assert all("GetMinDistance" in e or "GetMaxDistance" in e for e in errors), "\n".join(errors[:20])
