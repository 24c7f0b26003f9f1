"""CorrectLoopMap / UpdateMapAfterGlobalBA (host/LoopCorrection.h) through the stand-alone driver host/test_loop_correction.

Without a device (`host`): over a host-only resident map, the two drop-ins against transcriptions of the reference on a twin of the map
-- LoopClosing::CorrectLoop's steps 4.1-4.4 (src/LoopClosing.cc:645-727) with MapPoint::UpdateNormalAndDepth per point, and the map
update behind a global bundle adjustment (:925-989) -- on seeded stand-in maps and a hand-built case.  Compared bit for bit per point:
position, normal, distance band, mnCorrectedByKF, mnCorrectedReference; per keyframe: the pose, mTcwBefGBA, the connections; the two
Sim3 maps.  Every loop case holds a point observed by a connected keyframe before and one after its claimant in CorrectedSim3's order
(its normal differs if the refresh is batched across keyframes), every global-BA case a point of each kind; after
UpdateMapAfterGlobalBA the map Audits clean and a Flush sends no row.

With a device (`device`): the same cases and maps large enough for device batches, with the map in HBM."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(os.path.dirname(HERE), "multi_orb_slam_amd", "host")
DRIVER = os.path.join(HOST, "test_loop_correction")


def run(*args):
    assert os.path.exists(DRIVER), "host driver not built (build())"
    out = subprocess.run([DRIVER, *args], capture_output=True, text=True, timeout=600)
    print(out.stdout, out.stderr)
    return out


def check_report(out, what, loops, gbas):
    assert out.returncode == 0 and "loop correction %s ok" % what in out.stdout, out.stdout + out.stderr
    assert "FAIL" not in out.stdout and not out.stderr.strip()
    assert out.stdout.count("loop ") - 1 == loops and out.stdout.count("gba ") == gbas     # (- 1: the closing line)
    assert "loop hand straddle:" in out.stdout and out.stdout.count(" 0 differ") == loops + gbas


def test_host_only_route_equals_the_transcriptions_and_audit():
    check_report(run("host"), "host", 3, 2)


def test_class_under_asan_ubsan():
    """The sanitized build of the class and its driver (host/Makefile `test_loop_correction_san`), a stand-alone binary in the mode that
    needs no device: a report fails the run."""
    subprocess.check_call(["make", "-s", "-C", HOST, "test_loop_correction_san"], timeout=900)
    out = subprocess.run([os.path.join(HOST, "test_loop_correction_san"), "host"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "loop correction host ok" in out.stdout, out.stdout + out.stderr
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr


def test_usage_is_an_error():
    assert run().returncode == 2


@pytest.mark.gpu
def test_device_route_equals_the_transcriptions_and_audit():
    out = run("device")
    check_report(out, "device", 5, 4)
    assert out.stdout.count("device 1") == 9
