"""CovisibilityCounts / KeyFrameCulling (host/Covisibility.h) through the stand-alone driver host/test_covisibility.

Without a device (`host`): over a host-only resident map, CovisibilityCounts followed by the transcribed rest of
KeyFrame::UpdateConnections against a transcription of the whole reference function (src/KeyFrame.cc:486-668) on a twin of the map --
the weights, both ordered vectors and their weights, the parent, mbFirstConnection and the AddConnection calls in order --, and
KeyFrameCulling against a transcription of the reference's loops (src/LocalMapping.cc:966-1038) -- every keyframe's and point's
flags, counters, observations and matches, the SetBadFlag calls in order -- on seeded stand-in maps and on the hand-built cases: no
keyframe, one keyframe and two consecutive keyframes culled, a map where culling the first changes the verdict on a later one, a
keyframe that may not be erased, points that go bad with the keyframe, the ninety-percent rule at 9 of 10, 10 of 10 and 0 of 0.
Audit == 0 after every case.  The same program runs once more built with AddressSanitizer and UndefinedBehaviorSanitizer, as a
stand-alone binary.

With a device (`device`): the same cases with the map in HBM."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(os.path.dirname(HERE), "multi_orb_slam_amd", "host")
DRIVER = os.path.join(HOST, "test_covisibility")

HAND_CASES = ["none", "one", "two consecutive", "first changes second", "not erase", "points go bad", "9 of 10", "10 of 10", "0 of 0", "empty list"]


def run(driver, *args):
    assert os.path.exists(driver), "host driver not built (build())"
    out = subprocess.run([driver, *args], capture_output=True, text=True, timeout=600)
    print(out.stdout, out.stderr)
    return out


def check_report(out, what):
    assert out.returncode == 0 and "covisibility %s ok" % what in out.stdout, out.stdout + out.stderr
    assert "FAIL" not in out.stdout and not out.stderr.strip()
    for name in HAND_CASES:
        assert "culling %s:" % name in out.stdout
    assert out.stdout.count("connections ") == 5


def test_host_only_route_equals_the_transcriptions_and_audit():
    check_report(run(DRIVER, "host"), "host")


def test_class_under_asan_ubsan():
    """The sanitized build of the class and its driver (host/Makefile `test_covisibility_san`) in the mode that needs no device: a
    report fails the run."""
    subprocess.check_call(["make", "-s", "-C", HOST, "test_covisibility_san"], timeout=900)
    out = run(os.path.join(HOST, "test_covisibility_san"), "host")
    assert out.returncode == 0 and "covisibility host ok" in out.stdout, out.stdout + out.stderr
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr


def test_usage_is_an_error():
    assert run(DRIVER).returncode == 2


@pytest.mark.gpu
def test_device_route_equals_the_transcriptions_and_audit():
    check_report(run(DRIVER, "device"), "device")
