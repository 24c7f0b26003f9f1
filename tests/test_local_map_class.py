"""ResidentMap / UpdateLocalMap (host/LocalMap.h) through the stand-alone driver host/test_local_map.

Without a device (`host`): UpdateLocalMap over a host-only resident map against a transcription of the reference's
UpdateLocalKeyFrames / UpdateLocalPoints (src/Tracking.cc:1794-1949) on the stand-in types -- vpLocalKeyFrames, vpLocalMapPoints, the
reference keyframe, F.mvpMapPoints and every mnTrackReferenceForFrame, on seeded maps over three frames with mutations and their
Touch calls in between --, the hand-built cases (more than 80 K1 keyframes, a tie for the most votes, the parent that ends the walk
early together with a transcription WITHOUT the outer break that must give another list, neighbour lists whose first nine or ten
entries are marked or bad, no votes at all) and Audit (0 after Flush, > 0 after a mutation without its Touch, 0 again after it).
The same program runs once more built with AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone binary.

With a device (`device`, `search`): the map in HBM gives what the host-only map gives on the same worlds, and UpdateLocalMap +
SearchLocalPoints over the resident map leave what the transcription + the existing SearchLocalPoints leave."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(os.path.dirname(HERE), "multi_orb_slam_amd", "host")
DRIVER = os.path.join(HOST, "test_local_map")


def run(driver, *args):
    assert os.path.exists(driver), "host driver not built (build())"
    out = subprocess.run([driver, *args], capture_output=True, text=True, timeout=600)
    print(out.stdout, out.stderr)
    return out


def test_host_only_route_equals_the_transcription_cases_and_audit():
    out = run(DRIVER, "host")
    assert out.returncode == 0 and "local_map host ok" in out.stdout, out.stdout + out.stderr
    assert out.stdout.count("world ") == 3 and not out.stderr.strip()


def test_class_under_asan_ubsan():
    """The sanitized build of the class and its driver (host/Makefile `test_local_map_san`) in the mode that needs no device: a report
    fails the run."""
    subprocess.check_call(["make", "-s", "-C", HOST, "test_local_map_san"], timeout=900)
    out = run(os.path.join(HOST, "test_local_map_san"), "host")
    assert out.returncode == 0 and "local_map host ok" in out.stdout, out.stdout + out.stderr
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr


def test_usage_is_an_error():
    assert run(DRIVER).returncode == 2


@pytest.mark.gpu
def test_device_route_equals_the_host_only_route():
    out = run(DRIVER, "device")
    assert out.returncode == 0 and "local_map device ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("case_index", [1, 3])
def test_update_and_search_over_the_map_equal_the_reference_route(tmp_path, case_index):
    """A frustum world of 2 000 / 8 000 points spread over keyframes of 2 000, bad points and points the frame already holds in use:
    every tracking scratch field, mnVisible, both marks, F.mvpMapPoints, the point list and both counts, on two frames."""
    import numpy as np
    import frustum_worlds as fw
    case = fw.CASES[case_index]
    w = fw.make_world(*case)
    n = case[0]; N = case[1][0]
    rng = np.random.default_rng(case_index + 900)
    bad = (rng.random(n) < 0.05).astype(np.int32)
    feats = rng.permutation(N)[: N // 10]; owners = rng.permutation(n)[: N // 10]
    wpath = str(tmp_path / "world.bin")
    fw.write_driver_world(wpath, w, bad, list(zip(feats.tolist(), owners.tolist())))
    out = run(DRIVER, "search", wpath)
    assert out.returncode == 0 and "local_map search ok" in out.stdout, out.stdout + out.stderr
    listed = int(out.stdout.split("keyframes, ")[1].split(" listed")[0])
    bad[11:14] = 1                                         # (the driver's second frame, whose list it reports, turns these three bad)
    assert listed == int((bad == 0).sum())                 # every keyframe was voted for: the list is every good point
