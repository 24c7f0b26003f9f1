"""GPU parity of the local bundle adjustment on the device (orbm_local_ba: kernel chains driven by the host, one synchronisation per
Levenberg trial) with the library's host routine in DEVICE order -- byte for byte: every estimate, every float handed to SetPose /
SetWorldPos, every flag, every counter, how the call ended and how often the stop function was polled."""
import numpy as np
import pytest

import lba_worlds as lw

pytestmark = pytest.mark.gpu
DEVICE_WORLDS = ["f1_x0_p1_stereo", "f2_x1_p40_mixed_wrong10", "f7_x5_p3000_mixed_wrong10", "f7_x5_p300_mono_wrong40",
                 "f64_x40_p400_mixed_wrong10"]


@pytest.fixture(scope="module")
def matcher():
    import multi_orb_slam_amd as m
    mt = m.Matcher(0.8, True)
    yield mt
    mt.close()


def device_and_host(mt, W, stop=None, path=0):
    import multi_orb_slam_amd as m
    P = lw.to_problem(m, W)
    dev = mt.local_ba(P, stop=stop)
    last = mt.last_local_ba()
    hst = m.local_ba_host(P, m.POSE_ORDER_DEVICE, stop=stop)
    assert dev.same_bytes(hst) is None, (dev.same_bytes(hst), dev.rounds, hst.rounds, dev.ended, hst.ended)
    assert last[0] == path and last[3] == hst.polls
    if path == 0:
        # one synchronisation per Levenberg trial, plus: one per optimisation begun, one per stop inside a trial loop, the last
        assert last[2] <= int(hst.rounds["trials"].sum()) + 2 + 1 + 1 and last[1] > 0
    else:
        assert last[1] == 0 and last[2] == 0
    return dev


@pytest.mark.parametrize("name", DEVICE_WORLDS)
def test_device_equals_the_host_routine_in_device_order(matcher, name):
    R = device_and_host(matcher, lw.world(name))
    f, x = lw.WORLDS[name][:2]
    assert R.ended == 0 and R.optimisations == 2 and R.active_poses[0] == f


@pytest.mark.parametrize("name", ["seen_once_and_fixed_only", "keyframe_0_among_the_local", "pose_loses_all_edges", "zero_pivot", "depth_zero_in_camera_1", "bad_points", "no_edges"])
def test_hand_built_cases(matcher, name):
    W, expect = lw.hand_cases()[name]
    R = device_and_host(matcher, W, stop=10 ** 9)
    assert all(getattr(R, k) == v for k, v in expect.items()) if isinstance(expect, dict) else expect(R)


@pytest.mark.parametrize("name", list(lw.stop_cases()))
def test_stop_cases(matcher, name):
    W, n, ended, _, polls = lw.stop_cases()[name]
    R = device_and_host(matcher, W, stop=n)
    assert R.ended == ended and R.polls == polls


def test_the_call_made_twice_gives_the_same_result(matcher):
    W = lw.world("f7_x5_p300_mono_wrong40")
    a = device_and_host(matcher, W)
    device_and_host(matcher, lw.world("f2_x1_p40_mixed_wrong10"))       # (the buffers are reused by a smaller call in between)
    b = device_and_host(matcher, W)
    assert a.same_bytes(b) is None


def test_a_call_after_an_unrelated_search_on_the_same_matcher(matcher):
    import multi_orb_slam_amd as m
    import frustum_worlds as fw
    W = lw.world("f7_x5_p300_mono_wrong40")
    before = device_and_host(matcher, W)
    w = fw.make_world(2000, [1000, 500], 640, 480, 2, 3.0)
    F = matcher.frame(m.FrameData(**w["fr"]))
    with m.LocalPoints(matcher, len(w["points"])) as pts:
        pts.write(0, w["points"])
        _, nmatches, _, _ = matcher.SearchLocalPoints(F, pts, w["view"].native())
        assert nmatches > 100
        after = device_and_host(matcher, W)
    F.close()
    assert before.same_bytes(after) is None


def test_a_problem_past_a_cap_or_without_a_free_pose_reports_the_host_path(matcher):
    import multi_orb_slam_amd as m
    W = lw.world("f65_x3_p150_mixed")
    assert W["n_free"] == m.LBA_MAX_FREE + 1
    device_and_host(matcher, W, path=1)
    device_and_host(matcher, lw.hand_cases()["no_free_pose"][0], path=2)
