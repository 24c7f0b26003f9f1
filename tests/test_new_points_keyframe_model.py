"""The inputs of the chained call (orbv_create_new_points_keyframe) before any GPU test may rely on them: the worlds of
tests/new_points_worlds.py meet their conditions on the CPU reference chain, the library's host routine agrees with the model on every
round's pairs, and the class driver's host-only mode (baselines, flattening, the books of the resident-keyframe cache) runs clean.  CPU."""
import os
import subprocess

import numpy as np

import multi_orb_slam_amd as m
import new_points_worlds as nw
import triangulate_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "multi_orb_slam_amd", "host", "test_new_points_keyframe")


def test_the_world_meets_its_conditions():
    w, with_update, without = nw.world_and_chain(600, 5)
    print(nw.check_conditions(w, with_update, without))


def test_the_small_worlds_have_matches_in_every_size():
    for n, k in ((63, 2), (64, 2), (65, 2), (257, 4), (300, 15)):
        _, (M, R, _), _ = nw.world_and_chain(n, k)
        assert (M >= 0).sum() >= 20 and (R["outcome"] == tm.ACCEPTED).sum() >= 10, (n, k)


def test_host_routine_equals_the_model_on_every_round():
    w, (M, R, S), _ = nw.world_and_chain(600, 5)
    a = w.kf_a.native()
    for k, b in enumerate(w.nb):
        idx = np.flatnonzero(M[k] >= 0)
        got = m.triangulate_pairs_host(a, b.kf.native(), b.cam_enabled, np.stack([idx, M[k][idx]], 1), nw.RATIO)
        assert got.tobytes() == R[k][idx].tobytes(), k
        assert not R[k][M[k] < 0].tobytes().strip(b"\0")
        # the update: exactly the accepted features leave, and a feature matched in a round was free and on an enabled camera
        assert np.array_equal(S[k + 1], np.where(R[k]["outcome"] == tm.ACCEPTED, 0, S[k]))
        assert S[k][idx].all() and b.cam_enabled[w.kf_a.cam_of[idx]].all()


def test_the_contested_feature_goes_to_the_later_one_only_with_the_update():
    w, i0, i1, j = nw.contested_world()
    M, R, _ = nw.chain(w)
    M0, _, _ = nw.chain(w, update=False)
    assert R[0]["outcome"][i0] == tm.ACCEPTED and M[0][i1] < 0
    assert M[1][i1] == j and M[1][i0] == -1 and M0[1][i0] == j


def run_driver(tmp_path, world, *args, driver=None, monocular=False):
    f = tmp_path / "world.txt"
    nw.write_world(f, world, monocular)
    p = subprocess.run(["timeout", "-k", "10", "120", driver or DRIVER, str(f)] + list(args), capture_output=True, text=True, timeout=150)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    return nw.parse_driver(p.stdout)


def check_host_mode(tmp_path, driver=None):
    w, _, _ = nw.world_and_chain(257, 4)
    got = run_driver(tmp_path, w, "host", driver=driver)
    seen = nw.as_the_class_read_it(w, got)
    want = [(k + 1,) + p for k, p in enumerate(nw.planned(seen)) if p is not None]
    assert len(got["rounds"]) == len(want) == 4
    for g, e in zip(got["rounds"], want):
        assert g[0] == e[0] and np.float32(g[1]).tobytes() == e[1].tobytes() and np.float32(g[2]).tobytes() == e[2].tobytes() and g[3] == e[3], (g, e)
    # capacity 3 over 5 keyframes: three created, three reused, the two beyond the capacity push the two oldest out, Forget drops the
    # last one, and the keyframe refilled under another id and then with another feature count is created anew both times
    assert got["cache"] == [(3, 0, 0, 3), (3, 3, 0, 3), (5, 3, 2, 3), (7, 3, 2, 2)], got["cache"]
    assert "holds 0 0 1 1 1" in got["other"] and "forget holds 0 size 2" in got["other"] and "dry run ok" in got["other"]


def test_class_driver_without_a_device(tmp_path):
    check_host_mode(tmp_path)


def test_monocular_plans_no_round(tmp_path):
    w, _, _ = nw.world_and_chain(63, 2)
    got = run_driver(tmp_path, w, "host", monocular=True)
    assert got["rounds"] == []


def test_class_driver_without_a_device_under_the_sanitizers(tmp_path):
    """The sanitized build of NewMapPoints.cc and its driver (host/Makefile `san`) as a stand-alone program: a report fails the run."""
    host = os.path.join(ROOT, "multi_orb_slam_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "test_new_points_keyframe_san"], timeout=900)
    check_host_mode(tmp_path, driver=os.path.join(host, "test_new_points_keyframe_san"))
