"""CreateNewPointsOfKeyFrame and ResidentKeyFrames (host/NewMapPoints.h) through their driver host/test_new_points_keyframe: stand-in
keyframes written from a world of tests/new_points_worlds.py; per neighbour the pairs and verdicts against the CPU reference chain run
with the istrian the class derives from the baselines; a neighbour below both baselines; the resident keyframes of a second call."""
import numpy as np
import pytest

import new_points_worlds as nw
import triangulate_model as tm
from test_new_points_keyframe_model import run_driver


def planned_world(world, parsed):
    """The world as the class read it, without the neighbours it skips and with the istrian it derives (:338-341) in place of the
    world's own camera cycle -> (world, indices of the kept neighbours in the file: 1-based, the current keyframe is 0)."""
    seen = nw.as_the_class_read_it(world, parsed)
    keep, nb = [], []
    for k, p in enumerate(nw.planned(seen)):
        if p is not None:
            seen.nb[k].cam_enabled = np.array(p[2], np.uint8)
            keep.append(k + 1); nb.append(seen.nb[k])
    return nw.World(seen.kf_a, seen.side_a, nb), keep


def compare(world, got):
    w, keep = planned_world(world, got)
    assert [r[0] for r in got["rounds"]] == keep
    M, R, _ = nw.chain(w)
    assert len(got["calls"]) == 2
    for call in got["calls"]:
        assert sorted(call) == keep
        for k, j in enumerate(keep):
            pairs, rec, has = call[j]
            idx = np.flatnonzero(M[k] >= 0)
            assert np.array_equal(pairs, np.stack([idx, M[k][idx]], 1)), (j, "pairs")
            assert np.array_equal(rec["outcome"], R[k]["outcome"][idx]) and rec["x3D"].tobytes() == R[k]["x3D"][idx].tobytes(), (j, "verdicts")
            assert np.array_equal(has, R[k]["path"][idx] != tm.PATH_NONE)
    # the second call is served by the keyframes the first one made resident; Forget drops one of them
    n = len(keep) + 1
    assert got["cache"] == [(n, 0, 0, n), (n, n, 0, n)], got["cache"]
    assert "forget held 1 holds 0 size %d" % (n - 1) in got["other"]
    return M, R


@pytest.mark.gpu
def test_class_on_the_600_x_5_world(tmp_path):
    import torch  # noqa: F401
    world, _, _ = nw.world_and_chain(600, 5)
    M, R = compare(world, run_driver(tmp_path, world))
    assert ((M >= 0).sum(1) >= 20).all() and (R["outcome"] == tm.ACCEPTED).sum() > 200


@pytest.mark.gpu
def test_a_neighbour_below_both_baselines_is_skipped(tmp_path):
    import torch  # noqa: F401
    world = nw.make_world(257, 3, baselines=(0.27, 0.02, 0.30))
    got = run_driver(tmp_path, world)
    assert [r[0] for r in got["rounds"]] == [1, 3]
    compare(world, got)


def test_the_skipped_neighbour_without_a_device(tmp_path):
    world = nw.make_world(257, 3, baselines=(0.27, 0.02, 0.30))
    got = run_driver(tmp_path, world, "host")
    _, keep = planned_world(world, got)
    assert [r[0] for r in got["rounds"]] == keep == [1, 3]
