"""The library's two host routines of the local map (orbm_local_map_vote_host, orbm_local_map_points_host: the fallback of the
device calls and their cross-check) against the model of tests/localmap_model.py, written from the reference's loops
(src/Tracking.cc:1794-1949).  Equality of integers; no device."""
import numpy as np
import pytest

import localmap_model as lm
import localmap_worlds as lw


def routines(w, local_kfs=None):
    import multi_orb_slam_amd as m
    v = m.local_map_vote_host(w["obs"], w["flags"], w["frame_points"], w["n_kfs"])
    lst = m.local_map_points_host(w["kf_rows"], w["kf_count"], w["flags"], w["local_kfs"] if local_kfs is None else local_kfs)
    return v, lst


@pytest.mark.parametrize("case", lw.CASES, ids=lambda c: "%dkf_%dpts" % (c[1], c[2]))
def test_host_routines_equal_the_model(case):
    w = lw.make_world(*case)
    if case[1] >= 40:
        e_votes, e_list = lw.check_conditions(w)          # the full-size worlds hold every case, asserted first
    else:
        e_votes = lm.votes(w["obs"], w["flags"], w["frame_points"], w["n_kfs"])
        e_list = lm.local_points(w["kf_rows"], w["kf_count"], w["flags"], w["local_kfs"])
    v, lst = routines(w)
    assert v.dtype == np.int32 and np.array_equal(v, e_votes)
    assert np.array_equal(lst, e_list)
    # the order of the local keyframes decides the order of the list, not its content
    rev = w["local_kfs"][::-1].copy()
    e_rev = lm.local_points(w["kf_rows"], w["kf_count"], w["flags"], rev)
    assert np.array_equal(routines(w, rev)[1], e_rev)
    assert sorted(e_rev.tolist()) == sorted(e_list.tolist())
    if len(e_list) > 1 and len(w["local_kfs"]) > 1:
        assert not np.array_equal(e_rev, e_list)
    # a keyframe listed twice adds nothing
    twice = np.concatenate([w["local_kfs"], w["local_kfs"][:1]])
    assert np.array_equal(routines(w, twice)[1], e_list)


def test_a_point_at_two_features_votes_twice_and_a_bad_one_not_at_all():
    obs = np.array([(0, 1), (-1, -1), (1, 1), (1, 2), (2, 0)], lw.OBS_DTYPE)
    flags = np.array([0, 0, 1], np.uint8)
    import multi_orb_slam_amd as m
    v = m.local_map_vote_host(obs, flags, [1, -1, 1, 0, 2, 2], 3)
    assert v.tolist() == [0, 3, 2] == lm.votes(obs, flags, [1, -1, 1, 0, 2, 2], 3).tolist()


def test_every_candidate_bad_or_empty_gives_an_empty_list_and_no_votes():
    w = lw.make_barren_world(9)
    assert np.all(w["flags"] & lm.BAD) and np.any(w["kf_rows"] >= 0)
    v, lst = routines(w)
    assert len(lst) == 0 and len(lm.local_points(w["kf_rows"], w["kf_count"], w["flags"], w["local_kfs"])) == 0
    assert not v.any() and not lm.votes(w["obs"], w["flags"], w["frame_points"], w["n_kfs"]).any()


def test_list_capacity_and_bad_arguments_are_loud():
    import multi_orb_slam_amd as m
    from multi_orb_slam_amd import _lib
    w = lw.make_world(*lw.CASES[0])
    e_list = lm.local_points(w["kf_rows"], w["kf_count"], w["flags"], w["local_kfs"])
    assert np.array_equal(m.local_map_points_host(w["kf_rows"], w["kf_count"], w["flags"], w["local_kfs"], len(e_list)), e_list)
    with pytest.raises(m.OrbError) as e:
        m.local_map_points_host(w["kf_rows"], w["kf_count"], w["flags"], w["local_kfs"], len(e_list) - 1)
    assert e.value.code == _lib.ORB_E_CAPACITY
    with pytest.raises(m.OrbError) as e:                            # a local keyframe outside the map
        m.local_map_points_host(w["kf_rows"], w["kf_count"], w["flags"], [w["n_kfs"]])
    assert e.value.code == _lib.ORB_E_ARG
    bad = w["obs"].copy(); bad["keyframe"][np.nonzero(bad["point"] >= 0)[0][0]] = w["n_kfs"]
    with pytest.raises(m.OrbError) as e:                            # a record outside the map
        m.local_map_vote_host(bad, w["flags"], w["frame_points"], w["n_kfs"])
    assert e.value.code == _lib.ORB_E_ARG


def test_k2_walk_of_the_model_leaves_the_outer_loop_at_the_parent():
    """The parent branch's break (:1938) ends the whole walk: with it the second K1 keyframe contributes nothing."""
    n = 8
    counter = np.zeros(n, np.int32); counter[[1, 2]] = [3, 5]
    none = [[] for _ in range(n)]
    neighbours = [list(x) for x in none]; neighbours[1] = [4]; neighbours[2] = [5]
    children = [set() for _ in range(n)]; children[2] = {6}
    parent = [-1] * n; parent[1] = 7
    bad = np.zeros(n, np.uint8)
    with_break = lm.local_keyframes(counter, bad, neighbours, children, parent, [-1] * n, 3)
    without = lm.local_keyframes(counter, bad, neighbours, children, parent, [-1] * n, 3, outer_break=False)
    assert with_break == ([1, 2, 4, 7], 2)
    assert without == ([1, 2, 4, 7, 5, 6], 2)
    assert lm.local_keyframes(np.zeros(n, np.int32), bad, neighbours, children, parent, [-1] * n, 3) is None
