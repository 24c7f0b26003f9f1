"""The library's two host routines of the covisibility and culling counts (orbm_local_map_covisibility_host,
orbm_local_map_culling_host: the fallback of the device calls and their cross-check) against the model of tests/covis_model.py,
written from the reference's functions (src/KeyFrame.cc:486-552, src/LocalMapping.cc:966-1038).  Equality of integers; no device."""
import numpy as np
import pytest

import covis_model as cm
import covis_worlds as cw


@pytest.mark.parametrize("case", cw.CASES, ids=lambda c: "%dkf_%dpts" % (c[1], c[2]))
def test_host_routines_equal_the_model(case):
    import multi_orb_slam_amd as m
    w = cw.make_world(*case)
    rng = np.random.default_rng(case[0])
    listed = rng.permutation(w["n_kfs"])[:12].astype(np.int32)
    if case[1] >= 40:
        cw.check_conditions(w, listed)                       # the full-size worlds hold every case, asserted first
    objects = cm.build(w)
    for mono in (False, True):
        cov, cull = cw.host(m, w, listed, mono)
        assert cull.dtype == np.int32 and np.array_equal(cull, cm.culling_counts(w, listed, mono, objects))
        assert cw.same_lists(cov, cm.covisibility(w, listed, objects))
    # a keyframe named twice gets two equal lists, and the order of the call is the order of the answer
    twice = np.concatenate([listed[::-1], listed[:1]])
    cov2, cull2 = cw.host(m, w, twice)
    cov, cull = cw.host(m, w, listed)
    assert cw.same_lists(cov2, cov[::-1] + cov[:1]) and np.array_equal(cull2, np.concatenate([cull[::-1], cull[:1]]))


@pytest.mark.parametrize("name", sorted(cw.hand_cases()))
def test_hand_built_cases(name):
    import multi_orb_slam_amd as m
    w, listed, e_cull, e_cov = cw.hand_cases()[name]
    cov, cull = cw.host(m, w, listed)
    assert np.array_equal(cull, cm.culling_counts(w, listed)) and cw.same_lists(cov, cm.covisibility(w, listed))
    assert np.array_equal(cw.host(m, w, listed, True)[1], cm.culling_counts(w, listed, True))
    if e_cull is not None:
        assert cull.tolist() == [list(c) for c in e_cull]
    if e_cov is not None:
        assert np.array_equal(cov[0], cw.entries_of(e_cov))


def test_mono_skips_the_far_test():
    import multi_orb_slam_amd as m
    w, listed, e_cull, _ = cw.hand_cases()["far_feature"]
    assert cw.host(m, w, listed, False)[1].tolist() == [[1, 1]] and cw.host(m, w, listed, True)[1].tolist() == [[2, 2]]


def test_every_other_keyframe_of_a_hand_case_agrees_too():
    import multi_orb_slam_amd as m
    for name, (w, _, _, _) in cw.hand_cases().items():
        listed = np.arange(w["n_kfs"], dtype=np.int32)
        cov, cull = cw.host(m, w, listed)
        assert np.array_equal(cull, cm.culling_counts(w, listed)) and cw.same_lists(cov, cm.covisibility(w, listed)), name


def test_capacity_and_bad_arguments_are_loud():
    import multi_orb_slam_amd as m
    from multi_orb_slam_amd import _lib
    from multi_orb_slam_amd._lib import ptr
    w = cw.make_world(*cw.CASES[0])
    listed = np.arange(5, dtype=np.int32)
    cov = cm.covisibility(w, listed)
    total = sum(len(e) for e in cov)
    assert total > 5

    def call(cap, kfs=listed, obs=w["obs"], feat=w["obs_feat"]):
        first = np.zeros(len(kfs) + 1, np.int32); ent = np.zeros(max(cap, 1), cm.COVIS_DTYPE)
        rows = np.ascontiguousarray(w["kf_rows"]); kfs = np.ascontiguousarray(kfs, np.int32)
        rc = _lib.lib().orbm_local_map_covisibility_host(ptr(obs), ptr(feat), len(obs), ptr(w["flags"]), len(w["flags"]), ptr(rows),
                                                         ptr(w["kf_count"]), ptr(w["kf_ncam1"]), w["n_kfs"], w["stride"], ptr(kfs), len(kfs),
                                                         ptr(first), ptr(ent), cap)
        return rc, first, ent

    rc, first, ent = call(total)
    assert rc == 0 and first[-1] == total and np.array_equal(ent, np.concatenate(cov))
    rc, first, ent = call(total - 1)
    assert rc == _lib.ORB_E_CAPACITY and first[-1] == total           # the number needed is reported
    assert call(total, kfs=np.array([w["n_kfs"]], np.int32))[0] == _lib.ORB_E_ARG      # a keyframe outside the map
    live = np.nonzero(w["obs"]["point"] >= 0)[0][0]
    bad = w["obs"].copy(); bad["keyframe"][live] = w["n_kfs"]
    assert call(total, obs=bad)[0] == _lib.ORB_E_ARG                   # a record outside the map
    feat = w["obs_feat"].copy(); feat[live] = w["stride"]
    assert call(total, feat=feat)[0] == _lib.ORB_E_ARG                 # a feature outside the row
    with pytest.raises(m.OrbError):
        m.local_map_culling_host(bad, w["obs_feat"], w["flags"], w["n_obs"], w["kf_rows"], w["kf_count"], w["kf_feat"], listed)


@pytest.mark.parametrize("red,mps,verdict", [(9, 10, False), (10, 10, True), (0, 0, False)])
def test_the_ninety_percent_rule_of_the_model(red, mps, verdict):
    """nRedundantObservations > 0.90 * nMPs in double: 9 of 10 stays (9 > 9.0 is false), 10 of 10 goes, an empty keyframe stays."""
    assert cm.culled(red, mps) is verdict
