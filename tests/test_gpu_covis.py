"""GPU parity of the covisibility and culling counts over the resident map (orbm_map_covisibility, orbm_map_culling_counts) against
the library's host routines on plain arrays (which tests/test_covis_model.py holds to the model of the reference's functions).
Every comparison is equality of integers: entry for entry, count for count."""
import numpy as np
import pytest

import covis_worlds as cw
import frustum_worlds as fw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher():
    import multi_orb_slam_amd as m
    mt = m.Matcher(0.8, True)
    yield mt
    mt.close()


def both_calls_twice(rm, w, listed, n_live_slab, expect_rebuild=True):
    """Covisibility and culling (mono off and on) of the listed keyframes against the host routines; every call twice, the index
    built by the first call alone."""
    import multi_orb_slam_amd as m
    listed = np.asarray(listed, np.int32)
    e_cov, e_cull = cw.host(m, w, listed)
    e_mono = cw.host(m, w, listed, True)[1]
    for call in range(2):
        cov = rm.covisibility(listed)
        last = rm.last_covisibility()
        assert last == (1, 1 if (call == 0 and expect_rebuild) else 0, n_live_slab, len(listed)), last
        assert cw.same_lists(cov, e_cov)
        cull = rm.culling_counts(listed)
        assert rm.last_covisibility() == (1, 0, n_live_slab, len(listed))
        assert cull.dtype == np.int32 and np.array_equal(cull, e_cull)
        assert np.array_equal(rm.culling_counts(listed, mono=True), e_mono)
    print("covisibility: %d keyframes listed of %d, %d record slots -> %d entries, %d counted points, %d redundant"
          % (len(listed), w["n_kfs"], n_live_slab, sum(len(e) for e in e_cov), int(e_cull[:, 0].sum()), int(e_cull[:, 1].sum())))
    return e_cov, e_cull


@pytest.mark.parametrize("n_rec", [0, 1, 63, 64, 65, 70000])
def test_record_counts(matcher, n_rec):
    """The slab holds exactly n_rec record slots, every one written (k_map_chain: one lane per slot, 64 lanes a wave, 256 a
    workgroup).  The rows keep the points whose records were cut off: entries without a record of their own."""
    import multi_orb_slam_amd as m
    if n_rec > 1000:
        w = cw.make_world(100 + n_rec, 257, 3000, 512, n_rec + 4, min_count=440)
    else:
        w = cw.make_world(100 + n_rec, 257, 8, 96, n_rec + 4)             # few points: the few records share them
    assert len(w["obs"]) >= n_rec
    w["obs"] = w["obs"][:n_rec].copy(); w["obs_feat"] = w["obs_feat"][:n_rec].copy()
    assert n_rec < 63 or 0 < (w["obs"]["point"] < 0).sum() < n_rec / 2
    with cw.to_resident(m, matcher, w) as rm:
        listed = np.random.default_rng(n_rec + 1).permutation(257)[:40]
        e_cov, e_cull = both_calls_twice(rm, w, listed, n_rec, expect_rebuild=n_rec > 0)
        assert n_rec < 63 or sum(len(e) for e in e_cov) > 10
        assert n_rec < 70000 or (sum(len(e) for e in e_cov) > 1000 and e_cull[:, 1].sum() > 0)


@pytest.mark.parametrize("n_kfs", [1, 2, 255, 256, 257, 4096, 16384])
def test_keyframe_counts_of_the_map(matcher, n_kfs):
    """The bins of k_map_covis: one per keyframe of the map, cleared and compacted 256 at a time; 16 384 is the largest map (64 KiB)."""
    import multi_orb_slam_amd as m
    w = cw.make_world(200 + n_kfs, n_kfs, 400, 12, 6000, min_count=4)
    rng = np.random.default_rng(n_kfs)
    listed = np.concatenate([[0, n_kfs - 1], rng.permutation(n_kfs)[:30]])
    if n_kfs >= 255:
        # a good point of a listed keyframe's row gets the first and the last keyframe of the map as observers: entries in the
        # first and the last bin
        def good_points(k):
            row = w["kf_rows"][k, :w["kf_count"][k]]
            return row[(row >= 0) & (w["flags"][np.maximum(row, 0)] == 0)]
        j = next(j for j in range(2, len(listed)) if 0 < listed[j] < n_kfs - 1 and len(good_points(listed[j])))
        g = int(good_points(listed[j])[0])
        have = set(w["obs"]["keyframe"][w["obs"]["point"] == g].tolist())
        extra = np.array([(g, e) for e in (0, n_kfs - 1) if e not in have], cw.OBS_DTYPE).reshape(-1)
        w["obs"] = np.concatenate([w["obs"], extra]); w["obs_feat"] = np.concatenate([w["obs_feat"], np.zeros(len(extra), np.int32)])
    with cw.to_resident(m, matcher, w) as rm:
        assert rm.keyframes == n_kfs
        e_cov, _ = both_calls_twice(rm, w, listed, len(w["obs"]))
        if n_kfs >= 255:
            assert e_cov[j]["keyframe"][0] == 0 and e_cov[j]["keyframe"][-1] == n_kfs - 1   # entries at both ends of the bins


@pytest.fixture(scope="module")
def big_world(matcher):
    import multi_orb_slam_amd as m
    w = cw.make_world(7, 4096, 3000, 24, 40000, min_count=6)
    rm = cw.to_resident(m, matcher, w)
    yield dict(w=w, rm=rm)
    rm.close()


@pytest.mark.parametrize("n_call", [0, 1, 2, 64, 65, 4096])
def test_keyframes_per_call(matcher, big_world, n_call):
    w, rm = big_world["w"], big_world["rm"]
    listed = np.random.default_rng(n_call).permutation(4096)[:n_call]
    if n_call == 65:
        listed[-1] = listed[0]                                          # a keyframe named twice: two equal lists
    both_calls_twice(rm, w, listed, len(w["obs"]), expect_rebuild=False if rm.last_covisibility()[2] else True)


@pytest.mark.parametrize("row", [1, 63, 64, 65, 8192])
def test_row_lengths(matcher, row):
    """Keyframe 0 has exactly `row` features, every one holding a point; lanes stride over the row 256 at a time."""
    import multi_orb_slam_amd as m
    stride = 8192 if row == 8192 else 80
    n_points = 9000 if row == 8192 else 60
    w = cw.make_world(300 + row, 6, n_points, stride, 6 * stride // 2, min_count=max(stride // 2, 1))
    rng = np.random.default_rng(row)
    w["kf_count"][0] = row
    seen = w["obs"]["point"][(w["obs"]["point"] >= 0) & (w["obs"]["keyframe"] != 0)]
    w["kf_rows"][0, :] = -1; w["kf_rows"][0, :row] = rng.choice(seen, row)       # points other keyframes observe
    w["kf_ncam1"][0] = max(row - 1, 1)
    with cw.to_resident(m, matcher, w) as rm:
        e_cov, e_cull = both_calls_twice(rm, w, [0, 3, 0], len(w["obs"]))
        assert row < 63 or (len(e_cov[0]) > 0 and e_cull[0, 1] > 0)


def test_chains_of_1_2_and_300_records(matcher):
    """Point 0 is seen by 1 keyframe, point 1 by 2, point 2 by 300; each sits in the rows of keyframes 0 and 1 (twice in keyframe 1's)."""
    import multi_orb_slam_amd as m
    n_kfs, stride = 301, 8
    w = cw.empty_world(n_kfs, 4, stride, 400)
    rng = np.random.default_rng(3)
    w["kf_feat"] = rng.integers(0, 8, (n_kfs, stride)).astype(np.uint8); w["kf_ncam1"][:] = rng.integers(0, stride + 1, n_kfs)
    w["n_obs"][:] = [1, 2, 300, 0]
    slots = rng.permutation(400).tolist()
    chains = {0: [0], 1: [0, 7], 2: list(range(1, 301))}
    for p, ks in chains.items():
        for k in ks:
            f = int(rng.integers(0, stride))
            while w["kf_rows"][k, f] >= 0:
                f = (f + 1) % stride
            cw._put(w, k, f, p, level=int(w["kf_feat"][k, f]) & 7, slot=slots.pop())
    w["kf_count"][:] = stride
    w["kf_rows"][0, np.nonzero(w["kf_rows"][0] < 0)[0][:1]] = 2          # keyframe 0 holds the long chain's point without a record
    spare = np.nonzero(w["kf_rows"][1] < 0)[0]
    w["kf_rows"][1, spare[0]] = 2; w["kf_rows"][1, spare[1]] = 0
    with cw.to_resident(m, matcher, w) as rm:
        e_cov, e_cull = both_calls_twice(rm, w, [0, 1, 7, 300], 400)
        assert len(e_cov[0]) == 300 and e_cov[1]["all"].max() == 2 and e_cull[0, 1] >= 1


@pytest.mark.parametrize("name", sorted(cw.hand_cases()))
def test_hand_built_cases(matcher, name):
    import multi_orb_slam_amd as m
    w, listed, e_cull, e_cov = cw.hand_cases()[name]
    with cw.to_resident(m, matcher, w) as rm:
        has_records = len(w["obs"]) > 0
        cov, cull = both_calls_twice(rm, w, np.arange(w["n_kfs"]), len(w["obs"]), expect_rebuild=has_records)
        if e_cull is not None:
            assert cull[listed].tolist() == [list(c) for c in e_cull]
        if e_cov is not None:
            assert np.array_equal(cov[listed[0]], cw.entries_of(e_cov))


def test_index_is_rebuilt_after_a_record_was_freed_and_its_slot_reused(matcher):
    import multi_orb_slam_amd as m
    w = cw.make_world(11, 60, 500, 40, 4000)
    listed = np.arange(60)
    with cw.to_resident(m, matcher, w, obs_capacity=len(w["obs"]) + 10) as rm:
        before = both_calls_twice(rm, w, listed, len(w["obs"]))
        # the records of point p go, their slots are taken by another point q in keyframes that do not hold q yet
        live = np.nonzero(w["obs"]["point"] >= 0)[0]
        per_point = np.bincount(w["obs"]["point"][live], minlength=500) * (w["flags"] == 0)
        p = int(per_point.argmax())
        gone = live[w["obs"]["point"][live] == p]
        assert len(gone) >= 3
        w["obs"][gone] = (-1, -1)
        rm.write_observations(gone, w["obs"][gone])
        mid = both_calls_twice(rm, w, listed, len(w["obs"]))
        assert not cw.same_lists(mid[0], before[0])
        per_point[p] = 0
        q = int(np.nonzero(per_point >= 2)[0][0])                            # a good point that some rows hold
        holders = set(w["obs"]["keyframe"][w["obs"]["point"] == q].tolist())
        new_kfs = [k for k in range(60) if k not in holders][:len(gone)]
        for r, k in zip(gone.tolist(), new_kfs):
            w["obs"][r] = (q, k); w["obs_feat"][r] = k % 40
        rm.write_observations(gone[::-1], w["obs"][gone[::-1]])
        assert rm.last_covisibility()[1] == 0
        rm.write_observation_features(gone, w["obs_feat"][gone])
        w["n_obs"][q] += len(gone); rm.write_point_nobs([q], [w["n_obs"][q]])
        after = both_calls_twice(rm, w, listed, len(w["obs"]))
        assert not cw.same_lists(after[0], mid[0])
        # a write of features, levels or n_obs alone leaves the index as it is
        rm.write_keyframe_features(3, w["kf_feat"][3], w["kf_ncam1"][3])
        both_calls_twice(rm, w, listed, len(w["obs"]), expect_rebuild=False)


def test_entries_cap_one_short_is_a_capacity_error_and_leaves_no_list(matcher):
    import multi_orb_slam_amd as m
    from multi_orb_slam_amd import _lib
    w = cw.make_world(12, 60, 500, 40, 4000)
    listed = np.arange(10, dtype=np.int32)
    with cw.to_resident(m, matcher, w) as rm:
        e_cov, _ = cw.host(m, w, listed)
        total = sum(len(e) for e in e_cov)
        assert total > 20
        assert cw.same_lists(rm.covisibility(listed, entries_cap=total), e_cov)
        with pytest.raises(m.OrbError) as e:
            rm.covisibility(listed, entries_cap=total - 1)
        assert e.value.code == _lib.ORB_E_CAPACITY and str(total) in str(e.value)
        first = np.full(len(listed) + 1, -7, np.int32); ent = np.zeros(total, m.COVIS_DTYPE)
        rc = _lib.lib().orbm_map_covisibility(matcher._h, rm._h, _lib.ptr(listed), len(listed), _lib.ptr(first), _lib.ptr(ent), total - 1)
        assert rc == _lib.ORB_E_CAPACITY and first[-1] == total and not first[:-1].any() and not ent.view(np.int32).any()
        assert cw.same_lists(rm.covisibility(listed), e_cov)                  # and the map still answers


def test_argument_errors(matcher):
    import multi_orb_slam_amd as m
    from multi_orb_slam_amd import _lib
    with m.ResidentMap(matcher, 4, 10, 10, 8) as rm:
        rm.write_keyframe(1, [3, -1, 3])
        for call, code in ((lambda: rm.write_observation_features([10], [0]), _lib.ORB_E_CAPACITY),
                           (lambda: rm.write_observation_features([-1], [0]), _lib.ORB_E_ARG),
                           (lambda: rm.write_observation_features([0], [8]), _lib.ORB_E_CAPACITY),
                           (lambda: rm.write_observation_features([0], [-1]), _lib.ORB_E_ARG),
                           (lambda: rm.write_point_nobs([10], [1]), _lib.ORB_E_CAPACITY), (lambda: rm.write_point_nobs([-1], [1]), _lib.ORB_E_ARG),
                           (lambda: rm.write_keyframe_features(4, [0], 0), _lib.ORB_E_CAPACITY),
                           (lambda: rm.write_keyframe_features(-1, [0], 0), _lib.ORB_E_ARG),
                           (lambda: rm.write_keyframe_features(0, [0] * 9, 0), _lib.ORB_E_CAPACITY),
                           (lambda: rm.write_keyframe_features(0, [0], 9), _lib.ORB_E_CAPACITY),
                           (lambda: rm.covisibility([2]), _lib.ORB_E_ARG), (lambda: rm.culling_counts([-1]), _lib.ORB_E_ARG),
                           (lambda: rm.covisibility(np.zeros(m.MAP_MAX_LOCAL + 1, np.int32)), _lib.ORB_E_CAPACITY),
                           (lambda: rm.culling_counts(np.zeros(m.MAP_MAX_LOCAL + 1, np.int32)), _lib.ORB_E_CAPACITY)):
            with pytest.raises(m.OrbError) as e:
                call()
            assert e.value.code == code
        # a refused write wrote nothing: the facts are what a map holds that was never written
        assert rm.culling_counts([1]).tolist() == [[2, 0]] and [len(e) for e in rm.covisibility([0, 1])] == [0, 0]


def test_vote_point_list_and_search_are_untouched_by_the_new_facts(matcher):
    """The three calls of the tracking thread return the same arrays before and after the four new facts are written and the index
    is built."""
    import multi_orb_slam_amd as m
    case = (500, [1000, 500], 640, 480, 1, 1.0)
    fwd = fw.make_world(*case)
    n = case[0]; nf = len(fwd["fr"]["un_x"])
    rng = np.random.default_rng(17)
    n_kfs, stride = 6, 200
    w = cw.make_world(13, n_kfs, n, stride, 800)
    F = matcher.frame(m.FrameData(**fwd["fr"]))
    view = fwd["view"].native()
    fp = np.where(rng.random(nf) < 0.3, rng.integers(0, n, nf), -1).astype(np.int32)
    with m.ResidentMap(matcher, n_kfs, n, len(w["obs"]), stride) as rm:
        rm.write_points(np.arange(n), fwd["points"], w["flags"])
        for k in range(n_kfs):
            rm.write_keyframe(k, w["kf_rows"][k, :w["kf_count"][k]])
        rm.write_observations(np.arange(len(w["obs"])), w["obs"])

        def tracking_calls():
            votes = rm.vote(fp)
            lst = rm.local_points(np.arange(n_kfs))
            ntm, nm, mo, track = rm.search(F, view, fp[:50], lst[:7], n_list=len(lst))
            return votes.tobytes(), lst.tobytes(), (ntm, nm), mo.tobytes(), track.tobytes()

        before = tracking_calls()
        assert before[2][0] > 0 and np.frombuffer(before[0], np.int32).sum() > 0
        rm.write_point_nobs(np.arange(n), w["n_obs"])
        rm.write_observation_features(np.arange(len(w["obs"])), w["obs_feat"])
        for k in range(n_kfs):
            rm.write_keyframe_features(k, w["kf_feat"][k], w["kf_ncam1"][k])
        both_calls_twice(rm, w, np.arange(n_kfs), len(w["obs"]))
        assert tracking_calls() == before
        both_calls_twice(rm, w, np.arange(n_kfs), len(w["obs"]), expect_rebuild=False)   # and the tracking calls leave the index alone
    F.close()


def test_host_route_of_the_map_gives_the_same_results():
    """MORB_HOST_RESOLVE=1 (read in orbm_create, hence a fresh child process): both calls through the host routines over the map's
    mirror (tests/covis_leg.py)."""
    import os
    import subprocess
    import sys
    leg = os.path.join(os.path.dirname(os.path.abspath(__file__)), "covis_leg.py")
    out = subprocess.run([sys.executable, leg], env=dict(os.environ, MORB_HOST_RESOLVE="1"), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "covis_leg ok" in out.stdout, out.stdout + out.stderr
