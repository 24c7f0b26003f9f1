"""GPU parity of the resident map (orbm_map_*): the keyframe votes and the point list against the library's host routines on plain
arrays (which tests/test_localmap_model.py holds to the model of the reference's loops), the search over the map against the
existing orbm_search_local_points over a table written in list order.  Every comparison is equality of integers or of raw bytes."""
import numpy as np
import pytest

import frustum_worlds as fw
import localmap_worlds as lw

pytestmark = pytest.mark.gpu

VOTE_BLOCK = 256 * 16          # records one workgroup of k_map_vote is sized for (MAP_BLOCK * MAP_VOTE_PER_LANE)
COMPACT_BLOCK = 256            # candidates per block of the compaction (MAP_BLOCK)


@pytest.fixture(scope="module")
def matcher():
    import multi_orb_slam_amd as m
    mt = m.Matcher(0.8, True)
    yield mt
    mt.close()


def random_records(rng, n_rec, n_points, n_kfs, free=0.15):
    """n_rec records over distinct (point, keyframe) pairs, about `free` of them free."""
    pairs = rng.choice(n_points * n_kfs, min(n_rec, n_points * n_kfs), replace=False) if n_rec else np.zeros(0, np.int64)
    obs = np.zeros(n_rec, lw.OBS_DTYPE); obs["point"] = -1; obs["keyframe"] = -1
    obs["point"][:len(pairs)] = pairs // n_kfs; obs["keyframe"][:len(pairs)] = pairs % n_kfs
    gone = rng.random(n_rec) < free
    obs["point"][gone] = -1; obs["keyframe"][gone] = -1
    return obs


def random_frame(rng, n_frame, n_points, flags):
    fp = np.where(rng.random(n_frame) < 0.7, rng.integers(0, n_points, n_frame), -1).astype(np.int32)
    if n_frame >= 3:
        fp[0] = fp[-1] = np.nonzero(flags == 0)[0][0]         # one point at two features
        fp[1] = np.nonzero(flags != 0)[0][0]                  # a bad one
    return fp


def vote_case(mt, n_rec, n_kfs, n_frame, kf_capacity=None, seed=0):
    import multi_orb_slam_amd as m
    rng = np.random.default_rng(1000 * seed + n_rec + 7 * n_kfs + n_frame)
    n_points = 300
    flags = (rng.random(n_points) < 0.1).astype(np.uint8); flags[:2] = [0, 1]
    obs = random_records(rng, n_rec, n_points, n_kfs)
    with m.ResidentMap(mt, n_kfs if kf_capacity is None else kf_capacity, n_points, max(n_rec, 1), 4) as rm:
        rm.write_points(np.arange(n_points), np.zeros(n_points, m.POINT_DTYPE), flags)
        rm.write_keyframe(n_kfs - 1, [])                        # the high-water mark of the keyframes
        if n_rec:
            rm.write_observations(np.arange(n_rec), obs)
        assert rm.keyframes == n_kfs
        for call in range(2):                                  # the second call finds the scratch as clean as the first
            fp = random_frame(rng, n_frame, n_points, flags)
            exp = m.local_map_vote_host(obs, flags, fp, n_kfs)
            got = rm.vote(fp)
            print("vote: %d records, %d keyframes, %d features, call %d -> %d votes" % (n_rec, n_kfs, n_frame, call, int(got.sum())))
            assert got.dtype == np.int32 and np.array_equal(got, exp)
            assert mt.last_local_map(rm)[:2] == (1, n_rec)
        return int(exp.sum())


@pytest.mark.parametrize("n_rec", [0, 1, 63, 64, 65, 255, 256, 257, VOTE_BLOCK - 1, VOTE_BLOCK, VOTE_BLOCK + 1, 70000])
def test_vote_record_counts(matcher, n_rec):
    total = vote_case(matcher, n_rec, 257, 2000)
    assert total > 0 or n_rec < 63


@pytest.mark.parametrize("n_kfs,cap", [(1, None), (2, None), (257, None), (300, 300), (16384, 16384)])
def test_vote_keyframe_counts(matcher, n_kfs, cap):
    """1, 2, 257 keyframes, and a map whose every keyframe slot is in use (the largest map: 64 KiB of bins per workgroup)."""
    assert vote_case(matcher, VOTE_BLOCK + 1, n_kfs, 2000, cap) > 0


def test_vote_frame_of_one_feature(matcher):
    vote_case(matcher, 5000, 257, 1)
    vote_case(matcher, 5000, 257, 2)


def test_vote_after_records_were_freed_and_reused(matcher):
    import multi_orb_slam_amd as m
    rng = np.random.default_rng(77)
    n_points, n_kfs, n_rec = 300, 40, 6000
    flags = (rng.random(n_points) < 0.1).astype(np.uint8); flags[:2] = [0, 1]
    obs = random_records(rng, n_rec, n_points, n_kfs)
    with m.ResidentMap(matcher, 64, n_points, 8000, 4) as rm:
        rm.write_points(np.arange(n_points), np.zeros(n_points, m.POINT_DTYPE), flags)
        rm.write_observations(np.arange(n_rec), obs)
        fp = random_frame(rng, 500, n_points, flags)
        before = rm.vote(fp)
        assert np.array_equal(before, m.local_map_vote_host(obs, flags, fp, n_kfs))
        # free every record of point fp[0] and 500 others, then reuse some of the freed slots and new ones behind the slab for
        # pairs that are not in the map yet (slots in scattered order, one call each)
        freed = np.unique(np.concatenate([np.nonzero(obs["point"] == fp[0])[0], rng.permutation(n_rec)[:500]])).astype(np.int32)
        assert np.any(obs["point"][freed] == fp[0])
        obs[freed] = (-1, -1)
        rm.write_observations(rng.permutation(freed), np.full(len(freed), -1, np.int32).repeat(2).view(lw.OBS_DTYPE))
        mid = rm.vote(fp)
        assert np.array_equal(mid, m.local_map_vote_host(obs, flags, fp, n_kfs)) and mid.sum() < before.sum()
        have = set(zip(obs["point"].tolist(), obs["keyframe"].tolist()))
        new = [(p, k) for p, k in zip(rng.integers(0, n_points, 900).tolist(), rng.integers(0, n_kfs, 900).tolist()) if (p, k) not in have]
        new = np.array(sorted(set(new))[:400], np.int32).view(lw.OBS_DTYPE).reshape(-1)
        slots = np.concatenate([freed[:len(new) // 2], np.arange(n_rec, n_rec + len(new) - len(new) // 2)]).astype(np.int32)
        slots = slots[rng.permutation(len(slots))]
        grown = np.concatenate([obs, np.full(2 * (len(new) - len(new) // 2), -1, np.int32).view(lw.OBS_DTYPE)])
        grown[slots] = new
        rm.write_observations(slots, new)
        after = rm.vote(fp)
        assert np.array_equal(after, m.local_map_vote_host(grown, flags, fp, n_kfs)) and after.sum() > mid.sum()
        assert matcher.last_local_map(rm)[1] == len(grown)


# ---- the point list -------------------------------------------------------------------------------------------------------------

LIST_KFS, LIST_POINTS, LIST_STRIDE = 300, 30000, 2000


@pytest.fixture(scope="module")
def list_world(matcher):
    """300 keyframes of 1 to 2 000 features over 30 000 point slots, written once: rows with empty features, bad points and points
    that sit twice in a row and in many rows.  Keyframes 0 .. 7 have 1, 2 and the compaction's block size - 1, +0, +1 features."""
    import multi_orb_slam_amd as m
    rng = np.random.default_rng(5)
    flags = (rng.random(LIST_POINTS) < 0.08).astype(np.uint8)
    rows = np.where(rng.random((LIST_KFS, LIST_STRIDE)) < 0.75, rng.integers(0, LIST_POINTS, (LIST_KFS, LIST_STRIDE)), -1).astype(np.int32)
    count = rng.integers(1, LIST_STRIDE + 1, LIST_KFS).astype(np.int32)
    count[:8] = [1, 2, COMPACT_BLOCK - 1, COMPACT_BLOCK, COMPACT_BLOCK + 1, LIST_STRIDE, 2 * COMPACT_BLOCK, 2 * COMPACT_BLOCK + 1]
    rows[0, 0] = np.nonzero(flags == 0)[0][0]
    rows[8, :] = -1; rows[9, :] = np.nonzero(flags != 0)[0][:1]        # an empty keyframe and one of bad points only
    for k in range(LIST_KFS):
        rows[k, count[k]:] = -1
    rm = m.ResidentMap(matcher, LIST_KFS, LIST_POINTS, 1, LIST_STRIDE)
    rm.write_points(np.arange(LIST_POINTS), np.zeros(LIST_POINTS, m.POINT_DTYPE), flags)
    for k in range(LIST_KFS):
        rm.write_keyframe(k, rows[k, :count[k]])
    yield dict(rm=rm, rows=rows, count=count, flags=flags)
    rm.close()


def list_case(mt, W, local_kfs):
    import multi_orb_slam_amd as m
    local_kfs = np.asarray(local_kfs, np.int32)
    exp = m.local_map_points_host(W["rows"], W["count"], W["flags"], local_kfs)
    got = W["rm"].local_points(local_kfs)
    cand = int(W["count"][local_kfs].sum())
    print("point list: %d keyframes, %d candidates -> %d kept" % (len(local_kfs), cand, len(got)))
    assert got.dtype == np.int32 and np.array_equal(got, exp)
    assert mt.last_local_map(W["rm"])[0] == 1 and mt.last_local_map(W["rm"])[2:] == (cand, len(exp))
    return exp


@pytest.mark.parametrize("n_local", [1, 2, 81, 300])
def test_point_list_local_keyframe_counts(matcher, list_world, n_local):
    rng = np.random.default_rng(n_local)
    for _ in range(2):                                           # two orders of the same call: the marks of the first do not survive
        kfs = rng.permutation(LIST_KFS)[:n_local]
        if n_local == 300:
            kfs = kfs[:60]                                       # (all 300 rows hold more points than a list takes: see the capacity test)
            kfs = np.concatenate([kfs, kfs[::-1], kfs, kfs, kfs])   # 300 listed keyframes, every one five times
        exp = list_case(matcher, list_world, kfs)
        assert n_local < 81 or len(exp) < int(list_world["count"][kfs].sum()) * 0.7   # duplicates were dropped


@pytest.mark.parametrize("kfs", [[0], [1], [2], [3], [4], [5], [6], [7], [2, 3], [3, 4], [4, 2, 3], [7, 6, 0]], ids=str)
def test_point_list_candidate_counts_around_the_block_size(matcher, list_world, kfs):
    """Rows of 1, 2, 255, 256, 257, 2 000, 512 and 513 features, alone and together."""
    list_case(matcher, list_world, kfs)


def test_point_list_empty_results(matcher, list_world):
    assert len(list_case(matcher, list_world, [8])) == 0          # an empty keyframe
    assert len(list_case(matcher, list_world, [9])) == 0          # bad points only
    assert len(list_case(matcher, list_world, [8, 9, 8])) == 0
    assert len(list_case(matcher, list_world, [])) == 0           # no local keyframe at all
    assert len(list_case(matcher, list_world, [5])) > 0           # and the map still answers


def test_point_list_at_the_capacity_of_a_search(matcher):
    """33 keyframes of 2 000 distinct points, the last one trimmed: exactly ORBM_MAX_POINTS kept points; one more is ORB_E_CAPACITY."""
    import multi_orb_slam_amd as m
    from multi_orb_slam_amd import _lib
    n = m.MAX_POINTS + 1
    with m.ResidentMap(matcher, 34, n, 1, 2000) as rm:
        slots = np.random.default_rng(3).permutation(n).astype(np.int32)
        rows = np.full((33, 2000), -1, np.int32); count = np.full(33, 2000, np.int32); count[32] = n - 1 - 32 * 2000
        for k in range(33):
            rows[k, :count[k]] = slots[k * 2000:k * 2000 + count[k]]
            rm.write_keyframe(k, rows[k, :count[k]])
        flags = np.zeros(n, np.uint8)
        got = rm.local_points(np.arange(33))
        assert len(got) == m.MAX_POINTS and np.array_equal(got, slots[:m.MAX_POINTS])
        assert np.array_equal(got, m.local_map_points_host(rows, count, flags, np.arange(33)))
        count[32] += 1; rows[32, count[32] - 1] = slots[n - 1]
        rm.write_keyframe(32, rows[32, :count[32]])
        with pytest.raises(m.OrbError) as e:
            rm.local_points(np.arange(33))
        assert e.value.code == _lib.ORB_E_CAPACITY
        flags[slots[5]] = 1                                          # one point goes bad: the list fits again
        rm.write_points([slots[5]], np.zeros(1, m.POINT_DTYPE), [1])
        got = rm.local_points(np.arange(33))
        assert len(got) == m.MAX_POINTS and np.array_equal(got, m.local_map_points_host(rows, count, flags, np.arange(33)))


def test_map_argument_errors(matcher):
    import multi_orb_slam_amd as m
    from multi_orb_slam_amd import _lib
    for args in ((m.MAP_MAX_KEYFRAMES + 1, 10, 10, 10), (10, 10, 10, m.MAP_MAX_FEATURES + 1)):
        with pytest.raises(m.OrbError) as e:
            m.ResidentMap(matcher, *args)
        assert e.value.code == _lib.ORB_E_CAPACITY
    with m.ResidentMap(matcher, 4, 10, 10, 8) as rm:
        z = np.zeros(1, m.POINT_DTYPE)
        for call, code in ((lambda: rm.write_points([10], z), _lib.ORB_E_CAPACITY), (lambda: rm.write_points([-1], z), _lib.ORB_E_ARG),
                           (lambda: rm.write_observations([10], np.array([(0, 0)], lw.OBS_DTYPE)), _lib.ORB_E_CAPACITY),
                           (lambda: rm.write_observations([0], np.array([(10, 0)], lw.OBS_DTYPE)), _lib.ORB_E_CAPACITY),
                           (lambda: rm.write_observations([0], np.array([(0, 4)], lw.OBS_DTYPE)), _lib.ORB_E_CAPACITY),
                           (lambda: rm.write_keyframe(4, [0]), _lib.ORB_E_CAPACITY), (lambda: rm.write_keyframe(0, [0] * 9), _lib.ORB_E_CAPACITY),
                           (lambda: rm.write_keyframe(0, [10]), _lib.ORB_E_CAPACITY), (lambda: rm.vote([10]), _lib.ORB_E_ARG),
                           (lambda: rm.local_points([0]), _lib.ORB_E_ARG)):      # (no keyframe written yet)
            with pytest.raises(m.OrbError) as e:
                call()
            assert e.value.code == code
        rm.write_keyframe(1, [3, -1, 3], bad=True)
        assert rm.keyframes == 2 and rm.keyframe_bad(1) and not rm.keyframe_bad(0)
        rm.set_keyframe_bad(1, False)
        assert not rm.keyframe_bad(1)
        assert rm.local_points([1, 0]).tolist() == [3]
        with pytest.raises(m.OrbError) as e:
            rm.local_points(np.zeros(m.MAP_MAX_LOCAL + 1, np.int32))
        assert e.value.code == _lib.ORB_E_CAPACITY
        other = m.Matcher(0.8, True)                                 # a map belongs to the handle that made it
        try:
            fp = np.zeros(1, np.int32); votes = np.zeros(4, np.int32)
            assert _lib.lib().orbm_map_vote(other._h, rm._h, _lib.ptr(fp), 1, _lib.ptr(votes)) == _lib.ORB_E_ARG
        finally:
            other.close()


# ---- the search -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [(500, [1000, 500], 640, 480, 1, 1.0), (8000, [2000, 2000], 1280, 720, 4, 3.0)],
                         ids=lambda c: "%dpts_th%g" % (c[0], c[5]))
def test_search_over_the_map_equals_the_search_over_a_table_in_list_order(matcher, case):
    """The points of a frustum world scattered over a map of four times as many slots, listed through keyframe rows; the existing
    orbm_search_local_points gets the same points as a table in list order with the skip flags computed here."""
    import multi_orb_slam_amd as m
    w = fw.make_world(*case)
    n = case[0]; nf = len(w["fr"]["un_x"])
    rng = np.random.default_rng(case[4] + 300)
    slots = rng.permutation(4 * n)[:n].astype(np.int32)
    flags = (rng.random(n) < 0.05).astype(np.uint8)
    per_kf = 1500
    n_kfs = (n + per_kf - 1) // per_kf + 1
    F = matcher.frame(m.FrameData(**w["fr"]))
    view = w["view"].native()
    with m.ResidentMap(matcher, n_kfs, 4 * n, 1, 2000) as rm, m.LocalPoints(matcher, n) as table:
        rm.write_points(slots, w["points"], flags)
        rows = []; shuffled = slots[rng.permutation(n)]
        for k in range(n_kfs - 1):
            own = shuffled[k * per_kf:(k + 1) * per_kf]
            extra = slots[rng.integers(0, n, 300)]                   # points other keyframes hold too
            row = np.concatenate([own, extra, np.full(100, -1, np.int32)])[rng.permutation(len(own) + 400)]
            rows.append(row); rm.write_keyframe(k, row)
        rows.append(slots[rng.permutation(n)][:1900]); rm.write_keyframe(n_kfs - 1, rows[-1])
        lst = rm.local_points(rng.permutation(n_kfs))
        row_of_slot = np.full(4 * n, -1, np.int64); row_of_slot[slots] = np.arange(n)
        in_list = row_of_slot[lst]
        assert 0.8 * n <= len(lst) <= int((flags == 0).sum()) and np.all(in_list >= 0) and not flags[in_list].any()
        assert not np.array_equal(np.sort(lst), lst)                # scattered: the list order is not the slot order
        table.write(0, w["points"][in_list])
        for use in (False, True):
            if use:                                                 # the frame's own points, `seen` and `occupied` in use
                fp = np.where(rng.random(nf) < 0.1, slots[rng.integers(0, n, nf)], -1).astype(np.int32)
                fp[:3] = [slots[np.nonzero(flags)[0][0]], lst[0], lst[0]]
                seen = np.concatenate([lst[rng.permutation(len(lst))[:len(lst) // 10]], [-1, 4 * n - 1]]).astype(np.int32)
                occ = (fp >= 0).astype(np.uint8)
                good = fp[fp >= 0]; good = good[flags[row_of_slot[good]] == 0]
                skip = (np.isin(lst, good) | np.isin(lst, seen)).astype(np.uint8)
                assert skip[0] == 1 and 0.1 * len(lst) < skip.sum() < 0.5 * len(lst)
            else:
                fp = np.zeros(0, np.int32); seen = np.zeros(0, np.int32); occ = None; skip = None
            e_ntm, e_nm, e_mo, e_track = matcher.SearchLocalPoints(F, table, view, skip, occ, n=len(lst))
            assert matcher.last_resolve()[0] == 0, matcher.last_resolve()
            ntm, nm, mo, track = rm.search(F, view, fp, seen, occ, n_list=len(lst))
            assert matcher.last_resolve()[0] == 0, matcher.last_resolve()
            print("map search: %d listed, skip %s -> in view %d, matches %d" % (len(lst), None if skip is None else int(skip.sum()), ntm, nm))
            assert (ntm, nm) == (e_ntm, e_nm) and ntm >= 50 and nm >= 20
            assert track.tobytes() == e_track.tobytes() and mo.tobytes() == e_mo.tobytes()
            if use:
                assert not track["in_view"][skip != 0].any() and not occ[mo >= 0].any()
        # a point that went bad after the list was made is skipped, as the reference's second loop does
        victim = int(np.nonzero(e_track["in_view"])[0][0])
        rm.write_points([lst[victim]], w["points"][in_list[victim:victim + 1]], [1])
        sk = np.zeros(len(lst), np.uint8); sk[victim] = 1
        exp = matcher.SearchLocalPoints(F, table, view, sk, None, n=len(lst))
        got = rm.search(F, view, n_list=len(lst))
        assert got[:2] == exp[:2] and got[2].tobytes() == exp[2].tobytes() and got[3].tobytes() == exp[3].tobytes()
    F.close()


def test_search_without_a_list_is_an_error(matcher):
    import multi_orb_slam_amd as m
    from multi_orb_slam_amd import _lib
    w = fw.make_world(500, [1000, 500], 640, 480, 1, 1.0)
    F = matcher.frame(m.FrameData(**w["fr"]))
    with m.ResidentMap(matcher, 2, 10, 1, 8) as rm:
        with pytest.raises(m.OrbError) as e:
            rm.search(F, w["view"].native())
        assert e.value.code == _lib.ORB_E_ARG
        rm.write_keyframe(0, [-1, -1])
        assert len(rm.local_points([0])) == 0
        ntm, nm, mo, _ = rm.search(F, w["view"].native(), n_list=0)   # an empty list: nothing to match, every feature free
        assert (ntm, nm) == (0, 0) and np.all(mo == -1)
    F.close()


def test_host_route_of_the_map_gives_the_same_results():
    """MORB_HOST_RESOLVE=1 (read in orbm_create, hence a fresh child process): votes and list from the host routines over the map's
    mirror, the search through the host restatement with the skip flags rebuilt from the mirror (tests/local_map_leg.py)."""
    import os
    import subprocess
    import sys
    leg = os.path.join(os.path.dirname(os.path.abspath(__file__)), "local_map_leg.py")
    out = subprocess.run([sys.executable, leg], env=dict(os.environ, MORB_HOST_RESOLVE="1"), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "local_map_leg ok" in out.stdout, out.stdout + out.stderr
