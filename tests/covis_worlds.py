"""Seeded worlds for the covisibility and culling counts (tests/covis_model.py, orbm_map_covisibility / orbm_map_culling_counts): a
map of keyframes, points and observation records as plain arrays, with the four facts the two routines read beyond the local map's
-- the feature index of a record, the level / far byte of a feature, the camera-1 feature count of a keyframe, n_obs of a point.
check_conditions asserts that a full-size world holds the cases the reference's loops distinguish."""
import numpy as np

import covis_model as cm

OBS_DTYPE = np.dtype([("point", "<i4"), ("keyframe", "<i4")])


def empty_world(n_kfs, n_points, stride, n_slab=0):
    obs = np.zeros(n_slab, OBS_DTYPE); obs["point"] = -1; obs["keyframe"] = -1
    return dict(n_kfs=n_kfs, n_points=n_points, stride=stride, flags=np.zeros(n_points, np.uint8), n_obs=np.zeros(n_points, np.int32),
                kf_rows=np.full((n_kfs, stride), -1, np.int32), kf_count=np.zeros(n_kfs, np.int32),
                kf_feat=np.zeros((n_kfs, stride), np.uint8), kf_ncam1=np.zeros(n_kfs, np.int32), obs=obs,
                obs_feat=np.zeros(n_slab, np.int32))


def make_world(seed, n_kfs, n_points, stride, n_rec, slack=1.25, min_count=None):
    """About n_rec live records over distinct (point, keyframe) pairs, every one at a feature of its own in its keyframe's row; then
    the deviations: records whose feature is not where the row holds the point, row entries without a record of their own, a point
    at two features of one row, bad points, free records between live ones."""
    rng = np.random.default_rng(seed)
    w = empty_world(n_kfs, n_points, stride)
    lo = max(1, stride // 2) if min_count is None else min_count
    w["kf_count"] = rng.integers(lo, stride + 1, n_kfs).astype(np.int32)
    w["flags"] = (rng.random(n_points) < 0.08).astype(np.uint8)
    w["kf_feat"] = (rng.integers(0, 8, (n_kfs, stride)) | np.where(rng.random((n_kfs, stride)) < 0.25, cm.FAR, 0)).astype(np.uint8)
    # N: mostly inside the row, sometimes all of it, none of it or more than it
    nc = (w["kf_count"] * rng.random(n_kfs)).astype(np.int32)
    pick = rng.random(n_kfs)
    nc[pick < 0.1] = 0; nc[(pick >= 0.1) & (pick < 0.2)] = w["kf_count"][(pick >= 0.1) & (pick < 0.2)]; nc[pick > 0.95] = stride
    w["kf_ncam1"] = nc
    pairs = np.unique(rng.integers(0, max(n_points * n_kfs, 1), n_rec)) if n_points and n_rec else np.zeros(0, np.int64)
    p_of, k_of = (pairs // n_kfs).astype(np.int32), (pairs % n_kfs).astype(np.int32)
    order = np.argsort(k_of, kind="stable"); p_of, k_of = p_of[order], k_of[order]
    start = np.searchsorted(k_of, np.arange(n_kfs))
    rank = np.arange(len(k_of)) - start[k_of]
    keep = rank < np.maximum(w["kf_count"][k_of] - 2, 1)           # two features of every row stay spare
    p_of, k_of, rank = p_of[keep], k_of[keep], rank[keep]
    shift = rng.integers(0, stride, n_kfs)
    feat = ((rank + shift[k_of]) % w["kf_count"][k_of]).astype(np.int32)
    w["kf_rows"][k_of, feat] = p_of
    n_live = len(p_of)
    # deviations
    obs_feat = feat.copy()
    moved = rng.random(n_live) < 0.05                              # the record names another feature (and level) than the row's
    obs_feat[moved] = rng.integers(0, stride, int(moved.sum()))
    if n_points:
        for k in rng.permutation(n_kfs)[:max(1, n_kfs // 3)].tolist():   # row entries in the spare features
            c = int(w["kf_count"][k]); spare = np.nonzero(w["kf_rows"][k, :c] < 0)[0]
            if len(spare) >= 2:
                held = w["kf_rows"][k, :c]; held = held[held >= 0]
                w["kf_rows"][k, spare[0]] = rng.integers(0, n_points)       # (most likely) a point without a record of its own here
                if len(held):
                    w["kf_rows"][k, spare[1]] = held[0]                     # one point at two features
    perm = rng.permutation(n_live)                                 # records in no particular order, free ones in between
    n_slab = max(int(n_live * slack) + 2, n_live)
    at = np.sort(rng.permutation(n_slab)[:n_live])
    w["obs"] = np.zeros(n_slab, OBS_DTYPE); w["obs"]["point"] = -1; w["obs"]["keyframe"] = -1
    w["obs_feat"] = rng.integers(0, stride, n_slab).astype(np.int32)        # a free record keeps whatever feature it had
    w["obs"]["point"][at] = p_of[perm]; w["obs"]["keyframe"][at] = k_of[perm]; w["obs_feat"][at] = obs_feat[perm]
    # n_obs: the reference's counter, in which a stereo feature counts 2 -- anything from the number of records to twice it
    n_rec_of = np.bincount(p_of, minlength=n_points).astype(np.int32) if n_points else np.zeros(0, np.int32)
    w["n_obs"] = (n_rec_of + (n_rec_of * rng.random(n_points)).astype(np.int32)).astype(np.int32)
    return w


def check_conditions(w, listed):
    """The cases a full-size world must hold among the listed keyframes (asserted before anything is compared)."""
    rows, cnt, flags, obs, of = w["kf_rows"], w["kf_count"], w["flags"], w["obs"], w["obs_feat"]
    live = np.nonzero(obs["point"] >= 0)[0]
    assert np.any(obs["point"][:live[-1]] < 0), "no free record between live ones"
    have = {}
    for r in live.tolist():
        have[(int(obs["point"][r]), int(obs["keyframe"][r]))] = int(of[r])
    twice = missing = moved = bad = 0
    for k in np.asarray(listed).tolist():
        held = rows[k, :cnt[k]]
        good = held[held >= 0]
        twice += len(np.unique(good)) < len(good)
        bad += int(np.any(flags[good] != 0))
        for i in np.nonzero(held >= 0)[0].tolist():
            f = have.get((int(held[i]), k))
            missing += f is None
            moved += f is not None and f != i and not (f < cnt[k] and held[f] == held[i])
    assert twice and missing and moved and bad, (twice, missing, moved, bad)
    counts = cm.culling_counts(w, listed)
    assert np.any(counts[:, 1] > 0) and np.any(counts[:, 1] < counts[:, 0])
    assert not np.array_equal(counts, cm.culling_counts(w, listed, mono=True)), "the far bit decides nothing"
    cov = cm.covisibility(w, listed)
    assert any(np.any((e["cam1"] > 0) & (e["cam1"] < e["all"])) for e in cov) and any(np.any(e["cam1"] == 0) for e in cov if len(e))


def to_resident(m, mt, w, kf_capacity=None, obs_capacity=None):
    """The world written into a new ResidentMap of the matcher mt, every fact through its own call."""
    rm = m.ResidentMap(mt, kf_capacity or max(w["n_kfs"], 1), w["n_points"], obs_capacity or max(len(w["obs"]), 1), w["stride"])
    if w["n_points"]:
        rm.write_points(np.arange(w["n_points"]), np.zeros(w["n_points"], m.POINT_DTYPE), w["flags"])
        rm.write_point_nobs(np.arange(w["n_points"]), w["n_obs"])
    for k in range(w["n_kfs"]):
        rm.write_keyframe(k, w["kf_rows"][k, :w["kf_count"][k]], bad=bool(w["kf_bad"][k]) if "kf_bad" in w else False)
        rm.write_keyframe_features(k, w["kf_feat"][k], w["kf_ncam1"][k])
    if len(w["obs"]):
        rm.write_observations(np.arange(len(w["obs"])), w["obs"])
        rm.write_observation_features(np.arange(len(w["obs"])), w["obs_feat"])
    return rm


def host(m, w, listed, mono=False):
    """The library's two host routines on the world's arrays -> (covisibility lists, culling counts)."""
    cov = m.local_map_covisibility_host(w["obs"], w["obs_feat"], w["flags"], w["kf_rows"], w["kf_count"], w["kf_ncam1"], listed)
    cull = m.local_map_culling_host(w["obs"], w["obs_feat"], w["flags"], w["n_obs"], w["kf_rows"], w["kf_count"], w["kf_feat"], listed, mono)
    return cov, cull


def same_lists(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


# ---- hand-built cases (the issue's list): each returns (world, listed keyframes, expected culling counts or None, expected lists or None)

def _put(w, k, i, p, level=0, far=False, record=True, rec_feature=None, slot=None):
    """Point p at feature i of keyframe k, with (by default) its record naming that feature."""
    w["kf_rows"][k, i] = p; w["kf_count"][k] = max(w["kf_count"][k], i + 1)
    w["kf_feat"][k, i] = level | (cm.FAR if far else 0)
    if record:
        _record(w, p, k, i if rec_feature is None else rec_feature, slot)


def _record(w, p, k, feature, slot=None):
    free = np.nonzero(w["obs"]["point"] < 0)[0]
    r = int(free[0]) if slot is None else slot
    w["obs"][r] = (p, k); w["obs_feat"][r] = feature


def hand_cases():
    """name -> (world, listed, culling counts expected (mono False), covisibility of listed[0] expected as (keyframe, all, cam1) tuples)."""
    cases = {}
    cases["no_records"] = (empty_world(3, 4, 8), [0, 1, 2], [(0, 0)] * 3, [])
    w = empty_world(1, 3, 8, 4)
    for i in range(3):
        _put(w, 0, i, i); w["n_obs"][i] = 9
    cases["one_keyframe"] = (w, [0], [(3, 0)], [])

    def observers(w, p, level_of, first_kf=1, feature=2, far=False):
        for j, lv in enumerate(level_of):
            _put(w, first_kf + j, feature, p, level=lv, far=far)

    # a point at two features of keyframe 0, seen by three others: counts twice everywhere
    w = empty_world(4, 2, 8, 16); _put(w, 0, 1, 0, level=2); _put(w, 0, 4, 0, level=2, record=False)
    observers(w, 0, [0, 1, 2]); w["n_obs"][0] = 4; w["kf_ncam1"][:] = 8
    cases["point_at_two_features"] = (w, [0], [(2, 2)], [(1, 2, 2), (2, 2, 2), (3, 2, 2)])
    # keyframe 0 holds the point, the point holds no record of keyframe 0
    w = empty_world(4, 2, 8, 16); _put(w, 0, 3, 0, level=1, record=False); observers(w, 0, [0, 1, 2]); w["n_obs"][0] = 6; w["kf_ncam1"][:] = 8
    cases["own_record_missing"] = (w, [0], [(1, 1)], [(1, 1, 1), (2, 1, 1), (3, 1, 1)])
    # keyframe 1's record names feature 5 (level 7), its row holds the point at feature 2 (level 0): the record's feature decides
    w = empty_world(4, 2, 8, 16); _put(w, 0, 3, 0, level=0); _put(w, 1, 2, 0, level=0, rec_feature=5); w["kf_feat"][1, 5] = 7
    observers(w, 0, [0, 0], first_kf=2); w["n_obs"][0] = 8; w["kf_ncam1"][:] = 4
    cases["record_at_another_feature"] = (w, [0], [(1, 0)], [(1, 1, 0), (2, 1, 1), (3, 1, 1)])
    # a bad point counts nowhere
    w = empty_world(4, 2, 8, 16); _put(w, 0, 3, 0); observers(w, 0, [0, 0, 0]); w["n_obs"][0] = 8; w["flags"][0] = cm.BAD
    _put(w, 0, 4, 1); w["n_obs"][1] = 1
    cases["bad_point"] = (w, [0], [(1, 0)], [])
    # a far feature is skipped unless mono (mono gives (2, 2))
    w = empty_world(4, 2, 8, 16); _put(w, 0, 3, 0, far=True); observers(w, 0, [0, 0, 0], far=True); w["n_obs"][0] = 8
    _put(w, 0, 0, 1); observers(w, 1, [0, 0, 0], feature=6); w["n_obs"][1] = 8
    cases["far_feature"] = (w, [0], [(1, 1)], [(1, 2, 0), (2, 2, 0), (3, 2, 0)])
    # n_obs exactly 3 (not examined) and 4 (examined)
    w = empty_world(4, 2, 8, 16); _put(w, 0, 0, 0); observers(w, 0, [0, 0, 0]); w["n_obs"][0] = 3
    _put(w, 0, 1, 1); observers(w, 1, [0, 0, 0], feature=6); w["n_obs"][1] = 4
    cases["n_obs_3_and_4"] = (w, [0], [(2, 1)], None)
    # exactly 2 and exactly 3 qualifying observations
    w = empty_world(4, 2, 8, 16); _put(w, 0, 0, 0); observers(w, 0, [0, 0]); w["n_obs"][0] = 9
    _put(w, 0, 1, 1); observers(w, 1, [0, 0, 0], feature=6); w["n_obs"][1] = 9
    cases["two_and_three_qualifying"] = (w, [0], [(2, 1)], None)
    # observers at level l+1 (counts) and l+2 (does not): point 0 has three at l+1, point 1 two at l+1 and one at l+2
    w = empty_world(4, 2, 8, 16); _put(w, 0, 0, 0, level=2); observers(w, 0, [3, 3, 3]); w["n_obs"][0] = 9
    _put(w, 0, 1, 1, level=2); observers(w, 1, [3, 3, 4], feature=6); w["n_obs"][1] = 9
    cases["level_l_plus_1_and_2"] = (w, [0], [(2, 1)], None)
    # level 7, l + 1 = 8: the compare runs on the five bits of the byte, beyond the levels a pyramid has -- 8 counts, 31 does not
    w = empty_world(4, 1, 8, 16); _put(w, 0, 0, 0, level=7); observers(w, 0, [8, 31, 0]); w["n_obs"][0] = 9
    cases["level_7"] = (w, [0], [(1, 0)], None)
    w = empty_world(4, 1, 8, 16); _put(w, 0, 0, 0, level=7); observers(w, 0, [8, 8, 0]); w["n_obs"][0] = 9
    cases["level_7_all_admitted"] = (w, [0], [(1, 1)], None)
    # camera-1 features at N-1 and N on either side: N = 4 everywhere
    w = empty_world(4, 4, 8, 16); w["kf_ncam1"][:] = 4
    _put(w, 0, 3, 0); _put(w, 1, 3, 0)                   # N-1 here, N-1 there: camera 1
    _put(w, 0, 4, 1); _put(w, 1, 2, 1)                   # N here: not camera 1
    _put(w, 0, 2, 2); _put(w, 1, 4, 2)                   # N there: not camera 1
    _put(w, 0, 1, 3); _put(w, 2, 0, 3)                   # another keyframe, camera 1
    cases["cam1_boundaries"] = (w, [0], None, [(1, 3, 1), (2, 1, 1)])
    # free records between live ones
    w = empty_world(4, 1, 8, 16); _put(w, 0, 0, 0, slot=9)
    for j, s in enumerate([1, 5, 15]):
        _put(w, 1 + j, 2, 0, slot=s)
    w["n_obs"][0] = 4; w["kf_ncam1"][:] = 1
    cases["free_records_between"] = (w, [0], [(1, 1)], [(1, 1, 0), (2, 1, 0), (3, 1, 0)])
    # a bad observer is an observer (no kernel reads the keyframe's flag)
    w = empty_world(4, 1, 8, 16); _put(w, 0, 0, 0); observers(w, 0, [0, 0, 0]); w["n_obs"][0] = 4
    w["kf_bad"] = np.array([0, 1, 0, 0], np.uint8)
    cases["bad_observer"] = (w, [0], [(1, 1)], [(1, 1, 0), (2, 1, 0), (3, 1, 0)])
    return cases


def entries_of(tuples):
    return np.array(tuples, cm.COVIS_DTYPE).reshape(-1) if tuples else np.zeros(0, cm.COVIS_DTYPE)


# (seed, keyframes, points, stride, records): the worlds the CPU tests compare on
CASES = [(1, 40, 600, 64, 3000), (2, 300, 5000, 100, 25000), (3, 7, 50, 300, 200), (4, 2, 20, 33, 30)]
