"""Generated inputs of the map-point refresh (orbm_refresh_in) for tests/test_mappoint_model.py and tests/test_gpu_map_points.py,
and the conditions a world must meet before anything is compared on it."""
import numpy as np
import mappoint_model as mm

N_LEVELS = 8
CAP = 256                                     # ORBM_REFRESH_CAP
FORCED_COUNTS = (0, 1, 2, 3, 16, 17, 64, 65, CAP, CAP + 1)
SIZES = (500, 4000, 20000)


def scale_factors(n_levels=N_LEVELS, factor=1.2):
    """mvScaleFactors as ORBextractor builds them: a running float product."""
    s = np.ones(n_levels, np.float32)
    for k in range(1, n_levels):
        s[k] = s[k - 1] * np.float32(factor)
    return s


class Batch:
    """Plain holder of the orbm_refresh_in arrays (what multi_orb_slam_amd.RefreshBatch takes, in its argument order)."""

    def __init__(self, first, obs_desc, obs_centre, obs_alive, pos, ref_centre, ref_level, what, scale_factors):
        self.first = np.ascontiguousarray(first, np.int32); self.obs_desc = np.ascontiguousarray(obs_desc, np.uint8)
        self.obs_centre = np.ascontiguousarray(obs_centre, np.float32); self.obs_alive = np.ascontiguousarray(obs_alive, np.uint8)
        self.pos = np.ascontiguousarray(pos, np.float32); self.ref_centre = np.ascontiguousarray(ref_centre, np.float32)
        self.ref_level = np.ascontiguousarray(ref_level, np.int32); self.what = np.ascontiguousarray(what, np.uint8)
        self.scale_factors = np.ascontiguousarray(scale_factors, np.float32)
        self.n_points = len(self.first) - 1; self.n_obs = int(self.first[-1])

    def args(self):
        return (self.first, self.obs_desc, self.obs_centre, self.obs_alive, self.pos, self.ref_centre, self.ref_level, self.what,
                self.scale_factors)

    def native(self):
        import multi_orb_slam_amd as m
        return m.RefreshBatch(*self.args())

    def subset(self, rows):
        """The points `rows` (in that order) as a batch of their own."""
        rows = np.asarray(rows, np.int64)
        counts = (self.first[1:] - self.first[:-1])[rows]
        first = np.zeros(len(rows) + 1, np.int64); first[1:] = np.cumsum(counts)
        obs = np.concatenate([np.arange(self.first[p], self.first[p + 1]) for p in rows] + [np.zeros(0, np.int64)]).astype(np.int64)
        return Batch(first, self.obs_desc[obs], self.obs_centre[obs], self.obs_alive[obs], self.pos[rows], self.ref_centre[rows],
                     self.ref_level[rows], self.what[rows], self.scale_factors)

    def permuted(self, rng):
        """The same points with every observation list in another order (a permutation per point) + that permutation: observation j
        of the new list is observation perm[first[p] + j] - first[p] of the old one."""
        perm = np.arange(self.n_obs)
        for p in range(self.n_points):
            a, b = self.first[p], self.first[p + 1]
            perm[a:b] = a + rng.permutation(b - a)
        return Batch(self.first, self.obs_desc[perm], self.obs_centre[perm], self.obs_alive[perm], self.pos, self.ref_centre, self.ref_level,
                     self.what, self.scale_factors), perm


def make_world(n_points, seed):
    """n_points map points (at least 32): observation counts 1 + geometric(0.12) capped at 300; the descriptor of an observation is the
    point's base descriptor with 0-39 random bits flipped; the observing cameras stand at random range and bearing; about 10 % of the
    observations belong to bad keyframes; the job masks are mixed.  The first points carry the forced counts and the forced contents:
    rows 0-9 the counts of FORCED_COUNTS, row 10 all-identical descriptors, row 11 every observation dead, row 12 a camera centre
    equal to the position, rows 13 / 14 reference level 0 / n_levels - 1.  -> (Batch, dict of the forced rows)."""
    assert n_points >= 32
    rng = np.random.default_rng(seed)
    counts = np.minimum(rng.geometric(0.12, n_points), 300).astype(np.int64)      # support 1, 2, ...: 1 + the failures before a success
    counts[:len(FORCED_COUNTS)] = FORCED_COUNTS
    counts[10:15] = (7, 9, 5, 6, 6)
    first = np.zeros(n_points + 1, np.int64); first[1:] = np.cumsum(counts)
    n_obs = int(first[-1])
    owner = np.repeat(np.arange(n_points), counts)
    base = rng.integers(0, 256, (n_points, 32), dtype=np.uint8)
    bits = np.unpackbits(base[owner], axis=1)
    flips = rng.integers(0, 40, n_obs)
    mask = np.zeros((n_obs, 256), np.uint8)
    for a in range(0, n_obs, 16384):                                              # the first flips[i] of a random order of the 256 bits
        b = min(a + 16384, n_obs)
        order = np.argsort(rng.random((b - a, 256)), axis=1)
        np.put_along_axis(mask[a:b], order, (np.arange(256)[None, :] < flips[a:b, None]).astype(np.uint8), axis=1)
    obs_desc = np.packbits(bits ^ mask, axis=1)
    pos = rng.uniform(-20, 20, (n_points, 3)).astype(np.float32)
    bearing = rng.normal(size=(n_obs, 3)); bearing /= np.linalg.norm(bearing, axis=1)[:, None]
    rng_m = rng.uniform(0.3, 30.0, n_obs)[:, None]
    obs_centre = (pos[owner].astype(np.float64) + rng_m * bearing).astype(np.float32)
    obs_alive = (rng.random(n_obs) >= 0.10).astype(np.uint8)
    # reference keyframe: one of the point's own observers where it has any
    pick = first[:-1] + (rng.random(n_points) * np.maximum(counts, 1)).astype(np.int64)
    ref_centre = np.where((counts > 0)[:, None], obs_centre[np.minimum(pick, max(n_obs - 1, 0))], rng.uniform(-20, 20, (n_points, 3))).astype(np.float32)
    ref_level = rng.integers(0, N_LEVELS, n_points).astype(np.int32)
    what = rng.choice(np.array([0, 1, 2, 3], np.uint8), n_points, p=[0.05, 0.15, 0.15, 0.65]).astype(np.uint8)
    # forced contents
    what[:15] = 3
    forced = dict(counts=list(range(len(FORCED_COUNTS))), identical=10, all_dead=11, centre_at_pos=12, level_0=13, level_top=14)
    for p in range(len(FORCED_COUNTS)):                                            # the forced counts are counts of ALIVE observations too
        obs_alive[first[p]:first[p + 1]] = 1
    obs_desc[first[10]:first[11]] = base[10]; obs_alive[first[10]:first[11]] = 1
    obs_alive[first[11]:first[12]] = 0
    obs_centre[first[12] + 2] = pos[12]
    ref_level[13] = 0; ref_level[14] = N_LEVELS - 1
    return Batch(first, obs_desc, obs_centre, obs_alive, pos, ref_centre, ref_level, what, scale_factors()), forced


def check_conditions(batch, forced, rec, n_alive, tied):
    """Asserted on the MODEL's answer before anything is compared, so that a green comparison cannot be vacuous."""
    counts = batch.first[1:] - batch.first[:-1]
    assert [int(counts[p]) for p in forced["counts"]] == list(FORCED_COUNTS)
    # every size class and the fallback hold points with work
    busy = batch.what != 0
    assert (busy & (counts >= 1) & (counts <= 16)).sum() >= 1 and (busy & (counts > 16) & (counts <= 64)).sum() >= 1
    assert (busy & (counts > 64) & (counts <= CAP)).sum() >= 1 and (busy & (counts > CAP)).sum() >= 1
    assert set(np.unique(batch.what).tolist()) == {0, 1, 2, 3}
    dead = 1.0 - batch.obs_alive.mean()
    assert 0.05 < dead < 0.15, dead
    judged = ((batch.what & 1) != 0) & (n_alive >= 3)
    assert judged.sum() >= 0.5 * batch.n_points
    first_alive = np.array([batch.first[p] + int(np.argmax(batch.obs_alive[batch.first[p]:batch.first[p + 1]])) if n_alive[p] else -1
                            for p in range(batch.n_points)])
    not_first = rec["best_obs"][judged] != (first_alive[judged] - batch.first[:-1][judged])
    assert not_first.mean() >= 0.50, not_first.mean()          # the winner is not the first alive observation
    assert tied[judged].mean() >= 0.15, tied[judged].mean()    # the least median is attained more than once: the order decides
    # the forced contents are what they claim to be
    p = forced["identical"]; assert rec["best_obs"][p] == 0 and rec["best_median"][p] == 0
    p = forced["all_dead"]; assert rec["best_obs"][p] == -1 and not rec["desc"][p].any() and np.isfinite(rec["normal"][p]).all() and rec["max_dist"][p] > 0
    p = forced["centre_at_pos"]; assert not np.isfinite(rec["normal"][p]).any()
    p = forced["level_0"]; assert rec["max_dist"][p] > 0 and rec["min_dist"][p] < rec["max_dist"][p]
    p = forced["level_top"]; assert rec["max_dist"][p] > 0
    p = forced["counts"][0]; assert rec["best_obs"][p] == -1 and rec[p].tobytes()[:52] == bytes(52)
    return dict(not_first=float(not_first.mean()), tied=float(tied[judged].mean()), judged=int(judged.sum()))
