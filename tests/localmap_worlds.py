"""Seeded worlds for the local map (tests/localmap_model.py, orbm_map_*): a map of keyframes, points and observation records under
slots, and a frame.  Every world holds the cases the reference's loops distinguish; check_conditions asserts that it does before
anything is compared."""
import numpy as np

import localmap_model as lm

OBS_DTYPE = np.dtype([("point", "<i4"), ("keyframe", "<i4")])


def make_world(seed, n_kfs, n_points, stride, n_frame, mean_obs=5.0, slack=1.3, n_local=None):
    """n_kfs keyframes of up to `stride` features, n_points points at about mean_obs observations each, a frame of n_frame features.
    The record slab is `slack` times the live records, free records in between.  -> dict of arrays."""
    rng = np.random.default_rng(seed)
    flags = (rng.random(n_points) < 0.08).astype(np.uint8)
    kf_bad = (rng.random(n_kfs) < 0.1).astype(np.uint8)
    kf_rows = np.full((n_kfs, stride), -1, np.int32)
    kf_count = rng.integers(max(1, stride // 2), stride + 1, n_kfs).astype(np.int32)
    fill = np.zeros(n_kfs, np.int32)                              # features of a keyframe handed out so far
    order = [rng.permutation(int(c)) for c in kf_count]
    recs = []
    n_obs_of = np.minimum(rng.poisson(mean_obs, n_points), n_kfs)
    if n_points > 3:
        n_obs_of[rng.integers(0, n_points, max(1, n_points // 50))] = 0   # points nobody observes
    for p in range(n_points):
        for k in rng.choice(n_kfs, int(n_obs_of[p]), replace=False).tolist():
            if fill[k] >= max(kf_count[k] - 2, 1):
                continue                                          # the keyframe is full (two features stay spare): no observation
            kf_rows[k, order[k][fill[k]]] = p; fill[k] += 1
            recs.append((p, k))
    # a keyframe row that holds one point twice (no second record: one live record per (point, keyframe))
    for k in range(n_kfs):
        if 0 < fill[k] < kf_count[k] and rng.random() < 0.3:
            kf_rows[k, order[k][fill[k]]] = kf_rows[k, order[k][0]]; fill[k] += 1
    live = np.array(recs, np.int32).reshape(-1, 2)
    n_slab = max(int(len(live) * slack) + 2, len(live))
    obs = np.zeros(n_slab, OBS_DTYPE); obs["point"] = -1; obs["keyframe"] = -1
    at = np.sort(rng.permutation(n_slab)[:len(live)])
    obs["point"][at] = live[:, 0]; obs["keyframe"][at] = live[:, 1]
    # the frame: about 60 % of its features hold a point; one good point sits at two features, bad and unobserved points take part
    frame_points = np.where(rng.random(n_frame) < 0.6, rng.integers(0, max(n_points, 1), n_frame), -1).astype(np.int32)
    if n_points == 0:
        frame_points[:] = -1
    good = np.nonzero((flags == 0) & (n_obs_of > 0))[0]
    special = []
    if n_frame >= 4 and len(good) and n_points > 3:
        frame_points[0] = frame_points[n_frame - 1] = good[0]
        bad = np.nonzero(flags != 0)[0]
        if len(bad):
            frame_points[1] = bad[0]
        lonely = np.nonzero((n_obs_of == 0) & (flags == 0))[0]
        if len(lonely):
            frame_points[2] = lonely[0]
        special = [0, 1, 2, n_frame - 1]
    n_local = min(n_kfs, 12) if n_local is None else n_local
    local_kfs = rng.permutation(n_kfs)[:n_local].astype(np.int32)
    return dict(flags=flags, kf_bad=kf_bad, kf_rows=kf_rows, kf_count=kf_count, obs=obs, frame_points=frame_points,
                local_kfs=local_kfs, n_kfs=n_kfs, n_points=n_points, stride=stride, special=special)


def check_conditions(w):
    """The cases a full-size world must hold (asserted before anything is compared).  -> (votes, list) of the model."""
    fp, flags, obs = w["frame_points"], w["flags"], w["obs"]
    held = fp[fp >= 0]
    good_held = held[flags[held] == 0]
    assert len(np.unique(good_held)) < len(good_held), "no point at two features of the frame"
    assert np.any(flags[held] != 0), "no bad point in the frame"
    live = np.nonzero(obs["point"] >= 0)[0]
    assert np.any(obs["point"][:live[-1]] < 0), "no free record in the middle of the slab"
    observed = set(obs["point"][live].tolist())
    assert any(p not in observed for p in good_held.tolist()), "no frame point without observations"
    votes = lm.votes(obs, flags, fp, w["n_kfs"])
    assert np.any(votes[w["kf_bad"] != 0] > 0), "no votes for a bad keyframe"
    assert votes.sum() > 0
    rows = [w["kf_rows"][k, :w["kf_count"][k]] for k in w["local_kfs"].tolist()]
    assert any(len(np.unique(r[r >= 0])) < len(r[r >= 0]) for r in rows), "no keyframe row with the same point twice"
    allc = np.concatenate(rows); allc = allc[allc >= 0]
    per_kf = [set(r[r >= 0].tolist()) for r in rows]
    assert any(per_kf[i] & per_kf[j] for i in range(len(rows)) for j in range(i)), "no point in several local keyframes"
    assert np.any(flags[allc] != 0), "no bad point met on the way"
    lst = lm.local_points(w["kf_rows"], w["kf_count"], flags, w["local_kfs"])
    assert 0 < len(lst) < int((flags[allc] == 0).sum()), "no duplicate was dropped"
    assert len(np.unique(lst)) == len(lst) and not np.any(flags[lst] != 0)
    return votes, lst


def make_barren_world(seed):
    """A map whose local keyframes hold only bad points and empty features: the point list is empty, and nobody votes."""
    w = make_world(seed, 6, 40, 16, 12)
    w["flags"][:] = 1
    w["kf_rows"][::2] = -1
    return w


# (seed, keyframes, points, stride, frame features): the worlds the CPU tests compare on
CASES = [(1, 40, 600, 64, 200), (2, 300, 5000, 100, 2000), (3, 7, 50, 300, 30), (4, 1, 20, 33, 5)]
