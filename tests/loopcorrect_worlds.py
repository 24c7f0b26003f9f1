"""Seeded worlds and hand-built cases for the loop correction (tests/loopcorrect_model.py, orbm_map_correct_sim3 / _rigid): a map of
keyframe rows and points under slots, the keyframes of a loop's neighbourhood with their two Sim3s, and the tables of the update after
global BA.  A world is built to an exact number of kept (Sim3) or changed (rigid) points; the check_* functions assert, from the
model's own output, that every class of point the reference's loops distinguish occurs in it."""
import functools

import numpy as np

import loopcorrect_model as model

KEPT = [0, 1, 63, 64, 65, 255, 256, 257, 70000]   # kept / changed points of the seeded worlds
MAX_ROW = 8192                                    # ORBM_MAP_MAX_FEATURES


def random_sim3(rng, n, scale_one):
    """n Sim3s: a rotation of any angle (the quaternion normalised in double, so a unit one only to rounding), a translation of a few
    units, scale 1 or within 20 % of it."""
    q = rng.normal(size=(n, 4)); q = q / np.sqrt((q * q).sum(1))[:, None]
    t = rng.uniform(-3, 3, (n, 3))
    s = np.ones((n, 1)) if scale_one else rng.uniform(0.8, 1.25, (n, 1))
    return np.concatenate([q, t, s], axis=1)


def sim3_world(seed, kept, scale_one=False, same=False):
    """A map in which orbm_map_correct_sim3 keeps exactly `kept` points.  -> dict.
    Points: `kept` good ones that the listed rows hold at least once; bad ones; ones in `already`; good ones that only unlisted
    keyframes hold (they must not move).  kfs names one keyframe twice (from three listed keyframes on)."""
    rng = np.random.default_rng(seed)
    n_extra = max(4, kept // 10)
    n_points = kept + 3 * n_extra + 5
    slots = rng.permutation(n_points).astype(np.int32)
    good, bad, done, other = np.split(slots[:kept + 3 * n_extra], [kept, kept + n_extra, kept + 2 * n_extra])
    flags = np.zeros(n_points, np.uint8); flags[bad] = 1
    n_listed = max(4, -(-kept * 2 // 5000))                      # rows stay below MAX_ROW with the duplicates and the filler
    n_kfs = n_listed + 3
    kf_slots = rng.permutation(n_kfs).astype(np.int32)
    listed, unlisted = kf_slots[:n_listed], kf_slots[n_listed:]
    rows = [[] for _ in range(n_kfs)]
    home = rng.integers(0, n_listed, kept)
    if kept >= 2:
        home[:2] = [0, 2]                                        # position 0 claims something; so does a later one
    for p, h in zip(good.tolist(), home.tolist()):
        rows[listed[h]].append(p)
    if kept >= 8:
        for p in good[home == 0][:max(1, kept // 20)].tolist():  # held by positions 0 and 2: goes to 0
            rows[listed[2]].append(p)
        for p, h in list(zip(good.tolist(), home.tolist()))[2:2 + max(2, kept // 20)]:
            rows[listed[h]].append(p)                            # twice in one row
        for p in good[rng.integers(0, kept, max(1, kept // 10))].tolist():
            rows[listed[rng.integers(0, n_listed)]].append(p)    # and held by any other listed keyframe
    for k in listed.tolist():                                    # every listed row: bad points, points already corrected, holes
        rows[k] += bad[rng.integers(0, n_extra, 1 + n_extra // n_listed)].tolist()
        rows[k] += done[rng.integers(0, n_extra, 1 + n_extra // n_listed)].tolist()
        rows[k] += [-1] * (2 + len(rows[k]) // 8)
    for k in unlisted.tolist():
        rows[k] = other[rng.integers(0, n_extra, 1 + n_extra // 2)].tolist() + [-1]
    rows[unlisted[0]] = []                                       # an empty keyframe
    stride = max(max(len(r) for r in rows), 1)
    assert stride <= MAX_ROW, stride
    kf_rows = np.full((n_kfs, stride), -1, np.int32); kf_count = np.zeros(n_kfs, np.int32)
    for k, r in enumerate(rows):
        r = np.array(r, np.int32)[rng.permutation(len(r))] if r else np.zeros(0, np.int32)
        kf_rows[k, :len(r)] = r; kf_count[k] = len(r)
    kfs = listed.copy()
    kfs = np.concatenate([kfs[:3], kfs[1:2], kfs[3:]]).astype(np.int32)   # listed[1] a second time, at position 3
    before = random_sim3(rng, len(kfs), True)                    # NonCorrectedSim3: Sim3(R, t, 1.0)
    after = before.copy() if same else random_sim3(rng, len(kfs), scale_one)
    pos = rng.uniform(-10, 10, (n_points, 3)).astype(np.float32)
    already = np.concatenate([done, [-1]]).astype(np.int32)[rng.permutation(len(done) + 1)]
    return dict(kf_rows=kf_rows, kf_count=kf_count, flags=flags, pos=pos, kfs=kfs, before=before, after=after, already=already,
                n_points=n_points, n_kfs=n_kfs, stride=stride, kept=kept, untouched=np.concatenate([bad, done, other, slots[kept + 3 * n_extra:]]))


def check_sim3_world(w):
    """Asserts the classes from the model's output.  -> the model's (entries, pos_out, Tiw, new positions).
    The classes (a world of fewer than 63 kept points cannot hold them all and is asked for those that do not need a kept point):
      a point claimed by position 0; one claimed by a later position whose row ALSO lies behind an earlier row with a bad point in it (a
      bad point is met, skipped, and the claim goes on); one held by positions 0 and 2 that goes to 0; one twice in a row, claimed once;
      a keyframe named twice, whose second turn claims nothing; bad points, holes and points in `already` among the candidates."""
    ent, out, Tiw, new = model.correct_sim3(w["kf_rows"], w["kf_count"], w["flags"], w["pos"], w["kfs"], w["before"], w["after"], w["already"])
    assert len(ent) == w["kept"], (len(ent), w["kept"])
    kfs, rows, cnt, flags = w["kfs"], w["kf_rows"], w["kf_count"], w["flags"]
    cand = [rows[k, :cnt[k]] for k in kfs.tolist()]
    allc = np.concatenate(cand)
    assert np.any(allc < 0) and np.any(flags[allc[allc >= 0]] != 0) and np.isin(allc, w["already"][w["already"] >= 0]).any()
    assert len(np.unique(kfs)) < len(kfs)
    assert not np.isin(ent[:, 0], w["untouched"]).any()
    assert np.array_equal(new[w["untouched"]], w["pos"][w["untouched"]])
    if w["kept"] >= 63:
        pos_of = dict(zip(ent[:, 0].tolist(), ent[:, 1].tolist()))
        assert 0 in pos_of.values() and any(j > 0 for j in pos_of.values())
        first_bad = min(j for j, r in enumerate(cand) if np.any(flags[r[r >= 0]] != 0))
        assert any(j > first_bad for j in pos_of.values())
        in0 = set(cand[0][cand[0] >= 0].tolist()) & set(cand[2][cand[2] >= 0].tolist()) & set(pos_of)
        assert in0 and all(pos_of[p] == 0 for p in in0)
        twice = [p for r in cand for p, c in zip(*np.unique(r[r >= 0], return_counts=True)) if c > 1 and p in pos_of]
        assert twice
        second = [j for j, k in enumerate(kfs.tolist()) if k in kfs[:j].tolist()]
        assert second and not np.isin(ent[:, 1], second).any()
        assert len(np.unique(ent[:, 0])) == len(ent)
        moved = np.any(new[ent[:, 0]].view(np.uint32) != w["pos"][ent[:, 0]].view(np.uint32), axis=1)
        assert moved.mean() > 0.9 or np.array_equal(w["before"], w["after"])
    return ent, out, Tiw, new


def random_pose_rows(rng, n):
    """n rigid transforms as rows 0-2 of a float 4 x 4."""
    T = np.zeros((n, 3, 4), np.float32)
    for i in range(n):
        q = rng.normal(size=4); q /= np.sqrt((q * q).sum())
        T[i, :, :3] = model.quat_to_matrix(q).astype(np.float32)
    T[:, :, 3] = rng.uniform(-5, 5, (n, 3)).astype(np.float32)
    return T.reshape(n, 12)


RIGID_CLASSES = ["gba", "gba_bad", "gba_ref", "ref_not_corrected", "ref_none", "ref_beyond", "moved", "bad"]


def rigid_world(seed, changed, n_kfs=40):
    """A map in which orbm_map_correct_rigid over all points changes exactly `changed` of them.  -> dict; cls[slot] indexes RIGID_CLASSES."""
    rng = np.random.default_rng(seed)
    n_still = max(10, changed // 5)
    labels = np.concatenate([rng.choice([0, 2, 6], changed, p=[0.2, 0.1, 0.7]), rng.choice([1, 3, 4, 5, 7], n_still)])
    if changed >= 3:
        labels[:3] = [0, 2, 6]
    labels[changed:changed + 5] = [1, 3, 4, 5, 7]
    n_points = len(labels)
    cls = labels[rng.permutation(n_points)]
    kf_corrected = (rng.random(n_kfs) < 0.7).astype(np.uint8); kf_corrected[:2] = [1, 0]
    yes, no = np.nonzero(kf_corrected)[0], np.nonzero(kf_corrected == 0)[0]
    flags = np.isin(cls, [1, 7]).astype(np.uint8)
    ref = rng.choice(yes, n_points).astype(np.int32)              # gba, gba_bad, gba_ref, moved, bad: a corrected reference
    ref[cls == 0] = rng.choice(no, int((cls == 0).sum()))         # gba alone: the reference is not corrected
    ref[cls == 3] = rng.choice(no, int((cls == 3).sum()))
    ref[cls == 4] = -1
    ref[cls == 5] = n_kfs + rng.integers(0, 3, int((cls == 5).sum()))
    listed = np.nonzero(np.isin(cls, [0, 1, 2]))[0].astype(np.int32)
    gba_slots = listed[rng.permutation(len(listed))]
    if len(gba_slots):
        live = listed[np.isin(cls[listed], [0, 2])]
        dup = live[:1] if len(live) else gba_slots[:1]
        gba_slots = np.concatenate([gba_slots, dup, [-1]]).astype(np.int32)   # one point twice: its last entry counts
    gba_pos = rng.uniform(-10, 10, (len(gba_slots), 3)).astype(np.float32)
    pos = rng.uniform(-10, 10, (n_points, 3)).astype(np.float32)
    return dict(pos=pos, flags=flags, ref=ref, cls=cls, kf_corrected=kf_corrected, Tb=random_pose_rows(rng, n_kfs),
                Ta=random_pose_rows(rng, n_kfs), gba_slots=gba_slots, gba_pos=gba_pos, n_points=n_points, n_kfs=n_kfs, changed=changed)


def check_rigid_world(w, slots=None):
    """Asserts the classes from the model's output over all points.  -> the model's (status, pos_out, new positions) for `slots`."""
    st, _, new = model.correct_rigid(w["pos"], w["flags"], w["ref"], None, w["kf_corrected"], w["Tb"], w["Ta"], w["gba_slots"], w["gba_pos"])
    assert int((st != 0).sum()) == w["changed"]
    listed = np.zeros(w["n_points"], bool); listed[w["gba_slots"][w["gba_slots"] >= 0]] = True
    bad = w["flags"] != 0
    ref = w["ref"]; known = (ref >= 0) & (ref < w["n_kfs"])
    corr = np.zeros(w["n_points"], bool); corr[known] = w["kf_corrected"][ref[known]] != 0
    assert np.any(listed & bad & (st == 0)), "in gba_slots and bad"
    assert np.any(~listed & ~bad & known & ~corr & (st == 0)), "reference not corrected"
    assert np.any(~listed & ~bad & (ref == -1) & (st == 0)), "no reference"
    assert np.any(~listed & ~bad & (ref >= w["n_kfs"]) & (st == 0)), "reference beyond the table"
    assert np.any(~listed & bad & corr & (st == 0)), "bad with a corrected reference"
    if w["changed"] >= 3:
        assert np.any(listed & ~bad & ~corr & (st == 1)), "in gba_slots"
        assert np.any(listed & ~bad & corr & (st == 1)), "in gba_slots with a corrected reference"
        assert np.any(~listed & ~bad & corr & (st == 2)), "moved through the reference"
        twice = w["gba_slots"][-2]
        last = np.nonzero(w["gba_slots"] == twice)[0][-1]
        assert np.array_equal(new[twice], w["gba_pos"][last]) and not np.array_equal(w["gba_pos"][last], w["gba_pos"][np.nonzero(w["gba_slots"] == twice)[0][0]])
    same = st == 0
    assert np.array_equal(new[same].view(np.uint32), w["pos"][same].view(np.uint32))
    return model.correct_rigid(w["pos"], w["flags"], w["ref"], slots, w["kf_corrected"], w["Tb"], w["Ta"], w["gba_slots"], w["gba_pos"])


@functools.lru_cache(maxsize=None)
def sim3_case(kept, variant="scaled"):
    """(world, the model's checked output), computed once per process and shared by the tests (nobody writes into either).
    variant: "scaled" (CorrectedSim3 with a scale != 1), "fixed" (scale 1, a stereo loop), "same" (before == after)."""
    w = sim3_world(100 + kept, kept, scale_one=variant == "fixed", same=variant == "same")
    return w, check_sim3_world(w)


@functools.lru_cache(maxsize=None)
def rigid_case(changed):
    w = rigid_world(200 + changed, changed)
    return w, check_rigid_world(w)


# ---- hand-built cases

def identity_sim3(n=1):
    S = np.zeros((n, 8)); S[:, 3] = 1.0; S[:, 7] = 1.0
    return S


def hand_sim3():
    """Two keyframes over six points, worked by hand: keyframe 1 is listed first.  Row 1 = [2, -1, 4, 2, 5], row 0 = [4, 0, 1, 3];
    point 1 is bad, point 3 is in `already`.  Kept in order: (2, 0), (4, 0), (5, 0), (0, 1).  before = identity; after[0] = a scale of 2
    (the inverse halves: exact), after[1] = a translation by (1, 2, 3) (the inverse subtracts it: exact on these values)."""
    kf_rows = np.array([[4, 0, 1, 3, -1], [2, -1, 4, 2, 5]], np.int32); kf_count = np.array([4, 5], np.int32)
    flags = np.array([0, 1, 0, 0, 0, 0], np.uint8)
    pos = np.array([[1, 2, 3], [4, 5, 6], [2, 4, 8], [7, 7, 7], [-2, 0, 6], [0.5, 0.25, -1]], np.float32)
    before = identity_sim3(2); after = identity_sim3(2)
    after[0, 7] = 2.0; after[1, 4:7] = [1, 2, 3]
    exp_entries = np.array([[2, 0], [4, 0], [5, 0], [0, 1]], np.int32)
    exp_pos = np.array([[1, 2, 4], [-1, 0, 3], [0.25, 0.125, -0.5], [0, 0, 0]], np.float32)
    exp_Tiw = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1)); exp_Tiw[1, :3, 3] = [1, 2, 3]   # (a scale alone leaves [R | t/s] = [I | 0])
    return dict(kf_rows=kf_rows, kf_count=kf_count, flags=flags, pos=pos, kfs=np.array([1, 0], np.int32), before=before, after=after,
                already=np.array([3], np.int32), exp_entries=exp_entries, exp_pos=exp_pos, exp_Tiw=exp_Tiw)


def hand_rigid():
    """Three keyframes (0 and 2 corrected), seven points.  Keyframe 0: before = a translation by (1, 0, 0), after = a translation by
    (0, 0, 2); keyframe 2: before = a quarter turn about z, after = the identity."""
    Tb = np.zeros((3, 3, 4), np.float32); Ta = np.zeros((3, 3, 4), np.float32)
    Tb[:, :, :3] = np.eye(3); Ta[:, :, :3] = np.eye(3)
    Tb[0, :, 3] = [1, 0, 0]; Ta[0, :, 3] = [0, 0, 2]
    Tb[2, :, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    pos = np.array([[1, 2, 3], [1, 2, 3], [1, 2, 3], [1, 2, 3], [1, 2, 3], [1, 2, 3], [1, 2, 3]], np.float32)
    flags = np.array([0, 0, 1, 0, 0, 0, 1], np.uint8)
    ref = np.array([0, 2, 0, 1, -1, 3, 0], np.int32)
    gba_slots = np.array([5, 6, 5], np.int32); gba_pos = np.array([[9, 9, 9], [8, 8, 8], [7, 7, 7]], np.float32)
    exp_status = np.array([2, 2, 0, 0, 0, 1, 0], np.uint8)
    exp_pos = np.array([[2, 2, 5], [-2, 1, 3], [1, 2, 3], [1, 2, 3], [1, 2, 3], [7, 7, 7], [1, 2, 3]], np.float32)
    return dict(pos=pos, flags=flags, ref=ref, kf_corrected=np.array([1, 0, 1], np.uint8), Tb=Tb.reshape(3, 12), Ta=Ta.reshape(3, 12),
                gba_slots=gba_slots, gba_pos=gba_pos, exp_status=exp_status, exp_pos=exp_pos)
