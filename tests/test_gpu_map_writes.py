"""What the resident map's shared slot-write path and its column table could get wrong (orbm_map_write_points, _observations,
_observation_features, _point_nobs, _positions, _point_ref; orbm_map_create): a slot named twice in one call at the put kernel's block
edges, the state of a fresh map, the high-water marks, and a refused write.  The test keeps every column as a plain array with
last-entry-wins; HBM is read through read_points and the device calls that consume the column (vote, local_points, covisibility,
culling_counts, correct_rigid) and compared with the library's host routines over those arrays.  Every comparison is equality of
integers or of raw bytes.  Run as a script under MORB_HOST_RESOLVE=1 (read in orbm_create, hence a child process) the same cases read
the MIRROR instead: there the consuming calls take their host route over it.  Prints 'map_writes_leg ok'."""
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu

KFS, POINTS, RECORDS, STRIDE = 4, 300, 300, 8    # the capacities of every map here
HOT = 10                                         # the point slots the keyframe rows name
HOST_ROUTE = os.environ.get("MORB_HOST_RESOLVE") == "1"

# writer -> the entry counts that put n x words just below, at and just above one block of 256 lanes (words: 17, 2, 1, 1, 1, 3)
EDGES = {"points": [1, 15, 16, 257], "observations": [127, 128, 129], "observation_features": [255, 256, 257],
         "point_nobs": [255, 256, 257], "point_ref": [255, 256, 257], "positions": [85, 86]}
TWICE = [(w, n) for w in EDGES for n in EDGES[w]]


@pytest.fixture(scope="module")
def matcher():
    import multi_orb_slam_amd as m
    mt = m.Matcher(0.8, True)
    yield mt
    mt.close()


def random_rows(rng, n):
    """Rows whose every field is random bytes, beside a finite position."""
    import multi_orb_slam_amd as m
    rows = np.frombuffer(rng.bytes(n * m.POINT_DTYPE.itemsize), m.POINT_DTYPE).copy()
    rows["pos"] = rng.normal(0, 4, (n, 3)).astype(np.float32)
    return rows


class Model:
    """The columns as plain arrays in the state orbm_map_create leaves, and the writers with last-entry-wins."""

    def __init__(self):
        import multi_orb_slam_amd as m
        self.rows = np.zeros(POINTS, m.POINT_DTYPE); self.flags = np.zeros(POINTS, np.uint8)
        self.obs = np.full(RECORDS, -1, np.int32).repeat(2).view(m.OBS_DTYPE).copy()
        self.obs_feat = np.zeros(RECORDS, np.int32); self.nobs = np.zeros(POINTS, np.int32); self.ref = np.full(POINTS, -1, np.int32)
        self.kf_rows = np.full((KFS, STRIDE), -1, np.int32); self.kf_count = np.zeros(KFS, np.int32)
        self.kf_ncam1 = np.zeros(KFS, np.int32); self.kf_feat = np.zeros((KFS, STRIDE), np.uint8)
        self.points = 0; self.keyframes = 0

    def write(self, writer, slots, values, flags=None):
        for i, s in enumerate(slots):
            if writer == "points":
                self.rows[s] = values[i]; self.flags[s] = 0 if flags is None else flags[i]
            elif writer == "observations":
                self.obs[s] = values[i] if values[i]["point"] >= 0 else (-1, -1)
                if values[i]["point"] >= 0:
                    self.keyframes = max(self.keyframes, int(values[i]["keyframe"]) + 1)
            elif writer == "positions":
                self.rows["pos"][s] = values[i]
            else:
                {"observation_features": self.obs_feat, "point_nobs": self.nobs, "point_ref": self.ref}[writer][s] = values[i]
            if writer in ("points", "positions", "point_ref"):   # n_obs is a count ABOUT a point and does not bring its slot into use
                self.points = max(self.points, int(s) + 1)

    def write_keyframe(self, k, row):
        self.kf_rows[k] = -1; self.kf_rows[k, :len(row)] = row; self.kf_count[k] = len(row)
        self.keyframes = max(self.keyframes, k + 1)

    def write_keyframe_features(self, k, fb, n_cam1):
        self.kf_feat[k] = 0; self.kf_feat[k, :len(fb)] = fb; self.kf_ncam1[k] = n_cam1


def send(rm, md, writer, slots, values, flags=None):
    """One call of a slot writer on the map, and the same entries into the model once the call has succeeded."""
    slots = np.asarray(slots, np.int32)
    if writer == "points":
        rm.write_points(slots, values, flags)
    else:
        getattr(rm, "write_" + writer)(slots, values)
    md.write(writer, slots, values, flags)


def random_values(rng, writer, n):
    """n valid entries of a writer: (values, flags or None)."""
    import multi_orb_slam_amd as m
    if writer == "points":
        return random_rows(rng, n), (rng.random(n) < 0.2).astype(np.uint8)
    if writer == "observations":
        rec = np.zeros(n, m.OBS_DTYPE)
        rec["point"] = np.where(rng.random(n) < 0.15, -1, rng.integers(0, 4 * HOT, n)); rec["keyframe"] = rng.integers(0, KFS, n)
        return rec, None
    if writer == "positions":
        return rng.normal(0, 4, (n, 3)).astype(np.float32), None
    hi = {"observation_features": STRIDE, "point_nobs": 7, "point_ref": KFS}[writer]
    lo = -1 if writer == "point_ref" else 0
    return rng.integers(lo, hi, n).astype(np.int32), None


def build_world(mt, seed=5):
    """A map whose every column is written and whose consuming calls all have something to count: four keyframes over the HOT point
    slots with one record per (row entry, keyframe), further records of other points, every point slot written."""
    import multi_orb_slam_amd as m
    rng = np.random.default_rng(seed)
    rm = m.ResidentMap(mt, KFS, POINTS, RECORDS, STRIDE); md = Model()
    rows, flags = random_values(rng, "points", POINTS)
    flags[:HOT] = 0; flags[HOT - 1] = 1
    send(rm, md, "points", np.arange(POINTS), rows, flags)
    rec, feat = [], []
    for k in range(KFS):
        row = rng.permutation(HOT)[:STRIDE - (k % 2)].astype(np.int32); row[k] = -1
        rm.write_keyframe(k, row); md.write_keyframe(k, row)
        fb = (rng.integers(0, 4, STRIDE) | np.where(rng.random(STRIDE) < 0.2, m.FEATURE_FAR, 0)).astype(np.uint8)
        n_cam1 = int(rng.integers(3, STRIDE + 1))
        rm.write_keyframe_features(k, fb, n_cam1); md.write_keyframe_features(k, fb, n_cam1)
        rec += [(p, k) for p in row if p >= 0]; feat += [i for i, p in enumerate(row) if p >= 0]
    extra, _ = random_values(rng, "observations", 60)
    rec = np.concatenate([np.array(rec, m.OBS_DTYPE), extra]); feat = np.concatenate([feat, rng.integers(0, STRIDE, 60)]).astype(np.int32)
    where = rng.permutation(120)[:len(rec)]
    send(rm, md, "observations", where, rec)
    send(rm, md, "observation_features", where, feat)
    nobs, _ = random_values(rng, "point_nobs", POINTS); nobs[:HOT] = rng.integers(3, 6, HOT)
    send(rm, md, "point_nobs", np.arange(POINTS), nobs)
    send(rm, md, "point_ref", np.arange(POINTS), random_values(rng, "point_ref", POINTS)[0])
    return rm, md, rng


def rigid_inputs(rng):
    """Every keyframe but one corrected, by proper rigid motions."""
    def motion():
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        q *= np.sign(np.linalg.det(q))
        return np.hstack([q, rng.normal(0, 2, (3, 1))]).astype(np.float32).reshape(12)
    kc = np.ones(KFS, np.uint8); kc[1] = 0
    return kc, np.stack([motion() for _ in range(KFS)]), np.stack([motion() for _ in range(KFS)])


def compare(mt, rm, md, rng, busy=True):
    """Both sides of the map against the model: HBM through read_points and, on the device route, through every consuming call; under
    MORB_HOST_RESOLVE=1 the same calls read the mirror.  busy: the world gives every call something to count."""
    import multi_orb_slam_amd as m
    route = 0 if HOST_ROUTE else 1
    assert rm.points == md.points and rm.keyframes == md.keyframes
    assert rm.read_points(np.arange(POINTS)).tobytes() == md.rows.tobytes()
    nk = md.keyframes
    fp = np.concatenate([np.arange(HOT), rng.integers(0, 4 * HOT, 40), [-1, -1]]).astype(np.int32)
    votes = rm.vote(fp)                                                                   # records, flags
    assert rm.last_local_map()[0] == route
    assert np.array_equal(votes, m.local_map_vote_host(md.obs, md.flags, fp, nk))
    order = rng.permutation(nk)
    lst = rm.local_points(order)                                                          # keyframe rows, flags
    assert rm.last_local_map()[0] == route
    assert np.array_equal(lst, m.local_map_points_host(md.kf_rows[:nk], md.kf_count[:nk], md.flags, order))
    cov = rm.covisibility(order)                                                          # records, their features, n_cam1
    assert rm.last_covisibility()[0] == route
    exp = m.local_map_covisibility_host(md.obs, md.obs_feat, md.flags, md.kf_rows[:nk], md.kf_count[:nk], md.kf_ncam1[:nk], order)
    assert len(cov) == len(exp) and all(a.tobytes() == b.tobytes() for a, b in zip(cov, exp))
    redundant = 0
    for mono in (False, True):                                                            # n_obs, feature bytes
        counts = rm.culling_counts(order, mono)
        assert rm.last_covisibility()[0] == route
        assert np.array_equal(counts, m.local_map_culling_host(md.obs, md.obs_feat, md.flags, md.nobs, md.kf_rows[:nk], md.kf_count[:nk],
                                                               md.kf_feat[:nk], order, mono))
        redundant += int(counts[:, 1].sum())
    kc, tb, ta = rigid_inputs(rng)
    st, pos = rm.correct_rigid(None, kc, tb, ta)                                          # references, positions
    assert rm.last_correction()[0] == route
    est, epos, new = m.local_map_correct_rigid_host(md.rows["pos"], md.flags, md.ref, np.arange(md.points), kc, tb, ta)
    assert np.array_equal(st, est) and pos.tobytes() == epos.tobytes()
    md.rows["pos"] = new
    assert rm.read_points(np.arange(POINTS)).tobytes() == md.rows.tobytes()
    if busy:
        assert votes.sum() > 0 and len(lst) > 0 and sum(len(c) for c in cov) > 0 and redundant > 0 and (st == 2).any()


def twice_entries(rng, writer, n):
    """n entries whose first and last name one slot with different values; the others name other slots, each once."""
    cap = RECORDS if writer.startswith("observation") else POINTS
    hot = 3                                             # a point of every keyframe row / a record of the world
    others = rng.permutation(np.delete(np.arange(cap), hot))[:max(n - 2, 0)]
    slots = np.concatenate([[hot], others, [hot]])[-n:] if n > 1 else np.array([hot])
    values, flags = random_values(rng, writer, n)
    if n > 1:
        if writer == "points":
            flags[0], flags[-1] = 1, 0
        elif writer == "observations":
            values[0] = (-1, 2); values[-1] = (hot, 1)
        elif writer == "positions":
            values[0] += 1.0
        else:
            values[0] = 0; values[-1] = 2
        assert slots[0] == slots[-1] and values[0].tobytes() != values[-1].tobytes()
    return slots.astype(np.int32), values, flags


def case_slot_named_twice(mt, writer, n):
    rm, md, rng = build_world(mt)
    with rm:
        slots, values, flags = twice_entries(rng, writer, n)
        send(rm, md, writer, slots, values, flags)
        compare(mt, rm, md, rng)


def case_fresh_map(mt):
    import multi_orb_slam_amd as m
    rng = np.random.default_rng(9)
    with m.ResidentMap(mt, KFS, POINTS, RECORDS, STRIDE) as rm:
        md = Model()
        assert rm.points == 0 and rm.keyframes == 0
        send(rm, md, "points", np.arange(HOT), random_rows(rng, HOT))
        row = np.arange(STRIDE, dtype=np.int32)
        rm.write_keyframe(0, row); md.write_keyframe(0, row)
        kc, tb, ta = rigid_inputs(rng); kc[:] = 1
        st, pos = rm.correct_rigid(None, kc, tb, ta)                       # every reference is -1: nothing moves
        assert len(st) == HOT and not st.any() and pos.tobytes() == md.rows["pos"][:HOT].tobytes()
        cov = rm.covisibility([0])                                         # no records
        assert len(cov) == 1 and len(cov[0]) == 0
        for mono in (False, True):                                         # n_obs 0, no feature is far
            assert rm.culling_counts([0], mono).tolist() == [[STRIDE, 0]]
        assert rm.vote(row).tolist() == [0]
        rows = rm.read_points(np.arange(POINTS))                           # an unwritten slot is a row of zeros
        assert rows.tobytes() == md.rows.tobytes() and not np.frombuffer(rows[HOT:].tobytes(), np.uint8).any()
        # one live record in the LAST slot brings every record slot below it into the calls' reach: all of them are free, the chains
        # of the points end at once, the record's feature is 0 and so is either keyframe's camera-1 count
        send(rm, md, "observations", [RECORDS - 1], np.array([(2, 1)], m.OBS_DTYPE))
        compare(mt, rm, md, rng, busy=False)
        assert rm.vote(row).tolist() == [0, 1]
        assert [c.tolist() for c in rm.covisibility([0, 1])] == [[(1, 1, 0)], []]


def case_high_water_marks(mt):
    import multi_orb_slam_amd as m
    k = 41
    for writer, value, after in (("point_nobs", np.array([5], np.int32), 0), ("point_ref", np.array([2], np.int32), k + 1),
                                 ("positions", np.ones((1, 3), np.float32), k + 1)):
        with m.ResidentMap(mt, KFS, POINTS, RECORDS, STRIDE) as rm:
            getattr(rm, "write_" + writer)([k], value)
            assert rm.points == after, writer
            rm.write_point_nobs([k + 7], [1])
            assert rm.points == after, writer
    with m.ResidentMap(mt, KFS, POINTS, RECORDS, STRIDE) as rm:
        rm.write_observations([7], np.array([(-1, 3)], m.OBS_DTYPE))         # a freed record's keyframe field counts for nothing
        assert rm.keyframes == 0 and rm.points == 0
        rm.write_observations([8, 9], np.array([(4, 2), (-5, 3)], m.OBS_DTYPE))
        assert rm.keyframes == 3 and rm.points == 0


def case_refused_write(mt, writer):
    import multi_orb_slam_amd as m
    rm, md, rng = build_world(mt)
    with rm:
        n = 257
        cap = RECORDS if writer.startswith("observation") else POINTS
        slots = np.concatenate([rng.permutation(cap)[:n - 1], [cap]]).astype(np.int32)
        values, flags = random_values(rng, writer, n)
        with pytest.raises(m.OrbError) as e:
            send(rm, Model(), writer, slots, values, flags)
        assert e.value.code == m._lib.ORB_E_CAPACITY
        compare(mt, rm, md, rng)


@pytest.mark.parametrize("writer,n", TWICE)
def test_a_slot_named_twice_takes_its_last_entry(matcher, writer, n):
    case_slot_named_twice(matcher, writer, n)


def test_a_fresh_map_holds_the_initial_state(matcher):
    case_fresh_map(matcher)


def test_high_water_marks(matcher):
    case_high_water_marks(matcher)


@pytest.mark.parametrize("writer", list(EDGES))
def test_a_refused_write_changes_neither_side(matcher, writer):
    case_refused_write(matcher, writer)


def test_the_mirror_holds_what_hbm_holds():
    """MORB_HOST_RESOLVE=1 (read in orbm_create, hence a fresh child process): every case above once more, the consuming calls now on
    their host route over the mirror."""
    import subprocess
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, MORB_HOST_RESOLVE="1"), capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0 and "map_writes_leg ok" in out.stdout, out.stdout + out.stderr


def main():
    import multi_orb_slam_amd as m
    assert HOST_ROUTE
    mt = m.Matcher(0.8, True)
    for writer, n in TWICE:
        case_slot_named_twice(mt, writer, n)
    case_fresh_map(mt)
    case_high_water_marks(mt)
    for writer in EDGES:
        case_refused_write(mt, writer)
    mt.close()
    print("map_writes_leg ok")


if __name__ == "__main__":
    main()
