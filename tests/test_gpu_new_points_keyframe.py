"""CreateNewMapPoints for all neighbours of a keyframe in one enqueue (orbv_create_new_points_keyframe, include/orbv.h): the chained
call against the loop of fused calls with the flag update on the host (what a caller wrote before it existed), against the CPU
reference chain (tests/new_points_worlds.py), and at its edges: empty rounds in the middle, the workgroup edge of k_triangulate_round,
buffers that grow between calls, a feature contested between two features of the keyframe, and refused calls."""
import numpy as np
import pytest
import torch  # noqa: F401  (first: torch ships its own HIP runtime)
import multi_orb_slam_amd as m

import new_points_worlds as nw
import triangulate_model as tm
import triangulate_worlds as tw

pytestmark = pytest.mark.gpu
SF, S2, RATIO = nw.SF, nw.S2, nw.RATIO


@pytest.fixture(scope="module")
def search():
    S = m.BowSearch()
    yield S
    S.close()


def to_side(s, flags="own"):
    fv = m.FeatureVector(s["node_id"], s["node_start"], s["items"])
    return m.BowSide(s["desc"], s["angle"], fv, s["flags"] if isinstance(flags, str) else flags, s["x"], s["y"], s["octave"], s["cam_of"])


def resident(search, side, kf, geometry=True, flags="own"):
    K = search.keyframe(to_side(side, flags))
    if geometry:
        K.set_geometry(kf.uright, kf.depth, kf.cos_stereo, kf.xd, kf.yd)
    return K


class Device:
    """A world's keyframes resident on the device.  Odd rounds hand their neighbour's flags over per call (through the stage), even
    rounds leave them to the flags uploaded with the neighbour: the same bytes either way."""

    def __init__(self, search, world):
        self.search, self.world = search, world
        self.KA = resident(search, world.side_a, world.kf_a)
        self.KB = [resident(search, b.side, b.kf) for b in world.nb]
        self.a_native = world.kf_a.native()

    def flags_b(self, k):
        return self.world.nb[k].side["flags"] if k % 2 else None

    def round(self, k, KB=None, kf2=None):
        b = self.world.nb[k]
        return m.NewPointsRound(KB or self.KB[k], b.F12, b.ex, b.ey, SF, S2, self.a_native, kf2 or b.kf.native(), b.cam_enabled, RATIO, self.flags_b(k))

    def rounds(self):
        return [self.round(k) for k in range(self.world.K)]

    def chained(self, flags_a="own", rounds=None):
        fa = self.world.side_a["flags"] if isinstance(flags_a, str) else flags_a
        return self.search.create_new_points_keyframe(self.KA, self.rounds() if rounds is None else rounds, fa)

    def fused(self, k, fa):
        b = self.world.nb[k]
        match, rec, _ = self.search.create_new_points_resident(self.KA, self.KB[k], b.F12, b.ex, b.ey, SF, S2, self.a_native, b.kf.native(), b.cam_enabled,
                                                               RATIO, fa, self.flags_b(k))
        return match, rec

    def loop(self, flags_a=None):
        """The parent commit's path: one fused call and one synchronisation per neighbour, the flags updated in NumPy between them."""
        return nw.chain(self.world, self.fused, flags_a=flags_a)

    def close(self):
        for K in [self.KA] + self.KB:
            K.close()


def assert_equal(got, want, what=""):
    match, rec, nm, acc = got
    M, R = want[0], want[1]
    assert match.shape == M.shape and np.array_equal(match, M), (what, "match words", int((match != M).sum()))
    assert rec.tobytes() == R.tobytes(), (what, "records", [int((rec[k].tobytes() != R[k].tobytes())) for k in range(len(R))])
    assert nm.tolist() == (M >= 0).sum(1).tolist() and acc.tolist() == (R["outcome"] == tm.ACCEPTED).sum(1).tolist(), what


@pytest.mark.parametrize("n,k", [(600, 5), (300, 15)])
def test_chained_call_equals_the_loop_of_fused_calls(search, n, k):
    w, (M, R, _), _ = nw.world_and_chain(n, k)
    D = Device(search, w)
    want = D.loop()
    got = D.chained()
    assert_equal(got, want)
    assert search.last_keyframe_call() == (k, k, 1 + 4 * k, 1)          # no empty round: all enqueued; ONE synchronisation
    assert (got[2] > 0).all() and got[3].sum() > 100
    print("chained %d x %d: matches %s accepted %s" % (n, k, got[2].tolist(), got[3].tolist()))
    D.close()


def test_chained_call_equals_the_cpu_reference_chain(search):
    w, with_update, without = nw.world_and_chain(600, 5)
    print(nw.check_conditions(w, with_update, without))
    M, R, _ = with_update
    D = Device(search, w)
    match, rec, nm, acc = D.chained()
    assert np.array_equal(match, M)
    a_native = w.kf_a.native()
    for k, b in enumerate(w.nb):
        idx = np.flatnonzero(M[k] >= 0)
        want = np.zeros(w.n, m.TRI_OUT_DTYPE)
        want[idx] = m.triangulate_pairs_host(a_native, b.kf.native(), b.cam_enabled, np.stack([idx, M[k][idx]], 1), RATIO)
        assert rec[k].tobytes() == want.tobytes(), k
        assert want.tobytes() == R[k].tobytes(), k                        # and the model once more
    assert not (rec["outcome"] == tm.CAM_OFF).any()                       # a disabled camera never produces a pair
    D.close()


def test_one_round_equals_the_fused_call_and_no_rounds_do_nothing(search):
    w, _, _ = nw.world_and_chain(600, 5)
    D = Device(search, w)
    fa = w.side_a["flags"]
    match, rec, nm, acc = D.chained(rounds=[D.round(0)])
    m1, r1 = D.fused(0, nw.round_flags(w, fa & 1, 0))
    assert np.array_equal(match[0], m1) and rec[0].tobytes() == r1.tobytes() and nm[0] == (m1 >= 0).sum() > 20
    assert search.last_keyframe_call() == (1, 1, 5, 1)
    match, rec, nm, acc = D.chained(rounds=[])
    assert match.shape == (0, w.n) and rec.shape == (0, w.n) and len(nm) == 0 and len(acc) == 0
    assert search.last_keyframe_call() == (0, 0, 0, 0)
    D.close()


def test_keyframe_without_features(search):
    w, _, _ = nw.world_and_chain(600, 5)
    e = nw.make_world(0, 2)
    D = Device(search, w)
    KE = resident(search, e.side_a, e.kf_a)
    assert KE.n == 0
    rounds = [D.round(0), D.round(1)]
    match, rec, nm, acc = search.create_new_points_keyframe(KE, rounds, None)
    assert match.shape == (2, 0) and rec.shape == (2, 0) and nm.tolist() == [0, 0] and acc.tolist() == [0, 0]
    assert search.last_keyframe_call() == (2, 0, 0, 0)
    KE.close(); D.close()


def empty_side(kf_like, n):
    """A neighbour of n features without a FeatureVector node (n = 0: without features)."""
    kf = tw.KF(kf_like.Tcw[0, :, :3], kf_like.Tcw[0, :, 3], n)
    z = np.zeros(n)
    kf.set_features(z + 100, z + 100, z + 100, z + 100, z.astype(np.int32), z - 1, z - 1)
    side = dict(desc=np.zeros((n, 32), np.uint8), angle=np.zeros(n, np.float32), flags=np.ones(n, np.uint8), node_id=np.zeros(0, np.uint32),
                node_start=np.zeros(1, np.int32), items=np.zeros(0, np.uint32), x=kf.x, y=kf.y, octave=kf.octave, cam_of=kf.cam_of)
    return kf, side


def test_empty_rounds_in_the_middle_leave_the_rest_alone(search):
    """[n0, no features, n1 with both cameras off, n1, no FeatureVector nodes, n2] against [n0, n1, n2]."""
    w, _, _ = nw.world_and_chain(257, 4)
    D = Device(search, w)
    base = D.chained(rounds=[D.round(0), D.round(1), D.round(2)])
    assert_equal(base, nw.chain(nw.World(w.kf_a, w.side_a, w.nb[:3]), D.fused))
    kf0, s0 = empty_side(w.nb[0].kf, 0); kf1, s1 = empty_side(w.nb[0].kf, 40)
    K0, K1 = resident(search, s0, kf0), resident(search, s1, kf1)
    b = w.nb[1]
    dark = m.NewPointsRound(D.KB[1], b.F12, b.ex, b.ey, SF, S2, D.a_native, b.kf.native(), (0, 0), RATIO, D.flags_b(1))
    rounds = [D.round(0), D.round(3, K0, kf0.native()), dark, D.round(1), D.round(3, K1, kf1.native()), D.round(2)]
    match, rec, nm, acc = D.chained(rounds=rounds)
    assert search.last_keyframe_call() == (6, 4, 1 + 4 * 4, 1)           # the round with both cameras off is enqueued, the empty ones are not
    for k in (1, 2, 4):
        assert (match[k] == -1).all() and not rec[k].tobytes().strip(b"\0") and nm[k] == 0 and acc[k] == 0
    keep = [0, 3, 5]
    assert_equal((match[keep], rec[keep], nm[keep], acc[keep]), base)
    assert nm[5] > 0 and (nm[keep] > 0).all()
    K0.close(); K1.close(); D.close()


@pytest.mark.parametrize("n", [63, 64, 65, 257])
def test_workgroup_edge_of_the_round_kernel(search, n):
    w, _, _ = nw.world_and_chain(n, 2)
    D = Device(search, w)
    got = D.chained()
    assert_equal(got, D.loop())
    assert got[2].sum() > 0
    D.close()


def test_flags_of_the_keyframe_when_none_are_given(search):
    w, _, _ = nw.world_and_chain(257, 4)
    D = Device(search, w)
    assert_equal(D.chained(flags_a=None), D.loop())                       # the flags uploaded with the keyframe
    other = (w.side_a["flags"] ^ (np.arange(w.n) % 3 == 0)).astype(np.uint8)
    assert_equal(D.chained(flags_a=other), D.loop(other))                 # the flags of the moment
    bare = resident(search, w.side_a, w.kf_a, flags=None)                 # a keyframe uploaded without flags: every feature free, none stereo
    D.KA.close(); D.KA = bare
    ones = np.ones(w.n, np.uint8)
    got = D.chained(flags_a=None)
    assert_equal(got, D.loop(ones))
    assert_equal(got, D.chained(flags_a=ones))
    D.close()


def test_the_call_keeps_no_state_and_writes_no_keyframe(search):
    w, _, _ = nw.world_and_chain(600, 5)
    D = Device(search, w)
    b = w.nb[0]
    before = search.search_for_triangulation_resident(D.KA, D.KB[0], b.F12, b.ex, b.ey, SF, S2)
    first = D.chained(flags_a=None)
    second = D.chained(flags_a=None)
    for x, y in zip(first, second):
        assert x.tobytes() == y.tobytes()
    after = search.search_for_triangulation_resident(D.KA, D.KB[0], b.F12, b.ex, b.ey, SF, S2)
    assert before[0] == after[0] > 20 and np.array_equal(before[1], after[1])
    assert first[3][0] > 10                                               # features WERE taken out inside the call
    D.close()


def test_buffers_grow_and_are_reused_on_a_fresh_workspace():
    """A workspace of its own, so that every buffer of the call is reallocated inside the test: 64 x 2, then 600 x 5, then 64 x 2 again."""
    S = m.BowSearch()
    small, _, _ = nw.world_and_chain(64, 2)
    large, _, _ = nw.world_and_chain(600, 5)
    Ds, Dl = Device(S, small), Device(S, large)
    first = Ds.chained()                                                  # the very first call of the workspace
    assert_equal(first, Ds.loop(), "small")
    assert_equal(Dl.chained(), Dl.loop(), "large")
    again = Ds.chained()
    assert_equal(again, Ds.loop(), "small again")
    for x, y in zip(first, again):
        assert x.tobytes() == y.tobytes()
    Ds.close(); Dl.close(); S.close()


def test_a_feature_contested_between_two_features_of_the_keyframe(search):
    w, i0, i1, j = nw.contested_world()
    M, R, _ = nw.chain(w)
    M0, _, _ = nw.chain(w, update=False)
    # the condition, on the CPU chain: i0 is accepted in round 0; with the update i1 takes j in round 1, without it i0 does
    assert R[0]["outcome"][i0] == tm.ACCEPTED and M[0][i1] < 0
    assert M[1][i1] == j and M[1][i0] == -1 and M0[1][i0] == j
    D = Device(search, w)
    got = D.chained()
    assert_equal(got, (M, R))
    assert got[0][1][i1] == j and got[0][1][i0] == -1
    D.close()


def test_refused_calls_name_the_round_and_leave_the_workspace_usable(search):
    w, _, _ = nw.world_and_chain(64, 2)
    D = Device(search, w)
    want = D.loop()
    good = D.rounds()

    def refused(rounds, *words, code=-1):
        with pytest.raises(m.OrbError) as e:
            D.chained(rounds=rounds)
        assert e.value.code == code and all(t in str(e.value) for t in words), str(e.value)
        assert search.last_keyframe_call() == (0, 0, 0, 0)
        assert_equal(D.chained(), want)                                   # nothing has run: a following valid call is correct

    plain = resident(search, w.nb[1].side, w.nb[1].kf, geometry=False)
    refused([good[0], good[1], D.round(1, plain)], "round 2", "geometry")
    short = w.nb[1].kf.native(); short.n_levels = 3
    refused([good[0], D.round(1, None, short)], "round 1", "octave")
    refused([good[k % 2] for k in range(33)], "n_rounds = 33")
    n = 32769                                                             # one more than a vocabulary node may hold (JOIN_MAX_NODE)
    kf, side = empty_side(w.nb[0].kf, n)
    side.update(node_id=np.array([7], np.uint32), node_start=np.array([0, n], np.int32), items=np.arange(n, dtype=np.uint32))
    big = resident(search, side, kf)
    refused([good[0], good[1], good[0], D.round(0, big, kf.native())], "round 3", "limit", code=-3)
    plain.close(); big.close(); D.close()
