"""k_bow_transform and the device-built FeatureVector (k_fv_count, k_fv_offsets, k_fv_fill, k_side_misc) on the MI355X held to the boundary
worlds of tests/vocab_boundary_worlds.py.  Every world goes through Vocabulary.transform, transform_device on resident descriptors,
bow_vectors and BowSearch.keyframe_from_device + keyframe_download, and must equal the model byte for byte in each; every keyframe is
built twice on one workspace with a keyframe of another size between the two, with and without the triangulation arrays and d_uright, and
BowSearch.last_keyframe_build() must report the bins, chunks of 1024, nodes, largest node and items the model derives -- so no test
passes without running the chunk count it names.  The keyframes of the `fill` and `bins` worlds are then searched against each other
(search_by_bow_resident, modes 0 and 1) against oracle.search_by_bow on the model's FeatureVector, and last_join()'s largest node against
the model's: max_node arrives at the join.  The worlds' conditions and the wrong rules are asserted on the CPU in
tests/test_vocab_boundary_worlds.py."""
import functools
import numpy as np
import pytest
import multi_orb_slam_amd as m
from multi_orb_slam_amd import rt, synth
import vocab_boundary_worlds as vw
import oracle

pytestmark = pytest.mark.gpu

WORLDS = {w["name"]: w for w in vw.worlds()}
_VOCS = {}
_STATE = {}


def vocabulary(tree):
    hit = _VOCS.get(id(tree))
    if hit is None:
        hit = _VOCS[id(tree)] = m.Vocabulary(tree["parent"], tree["is_leaf"], tree["desc"], tree["weight"], tree["L"])
    return hit


def workspace():
    if "S" not in _STATE:
        _STATE["S"] = m.BowSearch()        # one workspace for every world of the process
    return _STATE["S"]


@functools.lru_cache(None)
def model_answer(name):
    w = WORLDS[name]
    return vw.model(w["tree"], w["feats"], w["levelsup"])


def angles(n, seed):
    return ((synth.hash32(np.arange(n, dtype=np.uint64) + np.uint64(seed * 7919)) % np.uint32(36000)).astype(np.float32) / np.float32(100.0))


def urights(n, seed):
    h = synth.hash32(np.arange(n, dtype=np.uint64) + np.uint64(seed * 104729))
    return np.where(h % np.uint32(3) == 0, np.float32(-1.0), (h % np.uint32(300)).astype(np.float32)).astype(np.float32)


class Resident:
    """The fields keyframe_from_device reads, filled from a world's own descriptors: device arrays of a two-camera frame."""

    def __init__(self, feats, seed, with_uright):
        n = len(feats)
        self.n_total, self.n_cams, self.counts, self.stream = n, 2, [n // 3, n - n // 3], None
        self.angle, self.uright = angles(n, seed), urights(n, seed) if with_uright else None
        self.x = angles(n, seed + 1); self.y = angles(n, seed + 2); self.octave = (np.arange(n) % 8).astype(np.int32)
        self.bufs = []
        self.d_desc = self._up(np.ascontiguousarray(feats, np.uint8)); self.d_angle = self._up(self.angle)
        self.d_uright = self._up(self.uright) if with_uright else None
        self.d_un_x, self.d_un_y, self.d_octave = self._up(self.x), self._up(self.y), self._up(self.octave)

    def _up(self, a):
        b = rt.DeviceBuffer(a.nbytes)
        if a.nbytes:
            b.upload(a)
        self.bufs.append(b)
        return b.ptr

    def flags(self):
        return np.ones(self.n_total, np.uint8) if self.uright is None else (1 | ((self.uright >= 0) << 1)).astype(np.uint8)

    def free(self):
        for b in self.bufs:
            b.free()


def expected_build(ans):
    return (ans["nbins"], (ans["nbins"] + vw.CHUNK - 1) // vw.CHUNK, len(ans["fv"][0]), ans["largest"], ans["items"])


def build_and_check(S, V, w, ans, tri, with_uright, seed):
    r = Resident(w["feats"], seed, with_uright)
    kf = S.keyframe_from_device(V, r, levelsup=w["levelsup"], triangulation=tri)
    assert S.last_keyframe_build() == expected_build(ans), (w["name"], S.last_keyframe_build(), expected_build(ans))
    word, node, fv = S.keyframe_download(kf)
    got = dict(word=word, node=node, fv=(fv.node_id, fv.node_start, fv.items))
    assert vw.differing(got, ans, ("word", "node", "fv")) == [], w["name"]
    side = dict(desc=w["feats"], angle=r.angle, flags=r.flags(), node_id=ans["fv"][0], node_start=ans["fv"][1], items=ans["fv"][2])
    r.free()
    return kf, side


def other_size(name):
    """a world of another size for the build in between: the neighbour in the list of worlds that the device accepts"""
    names = [n for n, w in WORLDS.items() if not w["promise"].get("refused")]
    k = names.index(name) if name in names else 0
    for step in range(1, len(names)):
        cand = names[(k + step) % len(names)]
        if len(WORLDS[cand]["feats"]) != len(WORLDS[name]["feats"]):
            return cand
    raise AssertionError(name)


def run_world(name):
    """every route of one world; -> [(keyframe, oracle side)] of its two builds (kept for the searches)"""
    if name in _STATE:
        return _STATE[name]
    w, ans = WORLDS[name], model_answer(name)
    V, S = vocabulary(w["tree"]), workspace()
    feats, n = w["feats"], len(w["feats"])
    # 1. transform
    word, node, weight = V.transform(feats, w["levelsup"])
    assert vw.differing(dict(word=word, node=node, weight=weight), ans, ("word", "node", "weight")) == [], name
    # 2. transform_device on resident descriptors
    d_f, d_w, d_n = rt.DeviceBuffer(feats.nbytes), rt.DeviceBuffer(4 * n), rt.DeviceBuffer(4 * n)
    if n:
        d_f.upload(feats)
    V.transform_device(d_f.ptr, n, w["levelsup"], d_w.ptr, d_n.ptr, V.stream)
    rt.stream_sync(V.stream)
    got = dict(word=d_w.download(np.uint32, n, V.stream), node=d_n.download(np.uint32, n, V.stream)) if n else dict(word=np.zeros(0, np.uint32), node=np.zeros(0, np.uint32))
    assert vw.differing(got, ans, ("word", "node")) == [], name
    for b in (d_f, d_w, d_n):
        b.free()
    # 3. bow_vectors
    bow, fv = V.bow_vectors(feats, w["levelsup"])
    assert vw.differing(dict(bow=bow, fv=(fv.node_id, fv.node_start, fv.items)), ans, ("bow", "fv")) == [], name
    # 4. keyframe_from_device + keyframe_download, twice, a keyframe of another size between
    oname = other_size(name)
    ow, oans = WORLDS[oname], model_answer(oname)
    built = []
    if w["promise"].get("refused"):
        r = Resident(feats, 3, True)
        with pytest.raises(m.OrbError) as e:
            S.keyframe_from_device(V, r, levelsup=w["levelsup"])
        assert e.value.code == -3 and S.last_keyframe_build() == (0, 0, 0, 0, 0) and ans["nbins"] == vw.MAX_BINS + 1
        r.free()
        k, _ = build_and_check(S, vocabulary(ow["tree"]), ow, oans, True, True, 5)     # the workspace builds the next keyframe correctly
        k.close()
    else:
        seed = 1 + sorted(WORLDS).index(name)
        built.append(build_and_check(S, V, w, ans, True, True, seed))
        k, _ = build_and_check(S, vocabulary(ow["tree"]), ow, oans, False, True, 5)
        k.close()
        built.append(build_and_check(S, V, w, ans, False, False, seed + 1000))
    _STATE[name] = built
    return built


def test_no_world_is_left_out():
    assert len(WORLDS) == vw.N_WORLDS == 106 and {w["group"] for w in WORLDS.values()} == set(vw.GROUPS)


@pytest.mark.parametrize("group", vw.GROUPS)
def test_every_route_equals_the_model_byte_for_byte(group):
    names = [n for n, w in WORLDS.items() if w["group"] == group]
    for name in names:
        run_world(name)
    assert len(names) == sum(w["group"] == group for w in WORLDS.values()) > 0
    if group == "bins":       # the forms: one to five chunks of 1024 bins ran, and the refusal
        chunks = {expected_build(model_answer(n))[1] for n in names if not WORLDS[n]["promise"].get("refused")}
        assert chunks == {1, 2, 3, 4, 5} and sum(bool(WORLDS[n]["promise"].get("refused")) for n in names) == 1
    if group == "fill":
        assert {expected_build(model_answer(n))[1] for n in names} == {5}
        assert max(expected_build(model_answer(n))[3] for n in names) == 300 and min(expected_build(model_answer(n))[3] for n in names) == 0


def search_and_check(S, A, B, name):
    (ka, sa), (kb, sb) = A, B
    total = 0
    for mode in (0, 1):
        nm, match = S.search_by_bow_resident(ka, kb, mode, None, None, 50, 0.8, True)
        onm, omatch = oracle.search_by_bow(sa, sb, mode, 50, 0.8, True)
        assert nm == onm and np.array_equal(match, omatch), (name, mode)
        if len(sa["node_id"]) and len(sb["node_id"]):      # (an empty side enqueues no join)
            largest = int(np.diff(sb["node_start"]).max())
            assert S.last_join()[1] == max(1, largest) and S.last_join()[3] == mode, (name, S.last_join(), largest)
            assert S.last_join()[0] == (4 if largest >= 128 else 1)
        total += nm
    return total


def test_keyframes_of_the_fill_and_bins_worlds_search_each_other_with_the_models_largest_node():
    S = workspace()
    names = [n for n, w in WORLDS.items() if w["group"] in ("fill", "bins") and not w["promise"].get("refused")]
    by_tree = {}
    for n in names:
        by_tree.setdefault(id(WORLDS[n]["tree"]), []).append(n)
    total, pairs, largest = 0, 0, set()
    for group in by_tree.values():
        for a, b in zip(group, group[1:] + group[:1]):
            A, B = run_world(a)[0], run_world(b)[1]       # (a == b for a tree with one world: its first build against its second)
            total += search_and_check(S, A, B, (a, b)); pairs += 1
            largest.add(model_answer(b)["largest"])
    assert pairs >= 30 and total > 300 and {0, 1, 130, 300} <= largest
