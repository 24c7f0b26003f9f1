"""Triangulation and gating of new map points on the device (include/orbv.h): orbv_triangulate_pairs against the NumPy model
(tests/triangulate_model.py) byte for byte, and the fused resident call against the existing resident search followed by the host routine."""
import numpy as np
import pytest
import torch  # noqa: F401  (first: torch ships its own HIP runtime)
import multi_orb_slam_amd as m
from helpers import make_bow_pair, rand_unit
from multi_orb_slam_amd import synth

import triangulate_model as tm
import triangulate_worlds as tw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def search():
    S = m.BowSearch()
    yield S
    S.close()


@pytest.mark.parametrize("name", list(tw.WORLDS))
def test_device_equals_the_model_on_the_generated_worlds(search, name):
    w, rec = tw.world_and_model(name)
    got = w.device(search)
    for k in rec.dtype.names:
        assert got[k].tobytes() == rec[k].tobytes(), (k, int((got[k] != rec[k]).sum()))
    assert got.tobytes() == rec.tobytes()


def test_the_worlds_meet_their_condition():
    print(tw.check_conditions([tw.world_and_model(name)[1] for name in tw.WORLDS]))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 3000])
def test_batch_sizes(search, n):
    w, rec = tw.world_and_model("5cm")
    sel = np.random.default_rng(n).permutation(len(w.pairs))[:n]
    got = w.device(search, w.pairs[sel])
    assert len(got) == n and got.tobytes() == rec[sel].tobytes()


def test_hand_built_pairs_and_one_camera_off(search):
    for name, (w, outcome, path) in tw.hand_built().items():
        got = w.device(search)
        assert (got["outcome"][0], got["path"][0]) == (outcome, path), name
        assert got.tobytes() == w.model().tobytes(), name
    for w in (tw.exact_world(), tw.exact_world(False, True), tw.exact_world(False, False), tw.exact_world(False, False, 0.25)):
        assert w.device(search).tobytes() == w.model().tobytes()
    w, rec = tw.world_and_model("25cm")
    cam = w.kf1.cam_of[w.pairs[:, 0]]
    for enabled in ((1, 0), (0, 1), (0, 0)):
        off = tw.World(w.kf1, w.kf2, w.pairs, cam_enabled=enabled)
        got = off.device(search)
        dropped = np.array([not enabled[c] for c in cam])
        assert (got["outcome"][dropped] == tm.CAM_OFF).all() and not got["x3D"][dropped].any()
        assert got[~dropped].tobytes() == rec[~dropped].tobytes()
        assert got[:300].tobytes() == off.model(w.pairs[:300]).tobytes()


def test_argument_errors_of_the_device_call(search):
    w, _ = tw.world_and_model("5cm")
    bad = w.pairs[:10].copy(); bad[4, 1] = w.kf2.n
    with pytest.raises(m.OrbError) as e:
        w.device(search, bad)
    assert e.value.code == -1 and "pair 4" in str(e.value)
    oc = w.kf1.octave.copy(); oc[w.pairs[2, 0]] = tw.N_LEVELS
    with pytest.raises(m.OrbError) as e:
        search.triangulate_pairs(w.kf1.native(octave=oc), w.kf2.native(), w.cam_enabled, w.pairs[:10], w.ratio_factor)
    assert "octave" in str(e.value)


class ProductVocabulary:
    """make_bow_pair's vocabulary argument through the product's own transform."""

    def __init__(self, voc):
        self.v = m.Vocabulary(voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"], voc["L"])

    def bow_vectors(self, desc, levelsup):
        bow, fv = self.v.bow_vectors(desc, levelsup)
        return bow, (fv.node_id, fv.node_start, fv.items)


def synthetic_keyframes(na=2000, nb=2100):
    """Two keyframes of about 2 000 features as tests/test_gpu_bow.py builds them, with the geometry of a 25 cm world around them."""
    voc = synth.vocabulary(10, 3, seed=6)
    V = ProductVocabulary(voc)
    a, b = make_bow_pair(voc, V, na, nb, seed=17, levelsup=2, stereo_p=0.6)
    V.v.close()
    base, _ = tw.world_and_model("25cm")
    kfs = []
    for s, pose, seed in ((a, base.kf1, 300), (b, base.kf2, 400)):
        n = len(s["x"])
        kf = tw.KF(pose.Tcw[0, :, :3], pose.Tcw[0, :, 3], n // 2)
        stereo = (s["flags"] & 2) != 0
        depth = np.where(stereo, 0.5 + rand_unit(n, seed) * 12.0, -1.0).astype(np.float32)
        uright = np.where(stereo, np.maximum(s["x"] - np.float32(tw.MBF) / np.where(stereo, depth, 1.0), 0.0), -1.0).astype(np.float32)
        kf.set_features(s["x"], s["y"], s["x"] + np.float32(0.25), s["y"] - np.float32(0.125), s["octave"], uright, depth, cam_of=s["cam_of"])
        kfs.append(kf)
    return a, b, kfs[0], kfs[1]


def to_side(s):
    fv = m.FeatureVector(s["node_id"], s["node_start"], s["items"])
    return m.BowSide(s["desc"], s["angle"], fv, s["flags"], s["x"], s["y"], s["octave"], s["cam_of"])


SF = tw.scale_factors(); S2 = (SF * SF).astype(np.float32)
F12 = np.array([[0, 0, 0, 0, 0, -1, 0, 1, 0], [1e-5, 0, 0.004, 0, 2e-5, -1, -0.004, 1, 0.3]], np.float32)
EX, EY = np.array([300.0, -50.0], np.float32), np.array([200.0, 240.0], np.float32)


def test_fused_call_equals_search_then_host_routine(search):
    a, b, kf1, kf2 = synthetic_keyframes()
    KA, KB = search.keyframe(to_side(a)), search.keyframe(to_side(b))
    ratio = np.float32(1.5) * SF[1]
    # the searches of a keyframe before it has geometry ...
    before = [search.search_for_triangulation_resident(KA, KB, F12, EX, EY, SF, S2),
              search.search_by_bow_resident(KA, KB, 0), search.search_by_bow_resident(KA, KB, 1)]
    with pytest.raises(m.OrbError) as e:
        search.create_new_points_resident(KA, KB, F12, EX, EY, SF, S2, kf1.native(), kf2.native(), (1, 1), ratio)
    assert "geometry" in str(e.value)
    for K, kf in ((KA, kf1), (KB, kf2)):
        K.set_geometry(kf.uright, kf.depth, kf.cos_stereo, kf.xd, kf.yd)
    # ... return what they returned, after it
    after = [search.search_for_triangulation_resident(KA, KB, F12, EX, EY, SF, S2),
             search.search_by_bow_resident(KA, KB, 0), search.search_by_bow_resident(KA, KB, 1)]
    for (n0, m0), (n1, m1) in zip(before, after):
        assert n0 == n1 and np.array_equal(m0, m1)
    total = 0
    for it, enabled in enumerate(((1, 1), (1, 0), (1, 1))):
        fa = fb = None
        if it == 2:                                    # the flags of the moment
            fa = ((rand_unit(len(a["x"]), 51) < 0.7).astype(np.uint8) | (a["flags"] & 2)).astype(np.uint8)
            fb = ((rand_unit(len(b["x"]), 61) < 0.7).astype(np.uint8) | (b["flags"] & 2)).astype(np.uint8)
        nm, want_match = search.search_for_triangulation_resident(KA, KB, F12, EX, EY, SF, S2, fa, fb)
        match, rec, accepted = search.create_new_points_resident(KA, KB, F12, EX, EY, SF, S2, kf1.native(), kf2.native(), enabled, ratio, fa, fb)
        assert np.array_equal(match, want_match) and nm == int((match >= 0).sum()) and nm > 20
        idx = np.flatnonzero(match >= 0)
        pairs = np.stack([idx, match[idx]], 1)
        want = np.zeros(len(match), m.TRI_OUT_DTYPE)
        want[idx] = m.triangulate_pairs_host(kf1.native(), kf2.native(), np.array(enabled, np.uint8), pairs, ratio)
        assert rec.tobytes() == want.tobytes()
        assert not rec[match < 0].tobytes().strip(b"\0")
        assert accepted == int((want["outcome"] == tm.ACCEPTED).sum())
        assert want[idx].tobytes() == tm.triangulate(kf1, kf2, enabled, pairs, ratio).tobytes()     # and the model once more
        total += len(idx)
        print("fused call %d: %d pairs, outcomes %s" % (it, len(idx), np.bincount(want["outcome"][idx], minlength=11).tolist()))
    assert total > 100
    # a table shorter than the keyframe's octaves is refused by name
    short = kf2.native(); short.n_levels = 3
    with pytest.raises(m.OrbError) as e:
        search.create_new_points_resident(KA, KB, F12, EX, EY, SF, S2, kf1.native(), short, (1, 1), ratio)
    assert "octave" in str(e.value)
    KA.close(); KB.close()


def test_set_geometry_refuses_a_stereo_feature_without_depth(search):
    a, b, kf1, _ = synthetic_keyframes(300, 320)
    KA = search.keyframe(to_side(a))
    depth = kf1.depth.copy()
    i = int(np.flatnonzero(kf1.uright >= 0)[3]); depth[i] = 0.0
    with pytest.raises(m.OrbError) as e:
        KA.set_geometry(kf1.uright, depth, kf1.cos_stereo, kf1.xd, kf1.yd)
    assert "feature %d" % i in str(e.value)
    KA.close()


def test_the_staged_block_grows_and_is_reused_on_a_fresh_workspace():
    """A workspace of its own, so that the staged block is reallocated inside the test: the one pair of a hand-built world (keyframes of
    one feature), then 2000 pairs of a generated world (keyframes of thousands), then the one pair again.  Every call byte for byte the
    host routine, the two small calls each other."""
    small = tw.exact_world(False, False, 0.25)
    large, _ = tw.world_and_model("25cm")
    pairs = large.pairs[:2000]
    S = m.BowSearch()
    try:
        first = small.device(S)
        assert len(first) == 1 and first.tobytes() == small.host().tobytes()
        got = large.device(S, pairs)
        assert len(got) == 2000 and got.tobytes() == large.host(pairs).tobytes()
        again = small.device(S)
        assert again.tobytes() == small.host().tobytes() == first.tobytes()
    finally:
        S.close()
