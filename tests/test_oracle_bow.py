"""Known-answer tests of the oracle's vocabulary transform and BoW-gated searches (oracle/bow_oracle.cpp), plus a
second, independent restatement in plain Python loops for small random cases.  No GPU, no product code."""
import numpy as np
import oracle
from bow_model import popcount, py_bin, py_search_by_bow, py_three_maxima, py_triangulation  # noqa: F401
from helpers import make_bow_pair
from multi_orb_slam_amd import synth


def tiny_tree():
    """root -> A (all 0x00), B (all 0xFF); A -> A1 (0x00), A2 (low nibbles set); B -> B1 (0xFF) [leaf], B2 (0xF0)."""
    d = lambda v: np.full(32, v, np.uint8)
    parent = [0, 0, 0, 1, 1, 2, 2]
    leaf = [0, 0, 0, 1, 1, 1, 1]
    desc = np.stack([d(0), d(0x00), d(0xFF), d(0x00), d(0x0F), d(0xFF), d(0xF0)])
    weight = [0, 0, 0, 1.5, 2.25, 0.0, 4.0]   # word 2 (node 5) is stopped
    return dict(parent=np.array(parent, np.int32), is_leaf=np.array(leaf, np.uint8), desc=desc, weight=np.array(weight), k=2, L=2)


def test_transform_known_answers():
    V = oracle.Vocabulary(tiny_tree())
    f = np.stack([np.full(32, 0x01, np.uint8),     # near A, then A1 (word 0)
                  np.full(32, 0x0F, np.uint8),     # 128 from A and from B: first child (A) wins the tie; then A2 exactly (word 1)
                  np.full(32, 0xFE, np.uint8),     # B, then B1 (word 2, weight 0)
                  np.full(32, 0xF0, np.uint8)])    # tie again -> A; A1 at 128, A2 at 256 -> A1
    w, nd, wt = V.transform(f, levelsup=1)         # nid_level = 1: the children of the root
    assert w.tolist() == [0, 1, 2, 0] and nd.tolist() == [1, 1, 2, 1] and wt.tolist() == [1.5, 2.25, 0.0, 1.5]
    w, nd, _ = V.transform(f, levelsup=0)          # nid_level = 2: the leaves themselves
    assert nd.tolist() == [3, 4, 5, 3]
    w, nd, _ = V.transform(f, levelsup=2)          # nid_level = 0: root
    assert nd.tolist() == [0, 0, 0, 0]


def test_bow_vectors_known_answers():
    V = oracle.Vocabulary(tiny_tree())
    f = np.stack([np.full(32, 0x01, np.uint8), np.full(32, 0x0F, np.uint8), np.full(32, 0xFE, np.uint8), np.full(32, 0xF0, np.uint8),
                  np.full(32, 0x00, np.uint8)])
    (ids, vals), (nid, nstart, items) = V.bow_vectors(f, levelsup=1)
    # word 0 three times (features 0, 3, 4), word 1 once; the stopped word 2 appears nowhere
    assert ids.tolist() == [0, 1]
    s0 = (1.5 + 1.5) + 1.5
    norm = abs(s0) + abs(2.25)
    assert vals.tolist() == [s0 / norm, 2.25 / norm]
    assert nid.tolist() == [1] and nstart.tolist() == [0, 4] and items.tolist() == [0, 1, 3, 4]


def test_bow_weights_are_added_one_by_one():
    """BowVector::addWeight accumulates per feature: n * w and w + w + ... + w differ in the last bits for some w."""
    t = tiny_tree(); t["weight"][3] = 0.1
    V = oracle.Vocabulary(t)
    f = np.zeros((10, 32), np.uint8)
    (ids, vals), _ = V.bow_vectors(f, 1)
    acc = 0.1
    for _ in range(9):
        acc += 0.1
    assert acc != 10 * 0.1 and ids.tolist() == [0] and vals.tolist() == [acc / abs(acc)]


def test_l1_score():
    a = (np.array([1, 5, 9], np.uint32), np.array([0.5, 0.25, 0.25]))
    b = (np.array([2, 5, 9, 11], np.uint32), np.array([0.25, 0.25, 0.125, 0.375]))
    assert oracle.bow_score_l1(a, a) == 1.0
    assert oracle.bow_score_l1(a, (np.array([2, 3], np.uint32), np.array([0.5, 0.5]))) == 0.0
    s = (abs(0.25 - 0.25) - 0.25 - 0.25) + (abs(0.25 - 0.125) - 0.25 - 0.125)
    assert oracle.bow_score_l1(a, b) == -s / 2.0


# ---- second restatement: tests/bow_model.py (plain NumPy over dict-of-lists feature vectors) ---------------------------------
def test_search_by_bow_matches_python_restatement():
    voc = synth.vocabulary(6, 3, seed=5)
    V = oracle.Vocabulary(voc)
    for seed, (na, nb) in enumerate([(150, 170), (60, 200), (220, 90)]):
        a, b = make_bow_pair(voc, V, na, nb, seed=seed + 1, levelsup=2)
        for mode in (0, 1):
            for (th, ratio, ori) in ((50, 0.7, True), (50, 0.9, False), (30, 0.75, True), (256, 1.0, True)):
                nm, match = oracle.search_by_bow(a, b, mode, th, ratio, ori)
                pn, pm = py_search_by_bow(a, b, mode, th, ratio, ori)
                assert nm == pn and match.tolist() == pm, (seed, mode, th)
                assert nm == int((match >= 0).sum())


def test_search_by_bow_threshold_edges():
    """mode 0 accepts best == TH_LOW (<=, ORBmatcher.cc:324), mode 1 does not (<, :1107); claimed features are skipped."""
    d0 = np.zeros(32, np.uint8)
    near = d0.copy(); near[:6] = 0xFF; near[6] = 0x03        # 50 bits
    far = np.full(32, 0xFF, np.uint8)
    fv = dict(node_id=np.array([7], np.uint32), node_start=np.array([0, 2], np.int32), items=np.array([0, 1], np.uint32))
    a = dict(desc=np.stack([d0, d0]), angle=np.zeros(2, np.float32), flags=np.ones(2, np.uint8), **fv)
    b = dict(desc=np.stack([near, far]), angle=np.zeros(2, np.float32), flags=np.ones(2, np.uint8), **fv)
    assert popcount(d0, near) == 50
    nm, m = oracle.search_by_bow(a, b, 0, 50, 0.7, False)
    assert nm == 1 and m.tolist() == [0, -1]                 # query 0 takes b0; query 1 only sees b1 at 256: best = 256, nothing
    nm, m = oracle.search_by_bow(a, b, 1, 50, 0.7, False)
    assert nm == 0 and m.tolist() == [-1, -1]
    nm, m = oracle.search_by_bow(a, b, 1, 51, 0.7, False)
    assert nm == 1 and m.tolist() == [0, -1]


def test_triangulation_matches_python_restatement():
    voc = synth.vocabulary(5, 3, seed=8)
    V = oracle.Vocabulary(voc)
    sf = (1.2 ** np.arange(8)).astype(np.float32); s2 = (sf * sf).astype(np.float32)
    for seed in (1, 2, 3):
        a, b = make_bow_pair(voc, V, 160, 180, seed=seed, levelsup=2, stereo_p=0.3)
        # a fundamental matrix of a sideways translation (epipolar lines = rows) makes many pairs consistent; one per camera
        F12 = np.array([[0, 0, 0, 0, 0, -1, 0, 1, 0], [0, 0, 0.01, 0, 0, -1, -0.01, 1, 0]], np.float32)
        ex, ey = np.array([300.0, -50.0], np.float32), np.array([200.0, 240.0], np.float32)
        for ori in (True, False):
            nm, match = oracle.search_for_triangulation(a, b, F12, ex, ey, sf, s2, 50, ori)
            pn, pm = py_triangulation(a, b, F12, ex, ey, sf, s2, 50, ori)
            assert nm == pn and match.tolist() == pm
            assert nm > 10
