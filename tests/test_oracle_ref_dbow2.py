"""The BowVector / FeatureVector half of the oracle's BoW row against the REFERENCE's own compiled classes.

tests/golden/dbow2_ref_vectors.npz and dbow2_ref_live.npz were produced by oracle/_ref/libdbow2_ref.so (the reference's
BowVector.cpp and FeatureVector.cpp compiled where they lie, tests/golden/make_dbow2_golden.py): the tests need nothing but
the stored vectors.  Where that library has been built, the live cases also check that it still produces them."""
import os
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_dbow2_golden as gold  # noqa: E402  (case list + input construction; loads nothing of the reference by itself)

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dbow2_ref_vectors.npz"))
LIVE = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dbow2_ref_live.npz"))
REF_SO = os.path.join(gold.ROOT, "oracle", "_ref", "libdbow2_ref.so")


def _same(got, bid, bval, fn, fs, fi):
    (gid, gval), (gn, gs, gi) = got
    assert np.array_equal(gid, bid) and np.array_equal(gn, fn) and np.array_equal(gs, fs) and np.array_equal(gi, fi)
    assert gval.dtype == np.float64 and np.array_equal(gval, bval)  # bit-identical doubles: same accumulation and division order


@pytest.mark.parametrize("i", range(int(GOLD["n_cases"])))
def test_oracle_matches_reference_classes_golden(i):
    c = gold.CASES[i]
    assert all(int(GOLD["c%d_%s" % (i, k)]) == int(v) for k, v in c.items())
    voc, feats = gold.case_inputs(c)
    V = oracle.Vocabulary(voc)
    word, node, weight = V.transform(feats, c["levelsup"])
    assert np.array_equal(word, GOLD["c%d_word" % i]) and np.array_equal(node, GOLD["c%d_node" % i])
    assert np.array_equal(weight, GOLD["c%d_weight" % i])
    _same(V.bow_vectors(feats, c["levelsup"]), *[GOLD["c%d_%s" % (i, k)] for k in ("bow_id", "bow_val", "fv_node", "fv_start", "fv_items")])
    # the L1 norm the reference's normalize() produced
    assert abs(GOLD["c%d_bow_val" % i].sum() - 1.0) < 1e-12


@pytest.mark.parametrize("seed", gold.LIVE_SEEDS)
def test_oracle_matches_reference_classes_live(seed):
    L = gold.ref_lib() if os.path.exists(REF_SO) else None
    voc, feats = gold.live_inputs(seed)
    V = oracle.Vocabulary(voc)
    for levelsup in gold.LIVE_LEVELSUP:
        stored = {k: LIVE["s%d_l%d_%s" % (seed, levelsup, k)] for k in gold.LIVE_KEYS}
        word, node, weight = V.transform(feats, levelsup)
        assert np.array_equal(word, stored["word"]) and np.array_equal(node, stored["node"]) and np.array_equal(weight, stored["weight"])
        ref = [stored[k] for k in ("bow_id", "bow_val", "fv_node", "fv_start", "fv_items")]
        if L is not None:   # the reference classes themselves, where they have been built: the stored vectors are still theirs
            live = gold.ref_build(L, np.ascontiguousarray(word), np.ascontiguousarray(weight), np.ascontiguousarray(node))
            assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(live, ref))
        _same(V.bow_vectors(feats, levelsup), *ref)
