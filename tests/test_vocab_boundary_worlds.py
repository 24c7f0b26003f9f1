"""The boundary worlds of the vocabulary descent and the device-built FeatureVector (tests/vocab_boundary_worlds.py) on the CPU, before any
device sees them: every world meets the conditions its group promises, the oracle (oracle.Vocabulary.transform / .bow_vectors) equals the
model byte for byte on every one of them, both equal the vectors the reference's own compiled BowVector / FeatureVector classes made of
the `ids`, `stop`, `bins` and `fill` worlds (tests/golden/dbow2_ref_boundaries.npz, tests/golden/make_dbow2_golden.py), and every wrong
rule the model offers parts from the oracle on a world of the group named for it.  No GPU, no product code."""
import collections
import functools
import os
import sys
import numpy as np
import pytest
import vocab_boundary_worlds as vw
import oracle

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_dbow2_golden as gold  # noqa: E402

WORLDS = {w["name"]: w for w in vw.worlds()}
BOUNDARY = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dbow2_ref_boundaries.npz"))
REF_SO = os.path.join(gold.ROOT, "oracle", "_ref", "libdbow2_ref.so")
_ORACLES = {}


@functools.lru_cache(None)
def oracle_answer(name):
    w = WORLDS[name]
    O = _ORACLES.setdefault(id(w["tree"]), oracle.Vocabulary(w["tree"]))
    word, node, weight = O.transform(w["feats"], w["levelsup"])
    bow, fv = O.bow_vectors(w["feats"], w["levelsup"])
    return dict(word=word, node=node, weight=weight, bow=bow, fv=fv)


@functools.lru_cache(None)
def model_answer(name, rules=()):
    w = WORLDS[name]
    return vw.model(w["tree"], w["feats"], w["levelsup"], rules)


def test_no_world_is_left_out():
    assert len(WORLDS) == vw.N_WORLDS == 106
    count = collections.Counter(w["group"] for w in WORLDS.values())
    assert count == dict(tie=19, fanout=12, depth=31, ids=4, stop=5, bins=13, fill=22) and set(count) == set(vw.GROUPS)
    assert {w["promise"]["nbins"] for w in WORLDS.values() if w["group"] == "bins"} == {1, 2, 1024, 1025, 1026, 2048, 2049, 4096, 4097, 4098}
    assert {w["promise"]["k"] for w in WORLDS.values() if w["group"] == "fanout"} == {1, 2, 15, 16, 17, 20, 32, 33}
    assert {w["promise"]["n"] for w in WORLDS.values() if "n" in w["promise"]} == set(vw.FILL_COUNTS) | {5000}
    for L in range(1, 7):
        assert {w["levelsup"] for w in WORLDS.values() if w["promise"].get("L") == L} == {0, 1, L - 1, L, L + 2}


@pytest.mark.parametrize("group", vw.GROUPS)
def test_the_worlds_meet_their_conditions(group):
    assert sum(vw.check_conditions(w) for w in WORLDS.values() if w["group"] == group) > 0


@pytest.mark.parametrize("group", vw.GROUPS)
def test_oracle_equals_model_on_every_world(group):
    n = 0
    for name, w in WORLDS.items():
        if w["group"] == group:
            assert vw.differing(model_answer(name), oracle_answer(name)) == [], name
            n += 1
    assert n == sum(w["group"] == group for w in WORLDS.values()) > 0


@pytest.mark.parametrize("group", gold.BOUNDARY_GROUPS)
def test_oracle_and_model_equal_the_reference_classes_recorded_vectors(group):
    L = gold.ref_lib() if os.path.exists(REF_SO) else None
    n = 0
    for name, w in WORLDS.items():
        if w["group"] != group:
            continue
        stored = {k: BOUNDARY["%s_%s" % (name, k)] for k in gold.LIVE_KEYS}
        ref = dict(word=stored["word"], node=stored["node"], weight=stored["weight"], bow=(stored["bow_id"], stored["bow_val"]),
                   fv=(stored["fv_node"], stored["fv_start"], stored["fv_items"]))
        assert vw.differing(oracle_answer(name), ref) == [] and vw.differing(model_answer(name), ref) == [], name
        if L is not None:   # the reference classes themselves, where they have been built: the stored vectors are still theirs
            live = gold.ref_build(L, *[np.ascontiguousarray(stored[k]) for k in ("word", "weight", "node")])
            assert all(np.array_equal(a, stored[k]) and a.dtype == stored[k].dtype for a, k in zip(live, gold.LIVE_KEYS[3:])), name
        n += 1
    assert n > 0
    assert len(BOUNDARY.files) == len(gold.LIVE_KEYS) * sum(w["group"] in gold.BOUNDARY_GROUPS for w in WORLDS.values())


@pytest.mark.parametrize("rule", vw.RULES)
def test_every_wrong_rule_is_caught_by_its_own_group(rule):
    group = vw.RULE_GROUP[rule]
    caught = [name for name, w in WORLDS.items() if w["group"] == group and vw.differing(model_answer(name, (rule,)), oracle_answer(name))]
    assert caught, rule
    # and where: the descent's rules in the per-feature outputs, the FeatureVector's rules in the FeatureVector alone
    for name in caught:
        d = vw.differing(model_answer(name, (rule,)), oracle_answer(name))
        if rule in ("bins_by_position", "items_descending", "root_bin_dropped", "chunk_base_not_carried"):
            assert d == ["fv"], (rule, name, d)
        elif rule in ("last_child_wins", "second_pass_dropped"):
            assert "word" in d, (rule, name, d)
        elif rule == "nid_one_level_late":
            assert "node" in d and "word" not in d and "bow" not in d, (rule, name, d)
        elif rule == "stopped_kept":
            assert "word" not in d and ("bow" in d or "fv" in d), (rule, name, d)
    wanted = {"last_child_wins": 15, "second_pass_dropped": 4, "chunk_base_not_carried": 8, "items_descending": 10}
    assert len(caught) >= wanted.get(rule, 1), (rule, caught)


def test_rules_part_where_they_should_and_nowhere_else():
    # a tie decides nothing where there is none; the second pass matters only from 17 children on
    assert not vw.differing(model_answer("tie_zero_best", ("last_child_wins",)), oracle_answer("tie_zero_best"))
    for k in (1, 2, 15, 16):
        assert not vw.differing(model_answer("fanout_k%d" % k, ("second_pass_dropped",)), oracle_answer("fanout_k%d" % k))
    # one chunk of bins: the base is never carried anywhere
    for name in ("bins_2", "bins_1024_wide", "bins_1_level_zero"):
        assert not vw.differing(model_answer(name, ("chunk_base_not_carried",)), oracle_answer(name))
    for name in ("bins_1025_binary", "bins_1025_k32", "bins_1026_wide", "bins_2048_wide", "bins_2049_binary", "bins_4096_wide", "bins_4097_binary", "bins_4097_k64"):
        assert vw.differing(model_answer(name, ("chunk_base_not_carried",)), oracle_answer(name)) == ["fv"], name
    # the root's bin is there to drop only where a path has no node at the level
    assert vw.differing(model_answer("depth_ragged_up1", ("root_bin_dropped",)), oracle_answer("depth_ragged_up1")) == ["fv"]
    assert vw.differing(model_answer("fill_root_only", ("root_bin_dropped",)), oracle_answer("fill_root_only")) == ["fv"]
    assert not vw.differing(model_answer("depth_L3_up1", ("root_bin_dropped",)), oracle_answer("depth_L3_up1"))
