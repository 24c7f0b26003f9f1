"""The boundary worlds of the keyframe database's query (tests/kfdb_boundary_worlds.py) on the CPU, before any device sees them: every
world meets the conditions its group promises, the model's score equals the oracle's L1 score and the library's host routine bit for bit
on every (query, entry) pair of every world, the model's list order equals the inverted file's (tests/kfdb_model.py), and every wrong
rule the model offers parts from the right one on a world of the group named for it -- and from the oracle.  No GPU."""
import functools
import numpy as np
import pytest
import multi_orb_slam_amd as m
import kfdb_boundary_worlds as kw
import oracle

WORLDS = {w["name"]: w for w in kw.worlds()}


@functools.lru_cache(None)
def transcript(name, rules=()):
    return kw.play(WORLDS[name], kw.ModelDB(WORLDS[name]["n_words"], rules))


def bits(x):
    return np.float64(x).tobytes()


def test_no_world_is_left_out():
    assert len(WORLDS) == kw.N_WORLDS == 6 and {w["group"] for w in WORLDS.values()} == set(kw.GROUPS)
    assert set(kw.RULE_GROUP) == set(kw.RULES) and set(kw.RULE_GROUP.values()) <= set(kw.GROUPS)


@pytest.mark.parametrize("name", list(WORLDS))
def test_the_world_meets_its_conditions(name):
    assert kw.check_conditions(WORLDS[name]) > 0


def pairs_of(w):
    """every distinct (query, entries alive at the query) of a world"""
    alive, seen = [], set()
    for op in w["ops"]:
        if op[0] == "add":
            alive.append((op[1], op[2]))
        elif op[0] == "erase":
            alive = [(k, b) for k, b in alive if k != op[1]]
        elif op[0] == "query":
            for q in kw._distinct(op[1]):
                sig = (id(q[0]), tuple(k for k, _ in alive))
                if sig not in seen:
                    seen.add(sig)
                    yield q, list(alive)


@pytest.mark.parametrize("name", list(WORLDS))
def test_model_equals_oracle_library_and_inverted_file(name):
    w = WORLDS[name]
    n = 0
    for q, alive in pairs_of(w):
        rows = []
        for key, e in alive:
            c, first, s = kw.pair(q, e)
            assert bits(s) == bits(oracle.bow_score_l1(q, e)) == bits(m.score_l1(q, e)), (name, key)
            assert c == len(np.intersect1d(q[0], e[0]))
            if c:
                assert first == int(np.intersect1d(q[0], e[0])[0])
                rows.append((key, c))
            n += 1
        if len(q[0]) <= 5000:          # (the list walk is one Python step per word and keyframe)
            db = kw.ModelDB(w["n_words"])
            for key, e in alive:
                db.add(key, e)
            keys, common, _ = db.query([q])[0]
            met, counts = kw.inverted_file_order(alive, q)
            assert keys.tolist() == met and common.tolist() == counts and sorted(met) == sorted(k for k, _ in rows)
    assert n >= 5


@pytest.mark.parametrize("name", list(WORLDS))
def test_alone_and_batched_agree_and_the_launch_is_the_one_derived(name):
    t = transcript(name)
    queries = [op for op in WORLDS[name]["ops"] if op[0] in ("query", "refused")]
    assert len(t) == len(queries)
    for (kind, rec), op in zip(t, queries):
        if kind == "refused":
            assert rec is True
            continue
        d = kw._distinct(op[1])
        where = {id(q[0]): k for k, q in enumerate(d)}
        for qi, q in enumerate(op[1]):
            assert rec["batch"][qi] == rec["alone"][where[id(q[0])]]
        assert rec["batch_launch"] == kw.launch_of([len(q[0]) for q in op[1]], rec["entries"])


RULE_WORLD = {r: g for r, g in kw.RULE_GROUP.items()}     # (one world per group: the world is named after its group)


@pytest.mark.parametrize("rule", kw.RULES)
def test_every_wrong_rule_is_caught_by_its_own_group(rule):
    name = RULE_WORLD[rule]
    diff = kw.differences(transcript(name, (rule,)), transcript(name))
    assert diff and all(what in ("alone", "batch", "scores") for _, what in diff), (rule, diff)
    # ... and by the comparison with the oracle: some pair's score, common count or first word is not the oracle's / the intersection's
    caught = 0
    w = WORLDS[name]
    for op in w["ops"]:
        if op[0] != "query":
            continue
        for qi, q in enumerate(op[1]):
            nxt = op[1][qi + 1] if qi + 1 < len(op[1]) else None
            after = None if nxt is None else (int(nxt[0][0]), float(nxt[1][0]))
            for o in w["ops"]:
                if o[0] != "add":
                    continue
                c, first, s = kw.pair(q, o[2], (rule,), after)
                inter = np.intersect1d(q[0], o[2][0])
                caught += bits(s) != bits(oracle.bow_score_l1(q, o[2])) or c != len(inter) or (c > 0 and len(inter) > 0 and first != int(inter[0]))
    assert caught > 0, rule


def test_rules_part_only_where_they_should():
    # the summation rules leave counts and order alone; the order rule leaves every score alone
    for rule in ("tree_sum", "descending_sum", "plus_zero"):
        a, b = transcript("values", (rule,)), transcript("values")
        for (_, x), (_, y) in zip(a, b):
            assert [r[:2] for r in x["batch"]] == [r[:2] for r in y["batch"]]
    a, b = transcript("chunk", ("first_from_last_chunk",)), transcript("chunk")
    assert a[0][1]["scores"] == b[0][1]["scores"] and a[0][1]["batch"][0][0] != b[0][1]["batch"][0][0]
    assert sorted(a[0][1]["batch"][0][0]) == sorted(b[0][1]["batch"][0][0])
    # the le_at_qn rule needs a neighbour in the packed block: alone nothing parts
    a, b = transcript("search", ("le_at_qn",)), transcript("search")
    assert all(x[1]["alone"] == y[1]["alone"] for x, y in zip(a, b)) and a[1][1]["batch"] != b[1][1]["batch"]
