"""CPU half of the boundary tests of the PnPsolver port (tests/pnp_boundary_worlds.py): the worlds meet their conditions on the model and
on the host routine; the host routine equals tests/pnp_model.py byte for byte on every boundary problem (which makes the boundary
values the reference's and not the code's own); and the worlds have teeth -- the model with one deliberately wrong rule parts from the
host routine on cases of that rule's kind.  No device is needed."""
import numpy as np
import pytest

import pnp_boundary_worlds as pb
import pnp_model as pm


def test_the_worlds_meet_their_conditions():
    text, counts = pb.check_conditions()
    print(text)
    assert set(counts) == {pb.G_HYP, pb.G_REF, pb.G_REAL, pb.G_NONFINITE, pb.G_RECORDS} and min(counts.values()) >= 1


def test_the_host_routine_equals_the_model_on_every_boundary_problem():
    for w, mod, got in zip(pb.problems(), pb.model_answers(), pb.host_answers()):
        assert pb.fields_differing(mod, got) == [], w["name"]


def test_the_model_without_a_rule_is_the_model():
    """evaluate() remembers the poses and hands out error2; without a rule it answers what pm.ransac_multi answers."""
    for w, mod in zip(pb.problems(), pb.model_answers()):
        ev = pb.evaluate(w)
        assert ev["rec"] == mod["rec"], w["name"]
        for k in ("R", "t", "err", "choice", "flags", "n_inliers", "words", "ref_R", "ref_t", "ref_flags", "ref_n_inliers", "ref_n_set", "ref_words"):
            assert np.asarray(ev[k]).tobytes() == np.asarray(mod[k]).tobytes(), (w["name"], k)


def test_a_batch_is_its_problems_one_by_one():
    """(the offsets of the mask words and of the refined masks are non-trivial in the batch: 1 to 5 words, 3 to 64 hypotheses)"""
    probs, answers = pb.problems(), pb.host_answers()
    for k in (0, 7, 9, 15, 20, len(probs) - 1):
        got, = pb.host([probs[k]])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, answers[k])), probs[k]["name"]


# ---- teeth ------------------------------------------------------------------------------------------------------------------------------
def parting(rule):
    """The model under `rule` against the host routine -> ({group: cases whose bit differs}, {group: names of the problems}); a problem
    whose records differ counts once under the record choice, and its refined cases are not looked at (their records are others)."""
    groups, names = {}, {}

    def add(g, name, n=1):
        groups[g] = groups.get(g, 0) + n
        names.setdefault(g, set()).add(name)
    for w, (hyp, words, ref, rwords) in zip(pb.problems(), pb.host_answers()):
        ev = pb.evaluate(w, rule)
        same_records = ev["rec"] == [int(h) for h in ref["hyp"]]
        if not same_records:
            add(pb.G_RECORDS, w["name"])
        for g, _, stage, k, i, _ in w["cases"]:
            if stage == "hyp" and pb.bit(ev["words"] ^ words, k, i):
                add(g, w["name"])
            if stage == "ref" and same_records and pb.bit(ev["ref_words"] ^ rwords, k, i):
                add(g, w["name"])
    return groups, names


def test_less_or_equal_is_caught_by_every_rejected_lane():
    """Every rejected lane of the hypothesis stage flips (its error2 EQUALS its threshold), rejected lanes of the refined stage do, and
    `inf <= inf` does."""
    groups, names = parting("inlier_le")
    print("inlier_le", groups)
    n_rejected = sum(1 for w in pb.problems() for c in w["cases"] if c[0] == pb.G_HYP and not c[5])
    assert groups[pb.G_HYP] == n_rejected > 0
    assert groups.get(pb.G_REF, 0) > 0 and groups.get(pb.G_NONFINITE, 0) > 0


@pytest.mark.parametrize("rule", ["fused_sum", "xc_double", "inv_float", "ue_float"])
def test_a_few_ulp_in_error2_are_caught_by_the_threshold_lanes(rule):
    """Asserted: lanes of a threshold group flip.  Not bounded: how many (printed; the table of the notes)."""
    groups, names = parting(rule)
    print(rule, groups)
    assert groups.get(pb.G_HYP, 0) + groups.get(pb.G_REF, 0) > 0
    assert "non_finite" not in names.get(pb.G_NONFINITE, ())


def test_greater_for_greater_or_equal_min_inliers_is_caught_where_a_count_equals_it():
    groups, names = parting("min_gt")
    print("min_gt", groups, sorted(names[pb.G_RECORDS]))
    assert "records/min_inliers = c" in names[pb.G_RECORDS] and "records/min_inliers = c + 1" not in names[pb.G_RECORDS]
    assert set(groups) == {pb.G_RECORDS}                      # (no mask bit of the hypothesis stage moves)


def test_greater_or_equal_for_greater_than_best_is_caught_where_a_count_equals_it():
    groups, names = parting("best_ge")
    print("best_ge", groups, sorted(names[pb.G_RECORDS]))
    assert {"records/best_start = c", "records/best_start = c1", "records/h0 twice"} <= names[pb.G_RECORDS]
    assert not {"records/best_start = c - 1", "records/best_start = c1 - 1"} & names[pb.G_RECORDS]
    assert set(groups) == {pb.G_RECORDS}


def test_an_unknown_rule_is_refused():
    with pytest.raises(AssertionError):
        pb.evaluate(pb.problems()[0], "no such rule")


def test_records_of_the_worlds_module_are_the_models():
    rng = np.random.default_rng(3)
    for _ in range(50):
        counts = rng.integers(0, 12, 20)
        mi, bs = int(rng.integers(0, 8)), int(rng.integers(0, 8))
        assert pb.records(counts, mi, bs) == pm.records(counts, mi, bs)
