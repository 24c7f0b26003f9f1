"""CPU half of the boundary tests of the triangulation, Sim3 and pose ports (tests/geometry_boundary_worlds.py): the worlds meet their
conditions on the host routine's answers; the independent models equal the host routines byte for byte on every boundary case (which
makes the boundary values the reference's and not the code's own); and the worlds have teeth -- a model with one deliberately wrong
rule parts from the host routine on cases of that rule's group and of no unrelated one.  No device is needed."""
import numpy as np
import pytest

import geometry_boundary_worlds as gb
import pose_model as pm
import sim3_model as sm

f32, f64 = np.float32, np.float64


def test_the_worlds_meet_their_conditions():
    text, counts = gb.check_conditions()
    print(text)
    assert len(counts) > 100 and min(counts.values()) >= 1


# ---- the models equal the host routines ------------------------------------------------------------------------------------------------
def test_triangulation_model_equals_the_host_routine():
    for (name, w, groups, sides), host in zip(gb.tri_worlds(), gb.tri_host()):
        rec = w.model()
        for k in rec.dtype.names:
            bad = np.flatnonzero((rec[k] != host[k]).reshape(len(rec), -1).any(axis=1))
            assert rec[k].tobytes() == host[k].tobytes(), (name, k, sorted({"%s[%s]" % (groups[p], sides[p]) for p in bad}))
        assert rec.tobytes() == host.tobytes(), name


def test_triangulation_host_routine_at_every_batch_position():
    """Every group of every world (the side worlds' single pairs repeated) with its members at positions 0, 63 and 64."""
    worlds, host = gb.tri_worlds(), gb.tri_host()
    orders = gb.batch_orders()
    assert {g for _, g, _ in orders} == {g for _, _, groups, _ in worlds for g in groups}
    for wi, g, order in orders:
        w = worlds[wi][1]
        assert w.host(w.pairs[order]).tobytes() == host[wi][order].tobytes(), g


def test_sim3_model_in_device_order_equals_the_host_routine():
    for (name, W, _), (hrec, hmasks) in zip(gb.sim3_problems(), gb.sim3_host_answers()):
        rec, masks, _, _ = sm.evaluate(W, "device")
        for k in hrec.dtype.names:
            assert rec[k].tobytes() == hrec[k].tobytes(), (name, k)
        assert masks.tobytes() == hmasks.tobytes(), name


def test_a_sim3_batch_is_its_problems_one_by_one():
    """(the offsets of the mask words are non-trivial in the batch: 64, 65, 130 and 200 correspondences, 8 to 64 hypotheses)"""
    probs = gb.sim3_problems()
    for k in (0, 5, 10, 15, 18, len(probs) - 1):
        (rec, masks), = gb.sim3_host([probs[k][1]])
        assert rec.tobytes() == gb.sim3_host_answers()[k][0].tobytes() and masks.tobytes() == gb.sim3_host_answers()[k][1].tobytes(), probs[k][0]


def test_pose_model_in_device_order_equals_the_host_routine():
    for (name, P, _), (hrec, hflags) in zip(gb.pose_problems(), gb.pose_host_answers()):
        rec, flags = pm.optimize(P, "device")
        for k in hrec.dtype.names:
            assert np.asarray(rec[k]).tobytes() == hrec[k].tobytes(), (name, k, rec[k], hrec[k])
        assert np.array_equal(flags, hflags), name


# ---- teeth ------------------------------------------------------------------------------------------------------------------------------
def tri_groups_parting(rule):
    """Groups (camera suffix removed) with a case on which the model under `rule` differs from the host routine."""
    out = set()
    for (name, w, groups, sides), host in zip(gb.tri_worlds(), gb.tri_host()):
        rec = w.model(rules=(rule,))
        for p in np.flatnonzero([rec[p].tobytes() != host[p].tobytes() for p in range(len(rec))]):
            out.add(groups[p].rsplit(", camera", 1)[0])
    return out


@pytest.mark.parametrize("rule, belongs", [
    ("reproj_ge", lambda g: g.startswith("reprojection") and g.endswith("equality")),
    ("stereo_7.815", lambda g: g.startswith("reprojection") and "stereo" in g and not g.endswith("equality")),
    ("depth_lt", lambda g: g.startswith(("z1 <= 0", "z2 <= 0"))),
    ("scale_le", lambda g: g.startswith("scale gate near")),      # (the bisected gates too: their last accepted float IS the equality)
])
def test_a_wrong_triangulation_rule_is_caught_by_its_own_group(rule, belongs):
    parting = tri_groups_parting(rule)
    print(rule, sorted(parting))
    assert parting and all(belongs(g) for g in parting), sorted(parting)


def test_the_reprojection_rules_are_caught_in_every_gate():
    mono_and_stereo = {"reprojection %d %s, equality" % (k, s) for k in (1, 2) for s in ("mono", "stereo")}
    assert tri_groups_parting("reproj_ge") == mono_and_stereo
    stereo = tri_groups_parting("stereo_7.815")
    assert {g.split(",")[0] for g in stereo} == {"reprojection %d stereo %s" % (k, f) for k in (1, 2) for f in ("x", "uright")}
    depth = tri_groups_parting("depth_lt")
    assert depth == {"z1 <= 0, unproject 1", "z2 <= 0, unproject 1"}          # (the SVD path has no exact zero: see the worlds' notes)
    assert "scale gate near, equality" in tri_groups_parting("scale_le")


def test_the_float_constant_for_0_9998_is_not_a_different_rule():
    """`cosParallaxRays < 0.9998f` for the reference's comparison in double: the issue lists it as a wrong rule to be caught.  It cannot
    be, by any input: 0.9998f is the double 0.9998 rounded UP to the next float, so for every float c, `(double)c < 0.9998` holds
    exactly when c is at most the float below 0.9998f, which is when `c < 0.9998f` holds.  The boundary cases sit on exactly these two
    floats, and the model under the float rule equals the host routine on all of them."""
    below, above = (c for c in gb.main_rig().cases if c["group"] == "rays < 0.9998" and c["cam"] == 0 and c["side"] in ("below", "above"))
    cos = [gb.trace1(gb.main_make, 0, c["f1"], c["f2"])["cos_rays"] for c in (below, above)]
    assert f64(cos[0]) < f64(0.9998) < f64(cos[1]) and gb.up(cos[0]) == cos[1]
    assert cos[1] == f32(0.9998) and f64(f32(0.9998)) > f64(0.9998)
    assert tri_groups_parting("float_0.9998") == set()


def sim3_parting(rule):
    """-> ({group: case bits that differ}, differing bits that carry no case, names of the problems that differ)"""
    groups, stray, names = {}, 0, set()
    for (name, W, cases), (hrec, hmasks) in zip(gb.sim3_problems(), gb.sim3_host_answers()):
        rec, masks, _, _ = sm.evaluate(W, "device", rules=(rule,))
        assert all(rec[k].tobytes() == hrec[k].tobytes() for k in hrec.dtype.names if k != "n_inliers")      # the hypotheses are not touched
        diff = masks ^ hmasks
        total = sum(bin(int(w)).count("1") for w in diff.reshape(-1))
        mine = 0
        for group, side, h, i, _ in cases:
            if gb.bit(diff, h, i):
                groups[group] = groups.get(group, 0) + 1
                mine += 1
        stray += total - mine
        if total:
            names.add(name)
    return groups, stray, names


def test_less_or_equal_in_sim3_inlier_is_caught_by_every_rejected_lane_and_by_nothing_without_a_case():
    """Every rejected lane of the threshold problems flips (its err EQUALS its threshold), no bit without a case does, and the
    infinite / NaN errors of depth_zero do not.  (A bisected integral case may flip as well: where the first rejected float gives an
    err of exactly the integral threshold, that case is an equality of the same decision.)"""
    groups, stray, names = sim3_parting("inlier_le")
    print(groups)
    lanes = ("sim3 err1 at its threshold", "sim3 err2 at its threshold")
    n_rejected = sum(1 for _, _, cases in gb.sim3_problems() for c in cases if c[0] in lanes and not c[4])
    assert sum(groups.get(g, 0) for g in lanes) == n_rejected and groups[lanes[0]] == groups[lanes[1]] > 0
    assert all(g.startswith("sim3 err") for g in groups) and stray == 0 and "depth_zero" not in names


@pytest.mark.parametrize("rule", ["float_sum", "fma_to_image"])
def test_a_few_ulp_in_sim3_inlier_are_caught_by_the_threshold_lanes(rule):
    """Asserted: lanes of both threshold groups flip, and depth_zero does not.  Not bounded: how many flip, and the bits that carry no
    case (another hypothesis' err of the same correspondence may lie within the few ulp too; the count is printed)."""
    groups, stray, names = sim3_parting(rule)
    print(rule, groups, "bits without a case:", stray)
    assert groups.get("sim3 err1 at its threshold", 0) > 0 and groups.get("sim3 err2 at its threshold", 0) > 0
    assert "depth_zero" not in names


def test_nine_for_ten_in_the_pose_edge_count_is_caught_by_the_nine_edge_problems_alone():
    parting = set()
    for (name, P, (group, side, _, _)), (hrec, hflags) in zip(gb.pose_problems(), gb.pose_host_answers()):
        rec, flags = pm.optimize(P, "device", rules=("nine_edges",))
        if np.asarray(rec).tobytes() != hrec.tobytes() or not np.array_equal(flags, hflags):
            parting.add((group, side.split()[0]))
    assert parting == {("pose edge count", "9")}


def test_the_hooks_refuse_an_unknown_rule():
    """(That the models without a rule answer what they answered before the hooks is held by the older model tests, not here.)"""
    w = gb.tri_worlds()[0][1]
    with pytest.raises(AssertionError):
        w.model(w.pairs[:1], rules=("no such rule",))
    with pytest.raises(AssertionError):
        sm.evaluate(gb.sim3_problems()[0][1], "device", rules=("no such rule",))
    with pytest.raises(AssertionError):
        pm.optimize(gb.pose_problems()[0][1], "device", rules=("no such rule",))
