"""The boundary worlds of the BoW-gated searches (tests/bow_boundary_worlds.py) on the CPU, before any device sees them: the worlds meet
their conditions, the NumPy restatement (tests/bow_model.py) equals the oracle word for word on every one of them, every boundary pair
lands on the sides its islands are named after, and every wrong rule the restatement offers parts from the oracle on an island of the
group that is there for it.  No GPU, no product code."""
import functools
import numpy as np
import pytest
import bow_boundary_worlds as bw
import bow_model as bm
import oracle

SIZES = bw.form_sizes()
SMALL = SIZES["one_wave"]


def modes_of(w):
    return {"bow": (0, 1), "tri": (2,), "rotation": (0, 1, 2)}[w["kind"]]


@functools.lru_cache(None)
def oracle_answer(name, mode, ori=True):
    nm, match = bw.run(oracle.search_by_bow, oracle.search_for_triangulation, WORLDS[name], mode, ori)
    assert nm == int((match >= 0).sum())
    return match


@functools.lru_cache(None)
def model_answer(name, mode, rules=(), ori=True):
    trace = {}
    fb = lambda *a: bm.py_search_by_bow(*a, rules=rules, trace=trace)
    ft = lambda *a: bm.py_triangulation(*a, rules=rules, trace=trace)
    nm, match = bw.run(fb, ft, WORLDS[name], mode, ori)
    return np.array(match, np.int32), trace


WORLDS = dict(bw.bow_worlds() + bw.rotation_worlds() + bw.tri_worlds())


def islands(w, group, side=None):
    return [(k, i) for k, i in enumerate(w["islands"]) if i["group"] == group and (side is None or i["side"] == side)]


def test_form_sizes_follow_the_join_arithmetic():
    s = SIZES
    assert bw.join_form(s["one_wave"]) == (1, s["one_wave"]) and bw.join_form(s["four_waves"]) == (4, s["four_waves"])
    assert s["four_waves"] == s["one_wave"] + 1 == bw.WIDE_FROM and s["tail"] == s["staged"] + 1
    assert bw.join_form(s["staged"]) == (4, s["staged"])
    waves, lds = bw.join_form(s["tail"])
    assert waves == 4 and 0 < lds < s["tail"] and lds % 64 == 0 and (lds + 64) * 40 + ((s["tail"] + 63) & ~63) > bw.JOIN_LDS_BYTES
    assert s["four_waves"] < s["rounds"] < s["staged"] and "same_lane_third_first" in bw.placements(s["rounds"], *bw.join_form(s["rounds"]))
    assert "same_lane_third_first" not in bw.placements(s["one_wave"], 1, s["one_wave"])       # (one wave: a lane sees two candidates at most)
    tail = bw.placements(s["tail"], *bw.join_form(s["tail"]))
    assert {"stage_end_and_after", "staged_and_tail_same_lane", "both_in_tail"} <= set(tail) and "tail_second_stripe_and_first" not in tail
    long_tail = bw.placements(s["long_tail"], *bw.join_form(s["long_tail"]))
    assert {"tail_second_stripe_and_first", "tail_first_and_third_stripe", "tail_same_lane_two_stripes"} <= set(long_tail) and s["long_tail"] <= 1800


def test_the_worlds_meet_their_conditions():
    for name, w in WORLDS.items():
        assert bw.check_isolation(w) > 0, name
        assert w["form"][:1] + w["form"][2:] == bw.join_form(w["size"]) and w["form"][1] == w["size"]
        assert len(w["a"]["desc"]) < 400 and len(w["a"]["node_id"]) == len(w["b"]["node_id"]) == len(w["islands"])
    for key, size in SIZES.items():
        w = WORLDS["bow_%s_0.7_th50" % key]
        groups = {i["group"] for i in w["islands"]}
        assert {"threshold", "ratio_edge", "ratio_float_equal", "ratio_runner_up", "placement", "claim", "usable"} <= groups
        assert {i["side"] for _, i in islands(w, "placement")} >= {"%s_%s" % (p, s) for p in bw.placements(size, *bw.join_form(size)) for s in ("accepted", "refused")}
    # float against double in the ratio test: pairs exist for the ratios whose float lies ABOVE the decimal; for the others the rule is
    # provably the same one (no pair of integer distances at all tells the two products apart) -- asserted here over every pair
    for r in bw.RATIOS:
        pairs = bw.float_double_pairs(r)
        assert bool(pairs) == (float(np.float32(r)) > r), r
    assert bw.float_double_pairs(0.6, 30) and bw.float_double_pairs(0.8, 50)
    assert sum(WORLDS["rotation_%s_one_wave" % p]["rot_half_exact"] for p in ("edges_a", "edges_b")) > 0


@pytest.mark.parametrize("kind", ["bow", "rotation", "tri"])
def test_model_equals_oracle_on_every_world(kind):
    for name, w in WORLDS.items():
        if w["kind"] != kind:
            continue
        for mode in modes_of(w):
            for ori in (True, False) if w["size"] == SMALL else (True,):
                got, _ = model_answer(name, mode, (), ori)
                want = oracle_answer(name, mode, ori)
                assert np.array_equal(got, want), (name, mode, ori, bw.kinds_of_differences(w, mode, got, want))


def probe_answers(name, mode, ori=True):
    w = WORLDS[name]
    return {(i["group"], i["side"]): a for i, a in zip(w["islands"], bw.answers(w, mode, oracle_answer(name, mode, ori)))}


@pytest.mark.parametrize("key", list(SIZES))
def test_bow_pairs_land_on_their_sides(key):
    for r in bw.RATIOS:
        name = "bow_%s_%g_th%d" % (key, r, 30 if r == bw.RATIOS[0] else 50)
        w = WORLDS[name]; th = w["th"]
        for mode in (0, 1):
            ans = probe_answers(name, mode)
            _, tr = model_answer(name, mode)
            for isl in w["islands"]:
                g, side, t = isl["group"], isl["side"], tr.get(isl["probe"])
                got = ans[(g, side)]
                if g == "threshold":
                    assert t["best"] == {"below": th - 1, "at": th, "above": th + 1}[side] and t["second"] == 256
                    assert got == [{"below": "a", "at": "a" if mode == 0 else "", "above": ""}[side]]
                elif g.startswith("ratio_") and g != "ratio_runner_up":
                    verdict, b, s = side.replace("_rev", "").split("_")
                    assert (t["best"], t["second"]) == (int(b), int(s)) and t["accepted"] == (verdict == "accepted") and got == ["a" if t["accepted"] else ""]
                    assert t["ratio"] == (float(b), float(np.float32(np.float32(r) * np.float32(int(s)))))
                    if g == "ratio_float_equal" and t["ratio"][0] == t["ratio"][1]:
                        assert not t["accepted"]
                elif g == "placement":
                    rb, rs = w["refused"]
                    assert (t["best"], t["second"]) == ((rb, rs) if side.endswith("refused") else (rb - 1, rs))
                    assert got == ["" if side.endswith("refused") else "a"]
            rb, rs = w["refused"]
            assert ans[("ratio_runner_up", "absent")] == ans[("ratio_runner_up", "at_256")] == ans[("ratio_runner_up", "at_256_with_fillers_at_256")] == ["a"]
            assert ans[("ratio_runner_up", "present")] == ans[("ratio_runner_up", "equal_to_best")] == [""]
            assert tr[dict((i["side"], i) for _, i in islands(w, "ratio_runner_up"))["at_256"]["probe"]]["second"] == 256
            # claims
            assert ans[("claim", "taken")] == ["a", "b"] and ans[("claim", "free")] == ["a"] and ans[("claim", "first_refused")] == ["", "a"]
            assert ans[("claim", "taken_across_the_block")] == [""] * 63 + ["a", "b"] and ans[("claim", "free_across_the_block")] == [""] * 64 + ["a"]
            assert ans[("claim", "chain_of_three")] == ["a", "b", "c" if 40 < th else ""]
            assert ans[("claim", "taken_then_filtered")] == ["", "b"] and probe_answers(name, mode, False)[("claim", "taken_then_filtered")] == ["a", "b"]
            assert ans[("usable", "b_cleared_on_best")] == [("a", "b")[mode]] and ans[("usable", "b_cleared_on_runner_up")] == [("", "a")[mode]]
            assert ans[("usable", "a_cleared_on_blocker")] == ["", "a"] and ans[("usable", "a_cleared_on_probe")] == [""]
            big = [s for (g, s) in ans if g == "claim" and s in ("taken_staged", "taken_last_staged", "taken_in_tail", "runner_up_in_tail",
                                                                 "taken_in_tail_stripe_1", "taken_in_tail_stripe_2")]
            assert all(ans[("claim", s)] == ["a", "b"] for s in big)
            assert len(big) == (0 if r not in bw.BIG_RATIOS else {"tail": 4, "long_tail": 6}.get(key, 2))
            stripes = [s for (g, s) in ans if g == "claim" and s.startswith("taken_in_stripe_")]
            assert all(ans[("claim", s)] == ["a", "b"] for s in stripes) and len(stripes) == (1 if key in ("one_wave", "four_waves") else 3)
            if len(stripes) == 3:
                assert ans[("claim", "chain_over_the_stripes")] == ["a", "b", "c" if 40 < th else ""]
    name = "bow_%s_%g_th50" % (key, bw.TIE_RATIO)
    for mode in (0, 1):
        ans = probe_answers(name, mode)
        assert ans[("tie", "equal_first_wins")] == ans[("tie", "equal_first_wins_far_apart")] == ["a"] and ans[("tie", "second_nearer")] == ["b"]


@pytest.mark.parametrize("key", list(SIZES))
def test_rotation_pairs_land_on_their_bins(key):
    want_maxima = {"ten_one_one": (10, 1, 1), "eleven_one_one": (11, 1, 1), "two_equal": (4, 4, 2), "three_equal": (3, 3, 3), "four_equal": (3, 3, 3), "empty": (0, 0, 0)}
    for p in bw.POPULATIONS:
        name = "rotation_%s_%s" % (p, key)
        w = WORLDS[name]
        for mode in (0, 1, 2):
            _, tr = model_answer(name, mode)
            named = 0
            for isl in w["islands"]:
                if "bin" in isl["side"]:
                    assert tr[isl["probe"]]["bin"] == int(isl["side"].split("bin")[1]), (name, isl["side"])
                    named += 1
            assert named or p == "empty"
            if p in want_maxima:
                assert tr["maxima"][:3] == want_maxima[p]
            if p == "wrap":
                sides = {i["side"]: tr[i["probe"]] for _, i in islands(w, "rot_zero")}
                assert sides["to_360"]["rot"] == np.float32(360.0) and sides["to_360"]["bin"] == 12 and sides["plus_zero"]["bin"] == sides["minus_zero"]["bin"] == 0
            if p.startswith("edges"):
                edge = [tr[i["probe"]] for _, i in islands(w, "rot_edge")]
                assert len({t["bin"] for t in edge}) >= 7
                halves = [t for t in edge if float(np.float32(t["rot"] * np.float32(1.0 / 30))) % 1.0 == 0.5]
                assert all(t["bin"] == int(float(np.float32(t["rot"] * np.float32(1.0 / 30))) + 0.5) for t in halves)
        # 10/1/1 keeps the two single bins (1.0f < 0.1f * 10.0f is false in float), 11/1/1 drops them
        if p in ("ten_one_one", "eleven_one_one"):
            ans = probe_answers(name, 1)
            singles = [a for (g, s), a in ans.items() if s in ("bin5", "bin8")]
            assert len(singles) == 2 and all(a == (["a"] if p == "ten_one_one" else [""]) for a in singles)


@pytest.mark.parametrize("key", list(SIZES))
def test_triangulation_pairs_land_on_their_sides(key):
    name = "tri_%s" % key
    w = WORLDS[name]; th = w["th"]; T = w["tri"]
    ans = probe_answers(name, 2)
    _, tr = model_answer(name, 2)
    by = {(i["group"], i["side"]): i for i in w["islands"]}
    gate = lambda g, s, role="a": tr[by[(g, s)]["probe"]]["gates"][by[(g, s)]["cands"][role]]
    assert ans[("threshold", "below")] == ans[("threshold", "at")] == ["a"] and ans[("threshold", "above")] == [""]
    yb = lambda g, s: w["b"]["y"][by[(g, s)]["cands"]["a"]]
    xb = lambda g, s: w["b"]["x"][by[(g, s)]["cands"]["a"]]
    for o in (0, 3, 7):
        for sgn in ("+1", "-1"):
            p, r = "pass_o%d%s" % (o, sgn), "reject_o%d%s" % (o, sgn)
            assert gate("dsqr", p)[0] == "pass" and gate("dsqr", r)[0] == "dsqr" and ans[("dsqr", p)] == ["a"] and ans[("dsqr", r)] == [""]
            assert abs(int(yb("dsqr", p).view(np.int32)) - int(yb("dsqr", r).view(np.int32))) == 1        # one float of y2 apart
            assert gate("dsqr", p)[2] == gate("dsqr", r)[2] == 3.84 * float(T["s2"][o])
            assert gate("epipole", p)[0] == "pass" and gate("epipole", r)[0] == "epipole" and ans[("epipole", p)] == ["a"] and ans[("epipole", r)] == [""]
            assert abs(int(xb("epipole", p).view(np.int32)) - int(xb("epipole", r).view(np.int32))) == 1
            assert gate("epipole", r)[2] == float(np.float32(100) * T["sf"][o])
    assert ans[("epipole", "equal_6_8_pass")] == ["a"]
    q = by[("epipole", "equal_6_8_pass")]; c = q["cands"]["a"]
    assert bm.epipole_rejects(T["ex"][0], T["ey"][0], w["b"]["x"][c], w["b"]["y"][c], T["sf"][0])[1:] == (np.float32(100.0), np.float32(100.0))
    for nq in ("mono", "stereo"):
        for ncn in ("mono", "stereo"):
            inside = "%s_%s_inside" % (nq, ncn)
            assert ans[("epipole_flags", inside)] == ([""] if (nq, ncn) == ("mono", "mono") else ["a"])
            assert ans[("epipole_flags", "%s_%s_outside" % (nq, ncn))] == ["a"]
    assert gate("epipole_flags", "mono_mono_inside")[0] == "epipole"
    assert gate("dsqr_equal", "zero_sigma_reject")[:2] == ("dsqr", 0.0) and gate("dsqr_equal", "zero_sigma_reject")[2] == 0.0 and ans[("dsqr_equal", "unit_sigma_pass")] == ["a"]
    assert gate("den", "zero")[0] == "den" and ans[("den", "zero")] == [""] and ans[("den", "rows")] == ["a"]
    assert ans[("camera", "other_is_nearer")] == ["b"] and ans[("camera", "same")] == ["a"] and ans[("camera", "only_other")] == [""]
    assert ans[("usable", "b_cleared_on_best")] == ["b"] and ans[("usable", "a_cleared")] == [""]
    assert ans[("ties", "two_equal")] == ["b"] and ans[("ties", "three_equal")] == ["c"] and ans[("ties", "later_equal_fails")] == ["a"]
    assert ans[("ties", "later_nearer_fails")] == ["a"] and ans[("ties", "earlier_nearer_fails")] == ["b"] and ans[("ties", "nearer_fails_epipole")] == ["b"]
    places = bw.placements(w["size"], 1, bw.join_form(w["size"])[1])
    assert places and ("tail" not in key or "both_in_tail" in places)
    for pname, p in places.items():
        assert ans[("tie_placement", pname)] == ["a" if p["b"] > p["s"] else "b"], pname                  # the later of the two that pass
    assert ans[("queries", "five_in_a_node")] == ["a"] * 5 and ans[("queries", "across_the_block")] == ["a"] * 67
    # the float / double compare and the contracted numerator part on the level whose sigma2 was placed for them
    for k, rule in (("float", "dsqr_float"), ("fma", "num_fma")):
        c = T[k]
        la, lb, lc = bm.epipolar_line(bw.SLANT, c["x1"], c["y1"])
        right = bm.dsqr_passes(bm.epipolar_dsqr(la, lb, lc, c["x2"], c["y2"])[0], c["sigma2"])
        wrong = bm.dsqr_passes(bm.epipolar_dsqr(la, lb, lc, c["x2"], c["y2"], (rule,))[0], c["sigma2"], (rule,))
        assert right != wrong and ans[("dsqr_" + k, "at_placed_sigma")] == (["a"] if right else [""])


# ---- every wrong rule parts from the oracle, on an island of the group that is there for it --------------------------------------------------
BOW_RULES = {   # rule -> (world, modes, groups one of which must own a differing word)
    "bin_half_even": ("rotation_edges_a_one_wave", (0, 1, 2), {"rot_edge"}),
    "bin_divide": ("rotation_edges_a_one_wave", (0, 1, 2), {"rot_edge", "rot_wrap"}),
    "maxima_double": ("rotation_ten_one_one_one_wave", (0, 1, 2), {"hist_ballast"}),
    "th_swapped": ("bow_one_wave_0.7_th50", (0, 1), {"threshold"}),
    "ratio_double": ("bow_one_wave_0.6_th30", (0, 1), {"ratio_float_double"}),
    "claims_ignored": ("bow_one_wave_0.7_th50", (0, 1), {"claim"}),
    "claims_after_rotation": ("bow_one_wave_0.7_th50", (0,), {"claim"}),
    "mode1_ignores_b_flag": ("bow_one_wave_0.7_th50", (1,), {"usable"}),
    "mode0_honours_b_flag": ("bow_one_wave_0.7_th50", (0,), {"usable"}),
    "last_on_ties": ("bow_one_wave_%g_th50" % bw.TIE_RATIO, (0, 1), {"tie"}),
}
TRI_RULES = {
    "bin_half_even": {"rot_edge"}, "bin_divide": {"rot_edge", "rot_wrap"}, "maxima_double": {"hist_ballast"},
    "epipole_le": {"epipole"}, "epipole_always": {"epipole_flags"}, "dsqr_float": {"dsqr_float"}, "dsqr_le": {"dsqr_equal"}, "num_fma": {"dsqr_fma"},
    "th_ge_rejects": {"threshold"}, "den_zero_accepted": {"den"}, "camera_ignored": {"camera"}, "shadow": {"ties"}, "first_on_ties": {"ties", "tie_placement"},
}


def parts(name, mode, rule):
    w = WORLDS[name]
    rules = (rule,)
    if (w["kind"] == "tri" or mode == 2) and rule not in bm.RULES_TRI or mode != 2 and rule not in bm.RULES_BOW:
        raise AssertionError(rule)
    got, _ = model_answer(name, mode, rules)
    return {k.split("[")[0] for k in bw.kinds_of_differences(w, mode, got, oracle_answer(name, mode))}


@pytest.mark.parametrize("rule", bm.RULES_BOW)
def test_every_wrong_bow_rule_parts_from_the_oracle(rule):
    name, modes, groups = BOW_RULES[rule]
    for mode in modes:
        if mode == 2:
            continue
        assert parts(name, mode, rule) & groups, (rule, mode)
    if rule == "ratio_double":
        assert parts("bow_one_wave_0.8_th50", 0, rule) & groups
        for r in (0.7, 0.75, 0.9):      # provably the same rule there (test_the_worlds_meet_their_conditions): nothing parts
            assert not parts("bow_one_wave_%g_th50" % r, 0, rule) and not parts("bow_one_wave_%g_th50" % r, 1, rule)
    if rule == "th_swapped":            # each mode parts on the island AT the threshold, and only there
        w = WORLDS[name]
        for mode in modes:
            got, _ = model_answer(name, mode, (rule,))
            assert bw.kinds_of_differences(w, mode, got, oracle_answer(name, mode)) == ["threshold[at]"]


@pytest.mark.parametrize("rule", bm.RULES_TRI)
def test_every_wrong_triangulation_rule_parts_from_the_oracle(rule):
    name = BOW_RULES[rule][0] if rule in bm.RULES_COMMON else "tri_one_wave"
    assert parts(name, 2, rule) & TRI_RULES[rule], rule


def test_every_offered_rule_is_held():
    assert set(BOW_RULES) == set(bm.RULES_BOW) and set(TRI_RULES) == set(bm.RULES_TRI)
