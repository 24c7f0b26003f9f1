"""The boundary worlds of tests/search_boundary_worlds.py against the ORACLE alone (no device): the worlds have something to find.

1. Every decision group marked `paired` gets at least two different answers from the oracle over its members (matched / not matched,
   another feature of the island, taken back by the rotation histogram).
2. The worlds do not pass under a wrong rule: a small NumPy restatement of the searches (below; it equals the oracle on every world
   under the right rules) decides differently from the oracle on at least one island of the matching kind under each of
   `<` for `<=` at the threshold, round-to-even for roundf, double for float in the ratio test and in the chi-square compare,
   `>=` for `>` in the right-coordinate gate, `<=` for `<` in the window.
3. Every kind is there, on both sides, and the builder left nothing out."""
import numpy as np
import pytest

import oracle
import search_boundary_worlds as sw
import test_oracle_undistort as undistort

f32 = np.float32
ROUND_BOUNDS = (0.0, 0.0, 640.0, 480.0)


def calibrated_bounds():
    return oracle.image_bounds(undistort.MULTI_YAML, 640, 480)


BOUNDS = {"round": lambda: ROUND_BOUNDS, "calibrated": calibrated_bounds}
TH = {"frames": 100, "points": 100, "loop2": 50, "best": 100}


# ------------------------------------------------------------------------------------------------ the restatement
RIGHT = dict(th_lt=False, hist_rint=False, insert_rint=False, ratio_double=False, chi2_double=False, right_ge=False, window_le=False)


def _rules(**kw):
    r = dict(RIGHT); r.update(kw)
    return r


class Model:
    def __init__(self, w, rules):
        fr = w["fr"]; self.w = w; self.fr = fr; self.R = rules
        self.G = sw.Grid(fr["bounds"])
        self.x = np.asarray(fr["un_x"], f32); self.y = np.asarray(fr["un_y"], f32)
        self.oct = np.asarray(fr["octave"]); self.ang = np.asarray(fr["angle"], f32); self.ur = np.asarray(fr["uright"], f32)
        self.cam = np.asarray(fr["cam_of"]); self.n = len(self.x)
        self.desc = np.concatenate(fr["descs"])
        rnd = (lambda v: int(np.rint(v))) if rules["insert_rint"] else sw.round_half_away
        self.cells = {}
        for g in range(self.n):
            px, py = rnd(self.G.posx(self.x[g])), rnd(self.G.posy(self.y[g]))
            if 0 <= px < sw.GRID_COLS and 0 <= py < sw.GRID_ROWS:
                self.cells.setdefault((int(self.cam[g]), px, py), []).append(g)

    def area(self, cam, x, y, r, lo, hi):
        G = self.G; x = f32(x); y = f32(y); r = f32(r)
        tx = f32(x - G.minX); ty = f32(y - G.minY)
        x0 = max(0, int(np.floor(f32(f32(tx - r) * G.invW))))
        x1 = min(sw.GRID_COLS - 1, int(np.ceil(f32(f32(tx + r) * G.invW))))
        y0 = max(0, int(np.floor(f32(f32(ty - r) * G.invH))))
        y1 = min(sw.GRID_ROWS - 1, int(np.ceil(f32(f32(ty + r) * G.invH))))
        if x0 >= sw.GRID_COLS or x1 < 0 or y0 >= sw.GRID_ROWS or y1 < 0:
            return []
        check = lo > 0 or hi >= 0
        inside = (lambda d: d <= r) if self.R["window_le"] else (lambda d: d < r)
        out = []
        for ix in range(x0, x1 + 1):
            for iy in range(y0, y1 + 1):
                for g in self.cells.get((cam, ix, iy), ()):
                    if check and (self.oct[g] < lo or (hi >= 0 and self.oct[g] > hi)):
                        continue
                    if inside(abs(f32(self.x[g] - x))) and inside(abs(f32(self.y[g] - y))):
                        out.append(g)
        return out

    def dist(self, q, g):
        return int(np.unpackbits(np.bitwise_xor(q["desc"], self.desc[g])).sum())

    def right_closed(self, q, g):
        if not self.ur[g] > 0:
            return False
        er = abs(f32(q["ur"] - self.ur[g]))
        return bool(er >= q["radius"]) if self.R["right_ge"] else bool(er > q["radius"])

    def accept(self, best, th):
        return best < th if self.R["th_lt"] else best <= th

    def frames(self, th, check_ori, occ):
        q = self.w["q"]; mo = np.full(self.n, -1, np.int64); nm = 0
        hist = [[] for _ in range(sw.HISTO_LENGTH)]
        rnd = (lambda v: int(np.rint(v))) if self.R["hist_rint"] else sw.round_half_away
        for i in range(len(q)):
            best, bi = 256, -1
            for g in self.area(int(q["cam"][i]), q["u"][i], q["v"][i], q["radius"][i], int(q["min_level"][i]), int(q["max_level"][i])):
                if occ is not None and occ[g] and mo[g] < 0:
                    continue
                if mo[g] >= 0 and q["blocks"][mo[g]]:
                    continue
                if self.right_closed(q[i], g):
                    continue
                d = self.dist(q[i], g)
                if d < best:
                    best, bi = d, g
            if bi >= 0 and self.accept(best, th):
                mo[bi] = i; nm += 1
                if check_ori:
                    hist[sw.rot_bin(sw.rot_of(q["angle"][i], self.ang[bi]), rnd)].append(bi)
        if check_ori:
            keep = oracle.three_maxima([len(h) for h in hist])
            for b, h in enumerate(hist):
                if b not in keep:
                    for g in h:
                        mo[g] = -2; nm -= 1
        return nm, mo

    def points(self, th, nnratio, occ):
        q = self.w["q"]; mo = np.full(self.n, -1, np.int64); nm = 0
        for i in range(len(q)):
            best, best2, lvl, lvl2, bi = 256, 256, -1, -1, -1
            for g in self.area(0, q["u"][i], q["v"][i], q["radius"][i], int(q["min_level"][i]), int(q["max_level"][i])):
                if occ is not None and occ[g]:
                    continue
                if mo[g] >= 0 and q["blocks"][mo[g]]:
                    continue
                if self.right_closed(q[i], g):
                    continue
                d = self.dist(q[i], g)
                if d < best:
                    best2, best, lvl2, lvl, bi = best, d, lvl, int(self.oct[g]), g
                elif d < best2:
                    lvl2, best2 = int(self.oct[g]), d
            if bi >= 0 and self.accept(best, th):
                if lvl == lvl2 and sw.ratio_rejects(best, best2, nnratio, self.R["ratio_double"]):
                    continue
                mo[bi] = i; nm += 1
        return nm, mo

    def loop2(self, th, occ):
        q = self.w["q"]; w2 = self.w["w2"]; mo = np.full(self.n, -1, np.int64); nm = 0
        for i in range(len(q)):
            best, bi = 256, -1
            wins = ((q["cam"][i], q["u"][i], q["v"][i], q["radius"][i], q["min_level"][i], q["max_level"][i]),
                    (w2["cam"][i], w2["u"][i], w2["v"][i], w2["radius"][i], w2["min_level"][i], w2["max_level"][i]))
            for cam, u, v, r, lo, hi in wins:
                if cam < 0:
                    continue
                for g in self.area(int(cam), u, v, r, -1, -1):
                    if (occ is not None and occ[g]) or mo[g] >= 0:
                        continue
                    if self.oct[g] < lo or self.oct[g] > hi:
                        continue
                    d = self.dist(q[i], g)
                    if d < best:
                        best, bi = d, g
            if bi >= 0 and self.accept(best, th):
                mo[bi] = i; nm += 1
        return nm, mo

    def best(self, gate, occ, sg):
        q = self.w["q"]; bi_out = np.full(len(q), -1, np.int64); bd_out = np.full(len(q), 256, np.int64)
        for i in range(len(q)):
            for g in self.area(int(q["cam"][i]), q["u"][i], q["v"][i], q["radius"][i], int(q["min_level"][i]), int(q["max_level"][i])):
                if occ is not None and occ[g]:
                    continue
                if gate == 1 and self.right_closed(q[i], g):
                    continue
                if gate == 2:
                    stereo = self.ur[g] >= 0
                    v = sw.chi2_value(f32(q["u"][i] - self.x[g]), f32(q["v"][i] - self.y[g]), f32(q["ur"][i] - self.ur[g]) if stereo else None,
                                      sg[self.oct[g]], self.R["chi2_double"])
                    if v > (7.8 if stereo else 5.99):
                        continue
                d = self.dist(q[i], g)
                if d < bd_out[i]:
                    bd_out[i], bi_out[i] = d, g
        return bi_out, bd_out


# ------------------------------------------------------------------------------------------------ oracle runs
def oracle_run(w, check_ori=True, gate=0):
    OF = oracle.FrameData(**w["fr"]); occ = w["occ"]
    if w["search"] == "frames":
        return oracle.search_by_projection_frames(OF, w["q"], w["th"], check_ori, occ)
    if w["search"] == "points":
        return oracle.search_by_projection_points(OF, w["q"], occ, w["nnratio"], w["th"])
    if w["search"] == "loop2":
        return oracle.search_by_projection_loop2(OF, w["q"], w["w2"], occ, w["th"])
    return oracle.project_best(OF, w["q"], occ, gate, w["inv_sigma2"])


def model_run(w, rules, check_ori=True, gate=0):
    M = Model(w, rules); occ = w["occ"]
    if w["search"] == "frames":
        return M.frames(w["th"], check_ori, occ)
    if w["search"] == "points":
        return M.points(w["th"], w["nnratio"], occ)
    if w["search"] == "loop2":
        return M.loop2(w["th"], occ)
    return M.best(gate, occ, w["inv_sigma2"])


def answers_of(w, result, unfiltered=None):
    if w["search"] == "best":
        bi = np.asarray(result[0])
        return np.array([w["roles"][g] if g >= 0 else "" for g in bi], dtype=object)
    return sw.answers(w, np.asarray(result[1]), None if unfiltered is None else np.asarray(unfiltered[1]))


def gate_of(kind):
    return 1 if kind.startswith("right") else 2 if kind.startswith("chi2") else 0


_worlds = {}


def world(search, bounds_name, nnratio=0.8, population=None):
    key = (search, bounds_name, nnratio, population)
    if key not in _worlds:
        _worlds[key] = sw.make_search_world(search, BOUNDS[bounds_name](), th=TH[search], nnratio=nnratio, population=population)
    return _worlds[key]


def all_worlds(bounds_name):
    for s in ("frames", "loop2", "best"):
        yield world(s, bounds_name)
    for r in sw.RATIOS:
        yield world("points", bounds_name, r)
    for p in sw.POPULATIONS:
        yield world("frames", bounds_name, population=p)


# ------------------------------------------------------------------------------------------------ which sides of a group face each other
PAIRS = {"threshold": [("at", "above"), ("below", "above")],
         "threshold_second": [("under", "over"), ("at", "over")],
         "tie_cell": [("equal", "second"), ("equal3", "third")],
         "tie_cells": [("equal3", "equal2"), ("equal3", "last"), ("equal2", "last")],
         "claimed": [("blocking", "unclaimed"), ("blocking", "overwritten")],
         "shortlist": [("k", "k+1"), ("k+1", "k+1_open"), ("k+1_at_th", "k+1_over_th"), ("k", "k+1_at_th")],
         "window_outside": [("%s_%s" % (n, a), "%s_%s" % (n, b)) for n in ("left", "right", "top", "bottom")
                            for a in ("inside", "partly") for b in ("beyond", "wholly")],
         "right_edge": [("on+1", "out+1"), ("on-1", "out-1")],
         "right_sign": [("zero", "smallest_positive"), ("minus_zero", "smallest_positive"), ("minus_one", "smallest_positive")],
         "chi2_branch": [("zero", "minus_one"), ("minus_zero", "largest_negative"), ("zero", "largest_negative")],
         "level2": [("lo>hi_o3", "lo<hi_o3"), ("lo<hi_o3", "lo<hi_o4"), ("lo==hi_o2", "lo==hi_o3"), ("lo==hi_o3", "lo==hi_o4"), ("lo>hi_o2", "lo<hi_o2")],
         "tie_windows": [("equal", "second_nearer"), ("equal", "only_second")],
         "ratio_second_hidden": [("second_counts", "second_occupied"), ("second_counts", "second_claimed")],
         "rot_zero": [("plus_zero", "to_360"), ("minus_zero", "to_360"), ("plus_zero", "to_360_from_one")]}


def pairs_of(kind, sides):
    """The boundary pairs of a group, by side name: each must get two different answers."""
    if len(sides) == 2:
        return [tuple(sides)]
    if kind in PAIRS:
        return [p for p in PAIRS[kind] if p[0] in sides and p[1] in sides]
    if kind == "capacity":                               # per list length: the winner at the end of the list against the tie the first entry wins
        return [(s, "first_" + s[5:]) for s in sides if s.startswith("last_")]
    if kind in ("ratio_edge", "ratio_float_double"):     # the largest accepted best against best + 1, in both visiting orders
        return [(a, b) for a in sides if a.startswith("accepted") for b in sides if b.startswith("rejected")]
    if kind == "rot_edge":                               # neighbours one ulp apart that fall into different bins (the side names its bin)
        return [(a, b) for i, a in enumerate(sides) for b in sides[i + 1:] if a.rsplit("_", 1)[1] != b.rsplit("_", 1)[1]]
    if kind == "level":                                  # octaves next to each other on either side of min_level / max_level
        lo, hi = (int(v) for v in sides[0].replace("min", "").replace("max", "").split("_")[:2])
        ok = lambda o: not ((lo > 0 or hi >= 0) and (o < lo or (hi >= 0 and o > hi)))
        octs = sorted(int(s.rsplit("_o", 1)[1]) for s in sides)
        return [("min%d_max%d_o%d" % (lo, hi, a), "min%d_max%d_o%d" % (lo, hi, b)) for a, b in zip(octs, octs[1:]) if ok(a) != ok(b)]
    raise AssertionError("no pairing known for kind %s: %s" % (kind, sides))


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("bounds_name", list(BOUNDS))
def test_every_paired_group_gets_two_answers_and_nothing_is_left_out(bounds_name):
    for w in all_worlds(bounds_name):
        assert w["dropped"] == 0                                         # the share of cases the builder may leave out is zero
        assert w["n_island_queries"] == len(w["q"]) and (w["groups"] >= 0).sum() > 0
        per_gate = {}
        for gate in ((0, 1, 2) if w["search"] == "best" else (0,)):
            res = oracle_run(w, True, gate)
            per_gate[gate] = answers_of(w, res, oracle_run(w, False) if w["search"] == "frames" else None)
        for g in range(len(w["paired"])):
            members = np.flatnonzero(w["groups"] == g)
            kind = str(w["group_kind"][g])
            assert kind == "hist_bin" or len(set(w["sides"][members])) == len(members) >= 2, (kind, w["sides"][members])
            got = per_gate[gate_of(kind) if w["search"] == "best" else 0][members]
            if w["paired"][g]:
                by_side = dict(zip(w["sides"][members].tolist(), got))
                pairs = pairs_of(kind, list(by_side))
                assert pairs, (kind, list(by_side))
                for a, b in pairs:                       # the two sides of EVERY boundary pair of the group, not just two answers in it
                    assert by_side[a] != by_side[b], (w["search"], w["population"], kind, a, b, by_side[a])


@pytest.mark.parametrize("bounds_name", list(BOUNDS))
def test_every_kind_is_present(bounds_name):
    want = {"frames": {"threshold", "threshold_second", "short_th", "tie_cell", "tie_cells", "occupied", "claimed", "shortlist", "capacity", "level",
                       "window_edge", "window_r0", "window_cells", "insert_round", "insert_last", "window_outside", "window_chunks",
                       "right_edge", "right_sign", "right_nan"},
            "loop2": {"threshold", "threshold_second", "short_th", "tie_cell", "tie_cells", "tie_windows", "occupied", "claimed", "shortlist",
                      "capacity", "level2"},
            "best": {"tie_cell", "tie_cells", "occupied", "level", "window_edge", "window_r0", "window_cells", "insert_round", "insert_last",
                     "window_outside", "window_chunks", "right_edge", "right_sign", "right_nan", "chi2_mono", "chi2_stereo", "chi2_branch"}}
    want["points"] = want["frames"] | {"ratio_edge", "ratio_levels", "ratio_second_hidden", "ratio_single"}
    for s in ("frames", "loop2", "best", "points"):
        w = world(s, bounds_name, 0.9 if s == "points" else 0.8)
        assert want[s] <= set(w["group_kind"].tolist()), want[s] - set(w["group_kind"].tolist())
    # the float / double pairs of the ratio test exist at 0.7 and 0.9 and nowhere else (25 per ratio within 1..256; those within TH_HIGH here)
    for r in sw.RATIOS:
        w = world("points", bounds_name, r)
        assert (w["float_double_ratio"] > 0) == (r in (0.7, 0.9)), (r, w["float_double_ratio"])
        assert ("ratio_float_double" in set(w["group_kind"].tolist())) == (r in (0.7, 0.9))
    assert len(sw.ratio_pairs(0.9, 256)[1]) == 25 and len(sw.ratio_pairs(0.7, 256)[1]) == 25
    assert world("best", bounds_name)["float_double_chi2"] > 0
    # rot * factor is exactly x.5 at some of the bin edges (15, 75, 135 among them): roundf and round-to-even part there
    assert world("frames", bounds_name, population="edges_a")["rot_half_exact"] >= 3
    for k in (0, 4):        # (75 * factor rounds to 2.5000002 in float; the float just below 75 is the one whose product is 2.5)
        assert f32(f32(15 + 30 * k) * f32(f32(1.0) / f32(30))) == f32(k + 0.5)
    if bounds_name == "round":                  # (k + 0.5 at insertion is exact only where invW is round)
        assert world("frames", bounds_name)["half_exact"] == 4
    assert world("frames", bounds_name)["cells_exact"] >= 2
    # histogram populations, from the oracle: which ballast bins survive
    def bins(pop):
        w = world("frames", bounds_name, population=pop)
        a = answers_of(w, oracle_run(w, True), oracle_run(w, False))
        b = [x for x in w["sides"] if x.startswith("bin")]
        return {s: set(a[w["sides"] == s]) for s in set(b)}, oracle_run(w, True)[0]
    assert bins("ten_one_one")[0] == {"bin2": {"a"}, "bin5": {"a"}, "bin8": {"a"}}              # 1 < 0.1f * 10 is false in float
    assert bins("eleven_one_one")[0] == {"bin2": {"a"}, "bin5": {"a/rejected"}, "bin8": {"a/rejected"}}
    assert bins("two_equal")[0] == {"bin2": {"a"}, "bin5": {"a"}, "bin8": {"a"}, "bin10": {"a/rejected"}}
    assert bins("three_equal")[0] == {"bin2": {"a"}, "bin5": {"a"}, "bin8": {"a"}, "bin10": {"a/rejected"}}
    assert bins("four_equal")[0] == {"bin2": {"a"}, "bin5": {"a"}, "bin8": {"a"}, "bin10": {"a/rejected"}}
    we = world("frames", bounds_name, population="empty")
    assert oracle_run(we, True)[0] == 0 and (oracle_run(we, True)[1] == -1).all()


@pytest.mark.parametrize("bounds_name", list(BOUNDS))
def test_the_restatement_equals_the_oracle_under_the_right_rules(bounds_name):
    for w in all_worlds(bounds_name):
        for gate in ((0, 1, 2) if w["search"] == "best" else (0,)):
            for ori in ((True, False) if w["search"] == "frames" else (True,)):
                e = oracle_run(w, ori, gate); g = model_run(w, RIGHT, ori, gate)
                if w["search"] == "best":
                    assert np.array_equal(g[0], e[0]) and np.array_equal(g[1], e[1]), (w["search"], gate)
                else:
                    assert g[0] == e[0] and np.array_equal(g[1], e[1]), (w["search"], w["population"], sw.kinds_of_differences(w, g[1], e[1]))


WRONG = [("th_lt", "frames", {}, 0, "threshold"), ("th_lt", "points", {}, 0, "threshold"), ("th_lt", "loop2", {}, 0, "threshold"),
         ("hist_rint", "frames", dict(population="edges_a"), 0, "rot_edge"),
         ("ratio_double", "points", dict(nnratio=0.9), 0, "ratio"), ("ratio_double", "points", dict(nnratio=0.7), 0, "ratio"),
         ("chi2_double", "best", {}, 2, "chi2"),
         ("right_ge", "frames", {}, 0, "right_edge"), ("right_ge", "points", {}, 0, "right_edge"), ("right_ge", "best", {}, 1, "right_edge"),
         ("window_le", "frames", {}, 0, "window_edge"), ("window_le", "points", {}, 0, "window_edge"), ("window_le", "best", {}, 0, "window_edge")]


@pytest.mark.parametrize("bounds_name", list(BOUNDS))
@pytest.mark.parametrize("rule,search,kw,gate,kind", WRONG, ids=lambda v: v if isinstance(v, str) else None)
def test_a_wrong_rule_is_seen_on_an_island_of_its_kind(bounds_name, rule, search, kw, gate, kind):
    w = world(search, bounds_name, **kw)
    e = answers_of(w, oracle_run(w, True, gate), oracle_run(w, False) if search == "frames" else None)
    g = answers_of(w, model_run(w, _rules(**{rule: True}), True, gate), model_run(w, _rules(**{rule: True}), False) if search == "frames" else None)
    differing = set(w["kinds"][np.flatnonzero(e != g)].tolist())
    assert kind in differing, (rule, search, differing)
    # ... and on no island of another kind: the rule changes that decision and nothing else
    also = {"hist_rint": {"rot_wrap"}, "th_lt": {"threshold_second", "shortlist"}, "window_le": {"window_r0"}}.get(rule, set())   # (the same compare)
    assert differing <= {kind} | also, differing


def test_round_to_even_at_insertion_is_seen_where_the_half_is_exact():
    w = world("frames", "round")
    e = answers_of(w, oracle_run(w, False)); g = answers_of(w, model_run(w, _rules(insert_rint=True), False))
    assert "insert_round" in set(w["kinds"][np.flatnonzero(e != g)].tolist())
    # the ratios whose float, double and exact compares agree everywhere cannot tell them apart: the double rule changes nothing there
    for r in (0.6, 0.75, 0.8):
        w = world("points", "round", r)
        assert np.array_equal(model_run(w, _rules(ratio_double=True))[1], oracle_run(w)[1])
