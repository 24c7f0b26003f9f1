"""The frame-assembly boundary worlds (tests/frame_boundary_worlds.py) on the CPU: the oracle held to the plain model on every world, byte
for byte; every group non-vacuous (both sides of its decision present, the exact ties counted); every wrong rule caught by the group
named for it, at the features that group marks and nowhere else."""
import numpy as np
import pytest

import frame_boundary_worlds as fw
import oracle
import test_oracle_undistort as undistort


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", fw.names())
def test_oracle_equals_model(name):
    w, M = fw.world(name), fw.expected(name)
    n = len(M["cell"])
    # UndistortKeyPoints
    ux, uy = oracle.undistort_points(w["calib"], M["kps"]["x"], M["kps"]["y"])
    assert u32(ux).tobytes() == u32(M["ux"]).tobytes() and u32(uy).tobytes() == u32(M["uy"]).tobytes()
    # ComputeStereoFromRGBD, camera after camera
    if w["depth"] is not None:
        cs = M["cam_start"]
        for c, k in enumerate(w["cams"]):
            ur, dp = oracle.stereo_from_depth(k, w["depth"], w["mbf"], M["ux"][cs[c]:cs[c + 1]])
            assert u32(ur).tobytes() == u32(M["uright"][cs[c]:cs[c + 1]]).tobytes(), c
            assert u32(dp).tobytes() == u32(M["depth"][cs[c]:cs[c + 1]]).tobytes(), c
    else:
        assert np.all(M["uright"] == -1) and np.all(M["depth"] == -1)
    # AssignFeaturesToGrid
    OF = oracle.FrameData(**fw.frame_data(w, M))
    ocs, oitems = oracle.grid_csr(OF)
    assert ocs.tobytes() == M["cell_start"].tobytes() and oitems.tobytes() == M["items"].tobytes()
    assert M["cell_start"][-1] == (M["cell"] >= 0).sum() and len(M["items"]) == M["cell_start"][-1] and n == M["cam_start"][-1]
    # GetFeaturesInArea around the marked features: the model's walk is the oracle's
    for label, idx in w["marks"].items():
        for g in idx[:6]:
            r = 1.3 * 10.0
            got = fw.features_in_area(w, M, int(M["cam"][g]), M["ux"][g], M["uy"][g], r)
            exp = oracle.features_in_area(OF, int(M["cam"][g]), float(M["ux"][g]), float(M["uy"][g]), r)
            assert np.array_equal(got, exp), (label, g)


def test_bounds_are_the_oracles():
    assert fw.MULTI_YAML == undistort.MULTI_YAML
    assert fw.BOUNDS["calibrated"]() == oracle.image_bounds(undistort.MULTI_YAML, 640, 480)
    b = fw.BOUNDS["calibrated"](); p = fw.BOUNDS["positive"]()
    assert b[0] < 0 and b[1] < 0 and p[0] > 0 and p[1] > 0
    assert float(fw.Grid(b).invW) != 0.1 and float(fw.Grid(fw.ROUND_BOUNDS).invW) == float(np.float32(0.1))


def test_the_issues_table():
    """the oracle on the round bounds: 5.0 rounds away from zero into column 1, -4.9 is still column 0, -5.0 and 640.0 are outside"""
    G = fw.Grid(fw.ROUND_BOUNDS)
    col = lambda v: int(G.index(np.float32(v), 0))
    assert col(5.0) == 1 and col(np.nextafter(np.float32(5), np.float32(0))) == 0 and col(-4.9) == 0 and col(-5.0) == -1
    assert col(np.nextafter(np.float32(635), np.float32(0))) == 63 and col(640.0) == 64
    xs = np.arange(640, dtype=np.float32); ys = np.arange(480, dtype=np.float32)
    px = G.pos(xs, 0); py = G.pos(ys, 1)
    assert int((px - np.floor(px) == 0.5).sum()) == 64 and int((py - np.floor(py) == 0.5).sum()) == 48


def test_every_group_has_both_sides(capsys):
    lines = []
    for group in fw.GROUPS:
        ns = fw.names(group)
        assert ns, group
        feats = sum(len(fw.expected(n)["cell"]) for n in ns)
        cases = sum(fw.world(n)["notes"].get("cases", 0) for n in ns)
        ties = sum(fw.world(n)["notes"].get("exact_ties", 0) for n in ns)
        lines.append("%-12s worlds %2d  features %6d  cases %3d  exact ties %2d" % (group, len(ns), feats, cases, ties))
    for b in fw.BOUNDS:
        w, M = fw.world("cell_round/" + b), fw.expected("cell_round/" + b)
        G = fw.Grid(w["bounds"])
        stay, move = w["marks"]["stay"], w["marks"]["move"]
        assert len(stay) == len(move) == w["notes"]["cases"] == 12
        # the pair of a case lies one ulp apart in one coordinate and in neighbouring cells (columns are 48 cells apart)
        pairs = 0
        for s in stay:
            for m in move:
                if M["cam"][s] == M["cam"][m] and M["cell"][m] - M["cell"][s] in (1, fw.ROWS) and \
                        (np.nextafter(M["ux"][s], np.float32(1e9)) == M["ux"][m] or np.nextafter(M["uy"][s], np.float32(1e9)) == M["uy"][m]):
                    pairs += 1
        assert pairs == 12
        cols = set(int(c) % fw.CELLS // fw.ROWS for c in M["cell"][np.concatenate([stay, move])])
        rows = set(int(c) % fw.ROWS for c in M["cell"][np.concatenate([stay, move])])
        assert set(fw.CELL_COLS) <= cols and set(fw.CELL_ROWS) <= rows
        lines.append("cell_round/%-10s exact ties %d of %d cases" % (b, w["notes"]["exact_ties"], w["notes"]["cases"]))
        if b == "round":
            assert w["notes"]["exact_ties"] == 12 and len(w["marks"]["tie"]) == 12
            assert np.all(M["cell"][w["marks"]["tie"]] == M["cell"][move])       # a tie moves on: away from zero
        w, M = fw.world("grid_exit/" + b), fw.expected("grid_exit/" + b)
        assert len(w["marks"]["in"]) == 6 and len(w["marks"]["out"]) == 6 and len(w["marks"]["below_min_in"]) == 2
        assert np.all(M["cell"][w["marks"]["in"]] >= 0) and np.all(M["cell"][w["marks"]["out"]] == -1)
        lines.append("grid_exit/%-10s exact ties %d (of 4 edges)" % (b, w["notes"]["exact_ties"]))
    for n in fw.names("depth_pick"):
        w, M = fw.world(n), fw.expected(n)
        assert len(w["marks"]["frac"]) == 20 and len(w["marks"]["last"]) == 6 and np.all(M["depth"] > 0)
        whole = w["marks"]["whole"]                                 # truncation: the five fractional neighbours of (u, v) read ITS pixel
        assert len(np.unique(M["depth"][whole])) == 4 and sorted(np.unique(M["depth"][w["marks"]["frac"]])) == sorted(M["depth"][whole])
    w, M = fw.world("depth_pick/k1"), fw.expected("depth_pick/k1")
    mv = w["marks"]["moved"]
    assert len(mv) >= 3 and np.all((M["ux"][mv].astype(int) != M["kps"]["x"][mv].astype(int)) | (M["uy"][mv].astype(int) != M["kps"]["y"][mv].astype(int)))
    lines.append("depth_pick/k1: %d keypoints whose distorted and undistorted pixels differ" % len(mv))
    w, M = fw.world("depth_value"), fw.expected("depth_value")
    pos, ref = w["marks"]["positive"], w["marks"]["refused"]
    assert len(pos) == 10 and len(ref) == 5 and w["notes"]["inexact_quotients"] >= 3
    assert np.all(M["depth"][ref] == -1) and np.all(M["uright"][ref] == -1) and np.all(M["depth"][pos] > 0)
    assert np.isneginf(M["uright"][pos]).sum() == 4 and not np.isnan(M["uright"]).any() and not np.isnan(M["depth"]).any()   # 40 / dv overflows for the denormals, FLT_MIN and 1e-38
    lines.append("depth_value: %d accepted, %d refused, %d inexact quotients, %d x -inf" % (len(pos), len(ref), w["notes"]["inexact_quotients"], 4))
    for n in fw.names("cameras"):
        w, M = fw.world(n), fw.expected(n)
        counts = w["notes"]["counts"]
        assert len(w["marks"]["first"]) == sum(1 for c in counts if c > 0) and len(np.unique(M["cell"])) == len(M["cell"])
    assert any(0 in fw.CAMERA_LAYOUTS[l][1:-1] for l in fw.CAMERA_LAYOUTS) and any(1 in fw.CAMERA_LAYOUTS[l] for l in fw.CAMERA_LAYOUTS)
    assert sorted(len(v) for v in fw.CAMERA_LAYOUTS.values()) == [1, 2, 2, 4, 4, 5, 32, 33, 64]
    fullest = sorted(int(np.diff(fw.expected(n)["cell_start"]).max()) for n in fw.names("occupancy"))
    assert fullest == [0, 1, 10, 64, 1025, 1025] and fw.expected("occupancy/all_outside")["cell_start"][-1] == 0
    assert np.all(np.diff(fw.expected("occupancy/every_cell")["cell_start"]) == 1)
    for t in fw.TOTALS:
        M = fw.expected("sizes/total_%d" % t)
        assert len(M["cell"]) == t and (t < 100 or 0.05 < (M["cell"] < 0).mean() < 0.15)
    for c in fw.CAMERA_SIZES:
        assert len(fw.world("sizes/camera_%d" % c)["cams"][1]) == c
    assert len(fw.expected("sizes/zero")["cell"]) == 0
    with capsys.disabled():
        print()
        for l in lines:
            print("frame boundary worlds: " + l)


# wrong rule -> (the group that must catch it, the marks at which it must show first and may show besides, the outputs in which it shows)
WRONG = {"round half to even": (dict(round="even"), "cell_round", ("tie",), ("cell",)),
         "truncate instead of round": (dict(round="trunc"), "cell_round", ("move",), ("cell",)),
         "x < minX before rounding": (dict(below_first=True), "grid_exit", ("below_min_in",), ("cell",)),
         "<= at 64 / 48": (dict(exit_le=True), "grid_exit", ("out",), ("cell",)),
         "round before the depth lookup": (dict(pick="round"), "depth_pick", ("frac", "last", "moved"), ("depth", "uright")),
         "depth at the undistorted pixel": (dict(depth_at="undistorted"), "depth_pick", ("moved", "frac", "last", "whole"), ("depth", "uright")),
         "dv >= 0": (dict(dv_ge=True), "depth_value", ("refused",), ("depth", "uright")),
         "denormals flushed": (dict(flush=True), "depth_value", ("positive",), ("depth", "uright")),
         "base + n off by one": (dict(cam_gt=True), "cameras", ("first",), ("cell",)),
         "items in arrival order": (dict(order="arrival"), "occupancy", ("full",), ("items",))}


@pytest.mark.parametrize("rule", list(WRONG))
def test_wrong_rule_is_caught_by_its_group(rule):
    change, group, labels, outputs = WRONG[rule]
    caught = 0
    for name in fw.names(group):
        w, M = fw.world(name), fw.expected(name)
        X = fw.model(w, dict(fw.RIGHT, **change))
        if not any(l in w["marks"] for l in labels):
            continue
        marked = np.concatenate([w["marks"][l] for l in labels if l in w["marks"]])
        for out in outputs:
            if out == "items":
                if X["items"].tobytes() != M["items"].tobytes():
                    # the same features in the same cells, another order inside the marked cells only
                    assert X["cell_start"].tobytes() == M["cell_start"].tobytes() and np.array_equal(np.sort(X["items"]), np.sort(M["items"]))
                    assert set(np.flatnonzero(X["items"] != M["items"])) <= set(np.flatnonzero(np.isin(M["items"], marked)))
                    caught += 1
                continue
            differ = np.flatnonzero(u32(X[out]) != u32(M[out])) if X[out].dtype == np.float32 else np.flatnonzero(X[out] != M[out])
            assert set(differ) <= set(marked), (rule, name, out)            # nothing but the group's own cases shows the rule
            caught += len(set(differ) & set(w["marks"][labels[0]])) > 0 if labels[0] in w["marks"] else 0
    assert caught > 0, "no world of %s tells `%s` from the reference's rule" % (group, rule)
