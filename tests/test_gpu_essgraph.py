"""GPU parity of the essential graph on the device (orbm_essential_graph: one lane per edge and evaluation, the blocks of the system over
the pairs that exist, the blocked LDL^T across workgroups, one synchronisation per Levenberg trial, the points corrected behind the last
iteration) with the library's host routine in DEVICE order -- byte for byte: every estimate, every float handed to SetPose and
SetWorldPos, the round record, the counts."""
import numpy as np
import pytest

import eg_worlds as ew

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher():
    import multi_orb_slam_amd as m
    mt = m.Matcher(0.8, True)
    yield mt
    mt.close()


def device_and_host(mt, W, iterations=20, path=0):
    import multi_orb_slam_amd as m
    P = ew.make_problem(m, W)
    dev = mt.essential_graph(P, iterations)
    last = mt.last_essential_graph()
    hst = m.essential_graph_host(P, iterations, m.POSE_ORDER_DEVICE)
    assert dev.same_bytes(hst) is None, (dev.same_bytes(hst), dev.round, hst.round)
    assert last[0] == path and last[3] == 0 and last[7] == 0
    if path == 0:
        # one synchronisation per Levenberg trial, plus the last one
        assert last[2] <= int(hst.round["trials"][0]) + 3 and last[1] > 0
        ends = np.concatenate([W["edge_v0"], W["edge_v1"]])
        na = len(np.unique(ends[ends < W["n_free"]]))
        assert last[5] == na * (na + 1) // 2 and na <= last[4] <= last[5] and last[6] == (7 * na + m.BA_PANEL - 1) // m.BA_PANEL
    else:
        assert last[1] == 0 and last[2] == 0
    return dev, last


# rows of the system: 7 (the smallest), 63 (one short of a panel), 70 (a block straddles the first panel boundary), 133 (two
# boundaries), 448 (full panels), 1050 (many panels)
@pytest.mark.parametrize("fix_scale", [False, True])
@pytest.mark.parametrize("n_free", [1, 9, 10, 19, 64, 150])
def test_device_equals_host_routine(matcher, n_free, fix_scale):
    W = ew.ring(n_free, 100 + n_free, fix_scale=fix_scale, n_points=50)
    R, last = device_and_host(matcher, W, 20 if n_free < 100 else 3)      # (the host routine's dense solver is sequential)
    assert R.optimised == 1 and R.round["iterations"][0] >= 1 and last[6] == (7 * n_free + 63) // 64


def test_duplicate_pairs_and_a_fixed_vertex_in_both_roles(matcher):
    W = ew.ring(12, 77, n_points=20, doubles=6)
    pairs = [(min(a, b), max(a, b)) for a, b in zip(W["edge_v0"], W["edge_v1"])]
    assert len(set(pairs)) < len(pairs)
    fixed = W["n_free"]
    assert (W["edge_v0"] == fixed).any() and (W["edge_v1"] == fixed).any()
    device_and_host(matcher, W)


CASES = ew.hand_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_built_cases(matcher, name):
    W, iterations = CASES[name]
    device_and_host(matcher, W, iterations, path=2 if name == "no_edges" else 0)


@pytest.mark.parametrize("n_points", [0, 1, 10000])
def test_points_are_corrected_on_the_device(matcher, n_points):
    W = ew.ring(10, 31, n_points=n_points, unreferenced=0.2)
    assert n_points < 2 or ((W["point_ref"] == -1).any() and (W["point_ref"] >= 0).any())
    R, _ = device_and_host(matcher, W, 4)
    assert R.point_f.shape == (n_points, 3)
    if n_points > 1:
        moved = np.abs(R.point_f - W["points"]).max(axis=1) > 0
        assert moved[W["point_ref"] >= 0].any() and not moved[W["point_ref"] < 0].any()


def test_the_path_report_on_a_ring_of_forty(matcher):
    W = ew.ring(40, 140, n_points=10)
    R, last = device_and_host(matcher, W)
    assert last[2] <= int(R.round["trials"][0]) + 3
    assert last[4] < last[5]                       # block pairs computed < all pairs


def test_the_same_call_twice_with_other_calls_in_between(matcher):
    import multi_orb_slam_amd as m
    import frustum_worlds as fw
    W = ew.ring(64, 164, n_points=300)
    a, _ = device_and_host(matcher, W, 6)
    device_and_host(matcher, ew.ring(10, 110, n_points=5), 6)                    # (the buffers are reused by a smaller call in between)
    w = fw.make_world(2000, [1000, 500], 640, 480, 2, 3.0)                       # ... and by an unrelated search
    F = matcher.frame(m.FrameData(**w["fr"]))
    with m.LocalPoints(matcher, len(w["points"])) as pts:
        pts.write(0, w["points"])
        _, nmatches, _, _ = matcher.SearchLocalPoints(F, pts, w["view"].native())
        assert nmatches > 100
        b, _ = device_and_host(matcher, W, 6)
    F.close()
    assert a.same_bytes(b) is None


def test_a_problem_past_the_cap_reports_the_host_path(matcher):
    import multi_orb_slam_amd as m
    W = ew.ring(30, 91, n_points=10)
    extra = m.EG_MAX_FREE + 1 - 30                                               # edgeless free vertices: the dense solver stays small
    ident = np.array([[0., 0., 0., 1., 0., 0., 0., 1.]] * extra)
    V = np.concatenate([W["vertex"][:30], ident, W["vertex"][30:]])
    shift = lambda a: np.where(a >= 30, a + extra, a).astype(np.int32)
    W = dict(W, n_free=m.EG_MAX_FREE + 1, vertex=V, edge_v0=shift(W["edge_v0"]), edge_v1=shift(W["edge_v1"]), point_ref=shift(W["point_ref"]))
    R, _ = device_and_host(matcher, W, 5, path=1)
    assert R.active_vertices == 31 and R.optimised == 1
