"""The global bundle adjustment on the CPU: the library's host routine (orbm_bundle_adjust_host) against the NumPy model written from
the g2o sources (tests/gba_model.py) -- byte for byte, in both orders, on seeded trajectory worlds, hand-built cases and stop cases --
and what holds the solver of the reduced system (orbm_ba_ldlt): it solves, it is the local BA's factorisation, and its backward
substitution really runs in descending order."""
import numpy as np
import pytest

import multi_orb_slam_amd as m
import gba_model as gm
import gba_worlds as gw
import lba_model as lm

ORDERS = {"index": m.POSE_ORDER_INDEX, "device": m.POSE_ORDER_DEVICE}
# (world, iterations, robust): 1 / 7 / 20 free poses, the kernels on and off, 5 / 10 / 20 iterations
CASES = [("f1_p30_stereo", 5, True), ("f1_p30_stereo", 10, False), ("f7_p150_mixed_wrong10", 10, True), ("f7_p150_mixed_wrong10", 20, False),
         ("f7_p120_mono_one_camera", 5, False), ("f7_p120_mono_one_camera", 20, True), ("f20_p300_mixed_wrong10", 10, False),
         ("f20_p300_mixed_wrong10", 5, True)]
_runs = {}


def same(H, M, what):
    for k in gm.Result.FIELDS:
        a, b = getattr(H, k), getattr(M, k)
        if isinstance(a, np.ndarray):
            b = np.asarray(b)
            assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
            assert a.tobytes() == b.tobytes(), (what, k, int((a != b).sum()) if a.dtype.names is None else (a, b))
        else:
            assert a == b, (what, k, a, b)


def both(W, iterations, robust, order, stop=None, key=None):
    if key is not None and (key, order) in _runs:
        return _runs[(key, order)]
    H = m.bundle_adjust_host(gw.to_problem(m, W), iterations, robust, ORDERS[order], stop=stop)
    M = gm.optimize(W, iterations, robust, order, stop=stop)
    if key is not None:
        _runs[(key, order)] = (H, M)
    return H, M


def chi2_before_and_after(W, H, robust):
    G = lm.Graph(W)
    p0, x0 = gm.start(G, W)
    return gm.chi2_at(W, p0, x0, robust), gm.chi2_at(W, H.pose, H.point, robust)


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%d-%s" % (c[0], c[1], "robust" if c[2] else "plain"))
def test_host_routine_equals_the_model_byte_for_byte(case, order):
    name, iterations, robust = case
    W = gw.world(name)
    H, M = both(W, iterations, robust, order, key=case)
    same(H, M, (case, order))
    assert M.trace.solve_failed == 0, "a seeded world must not fail a solve"
    f = gw.WORLDS[name][0]
    assert H.optimised == 1 and H.active_poses == f and H.polls == 0 and 1 <= H.round["iterations"][0] <= iterations
    assert H.active_edges == len(W["edge_pose"]) and np.array_equal(H.Tcw[f:], W["Tcw"][f:])       # keyframe 0 stays
    before, after = chi2_before_and_after(W, H, robust)
    assert after <= before and after < 0.9 * before, (before, after)


def test_the_cases_cover_what_they_are_meant_to():
    assert {gw.WORLDS[c[0]][0] for c in CASES} == {1, 7, 20} and {c[1] for c in CASES} == {5, 10, 20} and {c[2] for c in CASES} == {True, False}
    assert {gw.WORLDS[c[0]][3] for c in CASES} == {"mono", "stereo", "mixed"} and {gw.WORLDS[c[0]][4] for c in CASES} == {0.0, 0.1}
    W = gw.world("f20_p300_mixed_wrong10")
    assert set(np.unique(W["edge_cam"])) == {0, 1} and set(np.unique(gw.world("f7_p120_mono_one_camera")["edge_cam"])) == {0}
    # most pose pairs share nothing
    G = lm.Graph(W)
    share = np.zeros((21, 21), bool)
    for l in range(G.n_points):
        ps = G.edge_pose[G.first[l]:G.first[l + 1]]
        share[np.ix_(ps, ps)] = True
    assert share[:20, :20].sum() < 0.5 * 400 and np.diff(W["first"]).max() <= 5


@pytest.mark.parametrize("case", [c for c in CASES if c[1] == 10], ids=lambda c: c[0])
def test_the_two_orders_agree_on_every_counter(case, capsys):
    name, iterations, robust = case
    (Hi, _), (Hd, _) = both(gw.world(name), iterations, robust, "index", key=case), both(gw.world(name), iterations, robust, "device", key=case)
    for k in ("optimised", "polls", "active_poses", "active_points", "active_edges"):
        assert getattr(Hi, k) == getattr(Hd, k), k
    assert Hi.round["iterations"][0] == Hd.round["iterations"][0] and Hi.round["trials"][0] == Hd.round["trials"][0]
    with capsys.disabled():
        print("\n[gba] %s: largest pose difference between the orders %.3g, largest point difference %.3g"
              % (name, float(np.abs(Hi.pose - Hd.pose).max()), float(np.abs(Hi.point - Hd.point).max())))


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("name", list(gw.hand_cases()))
def test_hand_built_cases(name, order):
    W, robust, expect = gw.hand_cases()[name]
    H, M = both(W, 10, robust, order, stop=10 ** 9)
    same(H, M, (name, order))
    assert expect(H), name
    if name in ("zero_pivot", "non_finite_pivot_at_a_pose"):
        assert M.trace.solve_failed >= 1 and all(not t[4] for t in M.trace.trials)
        assert np.array_equal(H.point_f, W["points"])                      # x was never written: nothing moved
    else:
        assert M.trace.solve_failed == 0
        before, after = chi2_before_and_after(W, H, robust)
        assert after <= before, (name, before, after)
    if name == "zero_pivot":
        assert "qmax" in M.trace.exits
    if name == "no_fixed_pose":
        assert len(W["Tcw"]) == W["n_free"]


@pytest.mark.parametrize("name", list(gw.stop_cases()))
def test_stop_cases(name):
    W, iterations, robust, n, exit_, polls = gw.stop_cases()[name]
    for order in ORDERS:
        H, M = both(W, iterations, robust, order, stop=n)
        same(H, M, (name, order))
        assert H.polls == polls and exit_ in M.trace.exits, (H.polls, M.trace.exits)
    if name == "at_poll_1":
        assert H.optimised == 1 and H.round["iterations"][0] == 0 and np.array_equal(H.point_f, W["points"])
    if name == "at_the_head_of_iteration_2":
        assert H.round["iterations"][0] == 1 and not np.array_equal(H.point_f, W["points"])      # the estimates reached so far
    if name == "inside_a_trial_loop":
        assert H.round["iterations"][0] == 1 and H.round["trials"][0] == 3


def test_zero_iterations_poll_nothing_and_move_nothing():
    W = gw.world("f7_p150_mixed_wrong10")
    for order in ORDERS:
        H, M = both(W, 0, True, order, stop=0)
        same(H, M, order)
        assert H.polls == 0 and H.optimised == 1 and np.array_equal(H.point_f, W["points"])


def test_bad_points_are_ignored():
    W = dict(gw.world("f7_p150_mixed_wrong10"))
    a = m.bundle_adjust_host(gw.to_problem(m, W), 5, False)
    W["bad"] = np.ones(len(W["points"]), np.uint8)
    b = m.bundle_adjust_host(gw.to_problem(m, W), 5, False)
    assert a.same_bytes(b) is None


# ---- the solver of the reduced system ----------------------------------------------------------------------------------------------------
def spd(n, cond, seed):
    """Q diag Q^T with a known spectrum: eigenvalues log-spaced from 1 to cond."""
    rng = np.random.RandomState(seed)
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    H = (Q * np.logspace(0, np.log10(cond), n)) @ Q.T
    return (H + H.T) / 2, rng.normal(size=n)


@pytest.mark.parametrize("n", [6, 66, 390])
def test_ba_ldlt_solves_within_the_backward_error_bound(n):
    """A backward-stable solve of H x = b is off the exact x by at most c(n) eps cond2(H) |x|; elimination without pivoting on a
    positive definite matrix has no growth, c(n) = 8 n covers it.  NumPy's Cholesky solve is held to the same bound first: if the bound
    were too tight for a stable method it would show there."""
    eps = np.finfo(np.float64).eps
    for cond in (1e2, 1e6):
        H, b = spd(n, cond, 300 + n)
        c2 = np.linalg.cond(H, 2)
        want = np.linalg.solve(H, b)
        bound = 8 * n * eps * c2
        Lc = np.linalg.cholesky(H)
        xc = np.linalg.solve(Lc.T, np.linalg.solve(Lc, b))
        ec = np.linalg.norm(xc - want) / np.linalg.norm(want)
        x = m.ba_ldlt(H, b)
        assert x is not None
        e = np.linalg.norm(x - want) / np.linalg.norm(want)
        print("[gba] ba_ldlt n = %d cond2 = %.3g: relative error %.3g (Cholesky by NumPy %.3g), bound %.3g" % (n, c2, e, ec, bound))
        assert ec <= bound and e <= bound
        if n <= 66:
            assert x.tobytes() == gm.ba_ldlt(H, b).tobytes()


def test_ba_ldlt_is_the_local_factorisation_with_a_descending_backward_substitution():
    rng = np.random.RandomState(5)
    for n in (1, 2):                             # at most one term per row: the order cannot matter
        for _ in range(20):
            A = rng.uniform(-1, 1, (n, n)); H = A @ A.T + np.eye(n); b = rng.uniform(-1, 1, n)
            assert m.ba_ldlt(H, b).tobytes() == m.lba_ldlt(H, b).tobytes()
    H, b = spd(66, 1e4, 77)
    x, xl, xm = m.ba_ldlt(H, b), m.lba_ldlt(H, b), gm.ba_ldlt(H, b)
    assert x.tobytes() == xm.tobytes() and lm.ldlt_solve(H, b).tobytes() == xl.tobytes()
    assert x[65] == xl[65] and x[64] == xl[64]   # rows with no or one term
    assert (x != xl).any(), "the two backward substitutions must differ somewhere in 66 rows"
    assert np.abs(x - xl).max() <= 1e-9 * np.abs(x).max()


def test_a_zero_or_non_finite_pivot_fails_the_factorisation_and_leaves_x():
    for H in (np.diag([2.0, 0.0, 3.0]), np.array([[4.0, 2.0], [2.0, 1.0]]), np.array([[4.0, 2.0], [2.0, np.inf]]), np.array([[4.0, 2.0], [2.0, np.nan]])):
        assert m.ba_ldlt(H, np.ones(len(H))) is None and gm.ba_ldlt(H, np.ones(len(H))) is None
    H = np.array([[1.0, 2.0], [2.0, 1.0]])        # indefinite, non-zero pivots: 1, -3
    x = m.ba_ldlt(H, np.array([1.0, 0.0]))
    assert x is not None and np.allclose(H @ x, [1.0, 0.0])
    assert m.ba_ldlt(np.zeros((0, 0)), np.zeros(0)) is not None
