"""The model of Sim3Solver (tests/sim3_model.py) against the library's host routine (orbm_sim3_ransac_host: the statement sequence the
kernels share) byte for byte in both orders, against known answers, and the two orders against each other.  No device needed."""
import math

import numpy as np
import pytest

import multi_orb_slam_amd as m
from multi_orb_slam_amd._lib import ORB_E_ARG
import sim3_model as sm
import sim3_worlds as sw
from pose_model import poly_sincos

F = np.float32
NAMES = [name for name, _ in sw.worlds()]
WORLD = dict(sw.worlds())
ORDER = {"libm": m.SIM3_MATH_LIBM, "device": m.SIM3_MATH_DEVICE}

# Measured here on the CPU (the tests below print them; profiles/r11/notes_sim3.md).
SIM3_MARGIN = 4                  # the pose stage's POSE_MARGIN
ORDER_DIFF_ERR = 0.0             # the largest relative difference of any err between the two orders over all worlds
EIGEN_RESIDUAL = 2.8e-7          # |N q - lambda q| / max|N| of the Jacobi restatement against numpy.linalg.eigh's largest eigenvalue
EIGEN_VALUE = 3.1e-7             # |lambda_model - lambda_eigh| / max|N|
ATAN2_ULP = 6.0                  # the + - * / sqrt atan2 against math.atan2
SINCOS_ULP = 1.0                 # the polynomial sine / cosine against math.sin / math.cos on [0, 2 pi], in ulp of max(|value|, 2^-10)


def host(W, order, triples=None):
    (rec, masks), = m.sim3_ransac_host([sw.to_problem(m, W, triples)], order=ORDER[order])
    return rec, masks


def assert_same(got, want, what):
    rec, masks = got
    mrec, mmasks = want
    for k in mrec.dtype.names:
        assert rec[k].tobytes() == mrec[k].tobytes(), (what, k, np.nonzero((rec[k] != mrec[k]).reshape(len(rec), -1).any(axis=1))[0][:5])
    assert rec.tobytes() == mrec.tobytes(), what
    assert masks.shape == mmasks.shape and masks.tobytes() == mmasks.tobytes(), (what, "masks")


def test_record_layouts_are_the_abi_structs():
    assert m.SIM3_HYP_DTYPE == sm.HYP_DTYPE and m.SIM3_HYP_DTYPE.itemsize == 184 and m.SIM3_PROBLEM_DTYPE.itemsize == 84
    assert [m.SIM3_HYP_DTYPE.fields[k][1] for k in ("R12", "t12", "s12", "T12", "T21", "n_inliers")] == [0, 36, 48, 52, 116, 180]
    assert (m.SIM3_CAP, m.SIM3_MAX_ITS, m.SIM3_MAX_BATCH) == (sm.CAP, sm.MAX_ITS, sm.MAX_BATCH)


def test_the_worlds_meet_their_guard_band():
    pairs, closest = sw.check_conditions()
    nudged = sw.nudged()
    print("%d (hypothesis, correspondence) pairs, none within %.0e of a threshold (closest %.3e); %d pairs had to be nudged out of the band: %s"
          % (pairs, sw.GUARD, closest, sum(nudged.values()), {k: v for k, v in nudged.items() if v}))
    assert closest > sw.GUARD
    # the axes the worlds are meant to span
    ns = sorted(len(W["x3dc1"]) for W in WORLD.values())
    assert ns[0] <= 15 and 2000 in ns and ns[-1] > sm.CAP
    assert {True, False} == {W["fix_scale"] for W in WORLD.values()} and {0.7, 1.0, 1.4} <= {W["s_true"] for W in WORLD.values()}
    both = [(bool(W["cam1"].any()), bool(W["cam2"].any())) for W in WORLD.values()]
    assert {(False, False), (True, False), (False, True), (True, True)} <= set(both)
    for W in WORLD.values():
        if len(W["x3dc1"]) >= 100:
            assert set(W["octave"].reshape(-1)) == set(range(sw.N_LEVELS))


@pytest.mark.parametrize("name", NAMES)
def test_libm_order_equals_the_model(name):
    rec, masks, _, _ = sw.evaluate("libm")[name]
    assert_same(host(WORLD[name], "libm"), (rec, masks), name)


@pytest.mark.parametrize("name", NAMES)
def test_device_order_equals_the_models_device_mode(name):
    rec, masks, _, _ = sw.evaluate("device")[name]
    assert_same(host(WORLD[name], "device"), (rec, masks), name)


def test_a_batch_is_its_problems_one_by_one():
    names = ["n64_free_1.4", "n12_below_min", "n300_fixed_wide", "degenerate_and_repeated", "n65_fixed_wrong60", "n1000_free_1.0_wrong30"]
    for order in ("libm", "device"):
        got = m.sim3_ransac_host([sw.to_problem(m, WORLD[n]) for n in names], order=ORDER[order])
        for n, g in zip(names, got):
            rec, masks, _, _ = sw.evaluate(order)[n]
            assert_same(g, (rec, masks), n)
    # problems without correspondences or without hypotheses inside a batch
    W = WORLD["n64_free_1.4"]
    empty = m.Sim3Problem(W["K1"], W["K2"], np.zeros((0, 3)), np.zeros((0, 3)), [], [], [], [], np.zeros((0, 3)))
    no_hyp = sw.to_problem(m, W, triples=np.zeros((0, 3), np.int32))
    got = m.sim3_ransac_host([empty, sw.to_problem(m, W), no_hyp], order=m.SIM3_MATH_DEVICE)
    assert len(got[0][0]) == 0 and len(got[2][0]) == 0 and got[2][1].shape == (0, 1)
    rec, masks, _, _ = sw.evaluate("device")["n64_free_1.4"]
    assert_same(got[1], (rec, masks), "between two empty problems")


def test_hand_built_cases_end_where_they_should():
    for order in ("libm", "device"):
        ev = sw.evaluate(order)
        rec, masks, e1, e2 = ev["degenerate_and_repeated"]
        # coincident points with an exact centroid: everything that depends on the rotation is non-finite, nothing is an inlier
        h = 7
        assert WORLD["degenerate_and_repeated"]["triples"][h].tolist() == [14, 15, 16]
        assert np.isnan(rec["R12"][h]).all() and np.isnan(rec["t12"][h]).all() and np.isnan(rec["T12"][h][:12]).all()
        assert rec["n_inliers"][h] == 0 and not masks[h].any()
        assert rec["T12"][h][12:].tolist() == [0, 0, 0, 1]
        # the same triple again gives the same record; a permutation of it may differ in the last bits but not in what it finds
        assert rec[2].tobytes() == rec[3].tobytes() == rec[6].tobytes() and masks[2].tobytes() == masks[3].tobytes()
        assert rec["n_inliers"][5] == rec["n_inliers"][2] == 27      # (all but 14, 15, 16, which were set without regard to the Sim3)
        # collinear points leave the rotation about their line open: whatever comes out, host, model and device agree on it (above)
        rec, masks, _, _ = ev["rotation_zero"]
        nan = np.isnan(rec["R12"]).all(axis=1)
        assert nan.sum() >= 15 and not rec["n_inliers"][nan].any() and not masks[nan].any()
        rec, masks, _, _ = ev["rotation_pi"]
        best = int(np.argmax(rec["n_inliers"]))
        assert rec["n_inliers"][best] == 30
        assert np.abs(rec["R12"][best].reshape(3, 3) - np.diag([-1.0, -1.0, 1.0])).max() < 1e-5
        rec, masks, _, _ = ev["rotation_small"]
        assert rec["n_inliers"].max() == 30 and np.isfinite(rec["R12"]).all()
        rec, masks, e1, e2 = ev["depth_zero"]
        # correspondence 13 has z = 0 in keyframe 1: its own image position is not finite and it is never an inlier
        assert not np.isfinite(e1[:, 13]).any() and not ((masks[:, 0] >> np.uint64(13)) & np.uint64(1)).any()
        assert rec["n_inliers"].max() >= 27


def clean_triangle_altitude(X, tr):
    a, b, c = X[tr].astype(np.float64)
    area2 = np.linalg.norm(np.cross(b - a, c - a))
    return area2 / max(np.linalg.norm(b - a), np.linalg.norm(c - a), np.linalg.norm(c - b))


@pytest.mark.parametrize("name", ["n15_free_1.0", "n2000_free_0.7_clean"])
def test_a_noise_free_world_returns_its_sim3(name):
    """Tolerance: every coordinate of both clouds was rounded to float, an error of at most 2^-24 * max|X| each; the centroid, the
    difference to it and the products of M add one float rounding of that size each.  That is 4 half-ulps per cloud, 8 for the two
    = 4 * 2^-23 * max|X| of point error.  Three points fix a rotation through the triangle's smallest altitude h (the lever arm), with
    the error acting at both of its ends: 2 * 4 * 2^-23 * max|X| / h.  The scale is a ratio of the same lengths (same bound, relative),
    the translation is O1 - s R O2 with |O2| <= max|X| (the bound times max|X|, plus the roundings of its own sum, which it covers)."""
    W = WORLD[name]
    X1 = W["x3dc1"]
    mx = float(np.abs(X1).max())
    worst = 0.0
    for order in ("libm", "device"):
        rec, masks = host(W, order)
        assert (rec["n_inliers"] == len(X1)).all()                       # every hypothesis of a clean world explains every point
        for h, tr in enumerate(W["triples"]):
            tol = 8 * 2.0 ** -23 * mx / clean_triangle_altitude(X1, tr)
            dR = np.abs(rec["R12"][h].reshape(3, 3) - W["R_true"]).max()
            ds = abs(float(rec["s12"][h]) - W["s_true"]) / W["s_true"]
            dt = np.abs(rec["t12"][h] - W["t_true"]).max()
            worst = max(worst, dR / tol, ds / tol, dt / (tol * mx))
            assert dR <= tol and ds <= tol and dt <= tol * mx, (name, h, dR, ds, dt, tol)
            # T12 = [s R | t] and T21 is its inverse
            T12, T21 = rec["T12"][h].reshape(4, 4).astype(np.float64), rec["T21"][h].reshape(4, 4).astype(np.float64)
            assert np.abs(T12 @ T21 - np.eye(4)).max() < 1e-5
    print("%s: largest error / tolerance %.2f" % (name, worst))


def test_the_jacobi_restatement_is_an_eigen_solver():
    """The model's 4x4 decomposition against numpy.linalg.eigh on the N matrix of every hypothesis of every world (matrices below 1e-3
    are left out: the sweep's stop is ABSOLUTE, FLT_EPSILON, as in OpenCV, and below it nothing is rotated).  Four times the measured
    figures: the restatement is an eigen-solver; that it is OpenCV's is not claimed."""
    res = val = 0.0
    count = 0
    for name, W in sw.worlds():
        X1, X2 = W["x3dc1"], W["x3dc2"]
        for tr in W["triples"][::3]:
            N = sm.horn(X1[tr].T, X2[tr].T, W["fix_scale"], "libm")["N"]
            if not np.isfinite(N).all() or np.abs(N).max() < 1e-3:
                continue
            with np.errstate(all="ignore"):
                q, e, V = sm.cv_eigen_row0([[F(v) for v in row] for row in N])
            Nd, q = N.astype(np.float64), np.array(q, np.float64)
            lam = np.linalg.eigh(Nd)[0][-1]
            res = max(res, float(np.abs(Nd @ q - lam * q).max() / np.abs(Nd).max()))
            val = max(val, float(abs(float(max(e)) - lam) / np.abs(Nd).max()))
            assert abs(np.linalg.norm(q) - 1) < 1e-5
            count += 1
    print("%d matrices: residual %.3e, eigenvalue %.3e (of max|N|)" % (count, res, val))
    assert count > 1000 and res <= SIM3_MARGIN * EIGEN_RESIDUAL and val <= SIM3_MARGIN * EIGEN_VALUE


def ulps(a, b, floor=0.0):
    return abs(a - b) / float(np.spacing(max(abs(b), floor))) if (b != 0 or floor) else (0.0 if a == 0 else math.inf)


def test_the_device_atan2_stays_within_its_measured_ulp_of_the_c_library():
    rng = np.random.RandomState(3)
    worst = 0.0
    pts = []
    for th in np.concatenate([np.linspace(0, math.pi, 100001), rng.uniform(0, math.pi, 50000)]):
        for r in (1.0, 0.37):
            pts.append((max(r * math.sin(th), 0.0), r * math.cos(th)))
    pts += list(zip(rng.uniform(0, 1, 100000), rng.uniform(-1, 1, 100000)))
    pts += list(zip(10.0 ** rng.uniform(-12, 0, 50000), rng.uniform(-1, 1, 50000)))
    for y, x in pts:
        worst = max(worst, ulps(sm.atan2_device(y, x), math.atan2(y, x)))
    print("largest deviation of the + - * / sqrt atan2 from math.atan2 over %d points: %.1f ulp" % (len(pts), worst))
    assert worst <= ATAN2_ULP
    # the library's sequence is the model's, bit for bit; the corners
    for y, x in pts[::97] + [(0.0, 1.0), (0.0, -1.0), (1.0, 0.0), (0.0, 0.0), (1e-300, 1.0), (1.0, 1.0), (1.0, -1.0)]:
        assert m.sim3_atan2(y, x) == sm.atan2_device(y, x), (y, x)
    assert m.sim3_atan2(0.0, 1.0) == 0.0 and m.sim3_atan2(0.0, -1.0) == math.pi and m.sim3_atan2(1.0, 0.0) == math.pi / 2
    assert math.isnan(m.sim3_atan2(math.nan, 0.5)) and math.isnan(m.sim3_atan2(0.5, math.nan))


def test_the_device_sine_and_cosine_on_the_range_rodrigues_uses():
    """theta = the norm of the angle-axis vector = 2 * ang in [0, 2 pi].  Near its zeros a sine's last place is far below the last place
    of the rotation matrix it goes into (entries of size 1), so the unit is the ulp of max(|value|, 2^-10)."""
    rng = np.random.RandomState(4)
    worst = 0.0
    for x in np.concatenate([np.linspace(0, 2 * math.pi, 100001), rng.uniform(0, 2 * math.pi, 50000)]):
        s, c = poly_sincos(float(x))
        worst = max(worst, ulps(s, math.sin(x), 2.0 ** -10), ulps(c, math.cos(x), 2.0 ** -10))
    print("largest deviation of the polynomial sine / cosine on [0, 2 pi]: %.2f ulp" % worst)
    assert worst <= SINCOS_ULP
    for x in list(rng.uniform(0, 2 * math.pi, 2000)) + [0.0, math.pi, 2 * math.pi]:
        assert m.pose_sincos(float(x)) == poly_sincos(float(x)), x


def test_draw_triples_is_the_take_and_swap_procedure():
    # randi always 0: the first pick is 0, the back (N - 1) moves into its place and is picked next, then N - 2
    assert sm.draw_triples(10, 2, lambda n: 0).tolist() == [[0, 9, 8], [0, 9, 8]]
    # randi always the last position: the back itself, three times
    assert sm.draw_triples(10, 1, lambda n: n - 1).tolist() == [[9, 8, 7]]
    seq = iter([3, 3, 0])
    assert sm.draw_triples(6, 1, lambda n: next(seq)).tolist() == [[3, 5, 0]]
    for name, W in sw.worlds():
        t = W["triples"]
        n = len(W["x3dc1"])
        assert t.min() >= 0 and t.max() < n
        if name != "degenerate_and_repeated":
            assert (t[:, 0] != t[:, 1]).all() and (t[:, 0] != t[:, 2]).all() and (t[:, 1] != t[:, 2]).all()


def run_walk(counts, N, min_inliers, calls):
    """The library's walk and the model's transcription of `iterate` through the same sequence of calls."""
    it = sm.Iterate(counts, N, min_inliers, len(counts))
    start, state = 0, None
    for n in calls:
        want = it.iterate(n)
        found, no_more, start, best, best_index = m.sim3_walk(counts, N, min_inliers, start, n, state)
        state = (best, best_index)
        n_inliers = counts[found] if found >= 0 else 0
        assert (found, no_more, n_inliers) == want, (counts, calls, n)
        assert (start, best, best_index) == (it.mnIterations, it.mnBestInliers, it.best)
        yield found, no_more


def test_walk_is_the_iterate_loop():
    rng = np.random.RandomState(11)
    for trial in range(300):
        H = int(rng.randint(1, 60))
        min_inliers = int(rng.randint(3, 25))
        N = int(rng.randint(min_inliers - 2, 60))
        counts = rng.randint(0, max(N, 1) + 1, H).astype(np.int32)
        if trial % 3 == 0:
            counts = np.minimum(counts, min_inliers)               # never strictly above: runs to the end
        calls = [5] * int(rng.randint(1, 15)) + [H]                # iterate(5) ..., then find()
        list(run_walk(counts, N, min_inliers, calls))
    # the `>=`: a count equal to the best so far replaces it
    r = list(run_walk(np.array([7, 7, 3], np.int32), 30, 20, [3]))
    assert m.sim3_walk(np.array([7, 7, 3], np.int32), 30, 20, 0, 3)[4] == 1 and r == [(-1, True)]
    # the strict `>`: a count equal to min_inliers does not end the call, one above does
    assert list(run_walk(np.array([20, 20, 21, 30], np.int32), 30, 20, [5])) == [(2, False)]
    assert list(run_walk(np.array([20, 20, 20], np.int32), 30, 20, [2, 2])) == [(-1, False), (-1, True)]
    # N < min_inliers: the empty matrix and bNoMore at once; N == min_inliers runs (with nIterations = 1 from SetRansacParameters)
    assert list(run_walk(np.array([12] * 5, np.int32), 12, 20, [5])) == [(-1, True)]
    assert m.sim3_iterations(0.99, 20, 300, 20) == 1
    assert list(run_walk(np.array([20], np.int32), 20, 20, [5])) == [(-1, True)]
    # after a success the next call goes on behind it
    assert list(run_walk(np.array([25, 1, 26, 2], np.int32), 30, 20, [5, 5, 5])) == [(0, False), (2, False), (-1, True)]


def test_iterations_is_set_ransac_parameters():
    for N in list(range(15, 400)) + list(range(400, 5001, 7)):
        for prob, mi, mx in ((0.99, 20, 300), (0.99, 6, 300), (0.999, 15, 1000), (0.5, 20, 5)):
            assert m.sim3_iterations(prob, mi, mx, N) == sm.iterations(prob, mi, mx, N), (N, prob, mi, mx)
    # the formula itself, where nothing is special: ceil(log(1 - p) / log(1 - (min / N)^3))
    eps = float(F(20) / F(100))
    assert m.sim3_iterations(0.99, 20, 100000, 100) == math.ceil(math.log(1 - 0.99) / math.log(1 - eps ** 3))
    assert m.sim3_iterations(0.99, 20, 300, 100) == 300 and m.sim3_iterations(0.99, 20, 300, 25) == 7
    # N < min_inliers: log of a negative number, NaN -> INT_MIN -> 1; N = 0 likewise
    assert m.sim3_iterations(0.99, 20, 300, 12) == sm.iterations(0.99, 20, 300, 12) == 1
    assert m.sim3_iterations(0.99, 20, 300, 0) == sm.iterations(0.99, 20, 300, 0) == 1


def test_the_two_orders_against_each_other():
    a, b = sw.evaluate("libm"), sw.evaluate("device")
    d_err = dR = dt = ds = 0.0
    hyps = 0
    for name, W in sw.worlds():
        ra, ma, e1a, e2a = a[name]
        rb, mb, e1b, e2b = b[name]
        assert np.array_equal(ra["n_inliers"], rb["n_inliers"]) and ma.tobytes() == mb.tobytes(), name     # EVERY hypothesis: identical
        assert np.array_equal(np.isfinite(ra["T12"]), np.isfinite(rb["T12"])) and np.array_equal(np.isfinite(ra["T21"]), np.isfinite(rb["T21"])), name
        hyps += len(ra)
        with np.errstate(all="ignore"):
            # an err relative to the scale its test lives on: the err itself, or the threshold where it is below it
            for ea, eb, th in ((e1a, e1b, W["max_err1"]), (e2a, e2b, W["max_err2"])):
                rel = np.abs(ea.astype(np.float64) - eb.astype(np.float64)) / np.maximum(np.abs(ea.astype(np.float64)), th.astype(np.float64).reshape(1, -1))
                rel = rel[np.isfinite(rel)]
                if rel.size:
                    d_err = max(d_err, float(rel.max()))
            fin = np.isfinite(ra["T12"]).all(axis=1) & np.isfinite(rb["T12"]).all(axis=1)
            if fin.any():
                dR = max(dR, float(np.abs(ra["R12"][fin].astype(np.float64) - rb["R12"][fin]).max()))
                dt = max(dt, float(np.abs(ra["t12"][fin].astype(np.float64) - rb["t12"][fin]).max()))
                ds = max(ds, float(np.abs(ra["s12"][fin].astype(np.float64) - rb["s12"][fin]).max()))
    print("libm order against device order over %d hypotheses of %d worlds: err %.3e (relative), R %.3e, t %.3e, s %.3e" % (hyps, len(a), d_err, dR, dt, ds))
    assert d_err <= SIM3_MARGIN * ORDER_DIFF_ERR + 4.2e-5            # (the one-ulp bound of sim3_worlds.GUARD's derivation)
    assert SIM3_MARGIN * d_err <= sw.GUARD


def test_bad_arguments_are_refused():
    W = WORLD["n64_free_1.4"]
    with pytest.raises(m.OrbError):
        host(W, "libm", triples=np.array([[0, 1, 64]], np.int32))          # a position outside the problem
    with pytest.raises(m.OrbError):
        host(W, "libm", triples=np.array([[0, -1, 3]], np.int32))
    with pytest.raises(m.OrbError):
        m.sim3_ransac_host([sw.to_problem(m, W)], order=7)
    with pytest.raises(m.OrbError):
        m.sim3_ransac_host([sw.to_problem(m, W, triples=W["triples"][:1])] * (m.SIM3_MAX_BATCH + 1))
    with pytest.raises(m.OrbError):
        host(W, "libm", triples=np.zeros((m.SIM3_MAX_ITS + 1, 3), np.int32) + np.array([0, 1, 2], np.int32))


def test_the_limits_themselves_are_accepted():
    """The other side of every refusal above, on the smallest shapes (three correspondences, one-hypothesis problems): the checks are
    shared with PnP (ransac_validate, csrc/ransac_dev.h), and a `<` turned `<=` there fails here or above."""
    W = sw.generate(31, 3, s=1.0, noise=0.0, H=1)
    run = lambda triples, copies=1: m.sim3_ransac_host([sw.to_problem(m, W, np.asarray(triples, np.int32))] * copies)
    tile = lambda H: np.tile(np.array([0, 1, 2], np.int32), (H, 1))
    for refused in (lambda: run([[0, 1, 3]]), lambda: run([[0, 1, -1]])):    # position n and position -1 of the smallest problem
        with pytest.raises(m.OrbError) as e:
            refused()
        assert e.value.code == ORB_E_ARG
    (rec, masks), = run([[2, 1, 0]])                                         # position n - 1
    assert len(rec) == 1 and masks.shape == (1, 1) and np.isfinite(rec["T12"]).all()
    one, = run(tile(1))
    batch = run(tile(1), m.SIM3_MAX_BATCH)
    assert len(batch) == m.SIM3_MAX_BATCH
    assert all(got[0].tobytes() == one[0].tobytes() and got[1].tobytes() == one[1].tobytes() for got in batch)
    (rec, masks), = run(tile(m.SIM3_MAX_ITS))
    assert len(rec) == m.SIM3_MAX_ITS and masks.shape == (m.SIM3_MAX_ITS, 1)
    assert rec.tobytes() == one[0].tobytes() * m.SIM3_MAX_ITS and (masks == one[1][0, 0]).all()
