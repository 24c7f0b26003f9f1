"""CPU tests of the Sim3 refinement (Optimizer::OptimizeSim3_cam1): the model of tests/sim3opt_model.py, written from the reference's
and g2o's sources, against the library's host routine orbm_sim3_optimize_host -- byte for byte, in both orders, every field of the
result record and every flag -- and the properties of the model itself: it finds the truth, its numeric Jacobian is a derivative, its
LDLT solves, the four traps of the sources change bytes when they are tidied away.  No device is needed."""
import math

import numpy as np
import pytest

import multi_orb_slam_amd as m
import sim3opt_model as sm
import sim3opt_worlds as sw
from pose_model import poly_sincos

NAMES = list(sw.WORLDS)
ORDERS = (("index", m.POSE_ORDER_INDEX), ("device", m.POSE_ORDER_DEVICE))
_EVAL = {}


def host(W, order):
    return m.sim3_optimize_host([sw.to_problem(m, W)], order)[0]


def evaluate(name, W=None):
    """model and host routine of a world in both orders, once per process -> {order name: (model rec, model flags, trace, host rec, host flags)}"""
    if name not in _EVAL:
        W = W if W is not None else sw.world(name)
        out = {}
        for on, oc in ORDERS:
            tr = sm.Trace()
            mrec, mflags = sm.optimize(W, on, tr)
            hrec, hflags = host(W, oc)
            out[on] = (mrec, mflags, tr, hrec, hflags)
        _EVAL[name] = out
    return _EVAL[name]


def assert_same(mrec, mflags, hrec, hflags, what):
    for k in hrec.dtype.names:
        assert hrec[k].tobytes() == mrec[k].tobytes(), (what, k, hrec[k], mrec[k])
    assert hrec.tobytes() == mrec.tobytes(), what
    assert np.array_equal(hflags, mflags), (what, "flags", int((hflags != mflags).sum()))


def test_the_record_layouts_agree():
    assert sm.RESULT_DTYPE == m.SIM3OPT_RESULT_DTYPE and m.SIM3OPT_RESULT_DTYPE.itemsize == 136 and m.SIM3OPT_PROBLEM_DTYPE.itemsize == 356
    assert 15 <= min(w[1] for w in sw.WORLDS.values()) and max(w[1] for w in sw.WORLDS.values()) > m.SIM3OPT_CAP and len(sw.WORLDS) >= 20


@pytest.mark.parametrize("name", NAMES)
def test_the_model_equals_the_host_routine_byte_for_byte_in_both_orders(name):
    ev = evaluate(name)
    for on, _ in ORDERS:
        mrec, mflags, tr, hrec, hflags = ev[on]
        assert_same(mrec, mflags, hrec, hflags, (name, on))
        assert hrec["n_correspondences"] == sw.world(name)["n"] and hrec["optimisations"] == 2 and hrec["written"] == 1


@pytest.mark.parametrize("name", NAMES)
def test_the_guard_band_holds_and_the_two_orders_agree_on_every_flag_and_return_value(name):
    """The band is a property of the inputs (sim3opt_worlds.GUARD); inside it the two orders could legitimately part."""
    ev = evaluate(name)
    for on, _ in ORDERS:
        tr = ev[on][2]
        assert len(tr.margins) == 2
        assert min(float(mg.min()) for mg in tr.margins) > sw.GUARD, (name, on)
    (ri, fi), (rd, fd) = ev["index"][3:5], ev["device"][3:5]
    assert np.array_equal(fi, fd)
    for k in ("n_inliers", "n_correspondences", "n_bad", "n_more_iterations", "written", "optimisations"):
        assert ri[k] == rd[k], (name, k)


def order_difference(ri, rd):
    """largest |difference| over the quaternion (either sign), the translation relative to its size, the scale relative to itself"""
    dq = float(min(np.abs(ri["q"] - rd["q"]).max(), np.abs(ri["q"] + rd["q"]).max()))
    dt = float(np.abs(ri["t"] - rd["t"]).max() / max(1.0, np.abs(ri["t"]).max()))
    ds = abs(float(ri["s"]) - float(rd["s"])) / float(ri["s"])
    return dq, dt, ds


def test_the_difference_of_the_two_orders_is_measured():
    """Measured, not fixed in advance: the orders differ by the summation tree and by a few ulp in sin, cos and exp, and the numeric
    Jacobian (differences of errors at 1e-9, rounded near 1e-13) amplifies that at every linearisation."""
    worst = (0.0, 0.0, 0.0)
    for name in NAMES:
        ev = evaluate(name)
        d = order_difference(ev["index"][3], ev["device"][3])
        print("%-34s q %.3e  t %.3e  s %.3e" % ((name,) + d))
        worst = tuple(max(a, b) for a, b in zip(worst, d))
    print("largest difference between the two orders: quaternion %.3e, translation %.3e (relative), scale %.3e (relative)" % worst)
    assert all(math.isfinite(v) for v in worst)


# ---- the hand-built exits -------------------------------------------------------------------------------------------------------------
CASES = sw.exit_cases()


@pytest.mark.parametrize("name", list(CASES))
def test_hand_built_exits(name):
    W, expect = CASES[name]
    ev = evaluate("exit/" + name, W)
    for on, _ in ORDERS:
        mrec, mflags, tr, hrec, hflags = ev[on]
        assert_same(mrec, mflags, hrec, hflags, (name, on))
        for k, v in expect.items():
            assert hrec[k] == v, (name, on, k, hrec[k], v)
        assert ("early_return" in tr.branches) == (hrec["written"] == 0)
        assert ("n_more_10" in tr.branches) == (hrec["n_bad"] > 0) and hrec["n_more_iterations"] == (10 if hrec["n_bad"] > 0 else 5)
        assert int((hflags == 1).sum()) == hrec["n_bad"]
        if hrec["written"]:
            assert hrec["n_inliers"] == W["n"] - hrec["n_bad"] - int((hflags == 2).sum())
        else:
            assert not (hflags == 2).any()


def test_the_early_return_keeps_its_removals_and_leaves_the_sim3_alone():
    """9 survivors of 14: the first optimisation has run and moved the vertex, its removals are flagged, and the record carries the
    START, converted as g2o::Sim3(Matrix3d, Vector3d, double) converts it, not the vertex."""
    W, _ = CASES["survivors_9"]
    for on, oc in ORDERS:
        rec, flags = host(W, oc)
        assert rec["n_inliers"] == 0 and rec["written"] == 0 and rec["optimisations"] == 1 and rec["round"][0]["iterations"] > 0
        assert list(flags) == [0] * 9 + [1] * 5
        start = sm.Sim3.from_matrix([[float(v) for v in row] for row in W["R"].reshape(3, 3)], [float(v) for v in W["t"]], float(W["s"]))
        assert list(rec["q"]) == start.q and list(rec["t"]) == start.t and rec["s"] == start.s
        moved, _ = sm.optimize(W, on, rules=("write_on_early_return",))
        assert moved["s"] != rec["s"]                                  # the vertex did move
    # one either side of `nCorrespondences - nBad < 10`
    assert host(CASES["survivors_10"][0], m.POSE_ORDER_INDEX)[0]["n_inliers"] == 10
    assert host(CASES["survivors_11"][0], m.POSE_ORDER_INDEX)[0]["n_inliers"] == 11


def test_every_branch_of_the_exponential_is_reached_inside_an_optimisation():
    seen = set()
    for name in CASES:
        for on, _ in ORDERS:
            seen |= evaluate("exit/" + name, CASES[name][0])[on][2].branches
    assert {"sim3_exp_0", "sim3_exp_1", "sim3_exp_2", "sim3_exp_3"} <= seen, seen
    assert {"early_return", "nothing_active", "rejected_trial", "n_more_5", "n_more_10"} <= seen, seen


@pytest.mark.parametrize("on,oc", ORDERS)
def test_the_exponential_map_of_the_library_is_the_models_in_all_four_branches(on, oc):
    rng = np.random.RandomState(5)
    count = [0, 0, 0, 0]
    for omega, sigma in ((1e-9, 0.0), (1e-9, 1e-9), (0.3, 0.0), (0.3, 5e-6), (4e-6, 0.2), (0.0, -0.4), (0.3, 0.2), (2.5, -0.7), (1e-4, 1e-4)):
        for _ in range(20):
            w = rng.randn(3)
            w = w / np.linalg.norm(w) * omega
            u = [float(v) for v in w] + [float(v) for v in rng.randn(3)] + [sigma]
            q, t, s, branch = m.sim3opt_expmap(u, oc)
            T, mbranch = sm.Sim3.exp(list(u), on)
            assert branch == mbranch and list(q) == T.q and list(t) == T.t and s == T.s, (u, on)
            count[branch] += 1
    assert min(count) >= 20, count


def test_a_fixed_scale_perturbs_dimension_6_by_nothing():
    """Under _fix_scale dimension 6 perturbs by Sim3(0): it reproduces the estimate exactly, and column 6 of every Jacobian is exactly 0."""
    fixed = [n for n in NAMES if sw.world(n)["fix_scale"]]
    assert len(fixed) >= 5
    for name in fixed:
        for on, _ in ORDERS:
            mrec, _, tr, hrec, _ = evaluate(name)[on]
            assert tr.fixed_scale_exact and tr.col6 and max(tr.col6) == 0.0, (name, on)
            assert hrec["s"] == 1.0
    free = evaluate("n40_free14_clean_off")["index"][2]
    assert min(free.col6) > 0.0
    for on, oc in ORDERS:
        q, t, s, branch = m.sim3opt_expmap([0.0] * 7, oc)
        assert list(q) == [0.0, 0.0, 0.0, 1.0] and list(t) == [0.0, 0.0, 0.0] and s == 1.0 and branch == 0


# ---- the four traps: the tidy alternative produces different bytes ----------------------------------------------------------------------
def differs(W, rule, order="index"):
    a, fa = sm.optimize(W, order)
    b, fb = sm.optimize(W, order, rules=(rule,))
    return a.tobytes() != b.tobytes() or not np.array_equal(fa, fb)


def test_a_normalising_product_changes_bytes():
    assert differs(sw.world("n40_free14_clean_off"), "normalising_mul") and differs(sw.world("n65_fixed_clean_near"), "normalising_mul")


def test_carrying_lambda_into_the_second_optimisation_changes_bytes():
    assert differs(sw.world("n24_free07_wrong20"), "carry_lambda") and differs(sw.world("n100_fixed_wrong50"), "carry_lambda")


def test_writing_the_sim3_back_on_the_early_return_changes_bytes():
    assert differs(CASES["survivors_9"][0], "write_on_early_return") and differs(CASES["nine_clean"][0], "write_on_early_return")
    assert not differs(CASES["survivors_10"][0], "write_on_early_return")


def stale_world():
    """Where the stale read matters.  An optimisation ends on a rejected trial only when rho is not negative (a step below the
    rounding of the errors) or after ten rejections (a step damped by 2^55), so the errors of the last computeActiveErrors and those at
    the accepted estimate agree to about 1e-12 of a chi2 -- measured over these worlds -- and no float32 observation can be placed
    between them.  They part when a trial is NOT A NUMBER: one point of keyframe 2 that the start (the identity) puts exactly on the
    principal plane of camera 1 projects to infinity, its numeric Jacobian is inf - inf, H, the step and the trial estimate are NaN,
    rho is NaN, the trial is rejected and the iteration ends on it.  Every chi2 the test then reads is NaN and compares false: nothing
    is removed, where a classification at the (finite, unchanged) estimate removes what lies off."""
    rng = np.random.RandomState(71)
    n = 30
    z = rng.uniform(2.0, 9.0, n)
    X1 = np.stack([rng.uniform(-0.5, 0.5, n) * z, rng.uniform(-0.4, 0.4, n) * z, z], axis=1)
    R, t = sw.rot([0.3, 1.0, -0.2], 0.012), np.array([0.03, -0.01, 0.02])
    X2 = (X1 - t) @ R                                      # X1 = R X2 + t
    X2[7] = (0.4, -0.3, 0.0)
    X1, X2 = X1.astype(np.float32), X2.astype(np.float32)
    seen2 = X2.astype(np.float64)
    seen2[7, 2] = 4.0                                      # (its observation in keyframe 2 is an ordinary, finite pixel)
    sig = sw.inv_level_sigma2()
    return dict(K1=sw.K1, K2=sw.K2, inv_level_sigma2_1=sig, inv_level_sigma2_2=sig, R=np.eye(3, dtype=np.float32).reshape(9),
                t=np.zeros(3, np.float32), s=np.float32(1), th2=np.float32(sw.TH2), fix_scale=True, x3dc1=X1, x3dc2=X2,
                obs1=sw.project(sw.K1, X1.astype(np.float64)).astype(np.float32), obs2=sw.project(sw.K2, seen2).astype(np.float32),
                octave1=np.zeros(n, np.int32), octave2=np.zeros(n, np.int32), n=n)


def test_classifying_at_the_accepted_estimate_changes_bytes():
    W = stale_world()
    tr = sm.Trace()
    rec, flags = sm.optimize(W, "index", tr)
    assert "ended_on_rejected_trial" in tr.branches and np.isnan(tr.class_chi[0][0]).all()
    assert rec["n_bad"] == 0 and rec["n_inliers"] == W["n"] and rec["written"] == 1 and not flags.any()
    assert list(rec["q"]) == [0.0, 0.0, 0.0, 1.0] and rec["s"] == 1.0       # the vertex never moved
    hrec, hflags = host(W, m.POSE_ORDER_INDEX)
    assert_same(rec, flags, hrec, hflags, "stale")
    tidy, tflags = sm.optimize(W, "index", rules=("classify_at_estimate",))
    assert tidy["n_bad"] > 0 and (tflags == 1).sum() == tidy["n_bad"]
    assert differs(W, "classify_at_estimate")


# ---- one boundary pair per edge type ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on,oc", ORDERS)
@pytest.mark.parametrize("edge", ["12", "21"])
def test_boundary_pairs_flip_exactly_one_flag(edge, on, oc):
    kept, removed = sw.host_boundary_pair(m, edge, 5, oc)
    key = "obs1" if edge == "12" else "obs2"
    a, b = kept[key][5, 0], removed[key][5, 0]
    assert a != b and np.nextafter(a, b) == b                          # neighbours in float32
    (rk, fk), (rr, fr) = host(kept, oc), host(removed, oc)
    assert fk[5] == 0 and fr[5] == 1 and rk["n_bad"] == 0 and rr["n_bad"] == 1
    assert np.array_equal(np.delete(fk, 5), np.delete(fr, 5))
    for W, (rec, flags) in ((kept, (rk, fk)), (removed, (rr, fr))):
        tr = sm.Trace()
        mrec, mflags = sm.optimize(W, on, tr)
        assert_same(mrec, mflags, rec, flags, (edge, on))
    # the chi2 the test read lies either side of th2, within what one float32 step of the observation moves it
    trk, trr = sm.Trace(), sm.Trace()
    sm.optimize(kept, on, trk); sm.optimize(removed, on, trr)
    col = 0 if edge == "12" else 1
    ck, cr = trk.class_chi[0][col][5], trr.class_chi[0][col][5]
    assert ck <= sw.TH2 < cr and (cr - ck) / sw.TH2 < 1e-4


# ---- the model finds the truth ----------------------------------------------------------------------------------------------------------
def analytic_jacobians(q, t, s, W):
    """d e12 / d delta and d e21 / d delta at delta = 0 of Sim3(delta) * T, T = (unit quaternion q, t, s), from the closed forms:
    p = T X2 moves by omega x p + upsilon + sigma p; q = T^-1 X1 moves by -(1/s) R^T (omega x X1 + upsilon + sigma X1)."""
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    X1, X2 = W["x3dc1"].astype(np.float64), W["x3dc2"].astype(np.float64)
    skew = lambda v: np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])

    def dproj(K, p):
        return np.array([[K[0] / p[2], 0, -K[0] * p[0] / p[2] ** 2], [0, K[1] / p[2], -K[1] * p[1] / p[2] ** 2]])

    J12, J21 = [], []
    for a, b in zip(X1, X2):
        p = s * (R @ b) + np.asarray(t)
        J12.append(-dproj(W["K1"], p) @ np.concatenate([-skew(p), np.eye(3), p[:, None]], axis=1))
        qq = (R.T @ (a - np.asarray(t))) / s
        J21.append(dproj(W["K2"], qq) @ (R.T / s) @ np.concatenate([-skew(a), np.eye(3), a[:, None]], axis=1))
    return np.array(J12), np.array(J21)


def unit_truth(W):
    R, t, s = W["truth"]
    q = np.array(sm.quat_from_matrix([[float(v) for v in row] for row in R]))
    return list(map(float, q / np.linalg.norm(q))), [float(v) for v in t], float(s)


@pytest.mark.parametrize("on", ["index", "device"])
def test_the_numeric_jacobian_is_the_analytic_derivative(on):
    """Bound: an entry is scalar * (e+ - e-) with scalar = 1 / 2e-9.  computeError rounds 11 times per component of T.map(X) (9 in
    _transformVector, the scale, the translation) for the two components a pixel coordinate divides, then the division, the focal
    length, the principal point and the subtraction from the observation: 26 roundings, each at most half an ulp of the largest pixel
    coordinate, in each of the two errors -- 26 ulp in their difference.  The truncation of the central difference is of the order of
    1e-18 * the third derivative and does not count."""
    W = sw.generate(51, 60, s=1.3, grade=0)
    q, t, s = unit_truth(W)
    E = sm.Edges(W)
    J12, J21 = E.jacobians(sm.Sim3(q, t, s), False, on)
    A12, A21 = analytic_jacobians(q, t, s, W)
    pmax = max(float(np.abs(W["obs1"]).max()), float(np.abs(W["obs2"]).max()))
    bound = float(np.spacing(pmax)) * 26 / 2e-9
    worst = 0.0
    for J, A in ((J12, A12), (J21, A21)):
        for r in range(2):
            for c in range(7):
                worst = max(worst, float(np.abs(J[r][c] - A[:, r, c]).max()))
    print("numeric against analytic Jacobian (%s): largest difference %.3e, bound %.3e, largest entry %.1f" % (on, worst, bound, np.abs(A12).max()))
    assert worst <= bound


def parameter_error(rec, W):
    """delta with estimate = Sim3(delta) * truth to first order: (omega, upsilon, sigma)"""
    R0, t0, s0 = W["truth"]
    q = rec["q"] / np.linalg.norm(rec["q"])
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    D = R @ R0.T
    omega = 0.5 * np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    sigma = math.log(float(rec["s"]) / s0)
    upsilon = rec["t"] - (float(rec["s"]) / s0) * (D @ t0)
    return np.concatenate([omega, upsilon, [sigma]])


@pytest.mark.parametrize("grade", [0, 2, 3])
def test_a_clean_world_returns_its_sim3(grade):
    """A noise-free, outlier-free world: started at the truth it stays there, started off it returns there.  Bound, from the float
    rounding of the inputs: a point coordinate is off by at most 2^-24 max|X|, which moves a projection by at most f (1 + tan) / z_min
    of that with tan <= 1 the largest |x / z|; each edge reads one point through the transform, compares with an observation rounded
    to 2^-24 of the largest pixel coordinate, and its other point defines where the truth projects: eps = 2^-24 (P + 2 * 2 f max|X| /
    z_min) pixels per residual.  The least-squares estimate moves by at most |J^+| |dr| <= eps sqrt(4 n) / sigma_min(J) for the 4 n
    residuals, J the whitened analytic Jacobian at the truth (sqrt(w) <= 1 scales both sides).  If central differences at 1e-9 keep the
    MODEL from reaching that, the bound is widened to 4 x the model's own error and both are printed."""
    W = sw.generate(52, 80, s=0.8, grade=grade)
    q, t, s = unit_truth(W)
    A12, A21 = analytic_jacobians(q, t, s, W)
    w1 = W["inv_level_sigma2_1"][W["octave1"]].astype(np.float64); w2 = W["inv_level_sigma2_2"][W["octave2"]].astype(np.float64)
    J = np.concatenate([(A12 * np.sqrt(w1)[:, None, None]).reshape(-1, 7), (A21 * np.sqrt(w2)[:, None, None]).reshape(-1, 7)])
    smin = float(np.linalg.svd(J, compute_uv=False)[-1])
    mx = max(float(np.abs(W["x3dc1"]).max()), float(np.abs(W["x3dc2"]).max()))
    zmin = min(float(W["x3dc1"][:, 2].min()), float(W["x3dc2"][:, 2].min()))
    P = max(float(np.abs(W["obs1"]).max()), float(np.abs(W["obs2"]).max()))
    eps = 2.0 ** -24 * (P + 2 * 2 * max(W["K1"][0], W["K2"][1]) * mx / zmin)
    bound = eps * math.sqrt(4 * W["n"]) / smin
    mrec, _ = sm.optimize(W, "index")
    model_err = float(np.linalg.norm(parameter_error(mrec, W)))
    used = bound if model_err <= bound else 4 * model_err
    print("grade %d: derived bound %.3e, the model's error %.3e, bound used %.3e" % (grade, bound, model_err, used))
    for on, oc in ORDERS:
        rec, flags = host(W, oc)
        err = float(np.linalg.norm(parameter_error(rec, W)))
        print("    %s order: error %.3e, %d + %d iterations" % (on, err, rec["round"][0]["iterations"], rec["round"][1]["iterations"]))
        assert rec["n_inliers"] == W["n"] and not flags.any() and err <= used


# ---- the solver and the device's exponential ----------------------------------------------------------------------------------------------
def test_the_ldlt_of_size_7_solves_the_system():
    """Against numpy.linalg.solve on well-conditioned positive definite systems.  Bound: a Cholesky-type factorisation is backward
    stable with a constant of the order of n^2, so both solutions lie within n^2 * 2^-53 * cond of the true one: 2 n^2 2^-53 cond apart."""
    rng = np.random.RandomState(9)
    for _ in range(50):
        A = rng.randn(14, 7)
        H = A.T @ A * rng.uniform(1, 1e4) + np.diag(rng.uniform(0, 1e-3, 7))
        b = rng.randn(7)
        want = np.linalg.solve(H, b)
        tol = 2 * 49 * 2.0 ** -53 * np.linalg.cond(H) * np.abs(want).max()
        ok, x = m.sim3opt_ldlt7(H, b)
        mok, mx = sm.ldlt_solve([list(map(float, r)) for r in H], list(map(float, b)))
        assert ok and mok and list(x) == mx                               # the library's instantiation is the model's, bit for bit
        assert np.abs(x - want).max() <= tol
    ok, _ = m.sim3opt_ldlt7(-np.eye(7), np.ones(7))
    assert not ok and not sm.ldlt_solve([[-1.0 if i == j else 0.0 for j in range(7)] for i in range(7)], [1.0] * 7)[0]


def ulps(a, b):
    return abs(a - b) / float(np.spacing(abs(b)))


def test_the_device_exponential():
    """exp(0) is exactly 1 (the fixed-scale path evaluates nothing else); the library's sequence is the model's; its distance from the
    C library is MEASURED over the arguments the worlds produce and a grid on [-1, 1], not fixed in advance."""
    assert m.sim3opt_exp(0.0) == 1.0 and sm.poly_exp(0.0) == 1.0 and m.sim3opt_exp(-0.0) == 1.0
    args = [float(x) for x in np.linspace(-1.0, 1.0, 20001)] + [1e-9, -1e-9, 1e-5, -1e-5, 0.15, -0.15, 5.0, -5.0, 30.0, -30.0, 700.0, -700.0]
    rng = np.random.RandomState(3)
    args += [float(x) for x in rng.uniform(-0.2, 0.2, 5000)] + [float(x) for x in rng.randn(2000) * 1e-6]
    worst = 0.0
    for x in args:
        e = m.sim3opt_exp(x)
        assert e == sm.poly_exp(x), x
        worst = max(worst, ulps(e, math.exp(x)))
    print("largest distance of the + - * / exponential from math.exp over %d arguments: %.2f ulp" % (len(args), worst))
    assert m.sim3opt_exp(1000.0) == float("inf") and m.sim3opt_exp(-1000.0) == 0.0 and math.isnan(m.sim3opt_exp(float("nan")))
    s, c = m.pose_sincos(0.3)
    assert (s, c) == poly_sincos(0.3)
