"""The model of the pose optimisation (tests/pose_model.py) against the library's host routine (orbm_pose_optimize_host: the statement
sequence the kernel shares) byte for byte in both summation orders, against known answers, and the two orders against each other --
which is where the tolerance of the device comparison comes from.  No device needed."""
import math

import numpy as np
import pytest

import multi_orb_slam_amd as m
import pose_model as pm
import pose_worlds as pw

NAMES = [name for name, _ in pw.worlds()]
WORLD = dict(pw.worlds())

# The largest differences between the index order and the device order over all worlds, measured here on the CPU with the model
# (test_the_two_orders_against_each_other prints them; profiles/r10/notes_pose.md).  The device comparison allows four times these:
# the margin the triangulation stage gives its LAPACK comparison, for another compiler's instruction selection and nothing more.
ORDER_DIFF_TRANSLATION = 2.4e-11
ORDER_DIFF_QUATERNION = 2.92e-13
ORDER_DIFF_CHI2 = 5.2e-8
POSE_MARGIN = 4


def host(P, order):
    (rec, flags), = m.pose_optimize_host([pw.to_problem(m, P)], order=order)
    return rec, flags


def assert_same(got, want, what):
    rec, flags = got
    mrec, mflags = want
    for k in mrec.dtype.names:
        assert rec[k].tobytes() == mrec[k].tobytes(), (what, k, rec[k], mrec[k])
    assert rec.tobytes() == mrec.tobytes(), what
    assert np.array_equal(flags, mflags), (what, "flags")


def test_record_layouts_are_the_abi_structs():
    assert m.POSE_RESULT_DTYPE == pm.RESULT_DTYPE and m.POSE_RESULT_DTYPE.itemsize == 232
    assert m.POSE_PROBLEM_DTYPE.itemsize == 272
    assert [m.POSE_RESULT_DTYPE.fields[k][1] for k in ("Tcw", "q", "t", "n_initial", "n_bad", "n_inliers", "rounds", "round")] == \
        [0, 64, 96, 120, 124, 128, 132, 136]


def test_the_worlds_meet_their_conditions():
    margin, rho, reached = pw.check_conditions(verbose=True)
    print("smallest classification margin %.3e (guard %.0e), smallest |rho| %.3e (guard %.0e), branches %s" % (
        margin, pw.GUARD, rho, pw.RHO_GUARD, sorted(reached)))


@pytest.mark.parametrize("name", NAMES)
def test_index_order_equals_the_model(name):
    rec, flags, _ = pw.evaluate("index")[name]
    assert_same(host(WORLD[name], m.POSE_ORDER_INDEX), (rec, flags), name)


@pytest.mark.parametrize("name", NAMES)
def test_device_order_equals_the_models_device_mode(name):
    rec, flags, _ = pw.evaluate("device")[name]
    assert_same(host(WORLD[name], m.POSE_ORDER_DEVICE), (rec, flags), name)


def test_a_batch_is_its_problems_one_by_one():
    names = ["stereo_60/all", "two/cam0", "mixed_400/cam0", "nine/all", "all_outliers/cam0", "rig_400/all"]
    for order, key in ((m.POSE_ORDER_INDEX, "index"), (m.POSE_ORDER_DEVICE, "device")):
        got = m.pose_optimize_host([pw.to_problem(m, WORLD[n]) for n in names], order=order)
        for n, g in zip(names, got):
            rec, flags, _ = pw.evaluate(key)[n]
            assert_same(g, (rec, flags), n)


def test_hand_built_cases_end_where_they_should():
    ev = pw.evaluate("index")
    rec, flags, tr = ev["two/cam0"]
    assert rec["n_inliers"] == 0 and rec["rounds"] == 0 and rec["Tcw"].tobytes() == WORLD["two/cam0"]["Tcw"].tobytes() and not flags.any()
    rec, flags, tr = ev["nine/cam0"]
    assert rec["rounds"] == 1 and rec["n_initial"] == 9 and not rec["round"][1]["iterations"]
    rec, flags, tr = ev["all_outliers/cam0"]
    assert flags.all() and rec["n_inliers"] == 0 and rec["round"][0]["iterations"] > 0 and not rec["round"][1:]["iterations"].any()
    assert "nothing_active" in tr.branches
    # nothing was optimised in the last round: the estimate is the start pose
    assert np.array_equal(rec["t"], np.array(pm.SE3.from_cv(WORLD["all_outliers/cam0"]["Tcw"]).t))
    rec, flags, tr = ev["exact/cam0"]
    assert "rho_zero" in tr.branches and rec["round"][0]["iterations"] == 1 and rec["round"][0]["trials"] == 1 and rec["round"][0]["chi2"] == 0
    assert rec["Tcw"].tolist() == np.eye(4, dtype=np.float32).reshape(16).tolist() and not flags.any()
    rec, flags, tr = ev["rejected/cam0"]
    assert "rejected_trial" in tr.branches and rec["round"]["trials"].sum() > rec["round"]["iterations"].sum()
    rec, flags, tr = ev["behind/all"]
    assert "depth_not_positive" in tr.branches


@pytest.mark.parametrize("kind,two_cams", [("mono", False), ("stereo", False), ("mixed", True)])
def test_a_noise_free_world_returns_the_true_pose(kind, two_cams):
    P = pw.generate(seed=41, n=200, kind=kind, outliers=0.0, start=(0.1, 4.0), two_cams=two_cams, noise=0.0)
    for mode in (pm.CAM0, pm.ALL_CAMS):
        rec, flags = host(pw.with_mode(P, mode), m.POSE_ORDER_INDEX)
        assert not flags.any() and rec["n_inliers"] == rec["n_initial"]
        # the points and observations are floats: the optimum sits within their rounding of the truth, the float pose within its own
        T = P["Tcw_true"]
        assert np.abs(rec["Tcw"].reshape(4, 4) - T).max() < 2e-5, np.abs(rec["Tcw"].reshape(4, 4) - T).max()
        R = np.array(pm.quat_to_matrix(list(rec["q"])))
        assert np.array_equal(rec["Tcw"].reshape(4, 4)[:3, :3], R.astype(np.float32))
        assert np.array_equal(rec["Tcw"].reshape(4, 4)[:3, 3], rec["t"].astype(np.float32))


@pytest.mark.parametrize("mode", [pm.CAM0, pm.ALL_CAMS])
def test_jacobians_agree_with_central_differences(mode):
    # all four edge types: mono and stereo edges in the plain form (CAM0) and in the _multi form of both cameras (ALL_CAMS)
    P = pw.with_mode(pw.generate(seed=42, n=64, kind="mixed", outliers=0.0, start=(0.05, 2.0), two_cams=True), mode)
    E = pm.Edges(P)
    assert E.stereo.any() and (~E.stereo).any() and (mode == pm.CAM0 or (E.cam1.any() and (~E.cam1).any()))
    T = pm.SE3.from_cv(P["Tcw"])
    _, _, p, pc = E.errors(T)
    J = E.jacobians(p, pc)
    # A monocular edge's error is a smooth double function: step 1e-6, agreement to 1e-5.  A stereo edge's cam_project rounds 1/z to
    # FLOAT (the reference's `const float invz`), so its error is quantised: half a float ulp of 1/z, 3e-8 relative, times |x / z| * fx
    # <= 385 pixels is 1.2e-5 pixels per evaluation, 2.3e-5 per difference, 1.2e-2 after the division by 2h = 2e-3 (rounded up to
    # 2e-2 absolute); the step's own truncation error, h^2 / 6 times a third derivative of a few |J|, adds 1e-4 relative.
    for stereo, h, tol in ((False, 1e-6, 1e-5), (True, 1e-3, 1e-4)):
        rows = E.stereo == stereo
        for k in range(6):
            d = [0.0] * 6
            d[k] = h
            ep, _, _, _ = E.errors(pm.SE3.exp(d, "index")[0] * T)
            d[k] = -h
            em, _, _, _ = E.errors(pm.SE3.exp(d, "index")[0] * T)
            for r in range(3 if stereo else 2):
                num = (ep[r] - em[r]) / (2 * h)
                allowed = (2e-2 if stereo else tol) + tol * np.abs(J[r][k][rows])
                assert (np.abs(num[rows] - J[r][k][rows]) <= allowed).all(), (mode, stereo, r, k, (np.abs(num[rows] - J[r][k][rows]) / allowed).max())


def test_the_polynomial_sine_and_cosine_stay_within_two_ulp_of_the_c_library():
    rng = np.random.RandomState(7)
    worst = 0.0
    for lo, hi, count in ((-math.pi, math.pi, 40000), (-100.0, 100.0, 40000), (1e-5, 1e-2, 5000)):
        for x in rng.uniform(lo, hi, count):
            s, c = pm.poly_sincos(float(x))
            rs, rc = math.sin(x), math.cos(x)
            worst = max(worst, abs(s - rs) / np.spacing(abs(rs)), abs(c - rc) / np.spacing(abs(rc)))
    print("largest deviation from math.sin / math.cos: %.1f ulp" % worst)
    assert worst <= 2.0
    # and the library's sequence is the model's, bit for bit
    for x in list(rng.uniform(-50, 50, 3000)) + [0.0, 1e-5, math.pi / 4, math.pi / 2, math.pi, 1e3]:
        assert m.pose_sincos(float(x)) == pm.poly_sincos(float(x)), x


def test_the_ldlt_restatement_solves_the_system():
    rng = np.random.RandomState(8)
    for _ in range(50):
        A = rng.randn(12, 6)
        H = A.T @ A * rng.uniform(1, 1e4) + np.diag(rng.uniform(0, 1e-3, 6))
        b = rng.randn(6)
        ok, x = pm.ldlt_solve([list(map(float, r)) for r in H], list(map(float, b)))
        assert ok and np.allclose(x, np.linalg.solve(H, b), rtol=1e-8, atol=1e-12)
    ok, x = pm.ldlt_solve([[-1.0 if i == j else 0.0 for j in range(6)] for i in range(6)], [1.0] * 6)
    assert not ok


def test_the_two_orders_against_each_other():
    a, b = pw.evaluate("index"), pw.evaluate("device")
    dt = dq = dchi = 0.0
    for name, P in pw.worlds():
        ra, fa, ta = a[name]
        rb, fb, tb = b[name]
        assert np.array_equal(fa, fb), name                      # the outlier flags: IDENTICAL
        assert ra["n_inliers"] == rb["n_inliers"] and ra["n_bad"] == rb["n_bad"] and ra["rounds"] == rb["rounds"], name
        dt = max(dt, float(np.abs(ra["t"] - rb["t"]).max()))
        dq = max(dq, float(min(np.abs(ra["q"] - rb["q"]).max(), np.abs(ra["q"] + rb["q"]).max())))
        # a classified chi2 relative to the scale its threshold test lives on: the chi2 itself, or the threshold where it is below it
        th = np.where(~(np.asarray(P["obs"], np.float32).reshape(-1, 3)[:, 2] < 0), 7.815, 5.991)
        for ca, cb in zip(ta.class_chi, tb.class_chi):
            with np.errstate(all="ignore"):
                rel = np.abs(ca - cb) / np.maximum(np.abs(ca), th)
            rel = rel[np.isfinite(rel)]
            if len(rel):
                dchi = max(dchi, float(rel.max()))
    print("index order against device order over %d worlds: translation %.3e, quaternion (up to sign) %.3e, classified chi2 %.3e" % (
        len(a), dt, dq, dchi))
    assert dt <= POSE_MARGIN * ORDER_DIFF_TRANSLATION and dq <= POSE_MARGIN * ORDER_DIFF_QUATERNION
    assert dchi * 100 <= pw.GUARD


def test_bad_arguments_are_refused():
    P = dict(WORLD["mono_60/cam0"])
    P["octave"] = P["octave"].copy()
    P["octave"][3] = pw.N_LEVELS
    with pytest.raises(m.OrbError):
        host(P, m.POSE_ORDER_INDEX)
    with pytest.raises(m.OrbError):
        host(WORLD["mono_60/cam0"], 7)
    with pytest.raises(m.OrbError):
        m.pose_optimize_host([pw.to_problem(m, WORLD["two/cam0"])] * 65)
