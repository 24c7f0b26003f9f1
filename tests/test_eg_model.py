"""The essential graph on the CPU: the host routine (orbm_essential_graph_host) against tests/eg_model.py byte for byte in both orders, what
holds the logarithm (round trip, four branches, ulp against the C library for the device order's sequences), the numeric Jacobian against
an independent evaluation on 4 x 4 matrices, the two orders against each other, and a consistent ring that has to close.  The recorded
figures are profiles/r22/notes_essential_graph.md's."""
import ctypes as C
import math

import numpy as np
import pytest

import multi_orb_slam_amd as m
from multi_orb_slam_amd import _lib

import eg_model as em
import eg_worlds as ew
from sim3opt_model import Sim3

ORD = {"index": m.POSE_ORDER_INDEX, "device": m.POSE_ORDER_DEVICE}
# free vertices, points, iterations: the model is Python, so the larger rings run fewer iterations
SEEDED = [(1, 0, 20), (9, 1, 20), (10, 5000, 20), (40, 1, 6), (150, 0, 1)]
# the recorded maxima (profiles/r22/notes_essential_graph.md), measured with the INDEX-order routine
ULP_LOG, ULP_ACOS = 2.0, 6.0
ROUND_TRIP = 3.8e-14
JACOBIAN = 3.6e-6
ORDERS_ESTIMATE = 5.7e-7
# chi2: measured.  lambda: measured 0 (every accepted trial's factor is one of the clamps 1/3, 2/3); where it is not a clamp it is
# 1 - (2 rho - 1)^3 with rho differing by the 1e-6 the guard band is derived from, hence the bound
ORDERS_CHI2, ORDERS_LAMBDA = 2.0e-9, 1.0e-6
RING_FRACTION = 4.3e-7
BAND = 1e-5


def same(R, H):
    for k in em.Result.FIELDS:
        a, b = getattr(R, k), getattr(H, k)
        if (a.tobytes() != b.tobytes()) if isinstance(a, np.ndarray) else (a != b):
            return k
    return None


def host(W, iterations, order):
    return m.essential_graph_host(ew.make_problem(m, W), iterations, ORD[order])


@pytest.mark.parametrize("order", ["index", "device"])
@pytest.mark.parametrize("fix_scale", [False, True])
@pytest.mark.parametrize("n_free,n_points,iterations", SEEDED)
def test_model_equals_host_routine_on_seeded_worlds(n_free, n_points, iterations, fix_scale, order):
    W = ew.ring(n_free, 100 + n_free, fix_scale=fix_scale, n_points=n_points, covis=2 if n_free > 100 else 3)
    H = host(W, iterations, order)
    assert same(em.optimize(W, iterations, order), H) is None
    assert H.optimised == 1 and H.active_vertices == n_free + 1 and H.round["trials"][0] >= H.round["iterations"][0] >= 1


CASES = ew.hand_cases()


@pytest.mark.parametrize("order", ["index", "device"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_model_equals_host_routine_on_hand_built_cases(name, order):
    W, iterations = CASES[name]
    tr = []
    R = em.optimize(W, iterations, order, trace=tr)
    H = host(W, iterations, order)
    assert same(R, H) is None
    rnd = H.round[0]
    if name == "no_edges":
        assert H.optimised == 0 and H.active_vertices == 0 and H.estimate.tobytes() == np.ascontiguousarray(W["vertex"]).tobytes()
    if name == "zero_iterations":
        assert H.optimised == 1 and rnd["iterations"] == 0 and H.estimate.tobytes() == np.ascontiguousarray(W["vertex"]).tobytes()
    if name == "exact_optimum":
        assert rnd["iterations"] == 1 and rnd["trials"] == 1 and rnd["chi2"] == 0.0 and ("exit", "rho0") in tr
    if name == "every_solve_fails":
        assert [t[2] for t in tr if t[0] == "solve"] and not any(t[2] for t in tr if t[0] == "solve")
        assert H.estimate.tobytes() == np.ascontiguousarray(W["vertex"]).tobytes() and math.isnan(rnd["chi2"])
    if name == "edge_between_fixed":
        fixed = (W["edge_v0"] >= W["n_free"]) & (W["edge_v1"] >= W["n_free"])
        assert fixed.any() and H.active_edges == len(fixed)
        # the edge between the fixed vertices counts in chi2: without it the sum is another one
        keep = ~fixed
        W2 = dict(W, measurement=W["measurement"][keep], edge_v0=W["edge_v0"][keep], edge_v1=W["edge_v1"][keep])
        assert host(W2, iterations, order).round["chi2"][0] != rnd["chi2"]
    if name == "vertex_without_edge":
        assert H.active_vertices == len(W["vertex"]) - 1 and H.estimate[4].tobytes() == W["vertex"][4].tobytes()


def test_the_logarithm_takes_each_branch_and_a_rotation_near_pi():
    for want, T in enumerate(ew.log_branch_sims()):
        for order in ("index", "device"):
            out, branch = m.sim3_log_eval(em.as_vec8(T), ORD[order])
            ref, b = em.sim3_log(T, order)
            assert branch == b == (want if want < 4 else 3)
            assert out.tobytes() == np.array(ref).tobytes()
    T = ew.log_branch_sims()[4]
    out, _ = m.sim3_log_eval(em.as_vec8(T), ORD["index"])
    # 1 - d*d = 2.5e-7 carries the rounding of d*d (1.1e-16: 4.4e-10 of it), half of that in the square root, times pi, and the
    # quaternion's own departure from unit norm the same way: a few 1e-9; the division is the reference's
    assert abs(np.linalg.norm(out[:3]) - (math.pi - 5e-4)) < 1e-8


def test_log_of_exp_returns_the_vector_in_each_branch():
    rng = np.random.default_rng(5)
    worst = 0.0
    for want, (th, sg) in enumerate([(3e-6, 3e-6), (0.8, 3e-6), (3e-6, 0.4), (0.8, 0.4)]):
        for _ in range(200):
            w = rng.normal(size=3)
            w = w / np.linalg.norm(w) * th * rng.uniform(0.3, 1)
            v = np.concatenate([w, rng.normal(size=3), [sg * rng.uniform(-1, 1)]])
            T, eb = Sim3.exp([float(x) for x in v], "index")
            out, lb = m.sim3_log_eval(em.as_vec8(T), ORD["index"])
            assert eb == lb == want
            worst = max(worst, float(np.abs(out - v).max()))
    print("[eg] log(exp(v)) - v: %.3g (recorded %.3g)" % (worst, ROUND_TRIP))
    assert worst <= 10 * ROUND_TRIP


def ulps(a, b):
    return abs(a - b) / float(np.spacing(abs(b)))


def test_device_order_logarithm_and_arc_cosine_in_ulp_of_the_c_library():
    """Over the arguments Sim3::log() can hand them: s in [1e-3, 1e3] (and a cluster around 1), d in [-1, 1 - 1e-5] (and clusters at
    both ends).  The arc cosine's 6 ulp are sim3_atan2's own 6 ulp: nothing is added on top of it."""
    rng = np.random.default_rng(1)
    s = np.concatenate([np.exp(rng.uniform(math.log(1e-3), math.log(1e3), 60000)), 1 + rng.uniform(-1e-4, 1e-4, 20000), [1e-3, 1e3, 1.0]])
    worst_log = max(ulps(m.pose_log(float(v)), math.log(float(v))) for v in s if v != 1.0)
    assert m.pose_log(1.0) == 0.0
    d = np.concatenate([rng.uniform(-1, 1 - 1e-5, 60000), 1 - 10 ** rng.uniform(-5, -1, 20000), -1 + 10 ** rng.uniform(-16, -1, 20000),
                        [-1.0, 1 - 1e-5, 0.0]])
    worst_acos = max(ulps(m.pose_acos(float(v)), math.acos(float(v))) for v in d)
    print("[eg] pose_log %.2f ulp, pose_acos %.2f ulp" % (worst_log, worst_acos))
    assert worst_log <= ULP_LOG and worst_acos <= ULP_ACOS
    for v in list(s[:2000]) + [1.0]:
        assert m.pose_log(float(v)) == em.poly_log(float(v))
    for v in list(d[:2000]) + [-1.0, 1.0]:
        assert m.pose_acos(float(v)) == em.poly_acos(float(v))


# ---- the Jacobian against an independent evaluation ------------------------------------------------------------------------------------
def mat4(v8):
    M = np.eye(4)
    M[:3, :3] = v8[7] * np.array(em.quat_to_matrix([float(x) for x in v8[:4]]))
    M[:3, 3] = v8[4:7]
    return M


def expm4(v):
    """exp of the generator [[sigma I + Omega, upsilon], [0, 0]] by its series."""
    G = np.zeros((4, 4))
    G[:3, :3] = [[v[6], -v[2], v[1]], [v[2], v[6], -v[0]], [-v[1], v[0], v[6]]]
    G[:3, 3] = v[3:6]
    out, term = np.eye(4), np.eye(4)
    for k in range(1, 30):
        term = term @ G / k
        out = out + term
    return out


def log4(M):
    """The logarithm of [[s R, t], [0, 1]] without the closed forms of Sim3::log: W = (s R - I) (sigma I + Omega)^-1 (sigma != 0)."""
    sR = M[:3, :3]
    s = np.cbrt(np.linalg.det(sR))
    R = sR / s
    theta = math.acos(min(1.0, max(-1.0, 0.5 * (np.trace(R) - 1))))
    dR = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    omega = dR * (0.5 if theta < 1e-7 else theta / (2 * math.sin(theta)))
    sigma = math.log(s)
    N = np.array([[sigma, -omega[2], omega[1]], [omega[2], sigma, -omega[0]], [-omega[1], omega[0], sigma]])
    Wm = (sR - np.eye(3)) @ np.linalg.inv(N)
    return np.concatenate([omega, np.linalg.solve(Wm, M[:3, 3]), [sigma]])


def error4(C, V0, V1):
    return log4(C @ V0 @ np.linalg.inv(V1))


def test_jacobians_agree_with_central_differences_of_a_4x4_evaluation():
    W = ew.ring(9, 109, n_points=0, drift=4.0)
    worst, worst_e = 0.0, 0.0
    h = 1e-6
    for e in range(len(W["edge_v0"])):
        M8, a8, b8 = W["measurement"][e] * 1.0, W["vertex"][W["edge_v0"][e]], W["vertex"][W["edge_v1"][e]]
        M8[7] *= 1.07                                    # sigma of the error away from 0: log4 needs it
        err, chi2, J0, J1 = m.eg_edge_eval(M8, a8, b8, False, ORD["index"])
        mo = em.edge_eval(M8, a8, b8, False, "index")
        assert err.tobytes() == mo[0].tobytes() and J0.tobytes() == mo[2].tobytes() and J1.tobytes() == mo[3].tobytes() and chi2 == mo[1]
        Cm, A, B = mat4(M8), mat4(a8), mat4(b8)
        worst_e = max(worst_e, float(np.abs(err - error4(Cm, A, B)).max()))
        for d in range(7):
            u = np.zeros(7)
            u[d] = h
            c0 = (error4(Cm, expm4(u) @ A, B) - error4(Cm, expm4(-u) @ A, B)) / (2 * h)
            c1 = (error4(Cm, A, expm4(u) @ B) - error4(Cm, A, expm4(-u) @ B)) / (2 * h)
            worst = max(worst, float(np.abs(J0[:, d] - c0).max()), float(np.abs(J1[:, d] - c1).max()))
    print("[eg] Jacobian against central differences at 1e-6: %.3g (recorded %.3g); the error itself %.3g" % (worst, JACOBIAN, worst_e))
    assert worst <= 10 * JACOBIAN and worst_e <= 1e-12


def test_fixed_scale_makes_column_six_exactly_zero():
    W = ew.ring(3, 57, fix_scale=True)
    for e in range(len(W["edge_v0"])):
        _, _, J0, J1 = m.eg_edge_eval(W["measurement"][e], W["vertex"][W["edge_v0"][e]], W["vertex"][W["edge_v1"][e]], True, ORD["index"])
        assert not J0[:, 6].any() and not J1[:, 6].any() and J0[:, :6].any() and J1[:, :6].any()
        _, _, F0, _ = m.eg_edge_eval(W["measurement"][e], W["vertex"][W["edge_v0"][e]], W["vertex"][W["edge_v1"][e]], False, ORD["index"])
        assert F0[:, 6].any()


@pytest.mark.parametrize("rule,case", [("perturb_fixed_scale", "fix_scale_column"), ("perturb_fixed_scale", "fix_scale_compute_scale"),
                                       ("skip_unreferenced", "unreferenced_points"), ("touch_inactive", "vertex_without_edge")])
def test_the_tidy_alternative_changes_bytes(rule, case):
    W, iterations = CASES[case]
    H = host(W, iterations, "index")
    assert same(em.optimize(W, iterations, "index"), H) is None
    assert same(em.optimize(W, iterations, "index", rules=(rule,)), H) is not None


def test_compute_scale_reads_zeros_either_way():
    """Statement 2 of the fixed scale (update(x) runs before computeScale()) cannot change a byte: with column 6 of every Jacobian
    exactly 0 the solver's x[6] is +-0 before oplusImpl zeroes it (tests/eg_model.py's docstring).  The model says so."""
    W, iterations = CASES["fix_scale_compute_scale"]
    assert same(em.optimize(W, iterations, "index", rules=("scale_before_update",)), host(W, iterations, "index")) is None


@pytest.mark.parametrize("fix_scale", [False, True])
@pytest.mark.parametrize("n_free,iterations", [(1, 1), (9, 2), (10, 2), (40, 2)])
def test_the_two_orders_agree_on_every_verdict(n_free, iterations, fix_scale):
    """The worlds meet the guard band first: no trial of the INDEX-order model run has |currentChi - tempChi| within BAND of currentChi,
    so no verdict `rho > 0` is within the rounding the orders differ by (profiles/r22/notes_essential_graph.md)."""
    W = ew.ring(n_free, 200 + n_free, fix_scale=fix_scale, n_points=2, drift=4.0)
    tr = []
    em.optimize(W, iterations, "index", trace=tr)
    margin = em.verdict_margin(tr)
    assert margin > BAND, margin
    a, b = host(W, iterations, "index"), host(W, iterations, "device")
    diff = float(np.abs(a.estimate - b.estimate).max())
    print("[eg] orders, %d free, fixed scale %s: estimates differ by %.3g, closest verdict %.3g" % (n_free, fix_scale, diff, margin))
    assert diff <= 10 * ORDERS_ESTIMATE
    assert a.round["iterations"][0] == b.round["iterations"][0] and a.round["trials"][0] == b.round["trials"][0]
    assert (a.optimised, a.active_vertices, a.active_edges) == (b.optimised, b.active_vertices, b.active_edges)
    # every verdict, trial by trial: the model equals the host routine byte for byte in each order, so its traces are the routine's
    td = []
    assert same(em.optimize(W, iterations, "device", trace=td), b) is None
    verdicts = lambda t: [(e[1], e[4] > 0 and abs(e[3]) <= em.DBL_MAX) for e in t if e[0] == "trial"]
    others = lambda t: [e for e in t if e[0] in ("solve", "exit")]
    assert verdicts(tr) == verdicts(td) and others(tr) == others(td) and len(verdicts(tr)) == a.round["trials"][0]
    chi = abs(a.round["chi2"][0] - b.round["chi2"][0]) / a.round["chi2"][0]
    lam = abs(a.round["lambda"][0] - b.round["lambda"][0]) / a.round["lambda"][0]
    print("[eg]   the round record: chi2 differs by %.3g of itself, lambda by %.3g" % (chi, lam))
    assert chi <= 10 * ORDERS_CHI2 and lam <= 10 * ORDERS_LAMBDA


@pytest.mark.parametrize("order", ["index", "device"])
@pytest.mark.parametrize("fix_scale", [False, True])
@pytest.mark.parametrize("n_free", [9, 40])
def test_a_consistent_ring_closes(n_free, fix_scale, order):
    W = ew.ring(n_free, 300 + n_free, fix_scale=fix_scale, drift=4.0, consistent=True)
    Cs = [em.as_sim3(v) for v in W["measurement"]]
    v0, v1 = list(W["edge_v0"]), list(W["edge_v1"])
    before = em.total_chi2(Cs, [em.as_sim3(v) for v in W["vertex"]], v0, v1, "index")
    H = host(W, 20, order)
    after = em.total_chi2(Cs, [em.as_sim3(v) for v in H.estimate], v0, v1, "index")
    print("[eg] consistent ring of %d, fixed scale %s, %s: chi2 %.4g -> %.4g (%.3g of it)" % (n_free, fix_scale, order, before, after, after / before))
    assert before > 1.0 and after <= 10 * RING_FRACTION * before


def test_the_record_layouts_equal_the_abi_structs():
    assert C.sizeof(_lib.EgProblem) == 8 * 4 + 6 * 8 and _lib.EgProblem.vertex.offset == 32 and _lib.EgProblem.point_ref.offset == 72
    assert C.sizeof(_lib.EgResult) == 3 * 8 + 24 + 4 * 4 and _lib.EgResult.round.offset == 24 and _lib.EgResult.optimised.offset == 48
    assert (m.EG_MAX_FREE, m.EG_MAX_VERTICES, m.EG_MAX_EDGES, m.EG_MAX_POINTS) == (877, 4096, 65536, 1 << 19)
    assert 7 * m.EG_MAX_FREE <= 6 * m.BA_MAX_FREE


def test_bad_arguments_are_refused():
    W = ew.ring(3, 7)
    with pytest.raises(_lib.OrbError):
        host(dict(W, edge_v1=W["edge_v0"]), 2, "index")            # an edge of a vertex to itself
    with pytest.raises(_lib.OrbError):
        host(dict(W, edge_v0=W["edge_v0"] + 100), 2, "index")
