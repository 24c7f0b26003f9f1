"""The local bundle adjustment on the CPU: the library's host routine (orbm_local_ba_host) against the NumPy model written from the
reference's and g2o's sources (tests/lba_model.py) -- byte for byte, in both orders, on seeded worlds, hand-built cases and stop cases --
and what holds the model itself: a noise-free world is returned, the Jacobians agree with central differences, the Schur step solves the
full damped system, the controller and lm_step take the same decisions."""
import math
import numpy as np
import pytest

import multi_orb_slam_amd as m
import lba_model as lm
import lba_worlds as lw

ORDERS = {"index": m.POSE_ORDER_INDEX, "device": m.POSE_ORDER_DEVICE}
_runs = {}


def same(H, M, what):
    for k in lm.Result.FIELDS:
        a, b = getattr(H, k), getattr(M, k)
        if isinstance(a, np.ndarray):
            b = np.asarray(b)
            assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
            assert a.tobytes() == b.tobytes(), (what, k, int((a != b).sum()) if a.dtype.names is None else (a, b))
        else:
            assert a == b, (what, k, a, b)


def both(W, order, stop=None, key=None):
    """The host routine and the model on one world -> (library's result, model's result); the seeded worlds are run once per order."""
    if key is not None and (key, order) in _runs:
        return _runs[(key, order)]
    H = m.local_ba_host(lw.to_problem(m, W), ORDERS[order], stop=stop)
    M = lm.optimize(W, order, stop=stop)
    if key is not None:
        _runs[(key, order)] = (H, M)
    return H, M


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("name", list(lw.WORLDS))
def test_host_routine_equals_the_model_byte_for_byte(name, order):
    H, M = both(lw.world(name), order, key=name)
    same(H, M, (name, order))
    lw.check_band(M)
    f, x, n = lw.WORLDS[name][:3]
    assert H.pose.shape == (f + x, 7) and H.point.shape == (n, 3) and H.ended == 0 and H.optimisations == 2
    assert H.active_poses[0] == f or n < 3 * f


def test_the_worlds_cover_what_they_are_meant_to():
    sizes = {lw.WORLDS[n][:2] for n in lw.WORLDS}
    assert {(1, 0), (2, 1), (7, 5), (20, 12), (64, 40)} <= sizes and any(f == m.LBA_MAX_FREE + 1 for f, _ in sizes)
    assert min(v[2] for v in lw.WORLDS.values()) == 1 and max(v[2] for v in lw.WORLDS.values()) == 3000
    assert {v[4] for v in lw.WORLDS.values()} == {"mono", "stereo", "mixed"} and {v[5] for v in lw.WORLDS.values()} == {0.0, 0.1, 0.4}
    assert {v[6] for v in lw.WORLDS.values()} == {"exact", "near", "off"}
    W = lw.world("f7_x5_p3000_mixed_wrong10")
    assert set(np.unique(W["edge_cam"])) == {0, 1} and (W["obs"][:, 2] < 0).any() and (W["obs"][:, 2] >= 0).any()
    deg = np.diff(W["first"])
    assert deg.min() <= 1 and deg.max() == 12


@pytest.mark.parametrize("name", list(lw.WORLDS))
def test_the_two_orders_agree_on_every_flag_and_counter(name, capsys):
    (Hi, _), (Hd, _) = both(lw.world(name), "index", key=name), both(lw.world(name), "device", key=name)
    assert np.array_equal(Hi.flags, Hd.flags)
    for k in ("ended", "optimisations", "polls", "n_level1", "n_erase", "active_poses", "active_points", "active_edges"):
        assert getattr(Hi, k) == getattr(Hd, k), k
    assert np.array_equal(Hi.rounds["iterations"], Hd.rounds["iterations"]) and np.array_equal(Hi.rounds["trials"], Hd.rounds["trials"])
    with capsys.disabled():
        print("\n[lba] %s: largest pose difference between the orders %.3g, largest point difference %.3g"
              % (name, float(np.abs(Hi.pose - Hd.pose).max()), float(np.abs(Hi.point - Hd.point).max())))


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("name", list(lw.hand_cases()))
def test_hand_built_cases(name, order):
    W, expect = lw.hand_cases()[name]
    H, M = both(W, order, stop=10 ** 9)
    same(H, M, (name, order))
    assert all(getattr(H, k) == v for k, v in expect.items()) if isinstance(expect, dict) else expect(H)
    if name == "zero_pivot":
        assert M.trace.solve_failed >= 1 and "qmax" in M.trace.exits
    if name == "depth_zero_in_camera_1":
        assert any(z.size and (z == 0.0).any() for _, z, _ in M.trace.tests)
    if name == "seen_once_and_fixed_only":
        deg = np.diff(W["first"])
        fixed_only = [l for l in range(len(deg)) if deg[l] and (W["edge_pose"][W["first"][l]:W["first"][l + 1]] >= W["n_free"]).all()]
        assert (deg == 1).any() and fixed_only
        assert not np.array_equal(H.point[fixed_only[0]], W["points"][fixed_only[0]].astype(np.float64))   # it is optimised all the same


def test_a_zero_pivot_fails_the_factorisation():
    """An EXACT zero pivot, in the library's factorisation (orbm_lba_ldlt: the routine the host route runs, statement for statement the
    one k_lba_solve runs) and in the model's.  A whole problem reaches a failing pivot only as a non-finite one (hand case zero_pivot):
    lambda is added to every diagonal entry, so an exact 0 needs lambda = 0, and that needs a system of zeros."""
    H = np.diag([2.0, 0.0, 3.0])
    assert lm.ldlt_solve(H, np.ones(3)) is None and m.lba_ldlt(H, np.ones(3)) is None
    H = np.array([[4.0, 2.0], [2.0, 1.0]])        # the second pivot is 1 - 0.5 * (4 * 0.5) = 0
    assert lm.ldlt_solve(H, np.ones(2)) is None and m.lba_ldlt(H, np.ones(2)) is None
    for bad in (np.inf, np.nan):
        H = np.array([[4.0, 2.0], [2.0, bad]])
        assert lm.ldlt_solve(H, np.ones(2)) is None and m.lba_ldlt(H, np.ones(2)) is None
    rng = np.random.RandomState(9)
    for n in (1, 6, 13, 60, 384):                 # ... and where it succeeds the two give the same bytes
        A = rng.uniform(-1, 1, (n, n)); H = A @ A.T + n * np.eye(n); b = rng.uniform(-1, 1, n)
        x, xm = m.lba_ldlt(H, b), lm.ldlt_solve(H, b)
        assert x is not None and x.tobytes() == xm.tobytes(), n
        assert np.abs(H @ x - b).max() <= 1e-10


@pytest.mark.parametrize("name", list(lw.stop_cases()))
def test_stop_cases(name):
    W, n, ended, exit_, polls = lw.stop_cases()[name]
    for order in ORDERS:
        H, M = both(W, order, stop=n)
        same(H, M, (name, order))
        assert H.ended == ended and H.polls == polls
        assert exit_ is None or exit_ in M.trace.exits
    if name == "at_poll_0":
        assert H.polls == 1 and not H.flags.any() and H.optimisations == 0
        assert np.array_equal(H.point_f, W["points"])                      # nothing moved
    if name == "after_optimize_5":
        assert H.polls == n + 1 and H.rounds["iterations"].tolist() == [5, 0] and H.n_level1 == 0 and H.n_erase > 0


def test_every_exit_of_the_levenberg_loop_is_reached():
    seen = set()
    for name in lw.WORLDS:
        seen |= set(both(lw.world(name), "index", key=name)[1].trace.exits)
    for name, (W, _) in lw.hand_cases().items():
        seen |= set(lm.optimize(W, "index", stop=10 ** 9).trace.exits)
    for name, (W, n, _, _, _) in lw.stop_cases().items():
        seen |= set(lm.optimize(W, "index", stop=n).trace.exits)
    assert seen >= {"accepted", "qmax", "rho0", "three_bad", "max_iter", "stopped", "stop_376"}, seen


# ---- what holds the model ----------------------------------------------------------------------------------------------------------------
def _system(W, lam):
    """The linearised system of the model at the start of W: (G, sums and blocks, hessian indices)."""
    G = lm.Graph(W)
    poses = np.zeros((G.n_poses, 7))
    for p in range(G.n_poses):
        T = lm.SE3.from_cv(G.Tcw[p]); poses[p] = T.q + T.t
    points = np.asarray(W["points"], np.float64)
    act = np.arange(G.n_edges)
    ev = lm.edge_pass(G, poses, points, act, True)
    robust = np.ones(G.n_edges, bool)
    bl_e, Hll_e, bp_e, Hpp_e, Hpl_e, rho0 = lm.quadratic_form(G, ev, robust)
    pose_h = np.full(G.n_poses, -1); free = np.unique(G.edge_pose[G.edge_pose < G.n_free]); pose_h[free] = np.arange(len(free))
    na, nl = len(free), G.n_points
    assert (np.diff(G.first) > 0).all()
    eh = pose_h[G.edge_pose]; fe = np.nonzero(eh >= 0)[0]
    Hll, bl = lm.ranked_sum(Hll_e, G.edge_point, nl), lm.ranked_sum(bl_e, G.edge_point, nl)
    Hpp, bp = lm.ranked_sum(Hpp_e[fe], eh[fe], na), lm.ranked_sum(bp_e[fe], eh[fe], na)
    return G, ev, (Hll, bl, Hpp, bp, Hpl_e[fe], eh[fe], G.edge_point[fe], na, nl)


def test_the_schur_step_solves_the_full_damped_system():
    W = lw.make_world(4, 2, 50, 31, "mixed", 0.0, "near", 5)
    G, _, S = _system(W, None)
    Hll, bl, Hpp, bp, Bi, eh, lm_of, na, nl = S
    md = max(np.abs(Hpp[:, range(6), range(6)]).max(), np.abs(Hll[:, range(3), range(3)]).max())
    for lam in (1e-5 * md, 1e-2 * md):
        xp, xl, _, _ = lm.schur_solve(*S, lam)
        n = 6 * na
        F = np.zeros((n + 3 * nl, n + 3 * nl))
        for a in range(na):
            F[6 * a:6 * a + 6, 6 * a:6 * a + 6] = Hpp[a]
        for l in range(nl):
            F[n + 3 * l:n + 3 * l + 3, n + 3 * l:n + 3 * l + 3] = Hll[l]
        for k in range(len(eh)):
            r, c = 6 * eh[k], n + 3 * lm_of[k]
            F[r:r + 6, c:c + 3] = Bi[k]; F[c:c + 3, r:r + 6] = Bi[k].T
        F = np.triu(F) + np.triu(F, 1).T                # the solver reads the upper triangle
        F[np.diag_indices_from(F)] += lam
        b = np.concatenate([bp.reshape(-1), bl.reshape(-1)])
        want = np.linalg.solve(F, b)
        got = np.concatenate([xp, xl])
        # both are backward-stable solutions of F x = b: each is off the exact one by at most c(N) * eps * cond(F) * |x| with a modest
        # growth constant; c(N) = N covers elimination without pivoting on a positive definite matrix (no growth) and LAPACK's LU
        cond = np.linalg.cond(F)
        N = len(b)
        bound = 2 * N * np.finfo(np.float64).eps * cond * np.linalg.norm(want)
        err = np.linalg.norm(got - want)
        print("[lba] Schur step against numpy.linalg.solve: N = %d, cond = %.3g, |x| = %.3g, error %.3g, bound %.3g" % (N, cond, np.linalg.norm(want), err, bound))
        assert err <= bound
        assert np.linalg.norm(F @ got - b) <= 2 * N * np.finfo(np.float64).eps * (np.linalg.norm(F, 2) * np.linalg.norm(got) + np.linalg.norm(b))


def test_all_four_jacobians_agree_with_central_differences():
    """Both Jacobians of both edge types.  The stereo edge's error passes through `const float invz`, so it is a staircase of steps up
    to 2^-24 |value| with |value| < 1024 px: a central difference over 2 h carries 2 * 2^-25 * 1024 / (2 h) of it per evaluation pair,
    and h^2 / 6 times a third derivative (at most 6 f / z times (lever / z)^3 <= 6 * 505 / 4 * (9 / 4)^3 < 1e4) of truncation."""
    rng = np.random.RandomState(7)
    Tcim = lw.tcim_pair()
    K5 = np.array([lw.FX, lw.FY, lw.CX, lw.CY, lw.BF], np.float32)
    h = 1e-3
    bound = 2.0 ** -24 * 1024 / h + h * h / 6 * 1e4
    worst = 0.0
    for stereo in (False, True):
        for cam in (0, 1):
            for _ in range(5):
                q = np.array([0.02, -0.03, 0.01, 1.0]) + rng.uniform(-0.01, 0.01, 4); q /= np.linalg.norm(q)
                pose = np.concatenate([q, rng.uniform(-0.5, 0.5, 3)])
                X = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(4, 8)])
                obs = np.array([300.0, 200.0, 290.0 if stereo else -1.0], np.float32)
                e0, chi2, zc, A, B = m.lba_edge_eval(Tcim, K5, pose, X, cam, obs, 0.5)
                D = 3 if stereo else 2
                assert zc > 0 and abs(chi2 - 0.5 * float(e0[:D] @ e0[:D])) <= 1e-12 * chi2 and np.abs(e0).max() < 1024
                assert np.abs(A[:D]).max() > 10 and np.abs(B[:D]).max() > 100          # the entries the bound is small against
                for k in range(3):                                 # by the point: _estimate += v
                    d = np.zeros(3); d[k] = h
                    num = (m.lba_edge_eval(Tcim, K5, pose, X + d, cam, obs, 0.5)[0] - m.lba_edge_eval(Tcim, K5, pose, X - d, cam, obs, 0.5)[0]) / (2 * h)
                    worst = max(worst, float(np.abs(num[:D] - A[:D, k]).max()))
                for k in range(6):                                 # by the pose: exp(x) * estimate
                    errs = []
                    for sg in (1.0, -1.0):
                        u = [0.0] * 6; u[k] = sg * h
                        dT, _ = lm.SE3.exp(u, "index")
                        T = dT * lm.raw_se3(pose[:4], pose[4:])
                        errs.append(m.lba_edge_eval(Tcim, K5, np.array(T.q + T.t), X, cam, obs, 0.5)[0])
                    num = (errs[0] - errs[1]) / (2 * h)
                    worst = max(worst, float(np.abs(num[:D] - B[:D, k]).max()))
                if not stereo:
                    assert not A[2].any() and not B[2].any() and e0[2] == 0.0
    print("[lba] Jacobians against central differences: worst absolute difference %.3g, bound %.3g" % (worst, bound))
    assert worst <= bound


def test_the_jacobians_of_the_double_path_agree_tightly():
    """The mono edge has no float step: its Jacobians agree with central differences to rounding, eps |e| / h + h^2."""
    rng = np.random.RandomState(8)
    Tcim = lw.tcim_pair(); K5 = np.array([lw.FX, lw.FY, lw.CX, lw.CY, lw.BF], np.float32)
    worst = 0.0
    for cam in (0, 1):
        for _ in range(10):
            q = np.array([0.02, -0.03, 0.01, 1.0]) + rng.uniform(-0.01, 0.01, 4); q /= np.linalg.norm(q)
            pose = np.concatenate([q, rng.uniform(-0.5, 0.5, 3)]); X = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(4, 8)])
            obs = np.array([300.0, 200.0, -1.0], np.float32)
            _, _, _, A, B = m.lba_edge_eval(Tcim, K5, pose, X, cam, obs, 1.0)
            h = 1e-5
            for k in range(3):
                d = np.zeros(3); d[k] = h
                num = (m.lba_edge_eval(Tcim, K5, pose, X + d, cam, obs, 1.0)[0] - m.lba_edge_eval(Tcim, K5, pose, X - d, cam, obs, 1.0)[0]) / (2 * h)
                worst = max(worst, float(np.abs(num[:2] - A[:2, k]).max()))
            for k in range(6):
                errs = []
                for sg in (1.0, -1.0):
                    u = [0.0] * 6; u[k] = sg * h
                    dT, _ = lm.SE3.exp(u, "index"); T = dT * lm.raw_se3(pose[:4], pose[4:])
                    errs.append(m.lba_edge_eval(Tcim, K5, np.array(T.q + T.t), X, cam, obs, 1.0)[0])
                worst = max(worst, float(np.abs(((errs[0] - errs[1]) / (2 * h))[:2] - B[:2, k]).max()))
    # |e| <= 500 px: rounding 2^-52 * 500 / 1e-5 = 1.1e-8 per evaluation pair; truncation h^2 / 6 * |third derivative| <= 1e-10 * 1e3
    assert worst <= 1e-6, worst


def test_a_noise_free_world_is_returned_within_the_rounding_of_its_inputs():
    W = lw.make_world(3, 2, 60, 41, "stereo", 0.0, "exact", 5, noise=False)
    H = m.local_ba_host(lw.to_problem(m, W), m.POSE_ORDER_INDEX)
    assert H.ended == 0 and H.n_level1 == 0 and H.n_erase == 0
    # The observations are the projections of the float truth, rounded to float: each is off by at most half an ulp of a value below
    # 1024, delta = 2^-14.  The minimiser of the whitened residuals moves from the truth by at most |J^+| |r| to first order, with
    # |r| <= sqrt(n_residuals) * delta * sqrt(max weight) and |J^+| = 1 / sigma_min(J), J the Jacobian at the truth over the free
    # unknowns; twice that covers the second order and the Levenberg iteration stopping short (it starts AT the truth).
    G, ev, S = _system(W, None)
    na, nl = S[7], S[8]
    assert float(np.max(np.abs(W["obs"]))) < 1024
    delta = 2.0 ** -14
    rows = []
    sw = np.sqrt(G.w)
    for e in range(G.n_edges):
        for k in range(3):
            row = np.zeros(6 * na + 3 * nl)
            p, l = G.edge_pose[e], G.edge_point[e]
            if p < G.n_free:
                row[6 * p:6 * p + 6] = [ev["B"][k][c][e] for c in range(6)]
            row[6 * na + 3 * l:6 * na + 3 * l + 3] = [ev["A"][k][c][e] for c in range(3)]
            rows.append(row * sw[e])
    J = np.array(rows)
    smin = np.linalg.svd(J, compute_uv=False)[-1]
    bound = 2 * math.sqrt(len(rows)) * delta * float(sw.max()) / smin
    dp = np.abs(H.point - W["truth"]["points"].astype(np.float64)).max()
    print("[lba] noise-free world: sigma_min %.3g, bound %.3g, largest point error %.3g" % (smin, bound, dp))
    assert dp <= bound
    # a pose: its matrix entries move by at most |xi| (1 + |t|) for an update xi, plus the float rounding of toCvMat
    T = H.Tcw.reshape(-1, 4, 4).astype(np.float64); T0 = W["truth"]["Tcw"].astype(np.float64)
    tmax = 1.0 + np.abs(T0[:, :3, 3]).max()
    assert np.abs(T - T0).max() <= bound * tmax + 2.0 ** -24 * tmax
    nf = W["n_free"]
    assert np.abs(T[nf:] - T0[nf:]).max() <= 2.0 ** -23 * tmax          # fixed poses: only toSE3Quat / toCvMat's rounding


def test_the_controller_and_lm_step_take_the_same_decisions():
    rng = np.random.RandomState(3)
    steps = 0
    verdicts = set()
    for trial in range(200):
        n = 60
        kind = trial % 4
        chi = np.empty(n)
        v = 1000.0 * rng.uniform(0.5, 2.0)
        for k in range(n):
            if kind == 0:
                v = v * rng.uniform(0.3, 1.0)                    # mostly accepted
            elif kind == 1:
                v = v * rng.uniform(0.9, 1.3)                    # mixed
            elif kind == 2:
                v = v * rng.uniform(0.999, 1.0005)               # stalls: three bad steps
            else:
                v = v * rng.uniform(1.0, 1.5)                    # rejected until qmax
            chi[k] = v
        if trial % 17 == 0:
            chi[5:9] = chi[4]                                    # rho == 0
        h = rng.uniform(1.0, 100.0, 6); b = rng.uniform(-10.0, 10.0, 6)
        for order in (m.POSE_ORDER_INDEX, m.POSE_ORDER_DEVICE):
            a, l = m.lba_controller_trace(chi, h, b, 5 + 5 * (trial % 2), order)
            assert a.tobytes() == l.tobytes(), (trial, order, a, l)
            steps += len(a)
            verdicts |= set(a[:, 2].tolist())
            assert a[-1, 2] == 3.0 or len(a) == n
    assert verdicts == {1.0, 2.0, 3.0} and steps > 2000
