"""A float64 model of Optimizer::BundleAdjustment (reference src/Optimizer.cc:47-330) from its graph on: ONE initializeOptimization(), ONE
optimize(nIterations) of g2o's Levenberg algorithm, the Huber kernels on every edge or on none, no chi-square test and no second
optimisation; the stop flag is polled where g2o polls it (core/sparse_optimizer.cpp:376, optimization_algorithm_levenberg.cpp:149) and
nowhere else.  Written from the g2o sources like tests/lba_model.py, whose per-edge columns (edge_pass, quadratic_form), per-vertex sums
(ranked_sum), Schur step (schur_solve) and chi2 orders (total_chi2, robust_chi2) it reuses; its own are the sequence and the solver of
the reduced system, ba_ldlt: the local BA's factorisation and forward substitution, the backward substitution summed in DESCENDING j.

order="index" / "device": as in lba_model."""
import math
import numpy as np

import lba_model as lm
from lba_model import SE3, raw_se3, quat_to_matrix, canonical, DBL_MAX, ROUND_DTYPE


class Result:
    FIELDS = ("pose", "Tcw", "point", "point_f", "round", "optimised", "polls", "active_poses", "active_points", "active_edges")


def ba_ldlt(H, b):
    """The dense LDL^T without pivoting: H n x n (its upper triangle is read), -> x or None on a zero or non-finite pivot.  Backward:
    s = 0; for j = n-1 .. i+1: s += L(j, i) y_j; x_i = y_i - s."""
    n = len(b)
    L = np.zeros((n, n)); d = np.zeros(n)
    for k in range(n):
        temp = d[:k] * L[k, :k]
        prods = L[k:, :k] * temp
        sums = np.add.accumulate(np.concatenate([np.zeros((n - k, 1)), prods], axis=1), axis=1)[:, -1]
        dk = H[k, k] - sums[0]
        if not (abs(dk) > 0) or not (abs(dk) <= DBL_MAX):
            return None
        d[k] = dk
        L[k + 1:, k] = (H[k, k + 1:] - sums[1:]) / dk
    y = np.zeros(n)
    for i in range(n):
        y[i] = b[i] - np.add.accumulate(np.concatenate([[0.0], L[i, :i] * y[:i]]))[-1]
    y = y / d
    for i in range(n - 1, -1, -1):
        y[i] = y[i] - np.add.accumulate(np.concatenate([[0.0], (L[i + 1:, i] * y[i + 1:])[::-1]]))[-1]
    return y


def schur_solve(*args):
    """lba_model's Schur step with the reduced system handed to ba_ldlt instead of its own solver (the one name it looks up)."""
    keep = lm.ldlt_solve
    lm.ldlt_solve = ba_ldlt
    try:
        return lm.schur_solve(*args)
    finally:
        lm.ldlt_solve = keep


def start(G, W):
    poses = np.zeros((G.n_poses, 7))
    for p in range(G.n_poses):
        T = SE3.from_cv(G.Tcw[p])
        poses[p] = T.q + T.t
    return poses, np.asarray(W["points"], np.float32).reshape(-1, 3).astype(np.float64)


def chi2_at(W, pose7, points, robust, order="index"):
    """activeRobustChi2 of the whole graph at the given estimates (pose7: n_poses x 7, points: n_points x 3)."""
    G = lm.Graph(W)
    act = np.arange(G.n_edges)
    ev = lm.edge_pass(G, np.asarray(pose7, np.float64), np.asarray(points, np.float64), act, False)
    return lm.total_chi2(G, act, lm.robust_chi2(G, ev, np.full(G.n_edges, bool(robust))), order)


def optimize(W, iterations, robust, order="index", stop=None, trace=None):
    """-> Result.  stop: None (no flag), a callable, or an int n: true from the n-th poll on."""
    G = lm.Graph(W)
    tr = trace if trace is not None else lm.Trace()
    polls = [0]
    if stop is None:
        poll = lambda: False
    else:
        fn = stop if callable(stop) else (lambda: polls[0] > int(stop))

        def poll():
            polls[0] += 1
            return bool(fn())
    poses, points = start(G, W)
    x = np.zeros(6 * G.n_free + 3 * G.n_points)
    R = Result()
    R.round = np.zeros(1, ROUND_DTYPE)
    rnd = R.round[0]
    # initializeOptimization(): every edge is at level 0; a vertex without an edge is not active
    act = np.arange(G.n_edges)
    ep, el = G.edge_pose, G.edge_point
    pose_h = np.full(G.n_poses, -1); point_h = np.full(G.n_points, -1)
    free_with_edge = np.unique(ep[ep < G.n_free])
    pose_h[free_with_edge] = np.arange(len(free_with_edge))
    pts_with_edge = np.unique(el)
    point_h[pts_with_edge] = np.arange(len(pts_with_edge))
    na, nl = len(free_with_edge), len(pts_with_edge)
    R.active_poses, R.active_points, R.active_edges = na, nl, G.n_edges
    R.optimised = 1 if na + nl > 0 else 0
    rob = np.full(G.n_edges, bool(robust))
    if na + nl > 0:
        n = 6 * na
        eh = pose_h[ep]
        fe = np.nonzero(eh >= 0)[0]
        lam, ni, n_bad_steps = 0.0, 2.0, 0
        ok = True
        i = 0
        while i < iterations:                   # for (int i=0; i<iterations && ! terminate() && ok; i++)
            if poll():
                tr.exits.append("stop_376")
                break
            if not ok:
                break
            ev = lm.edge_pass(G, poses, points, act, True)
            bl_e, Hll_e, bp_e, Hpp_e, Hpl_e, rho0 = lm.quadratic_form(G, ev, rob)
            current_chi = lm.total_chi2(G, act, rho0, order)
            ini_chi = current_chi
            Hll = lm.ranked_sum(Hll_e, point_h[el], nl); bl = lm.ranked_sum(bl_e, point_h[el], nl)
            Hpp = lm.ranked_sum(Hpp_e[fe], eh[fe], na); bp = lm.ranked_sum(bp_e[fe], eh[fe], na)
            if i == 0:                          # computeLambdaInit: `v > max` never takes a NaN
                md = 0.0
                for v in list(np.abs(Hpp[:, range(6), range(6)]).ravel()) + list(np.abs(Hll[:, range(3), range(3)]).ravel()):
                    if v > md:
                        md = float(v)
                lam, ni, n_bad_steps = 1e-5 * md, 2.0, 0
            qmax = 0
            rho = 0.0
            stopped = False
            while True:
                sol = schur_solve(Hll, bl, Hpp, bp, Hpl_e[fe], eh[fe], point_h[el[fe]], na, nl, lam)
                ok2 = sol is not None
                if ok2:
                    x[:n] = sol[0]
                    x[n:n + 3 * nl] = sol[1]
                else:
                    tr.solve_failed += 1
                t_poses, t_points = poses.copy(), points.copy()
                for a, p in enumerate(free_with_edge):
                    d, _ = SE3.exp([float(v) for v in x[6 * a:6 * a + 6]], order)
                    T = d * raw_se3(poses[p, :4], poses[p, 4:])
                    t_poses[p] = T.q + T.t
                t_points[pts_with_edge] = points[pts_with_edge] + x[n:n + 3 * nl].reshape(nl, 3)
                ev_t = lm.edge_pass(G, t_poses, t_points, act, False)
                temp_chi = lm.total_chi2(G, act, lm.robust_chi2(G, ev_t, rob), order)
                if not ok2:
                    temp_chi = DBL_MAX
                rho = current_chi - temp_chi
                bfull = np.concatenate([bp.reshape(-1), bl.reshape(-1)])
                xv = x[:n + 3 * nl]
                with np.errstate(all="ignore"):
                    scale = float(np.add.accumulate(np.concatenate([[0.0], xv * (lam * xv + bfull)]))[-1])   # computeScale
                scale += 1e-3
                rho /= scale
                tr.trials.append((0, i, lam, rho, ok2))
                if rho > 0 and abs(temp_chi) <= DBL_MAX:
                    u = 2 * rho - 1
                    cube = math.pow(u, 3) if order == "index" else u * u * u
                    alpha = 1. - cube
                    alpha = min(alpha, 2. / 3.)
                    lam *= max(1. / 3., alpha)
                    ni = 2.0
                    current_chi = temp_chi
                    poses, points = t_poses, t_points
                else:
                    lam *= ni
                    ni *= 2
                qmax += 1
                rnd["trials"] += 1
                if not (rho < 0 and qmax < 10):
                    break
                if poll():
                    stopped = True
                    break
            rnd["iterations"] += 1
            terminate = qmax == 10 or rho == 0
            tr.exits.append("stopped" if stopped else "qmax" if qmax == 10 else "rho0" if rho == 0 else "accepted")
            if not terminate:
                n_bad_steps = n_bad_steps + 1 if (ini_chi - current_chi) * 1e3 < ini_chi else 0
                if n_bad_steps >= 3:
                    terminate = True
                    tr.exits.append("three_bad")
            ok = not terminate
            rnd["chi2"], rnd["lambda"] = canonical(current_chi), canonical(lam)
            i += 1
    # Converter::toCvMat
    R.pose = np.array([[canonical(float(v)) for v in row] for row in poses]).reshape(G.n_poses, 7)
    R.Tcw = np.zeros((G.n_poses, 16), np.float32)
    for p in range(G.n_poses):
        Rm = quat_to_matrix([float(v) for v in poses[p, :4]])
        M = np.zeros((4, 4), np.float32)
        with np.errstate(all="ignore"):
            for r in range(3):
                for c in range(3):
                    M[r, c] = np.float32(Rm[r][c])
                M[r, 3] = np.float32(poses[p, 4 + r])
        M[3, 3] = 1.0
        R.Tcw[p] = M.reshape(16)
    R.point = points.reshape(G.n_points, 3).copy()
    with np.errstate(all="ignore"):
        R.point_f = R.point.astype(np.float32)
    R.polls = polls[0]
    R.trace = tr
    return R
