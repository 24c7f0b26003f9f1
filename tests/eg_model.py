"""A float64 model of Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:1373-1677) from its graph on and of the parts of g2o it
runs, written from the reference's and g2o's sources (Thirdparty/g2o/g2o/types/sim3.h, types/se3_ops.hpp, types/types_seven_dof_expmap.
{h,cpp}, core/base_binary_edge.hpp, core/block_solver.hpp, core/optimization_algorithm_levenberg.cpp, core/sparse_optimizer.cpp) and from
Eigen's published sources for the operators those call -- not from csrc/essgraph.hip: the loops below are g2o's nested loops (optimize ->
solve -> trials) over Python objects, every edge perturbs its vertices through oplus as BaseBinaryEdge::linearizeOplus does, and the
system is one dense matrix the edges add their blocks to in insertion order.

Sim3, its exponential and oplus are tests/sim3opt_model.py's (the same g2o class); the solver of the linear system is tests/gba_model.py's
ba_ldlt (the stated deviation: dense, no pivoting), the summation tree tests/lba_model.py's.

order="index":  the C library's log / acos / sin / cos / exp / pow, chi2 and computeScale summed sequentially.
order="device": poly_log, poly_acos, poly_sincos, poly_exp, the cube by multiplication; chi2 over edge positions 256 k .. 256 k + 255
                through the tree, the partials in ascending k, and computeScale's terms over the positions of x the same way.

rules: the deliberately WRONG, tidy-minded alternatives that tests/test_eg_model.py shows to change bytes:
    "perturb_fixed_scale" linearizeOplus steps along the scale although it is fixed (oplusImpl's `update[6] = 0` taken as a matter of
                          the solver's update alone): column 6 of the Jacobians is then not 0
    "skip_unreferenced"   a point without a reference vertex keeps its float position instead of going through two identities (a
                          coordinate of -0.0 comes back as +0.0 from them)
    "touch_inactive"      a vertex without an edge is written back normalised instead of as it came
and one that CANNOT change a byte, kept so that the test says so: "scale_before_update", computeScale reading the solver's x before
update(x) zeroed every seventh entry.  With column 6 of every Jacobian exactly 0, row 6 of every block is (0 .. lambda .. 0 | +-0), so
x[6] is +-0 before the zeroing and its term of computeScale is +0 either way."""
import math
import numpy as np

from pose_model import quat_to_matrix, poly_sincos, canonical, DBL_MAX, LANES, ROUND_DTYPE
from sim3_model import atan2_device
from sim3opt_model import Sim3, oplus, EPS
from lba_model import tree_partial
from gba_model import ba_ldlt

RULES = ("perturb_fixed_scale", "skip_unreferenced", "touch_inactive")
DELTA = 1e-9
SCALAR = 1.0 / (2 * DELTA)
LAMBDA_INIT = 1e-16
I7 = np.eye(7)


class Result:
    FIELDS = ("estimate", "Tiw", "point_f", "round", "optimised", "active_vertices", "active_edges")


# ---- the logarithm and arc cosine of the device order ---------------------------------------------------------------------------------
def poly_log(x):
    """x = 2^k m with m in [sqrt(1/2), sqrt(2)), z = (m - 1) / (m + 1), log m = 2 z (1 + z^2/3 + ... + z^22/23), a two-part ln 2."""
    if x != x or x < 0:
        return float("nan")
    if x == 0:
        return float("-inf")
    if x == float("inf"):
        return x
    sqrt2, sqrt1_2 = 1.41421356237309514547e+00, 7.07106781186547572737e-01
    ln2_hi, ln2_lo = 6.93147180369123816490e-01, 1.90821492927058770002e-10
    k = 0
    while x >= sqrt2:
        x = x * 0.5
        k += 1
    while x < sqrt1_2:
        x = x * 2.0
        k -= 1
    z = (x - 1.0) / (x + 1.0)
    w = z * z
    p = 1.0 / 23
    for d in (21, 19, 17, 15, 13, 11, 9, 7, 5, 3):
        p = p * w + (1.0 / d)
    kf = float(k)
    return kf * ln2_hi + ((2.0 * z + (2.0 * z) * (w * p)) + kf * ln2_lo)


def poly_acos(d):
    return atan2_device(math.sqrt((1.0 - d) * (1.0 + d)), d)


# ---- Eigen: Matrix3d::lu().solve (PartialPivLU, UNPINNED) ----------------------------------------------------------------------------
def lu3_solve(W, b):
    W = [list(r) for r in W]
    r = list(b)
    for k in range(3):
        row, big = k, abs(W[k][k])
        for i in range(k + 1, 3):
            if abs(W[i][k]) > big:
                row, big = i, abs(W[i][k])
        if big != 0.0:
            if row != k:
                W[k], W[row] = W[row], W[k]
                r[k], r[row] = r[row], r[k]
            for i in range(k + 1, 3):
                W[i][k] = W[i][k] / W[k][k]
        for i in range(k + 1, 3):
            for c in range(k + 1, 3):
                W[i][c] = W[i][c] - W[i][k] * W[k][c]
    r[1] = r[1] - W[1][0] * r[0]
    r[2] = r[2] - (W[2][0] * r[0] + W[2][1] * r[1])
    x2 = r[2] / W[2][2]
    x1 = (r[1] - W[1][2] * x2) / W[1][1]
    x0 = (r[0] - (W[0][1] * x1 + W[0][2] * x2)) / W[0][0]
    return [x0, x1, x2]


def _div(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        with np.errstate(all="ignore"):
            return float(np.float64(a) / np.float64(b))


def _sqrt(a):
    return math.sqrt(a) if a >= 0 else float("nan")


def sim3_log(T, order, branches=None):
    """Sim3::log() -> (7 values, branch)."""
    if order == "index":
        s = T.s
        sigma = math.log(s) if s > 0 and s != float("inf") else poly_log(s)
        acos = lambda d: math.acos(d) if -1 <= d <= 1 else float("nan")
        sincos = lambda a: (math.sin(a), math.cos(a)) if abs(a) != float("inf") and a == a else (float("nan"), float("nan"))
    else:
        sigma = poly_log(T.s)
        acos = poly_acos
        sincos = lambda a: poly_sincos(a) if a == a and abs(a) != float("inf") else (float("nan"), float("nan"))
    s = T.s
    R = quat_to_matrix(T.q)
    d = 0.5 * (R[0][0] + R[1][1] + R[2][2] - 1)
    dR = [R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]]
    near = d > 1 - EPS
    if abs(sigma) < EPS:
        C = 1
        if near:
            branch = 0
            omega = [0.5 * v for v in dR]
            A, B = 1. / 2., 1. / 6.
        else:
            branch = 1
            theta = acos(d)
            theta2 = theta * theta
            f = _div(theta, 2 * _sqrt(1 - d * d))
            omega = [f * v for v in dR]
            sn, cs = sincos(theta)
            A = _div(1 - cs, theta2)
            B = _div(theta - sn, theta2 * theta)
    else:
        C = _div(s - 1, sigma)
        if near:
            branch = 2
            sigma2 = sigma * sigma
            omega = [0.5 * v for v in dR]
            A = _div((sigma - 1) * s + 1, sigma2)
            B = _div((0.5 * sigma2 - sigma + 1) * s, sigma2 * sigma)
        else:
            branch = 3
            theta = acos(d)
            f = _div(theta, 2 * _sqrt(1 - d * d))
            omega = [f * v for v in dR]
            theta2 = theta * theta
            sn, cs = sincos(theta)
            a = s * sn
            b = s * cs
            c = theta2 + sigma * sigma
            A = _div(a * sigma + (1 - b) * theta, theta * c)
            B = _div((C - _div((b - 1) * sigma + a * theta, c)) * 1., theta2)
    if branches is not None:
        branches.add("sim3_log_%d" % branch)
    O = [[0.0, -omega[2], omega[1]], [omega[2], 0.0, -omega[0]], [-omega[1], omega[0], 0.0]]
    O2 = [[O[i][0] * O[0][j] + O[i][1] * O[1][j] + O[i][2] * O[2][j] for j in range(3)] for i in range(3)]
    W = [[(A * O[i][j] + B * O2[i][j]) + C * (1.0 if i == j else 0.0) for j in range(3)] for i in range(3)]
    with np.errstate(all="ignore"):
        W = [[float(np.float64(v)) for v in row] for row in W]
    try:
        ups = lu3_solve(W, T.t)
    except ZeroDivisionError:
        ups = [float(v) for v in _lu3_np(W, T.t)]
    return omega + ups + [sigma], branch


def _lu3_np(W, b):
    """lu3_solve over NumPy scalars: a division by zero gives the infinity or NaN IEEE asks for instead of raising."""
    with np.errstate(all="ignore"):
        return lu3_solve([[np.float64(v) for v in r] for r in W], [np.float64(v) for v in b])


def as_sim3(v8):
    return Sim3([float(x) for x in v8[:4]], [float(x) for x in v8[4:7]], float(v8[7]))


def as_vec8(T):
    return list(T.q) + list(T.t) + [T.s]


def edge_error(C, v0, v1, order, branches=None):
    """EdgeSim3::computeError: (C * v0 * v1.inverse()).log()"""
    return sim3_log(C * v0 * v1.inverse(), order, branches)[0]


def seq_matmul(X, Y):
    """X (a x n) times Y (n x b): every entry the sum of its n products in ascending index, from the first product on."""
    with np.errstate(all="ignore"):
        acc = np.multiply.outer(X[:, 0], Y[0, :])
        for k in range(1, X.shape[1]):
            acc = acc + np.multiply.outer(X[:, k], Y[k, :])
    return acc


def chi2_of(e):
    e = np.asarray(e, np.float64)
    return float(seq_matmul(e[None, :], seq_matmul(I7, e[:, None]))[0, 0])


def numeric_jacobian(C, est, which, other, fix_scale, order, rules=()):
    """BaseBinaryEdge::linearizeOplus for one vertex of the edge: add_v is ONE array across the dimensions, oplus writes through it."""
    J = np.zeros((7, 7))
    add = [0.0] * 7
    for d in range(7):
        errs = []
        for step in (DELTA, -DELTA):
            add[d] = step
            p = oplus(est, add, fix_scale and "perturb_fixed_scale" not in rules, order)
            errs.append(edge_error(C, p, other, order) if which == 0 else edge_error(C, other, p, order))
        add[d] = 0.0
        with np.errstate(all="ignore"):
            J[:, d] = SCALAR * (np.array(errs[0]) - np.array(errs[1]))
    return J


def edge_eval(measurement, v0, v1, fix_scale=False, order="index"):
    """What orbm_eg_edge_eval answers -> (error, chi2, Jacobian by vertex 0, by vertex 1)."""
    C, a, b = as_sim3(measurement), as_sim3(v0), as_sim3(v1)
    e = edge_error(C, a, b, order)
    return np.array(e), chi2_of(e), numeric_jacobian(C, a, 0, b, fix_scale, order), numeric_jacobian(C, b, 1, a, fix_scale, order)


def ordered_sum(terms, order):
    terms = np.asarray(terms, np.float64)
    with np.errstate(all="ignore"):
        if order == "index":
            return float(np.add.accumulate(np.concatenate([[0.0], terms]))[-1])
        s = 0.0
        for k in range(0, len(terms), LANES):
            s += float(tree_partial(terms[k:k + LANES]))
        return float(s)


def total_chi2(C, est, ev0, ev1, order):
    return ordered_sum([chi2_of(edge_error(C[e], est[ev0[e]], est[ev1[e]], order)) for e in range(len(C))], order)


def verdict_margin(trace):
    """The smallest |currentChi - tempChi| / currentChi over the trials of a run whose solve succeeded: how far the closest verdict
    `rho > 0` was from changing."""
    m = float("inf")
    for t in trace:
        if t[0] == "trial" and t[3] < DBL_MAX and t[2] > 0:
            m = min(m, abs(t[2] - t[3]) / t[2])
    return m


def optimize(W, iterations=20, order="index", rules=(), trace=None):
    """W: dict with n_free, vertex (n x 8), measurement (m x 8), edge_v0, edge_v1, points, point_ref, fix_scale -> Result."""
    n_free, fix_scale = int(W["n_free"]), bool(W["fix_scale"])
    vertex = np.asarray(W["vertex"], np.float64).reshape(-1, 8)
    nv = len(vertex)
    C = [as_sim3(m) for m in np.asarray(W["measurement"], np.float64).reshape(-1, 8)]
    ev0 = [int(v) for v in W["edge_v0"]]
    ev1 = [int(v) for v in W["edge_v1"]]
    ne = len(C)
    est = [as_sim3(v) for v in vertex]
    # initializeOptimization(): the vertices of the edges; the hessian indices of the free ones in ascending id
    with_edge = sorted(set(ev0) | set(ev1))
    free_active = [v for v in with_edge if v < n_free]
    hidx = {v: a for a, v in enumerate(free_active)}
    na = len(free_active)
    n = 7 * na
    R = Result()
    R.round = np.zeros(1, ROUND_DTYPE)
    rnd = R.round[0]
    R.active_vertices, R.active_edges = len(with_edge), ne
    R.optimised = 1 if na > 0 else 0
    x = np.zeros(n)
    if na > 0:
        lam, ni, n_bad_steps = 0.0, 2.0, 0
        ok = True
        i = 0
        while i < iterations and ok:            # for (int i=0; i<iterations && ! terminate() && ok; i++)
            # computeActiveErrors, activeRobustChi2, buildSystem: linearizeOplus and constructQuadraticForm edge by edge
            H = np.zeros((n, n))
            b = np.zeros(n)
            chis = []
            for e in range(ne):
                v0, v1 = ev0[e], ev1[e]
                err = np.array(edge_error(C[e], est[v0], est[v1], order))
                chis.append(chi2_of(err))
                h0, h1 = hidx.get(v0, -1), hidx.get(v1, -1)
                if h0 < 0 and h1 < 0:
                    continue
                with np.errstate(all="ignore"):
                    omega_r = -seq_matmul(I7, err[:, None])
                    if h0 >= 0:
                        A = numeric_jacobian(C[e], est[v0], 0, est[v1], fix_scale, order, rules)
                        AtO = seq_matmul(A.T, I7)
                        b[7 * h0:7 * h0 + 7] += seq_matmul(A.T, omega_r)[:, 0]
                        H[7 * h0:7 * h0 + 7, 7 * h0:7 * h0 + 7] += seq_matmul(AtO, A)
                    if h1 >= 0:
                        B = numeric_jacobian(C[e], est[v1], 1, est[v0], fix_scale, order, rules)
                        if h0 >= 0:
                            if h0 > h1:         # _hessianRowMajor: the block of (to, from), written as transposed
                                H[7 * h1:7 * h1 + 7, 7 * h0:7 * h0 + 7] += seq_matmul(B.T, AtO.T)
                            else:
                                H[7 * h0:7 * h0 + 7, 7 * h1:7 * h1 + 7] += seq_matmul(AtO, B)
                        b[7 * h1:7 * h1 + 7] += seq_matmul(B.T, omega_r)[:, 0]
                        H[7 * h1:7 * h1 + 7, 7 * h1:7 * h1 + 7] += seq_matmul(seq_matmul(B.T, I7), B)
            current_chi = ordered_sum(chis, order)
            ini_chi = current_chi
            if i == 0:                          # computeLambdaInit: the user's value
                lam, ni, n_bad_steps = LAMBDA_INIT, 2.0, 0
            qmax = 0
            rho = 0.0
            diag = H[range(n), range(n)].copy()
            while True:
                Hd = H.copy()
                with np.errstate(all="ignore"):
                    Hd[range(n), range(n)] = diag + lam                 # setLambda
                    sol = ba_ldlt(Hd, b)
                ok2 = sol is not None
                if ok2:
                    x[:] = sol
                if trace is not None:
                    trace.append(("solve", i, ok2))
                x_before = x.copy()
                trial = list(est)
                for a, v in enumerate(free_active):      # update(x): oplusImpl writes update[6] = 0 into the solver's x
                    upd = [float(u) for u in x[7 * a:7 * a + 7]]
                    trial[v] = oplus(est[v], upd, fix_scale, order)
                    x[7 * a:7 * a + 7] = upd
                temp_chi = total_chi2(C, trial, ev0, ev1, order)
                if not ok2:
                    temp_chi = DBL_MAX
                rho = current_chi - temp_chi
                xs = x_before if "scale_before_update" in rules else x
                with np.errstate(all="ignore"):
                    scale = ordered_sum(xs * (lam * xs + b), order)   # computeScale
                    scale += 1e-3
                    rho /= scale
                if trace is not None:
                    trace.append(("trial", i, current_chi, temp_chi, rho))
                if rho > 0 and abs(temp_chi) <= DBL_MAX:
                    u = 2 * rho - 1
                    try:
                        cube = math.pow(u, 3) if order == "index" else u * u * u
                    except OverflowError:
                        cube = float("inf") if u > 0 else float("-inf")
                    alpha = 1. - cube
                    alpha = min(alpha, 2. / 3.)
                    lam *= max(1. / 3., alpha)
                    ni = 2.0
                    current_chi = temp_chi
                    est = trial                 # discardTop
                else:
                    lam *= ni
                    ni *= 2                     # pop
                qmax += 1
                rnd["trials"] += 1
                if not (rho < 0 and qmax < 10):
                    break
            rnd["iterations"] += 1
            terminate = qmax == 10 or rho == 0
            if trace is not None:
                trace.append(("exit", "qmax" if qmax == 10 else "rho0" if rho == 0 else "accepted"))
            if not terminate:
                n_bad_steps = n_bad_steps + 1 if (ini_chi - current_chi) * 1e3 < ini_chi else 0
                if n_bad_steps >= 3:
                    terminate = True
            ok = not terminate
            rnd["chi2"], rnd["lambda"] = canonical(current_chi), canonical(lam)
            i += 1
    # step 6: SetPose receives [R | t * (1./s)]
    R.estimate = np.zeros((nv, 8))
    R.Tiw = np.zeros((nv, 16), np.float32)
    for v in range(nv):
        T = est[v]
        if "touch_inactive" in rules and v not in with_edge:
            nq = math.sqrt(sum(c * c for c in T.q))
            T = Sim3([c / nq for c in T.q], T.t, T.s)
        R.estimate[v] = [canonical(c) for c in as_vec8(T)]
        Rm = quat_to_matrix(T.q)
        inv = _div(1., T.s)
        M = np.zeros((4, 4), np.float32)
        with np.errstate(all="ignore"):
            for r in range(3):
                for c in range(3):
                    M[r, c] = np.float32(Rm[r][c])
                M[r, 3] = np.float32(T.t[r] * inv)
        M[3, 3] = 1.0
        R.Tiw[v] = M.reshape(16)
    # step 7: correctedSwr.map(Srw.map(P)), vScw / vCorrectedSwc default-constructed where no keyframe wrote them
    pts = np.asarray(W["points"], np.float32).reshape(-1, 3)
    ref = [int(r) for r in W["point_ref"]]
    R.point_f = np.zeros((len(pts), 3), np.float32)
    for l in range(len(pts)):
        if ref[l] < 0:
            if "skip_unreferenced" in rules:
                R.point_f[l] = pts[l]
                continue
            Srw, Swr = Sim3([0., 0., 0., 1.], [0., 0., 0.], 1.), Sim3([0., 0., 0., 1.], [0., 0., 0.], 1.)
        else:
            Srw, Swr = as_sim3(vertex[ref[l]]), est[ref[l]].inverse()
        p = Swr.map(Srw.map([float(c) for c in pts[l]]))
        with np.errstate(all="ignore"):
            R.point_f[l] = np.array(p, np.float64).astype(np.float32)
    return R
