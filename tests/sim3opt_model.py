"""A float64 model of Optimizer::OptimizeSim3_cam1 (reference src/Optimizer.cc:1984-2243) and of the parts of g2o it runs, written from
the reference's and g2o's sources (Thirdparty/g2o/g2o/types/sim3.h, types/types_seven_dof_expmap.h, core/base_binary_edge.hpp,
core/robust_kernel_impl.cpp, core/optimization_algorithm_levenberg.cpp, core/sparse_optimizer.cpp, solvers/linear_solver_dense.h) and
from Eigen's published sources for the operators those call -- not from csrc/sim3opt.hip: the loops below are g2o's nested loops
(optimize -> solve -> trials), not a state machine, the edges are evaluated as NumPy columns, and the numeric Jacobian perturbs the
vertex through oplus (Sim3(update) * estimate) as BaseBinaryEdge::linearizeOplus does.

Every per-edge operation is an element-wise IEEE + - * / sqrt of float64 columns, sums over edges are explicit (np.add.accumulate is
strictly sequential), and everything that happens once per trial is Python float arithmetic with the C library's math functions.

order="index":  the sums run over the edges in the order of addEdge (e12 and e21 of correspondence 0, of 1, ...); sin, cos, exp and
                pow(., 3) from the C library.
order="device": the sums run in the device kernel's tree (256 lanes, lane l owns correspondences l, l + 256, ... in ascending order,
                e12 before e21; an xor butterfly 1 .. 32 inside each group of 64 lanes; the four groups in order); sine and cosine from
                pose_model.poly_sincos, the exponential from poly_exp below, the cube by multiplication.

rules: the deliberately WRONG, tidy-minded alternatives that tests/test_sim3opt_model.py shows to change bytes:
    "normalising_mul"      Sim3::operator* normalises the quaternion of the product
    "classify_at_estimate" the chi-square tests read the errors at the accepted estimate, not those of the last computeActiveErrors
    "carry_lambda"         the second optimize() goes on with the damping the first one ended with
    "write_on_early_return" g2oS12 is written before `return 0`"""
import math
import numpy as np

from pose_model import quat_from_matrix, quat_rotate, quat_mul, poly_sincos, canonical, DBL_MAX, LANES, ROUND_DTYPE

RESULT_DTYPE = np.dtype([("q", "<f8", (4,)), ("t", "<f8", (3,)), ("s", "<f8"), ("n_inliers", "<i4"), ("n_correspondences", "<i4"),
                         ("n_bad", "<i4"), ("n_more_iterations", "<i4"), ("written", "<i4"), ("optimisations", "<i4"),
                         ("round", ROUND_DTYPE, (2,))])
RULES = ("normalising_mul", "classify_at_estimate", "carry_lambda", "write_on_early_return")
DELTA = 1e-9
SCALAR = 1.0 / (2 * DELTA)
EPS = 0.00001


def poly_exp(x):
    """exp of the device order: the quotient by ln 2 rounded by adding and subtracting 1.5 * 2^52, a two-part ln 2, the Taylor
    polynomial to r^14 in Horner form, |k| doublings or halvings; + - * / only."""
    if x != x:
        return x
    if x > 709.782712893384:
        return float("inf")
    if x < -745.2:
        return 0.0
    inv_ln2 = 1.44269504088896338700e+00
    ln2_hi, ln2_lo = 6.93147180369123816490e-01, 1.90821492927058770002e-10
    magic = 6755399441055744.0
    kf = (x * inv_ln2 + magic) - magic
    r = (x - kf * ln2_hi) - kf * ln2_lo
    p = 1.0 / 87178291200.0
    for c in (1.0 / 6227020800.0, 1.0 / 479001600, 1.0 / 39916800, 1.0 / 3628800, 1.0 / 362880, 1.0 / 40320, 1.0 / 5040, 1.0 / 720,
              1.0 / 120, 1.0 / 24, 1.0 / 6, 1.0 / 2):
        p = p * r + c
    e = 1.0 + (r + (r * r) * p)
    k = int(kf)
    f = 0.5 if k < 0 else 2.0
    for _ in range(abs(k)):
        e = e * f
    return e


def ldlt_solve(H, b):
    """Eigen::LDLT<MatrixXd>::compute(H) (unblocked, in place over the lower triangle, pivoting on the first largest |diagonal|),
    isPositive(), solve(b) for any size -> (ok, x or None)."""
    n = len(b)
    A = [list(row) for row in H]
    tr = [0] * n
    sign = 0
    for k in range(n):
        idx, big = k, abs(A[k][k])
        for i in range(k + 1, n):
            if abs(A[i][i]) > big:
                idx, big = i, abs(A[i][i])
        tr[k] = idx
        if idx != k:
            for j in range(k):
                A[k][j], A[idx][j] = A[idx][j], A[k][j]
            for i in range(idx + 1, n):
                A[i][k], A[i][idx] = A[i][idx], A[i][k]
            A[k][k], A[idx][idx] = A[idx][idx], A[k][k]
            for i in range(k + 1, idx):
                A[i][k], A[idx][i] = A[idx][i], A[i][k]
        if k > 0:
            temp = [A[j][j] * A[k][j] for j in range(k)]
            s = 0.0
            for j in range(k):
                s += A[k][j] * temp[j]
            A[k][k] -= s
            for i in range(k + 1, n):
                r = 0.0
                for j in range(k):
                    r += A[i][j] * temp[j]
                A[i][k] -= r
        akk = A[k][k]
        valid = abs(akk) > 0
        if k == 0 and not valid:
            tr = list(range(n))
            break
        if valid:
            for i in range(k + 1, n):
                A[i][k] = A[i][k] / akk
        if sign == 1:
            if akk < 0:
                sign = 2
        elif sign == -1:
            if akk > 0:
                sign = 2
        elif sign == 0:
            if akk > 0:
                sign = 1
            elif akk < 0:
                sign = -1
    if sign not in (0, 1):
        return False, None
    x = list(b)
    for k in range(n):
        x[k], x[tr[k]] = x[tr[k]], x[k]
    for i in range(1, n):
        s = 0.0
        for j in range(i):
            s += A[i][j] * x[j]
        x[i] -= s
    tol = 1.0 / DBL_MAX
    for i in range(n):
        x[i] = x[i] / A[i][i] if abs(A[i][i]) > tol else 0.0
    for i in range(n - 2, -1, -1):
        s = 0.0
        for j in range(i + 1, n):
            s += A[j][i] * x[j]
        x[i] -= s
    for k in range(n - 1, -1, -1):
        x[k], x[tr[k]] = x[tr[k]], x[k]
    return True, x


# ---- g2o::Sim3 ------------------------------------------------------------------------------------------------------------------------
class Sim3:
    """r (x y z w), t, s.  Nothing here normalises the quaternion: g2o::Sim3 does not."""
    normalising_mul = False

    def __init__(self, q, t, s):
        self.q = list(q)
        self.t = list(t)
        self.s = s

    @staticmethod
    def from_matrix(R, t, s):
        return Sim3(quat_from_matrix(R), t, s)

    def map(self, v):
        r = quat_rotate(self.q, v)
        return [self.s * r[0] + self.t[0], self.s * r[1] + self.t[1], self.s * r[2] + self.t[2]]

    def inverse(self):
        c = -1. / self.s
        qc = [-self.q[0], -self.q[1], -self.q[2], self.q[3]]
        return Sim3(qc, quat_rotate(qc, [c * self.t[0], c * self.t[1], c * self.t[2]]), 1. / self.s)

    def __mul__(self, o):
        q = quat_mul(self.q, o.q)
        if Sim3.normalising_mul:
            n = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
            q = [c / n for c in q]
        r = quat_rotate(self.q, o.t)
        return Sim3(q, [self.s * r[0] + self.t[0], self.s * r[1] + self.t[1], self.s * r[2] + self.t[2]], self.s * o.s)

    @staticmethod
    def exp(update, order, branches=None):
        """Sim3(const Vector7d& update)"""
        o = update[:3]
        ups = update[3:6]
        sigma = update[6]
        theta = math.sqrt(o[0] * o[0] + o[1] * o[1] + o[2] * o[2])
        O = [[0.0, -o[2], o[1]], [o[2], 0.0, -o[0]], [-o[1], o[0], 0.0]]
        O2 = [[O[i][0] * O[0][j] + O[i][1] * O[1][j] + O[i][2] * O[2][j] for j in range(3)] for i in range(3)]
        eye = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
        if order == "index":
            s = math.exp(sigma) if sigma < 709.782712893384 else float("inf")
            sincos = lambda a: (math.sin(a), math.cos(a))
        else:
            s = poly_exp(sigma)
            sincos = poly_sincos
        if abs(sigma) < EPS:
            C = 1
            if theta < EPS:
                branch = 0
                A = 1. / 2.
                B = 1. / 6.
                R = [[(eye[i][j] + O[i][j]) + O2[i][j] for j in range(3)] for i in range(3)]
            else:
                branch = 1
                sn, cs = sincos(theta)
                theta2 = theta * theta
                A = (1 - cs) / theta2
                B = (theta - sn) / (theta2 * theta)
                a, c = sn / theta, (1 - cs) / (theta * theta)
                R = [[(eye[i][j] + a * O[i][j]) + c * O2[i][j] for j in range(3)] for i in range(3)]
        else:
            C = (s - 1) / sigma
            if theta < EPS:
                branch = 2
                sigma2 = sigma * sigma
                A = ((sigma - 1) * s + 1) / sigma2
                B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
                R = [[(eye[i][j] + O[i][j]) + O2[i][j] for j in range(3)] for i in range(3)]
            else:
                branch = 3
                sn, cs = sincos(theta)
                ra, rc = sn / theta, (1 - cs) / (theta * theta)
                R = [[(eye[i][j] + ra * O[i][j]) + rc * O2[i][j] for j in range(3)] for i in range(3)]
                a = s * sn
                b = s * cs
                theta2 = theta * theta
                sigma2 = sigma * sigma
                c = theta2 + sigma2
                A = (a * sigma + (1 - b) * theta) / (theta * c)
                B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2
        if branches is not None:
            branches.add("sim3_exp_%d" % branch)
        W = [[(A * O[i][j] + B * O2[i][j]) + C * eye[i][j] for j in range(3)] for i in range(3)]
        t = [W[i][0] * ups[0] + W[i][1] * ups[1] + W[i][2] * ups[2] for i in range(3)]
        return Sim3(quat_from_matrix(R), t, s), branch


def oplus(est, update, fix_scale, order, branches=None):
    """VertexSim3Expmap::oplusImpl; `update` is the caller's vector and is written through, as the reference does."""
    if fix_scale:
        update[6] = 0
    d, _ = Sim3.exp(update, order, branches)
    return d * est


# ---- the edges ------------------------------------------------------------------------------------------------------------------------
class Edges:
    """The constants of a problem's edges as float64 columns."""

    def __init__(self, P):
        f64 = lambda a, shape: np.asarray(a, np.float32).astype(np.float64).reshape(shape)
        self.n = len(P["octave1"])
        X1, X2 = f64(P["x3dc1"], (-1, 3)), f64(P["x3dc2"], (-1, 3))
        o1, o2 = f64(P["obs1"], (-1, 2)), f64(P["obs2"], (-1, 2))
        self.X1 = [X1[:, k] for k in range(3)]
        self.X2 = [X2[:, k] for k in range(3)]
        self.obs1 = [o1[:, 0], o1[:, 1]]
        self.obs2 = [o2[:, 0], o2[:, 1]]
        s1 = np.asarray(P["inv_level_sigma2_1"], np.float32).astype(np.float64)
        s2 = np.asarray(P["inv_level_sigma2_2"], np.float32).astype(np.float64)
        self.w1 = s1[np.asarray(P["octave1"], np.int64)] if self.n else np.zeros(0)
        self.w2 = s2[np.asarray(P["octave2"], np.int64)] if self.n else np.zeros(0)
        self.K1 = [float(np.float32(v)) for v in P["K1"]]
        self.K2 = [float(np.float32(v)) for v in P["K2"]]
        th2 = np.float32(P["th2"])
        with np.errstate(all="ignore"):
            delta = np.sqrt(th2)                          # `const float deltaHuber = sqrt(th2)`: the float overload
        self.delta = float(delta)                         # setDelta: _delta = the float as a double,
        self.dsqr = float(np.float32(self.delta * self.delta))   # dsqr a float member
        self.th2 = float(th2)

    @staticmethod
    def project(T, X, obs, K):
        """obs - cam_map(project(T.map(X)))"""
        with np.errstate(all="ignore"):
            p = T.map(X)
            return [obs[0] - ((p[0] / p[2]) * K[0] + K[2]), obs[1] - ((p[1] / p[2]) * K[1] + K[3])]

    def errors(self, est):
        """computeError of both edges of every correspondence at the estimate -> (e12, chi12, e21, chi21)"""
        inv = est.inverse()
        e12 = self.project(est, self.X2, self.obs1, self.K1)
        e21 = self.project(inv, self.X1, self.obs2, self.K2)
        with np.errstate(all="ignore"):
            chi12 = e12[0] * (self.w1 * e12[0]) + e12[1] * (self.w1 * e12[1])
            chi21 = e21[0] * (self.w2 * e21[0]) + e21[1] * (self.w2 * e21[1])
        return e12, chi12, e21, chi21

    def jacobians(self, est, fix_scale, order, branches=None):
        """BaseBinaryEdge::linearizeOplus for the Sim3 vertex (the point vertex is fixed): per dimension push, oplus(+delta),
        computeError, pop, push, oplus(-delta), computeError, pop; column = scalar * (error+ - error-).  -> J12[row][col], J21[row][col]"""
        J12 = [[None] * 7 for _ in range(2)]
        J21 = [[None] * 7 for _ in range(2)]
        add = [0.0] * 7
        for d in range(7):
            add[d] = DELTA
            plus = oplus(est, add, fix_scale, order, branches)
            add[d] = -DELTA
            minus = oplus(est, add, fix_scale, order, branches)
            add[d] = 0.0
            with np.errstate(all="ignore"):
                ep = self.project(plus, self.X2, self.obs1, self.K1)
                em = self.project(minus, self.X2, self.obs1, self.K1)
                J12[0][d] = SCALAR * (ep[0] - em[0])
                J12[1][d] = SCALAR * (ep[1] - em[1])
                ep = self.project(plus.inverse(), self.X1, self.obs2, self.K2)
                em = self.project(minus.inverse(), self.X1, self.obs2, self.K2)
                J21[0][d] = SCALAR * (ep[0] - em[0])
                J21[1][d] = SCALAR * (ep[1] - em[1])
        return J12, J21

    def huber(self, chi):
        with np.errstate(all="ignore"):
            sq = np.sqrt(chi)
            inl = chi <= self.dsqr
            return np.where(inl, chi, 2 * sq * self.delta - self.dsqr), np.where(inl, 1.0, self.delta / sq)


def ordered_sum(ta, tb, order):
    """Sum of the rows of the edge terms (ta: the e12 of every correspondence, tb: the e21, n x K each, zero rows for the removed ones)
    in the chosen order -> K floats."""
    n, K = ta.shape
    if order == "index":
        inter = np.zeros((2 * n + 1, K))
        inter[1::2] = ta
        inter[2::2] = tb
        return np.add.accumulate(inter, axis=0)[-1]
    rows = -(-max(n, 1) // LANES)
    pa = np.zeros((rows * LANES, K))
    pb = np.zeros((rows * LANES, K))
    pa[:n] = ta
    pb[:n] = tb
    inter = np.zeros((2 * rows + 1, LANES, K))              # (row 0: the accumulators start at zero)
    inter[1::2] = pa.reshape(rows, LANES, K)
    inter[2::2] = pb.reshape(rows, LANES, K)
    lanes = np.add.accumulate(inter, axis=0)[-1]
    for off in (1, 2, 4, 8, 16, 32):
        lanes = lanes + lanes[np.arange(LANES) ^ off]
    return ((lanes[0] + lanes[64]) + lanes[128]) + lanes[192]


class Trace:
    def __init__(self):
        self.margins = []       # per classification: |chi2 - th2| / th2 of both edges of every correspondence still in the graph
        self.class_chi = []     # per classification: (chi12, chi21) columns
        self.rhos = []
        self.branches = set()
        self.col6 = []          # per linearisation: the largest |J[., 6]|
        self.fixed_scale_exact = True   # Sim3(0) * estimate reproduced the estimate in every linearisation under fix_scale


def _edge_terms(E, J, e, w, rho0, rho1):
    cols = []
    rw = rho1 * w
    with np.errstate(all="ignore"):
        for a in range(7):
            for b in range(a, 7):
                cols.append((J[0][a] * rw) * J[0][b] + (J[1][a] * rw) * J[1][b])
        for a in range(7):
            cols.append(-(rho1 * (J[0][a] * (w * e[0]) + J[1][a] * (w * e[1]))))   # b -= ...: x - t is x + (-t), bit for bit
    cols.append(rho0)
    return np.stack(cols, axis=1)


def optimize(P, order="index", trace=None, rules=()):
    """-> (RESULT_DTYPE record, flag per correspondence: 0 kept, 1 removed after the first optimisation, 2 failed the final test)"""
    assert all(r in RULES for r in rules), rules
    Sim3.normalising_mul = "normalising_mul" in rules
    try:
        return _optimize(P, order, trace if trace is not None else Trace(), rules)
    finally:
        Sim3.normalising_mul = False


def _optimize(P, order, tr, rules):
    E = Edges(P)
    n = E.n
    fix_scale = bool(P["fix_scale"])
    res = np.zeros(1, RESULT_DTYPE)[0]
    R = np.asarray(P["R"], np.float32).reshape(3, 3)
    t = np.asarray(P["t"], np.float32).reshape(3)
    start = Sim3.from_matrix([[float(R[r, c]) for c in range(3)] for r in range(3)], [float(v) for v in t], float(np.float32(P["s"])))
    res["n_correspondences"] = n
    flags = np.zeros(n, np.uint8)
    state = {"est": start, "last": None, "lam": 0.0, "x_last": [0.0] * 7}

    def active_chi(T, active):
        _, chi12, _, chi21 = E.errors(T)
        a, _ = E.huber(chi12)
        b, _ = E.huber(chi21)
        z = np.zeros(n)
        return float(ordered_sum(np.where(active, a, z)[:, None], np.where(active, b, z)[:, None], order)[0])

    def run(stage, iterations_max):
        """initializeOptimization(); optimize(iterations_max) over the edges still in the graph"""
        active = flags == 0
        if not active.any():                            # no active edge, no active vertex: optimize() returns at once
            tr.branches.add("nothing_active")
            return
        est = state["est"]
        lam = state["lam"] if ("carry_lambda" in rules and stage == 1) else 0.0
        ni, strikes = 2.0, 0
        iterations = trials = 0
        current = 0.0
        x_last = state["x_last"]
        for i in range(iterations_max):
            # OptimizationAlgorithmLevenberg::solve(i): computeActiveErrors, linearizeOplus, constructQuadraticForm
            e12, chi12, e21, chi21 = E.errors(est)
            state["last"] = est
            J12, J21 = E.jacobians(est, fix_scale, order, tr.branches)
            if fix_scale:
                z = [0.0] * 7
                same = oplus(est, z, True, order)
                tr.fixed_scale_exact &= (same.q == est.q and same.t == est.t and same.s == est.s)
            with np.errstate(all="ignore"):
                tr.col6.append(max([0.0] + [float(np.max(np.abs(J[r][6]))) for J in (J12, J21) for r in range(2)]))
            r0a, r1a = E.huber(chi12)
            r0b, r1b = E.huber(chi21)
            ta = np.where(active[:, None], _edge_terms(E, J12, e12, E.w1, r0a, r1a), 0.0)
            tb = np.where(active[:, None], _edge_terms(E, J21, e21, E.w2, r0b, r1b), 0.0)
            sums = ordered_sum(ta, tb, order)
            current = float(sums[35])
            ini = current
            H = [[0.0] * 7 for _ in range(7)]
            k = 0
            for a in range(7):
                for b in range(a, 7):
                    H[a][b] = H[b][a] = float(sums[k])
                    k += 1
            bvec = [float(v) for v in sums[28:35]]
            if i == 0 and not ("carry_lambda" in rules and stage == 1):
                lam = 1e-5 * max([0.0] + [abs(H[j][j]) for j in range(7)])      # computeLambdaInit
            if i == 0:
                ni, strikes = 2.0, 0
            qmax = 0
            while True:
                Hl = [row[:] for row in H]
                for j in range(7):
                    Hl[j][j] += lam
                ok2, x = ldlt_solve(Hl, bvec)
                if not ok2:
                    tr.branches.add("not_positive")
                    x = x_last                       # the solver's x keeps what the last successful solve left
                x = list(x)
                trial = oplus(est, x, fix_scale, order, tr.branches)   # (writes x[6] = 0 under fix_scale: computeScale reads it)
                x_last = x
                temp = active_chi(trial, active)
                state["last"] = trial
                if not ok2:
                    temp = DBL_MAX
                rho = current - temp
                scale = 0.0
                for j in range(7):
                    scale += x[j] * (lam * x[j] + bvec[j])
                scale += 1e-3
                rho /= scale
                tr.rhos.append(rho)
                if rho > 0 and math.isfinite(temp):
                    u = 2 * rho - 1
                    alpha = 1. - (math.pow(u, 3) if order == "index" else u * u * u)
                    alpha = min(alpha, 2. / 3.)
                    lam *= max(1. / 3., alpha)
                    ni = 2.0
                    current = temp
                    est = trial
                else:
                    lam *= ni
                    ni *= 2
                    tr.branches.add("rejected_trial")
                qmax += 1
                trials += 1
                if not (rho < 0 and qmax < 10):
                    break
            iterations += 1
            if qmax == 10 or rho == 0:
                tr.branches.add("qmax_10" if qmax == 10 else "rho_zero")
                break
            if (ini - current) * 1e3 < ini:
                strikes += 1
            else:
                strikes = 0
            if strikes >= 3:
                tr.branches.add("three_strikes")
                break
        else:
            tr.branches.add("all_iterations_%d" % iterations_max)
        if state["last"] is not est:
            tr.branches.add("ended_on_rejected_trial")
        state["est"], state["lam"], state["x_last"] = est, lam, x_last
        res["optimisations"] = stage + 1
        res["round"][stage]["iterations"] = iterations
        res["round"][stage]["trials"] = trials
        res["round"][stage]["chi2"] = canonical(current)
        res["round"][stage]["lambda"] = canonical(lam)

    def failed():
        """`e12->chi2()>th2 || e21->chi2()>th2` over the edges still in the graph: _error is the last computeActiveErrors'"""
        at = state["est"] if "classify_at_estimate" in rules else state["last"]
        if at is None:
            return np.zeros(n, bool)
        _, chi12, _, chi21 = E.errors(at)
        act = flags == 0
        with np.errstate(all="ignore"):
            tr.margins.append(np.concatenate([np.abs(chi12[act] - E.th2) / E.th2, np.abs(chi21[act] - E.th2) / E.th2]))
            tr.class_chi.append((chi12.copy(), chi21.copy()))
            return act & ((chi12 > E.th2) | (chi21 > E.th2))

    def write(T):
        res["q"] = [canonical(c) for c in T.q]
        res["t"] = [canonical(c) for c in T.t]
        res["s"] = canonical(T.s)

    run(0, 5)
    bad = failed()
    flags[bad] = 1
    n_bad = int(bad.sum())
    res["n_bad"] = n_bad
    n_more = 10 if n_bad > 0 else 5
    res["n_more_iterations"] = n_more
    tr.branches.add("n_more_%d" % n_more)
    if n - n_bad < 10:
        tr.branches.add("early_return")
        write(state["est"] if "write_on_early_return" in rules else start)
        return res, flags
    run(1, n_more)
    bad = failed()
    flags[bad] = 2
    res["n_inliers"] = n - n_bad - int(bad.sum())
    res["written"] = 1
    write(state["est"])
    return res, flags
