"""A float64 model of Optimizer::PoseOptimization (reference src/Optimizer.cc:352-898) and of the parts of g2o it runs, written from
the reference's and g2o's sources (Thirdparty/g2o/g2o/types/types_six_dof_expmap.{h,cpp}, types/se3quat.h, types/se3_ops.hpp,
core/base_unary_edge.hpp, core/robust_kernel_impl.cpp, core/optimization_algorithm_levenberg.cpp, core/sparse_optimizer.cpp,
solvers/linear_solver_dense.h) and from Eigen's published sources for the operators those call -- not from csrc/pose.hip: the loops
below are g2o's nested loops (optimize -> solve -> trials), not a state machine, and the edges are evaluated as NumPy columns.

Every per-edge operation is an element-wise IEEE + - * / of float64 columns (NumPy rounds each of them exactly as the scalar
operation), sums over edges are explicit (np.add.accumulate is strictly sequential; np.sum is pairwise and is not used), and everything
that happens once per trial is Python float arithmetic with math.sqrt / math.sin / math.cos / math.pow -- the C library's.

order="index":  every sum over edges runs in ascending edge position; sin, cos and pow(., 3) from the C library.
order="device": the sums run in the device kernel's tree (256 lanes, lane l owns edges l, l + 256, ... in ascending order; an xor
                butterfly 1, 2, 4, 8, 16, 32 inside each group of 64 lanes; the four groups in order); sine and cosine from the fixed
                polynomial sequence below; the cube by multiplication."""
import math
import numpy as np

ROUND_DTYPE = np.dtype([("iterations", "<i4"), ("trials", "<i4"), ("chi2", "<f8"), ("lambda", "<f8")])
RESULT_DTYPE = np.dtype([("Tcw", "<f4", (16,)), ("q", "<f8", (4,)), ("t", "<f8", (3,)), ("n_initial", "<i4"), ("n_bad", "<i4"),
                         ("n_inliers", "<i4"), ("rounds", "<i4"), ("round", ROUND_DTYPE, (4,))])
CAM0, ALL_CAMS = 0, 1
LANES = 256
DBL_MAX = 1.7976931348623157e308


# ---- sine / cosine of the device order -----------------------------------------------------------------------------------------------
def poly_sincos(x):
    """Range reduction by pi/2 (the quotient rounded by adding and subtracting 1.5 * 2^52, a two-part pi/2) and Taylor polynomials
    up to z^8 in Horner form; + - * / only."""
    two_over_pi = 6.36619772367581382433e-01
    pio2_hi, pio2_lo = 1.57079632673412561417e+00, 6.07710050650619224932e-11
    magic = 6755399441055744.0
    kf = (x * two_over_pi + magic) - magic
    r = (x - kf * pio2_hi) - kf * pio2_lo
    z = r * r
    ps = 1.0 / 355687428096000.0
    for c in (-1.0 / 1307674368000.0, 1.0 / 6227020800.0, -1.0 / 39916800, 1.0 / 362880, -1.0 / 5040, 1.0 / 120, -1.0 / 6):
        ps = ps * z + c
    s = r + r * (z * ps)
    pc = 1.0 / 20922789888000.0
    for c in (-1.0 / 87178291200.0, 1.0 / 479001600, -1.0 / 3628800, 1.0 / 40320, -1.0 / 720, 1.0 / 24, -1.0 / 2):
        pc = pc * z + c
    c = 1.0 + z * pc
    q = int(kf) & 3
    return ((s, c, -s, -c)[q], (c, -s, -c, s)[q])


# ---- Eigen's operators (restated from its sources; UNPINNED: DESIGN.md section 2) -----------------------------------------------------
def quat_from_matrix(m):
    """Quaterniond(Matrix3d): m is a 3x3 nested list -> [x, y, z, w]."""
    q = [0.0] * 4
    t = m[0][0] + m[1][1] + m[2][2]
    if t > 0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[2][1] - m[1][2]) * t
        q[1] = (m[0][2] - m[2][0]) * t
        q[2] = (m[1][0] - m[0][1]) * t
    else:
        i = 0
        if m[1][1] > m[0][0]:
            i = 1
        if m[2][2] > m[i][i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = math.sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[k][j] - m[j][k]) * t
        q[j] = (m[j][i] + m[i][j]) * t
        q[k] = (m[k][i] + m[i][k]) * t
    return q


def quat_normalized(q):
    n = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return [q[0] / n, q[1] / n, q[2] / n, q[3] / n]


def quat_rotate(q, v):
    """q * v for scalars or columns: uv = vec x v; uv += uv; v + w * uv + vec x uv."""
    uv0 = q[1] * v[2] - q[2] * v[1]
    uv1 = q[2] * v[0] - q[0] * v[2]
    uv2 = q[0] * v[1] - q[1] * v[0]
    uv0 = uv0 + uv0
    uv1 = uv1 + uv1
    uv2 = uv2 + uv2
    c0 = q[1] * uv2 - q[2] * uv1
    c1 = q[2] * uv0 - q[0] * uv2
    c2 = q[0] * uv1 - q[1] * uv0
    return [v[0] + q[3] * uv0 + c0, v[1] + q[3] * uv1 + c1, v[2] + q[3] * uv2 + c2]


def quat_mul(a, b):
    return [a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
            a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
            a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
            a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]]


def quat_to_matrix(q):
    tx, ty, tz = 2 * q[0], 2 * q[1], 2 * q[2]
    twx, twy, twz = tx * q[3], ty * q[3], tz * q[3]
    txx, txy, txz = tx * q[0], ty * q[0], tz * q[0]
    tyy, tyz, tzz = ty * q[1], tz * q[1], tz * q[2]
    return [[1 - (tyy + tzz), txy - twz, txz + twy],
            [txy + twz, 1 - (txx + tzz), tyz - twx],
            [txz - twy, tyz + twx, 1 - (txx + tyy)]]


def ldlt_solve(H, b):
    """Eigen::LDLT<MatrixXd>::compute(H) (the unblocked in-place form over the lower triangle, pivoting on the first largest
    |diagonal|), isPositive(), solve(b).  -> (ok, x); x is None when the factorisation is not positive."""
    n = 6
    A = [row[:] for row in H]
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


# ---- g2o::SE3Quat ---------------------------------------------------------------------------------------------------------------------
class SE3:
    def __init__(self, q, t):
        self.q = list(q)
        self.t = list(t)
        if self.q[3] < 0:                       # normalizeRotation
            self.q = [c * -1 for c in self.q]
        self.q = quat_normalized(self.q)

    @staticmethod
    def from_matrix(R, t):
        return SE3(quat_from_matrix(R), t)

    @staticmethod
    def from_cv(M):
        """Converter::toSE3Quat of a float 4x4."""
        M = np.asarray(M, np.float32).reshape(4, 4)
        return SE3.from_matrix([[float(M[r, c]) for c in range(3)] for r in range(3)], [float(M[r, 3]) for r in range(3)])

    def map(self, v):
        r = quat_rotate(self.q, v)
        return [r[0] + self.t[0], r[1] + self.t[1], r[2] + self.t[2]]

    def __mul__(self, o):
        r = quat_rotate(self.q, o.t)
        return SE3(quat_mul(self.q, o.q), [self.t[0] + r[0], self.t[1] + r[1], self.t[2] + r[2]])

    @staticmethod
    def exp(update, order):
        o = update[:3]
        ups = update[3:]
        theta = math.sqrt(o[0] * o[0] + o[1] * o[1] + o[2] * o[2])
        O = [[0.0, -o[2], o[1]], [o[2], 0.0, -o[0]], [-o[1], o[0], 0.0]]
        O2 = [[O[i][0] * O[0][j] + O[i][1] * O[1][j] + O[i][2] * O[2][j] for j in range(3)] for i in range(3)]
        eye = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
        small = theta < 0.00001
        if small:
            R = [[(eye[i][j] + O[i][j]) + O2[i][j] for j in range(3)] for i in range(3)]
            V = R
        else:
            if order == "index":
                sn, cs, th3 = math.sin(theta), math.cos(theta), math.pow(theta, 3)
            else:
                sn, cs = poly_sincos(theta)
                th3 = theta * theta * theta
            a = sn / theta
            c = (1 - cs) / (theta * theta)
            d = (theta - sn) / th3
            R = [[(eye[i][j] + a * O[i][j]) + c * O2[i][j] for j in range(3)] for i in range(3)]
            V = [[(eye[i][j] + c * O[i][j]) + d * O2[i][j] for j in range(3)] for i in range(3)]
        t = [V[i][0] * ups[0] + V[i][1] * ups[1] + V[i][2] * ups[2] for i in range(3)]
        return SE3.from_matrix(R, t), small


def canonical(x):
    """A NaN leaves as the NaN x86 makes from an invalid operation."""
    return x if x == x else float(np.frombuffer(np.uint64(0xfff8000000000000).tobytes(), np.float64)[0])


# ---- the edges ------------------------------------------------------------------------------------------------------------------------
class Edges:
    """The constants of a problem's edges as float64 columns."""

    def __init__(self, P):
        f64 = lambda a: np.asarray(a, np.float32).astype(np.float64)
        self.n = len(P["feat"])
        self.multi = P["mode"] == ALL_CAMS
        pos = f64(P["pos"]).reshape(-1, 3)
        obs32 = np.asarray(P["obs"], np.float32).reshape(-1, 3)
        obs = obs32.astype(np.float64)
        self.X = [pos[:, 0], pos[:, 1], pos[:, 2]]
        self.obs = [obs[:, 0], obs[:, 1], obs[:, 2]]
        self.stereo = ~(obs32[:, 2] < 0)
        self.w = f64(np.asarray(P["inv_level_sigma2"], np.float32)[np.asarray(P["octave"], np.int64)]) if self.n else np.zeros(0)
        self.cam1 = (np.asarray(P["feat"], np.int64) >= P["n_cam0"]) if self.multi else np.zeros(self.n, bool)
        self.fx, self.fy, self.cx, self.cy, self.bf = (float(np.float32(P[k])) for k in ("fx", "fy", "cx", "cy", "bf"))
        # Tcam11 = eye, Tcam21 = [Rcam12.t() | -Rcam12.t() * tcam12] in float (cv::gemm's small path: float products summed left to
        # right, then the scale by alpha = -1 in double)
        R12 = np.asarray(P["Rcam12"], np.float32).reshape(3, 3)
        t12 = np.asarray(P["tcam12"], np.float32).reshape(3)
        T21 = np.zeros((4, 4), np.float32)
        T21[:3, :3] = R12.T
        for r in range(3):
            s = R12[0, r] * t12[0] + R12[1, r] * t12[1]
            s = s + R12[2, r] * t12[2]
            T21[r, 3] = np.float32(np.float64(s) * -1.0 + 0.0 * 0.0)
        T21[3, 3] = 1
        self.Tc = [SE3.from_cv(np.eye(4, dtype=np.float32)), SE3.from_cv(T21)]
        self.Rc = [quat_to_matrix(T.q) for T in self.Tc]
        dm, ds = np.float32(math.sqrt(5.991)), np.float32(math.sqrt(7.815))   # `const float deltaMono = sqrt(5.991)`
        delta = np.where(self.stereo, float(ds), float(dm))
        self.delta = delta
        self.dsqr = np.where(self.stereo, float(np.float32(float(ds) * float(ds))), float(np.float32(float(dm) * float(dm))))   # a float member

    def camera_points(self, T):
        p = T.map(self.X)
        if not self.multi:
            return p, p
        a = self.Tc[0].map(p)
        b = self.Tc[1].map(p)
        return p, [np.where(self.cam1, b[k], a[k]) for k in range(3)]

    def errors(self, T):
        """computeError + chi2 of every edge at pose T -> (e columns, chi2, p, pc)."""
        with np.errstate(all="ignore"):
            p, pc = self.camera_points(T)
            m0 = self.obs[0] - ((pc[0] / pc[2]) * self.fx + self.cx)
            m1 = self.obs[1] - ((pc[1] / pc[2]) * self.fy + self.cy)
            invz = (1.0 / pc[2]).astype(np.float32).astype(np.float64)       # `const float invz = 1.0f/trans_xyz[2]`
            r0 = pc[0] * invz * self.fx + self.cx
            r1 = pc[1] * invz * self.fy + self.cy
            r2 = r0 - self.bf * invz
            e0 = np.where(self.stereo, self.obs[0] - r0, m0)
            e1 = np.where(self.stereo, self.obs[1] - r1, m1)
            e2 = np.where(self.stereo, self.obs[2] - r2, 0.0)
            w = self.w
            chi = e0 * (w * e0) + e1 * (w * e1)
            chi = np.where(self.stereo, chi + e2 * (w * e2), chi)
        return [e0, e1, e2], chi, p, pc

    def jacobians(self, p, pc):
        """linearizeOplus of every edge -> J[row][col] columns (row 2 is only meaningful for stereo edges)."""
        fx, fy, bf = self.fx, self.fy, self.bf
        with np.errstate(all="ignore"):
            if not self.multi:
                x, y = p[0], p[1]
                invz = 1.0 / p[2]
                invz_2 = invz * invz
                zero = np.zeros(self.n)
                J0 = [x * y * invz_2 * fx, -(1 + (x * x * invz_2)) * fx, y * invz * fx, -invz * fx, zero, x * invz_2 * fx]
                J1 = [(1 + y * y * invz_2) * fy, -x * y * invz_2 * fy, -x * invz * fy, zero, -invz * fy, y * invz_2 * fy]
                J2 = [J0[0] - bf * y * invz_2, J0[1] + bf * x * invz_2, J0[2], J0[3], zero, J0[5] - bf * invz_2]
                return [J0, J1, J2]
            x, y, z = p
            xc, yc, zc = pc
            zc_2 = zc * zc
            a1 = bf / zc_2
            r = [[np.where(self.cam1, self.Rc[1][i][j], self.Rc[0][i][j]) for j in range(3)] for i in range(3)]
            t100, t102 = -fx / zc, fx * xc / zc_2
            t111, t112 = -fy / zc, fy * yc / zc_2
            t2 = [[t100 * r[0][0] + t102 * r[2][0], t100 * r[0][1] + t102 * r[2][1], t100 * r[0][2] + t102 * r[2][2]],
                  [t111 * r[1][0] + t112 * r[2][0], t111 * r[1][1] + t112 * r[2][1], t111 * r[1][2] + t112 * r[2][2]]]
            t2.append([t2[0][0] - a1 * r[2][0], t2[0][1] - a1 * r[2][1], t2[0][2] - a1 * r[2][2]])
            return [[-t2[k][1] * z + t2[k][2] * y, t2[k][0] * z - t2[k][2] * x, -t2[k][0] * y + t2[k][1] * x, t2[k][0], t2[k][1], t2[k][2]]
                    for k in range(3)]


def ordered_sum(terms, order):
    """Sum of the rows of `terms` (n x K, zero rows for the edges that do not take part) in the chosen order -> K floats."""
    n, K = terms.shape
    if order == "index":
        return np.add.accumulate(np.concatenate([np.zeros((1, K)), terms]), axis=0)[-1]
    rows = -(-max(n, 1) // LANES)
    padded = np.zeros((rows * LANES + LANES, K))
    padded[LANES:LANES + n] = terms                          # (row 0: the accumulators start at zero)
    lanes = np.add.accumulate(padded.reshape(rows + 1, LANES, K), axis=0)[-1]
    for off in (1, 2, 4, 8, 16, 32):
        lanes = lanes + lanes[np.arange(LANES) ^ off]
    return ((lanes[0] + lanes[64]) + lanes[128]) + lanes[192]


class Trace:
    """What check_conditions looks at: every classification margin, every trial's rho, the branches reached."""

    def __init__(self):
        self.margins = []       # |(float)chi2 - th| / th of every edge at every classification
        self.rhos = []
        self.class_chi = []     # per classification: the double chi2 column
        self.branches = set()


def optimize(P, order="index", trace=None, rules=()):
    """-> (RESULT_DTYPE record, outlier flag per edge).  rules: ("nine_edges",) is the deliberately WRONG rule `n < 9` for the `n < 10`
    that ends the call after one round (tests/test_geometry_boundary_worlds.py shows that the boundary worlds catch it)."""
    assert all(r == "nine_edges" for r in rules), rules
    few = 9 if "nine_edges" in rules else 10
    tr = trace if trace is not None else Trace()
    E = Edges(P)
    n = E.n
    res = np.zeros(1, RESULT_DTYPE)[0]
    Tcw = np.asarray(P["Tcw"], np.float32).reshape(16)
    start = SE3.from_cv(Tcw)
    flags = np.zeros(n, bool)
    res["n_initial"] = n
    if n < 3:
        res["Tcw"] = Tcw
        res["q"] = [canonical(c) for c in start.q]
        res["t"] = [canonical(c) for c in start.t]
        tr.branches.add("fewer_than_3")
        return res, flags.astype(np.uint8)
    robust = True
    n_bad = 0
    est = start
    x_last = [0.0] * 6
    for it in range(4):
        est = start                                   # vSE3->setEstimate(Converter::toSE3Quat(pFrame->mTcw))
        active = ~flags                               # initializeOptimization(0): the edges of level 0
        last = None                                   # the pose of the last computeActiveErrors
        if active.any():                              # otherwise optimize() finds no vertex and returns
            lam, ni, strikes = 0.0, 2.0, 0
            iterations = trials = 0
            current = 0.0

            def robust_terms(chi):
                if not robust:
                    return chi, np.ones(n)
                with np.errstate(all="ignore"):
                    sq = np.sqrt(chi)
                    inl = chi <= E.dsqr
                    return np.where(inl, chi, 2 * sq * E.delta - E.dsqr), np.where(inl, 1.0, E.delta / sq)

            def active_chi(T):
                _, chi, _, _ = E.errors(T)
                rho0, _ = robust_terms(chi)
                return float(ordered_sum(np.where(active, rho0, 0.0)[:, None], order)[0])

            for i in range(10):
                # OptimizationAlgorithmLevenberg::solve(i)
                e, chi, p, pc = E.errors(est)
                last = est
                rho0, rho1 = robust_terms(chi)
                J = E.jacobians(p, pc)
                cols = []
                w = E.w
                rw = rho1 * w
                with np.errstate(all="ignore"):
                    for a in range(6):
                        for b in range(a, 6):
                            h = (J[0][a] * rw) * J[0][b] + (J[1][a] * rw) * J[1][b]
                            cols.append(np.where(E.stereo, h + (J[2][a] * rw) * J[2][b], h))
                    for a in range(6):
                        g = J[0][a] * (w * e[0]) + J[1][a] * (w * e[1])
                        g = np.where(E.stereo, g + J[2][a] * (w * e[2]), g)
                        cols.append(rho1 * g)
                cols.append(rho0)
                terms = np.where(active[:, None], np.stack(cols, axis=1), 0.0)
                terms[:, 21:27] = -terms[:, 21:27]        # b -= ...: 0 - t and then x - t: the same bits as adding -t
                sums = ordered_sum(terms, order)
                current = float(sums[27])
                ini = current
                H = [[0.0] * 6 for _ in range(6)]
                k = 0
                for a in range(6):
                    for b in range(a, 6):
                        H[a][b] = H[b][a] = float(sums[k])
                        k += 1
                bvec = [float(v) for v in sums[21:27]]
                if i == 0:
                    lam = 1e-5 * max([0.0] + [abs(H[j][j]) for j in range(6)])
                    ni, strikes = 2.0, 0
                qmax = 0
                while True:
                    Hl = [row[:] for row in H]
                    for j in range(6):
                        Hl[j][j] += lam
                    ok2, x = ldlt_solve(Hl, bvec)
                    if not ok2:
                        tr.branches.add("not_positive")
                        x = x_last                       # the solver's x keeps what the last successful solve left
                    x_last = x
                    d, small = SE3.exp(x, order)
                    if small:
                        tr.branches.add("small_theta")
                    trial = d * est
                    temp = active_chi(trial)
                    last = trial
                    if not ok2:
                        temp = DBL_MAX
                    rho = current - temp
                    scale = 0.0
                    for j in range(6):
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
                tr.branches.add("ten_iterations")
            res["round"][it]["iterations"] = iterations
            res["round"][it]["trials"] = trials
            res["round"][it]["chi2"] = canonical(current)
            res["round"][it]["lambda"] = canonical(lam)
        else:
            tr.branches.add("nothing_active")
        # the classification: an outlier's error is recomputed at the estimate, an inlier keeps its last error
        _, chi_est, _, pc_est = E.errors(est)
        chi = chi_est
        if last is not None:
            _, chi_last, _, _ = E.errors(last)
            chi = np.where(flags, chi_est, chi_last)
        if (pc_est[2] <= 0).any():
            tr.branches.add("depth_not_positive")
        chi32 = chi.astype(np.float32)
        th = np.where(E.stereo, np.float32(7.815), np.float32(5.991)).astype(np.float32)
        with np.errstate(all="ignore"):
            tr.margins.append(np.abs(chi32.astype(np.float64) - th.astype(np.float64)) / th.astype(np.float64))
        tr.class_chi.append(chi.copy())
        flags = chi32 > th
        n_bad = int(flags.sum())
        res["rounds"] = it + 1
        if it == 2:
            robust = False
        if n < few:
            tr.branches.add("fewer_than_10")
            break
    res["n_bad"] = n_bad
    res["n_inliers"] = n - n_bad
    R = quat_to_matrix(est.q)
    M = np.zeros((4, 4), np.float32)
    with np.errstate(all="ignore"):
        for r in range(3):
            for c in range(3):
                M[r, c] = np.float32(R[r][c])
            M[r, 3] = np.float32(est.t[r])
    M[3, 3] = 1
    M[np.isnan(M)] = np.frombuffer(np.uint32(0xffc00000).tobytes(), np.float32)[0]
    res["Tcw"] = M.reshape(16)
    res["q"] = [canonical(c) for c in est.q]
    res["t"] = [canonical(c) for c in est.t]
    return res, flags.astype(np.uint8)
