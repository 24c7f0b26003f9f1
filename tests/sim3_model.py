"""A NumPy / math model of Sim3Solver (reference src/Sim3Solver.cc) written from the sources and from OpenCV's semantics, np.float32 /
np.float64 step by step: ComputeCentroid, ComputeSim3 (steps 1-8), Project, FromCameraToImage, CheckInliers, the `iterate` loop,
SetRansacParameters and the take-and-swap drawing of the triples.  It shares no code with the library: the tests hold the library's
host routine against it byte for byte in both orders ("libm": atan2 / sin / cos of the C library; "device": the + - * / sqrt atan2 and
the polynomial sine / cosine).  The Horn part is scalar (one hypothesis at a time), the inlier part is array arithmetic over
(hypotheses x correspondences): element-wise float32 operations round exactly as the scalar statements do."""
import math

import numpy as np

from pose_model import poly_sincos

F = np.float32
D = np.float64
FLT_EPSILON = F(1.1920929e-07)
DBL_EPSILON = 2.220446049250313e-16
CAP, MAX_ITS, MAX_BATCH = 8192, 1024, 64

HYP_DTYPE = np.dtype([("R12", "<f4", (9,)), ("t12", "<f4", (3,)), ("s12", "<f4"), ("T12", "<f4", (16,)), ("T21", "<f4", (16,)),
                      ("n_inliers", "<i4")])


# ---- the two orders' transcendental calls ----------------------------------------------------------------------------------------
def atan_unit(a):
    for _ in range(3):
        a = a / (1.0 + math.sqrt(1.0 + a * a))
    z = a * a
    q = 1.0 / 19
    for d in (17, 15, 13, 11, 9, 7, 5, 3):
        q = 1.0 / d - z * q
    return 8.0 * (a - a * (z * q))


def atan2_device(y, x):
    """y >= 0, x in [-1, 1]: + - * / sqrt in double."""
    pi_hi, pi_lo = 3.141592653589793116e+00, 1.224646799147353207e-16
    pio2_hi, pio2_lo = 1.570796326794896558e+00, 6.123233995736766036e-17
    ax = abs(x)
    if ax >= y:
        r = atan_unit(0.0 if (ax == 0 and y == 0) else y / ax)
        return (pi_hi - r) + pi_lo if x < 0 else r
    if y != y or x != x:
        return math.nan
    return (pio2_hi - atan_unit(x / y)) + pio2_lo


def atan2_libm(y, x):
    return math.atan2(y, x)


def div(a, b):
    """IEEE double division (Python raises on a zero divisor)."""
    with np.errstate(all="ignore"):
        return float(D(a) / D(b))


# ---- the OpenCV operators --------------------------------------------------------------------------------------------------------
def cv_scale(x, alpha):
    """A scaled matrix evaluated on its own: add(M, 0), subtract(0, M), or convertTo's x * (float)alpha + 0."""
    if alpha == 1:
        return x + F(0)
    if alpha == -1:
        return F(0) - x
    return x * F(alpha) + F(0)


def cv_scale_t(x, alpha):
    return x * F(alpha) + F(0) if alpha != 1 else x


def cv_gemm3(a0, a1, a2, b0, b1, b2, alpha, c, beta):
    """cv::gemm's small path, inner length 3: float products and sums from the left, then (float)(t*alpha + c*beta) in double.
    Scalars or arrays."""
    t = a0 * b0 + a1 * b1
    t = t + a2 * b2
    r = (np.asarray(t, D) * D(alpha) + np.asarray(c, D) * D(beta)).astype(F)
    return r[()] if r.ndim == 0 else r


def cv_gemm3_bt(a, b):
    s0 = 0.0
    for k in range(3):
        s0 += float(a[k]) * float(b[k])
    return F((((s0 + 0.0) + 0.0) + 0.0) * 1.0)


def cv_norm3(v):
    s = 0.0
    for k in range(3):
        s += float(v[k]) * float(v[k])
    return math.sqrt(s) if s == s and s != math.inf else s


def cv_hypot(a, b):
    a, b = abs(a), abs(b)
    if a > b:
        b = b / a
        return a * F(math.sqrt(float(F(1) + b * b)))
    if b > 0:
        a = a / b
        return b * F(math.sqrt(float(F(1) + a * a)))
    return F(0)


def sqrt_d(x):
    return math.sqrt(x) if x >= 0 and x != math.inf else (x if x == math.inf else math.nan)


def cv_eigen_row0(A):
    """JacobiImpl_<float> on a symmetric 4x4 (list of lists of np.float32, upper triangle used, destroyed): the row of V that belongs
    to the first largest eigenvalue -- evec.row(0) after the descending sort -- and the eigenvalues with V (for the known-answer test)."""
    V = [[F(1) if i == j else F(0) for j in range(4)] for i in range(4)]
    e = [A[i][i] for i in range(4)]
    pairs = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))

    def rot(r0, c0, r1, c1, M0, M1):
        a0, b0 = M0[r0][c0], M1[r1][c1]
        M0[r0][c0] = a0 * c - b0 * s
        M1[r1][c1] = a0 * s + b0 * c

    for _ in range(480):
        K, L = pairs[0]
        mv = abs(A[0][1])
        for (k, l) in pairs[1:]:
            v = abs(A[k][l])
            if mv < v:
                mv, K, L = v, k, l
        if mv <= FLT_EPSILON:
            break
        p = A[K][L]
        y = (e[L] - e[K]) * F(0.5)
        t = abs(y) + cv_hypot(p, y)
        s = cv_hypot(p, t)
        c = t / s
        s = p / s
        t = (p / t) * p
        if y < 0:
            s, t = -s, -t
        A[K][L] = F(0)
        e[K] = e[K] - t
        e[L] = e[L] + t
        for i in range(4):
            if i < K:
                rot(i, K, i, L, A, A)
            elif K < i < L:
                rot(K, i, i, L, A, A)
            elif i > L:
                rot(K, i, L, i, A, A)
        for i in range(4):
            rot(K, i, L, i, V, V)
    m = 0
    for i in range(1, 4):
        if e[m] < e[i]:
            m = i
    return list(V[m]), e, V


def cv_rodrigues(vec, order):
    rx, ry, rz = float(vec[0]), float(vec[1]), float(vec[2])
    theta = sqrt_d(rx * rx + ry * ry + rz * rz)
    if theta < DBL_EPSILON:
        return [F(1) if k % 4 == 0 else F(0) for k in range(9)]
    if theta != theta or theta == math.inf:
        c = s = math.nan
    elif order == "libm":
        c, s = math.cos(theta), math.sin(theta)
    else:
        s, c = poly_sincos(theta)
    c1 = 1. - c
    itheta = div(1., theta) if theta else 0.
    rx *= itheta; ry *= itheta; rz *= itheta
    rrt = [rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz]
    r_x = [0, -rz, ry, rz, 0, -rx, -ry, rx, 0]
    return [F((c * (1.0 if k % 4 == 0 else 0.0) + c1 * rrt[k]) + s * r_x[k]) for k in range(9)]


# ---- one hypothesis ----------------------------------------------------------------------------------------------------------------
def horn(P1, P2, fix_scale, order):
    """P1, P2: 3 x 3 float32, [row x y z][column = point].  -> dict R (9), t (3), s, T12 (16), T21 (16) of np.float32, plus the
    intermediate N matrix and quaternion (for the known-answer tests)."""
    with np.errstate(all="ignore"):
        P1 = [[F(v) for v in r] for r in P1]
        P2 = [[F(v) for v in r] for r in P2]
        third = 1. / 3
        O1 = [cv_scale((P1[r][0] + P1[r][1]) + P1[r][2], third) for r in range(3)]
        O2 = [cv_scale((P2[r][0] + P2[r][1]) + P2[r][2], third) for r in range(3)]
        Pr1 = [[P1[r][i] - O1[r] for i in range(3)] for r in range(3)]
        Pr2 = [[P2[r][i] - O2[r] for i in range(3)] for r in range(3)]
        M = [[cv_gemm3_bt(Pr2[i], Pr1[j]) for j in range(3)] for i in range(3)]
        N = [[F(0)] * 4 for _ in range(4)]
        N[0][0] = (M[0][0] + M[1][1]) + M[2][2]
        N[0][1] = M[1][2] - M[2][1]
        N[0][2] = M[2][0] - M[0][2]
        N[0][3] = M[0][1] - M[1][0]
        N[1][1] = (M[0][0] - M[1][1]) - M[2][2]
        N[1][2] = M[0][1] + M[1][0]
        N[1][3] = M[2][0] + M[0][2]
        N[2][2] = (-M[0][0] + M[1][1]) - M[2][2]
        N[2][3] = M[1][2] + M[2][1]
        N[3][3] = (-M[0][0] - M[1][1]) + M[2][2]
        for i in range(4):
            for j in range(i):
                N[i][j] = N[j][i]
        N_in = np.array(N, F)
        q, _, _ = cv_eigen_row0(N)
        vec = [q[1], q[2], q[3]]
        nrm = cv_norm3(vec)
        ang = (atan2_libm if order == "libm" else atan2_device)(nrm, float(q[0]))
        w = (2 * ang) * div(1., nrm)
        vec = [cv_scale(v, w) for v in vec]
        R = cv_rodrigues(vec, order)
        P3 = [[cv_gemm3(R[3 * i], R[3 * i + 1], R[3 * i + 2], Pr2[0][j], Pr2[1][j], Pr2[2][j], 1.0, F(0), 0.0) for j in range(3)] for i in range(3)]
        ms = F(1)
        if not fix_scale:
            nom = den = 0.0
            for i in range(3):
                for j in range(3):
                    nom += float(Pr1[i][j]) * float(P3[i][j])
                    den += float(P3[i][j] * P3[i][j])
            ms = F(div(nom, den))
        s = float(ms)
        t = [cv_gemm3(R[3 * i], R[3 * i + 1], R[3 * i + 2], O2[0], O2[1], O2[2], -s, O1[i], 1.0) for i in range(3)]
        inv_s = div(1.0, s)
        T12 = [F(0)] * 16
        T21 = [F(0)] * 16
        sRinv = [[cv_scale_t(R[3 * j + i], inv_s) for j in range(3)] for i in range(3)]
        for i in range(3):
            for j in range(3):
                T12[4 * i + j] = cv_scale(R[3 * i + j], s)
                T21[4 * i + j] = sRinv[i][j]
            T12[4 * i + 3] = t[i]
            T21[4 * i + 3] = cv_gemm3(sRinv[i][0], sRinv[i][1], sRinv[i][2], t[0], t[1], t[2], -1.0, F(0), 0.0)
        T12[15] = T21[15] = F(1)
    return dict(R=np.array(R, F), t=np.array(t, F), s=ms, T12=np.array(T12, F), T21=np.array(T21, F), N=N_in, q=np.array(q, F))


# ---- the inlier phase, all hypotheses of a problem at once ------------------------------------------------------------------------------
RULES = ("inlier_le", "float_sum", "fma_to_image")      # the deliberately WRONG rules of evaluate(..., rules=)


def to_image(X, Y, Z, fx, fy, cx, cy, rules=()):
    invz = F(1) / Z
    x, y = X * invz, Y * invz
    if "fma_to_image" in rules:      # fx*x + cx rounded once: the product of two floats is exact in double, the sum rounds to double and
        return (np.asarray(fx, D) * x + D(cx)).astype(F), (np.asarray(fy, D) * y + D(cy)).astype(F)       # then to float
    return fx * x + cx, fy * y + cy


def project(T, W, second, X, Y, Z, fx, fy, cx, cy, rules=()):
    """T: (H, 16) float32 as columns of shape (H, 1); X, Y, Z: (1, N)."""
    col = lambda k: T[:, k:k + 1]
    p0 = cv_gemm3(col(0), col(1), col(2), X, Y, Z, 1.0, col(3), 1.0)
    p1 = cv_gemm3(col(4), col(5), col(6), X, Y, Z, 1.0, col(7), 1.0)
    p2 = cv_gemm3(col(8), col(9), col(10), X, Y, Z, 1.0, col(11), 1.0)
    R, t = W["Rcam21"], W["tcam21"]
    c0 = cv_gemm3(R[0], R[1], R[2], p0, p1, p2, 1.0, t[0], 1.0)
    c1 = cv_gemm3(R[3], R[4], R[5], p0, p1, p2, 1.0, t[1], 1.0)
    c2 = cv_gemm3(R[6], R[7], R[8], p0, p1, p2, 1.0, t[2], 1.0)
    p0, p1, p2 = np.where(second, c0, p0), np.where(second, c1, p1), np.where(second, c2, p2)
    return to_image(p0, p1, p2, fx, fy, cx, cy, rules)


def check_inliers(W, T12, T21, rules=()):
    """-> (inlier (H, N) bool, err1, err2 (H, N) float32)."""
    with np.errstate(all="ignore"):
        X1 = np.asarray(W["x3dc1"], F).reshape(-1, 3); X2 = np.asarray(W["x3dc2"], F).reshape(-1, 3)
        row = lambda a: np.ascontiguousarray(a, F).reshape(1, -1)
        x1, y1, z1, x2, y2, z2 = row(X1[:, 0]), row(X1[:, 1]), row(X1[:, 2]), row(X2[:, 0]), row(X2[:, 1]), row(X2[:, 2])
        fx1, fy1, cx1, cy1 = (F(v) for v in W["K1"]); fx2, fy2, cx2, cy2 = (F(v) for v in W["K2"])
        u1, v1 = to_image(x1, y1, z1, fx1, fy1, cx1, cy1, rules)
        u2, v2 = to_image(x2, y2, z2, fx2, fy2, cx2, cy2, rules)
        s1 = (np.asarray(W["cam1"]) == 1).reshape(1, -1); s2 = (np.asarray(W["cam2"]) == 1).reshape(1, -1)
        pu, pv = project(T12, W, s2, x2, y2, z2, fx1, fy1, cx1, cy1, rules)
        d10, d11 = u1 - pu, v1 - pv
        pu, pv = project(T21, W, s1, x1, y1, z1, fx2, fy2, cx2, cy2, rules)
        d20, d21 = pu - u2, pv - v2
        if "float_sum" in rules:
            err1, err2 = d10 * d10 + d11 * d11, d20 * d20 + d21 * d21
        else:
            err1 = (d10.astype(D) * d10.astype(D) + d11.astype(D) * d11.astype(D)).astype(F)
            err2 = (d20.astype(D) * d20.astype(D) + d21.astype(D) * d21.astype(D)).astype(F)
        if "inlier_le" in rules:
            inl = (err1 <= row(W["max_err1"])) & (err2 <= row(W["max_err2"]))
        else:
            inl = (err1 < row(W["max_err1"])) & (err2 < row(W["max_err2"]))
    return inl, err1, err2


def canonical(a):
    """The NaN x86 makes from an invalid operation in place of every NaN."""
    a = np.ascontiguousarray(a, F).copy()
    a.view(np.uint32)[np.isnan(a)] = 0xffc00000
    return a


def pack_masks(inl):
    H, N = inl.shape
    Wd = (N + 63) // 64
    bits = np.zeros((H, Wd * 64), np.uint8)
    bits[:, :N] = inl
    return np.packbits(bits.reshape(H, Wd, 8, 8), axis=-1, bitorder="little").reshape(H, Wd, 8).copy().view("<u8").reshape(H, Wd)


def evaluate(W, order, rules=()):
    """A world (dict: K1, K2, Rcam21, tcam21, fix_scale, x3dc1, x3dc2, cam1, cam2, max_err1, max_err2, triples) -> (records HYP_DTYPE H,
    mask words (H, W) uint64, err1, err2 (H, N) float32).  rules: names of deliberately WRONG rules of the inlier phase (RULES: "<=" for
    "<", the sum of squares in float, a fused multiply-add in FromCameraToImage / Project's last step), which the boundary worlds must
    catch (tests/test_geometry_boundary_worlds.py)."""
    assert all(r in RULES for r in rules), rules
    X1 = np.asarray(W["x3dc1"], F).reshape(-1, 3); X2 = np.asarray(W["x3dc2"], F).reshape(-1, 3)
    tri = np.asarray(W["triples"], np.int64).reshape(-1, 3)
    H = len(tri)
    rec = np.zeros(H, HYP_DTYPE)
    for h in range(H):
        r = horn(X1[tri[h]].T, X2[tri[h]].T, W["fix_scale"], order)
        rec["R12"][h] = r["R"]; rec["t12"][h] = r["t"]; rec["s12"][h] = r["s"]; rec["T12"][h] = r["T12"]; rec["T21"][h] = r["T21"]
    for k in ("R12", "t12", "s12", "T12", "T21"):
        rec[k] = canonical(rec[k])
    Wm = dict(W, Rcam21=np.asarray(W["Rcam21"], F).reshape(9), tcam21=np.asarray(W["tcam21"], F).reshape(3))
    inl, e1, e2 = check_inliers(Wm, rec["T12"], rec["T21"], rules)
    if H:
        rec["n_inliers"] = inl.sum(axis=1)
    return rec, pack_masks(inl), e1, e2


# ---- the sequential parts -----------------------------------------------------------------------------------------------------------------
def draw_triples(N, H, randi):
    """The reference's take-and-swap procedure (:211-231) for H iterations; randi(n) = DUtils::Random::RandomInt(0, n - 1)."""
    out = []
    for _ in range(H):
        avail = list(range(N))
        tr = []
        for _ in range(3):
            r = randi(len(avail))
            tr.append(avail[r])
            avail[r] = avail[-1]
            avail.pop()
        out.append(tr)
    return np.array(out, np.int32).reshape(-1, 3)


def iterations(probability, min_inliers, max_its, N):
    """SetRansacParameters (:156-182) -> mRansacMaxIts.  log, pow and ceil are the C library's (math); a NaN or a value beyond int
    converts to INT_MIN, as x86's cvttsd2si does."""
    with np.errstate(all="ignore"):
        epsilon = float(F(min_inliers) / F(N))
    if min_inliers == N:
        n = 1
    else:
        d = math.nan
        if math.isfinite(epsilon):
            arg = 1 - math.pow(epsilon, 3)
            num = math.log(1 - probability)
            if arg > 0:
                den = math.log(arg)
                d = float(D(num) / D(den)) if den == den else math.nan
            elif arg == 0:
                d = float(D(num) / D(-math.inf))
        d = math.ceil(d) if math.isfinite(d) else d
        n = int(d) if math.isfinite(d) and -2147483648.0 <= d < 2147483648.0 else -2 ** 31
    return max(1, min(n, max_its))


class Iterate:
    """Sim3Solver::iterate (:186-263) over precomputed counts and masks: a direct transcription, members named as in the reference."""

    def __init__(self, counts, N, min_inliers, max_its):
        self.counts = list(counts); self.N = N
        self.mRansacMinInliers = min_inliers; self.mRansacMaxIts = max_its
        self.mnIterations = 0; self.mnBestInliers = 0; self.best = -1

    def iterate(self, nIterations):
        """-> (index of the hypothesis whose T12 is returned or -1 for the empty matrix, bNoMore, nInliers)"""
        bNoMore = False
        nInliers = 0
        if self.N < self.mRansacMinInliers:
            return -1, True, 0
        nCurrentIterations = 0
        while self.mnIterations < self.mRansacMaxIts and nCurrentIterations < nIterations:
            nCurrentIterations += 1
            h = self.mnIterations
            self.mnIterations += 1
            mnInliersi = self.counts[h]
            if mnInliersi >= self.mnBestInliers:
                self.mnBestInliers = mnInliersi
                self.best = h
                if mnInliersi > self.mRansacMinInliers:
                    nInliers = mnInliersi
                    return h, bNoMore, nInliers
        if self.mnIterations >= self.mRansacMaxIts:
            bNoMore = True
        return -1, bNoMore, nInliers
