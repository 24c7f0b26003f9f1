"""A NumPy model of PnPsolver (reference src/PnPsolver.cc) and of the OpenCV operators it calls, written from the reference's statements and
OpenCV's published sources (modules/core/src/lapack.cpp, matmul.cpp; 3.2), independent of the C++ of this repository.

Every scalar of the reference is an array with one element per hypothesis here (the batch axis comes first), every statement one
elementwise NumPy operation in float64 -- IEEE double, one rounding per operation, no contraction -- and every sum a Python loop in the
reference's element order.  Data-dependent branches become np.where over the batch; the two rare ones (the random completion of the
SVD and nothing else) drop to a scalar routine for the hypotheses that take them.  The n-point pose of Refine() is the same code with
a batch of one.

The one definition the reference leaves open is stated in include/orbm.h: gauss_newton's x starts as zeros and a singular qr_solve
leaves it as it was."""
import math
import numpy as np

DBL_EPS = float(np.finfo(np.float64).eps)
DBL_MIN = float(np.finfo(np.float64).tiny)
FLAG_SINGULAR_QR, FLAG_RANDOM_SVD = 1, 2
MAX_RECORDS = 16
X86_NAN = np.frombuffer(np.uint64(0xfff8000000000000).tobytes(), np.float64)[0]


def x86_nan(a):
    """A NaN leaves as the NaN x86 makes from an invalid operation."""
    a = np.array(a, np.float64)
    a[np.isnan(a)] = X86_NAN
    return a


def _seqsum(terms):
    """The running sum 0 + t0 + t1 + ... over the LAST axis, in order."""
    s = np.zeros(terms.shape[:-1])
    for k in range(terms.shape[-1]):
        s = s + terms[..., k]
    return s


# ---- OpenCV ----------------------------------------------------------------------------------------------------------------------
class CvRNG:
    def __init__(self, state=0x12345678):
        self.state = state

    def next(self):
        self.state = ((self.state & 0xffffffff) * 4164903690 + (self.state >> 32)) & 0xffffffffffffffff
        return self.state & 0xffffffff


def _complete_one(At, W):
    """JacobiSVDImpl_'s last loop for ONE matrix (At n x m, W n), scalar Python floats; returns whether the random branch ran."""
    n, m = At.shape
    eps = DBL_EPS * 10
    rng = CvRNG()
    random = False
    for i in range(n):
        sd = float(W[i])
        ii = 0
        while ii < 100 and sd <= DBL_MIN:
            random = True
            val0 = 1. / m
            for k in range(m):
                At[i, k] = val0 if (rng.next() & 256) != 0 else -val0
            for _ in range(2):
                for j in range(i):
                    sd = 0.0
                    for k in range(m):
                        sd += float(At[i, k]) * float(At[j, k])
                    asum = 0.0
                    for k in range(m):
                        t = float(At[i, k]) - sd * float(At[j, k])
                        At[i, k] = t
                        asum += abs(t)
                    asum = 1 / asum if asum > eps * 100 else 0.0
                    for k in range(m):
                        At[i, k] = float(At[i, k]) * asum
            sd = 0.0
            for k in range(m):
                t = float(At[i, k])
                sd += t * t
            sd = math.sqrt(sd)
            ii += 1
        s = 1 / sd if sd > DBL_MIN else 0.
        for k in range(m):
            At[i, k] = float(At[i, k]) * s
    return random


def jacobi_svd(A, want_vt=True):
    """cv::SVD::compute / cvSVD of a batch of m x n matrices (H, m, n), m >= n: JacobiSVDImpl_<double> on the transposes.
    -> w (H, n), ut (H, n, m) = U transposed, vt (H, n, n), random (H,) bool."""
    A = np.asarray(A, np.float64)
    H, m, n = A.shape
    At = np.ascontiguousarray(np.transpose(A, (0, 2, 1)))
    eps = DBL_EPS * 10
    W = np.zeros((H, n))
    Vt = np.zeros((H, n, n))
    for i in range(n):
        W[:, i] = _seqsum(At[:, i, :] * At[:, i, :])
        Vt[:, i, i] = 1
    with np.errstate(all="ignore"):
        for _ in range(max(m, 30)):
            changed = False
            for i in range(n - 1):
                for j in range(i + 1, n):
                    a = W[:, i].copy(); b = W[:, j].copy()
                    p = _seqsum(At[:, i, :] * At[:, j, :])
                    rot = ~(np.abs(p) <= eps * np.sqrt(a * b))
                    if not rot.any():
                        continue
                    changed = True
                    p = p * 2
                    beta = a - b
                    gamma = np.sqrt(p * p + beta * beta)          # hypot as cv_hypot_libm: the stated stand-in for libm's
                    delta = (gamma - beta) * 0.5
                    s1 = np.sqrt(delta / gamma); c1 = p / (gamma * s1 * 2)
                    c2 = np.sqrt((gamma + beta) / (gamma * 2)); s2 = p / (gamma * c2 * 2)
                    neg = beta < 0
                    c = np.where(neg, c1, c2)[:, None]; s = np.where(neg, s1, s2)[:, None]
                    x = At[:, i, :].copy(); y = At[:, j, :].copy()
                    t0 = c * x + s * y
                    t1 = -s * x + c * y
                    r = rot[:, None]
                    At[:, i, :] = np.where(r, t0, x); At[:, j, :] = np.where(r, t1, y)
                    W[:, i] = np.where(rot, _seqsum(t0 * t0), a); W[:, j] = np.where(rot, _seqsum(t1 * t1), b)
                    if want_vt:
                        x = Vt[:, i, :].copy(); y = Vt[:, j, :].copy()
                        Vt[:, i, :] = np.where(r, c * x + s * y, x); Vt[:, j, :] = np.where(r, -s * x + c * y, y)
            if not changed:
                break
        for i in range(n):
            W[:, i] = np.sqrt(_seqsum(At[:, i, :] * At[:, i, :]))
        ar = np.arange(H)
        for i in range(n - 1):
            j = np.full(H, i)
            for k in range(i + 1, n):
                j = np.where(W[ar, j] < W[:, k], k, j)
            wi = W[:, i].copy(); W[:, i] = W[ar, j]; W[ar, j] = wi
            ri = At[:, i, :].copy(); At[:, i, :] = At[ar, j, :]; At[ar, j, :] = ri
            ri = Vt[:, i, :].copy(); Vt[:, i, :] = Vt[ar, j, :]; Vt[ar, j, :] = ri
        random = np.zeros(H, bool)
        small = (W <= DBL_MIN).any(axis=1)
        for h in np.nonzero(small)[0]:
            random[h] = _complete_one(At[h], W[h])
        ok = ~small
        s = np.where(W[ok] > DBL_MIN, 1 / W[ok], 0.)
        At[ok] = At[ok] * s[:, :, None]
    return W, At, Vt, random


def backsubst_vec(w, ut, vt, b):
    """SVBkSb with one right-hand side (cvSolve(A, b, x, CV_SVD)): w (H, n), ut (H, n, m), vt (H, n, n), b (H, m) -> x (H, n)."""
    H, n, m = ut.shape
    x = np.zeros((H, n))
    thr = _seqsum(w) * (DBL_EPS * 2)
    with np.errstate(all="ignore"):
        for i in range(n):
            use = ~(np.abs(w[:, i]) <= thr)
            wi = 1 / w[:, i]
            s = _seqsum(ut[:, i, :] * b) * wi
            x = np.where(use[:, None], x + s[:, None] * vt[:, i, :], x)
    return x


def backsubst_inv(w, ut, vt):
    """SVBkSb without a right-hand side (cvInvert(A, Ainv, CV_SVD)), n x n -> (H, n, n)."""
    H, n, _ = ut.shape
    x = np.zeros((H, n, n))
    thr = _seqsum(w) * (DBL_EPS * 2)
    with np.errstate(all="ignore"):
        for i in range(n):
            use = ~(np.abs(w[:, i]) <= thr)
            wi = 1 / w[:, i]
            buf = ut[:, i, :] * wi[:, None]                       # buffer[j] = u[j][i] * wi
            x = np.where(use[:, None, None], x + vt[:, i, :, None] * buf[:, None, :], x)
    return x


# ---- PnPsolver.cc ----------------------------------------------------------------------------------------------------------------
def qr_solve(A, b, X):
    """qr_solve (:866-956) on a batch: A (H, nr, nc), b (H, nr), X (H, nc) as it is on entry -> (X, singular (H,)).  The first loop of
    every column starts at A[k][k] AGAIN and advances after the comparison: row nr-1 is never looked at."""
    A = np.array(A, np.float64); b = np.array(b, np.float64); X = np.array(X, np.float64)
    H, nr, nc = A.shape
    A1 = np.zeros((H, nc)); A2 = np.zeros((H, nc))
    sing = np.zeros(H, bool)
    with np.errstate(all="ignore"):
        for k in range(nc):
            eta = np.abs(A[:, k, k])
            for i in range(k + 1, nr):
                elt = np.abs(A[:, i - 1, k])
                eta = np.where(eta < elt, elt, eta)
            sing |= eta == 0
            inv_eta = 1. / eta
            ssum = np.zeros(H)
            for i in range(k, nr):
                A[:, i, k] = A[:, i, k] * inv_eta
                ssum = ssum + A[:, i, k] * A[:, i, k]
            sigma = np.sqrt(ssum)
            sigma = np.where(A[:, k, k] < 0, -sigma, sigma)
            A[:, k, k] = A[:, k, k] + sigma
            A1[:, k] = sigma * A[:, k, k]
            A2[:, k] = -eta * sigma
            for j in range(k + 1, nc):
                s = np.zeros(H)
                for i in range(k, nr):
                    s = s + A[:, i, k] * A[:, i, j]
                tau = s / A1[:, k]
                for i in range(k, nr):
                    A[:, i, j] = A[:, i, j] - tau * A[:, i, k]
        for j in range(nc):
            tau = np.zeros(H)
            for i in range(j, nr):
                tau = tau + A[:, i, j] * b[:, i]
            tau = tau / A1[:, j]
            for i in range(j, nr):
                b[:, i] = b[:, i] - tau * A[:, i, j]
        Xn = np.zeros((H, nc))
        Xn[:, nc - 1] = b[:, nc - 1] / A2[:, nc - 1]
        for i in range(nc - 2, -1, -1):
            s = np.zeros(H)
            for j in range(i + 1, nc):
                s = s + A[:, i, j] * Xn[:, j]
            Xn[:, i] = (b[:, i] - s) / A2[:, i]
    return np.where(sing[:, None], X, Xn), sing


def _dot3(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def numpy_svd(A, want_vt=True):
    """numpy.linalg.svd in the place of jacobi_svd (same return values): the float64 reference EPnP of tests/test_pnp_numeric.py."""
    U, w, Vt = np.linalg.svd(np.asarray(A, np.float64), full_matrices=False)
    return w, np.ascontiguousarray(np.transpose(U, (0, 2, 1))), Vt, np.zeros(len(A), bool)


def compute_pose(pws, us, K, svd=None):
    """compute_pose (:483-531) of a batch: pws (H, n, 3), us (H, n, 2) float64, K (H, 4) = fu fv uc vc
    -> dict R (H, 3, 3), t (H, 3), err (H,), choice (H,), flags (H,).  svd: what stands for cvSVD (jacobi_svd; numpy_svd for the reference
    EPnP of the numeric test)."""
    svd = jacobi_svd if svd is None else svd
    pws = np.asarray(pws, np.float64); us = np.asarray(us, np.float64); K = np.asarray(K, np.float64)
    H, n, _ = pws.shape
    fu, fv, uc, vc = K[:, 0], K[:, 1], K[:, 2], K[:, 3]
    flags = np.zeros(H, np.int32)
    dn = float(n)
    with np.errstate(all="ignore"):
        # choose_control_points
        cws = np.zeros((H, 4, 3))
        s = np.zeros((H, 3))
        for i in range(n):
            s = s + pws[:, i, :]
        cws[:, 0, :] = s / dn
        PW0 = pws - cws[:, None, 0, :]
        pw0tpw0 = np.zeros((H, 3, 3))
        for i in range(n):                                          # cvMulTransposed: every element one running sum over the rows
            pw0tpw0 = pw0tpw0 + PW0[:, i, :, None] * PW0[:, i, None, :]
        iu = np.triu_indices(3)
        pw0tpw0[:, iu[1], iu[0]] = pw0tpw0[:, iu[0], iu[1]]         # the upper triangle is computed, then mirrored
        dc, uct, _, rnd = svd(pw0tpw0, False)
        flags[rnd] |= FLAG_RANDOM_SVD
        for i in range(1, 4):
            k = np.sqrt(dc[:, i - 1] / dn)
            cws[:, i, :] = cws[:, 0, :] + k[:, None] * uct[:, i - 1, :]
        # compute_barycentric_coordinates
        cc = np.zeros((H, 3, 3))
        for i in range(3):
            for j in range(1, 4):
                cc[:, i, j - 1] = cws[:, j, i] - cws[:, 0, i]
        w, ut3, vt3, rnd = svd(cc, True)
        flags[rnd] |= FLAG_RANDOM_SVD
        ci = backsubst_inv(w, ut3, vt3)
        d = pws - cws[:, None, 0, :]
        alphas = np.zeros((H, n, 4))
        for j in range(3):
            alphas[:, :, 1 + j] = ci[:, None, j, 0] * d[:, :, 0] + ci[:, None, j, 1] * d[:, :, 1] + ci[:, None, j, 2] * d[:, :, 2]
        alphas[:, :, 0] = 1.0 - alphas[:, :, 1] - alphas[:, :, 2] - alphas[:, :, 3]
        # fill_M, cvMulTransposed(M, MtM, 1)
        mtm = np.zeros((H, 12, 12))
        for i in range(n):
            M1 = np.zeros((H, 12)); M2 = np.zeros((H, 12))
            for q in range(4):
                a = alphas[:, i, q]
                M1[:, 3 * q] = a * fu; M1[:, 3 * q + 2] = a * (uc - us[:, i, 0])
                M2[:, 3 * q + 1] = a * fv; M2[:, 3 * q + 2] = a * (vc - us[:, i, 1])
            mtm = mtm + M1[:, :, None] * M1[:, None, :]
            mtm = mtm + M2[:, :, None] * M2[:, None, :]
        iu = np.triu_indices(12)
        mtm[:, iu[1], iu[0]] = mtm[:, iu[0], iu[1]]
        _, ut, _, rnd = svd(mtm, False)
        flags[rnd] |= FLAG_RANDOM_SVD
        # compute_L_6x10, compute_rho
        v = [ut[:, 11 - i, :].reshape(H, 4, 3) for i in range(4)]
        pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
        L = np.zeros((H, 6, 10)); rho = np.zeros((H, 6))
        for j, (a, b) in enumerate(pairs):
            dv = [v[i][:, a, :] - v[i][:, b, :] for i in range(4)]
            L[:, j, 0] = _dot3(dv[0], dv[0]); L[:, j, 1] = 2.0 * _dot3(dv[0], dv[1]); L[:, j, 2] = _dot3(dv[1], dv[1])
            L[:, j, 3] = 2.0 * _dot3(dv[0], dv[2]); L[:, j, 4] = 2.0 * _dot3(dv[1], dv[2]); L[:, j, 5] = _dot3(dv[2], dv[2])
            L[:, j, 6] = 2.0 * _dot3(dv[0], dv[3]); L[:, j, 7] = 2.0 * _dot3(dv[1], dv[3]); L[:, j, 8] = 2.0 * _dot3(dv[2], dv[3])
            L[:, j, 9] = _dot3(dv[3], dv[3])
            e = cws[:, a, :] - cws[:, b, :]
            rho[:, j] = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2]
        best = None
        negs = []
        for approx in (1, 2, 3):
            cols = {1: [0, 1, 3, 6], 2: [0, 1, 2], 3: [0, 1, 2, 3, 4]}[approx]
            w, utk, vtk, rnd = svd(L[:, :, cols], True)
            flags[rnd] |= FLAG_RANDOM_SVD
            bb = backsubst_vec(w, utk, vtk, rho)
            betas = np.zeros((H, 4))
            neg0 = bb[:, 0] < 0
            if approx == 1:
                b0 = np.where(neg0, np.sqrt(-bb[:, 0]), np.sqrt(bb[:, 0]))
                betas[:, 0] = b0
                for k in (1, 2, 3):
                    betas[:, k] = np.where(neg0, -bb[:, k] / b0, bb[:, k] / b0)
            else:
                b0 = np.where(neg0, np.sqrt(-bb[:, 0]), np.sqrt(bb[:, 0]))
                betas[:, 1] = np.where(neg0, np.where(bb[:, 2] < 0, np.sqrt(-bb[:, 2]), 0.0), np.where(bb[:, 2] > 0, np.sqrt(bb[:, 2]), 0.0))
                b0 = np.where(bb[:, 1] < 0, -b0, b0)
                betas[:, 0] = b0
                if approx == 3:
                    betas[:, 2] = bb[:, 3] / b0
            # gauss_newton
            x = np.zeros((H, 4))
            for _ in range(5):
                A = np.zeros((H, 6, 4)); b = np.zeros((H, 6))
                b0, b1, b2, b3 = betas[:, 0], betas[:, 1], betas[:, 2], betas[:, 3]
                for i in range(6):
                    r = [L[:, i, k] for k in range(10)]
                    A[:, i, 0] = 2 * r[0] * b0 + r[1] * b1 + r[3] * b2 + r[6] * b3
                    A[:, i, 1] = r[1] * b0 + 2 * r[2] * b1 + r[4] * b2 + r[7] * b3
                    A[:, i, 2] = r[3] * b0 + r[4] * b1 + 2 * r[5] * b2 + r[8] * b3
                    A[:, i, 3] = r[6] * b0 + r[7] * b1 + r[8] * b2 + 2 * r[9] * b3
                    b[:, i] = rho[:, i] - (r[0] * b0 * b0 + r[1] * b0 * b1 + r[2] * b1 * b1 + r[3] * b0 * b2 + r[4] * b1 * b2 +
                                           r[5] * b2 * b2 + r[6] * b0 * b3 + r[7] * b1 * b3 + r[8] * b2 * b3 + r[9] * b3 * b3)
                x, sing = qr_solve(A, b, x)
                flags[sing] |= FLAG_SINGULAR_QR
                betas = betas + x
            # compute_ccs, compute_pcs, solve_for_sign
            ccs = np.zeros((H, 4, 3))
            for i in range(4):
                ccs = ccs + betas[:, i, None, None] * v[i]
            pcs = np.zeros((H, n, 3))
            for j in range(3):
                pcs[:, :, j] = (alphas[:, :, 0] * ccs[:, None, 0, j] + alphas[:, :, 1] * ccs[:, None, 1, j] + alphas[:, :, 2] * ccs[:, None, 2, j] +
                                alphas[:, :, 3] * ccs[:, None, 3, j])
            neg = pcs[:, 0, 2] < 0.0
            negs.append(neg)
            pcs = np.where(neg[:, None, None], -pcs, pcs)
            # estimate_R_and_t
            pc0 = np.zeros((H, 3)); pw0 = np.zeros((H, 3))
            for i in range(n):
                pc0 = pc0 + pcs[:, i, :]; pw0 = pw0 + pws[:, i, :]
            pc0 = pc0 / dn; pw0 = pw0 / dn
            abt = np.zeros((H, 3, 3))
            for i in range(n):
                abt = abt + (pcs[:, i, :] - pc0)[:, :, None] * (pws[:, i, :] - pw0)[:, None, :]
            _, utr, vtr, rnd = svd(abt, True)
            flags[rnd] |= FLAG_RANDOM_SVD
            U = np.transpose(utr, (0, 2, 1)); V = np.transpose(vtr, (0, 2, 1))
            R = np.zeros((H, 3, 3))
            for i in range(3):
                for j in range(3):
                    R[:, i, j] = U[:, i, 0] * V[:, j, 0] + U[:, i, 1] * V[:, j, 1] + U[:, i, 2] * V[:, j, 2]
            det = (R[:, 0, 0] * R[:, 1, 1] * R[:, 2, 2] + R[:, 0, 1] * R[:, 1, 2] * R[:, 2, 0] + R[:, 0, 2] * R[:, 1, 0] * R[:, 2, 1] -
                   R[:, 0, 2] * R[:, 1, 1] * R[:, 2, 0] - R[:, 0, 1] * R[:, 1, 0] * R[:, 2, 2] - R[:, 0, 0] * R[:, 1, 2] * R[:, 2, 1])
            R[:, 2, :] = np.where((det < 0)[:, None], -R[:, 2, :], R[:, 2, :])
            t = np.stack([pc0[:, i] - _dot3(R[:, i, :], pw0) for i in range(3)], 1)
            # reprojection_error
            Xc = _dot3(R[:, None, 0, :], pws) + t[:, None, 0]
            Yc = _dot3(R[:, None, 1, :], pws) + t[:, None, 1]
            inv_Zc = 1.0 / (_dot3(R[:, None, 2, :], pws) + t[:, None, 2])
            ue = uc[:, None] + fu[:, None] * Xc * inv_Zc
            ve = vc[:, None] + fv[:, None] * Yc * inv_Zc
            du = us[:, :, 0] - ue; dv_ = us[:, :, 1] - ve
            err = _seqsum(np.sqrt(du * du + dv_ * dv_)) / dn
            if best is None:
                best = {"R": R, "t": t, "err": err, "choice": np.full(H, 1, np.int32)}
            else:
                take = err < best["err"]
                best["R"] = np.where(take[:, None, None], R, best["R"]); best["t"] = np.where(take[:, None], t, best["t"])
                best["err"] = np.where(take, err, best["err"]); best["choice"] = np.where(take, approx, best["choice"]).astype(np.int32)
    best["flags"] = flags
    best["neg"] = np.stack(negs, 1)                                  # (inspection) solve_for_sign's test, per approximation
    return best


def errors2(R, t, K, p3dw, p2d):
    """error2 of CheckInliers (:314-341) of a batch of poses on one correspondence list: R (H, 3, 3), t (H, 3) float64, K = fu fv uc vc,
    p3dw (N, 3), p2d (N, 2) -> float32 (H, N)."""
    p3dw = np.asarray(p3dw, np.float32); p2d = np.asarray(p2d, np.float32)
    X = p3dw.astype(np.float64)
    fu, fv, uc, vc = [float(k) for k in K]
    with np.errstate(all="ignore"):
        row = lambda r: R[:, None, r, 0] * X[None, :, 0] + R[:, None, r, 1] * X[None, :, 1] + R[:, None, r, 2] * X[None, :, 2] + t[:, None, r]
        Xc = row(0).astype(np.float32); Yc = row(1).astype(np.float32)
        invZc = (1 / row(2)).astype(np.float32)
        ue = uc + fu * Xc.astype(np.float64) * invZc.astype(np.float64)
        ve = vc + fv * Yc.astype(np.float64) * invZc.astype(np.float64)
        distX = (p2d[None, :, 0].astype(np.float64) - ue).astype(np.float32)
        distY = (p2d[None, :, 1].astype(np.float64) - ve).astype(np.float32)
        return distX * distX + distY * distY


def check_inliers(R, t, K, p3dw, p2d, max_err):
    """CheckInliers (:314-345): `error2 < mvMaxError[i]`; max_err (N,) float32 -> bool (H, N)."""
    with np.errstate(all="ignore"):
        return errors2(R, t, K, p3dw, p2d) < np.asarray(max_err, np.float32)[None, :]


def mask_words(inl):
    """bool (..., N) -> uint64 words (..., W), bit i & 63 of word i >> 6."""
    N = inl.shape[-1]
    W = (N + 63) // 64
    pad = np.zeros(inl.shape[:-1] + (W * 64,), np.uint8)
    pad[..., :N] = inl
    return np.packbits(pad.reshape(inl.shape[:-1] + (W, 64)), axis=-1, bitorder="little").view("<u8").reshape(inl.shape[:-1] + (W,))


def records(counts, min_inliers, best_start):
    """The hypotheses `iterate` copies into mvbBestInliers, in order: strict prefix maxima above best_start among counts >= min_inliers."""
    out, best = [], best_start
    for h, c in enumerate(counts):
        if c >= min_inliers and c > best:
            best = c
            out.append(h)
    return out


def hypotheses_multi(problems):
    """The four-point poses of several problems in ONE batch; problems: dicts K p3dw p2d max_err quads min_inliers best_start
    -> per problem (pose dict, inliers bool (H, N))."""
    pws, us, Ks = [], [], []
    for p in problems:
        q = np.asarray(p["quads"], np.int64).reshape(-1, 4)
        pws.append(np.asarray(p["p3dw"], np.float32)[q].astype(np.float64).reshape(-1, 4, 3))
        us.append(np.asarray(p["p2d"], np.float32)[q].astype(np.float64).reshape(-1, 4, 2))
        Ks.append(np.tile(np.asarray([float(np.float32(k)) for k in p["K"]]), (len(q), 1)).reshape(-1, 4))
    total = sum(len(x) for x in pws)
    allp = compute_pose(np.concatenate(pws), np.concatenate(us), np.concatenate(Ks)) if total else None
    out, h0 = [], 0
    for p, x in zip(problems, pws):
        H = len(x)
        if H:
            pose = {k: allp[k][h0:h0 + H] for k in ("R", "t", "err", "choice", "flags")}
        else:
            pose = {"R": np.zeros((0, 3, 3)), "t": np.zeros((0, 3)), "err": np.zeros(0), "choice": np.zeros(0, np.int32), "flags": np.zeros(0, np.int32)}
        K = [float(np.float32(k)) for k in p["K"]]
        N = len(np.asarray(p["p3dw"]).reshape(-1, 3))
        inl = check_inliers(pose["R"], pose["t"], K, p["p3dw"], p["p2d"], p["max_err"]) if H else np.zeros((0, N), bool)
        out.append((pose, inl))
        h0 += H
    return out


def refine(p, inl_row):
    """Refine() (:266-311) on one mask -> (pose dict of a batch of one, inliers bool (N,))."""
    idx = np.nonzero(inl_row)[0]
    K = [float(np.float32(k)) for k in p["K"]]
    pose = compute_pose(np.asarray(p["p3dw"], np.float32)[idx].astype(np.float64)[None], np.asarray(p["p2d"], np.float32)[idx].astype(np.float64)[None],
                        np.asarray(K)[None])
    return pose, check_inliers(pose["R"], pose["t"], K, p["p3dw"], p["p2d"], p["max_err"])[0]


def ransac_multi(problems):
    """What orbm_pnp_ransac answers -> per problem dict: R t err choice flags n_inliers (per hypothesis), words (H, W), rec (list of
    hypotheses), ref_R ref_t ref_flags ref_n_inliers ref_n_set (per record), ref_words (R, W)."""
    res = []
    for p, (pose, inl) in zip(problems, hypotheses_multi(problems)):
        counts = inl.sum(axis=1).astype(np.int32)
        rec = records(counts, p["min_inliers"], p.get("best_start", 0))
        N = inl.shape[1]
        d = {"R": x86_nan(pose["R"]), "t": x86_nan(pose["t"]), "err": x86_nan(pose["err"]), "choice": pose["choice"], "flags": pose["flags"],
             "n_inliers": counts, "words": mask_words(inl), "rec": rec, "ref_R": np.zeros((len(rec), 3, 3)), "ref_t": np.zeros((len(rec), 3)),
             "ref_flags": np.zeros(len(rec), np.int32), "ref_n_inliers": np.zeros(len(rec), np.int32), "ref_n_set": np.zeros(len(rec), np.int32),
             "ref_words": np.zeros((len(rec), (N + 63) // 64), np.uint64)}
        for r, h in enumerate(rec):
            rp, rin = refine(p, inl[h])
            d["ref_R"][r] = x86_nan(rp["R"][0]); d["ref_t"][r] = x86_nan(rp["t"][0]); d["ref_flags"][r] = rp["flags"][0]
            d["ref_n_inliers"][r] = rin.sum(); d["ref_n_set"][r] = counts[h]; d["ref_words"][r] = mask_words(rin)
        res.append(d)
    return res


# ---- iterate and SetRansacParameters ---------------------------------------------------------------------------------------------
class IterateModel:
    """PnPsolver::iterate (:171-264) transcribed, over evaluated hypotheses: counts[h] = mnInliersi of iteration h, refined(h) -> the
    mnRefinedInliers of Refine() on the mask of hypothesis h (a function of the current best record alone)."""

    def __init__(self, N, min_inliers, max_its):
        self.N, self.min_inliers, self.max_its = N, min_inliers, max_its
        self.iterations = 0; self.best_inliers = 0; self.best_hyp = -1

    def iterate(self, n_iterations, counts, refined):
        """-> (answer, no_more, index): ('refined', hypothesis of the best record) / ('best', best hypothesis) / ('nothing', -1)"""
        no_more = False
        if self.N < self.min_inliers:
            return "nothing", True, -1
        current = 0
        while self.iterations < self.max_its or current < n_iterations:
            current += 1
            h = self.iterations
            self.iterations += 1
            n = counts[h]
            if n >= self.min_inliers:
                if n > self.best_inliers:
                    self.best_inliers = n
                    self.best_hyp = h
                if refined(self.best_hyp) > self.min_inliers:
                    return "refined", no_more, self.best_hyp
        if self.iterations >= self.max_its:
            no_more = True
            if self.best_inliers >= self.min_inliers:
                return "best", no_more, self.best_hyp
        return "nothing", no_more, -1


def _cvtt(x):
    return int(x) if (x == x and -2147483648.0 <= x < 2147483648.0) else -2147483648


def parameters(N, probability=0.99, min_inliers=8, max_its=300, min_set=4, epsilon=0.4):
    """SetRansacParameters (:126-162) -> (mRansacMaxIts, mRansacMinInliers, mRansacEpsilon float32)."""
    eps = np.float32(epsilon)
    with np.errstate(all="ignore"):
        n_min = _cvtt(float(np.float32(N) * eps))
        n_min = max(n_min, min_inliers)
        n_min = max(n_min, min_set)
        ratio = np.float32(n_min) / np.float32(N)
        if eps < ratio:
            eps = ratio
        if n_min == N:
            its = 1
        else:
            e = float(eps)
            den = math.log(1 - e ** 3) if 1 - e ** 3 > 0 else (float("-inf") if 1 - e ** 3 == 0 else float("nan"))
            num = math.log(1 - probability)
            q = num / den if den != 0 else (float("inf") if num > 0 else float("-inf") if num < 0 else float("nan"))
            its = _cvtt(math.ceil(q)) if (q == q and abs(q) != float("inf")) else -2147483648
    return max(1, min(its, max_its)), n_min, eps
