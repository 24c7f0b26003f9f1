"""orbm_pnp_svd (the restated cvSVD: one-sided Jacobi with the completion that makes U) against numpy.linalg.svd on the five shapes
PnPsolver uses, including a rank-8 12x12 built as M^T M from four points -- the case EPnP lives on: it reads the four rows of Ut that
belong to the (almost) zero singular values.

Bounds.  Both algorithms are backward stable: the computed factors are exact for A + E with |E| <= p(m, n) * eps * |A|_2, p a small
polynomial; p = m * n is taken.  B = m * n * DBL_EPSILON * w_max is therefore the unit for singular values (Weyl) and for the residual
u^T A of a null row, and Jacobi's own stopping rule (|u_i . u_j| <= 10 * DBL_EPSILON for normalised rows) the unit for U^T U - I.  The
same quantities are measured for numpy's factors, and one order of magnitude over the larger of the two is allowed: the null-space
basis of the two differs, its quality may not.  The measured values are printed before they are asserted."""
import numpy as np
import multi_orb_slam_amd as m
import pnp_worlds as pw

EPS = float(np.finfo(np.float64).eps)


def rank8_mtm(seed):
    w = pw.world(4, 0.0, 0.0, seed=seed, H=1)
    pws = w["p3dw"].astype(np.float64); us = w["p2d"].astype(np.float64)
    fu, fv, uc, vc = [float(np.float32(k)) for k in w["K"]]
    alphas = np.random.default_rng(seed).normal(size=(4, 4)); alphas /= alphas.sum(axis=1, keepdims=True)
    M = np.zeros((8, 12))
    for i in range(4):
        for q in range(4):
            M[2 * i, 3 * q] = alphas[i, q] * fu; M[2 * i, 3 * q + 2] = alphas[i, q] * (uc - us[i, 0])
            M[2 * i + 1, 3 * q + 1] = alphas[i, q] * fv; M[2 * i + 1, 3 * q + 2] = alphas[i, q] * (vc - us[i, 1])
    return M.T @ M


def cases():
    rng = np.random.default_rng(4)
    out = [("%dx%d" % s, rng.normal(size=s)) for s in ((3, 3), (12, 12), (6, 3), (6, 4), (6, 5)) for _ in range(5)]
    out += [("rank8_12x12", rank8_mtm(s)) for s in range(5)]
    return out


def quality(A, w, ut, null_from):
    """(max |U^T U - I|, max |u A| over the rows from null_from on) of a factorisation."""
    n = len(w)
    g = np.abs(ut @ ut.T - np.eye(n)).max()
    r = np.abs(ut[null_from:] @ A).max() if null_from < n else 0.0
    return g, r


def test_svd_against_numpy():
    for name, A in cases():
        m_, n = A.shape
        w, ut, vt, random = m.pnp_svd(A)
        U, wn, Vtn = np.linalg.svd(A, full_matrices=False)
        B = m_ * n * EPS * wn[0]
        null_from = 8 if name.startswith("rank8") else n
        g, r = quality(A, w, ut, null_from)
        gn, rn = quality(A, wn, U.T, null_from)
        dw = np.abs(w - wn).max()
        rec = np.abs((ut.T * w) @ vt - A).max()
        print("%-12s  |w - w_np| %.3e (unit %.3e)  U^T U - I %.3e (numpy %.3e)  null residual %.3e (numpy %.3e, unit %.3e)  |U W Vt - A| %.3e"
              % (name, dw, B, g, gn, r, rn, B, rec))
        assert not random
        assert dw <= 10 * B
        assert g <= 10 * max(gn, 10 * EPS)
        assert r <= 10 * max(rn, B)
        assert rec <= 10 * B
        assert (np.diff(w) <= 0).all()          # sorted, descending


# ---- the poses are geometrically right: reprojection on noise-free worlds -----------------------------------------------------------
# The reference quantity is measured on a float64 NumPy EPnP: tests/pnp_model.py's transcription with numpy.linalg.svd in the place of
# the restated cvSVD (another null-space basis, the same algorithm).  One order of magnitude over it is allowed.  A four-point EPnP
# is NOT exact -- its four null vectors are fitted by three approximations and five Gauss-Newton steps -- so for the RANSAC hypotheses
# the quantity is a distribution over the hypotheses (its median and its maximum, over the non-degenerate quadruples: third singular
# value of the centred points above 0.05 of the first), and the share of hypotheses that land within 0.01 px may not be smaller than
# half the reference's.  The n-point pose over all points of a world is exact up to the float32 inputs, and is held to ten times the
# reference's error.
import pnp_model as pm  # noqa: E402

NOISE_FREE = (15, 63, 64, 65, 300)


def reprojection(R, t, w):
    """max over the world's points of the distance between projection and observation, per pose (float64; a non-finite one is inf)"""
    X = w["p3dw"].astype(np.float64)
    K = [float(np.float32(k)) for k in w["K"]]
    Xc = np.einsum("hij,nj->hni", np.asarray(R, np.float64).reshape(-1, 3, 3), X) + np.asarray(t, np.float64).reshape(-1, 1, 3)
    with np.errstate(all="ignore"):
        u = K[0] * Xc[..., 0] / Xc[..., 2] + K[2]
        v = K[1] * Xc[..., 1] / Xc[..., 2] + K[3]
        d = np.hypot(u - w["p2d"][None, :, 0].astype(np.float64), v - w["p2d"][None, :, 1].astype(np.float64))
    return np.nan_to_num(d, nan=np.inf).max(axis=1)


def test_poses_reproject_the_points_of_noise_free_worlds():
    for N in NOISE_FREE:
        w = pw.world(N, 0.0, 0.0, seed=3000 + N, H=300)
        q = w["quads"]
        P = w["p3dw"][q].astype(np.float64); us = w["p2d"][q].astype(np.float64)
        Kd = np.array([float(np.float32(k)) for k in w["K"]])
        sv = np.linalg.svd(P - P.mean(axis=1, keepdims=True), compute_uv=False)
        good = sv[:, 2] / sv[:, 0] > 0.05
        assert good.sum() > 200
        hyp = m.pnp_ransac_host([pw.problem(m, w)])[0][0]
        lib = reprojection(hyp["R"], hyp["t"], w)[good]
        ref = pm.compute_pose(P, us, np.tile(Kd, (len(q), 1)), svd=pm.numpy_svd)
        ref = reprojection(ref["R"], ref["t"], w)[good]
        # the n-point pose over all points
        allp, allu = w["p3dw"].astype(np.float64), w["p2d"].astype(np.float64)
        R, t, err, choice, flags = m.pnp_compute_pose(allp, allu, Kd)
        lib_n = reprojection(R, t, w)[0]
        rn = pm.compute_pose(allp[None], allu[None], Kd[None], svd=pm.numpy_svd)
        ref_n = reprojection(rn["R"], rn["t"], w)[0]
        print("N %3d  four-point, %d hypotheses: median %.3e px (numpy EPnP %.3e)  max %.3e (%.3e)  within 0.01 px %.3f (%.3f)   n-point: %.3e px (%.3e)"
              % (N, good.sum(), np.median(lib), np.median(ref), lib.max(), ref.max(), (lib < 1e-2).mean(), (ref < 1e-2).mean(), lib_n, ref_n))
        assert np.median(lib) <= 10 * np.median(ref)
        assert lib.max() <= 10 * ref.max()
        assert (lib < 1e-2).mean() >= 0.5 * (ref < 1e-2).mean() > 0.1
        assert lib_n <= 10 * ref_n and ref_n < 1e-2
