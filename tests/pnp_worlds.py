"""Worlds for the PnPsolver tests: a camera pose, map points in front of it, their projections with a share of wrong correspondences and
pixel noise, every octave, and the RANSAC quadruples drawn up front (take-and-swap over the index list, as the solver draws them).
A world is the dict tests/pnp_model.py takes; problem() turns it into the library's PnPProblem."""
import math
import numpy as np
import pnp_model as pm

K = (458.654, 457.296, 367.215, 248.375)
LEVELS = 8
SIGMA2 = np.array([np.float32(1.2) ** (2 * l) for l in range(LEVELS)], np.float32)
TH2 = np.float32(5.991)
SIZES = (4, 5, 15, 63, 64, 65, 300, 2000, 8200)
BAD = (0.0, 0.3, 0.6)
NOISE = (0.0, 1.0)


def rotation(rv):
    rv = np.asarray(rv, np.float64)
    th = np.linalg.norm(rv)
    if th == 0:
        return np.eye(3)
    k = rv / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


def project(R, t, Xw, Kc=K):
    Xc = Xw @ R.T + t
    return np.stack([Kc[0] * Xc[:, 0] / Xc[:, 2] + Kc[2], Kc[1] * Xc[:, 1] / Xc[:, 2] + Kc[3]], 1)


def draw_quads(rng, N, H):
    """H quadruples of distinct positions: `randi = RandomInt(0, size-1); take; overwrite with the last; pop`."""
    quads = np.zeros((H, 4), np.int32)
    for h in range(H):
        avail = list(range(N))
        for i in range(4):
            r = int(rng.integers(0, len(avail)))
            quads[h, i] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return quads


def world(N, bad, noise, seed, H=300, decoy=False, min_inliers=None):
    """N correspondences, ceil(bad * N) of them wrong (uniform over the image, or -- decoy -- consistent with a second pose), Gaussian
    pixel noise on the others, octaves cycling through every level."""
    rng = np.random.default_rng(seed)
    R = rotation(rng.uniform(-0.3, 0.3, 3)); t = rng.uniform(-0.5, 0.5, 3)
    Xc = np.stack([rng.uniform(-2, 2, N), rng.uniform(-1.5, 1.5, N), rng.uniform(3, 9, N)], 1)
    Xw = (Xc - t) @ R                                             # R^T (Xc - t)
    Xw = Xw.astype(np.float32)
    uv = project(R, t, Xw.astype(np.float64))
    octave = np.arange(N) % LEVELS
    uv = uv + noise * rng.normal(size=(N, 2)) * np.sqrt(SIGMA2[octave].astype(np.float64))[:, None]
    nbad = int(math.ceil(bad * N))
    wrong = rng.permutation(N)[:nbad]
    if decoy:
        R2 = rotation(rng.uniform(-0.3, 0.3, 3)) @ R; t2 = t + rng.uniform(-0.5, 0.5, 3)
        uv[wrong] = project(R2, t2, Xw[wrong].astype(np.float64))
    else:
        uv[wrong] = np.stack([rng.uniform(0, 752, nbad), rng.uniform(0, 480, nbad)], 1)
    mi = pm.parameters(N)[1] if min_inliers is None else min_inliers
    return {"K": K, "p3dw": Xw, "p2d": uv.astype(np.float32), "max_err": (SIGMA2[octave] * TH2).astype(np.float32),
            "quads": draw_quads(rng, N, H) if N >= 4 else np.zeros((0, 4), np.int32), "min_inliers": mi, "best_start": 0,
            "R": R, "t": t, "wrong": wrong, "name": "N%d_bad%d_noise%d%s" % (N, int(bad * 100), int(noise), "_decoy" if decoy else "")}


def seeded_worlds():
    """The grid of the issue: 9 sizes x 3 shares of wrong correspondences x 2 noise levels, 300 hypotheses each."""
    out = []
    for N in SIZES:
        for bad in BAD:
            for noise in NOISE:
                out.append(world(N, bad, noise, seed=1000 + len(out)))
    return out


def decoy_worlds():
    """Worlds whose wrong correspondences agree with a second pose: the true set is exactly min_inliers strong (a record whose
    refinement cannot succeed), the decoy set is larger (a later record whose refinement does)."""
    return [world(64, 0.6, 0.0, seed=s, decoy=True) for s in (7, 11, 12, 13, 21, 23)]


def _exact(Xw, quads, min_inliers, name, Kc=K, R=None, t=None, max_err=None, p2d=None):
    Xw = np.asarray(Xw, np.float32)
    R = np.eye(3) if R is None else R
    t = np.zeros(3) if t is None else t
    with np.errstate(all="ignore"):
        uv = project(R, t, Xw.astype(np.float64), Kc) if p2d is None else np.asarray(p2d)
    uv = np.nan_to_num(uv, nan=0.0, posinf=1e6, neginf=-1e6)
    N = len(Xw)
    return {"K": Kc, "p3dw": Xw, "p2d": uv.astype(np.float32), "max_err": np.full(N, TH2, np.float32) if max_err is None else np.asarray(max_err, np.float32),
            "quads": np.asarray(quads, np.int32).reshape(-1, 4), "min_inliers": min_inliers, "best_start": 0, "name": name}


def hand_built():
    rng = np.random.default_rng(77)
    gen = lambda n: np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(3, 9, n)], 1)
    out = []
    base = gen(12)
    # four coplanar points (an axis-aligned plane: one singular value of PW0^T PW0 is exactly zero), then general ones
    P = base.copy(); P[:4, 2] = 5.0
    out.append(_exact(P, [[0, 1, 2, 3], [3, 2, 1, 0], [4, 5, 6, 7]], 4, "coplanar"))
    # four collinear points
    P = base.copy(); P[:4] = [[-1.5, 0.5, 4], [-0.5, 0.5, 4], [0.5, 0.5, 4], [1.5, 0.5, 4]]
    out.append(_exact(P, [[0, 1, 2, 3], [1, 3, 0, 2]], 4, "collinear"))
    # two coincident points of a quadruple; four coincident points
    P = base.copy(); P[1] = P[0]; P[2, 2] = P[0, 2]; P[3, 2] = P[0, 2]
    out.append(_exact(P, [[0, 1, 2, 3], [2, 0, 3, 1]], 4, "two_coincident"))
    P = base.copy(); P[1] = P[0]; P[2] = P[0]; P[3] = P[0]
    out.append(_exact(P, [[0, 1, 2, 3]], 4, "four_coincident"))
    # a correspondence at camera depth 0 (CheckInliers divides by it), not in a quadruple
    P = base.copy(); P[11] = [0.3, -0.2, 0.0]
    out.append(_exact(P, [[0, 1, 2, 3], [4, 5, 6, 7]], 4, "depth_zero"))
    # the first point of the quadruple lies behind the camera (solve_for_sign reads pcs[2] alone)
    P = base.copy(); P[0] = [0.4, 0.3, -3.0]
    out.append(_exact(P, [[0, 1, 2, 3], [1, 0, 2, 3]], 4, "behind_first"))
    # N below, at and one above min_inliers
    for n in (7, 8, 9):
        out.append(_exact(gen(n), draw_quads(rng, n, 6), 8, "N%d_min8" % n))
    return out


def many_records():
    """More than ORBM_PNP_MAX_RECORDS strict prefix maxima: 48 groups of four correspondences whose pixel noise falls from group to
    group -- hypothesis k draws group k, so its pose error falls with k -- and 120 exact probes whose thresholds are spread over sixteen
    decades, so that the count climbs with the pose's accuracy."""
    rng = np.random.default_rng(7)
    G, Pn = 48, 120
    Xw = np.stack([rng.uniform(-2, 2, 4 * G + Pn), rng.uniform(-1.5, 1.5, 4 * G + Pn), rng.uniform(3, 9, 4 * G + Pn)], 1).astype(np.float32)
    uv = project(np.eye(3), np.zeros(3), Xw.astype(np.float64))
    max_err = np.full(len(Xw), 1e-30, np.float32)
    for k in range(G):
        uv[4 * k:4 * k + 4] += rng.normal(size=(4, 2)) * 10.0 ** (1.5 - k / 6)
    max_err[4 * G:] = 10.0 ** np.linspace(-12, 4, Pn)
    quads = np.arange(4 * G).reshape(G, 4)
    return _exact(Xw, quads, 4, "many_records", max_err=max_err, p2d=uv)


def problem(m, w, best_start=None, quads=None):
    """The library's PnPProblem of a world."""
    return m.PnPProblem(w["K"], w["p3dw"], w["p2d"], w["max_err"], w["quads"] if quads is None else quads, w["min_inliers"],
                        w.get("best_start", 0) if best_start is None else best_start)
