"""Worlds for the Sim3Solver tests: two keyframes looking at a shared cloud with a known Sim3 between them, as the vectors the
constructor leaves (mvX3Dc1, mvX3Dc2, camIdx1/2, mvnMaxError1/2) plus 300 drawn triples.  Every world satisfies a GUARD BAND: under the
model in libm order no err1 / err2 of any (hypothesis, correspondence) pair lies within the relative distance GUARD of its threshold, so
that the inlier masks of the two orders are equal because of the inputs, not by luck.  The generator nudges the points of offending
pairs (never a test does); check_conditions() verifies the band and is itself a test."""
import math

import numpy as np

import sim3_model as sm

F = np.float32
N_LEVELS = 8
SCALE_FACTOR = 1.2
# GUARD = SIM3_MARGIN (4, the pose stage's margin) x the largest relative difference of any err between the two orders.  MEASURED over
# these worlds that difference is 0: the orders differ by a few ulp of a double inside atan2 / sin / cos, and no element of R, t or s
# straddled a float rounding boundary (tests/test_sim3_model.py, profiles/r11/notes_sim3.md).  A band of 4 x 0 would guard nothing, so
# the figure is the bound of the smallest difference that CAN occur, one float ulp in one element of sR: it moves a projection by at most
# fx * 2^-23 * |X_k| / z <= 520 * 1.2e-7 * 1 = 6.2e-5 pixels, and an err at its threshold (d >= sqrt(9) = 3 pixels) by 2 * 6.2e-5 / 3 =
# 4.2e-5 of itself; times the margin 1.7e-4, rounded up.
GUARD = 2e-4
K1 = (520.0, 522.0, 318.5, 241.0)
K2 = (515.0, 517.0, 322.0, 238.5)
_NUDGED = {}


def rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * Kx + (1 - math.cos(angle)) * (Kx @ Kx)


def level_sigma2():
    """mvLevelSigma2 as ORBextractor builds it: float scale factors by repeated multiplication, squared in float."""
    s = [F(1)]
    for _ in range(1, N_LEVELS):
        s.append(s[-1] * F(SCALE_FACTOR))
    return [v * v for v in s]


def max_errors(octaves):
    """mvnMaxError: 9.210 * sigmaSquare in double, through the reference's std::vector<size_t>, read by a float comparison."""
    sig = level_sigma2()
    return np.array([F(int(9.210 * float(sig[o]))) for o in octaves], F)


def randi_stream(seed):
    rng = np.random.RandomState(seed)
    return lambda n: int(rng.randint(0, n))


def generate(seed, n, s=1.0, fix_scale=False, cams=(0.0, 0.0), wrong=0.0, noise=0.0, rig="small", H=300):
    """cams: share of correspondences whose feature lies in the second camera, per keyframe; rig: the second camera's extrinsics
    ("small": a few milliradians and millimetres, so that second-camera points pass or fail by a little; "wide": a real rig)."""
    rng = np.random.RandomState(seed)
    z = rng.uniform(2.0, 9.0, n)
    X1 = np.stack([rng.uniform(-0.55, 0.55, n) * z, rng.uniform(-0.4, 0.4, n) * z, z], axis=1)
    R = rot(rng.randn(3), rng.uniform(0.05, 0.6))
    t = rng.uniform(-0.5, 0.5, 3)
    X2 = ((X1 - t) @ R) / s                               # X1 = s R X2 + t
    if noise > 0:
        X1 = X1 + rng.randn(n, 3) * (noise * X1[:, 2:3] / K1[0]) * [1, 1, 0.3]
        X2 = X2 + rng.randn(n, 3) * (noise * np.abs(X2[:, 2:3]) / K2[0]) * [1, 1, 0.3]
    bad = rng.rand(n) < wrong
    X2[bad] = X2[rng.permutation(n)][bad] + rng.randn(int(bad.sum()), 3) * 0.3
    octave = rng.randint(0, N_LEVELS, (2, n))
    octave[:, :N_LEVELS] = np.arange(N_LEVELS) if n >= N_LEVELS else octave[:, :N_LEVELS]
    cam1 = (rng.rand(n) < cams[0]).astype(np.int32); cam2 = (rng.rand(n) < cams[1]).astype(np.int32)
    if rig == "small":
        Rc12, tc12 = rot([0.2, 1.0, 0.1], 0.0015), np.array([0.004, 0.0, 0.001])
    else:
        Rc12, tc12 = rot([0.05, 1.0, 0.02], 0.5), np.array([0.3, 0.0, 0.05])
    calib = np.concatenate([Rc12, tc12.reshape(1, 3)]).astype(F)
    R21 = np.ascontiguousarray(calib[:3, :3].T)
    tt = R21[:, 0] * calib[3, 0] + R21[:, 1] * calib[3, 1]
    tt = tt + R21[:, 2] * calib[3, 2]
    t21 = (tt.astype(np.float64) * -1.0 + 0.0 * 0.0).astype(F)
    W = dict(K1=K1, K2=K2, calib=calib, Rcam21=R21.reshape(9), tcam21=t21, fix_scale=bool(fix_scale), x3dc1=X1.astype(F), x3dc2=X2.astype(F),
             cam1=cam1, cam2=cam2, octave=octave, max_err1=max_errors(octave[0]), max_err2=max_errors(octave[1]),
             triples=sm.draw_triples(n, H, randi_stream(seed + 1000)), R_true=R, t_true=t, s_true=float(s), seed=seed)
    return W


def in_band(W, e1, e2, guard=None):
    """(hypothesis, correspondence) pairs with an err within the relative distance GUARD of its threshold -> bool (H, N)."""
    g = GUARD if guard is None else guard
    t1 = W["max_err1"].astype(np.float64).reshape(1, -1); t2 = W["max_err2"].astype(np.float64).reshape(1, -1)
    with np.errstate(all="ignore"):
        return (np.abs(e1.astype(np.float64) - t1) <= g * t1) | (np.abs(e2.astype(np.float64) - t2) <= g * t2)


def nudge(name, W):
    """Moves the points of offending pairs a little (a seeded fraction of a millimetre in keyframe 2's frame) until no pair is in the
    band; counts the pairs that had to be moved."""
    rng = np.random.RandomState(W["seed"] + 77)
    moved = 0
    for _ in range(20):
        _, _, e1, e2 = sm.evaluate(W, "libm")
        off = in_band(W, e1, e2)
        if not off.any():
            _NUDGED[name] = moved
            return W
        cols = np.nonzero(off.any(axis=0))[0]
        moved += int(off.sum())
        x = W["x3dc2"].copy()
        x[cols] = (x[cols].astype(np.float64) + rng.uniform(-1, 1, (len(cols), 3)) * 2e-3 * np.abs(x[cols, 2:3])).astype(F)
        W = dict(W, x3dc2=x)
    raise AssertionError("world %s: pairs are still inside the guard band after 20 rounds" % name)


GENERATED = [
    # name, seed, n, s, fix_scale, cams, wrong, noise, rig
    ("n15_free_1.0", 1, 15, 1.0, False, (0.0, 0.0), 0.0, 0.0, "small"),
    ("n20_fixed", 2, 20, 1.0, True, (0.0, 0.0), 0.0, 1.0, "small"),
    ("n40_free_0.7_wrong30", 3, 40, 0.7, False, (0.3, 0.0), 0.3, 1.0, "small"),
    ("n64_free_1.4", 4, 64, 1.4, False, (0.0, 0.3), 0.0, 1.0, "small"),
    ("n65_fixed_wrong60", 5, 65, 1.0, True, (0.3, 0.3), 0.6, 1.0, "small"),
    ("n100_free_1.0_wrong30", 6, 100, 1.0, False, (0.0, 0.0), 0.3, 0.0, "small"),
    ("n128_free_0.7_both", 7, 128, 0.7, False, (0.5, 0.5), 0.0, 1.0, "small"),
    ("n300_fixed_wide", 8, 300, 1.0, True, (0.4, 0.4), 0.3, 1.0, "wide"),
    ("n500_free_1.4_wrong60", 9, 500, 1.4, False, (0.2, 0.0), 0.6, 1.0, "small"),
    ("n1000_free_1.0_wrong30", 10, 1000, 1.0, False, (0.0, 0.2), 0.3, 1.0, "small"),
    ("n2000_fixed_wrong30", 11, 2000, 1.0, True, (0.3, 0.3), 0.3, 1.0, "small"),
    ("n2000_free_0.7_clean", 12, 2000, 0.7, False, (0.0, 0.0), 0.0, 0.0, "small"),
    ("n8200_free_1.4_over_the_cap", 13, sm.CAP + 8, 1.4, False, (0.2, 0.2), 0.3, 1.0, "small"),
]


def flat(n, seed, points1, points2, triples, **kw):
    """A hand-built world: the given points, every octave 0, identity second camera unless given."""
    W = generate(seed, n, **kw)
    W.update(x3dc1=np.asarray(points1, F), x3dc2=np.asarray(points2, F), triples=np.asarray(triples, np.int32).reshape(-1, 3))
    return W


def hand_built():
    out = []
    base = generate(21, 30, s=1.0, noise=0.0)
    X1, X2 = base["x3dc1"].copy(), base["x3dc2"].copy()
    # three coincident points (0, 1, 2 in both frames: the float centroid is not exactly the point, what is left is rounding noise below
    # the Jacobi sweep's absolute stop), three coincident points whose centroid IS exact (14, 15, 16: M = 0, the quaternion (1, 0, 0, 0),
    # norm(vec) = 0, `2*ang*vec/norm(vec)` = 0 * inf), three collinear points (3, 4, 5), a triple that repeats across iterations
    X1[1] = X1[0]; X1[2] = X1[0]; X2[1] = X2[0]; X2[2] = X2[0]
    X1[14:17] = np.array([1.5, -0.75, 3.0], F); X2[14:17] = np.array([0.5, 0.25, 4.0], F)
    X1[4] = X1[3] + F(0.5) * (X1[5] - X1[3]); X2[4] = X2[3] + F(0.5) * (X2[5] - X2[3])
    tri = [[0, 1, 2], [3, 4, 5], [6, 7, 8], [6, 7, 8], [9, 10, 11], [8, 6, 7], [6, 7, 8], [14, 15, 16]] + sm.draw_triples(30, 12, randi_stream(5)).tolist()
    out.append(("degenerate_and_repeated", flat(30, 21, X1, X2, tri)))
    # a rotation of exactly 0: both frames hold the same points up to a translation of exactly representable numbers -> the quaternion
    # is (1, 0, 0, 0), norm(vec) = 0 and `2*ang*vec/norm(vec)` is 0 * inf: the reference's own NaN
    Y1 = np.round(base["x3dc1"] * 64) / 64
    out.append(("rotation_zero", flat(30, 22, Y1, Y1 + F(0.25), sm.draw_triples(30, 20, randi_stream(6)), fix_scale=True)))
    # a rotation of pi about the z axis: X1 = diag(-1, -1, 1) X2 + t, with t keeping both clouds in front of their cameras
    Z2 = Y1.copy()
    Z1 = Z2 * np.array([-1, -1, 1], F) + np.array([0.5, 0.25, 0], F)
    out.append(("rotation_pi", flat(30, 23, Z1, Z2, sm.draw_triples(30, 20, randi_stream(7)))))
    # a rotation of 1e-4 rad.  (Rodrigues' own small-angle branch, theta < DBL_EPSILON, cannot be reached from ComputeSim3: the Jacobi
    # sweep stops at pivots of FLT_EPSILON, so a non-zero imaginary part of the quaternion is never that small, and a zero one gives
    # the NaN above before Rodrigues is called; profiles/r11/notes_sim3.md.)
    T2 = Y1.copy()
    T1 = (T2.astype(np.float64) @ rot([0.3, 0.2, 1.0], 1e-4).T + [0.1, 0.0, 0.05]).astype(F)
    out.append(("rotation_small", flat(30, 24, T1, T2, sm.draw_triples(30, 20, randi_stream(8)), fix_scale=True)))
    # a point with z = 0 after the transform: correspondence 12 of keyframe 2 is sent to keyframe 1's image plane
    V = generate(25, 30, s=1.0, noise=0.0)
    V2 = V["x3dc2"].copy()
    target = np.array([0.3, -0.2, 0.0])
    V2[12] = ((target - V["t_true"]) @ V["R_true"]).astype(F)
    V1 = V["x3dc1"].copy(); V1[13] = np.array([0.4, 0.1, 0.0], F)
    out.append(("depth_zero", flat(30, 25, V1, V2, sm.draw_triples(30, 20, randi_stream(9)))))
    # fewer correspondences than min_inliers (20), and exactly as many
    out.append(("n12_below_min", generate(26, 12, s=1.0, noise=0.0, H=20)))
    out.append(("n20_equal_min", generate(27, 20, s=1.0, noise=0.0, H=20)))
    return out


_WORLDS = None


def worlds():
    global _WORLDS
    if _WORLDS is None:
        ws = [(name, generate(seed, n, s=s, fix_scale=fs, cams=cams, wrong=wrong, noise=noise, rig=rig))
              for name, seed, n, s, fs, cams, wrong, noise, rig in GENERATED] + hand_built()
        _WORLDS = [(name, nudge(name, W)) for name, W in ws]
    return _WORLDS


def nudged():
    worlds()
    return dict(_NUDGED)


_EVAL = {}


def evaluate(order="libm"):
    """{name: (records, mask words, err1, err2)} of every world under the model, cached per order."""
    if order not in _EVAL:
        _EVAL[order] = {name: sm.evaluate(W, order) for name, W in worlds()}
    return _EVAL[order]


def check_conditions():
    """The guard band over every pair of every world (libm order) -> (pairs checked, smallest relative distance to a threshold)."""
    pairs, closest = 0, math.inf
    for name, W in worlds():
        _, _, e1, e2 = evaluate("libm")[name]
        assert not in_band(W, e1, e2).any(), name
        pairs += e1.size
        with np.errstate(all="ignore"):
            for e, t in ((e1, W["max_err1"]), (e2, W["max_err2"])):
                d = np.abs(e.astype(np.float64) - t.astype(np.float64).reshape(1, -1)) / t.astype(np.float64).reshape(1, -1)
                d = d[np.isfinite(d)]
                if d.size:
                    closest = min(closest, float(d.min()))
    return pairs, closest


def to_problem(m, W, triples=None):
    return m.Sim3Problem(W["K1"], W["K2"], W["x3dc1"], W["x3dc2"], W["cam1"], W["cam2"], W["max_err1"], W["max_err2"],
                         W["triples"] if triples is None else triples, fix_scale=W["fix_scale"], calib=W["calib"])
