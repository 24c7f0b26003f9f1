"""Worlds for the Sim3 refinement tests (Optimizer::OptimizeSim3_cam1): two keyframes looking at a shared cloud with a known Sim3 S12
between them (X1 = s R X2 + t), as the arrays orbm_sim3_optimize takes: camera-frame float points of both keyframes, both undistorted
observations, both octaves, a start for g2oS12 graded from exact to well off, th2 = 10 as LoopClosing passes it.

Every world satisfies a GUARD BAND: under the model, in both orders, no chi2 of any correspondence at either chi-square test lies
within the relative distance GUARD of th2, so that the flags and return values of the two orders are equal because of the inputs, not
by luck.  tests/test_sim3opt_model.py checks the band on the CPU; a world that broke it would be replaced here, never nudged by a test.

GUARD: the two orders differ by the summation order of H, b and chi2 (a few ulp of a double each), by at most 2 ulp in sin / cos and 1
ulp in exp.  A Levenberg step x solves (H + lambda I) x = b, so a relative perturbation eps of H and b moves x by about cond(H) * eps *
|x|; with central differences at 1e-9 the Jacobian itself carries a relative error near 1e-7, which bounds how well conditioned the
system can be taken to be, and the estimate of either order is only defined to about 1e-7 of a pixel through it.  Taking that figure
-- 1e-7 pixel in a projection -- a chi2 at th2 = 10 (an error of sqrt(10 / w) >= 3.1 pixels at w <= 1) moves by 2 * 1e-7 / 3.1 =
6.5e-8 of itself; times the margin 4 of the sibling worlds, rounded up."""
import math

import numpy as np

F = np.float32
N_LEVELS = 8
SCALE_FACTOR = 1.2
GUARD = 3e-7
TH2 = 10.0
K1 = (520.0, 522.0, 318.5, 241.0)
K2 = (515.0, 517.0, 322.0, 238.5)
# start grades: rotation off by (radians), translation off by (units of the scene), log-scale off by
GRADES = {0: (0.0, 0.0, 0.0), 1: (0.004, 0.01, 0.01), 2: (0.03, 0.05, 0.05), 3: (0.1, 0.2, 0.15)}


def rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * Kx + (1 - math.cos(angle)) * (Kx @ Kx)


def inv_level_sigma2():
    """mvInvLevelSigma2 as ORBextractor builds it: float scale factors by repeated multiplication, squared, 1.0f / that."""
    s = [F(1)]
    for _ in range(1, N_LEVELS):
        s.append(s[-1] * F(SCALE_FACTOR))
    return np.array([F(1) / (v * v) for v in s], F)


def project(K, X):
    return np.stack([K[0] * X[:, 0] / X[:, 2] + K[2], K[1] * X[:, 1] / X[:, 2] + K[3]], axis=1)


def generate(seed, n, s=1.0, fix_scale=False, wrong=0.0, noise=0.0, grade=1, n_wrong=None, start_scale_only=False):
    """wrong: share of correspondences whose observation in keyframe 1 belongs to another point (n_wrong: that many exactly, the LAST
    ones); noise: pixels (sigma) on both observations; grade: how far the start is from the truth (GRADES)."""
    rng = np.random.RandomState(seed)
    z = rng.uniform(2.0, 9.0, n)
    X1 = np.stack([rng.uniform(-0.55, 0.55, n) * z, rng.uniform(-0.4, 0.4, n) * z, z], axis=1)
    R = rot(rng.randn(3), rng.uniform(0.05, 0.4))
    t = rng.uniform(-0.4, 0.4, 3)
    if fix_scale:
        s = 1.0
    X2 = ((X1 - t) @ R) / s                               # X1 = s R X2 + t
    X1 = X1.astype(F); X2 = X2.astype(F)
    obs1 = project(K1, X1.astype(np.float64)); obs2 = project(K2, X2.astype(np.float64))
    if noise > 0:
        obs1 = obs1 + rng.randn(n, 2) * noise; obs2 = obs2 + rng.randn(n, 2) * noise
    bad = rng.rand(n) < wrong
    if n_wrong is not None:
        bad = np.arange(n) >= n - n_wrong
    shift = rng.uniform(25.0, 120.0, (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))
    obs1[bad] = obs1[bad] + shift[bad]
    octave = rng.randint(0, N_LEVELS, (2, n))
    if n >= N_LEVELS:
        octave[0, :N_LEVELS] = np.arange(N_LEVELS); octave[1, :N_LEVELS] = np.arange(N_LEVELS)[::-1]
    da, dt, ds = GRADES[grade]
    if start_scale_only:
        da, dt = 0.0, 0.0
    R0 = rot(rng.randn(3), da) @ R if da else R
    t0 = t + rng.randn(3) / math.sqrt(3) * dt
    s0 = s if fix_scale else s * math.exp(ds)
    sig = inv_level_sigma2()
    return dict(K1=K1, K2=K2, inv_level_sigma2_1=sig, inv_level_sigma2_2=sig, R=R0.astype(F).reshape(9), t=t0.astype(F), s=F(s0), th2=F(TH2),
                fix_scale=bool(fix_scale), x3dc1=X1, x3dc2=X2, obs1=obs1.astype(F), obs2=obs2.astype(F), octave1=octave[0].astype(np.int32),
                octave2=octave[1].astype(np.int32), truth=(R, t, s), n=n, seed=seed)


# name: (seed, n, keyword arguments).  15 to 8 200 correspondences; scale fixed, and free at 0.7 / 1.0 / 1.4; 0 / 20 / 50 % wrong; 0 and
# 1 pixel of noise; all octaves; starts from exact to well off.
WORLDS = {
    "n15_fixed_clean_exact": (1, 15, dict(fix_scale=True, grade=0)),
    "n15_free10_noise_near": (2, 15, dict(s=1.0, noise=1.0, grade=1)),
    "n24_free07_wrong20": (3, 24, dict(s=0.7, wrong=0.2, grade=1)),
    "n40_fixed_wrong20_noise": (4, 40, dict(fix_scale=True, wrong=0.2, noise=1.0, grade=2)),
    "n40_free14_clean_off": (5, 40, dict(s=1.4, grade=3)),
    "n64_free10_wrong50_noise": (6, 64, dict(s=1.0, wrong=0.5, noise=1.0, grade=1)),
    "n65_fixed_clean_near": (7, 65, dict(fix_scale=True, grade=1)),
    "n100_free07_noise_mid": (8, 100, dict(s=0.7, noise=1.0, grade=2)),
    "n100_fixed_wrong50": (9, 100, dict(fix_scale=True, wrong=0.5, grade=1)),
    "n150_free14_wrong20_noise_off": (10, 150, dict(s=1.4, wrong=0.2, noise=1.0, grade=3)),
    "n255_free10_clean_exact": (11, 255, dict(s=1.0, grade=0)),
    "n256_fixed_noise_mid": (12, 256, dict(fix_scale=True, noise=1.0, grade=2)),
    "n257_free07_wrong20_noise": (13, 257, dict(s=0.7, wrong=0.2, noise=1.0, grade=2)),
    "n300_free10_scale_only": (14, 300, dict(s=1.0, grade=3, start_scale_only=True)),
    "n400_free14_wrong50_noise": (15, 400, dict(s=1.4, wrong=0.5, noise=1.0, grade=1)),
    "n600_fixed_wrong20_noise_off": (16, 600, dict(fix_scale=True, wrong=0.2, noise=1.0, grade=3)),
    "n1000_free10_noise_near": (17, 1000, dict(s=1.0, noise=1.0, grade=1)),
    "n2000_free07_wrong20_noise": (18, 2000, dict(s=0.7, wrong=0.2, noise=1.0, grade=2)),
    "n8192_fixed_noise": (19, 8192, dict(fix_scale=True, noise=1.0, grade=1)),
    "n8200_free14_wrong20_noise": (20, 8200, dict(s=1.4, wrong=0.2, noise=1.0, grade=2)),
}
_CACHE = {}


def world(name):
    if name not in _CACHE:
        seed, n, kw = WORLDS[name]
        _CACHE[name] = generate(seed, n, **kw)
    return _CACHE[name]


# ---- hand-built cases: one per exit ---------------------------------------------------------------------------------------------------
def exit_cases():
    """name -> (world, what the test expects of it)"""
    cases = {
        "zero": (generate(31, 0), dict(n_inliers=0, written=0, n_bad=0, n_more_iterations=5, optimisations=0)),
        "survivors_9": (generate(32, 14, s=1.1, n_wrong=5, grade=2), dict(n_inliers=0, written=0, n_bad=5, n_more_iterations=10, optimisations=1)),
        "survivors_10": (generate(32, 14, s=1.1, n_wrong=4, grade=2), dict(written=1, n_bad=4, n_more_iterations=10, optimisations=2)),
        "survivors_11": (generate(32, 14, s=1.1, n_wrong=3, grade=2), dict(written=1, n_bad=3, n_more_iterations=10, optimisations=2)),
        "none_bad": (generate(33, 30, s=0.9, grade=1), dict(n_inliers=30, written=1, n_bad=0, n_more_iterations=5, optimisations=2)),
        "some_bad": (generate(34, 30, s=0.9, n_wrong=6, grade=1), dict(n_inliers=24, written=1, n_bad=6, n_more_iterations=10, optimisations=2)),
        "nine_clean": (generate(35, 9, grade=1), dict(n_inliers=0, written=0, n_bad=0, n_more_iterations=5, optimisations=1)),
        "all_removed": (generate(36, 20, n_wrong=20, grade=0), dict(n_inliers=0, written=0, n_bad=20, n_more_iterations=10, optimisations=1)),
        "branches_free": (generate(37, 50, s=1.2, grade=3), dict(written=1)),
        "branches_fixed": (generate(38, 50, fix_scale=True, grade=3), dict(written=1)),
        "branches_scale_only": (generate(39, 50, s=1.2, grade=3, start_scale_only=True), dict(written=1)),
    }
    return cases


def as_f32(x):
    return np.asarray(x, F)


def next_f32(x, up):
    return np.nextafter(F(x), F(np.inf) if up else F(-np.inf))


def boundary_pair(run_flags, edge, position, n=70, seed=41):
    """A clean, exactly started world of n correspondences in which the x observation of correspondence `position` in keyframe 1
    (edge "12": EdgeSim3ProjectXYZ) or keyframe 2 (edge "21": EdgeInverseSim3ProjectXYZ) is bisected over the float32 numbers until two
    NEIGHBOURING floats give a different flag for that correspondence at the first chi-square test.  run_flags(world) -> flags.
    -> (world_kept, world_removed)"""
    base = generate(seed, n, s=1.0, grade=0)
    key = "obs1" if edge == "12" else "obs2"
    w = 1.0 / float(base["inv_level_sigma2_1"][(base["octave1"] if edge == "12" else base["octave2"])[position]])

    def variant(v):
        W = dict(base)
        o = base[key].copy()
        o[position, 0] = v
        W[key] = o
        return W

    lo = F(base[key][position, 0])                                   # on the projection: chi2 = 0
    sign = F(-1.0) if lo < 0 else F(1.0)                             # away from zero: the order of the magnitudes is that of their bits
    hi = F(lo + sign * F(3.0 * math.sqrt(TH2 * w)))                  # three thresholds away
    assert run_flags(variant(lo))[position] == 0 and run_flags(variant(hi))[position] == 1
    value = lambda bits: sign * np.asarray(bits, np.int32).view(F)
    a, b = int(np.asarray(abs(lo), F).view(np.int32)), int(np.asarray(abs(hi), F).view(np.int32))
    assert 0 <= a < b
    while b - a > 1:
        mid = (a + b) // 2
        if run_flags(variant(value(mid)))[position] == 0:
            a = mid
        else:
            b = mid
    return variant(value(a)), variant(value(b))


# ---- the library's side -----------------------------------------------------------------------------------------------------------------
def to_problem(m, W):
    return m.Sim3OptProblem(W["K1"], W["K2"], W["inv_level_sigma2_1"], W["inv_level_sigma2_2"], W["R"], W["t"], W["s"], W["th2"],
                            W["fix_scale"], W["x3dc1"], W["x3dc2"], W["obs1"], W["obs2"], W["octave1"], W["octave2"])


def sized(n, seed=60, fix_scale=None):
    """A world of exactly n correspondences for the tests of counts: a fifth wrong, a pixel of noise, a start a little off."""
    fixed = (n % 2 == 1) if fix_scale is None else fix_scale
    return generate(seed + n % 89, n, s=1.25, fix_scale=fixed, wrong=0.2, noise=1.0, grade=2)


_PAIRS = {}


def host_boundary_pair(m, edge, position, order):
    """boundary_pair through the library's host routine in the given order (cached per process)."""
    key = (edge, position, order)
    if key not in _PAIRS:
        run = lambda W: m.sim3_optimize_host([to_problem(m, W)], order)[0][1]
        _PAIRS[key] = boundary_pair(run, edge, position)
    return _PAIRS[key]


def candidates(seed, n, k, fix_scale=False):
    """k candidates of one loop: keyframe 1 (its points, observations and octaves) is shared bit for bit, every candidate has a keyframe 2 of its own
    (another Sim3, another share of wrong correspondences, another start)."""
    base = generate(seed, n, s=1.0, fix_scale=fix_scale, noise=0.5, grade=1)
    X1 = base["x3dc1"].astype(np.float64)
    out = []
    for b in range(k):
        rng = np.random.RandomState(seed + 7 * b + 1)
        W = dict(generate(seed + 100 * (b + 1), n, s=(0.8, 1.0, 1.3)[b % 3], fix_scale=fix_scale, grade=1 + b % 3))   # (its truth and its start)
        R, t, s = W["truth"]
        W["x3dc1"], W["octave1"] = base["x3dc1"], base["octave1"]
        W["x3dc2"] = (((X1 - t) @ R) / s).astype(F)
        wrong = rng.rand(n) < (0.0, 0.2, 0.5)[b % 3]
        shift = rng.uniform(25.0, 120.0, (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))
        W["obs1"] = base["obs1"]                            # (keyframe 1 is ONE keyframe: a wrong correspondence is wrong in keyframe 2)
        obs2 = project(K2, W["x3dc2"].astype(np.float64)) + rng.randn(n, 2) * 0.5
        W["obs2"] = np.where(wrong[:, None], obs2 + shift, obs2).astype(F)
        out.append(W)
    return out
