"""Generated and hand-built worlds for the pose-optimisation tests: a rig with a known true pose, map points in front of its
cameras, their noisy observations, gross outliers, and a start pose some way off the truth.  A problem is a dict of the fields
tests/pose_model.py reads (and multi_orb_slam_amd.PoseProblem takes, see `to_problem`).

check_conditions(): what every world must satisfy, evaluated with the model in index order, so that the device and the two host
orders cannot legitimately disagree on a decision -- no edge's (float)chi2 within a relative GUARD of its threshold at any
classification, no trial decision with |rho| < RHO_GUARD -- and that the listed branches are reached across the set.  Seeds were
chosen on the CPU so that the conditions hold with no edge excluded; a world that fails gets another seed."""
import math
import numpy as np
import pose_model as pm

# The guard band around the classification thresholds.  It started at 1e-6; the two summation orders then turned out to differ by up to
# 5.2e-8 (relative to the threshold scale) in a classified chi2 -- an inlier keeps the error of the round's LAST trial, and where the two
# orders take a different number of rejected trials at convergence that pose differs in its ninth digit -- which is not 100 times
# below 1e-6, so the band was widened to 1e-5 and the seeds re-checked against it (profiles/r10/notes_pose.md).
GUARD = 1e-5
RHO_GUARD = 1e-9
N_LEVELS = 8
INV_SIGMA2 = (1.0 / (np.float32(1.2) ** np.arange(N_LEVELS, dtype=np.float32)) ** 2).astype(np.float32)
FX, FY, CX, CY, BF = 458.654, 457.296, 367.215, 248.375, 47.9
W, H = 752, 480


def rot(axis, angle):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def pose(R, t):
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


def generate(seed, n, kind="mixed", outliers=0.1, start=(0.05, 2.0), two_cams=False, noise=1.0, behind=0):
    """kind: "mono" | "stereo" | "mixed".  start = (metres, degrees) between the start pose and the truth.  two_cams: the second half
    of the features belongs to camera 2 of a rig with a non-trivial Rcam12 / tcam12.  behind: that many points get a camera depth <= 0."""
    rng = np.random.RandomState(seed)
    T_true = pose(rot(rng.randn(3), rng.uniform(0.1, 0.6)), rng.uniform(-2, 2, 3))
    R12 = rot([0.1, 1.0, 0.05], math.radians(35.0)).astype(np.float32)
    t12 = np.array([0.31, -0.02, 0.07], np.float32)
    T21 = pose(R12.astype(np.float64).T, -R12.astype(np.float64).T @ t12.astype(np.float64))
    n_cam0 = n - n // 2 if two_cams else n
    cam = (np.arange(n) >= n_cam0).astype(np.int64)
    octave = rng.randint(0, N_LEVELS, n)
    u = rng.uniform(20, W - 20, n)
    v = rng.uniform(20, H - 20, n)
    z = rng.uniform(1.5, 25.0, n)
    if behind:
        z[rng.choice(n, behind, replace=False)] = -rng.uniform(1.0, 5.0, behind)
    Xc = np.stack([(u - CX) / FX * z, (v - CY) / FY * z, z], axis=1)
    Twc = np.linalg.inv(T_true)
    T12 = np.linalg.inv(T21)
    Xw = np.empty((n, 3))
    for i in range(n):
        Xb = Xc[i] if cam[i] == 0 else T12[:3, :3] @ Xc[i] + T12[:3, 3]
        Xw[i] = Twc[:3, :3] @ Xb + Twc[:3, 3]
    sigma = noise * np.float64(np.float32(1.2)) ** octave
    uo = u + rng.randn(n) * sigma
    vo = v + rng.randn(n) * sigma
    ur = u - BF / z + rng.randn(n) * sigma
    stereo = {"mono": np.zeros(n, bool), "stereo": np.ones(n, bool), "mixed": rng.rand(n) < 0.5}[kind]
    stereo &= z > 0
    bad = rng.rand(n) < outliers
    ang = rng.uniform(0, 2 * math.pi, n)
    mag = rng.uniform(15, 120, n)
    uo = np.where(bad, uo + mag * np.cos(ang), uo)
    vo = np.where(bad, vo + mag * np.sin(ang), vo)
    obs = np.stack([uo, vo, np.where(stereo, np.maximum(ur, 0.0), -1.0)], axis=1).astype(np.float32)
    dT = pose(rot(rng.randn(3), math.radians(start[1])), rng.randn(3) / math.sqrt(3) * start[0])
    return {"Tcw": (dT @ T_true).astype(np.float32).reshape(16), "Tcw_true": T_true,
            "fx": FX, "fy": FY, "cx": CX, "cy": CY, "bf": BF, "inv_level_sigma2": INV_SIGMA2,
            "Rcam12": R12.reshape(9), "tcam12": t12, "n_cam0": n_cam0, "mode": pm.ALL_CAMS if two_cams else pm.CAM0,
            "feat": np.arange(n, dtype=np.int32), "pos": Xw.astype(np.float32), "obs": obs, "octave": octave.astype(np.int32)}


def with_mode(P, mode):
    """The problem the reference's other overload sees: PoseOptimization(Frame*) walks the features of camera 1 only."""
    Q = dict(P)
    Q["mode"] = mode
    if mode == pm.CAM0:
        keep = P["feat"] < P["n_cam0"]
        for k in ("feat", "pos", "obs", "octave"):
            Q[k] = P[k][keep]
    return Q


def take(P, idx):
    Q = dict(P)
    for k in ("pos", "obs", "octave"):
        Q[k] = P[k][idx]
    Q["feat"] = np.arange(len(idx), dtype=np.int32)
    Q["n_cam0"] = len(idx)
    return Q


# (name, generate() arguments).  Sizes 60 / 400 / 2 000 / 8 000; mono, stereo, mixed; two cameras; 10 % and 40 % outliers; starts from
# 1 cm / 0.5 deg to 30 cm / 10 deg.
GENERATED = [
    ("mono_60", dict(seed=1361, n=60, kind="mono", outliers=0.1, start=(0.01, 0.5))),
    ("stereo_60", dict(seed=12, n=60, kind="stereo", outliers=0.4, start=(0.05, 2.0))),
    ("mixed_400", dict(seed=23, n=400, kind="mixed", outliers=0.1, start=(0.1, 4.0))),
    ("mono_400_far", dict(seed=74, n=400, kind="mono", outliers=0.4, start=(0.3, 10.0))),
    ("stereo_2000", dict(seed=15, n=2000, kind="stereo", outliers=0.1, start=(0.3, 10.0))),
    ("mixed_2000", dict(seed=16, n=2000, kind="mixed", outliers=0.4, start=(0.05, 2.0), behind=2)),
    ("mixed_8000", dict(seed=17, n=8000, kind="mixed", outliers=0.1, start=(0.1, 4.0))),
    ("rig_400", dict(seed=118, n=400, kind="mixed", outliers=0.1, start=(0.05, 2.0), two_cams=True)),
    ("rig_2000", dict(seed=19, n=2000, kind="mixed", outliers=0.4, start=(0.3, 10.0), two_cams=True)),
    ("rig_8000_mono", dict(seed=120, n=8000, kind="mono", outliers=0.1, start=(0.01, 0.5), two_cams=True)),
]


def exact_world(n=12):
    """A start pose AT the optimum: the identity pose and points whose projections are exact in float, so that every error is 0, the
    step is 0, the trial pose is the estimate bit for bit and the first iteration ends on rho == 0."""
    fx = fy = 512.0
    cx, cy = 320.0, 240.0
    pos, obs = [], []
    for i in range(n):
        z = 4.0
        x, y = 0.5 * (i % 4) - 0.75, 0.25 * (i // 4) - 0.25
        pos.append([x, y, z])
        u = x / z * fx + cx
        obs.append([u, y / z * fy + cy, (u - 32.0 / z) if i % 2 else -1.0])
    return {"Tcw": np.eye(4, dtype=np.float32).reshape(16), "Tcw_true": np.eye(4), "fx": fx, "fy": fy, "cx": cx, "cy": cy, "bf": 32.0,
            "inv_level_sigma2": INV_SIGMA2, "Rcam12": np.eye(3, dtype=np.float32).reshape(9), "tcam12": np.zeros(3, np.float32),
            "n_cam0": n, "mode": pm.CAM0, "feat": np.arange(n, dtype=np.int32), "pos": np.array(pos, np.float32),
            "obs": np.array(obs, np.float32), "octave": np.zeros(n, np.int32)}


def hand_built():
    base = generate(seed=31, n=40, kind="mixed", outliers=0.0, start=(0.02, 1.0))
    out = [("two", take(base, np.arange(2))),                       # returns 0, the pose untouched
           ("nine", take(base, np.arange(9))),                      # one round only
           ("exact", exact_world())]                                # rho == 0
    # every edge an outlier after round 0: observations that have nothing to do with the points
    rng = np.random.RandomState(32)
    junk = take(base, np.arange(14))
    junk["obs"] = np.stack([rng.uniform(0, W, 14), rng.uniform(0, H, 14), -np.ones(14)], axis=1).astype(np.float32)
    out.append(("all_outliers", junk))
    # a point with camera depth <= 0 among good ones
    out.append(("behind", generate(seed=35, n=30, kind="mixed", outliers=0.1, start=(0.02, 1.0), behind=3)))
    # a world in which trials are rejected: far start, many outliers, few points
    out.append(("rejected", generate(seed=352, n=24, kind="mono", outliers=0.4, start=(0.6, 25.0))))
    return out


_cache = {}


def worlds():
    """[(name, problem)]: every generated world in both camera modes, then the hand-built cases."""
    if "w" not in _cache:
        out = []
        for name, kw in GENERATED:
            P = generate(**kw)
            out.append((name + "/cam0", with_mode(P, pm.CAM0)))
            out.append((name + "/all", with_mode(P, pm.ALL_CAMS)))
        for name, P in hand_built():
            out.append((name + "/cam0", with_mode(P, pm.CAM0)))
            out.append((name + "/all", with_mode(P, pm.ALL_CAMS)))
        _cache["w"] = out
    return _cache["w"]


REQUIRED_BRANCHES = ("fewer_than_3", "fewer_than_10", "nothing_active", "rho_zero", "rejected_trial", "depth_not_positive")


def evaluate(order="index"):
    """{name: (record, flags, trace)} of the model over all worlds (cached per order)."""
    key = "eval_" + order
    if key not in _cache:
        out = {}
        for name, P in worlds():
            tr = pm.Trace()
            rec, flags = pm.optimize(P, order, tr)
            out[name] = (rec, flags, tr)
        _cache[key] = out
    return _cache[key]


def check_conditions(verbose=False):
    reached = set()
    worst_margin, worst_rho = math.inf, math.inf
    for name, (rec, flags, tr) in evaluate("index").items():
        margin = min([float(np.nanmin(m)) for m in tr.margins if len(m)] or [math.inf])
        rho = min([abs(r) for r in tr.rhos if r != 0] or [math.inf])    # (rho == 0 exactly is the termination test, not a sign decision)
        if verbose:
            print("%-22s n=%5d rounds=%d inliers=%5d  min margin %.3e  min |rho| %.3e  %s" % (
                name, rec["n_initial"], rec["rounds"], rec["n_inliers"], margin, rho, sorted(tr.branches)))
        assert margin > GUARD, (name, margin)
        assert rho > RHO_GUARD, (name, rho)
        worst_margin, worst_rho = min(worst_margin, margin), min(worst_rho, rho)
        reached |= tr.branches
    for b in REQUIRED_BRANCHES:
        assert b in reached, b
    return worst_margin, worst_rho, reached


def to_problem(m, P):
    """multi_orb_slam_amd.PoseProblem of a world."""
    return m.PoseProblem(P["Tcw"], P["fx"], P["fy"], P["cx"], P["cy"], P["bf"], P["inv_level_sigma2"], P["feat"], P["pos"], P["obs"],
                         P["octave"], mode=P["mode"], n_cam0=P["n_cam0"], Rcam12=P["Rcam12"], tcam12=P["tcam12"])
