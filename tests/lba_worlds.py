"""Seeded, geometry-consistent worlds for the local bundle adjustment (tests/test_lba_model.py, tests/test_gpu_lba.py): keyframes on a
path, points in front of them seen by 1 to all of the keyframes through either camera of the rig, mono / stereo / mixed observations,
0 / 10 / 40 % of them wrong by tens of pixels, starts from exact to 5 cm / 2 degrees off.  A world is the dict the model reads
(tests/lba_model.py) and to_problem() hands to the library; `truth` holds what the observations were made from.

check_band() asserts the guard band around 5.991 / 7.815 and around depth 0 at both tests of a model run, so that the two orders of the
host routine (and the device) agreeing on every flag is a property of the inputs, not luck."""
import math
import numpy as np

FX, FY, CX, CY, BF = 500.0, 505.0, 320.0, 240.0, 40.0
BAND = 1e-7            # relative distance every tested chi2 keeps from its threshold, absolute distance every depth keeps from 0


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]); Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


TCAM12 = (0.12, 0.0, 0.01)   # mtcam12 of the rig


def tcim_pair(yaw_deg=8.0, t=TCAM12):
    """Tcam11 and Tcam21 as the reference builds them from mRcam12 / mtcam12 (Optimizer.cc:1048-1061), in float."""
    R12 = rot(0.0, math.radians(yaw_deg), 0.0).astype(np.float32)
    t12 = np.asarray(t, np.float32).reshape(3, 1)
    T21 = np.zeros((4, 4), np.float32)
    R21 = R12.T.copy()
    T21[:3, :3] = R21
    T21[:3, 3:] = -(R21 @ t12)
    T21[3, 3] = 1.0
    return np.stack([np.eye(4, dtype=np.float32), T21])


def make_world(n_free, n_fixed, n_points, seed, form="mixed", wrong=0.1, start="off", max_obs=6, noise=True, two_cams=True):
    rng = np.random.RandomState(seed)
    n_poses = n_free + n_fixed
    Tcim = tcim_pair()
    Tcw = np.zeros((n_poses, 4, 4))
    span = 0.4 * max(n_poses - 1, 1)
    order = rng.permutation(n_poses) if n_poses > 2 else np.arange(n_poses)   # free and fixed keyframes are interleaved along the path
    for slot, p in enumerate(order):
        c = np.array([0.4 * slot, rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)])
        Rwc = rot(rng.uniform(-0.03, 0.03), rng.uniform(-0.09, 0.09), rng.uniform(-0.03, 0.03))
        Tcw[p, :3, :3] = Rwc.T; Tcw[p, :3, 3] = -Rwc.T @ c; Tcw[p, 3, 3] = 1.0
    pts = np.stack([rng.uniform(-2.0, span + 2.0, n_points), rng.uniform(-1.5, 1.5, n_points), rng.uniform(4.0, 10.0, n_points)], axis=1)
    Tcw32 = Tcw.astype(np.float32); pts32 = pts.astype(np.float32)
    first, edge_pose, edge_cam, obs, w = [0], [], [], [], []
    n_wrong = 0
    for l in range(n_points):
        k = int(rng.randint(1, min(n_poses, max_obs) + 1))
        seen = rng.permutation(n_poses)[:k]                       # the caller's order inside a point: any
        for p in seen:
            cam = int(rng.randint(0, 2)) if two_cams else 0
            pm = Tcw32[p, :3, :3].astype(np.float64) @ pts32[l].astype(np.float64) + Tcw32[p, :3, 3]
            pc = Tcim[cam, :3, :3].astype(np.float64) @ pm + Tcim[cam, :3, 3]
            if pc[2] < 0.5:
                continue
            octave = int(rng.randint(0, 8))
            sigma = 1.2 ** octave
            u, v = FX * pc[0] / pc[2] + CX, FY * pc[1] / pc[2] + CY
            ur = u - BF / pc[2]
            if noise:
                u, v, ur = u + rng.normal(0, 0.6 * sigma), v + rng.normal(0, 0.6 * sigma), ur + rng.normal(0, 0.6 * sigma)
            if rng.uniform() < wrong:
                d = rng.uniform(15.0, 60.0) * (1 if rng.uniform() < 0.5 else -1)
                u, v, ur = u + d, v - 0.7 * d, ur + d
                n_wrong += 1
            stereo = form == "stereo" or (form == "mixed" and rng.uniform() < 0.5)
            edge_pose.append(int(p)); edge_cam.append(cam); obs.append([u, v, ur if stereo else -1.0]); w.append(1.0 / (sigma * sigma))
        first.append(len(edge_pose))
    truth = {"Tcw": Tcw32.copy(), "points": pts32.copy()}
    Tcw0, pts0 = Tcw32.copy(), pts32.copy()
    if start != "exact":
        mag = {"near": 0.2, "off": 1.0}[start]
        for p in range(n_free):
            dR = rot(*(rng.uniform(-1, 1, 3) * math.radians(2.0) * mag))
            M = np.eye(4); M[:3, :3] = dR; M[:3, 3] = rng.uniform(-1, 1, 3) * 0.05 * mag
            Tcw0[p] = (M @ Tcw32[p].astype(np.float64)).astype(np.float32)
        pts0 = (pts32 + rng.uniform(-1, 1, (n_points, 3)) * 0.05 * mag).astype(np.float32)
    K = np.tile(np.array([FX, FY, CX, CY, BF], np.float32), (n_poses, 1))
    return {"n_free": n_free, "Tcw": Tcw0.reshape(-1, 16), "K": K, "points": pts0, "first": np.asarray(first, np.int32),
            "edge_pose": np.asarray(edge_pose, np.int32).reshape(-1), "edge_cam": np.asarray(edge_cam, np.uint8).reshape(-1),
            "obs": np.asarray(obs, np.float32).reshape(-1, 3), "inv_sigma2": np.asarray(w, np.float32).reshape(-1), "Tcim": Tcim.reshape(2, 16),
            "bad": None, "truth": truth, "n_wrong": n_wrong}


# name -> (free, fixed, points, seed, form, wrong, start, max_obs)
WORLDS = {
    "f1_x0_p1_stereo": (1, 0, 1, 11, "stereo", 0.0, "near", 6),
    "f2_x1_p40_mixed_wrong10": (2, 1, 40, 12, "mixed", 0.1, "off", 6),
    "f7_x5_p3000_mixed_wrong10": (7, 5, 3000, 13, "mixed", 0.1, "off", 12),
    "f7_x5_p300_mono_wrong40": (7, 5, 300, 14, "mono", 0.4, "near", 12),
    "f20_x12_p600_stereo_clean_exact": (20, 12, 600, 15, "stereo", 0.0, "exact", 8),
    "f64_x40_p400_mixed_wrong10": (64, 40, 400, 16, "mixed", 0.1, "off", 6),
    "f65_x3_p150_mixed": (65, 3, 150, 17, "mixed", 0.1, "near", 8),          # past ORBM_LBA_MAX_FREE
}
_cache = {}


def world(name):
    if name not in _cache:
        f, x, n, seed, form, wrong, start, mo = WORLDS[name]
        _cache[name] = make_world(f, x, n, seed, form, wrong, start, mo)
    return _cache[name]


def to_problem(m, W):
    return m.LocalBAProblem(W["n_free"], W["Tcw"], W["K"], W["points"], W["first"], W["edge_pose"], W["edge_cam"], W["obs"], W["inv_sigma2"],
                            W["Tcim"], W.get("bad"))


def check_band(R):
    """Every chi2 a test of the model run R compared keeps BAND (relative) from its threshold, every depth BAND from 0."""
    import lba_model as lm
    assert R.trace.tests or R.ended == lm.ENDED_STOPPED_AT_START
    for chi2, zc, tested in R.trace.tests:
        for th in (lm.TH_MONO, lm.TH_STEREO):
            with np.errstate(invalid="ignore"):
                margin = np.abs(chi2[tested] - th) / th
            assert not (margin < BAND).any(), ("a chi2 within the guard band of", th, float(np.nanmin(margin)))
        finite = np.isfinite(zc)
        assert not (np.abs(zc[finite & tested]) < BAND).any(), "a depth within the guard band of 0"


# ---- hand-built cases --------------------------------------------------------------------------------------------------------------------
def _with(W, **kw):
    out = dict(W)
    out.update(kw)
    return out


def hand_cases():
    """name -> (world, what the result must show: a dict of attribute -> value, or a callable on the model's / library's result)."""
    cases = {}
    base = make_world(3, 2, 60, 21, "mixed", 0.1, "off", 5)
    # a point seen once; a point seen only by fixed poses
    W = make_world(3, 2, 30, 22, "mixed", 0.0, "near", 5)
    first = W["first"].copy(); l = int(np.argmax(np.diff(first) >= 2))
    keep = np.ones(len(W["edge_pose"]), bool); keep[first[l] + 1:first[l + 1]] = False      # point l keeps one edge
    l2 = l + 1
    fixed_only = W["edge_pose"][first[l2]:first[l2 + 1]] >= W["n_free"]
    if not fixed_only.any():
        W["edge_pose"][first[l2]] = W["n_free"]                                            # ... make one fixed
        fixed_only = W["edge_pose"][first[l2]:first[l2 + 1]] >= W["n_free"]
    keep[first[l2]:first[l2 + 1]] = fixed_only
    for a in range(first[l2], first[l2 + 1]):                                              # (no duplicate pose inside the row)
        if keep[a] and (W["edge_pose"][first[l2]:a][keep[first[l2]:a]] == W["edge_pose"][a]).any():
            keep[a] = False
    counts = np.add.reduceat(keep.astype(np.int64), first[:-1]) if len(keep) else np.zeros(0, np.int64)
    counts[np.diff(first) == 0] = 0
    nf = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    cases["seen_once_and_fixed_only"] = (_with(W, first=nf, edge_pose=W["edge_pose"][keep], edge_cam=W["edge_cam"][keep], obs=W["obs"][keep],
                                               inv_sigma2=W["inv_sigma2"][keep]), {"ended": 0, "optimisations": 2})
    # keyframe 0 among the local ones: the caller hands it in as the first fixed pose.  It is covisible with the free keyframes, so it
    # sees most of their points (every point here is seen by up to all four keyframes), unlike a fixed camera at the rim of the map
    W = make_world(3, 1, 40, 27, "mixed", 0.1, "off", 4)
    cases["keyframe_0_among_the_local"] = (W, lambda R, W=W: R.ended == 0 and R.optimisations == 2 and R.active_poses == (3, 3)
                                           and (W["edge_pose"] == 3).sum() > 20)
    # ... and when keyframe 0 is the ONLY local keyframe no pose is free
    W = make_world(0, 3, 25, 23, "stereo", 0.0, "near", 3)
    cases["no_free_pose"] = (W, {"ended": 0, "optimisations": 2, "active_poses": (0, 0)})
    # an optimisation in which a pose loses all its edges at the first test: free pose 1 starts looking the other way, so every point
    # it observes lies behind it (isDepthPositive fails) and five iterations do not turn it round
    W = dict(base)
    Tcw = W["Tcw"].copy().reshape(-1, 4, 4)
    Tcw[1] = (np.diag([-1.0, 1.0, -1.0, 1.0]) @ Tcw[1].astype(np.float64)).astype(np.float32)
    cases["pose_loses_all_edges"] = (_with(W, Tcw=Tcw.reshape(-1, 16)), lambda R: R.active_poses == (3, 2) and R.optimisations == 2)
    # a failed solve: with every weight zero the system is zero, lambda = 1e-5 * 0, D.inverse() is 0 * inf and the first pivot is not finite
    W = make_world(2, 1, 20, 24, "mono", 0.0, "near", 3)
    cases["zero_pivot"] = (_with(W, inv_sigma2=np.zeros_like(W["inv_sigma2"])), lambda R: R.rounds["trials"][0] >= 1 and R.rounds["lambda"][0] == 0.0)
    # a point at depth 0 in camera 1: identity pose, point at z = 1, Tcim[1] moves it back by exactly 1
    Tcim = np.stack([np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)]); Tcim[1, 2, 3] = -1.0
    W = make_world(2, 1, 12, 25, "mono", 0.0, "exact", 3, two_cams=False)
    Tcw = W["Tcw"].copy(); Tcw[0] = np.eye(4, dtype=np.float32).reshape(16)
    pts = W["points"].copy(); pts[0] = (0.25, -0.125, 1.0)
    e0 = int(W["first"][0])
    ep, ec = W["edge_pose"].copy(), W["edge_cam"].copy()
    row = slice(int(W["first"][0]), int(W["first"][1]))
    others = [p for p in range(3) if p != 0]
    for j, a in enumerate(range(row.start, row.stop)):
        ep[a] = 0 if j == 0 else others[(j - 1) % 2]
    if row.stop - row.start > 3:
        raise AssertionError("the first point has too many edges for this case")
    ec[e0] = 1
    cases["depth_zero_in_camera_1"] = (_with(W, Tcw=Tcw, points=pts, edge_pose=ep, edge_cam=ec, Tcim=Tcim.reshape(2, 16)),
                                       lambda R: bool(R.flags[e0] & 2))
    # bad points keep their edges out of both tests
    W = dict(base); bad = np.zeros(len(W["points"]), np.uint8); bad[::3] = 1
    per_edge = np.repeat(bad, np.diff(W["first"])) != 0
    cases["bad_points"] = (_with(W, bad=bad), lambda R, per_edge=per_edge: not R.flags[per_edge].any() and R.flags.any())
    # no edge at all, no point at all
    W = make_world(2, 1, 5, 26, "mono", 0.0, "near", 3)
    cases["no_edges"] = (_with(W, first=np.zeros(6, np.int32), edge_pose=np.zeros(0, np.int32), edge_cam=np.zeros(0, np.uint8),
                               obs=np.zeros((0, 3), np.float32), inv_sigma2=np.zeros(0, np.float32)), {"optimisations": 0, "n_erase": 0})
    return cases


def stop_cases():
    """name -> (world, n: the stop function is true from the n-th poll on, ended, an exit the model's trace must show or None, the polls
    the call makes).  The polls
    of a run: 0 is Optimizer.cc:1204, then one per iteration of optimize() (sparse_optimizer.cpp:376) and one per rejected trial that
    would be followed by another (levenberg.cpp:149), then :1217."""
    W = world("f7_x5_p300_mono_wrong40")        # five accepted iterations in optimize(5): polls 1 .. 5, no sixth (i == iterations), :1217 is poll 6
    Z = hand_cases()["zero_pivot"][0]           # every trial is rejected: poll 1 is :376, polls 2 .. are :149
    return {"at_poll_0": (W, 0, 1, None, 1),                        # :1204 and nothing else
            "after_optimize_5": (W, 6, 2, None, 7),                 # 0 .. 5 false, :1217 true
            "inside_optimize_5": (W, 3, 2, "stop_376", 5),          # :376 true at poll 3, then :1217
            "inside_optimize_10": (W, 9, 0, "stop_376", 10),        # :1217 was poll 6; :376 of the third iteration of optimize(10), no poll behind it
            "inside_a_trial_loop": (Z, 4, 2, "stopped", 7)}         # :149 true at poll 4, :376 of the next iteration, :1217
