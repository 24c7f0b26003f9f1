"""Seeded worlds for the global bundle adjustment (tests/test_gba_model.py, tests/test_gpu_gba.py): a keyframe TRAJECTORY.  Keyframe 0
is fixed (it is the problem's last pose: free poses come first), every other keyframe is free; a point is seen by a window of consecutive
keyframes, so most pairs of poses share no point and the reduced system is block-banded -- or, with window=None, by every keyframe, so
that every block pair exists.  Mono / stereo / mixed observations through either camera of the rig, 0 / 10 % of them wrong by tens of
pixels, built from lba_worlds' pieces (its rig, its intrinsics, its noise model).  A world is the dict lba_model.Graph reads and
lba_worlds.to_problem hands to the library.

The seeded worlds are chosen so that every solve of the host routine succeeds (the model's trace counts the failures;
tests/test_gba_model.py asserts 0 for the worlds it runs, and the larger worlds of tests/test_gpu_gba.py were run through the model once
when their seeds were fixed).  Only the hand-built cases may fail a solve."""
import math
import numpy as np

import lba_worlds as lw
from lba_worlds import FX, FY, CX, CY, BF, rot, tcim_pair

STEP = 0.4             # metres between consecutive keyframes along x


def make_world(n_free, n_points, seed, form="mixed", wrong=0.1, window=5, two_cams=True, start="off", n_fixed=1):
    """n_free free keyframes at slots n_fixed .. of the path, n_fixed fixed ones at slots 0 ..; a point is seen by `window` (at most)
    consecutive slots around the place it lies in front of, window=None: by all."""
    rng = np.random.RandomState(seed)
    n_poses = n_free + n_fixed
    Tcim = tcim_pair()
    slot_pose = [n_free + s if s < n_fixed else s - n_fixed for s in range(n_poses)]      # slot -> pose index
    Tcw = np.zeros((n_poses, 4, 4))
    for s, p in enumerate(slot_pose):
        c = np.array([STEP * s, rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)])
        Rwc = rot(rng.uniform(-0.03, 0.03), rng.uniform(-0.06, 0.06), rng.uniform(-0.03, 0.03))
        Tcw[p, :3, :3] = Rwc.T; Tcw[p, :3, 3] = -Rwc.T @ c; Tcw[p, 3, 3] = 1.0
    Tcw32 = Tcw.astype(np.float32)
    pts = np.zeros((n_points, 3))
    first, edge_pose, edge_cam, obs, w = [0], [], [], [], []
    n_wrong = 0
    for l in range(n_points):
        if window is None:
            s0, k = 0, n_poses
            pts[l] = (rng.uniform(-1.0, STEP * (n_poses - 1) + 1.0), rng.uniform(-1.5, 1.5), rng.uniform(5.0, 10.0))
        else:
            k = int(rng.randint(2, min(n_poses, window) + 1)) if n_poses > 1 else 1
            s0 = int(rng.randint(0, n_poses - k + 1))
            pts[l] = (STEP * (s0 + 0.5 * (k - 1)) + rng.uniform(-1.0, 1.0), rng.uniform(-1.5, 1.5), rng.uniform(4.0, 10.0))
        X = pts[l].astype(np.float32).astype(np.float64)
        for s in rng.permutation(np.arange(s0, s0 + k)):          # the caller's order inside a point: any
            p = slot_pose[int(s)]
            cam = int(rng.randint(0, 2)) if two_cams else 0
            pm = Tcw32[p, :3, :3].astype(np.float64) @ X + Tcw32[p, :3, 3]
            pc = Tcim[cam, :3, :3].astype(np.float64) @ pm + Tcim[cam, :3, 3]
            if pc[2] < 0.5:
                continue
            octave = int(rng.randint(0, 8))
            sigma = 1.2 ** octave
            u, v = FX * pc[0] / pc[2] + CX, FY * pc[1] / pc[2] + CY
            ur = u - BF / pc[2]
            u, v, ur = u + rng.normal(0, 0.6 * sigma), v + rng.normal(0, 0.6 * sigma), ur + rng.normal(0, 0.6 * sigma)
            if rng.uniform() < wrong:
                d = rng.uniform(15.0, 60.0) * (1 if rng.uniform() < 0.5 else -1)
                u, v, ur = u + d, v - 0.7 * d, ur + d
                n_wrong += 1
            stereo = form == "stereo" or (form == "mixed" and rng.uniform() < 0.5)
            edge_pose.append(int(p)); edge_cam.append(cam); obs.append([u, v, ur if stereo else -1.0]); w.append(1.0 / (sigma * sigma))
        first.append(len(edge_pose))
    pts32 = pts.astype(np.float32)
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


# name -> (free, points, seed, form, wrong, window, two_cams)
WORLDS = {
    # the model's worlds (CPU)
    "f1_p30_stereo": (1, 30, 101, "stereo", 0.0, 5, True),
    "f7_p150_mixed_wrong10": (7, 150, 102, "mixed", 0.1, 4, True),
    "f7_p120_mono_one_camera": (7, 120, 103, "mono", 0.0, 4, False),
    "f20_p300_mixed_wrong10": (20, 300, 104, "mixed", 0.1, 5, True),
    # the device's worlds: the panel boundary (10 and 11 poses: 60 and 66 rows), the local BA's cap and past it, more than one panel
    "f10_p150_mixed_wrong10": (10, 150, 105, "mixed", 0.1, 5, True),
    "f11_p150_stereo": (11, 150, 106, "stereo", 0.0, 5, True),
    "f64_p400_mixed_wrong10": (64, 400, 107, "mixed", 0.1, 6, True),
    "f65_p400_mixed_wrong10": (65, 400, 108, "mixed", 0.1, 6, True),
    "f96_p600_mono_wrong10": (96, 600, 109, "mono", 0.1, 6, True),
    # every keyframe sees every point: every block pair exists
    "f12_p150_dense_mixed": (12, 150, 110, "mixed", 0.0, None, True),
}
_cache = {}


def world(name):
    if name not in _cache:
        f, n, seed, form, wrong, window, two = WORLDS[name]
        _cache[name] = make_world(f, n, seed, form, wrong, window, two)
    return _cache[name]


to_problem = lw.to_problem


def _keep_edges(W, keep):
    first = W["first"]
    counts = np.array([int(keep[first[l]:first[l + 1]].sum()) for l in range(len(first) - 1)], np.int64)
    nf = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    out = dict(W)
    out.update(first=nf, edge_pose=W["edge_pose"][keep], edge_cam=W["edge_cam"][keep], obs=W["obs"][keep], inv_sigma2=W["inv_sigma2"][keep])
    return out


def hand_cases(n_free=7, bad_pose=None):
    """name -> (world, robust, what the result must show: a callable on the library's result).  bad_pose: the free pose whose diagonal
    block holds the failing pivot of `non_finite_pivot_at_a_pose` (default: the middle one; the device's tests place it beyond the
    first panel)."""
    cases = {}
    # no fixed pose at all: the gauge is free, the damping alone makes the system definite
    W = make_world(n_free, 20 * n_free, 201, "mixed", 0.0, 4, True, "near", n_fixed=0)
    cases["no_fixed_pose"] = (W, True, lambda R, W=W: R.optimised == 1 and R.active_poses == W["n_free"])
    # a point seen only by the fixed pose: it is optimised all the same, and shares nothing with any free pose
    W = make_world(n_free, 20 * n_free, 202, "mixed", 0.0, 4, True, "near")
    keep = np.ones(len(W["edge_pose"]), bool)
    l = int(np.argmax([(W["edge_pose"][W["first"][q]:W["first"][q + 1]] == n_free).any() for q in range(len(W["points"]))]))
    row = slice(int(W["first"][l]), int(W["first"][l + 1]))
    keep[row] = W["edge_pose"][row] == n_free
    Wk = _keep_edges(W, keep)
    cases["a_point_seen_only_by_the_fixed_pose"] = (Wk, False, lambda R, l=l, W=Wk: R.optimised == 1 and int(np.diff(W["first"])[l]) == 1
                                                    and not np.array_equal(R.point[l], W["points"][l].astype(np.float64)))
    # a keyframe that loses all its edges is not active: its estimate comes back as it went in
    W = make_world(n_free, 20 * n_free, 203, "mixed", 0.0, 4, True, "near")
    gone = n_free // 2
    Wk = _keep_edges(W, W["edge_pose"] != gone)
    cases["a_keyframe_without_edges"] = (Wk, True, lambda R, W=Wk, g=gone: R.active_poses == W["n_free"] - 1
                                         and float(np.abs(R.Tcw[g] - W["Tcw"][g]).max()) < 1e-6)     # (through toSE3Quat and back)
    # a failed solve at the first pivot, the local BA's case: with every weight zero the system is zero, lambda = 1e-5 * 0, D.inverse()
    # is 0 * inf and the first pivot is not finite.  Every trial is rejected with rho < 0, so the trial loop runs to qmax.
    W = make_world(n_free, 20 * n_free, 204, "mono", 0.0, 4, True, "near")
    cases["zero_pivot"] = (_with(W, inv_sigma2=np.zeros_like(W["inv_sigma2"])), False,
                           lambda R: R.round["trials"][0] >= 1 and R.round["lambda"][0] == 0.0)
    # a failed solve at a CHOSEN pivot: one more point, seen by bad_pose alone, whose observation is NaN.  Behind the Huber kernel
    # rho'(NaN) is NaN, so that edge's blocks are NaN: the diagonal block of bad_pose and nothing else of the reduced system (the point
    # is shared with nobody; computeLambdaInit's maximum never takes a NaN).  The rows before 6 * bad_pose factorise, pivot
    # 6 * bad_pose is NaN.  (An EXACT zero at a chosen pivot of a whole problem would need Hpp + lambda to cancel against the Schur
    # terms to the last bit; the solver's own tests place exact zeros.)
    W = make_world(n_free, 20 * n_free, 206, "mono", 0.0, 4, True, "near")
    bp = n_free // 2 if bad_pose is None else int(bad_pose)
    Wn = dict(W)
    Wn.update(points=np.concatenate([W["points"], [[STEP * (bp + 1), 0.0, 6.0]]]).astype(np.float32),
              first=np.concatenate([W["first"], [W["first"][-1] + 1]]).astype(np.int32),
              edge_pose=np.concatenate([W["edge_pose"], [bp]]).astype(np.int32), edge_cam=np.concatenate([W["edge_cam"], [0]]).astype(np.uint8),
              obs=np.concatenate([W["obs"], [[np.nan, np.nan, -1.0]]]).astype(np.float32),
              inv_sigma2=np.concatenate([W["inv_sigma2"], [1.0]]).astype(np.float32))
    cases["non_finite_pivot_at_a_pose"] = (Wn, True, lambda R, W=Wn: R.round["trials"][0] >= 1 and float(np.abs(R.Tcw - W["Tcw"].reshape(-1, 16)).max()) < 1e-6)
    # no edge at all
    W = make_world(n_free, 12, 205, "mono", 0.0, 4, True, "near")
    Wk = _keep_edges(W, np.zeros(len(W["edge_pose"]), bool))
    cases["no_edges"] = (Wk, True, lambda R: R.optimised == 0 and R.active_poses == 0 and R.active_edges == 0 and R.round["trials"][0] == 0)
    return cases


def _with(W, **kw):
    out = dict(W)
    out.update(kw)
    return out


def stop_cases():
    """name -> (world, iterations, robust, n: the stop function is true from the n-th poll on, an exit the model's trace must show, the
    polls the call makes).  Poll 1 is sparse_optimizer.cpp:376 of the first iteration; a rejected trial that would be followed by another
    polls levenberg.cpp:149."""
    W = world("f7_p150_mixed_wrong10")
    Z = hand_cases()["zero_pivot"][0]           # every trial is rejected: poll 1 is :376, polls 2 .. are :149
    return {"at_poll_1": (W, 10, True, 0, "stop_376", 1),
            "at_the_head_of_iteration_2": (W, 10, True, 1, "stop_376", 2),
            "inside_a_trial_loop": (Z, 10, False, 3, "stopped", 5)}
