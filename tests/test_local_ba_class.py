"""Optimizer::LocalBundleAdjustment (host/Optimizer.h, host/LocalBA.cc) through its driver host/test_local_ba: a stand-in map built from a
world of tests/lba_worlds.py -- keyframes with their covisibility lists, features and map-point matches, map points with their
observations -- against a transcription of steps 1-4 (the local keyframes, local points and fixed cameras with their marks) and 12-13
(the erasures, SetPose, SetWorldPos, UpdateNormalAndDepth) of the reference around the library's own call on the arrays the transcription
makes: the marks, the erasures, the values written, and the ORDER of the calls on the map, which the stand-in types record (the lock,
EraseMapPointMatch, EraseObservation, SetPose, SetWorldPos, SetNormalAndDepth, the unlock, each with its mnIds).  The CPU half
stays under LBA_HOST_BELOW edges (the class takes the host routine), the GPU half lies above it (the device)."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import multi_orb_slam_amd as m
import lba_worlds as lw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "multi_orb_slam_amd", "host", "test_local_ba")
HOST_BELOW = int(re.search(r"const int LBA_HOST_BELOW = (\d+);", open(os.path.join(ROOT, "multi_orb_slam_amd", "host", "LocalBA.cc")).read()).group(1))


def hx(v):
    return "%08x" % struct.unpack("<I", struct.pack("<f", float(np.float32(v))))[0]


def make_map(W, seed, with_kf0=False, bad_kf=False, stop=-1):
    """Keyframe i of the map is pose i of the world.  The current keyframe is free pose 0, the other free poses are its covisible
    keyframes (shuffled), the world's fixed poses are connected to nobody.  mnIds are shuffled; with_kf0 gives a covisible keyframe mnId 0."""
    rng = np.random.RandomState(seed)
    n_poses, n_free, n_points = len(W["Tcw"]), W["n_free"], len(W["points"])
    kf_id = rng.permutation(n_poses) + 1
    if with_kf0:
        kf_id[1 if n_free > 1 else 0] = 0
    mp_id = rng.permutation(n_points) + 100
    edge_point = np.repeat(np.arange(n_points), np.diff(W["first"]))
    kfs = []
    for i in range(n_poses):
        feats = []
        for e in np.nonzero(W["edge_pose"] == i)[0]:
            octave = int(round(-0.5 * np.log(W["inv_sigma2"][e]) / np.log(1.2)))
            feats.append([W["obs"][e, 0], W["obs"][e, 1], octave, W["obs"][e, 2], int(W["edge_cam"][e]), int(edge_point[e])])
            if rng.uniform() < 0.2:
                feats.append([10.0, 20.0, 0, -1.0, 0, -1])                       # a feature without a point
        order = rng.permutation(len(feats))
        kfs.append({"id": int(kf_id[i]), "bad": 0, "K": W["K"][i], "Tcw": W["Tcw"][i], "cov": [], "feats": [feats[k] for k in order]})
    kfs[0]["cov"] = [int(k) for k in rng.permutation(np.arange(1, n_free))]
    if bad_kf and n_free > 2:
        kfs[2]["bad"] = 1
    levels = 8
    inv_sigma2 = [np.float32(1.0 / (1.2 ** k) ** 2) for k in range(levels)]
    # (the observations carry the table's own entries, so that mvInvLevelSigma2[octave] is the world's weight bit for bit)
    for e in range(len(W["inv_sigma2"])):
        octave = int(round(-0.5 * np.log(W["inv_sigma2"][e]) / np.log(1.2)))
        assert inv_sigma2[octave] == W["inv_sigma2"][e]
    mps = []
    for l in range(n_points):
        seen = W["edge_pose"][W["first"][l]:W["first"][l + 1]]
        mps.append({"id": int(mp_id[l]), "bad": 1 if (l % 17 == 5) else 0, "pos": W["points"][l], "ref": int(seen[0]) if len(seen) else 0})
    T = W["Tcim"].reshape(2, 4, 4)
    R21, t21 = T[1, :3, :3], T[1, :3, 3]
    return {"kfs": kfs, "mps": mps, "current": 0, "stop": stop, "Rcam12": R21.T.copy(), "tcam12": lw.TCAM12, "levels": inv_sigma2,
            "scale": [np.float32(1.2 ** k) for k in range(levels)]}


def write_map(M, path):
    out = ["%d %d %d %d" % (len(M["kfs"]), len(M["mps"]), M["current"], M["stop"])]
    out.append(" ".join(hx(v) for v in np.asarray(M["Rcam12"], np.float32).reshape(9)))
    out.append(" ".join(hx(v) for v in np.asarray(M["tcam12"], np.float32).reshape(3)))
    out.append("%d" % len(M["levels"]))
    out.append(" ".join(hx(v) for v in M["levels"])); out.append(" ".join(hx(v) for v in M["scale"]))
    for K in M["kfs"]:
        out.append("%d %d" % (K["id"], K["bad"]))
        out.append(" ".join(hx(v) for v in K["K"])); out.append(" ".join(hx(v) for v in K["Tcw"]))
        out.append("%d %s" % (len(K["cov"]), " ".join(str(k) for k in K["cov"])))
        out.append("%d" % len(K["feats"]))
        for x, y, octave, ur, cam, mp in K["feats"]:
            out.append("%s %s %d %s %d %d" % (hx(x), hx(y), octave, hx(ur), cam, mp))
    for P in M["mps"]:
        out.append("%d %d %s %d" % (P["id"], P["bad"], " ".join(hx(v) for v in P["pos"]), P["ref"]))
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


def transcription(M, run):
    """Steps 1-4 and 12-13 of src/Optimizer.cc:921-1353 over the map M; run(problem, stop) -> LocalBAResult is the library's call.
    -> what the driver prints: per keyframe (local mark, fixed mark, pose 16 floats, matches), per point (local mark, position, observers)."""
    kfs, mps = M["kfs"], M["mps"]
    cur = kfs[M["current"]]
    local_mark = {i: 0 for i in range(len(kfs))}; fixed_mark = dict(local_mark); mp_mark = {l: 0 for l in range(len(mps))}
    matches = [[f[5] for f in K["feats"]] for K in kfs]
    observers = [dict() for _ in mps]                         # point -> {keyframe index: feature index}
    for i, K in enumerate(kfs):
        for f, feat in enumerate(K["feats"]):
            if feat[5] >= 0 and i not in observers[feat[5]]:
                observers[feat[5]][i] = f
    local = [M["current"]]; local_mark[M["current"]] = cur["id"]
    for k in cur["cov"]:
        local_mark[k] = cur["id"]
        if not kfs[k]["bad"]:
            local.append(k)
    lpoints = []
    for i in local:
        for mp in matches[i]:
            if mp >= 0 and not mps[mp]["bad"] and mp_mark[mp] != cur["id"]:
                lpoints.append(mp); mp_mark[mp] = cur["id"]
    fixed = []
    for mp in lpoints:
        for i in observers[mp]:
            if local_mark[i] != cur["id"] and fixed_mark[i] != cur["id"]:
                fixed_mark[i] = cur["id"]
                if not kfs[i]["bad"]:
                    fixed.append(i)
    free = sorted([i for i in local if kfs[i]["id"] != 0], key=lambda i: kfs[i]["id"])
    poses = free + [i for i in local if kfs[i]["id"] == 0] + fixed
    pose_of = {i: p for p, i in enumerate(poses)}
    points = sorted(lpoints, key=lambda l: mps[l]["id"])
    first, edge_pose, edge_cam, obs, w, edge_kf, edge_mp = [0], [], [], [], [], [], []
    for l in points:
        for i in sorted(observers[l], key=lambda i: kfs[i]["id"]):
            if kfs[i]["bad"] or i not in pose_of:
                continue
            x, y, octave, ur, cam, _ = kfs[i]["feats"][observers[l][i]]
            edge_pose.append(pose_of[i]); edge_cam.append(cam); obs.append([x, y, ur]); w.append(M["levels"][octave]); edge_kf.append(i); edge_mp.append(l)
        first.append(len(edge_pose))
    R12 = np.asarray(M["Rcam12"], np.float32); t12 = np.asarray(M["tcam12"], np.float32).reshape(3, 1)
    T21 = np.zeros((4, 4), np.float32); R21 = R12.T.copy(); T21[:3, :3] = R21; T21[3, 3] = 1.0
    for r in range(3):      # `-Rcam21 * pKF->mtcam12`: cv::gemm's small path, float products and sums left to right, alpha = -1 in double
        t = np.float32(np.float32(R21[r, 0] * t12[0, 0]) + np.float32(R21[r, 1] * t12[1, 0]))
        t = np.float32(t + np.float32(R21[r, 2] * t12[2, 0]))
        T21[r, 3] = np.float32(float(t) * -1.0)
    P = m.LocalBAProblem(len(free), np.array([kfs[i]["Tcw"] for i in poses], np.float32).reshape(-1, 16),
                         np.array([kfs[i]["K"] for i in poses], np.float32).reshape(-1, 5), np.array([mps[l]["pos"] for l in points], np.float32).reshape(-1, 3),
                         np.asarray(first, np.int32), np.asarray(edge_pose, np.int32), np.asarray(edge_cam, np.uint8),
                         np.asarray(obs, np.float32).reshape(-1, 3), np.asarray(w, np.float32), np.stack([np.eye(4, dtype=np.float32), T21]))
    stop = None if M["stop"] < 0 else (lambda: M["stop"] > 0)
    R = run(P, stop)
    pose = {i: np.asarray(kfs[i]["Tcw"], np.float32) for i in range(len(kfs))}
    pos = {l: np.asarray(mps[l]["pos"], np.float32) for l in range(len(mps))}
    calls = []                                              # the calls on the map, in the reference's order (:1311-1347)
    if R.ended != m.LBA_ENDED_STOPPED_AT_START:
        calls.append(("lock", 0, 0))                        # unique_lock<mutex> lock(pMap->mMutexMapUpdate) BEFORE the erasures
        for stereo in (False, True):                        # the mono edges, then the stereo ones
            for e in range(len(edge_pose)):
                if (obs[e][2] >= 0) == stereo and not mps[edge_mp[e]]["bad"] and R.flags[e] & m.LBA_FLAG_ERASE:
                    i, l = edge_kf[e], edge_mp[e]
                    calls.append(("EraseMapPointMatch", kfs[i]["id"], mps[l]["id"]))     # the keyframe first: it asks the point for its index
                    calls.append(("EraseObservation", mps[l]["id"], kfs[i]["id"]))
                    if i in observers[l]:
                        matches[i][observers[l][i]] = -1
                        del observers[l][i]
        for i in local:                                     # lLocalKeyFrames' order
            pose[i] = R.Tcw[pose_of[i]]
            calls.append(("SetPose", kfs[i]["id"], 0))
        point_row = {l: k for k, l in enumerate(points)}
        for l in lpoints:                                   # lLocalMapPoints' order, not that of the vertex ids
            pos[l] = R.point_f[point_row[l]]
            calls.append(("SetWorldPos", mps[l]["id"], 0))
        # UpdateNormalAndDepth of every local point that still has an observation, batched behind the last SetWorldPos
        calls += [("SetNormalAndDepth", mps[l]["id"], 0) for l in lpoints if observers[l]]
        calls.append(("unlock", 0, 0))
    want_kf = [(kfs[i]["id"], local_mark[i], fixed_mark[i], pose[i].tobytes(), matches[i]) for i in range(len(kfs))]
    want_mp = [(mps[l]["id"], mp_mark[l], pos[l].tobytes(), sorted(kfs[i]["id"] for i in observers[l])) for l in range(len(mps))]
    return want_kf, want_mp, calls, R, P


def drive(M, tmp_path):
    path = str(tmp_path / "map.txt")
    write_map(M, path)
    out = subprocess.run([DRIVER, path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    got_kf, got_mp, got_calls = [], [], []
    for line in out.stdout.splitlines():
        t = line.split()
        if t[0] == "KF":
            pose = np.array([int(v, 16) for v in t[4:20]], np.uint32).view(np.float32)
            got_kf.append((int(t[1]), int(t[2]), int(t[3]), pose.tobytes(), [int(v) for v in t[20:]]))
        elif t[0] == "MP":
            pos = np.array([int(v, 16) for v in t[3:6]], np.uint32).view(np.float32)
            got_mp.append((int(t[1]), int(t[2]), pos.tobytes(), sorted(int(v) for v in t[6:])))
        elif t[0] == "CALL":
            got_calls.append((t[1], int(t[2]), int(t[3])))
    return got_kf, got_mp, got_calls


def check(M, tmp_path, run):
    want_kf, want_mp, want_calls, R, P = transcription(M, run)
    got_kf, got_mp, got_calls = drive(M, tmp_path)
    assert len(got_kf) == len(want_kf) and len(got_mp) == len(want_mp)
    for g, w in zip(got_kf, want_kf):
        assert g == w, ("keyframe", g[:3], w[:3], g[3] == w[3], g[4] == w[4])
    for g, w in zip(got_mp, want_mp):
        assert g == w, ("point", g[:2], w[:2], g[2] == w[2], g[3], w[3])
    # the order of calls: the lock before the first erasure, EraseMapPointMatch before EraseObservation pair by pair, mono pairs before
    # stereo pairs, every SetPose before the first SetWorldPos, the refresh behind the last SetWorldPos, the lock held to the end
    first_diff = next((k for k, (g, w) in enumerate(zip(got_calls, want_calls)) if g != w), None)
    assert first_diff is None and len(got_calls) == len(want_calls), (first_diff, len(got_calls), len(want_calls),
                                                                        got_calls[first_diff or 0:(first_diff or 0) + 3], want_calls[first_diff or 0:(first_diff or 0) + 3])
    return R, P, want_calls


def host_route(P, stop):
    assert P.n_edges < HOST_BELOW
    return m.local_ba_host(P, m.POSE_ORDER_DEVICE, stop=stop)


@pytest.mark.parametrize("case", ["plain", "keyframe_0_local", "bad_keyframe", "no_flag", "stopped_at_start"])
def test_the_class_on_the_host_route(case, tmp_path):
    # 15 points, one of them bad: fewer local points than REFRESH_HOST_BELOW (16), so that RefreshMapPoints too takes its host routine
    # and the whole sequence of calls is the same with and without a device
    W = lw.make_world(4, 3, 15, 54, "mixed", 0.3, "off", 5)
    M = make_map(W, 3, with_kf0=case == "keyframe_0_local", bad_kf=case == "bad_keyframe", stop={"no_flag": -1, "stopped_at_start": 1}.get(case, 0))
    R, P, calls = check(M, tmp_path, host_route)
    if case == "stopped_at_start":
        assert R.ended == m.LBA_ENDED_STOPPED_AT_START and R.polls == 1 and calls == []
    else:
        assert R.ended == 0 and R.n_erase > 0 and P.n_free == (3 if case in ("keyframe_0_local", "bad_keyframe") else 4)
        assert (R.polls == 0) == (case == "no_flag")
        kinds = [c[0] for c in calls]
        assert kinds[0] == "lock" and kinds[-1] == "unlock" and kinds.count("EraseObservation") == kinds.count("EraseMapPointMatch") > 0
        assert kinds.count("SetPose") == P.n_free + (1 if case == "keyframe_0_local" else 0) and kinds.count("SetNormalAndDepth") > 0


@pytest.mark.gpu
def test_the_class_on_the_device(tmp_path):
    W = lw.make_world(6, 4, 900, 52, "mixed", 0.1, "off", 8)
    M = make_map(W, 4, stop=0)
    mt = m.Matcher(0.8, True)
    try:
        def device_route(P, stop):
            assert P.n_edges >= HOST_BELOW
            R = mt.local_ba(P, stop=stop)
            assert mt.last_local_ba()[0] == 0
            return R
        R, _, calls = check(M, tmp_path, device_route)
        assert R.ended == 0 and R.n_erase > 0
        kinds = [c[0] for c in calls]
        assert kinds.count("SetNormalAndDepth") > 100 and {"mono", "stereo"} == {"stereo" if o >= 0 else "mono" for o in W["obs"][:, 2]}
    finally:
        mt.close()
