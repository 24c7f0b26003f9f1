"""Optimizer::GlobalBundleAdjustemnt / BundleAdjustment (host/Optimizer.h, host/GlobalBA.cc) through its driver host/test_global_ba: a
stand-in map built from a world of tests/gba_worlds.py (the map builder and the file format are the local BA's,
tests/test_local_ba_class.py) against a transcription of the reference's filtering (src/Optimizer.cc:102-276: bad keyframes and bad
points skipped, a pose fixed iff mnId == 0, observations of bad keyframes dropped, a point without an edge left out) and recovery
(:282-328) around the library's own call on the arrays the transcription makes: the values written by SetPose / SetWorldPos or into
mTcwGBA / mPosGBA, the mnBAGlobalForKF marks, and the ORDER of the calls on the map.  The CPU half stays under GBA_HOST_BELOW edges (the
class takes the host routine), the GPU half lies above it (the device)."""
import os
import re
import subprocess

import numpy as np
import pytest

import multi_orb_slam_amd as m
import gba_worlds as gw
import test_local_ba_class as lbc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "multi_orb_slam_amd", "host")
DRIVER = os.path.join(HOST, "test_global_ba")
HOST_BELOW = int(re.search(r"const int GBA_HOST_BELOW = (\d+);", open(os.path.join(HOST, "GlobalBA.cc")).read()).group(1))


def make_map(W, seed, loop_kf, with_kf0=True, bad_kf=False, stop=-1):
    """The local BA's stand-in map of the world (keyframe i is pose i, mnIds shuffled, every 17th point bad, features shuffled); its
    `current` field carries nLoopKF.  with_kf0: one keyframe has mnId 0 and is therefore fixed -- whatever the world meant it to be."""
    M = lbc.make_map(W, seed, with_kf0=with_kf0, bad_kf=bad_kf, stop=stop)
    M["current"] = loop_kf
    return M


def transcription(M, iterations, robust, run):
    kfs, mps = M["kfs"], M["mps"]
    loop_kf = M["current"]
    observers = [dict() for _ in mps]
    for i, K in enumerate(kfs):
        for f, feat in enumerate(K["feats"]):
            if feat[5] >= 0 and i not in observers[feat[5]]:
                observers[feat[5]][i] = f
    good = [i for i in range(len(kfs)) if not kfs[i]["bad"]]
    max_id = max([kfs[i]["id"] for i in good] + [0])
    free = sorted([i for i in good if kfs[i]["id"] != 0], key=lambda i: kfs[i]["id"])
    poses = free + [i for i in good if kfs[i]["id"] == 0]
    pose_of = {i: p for p, i in enumerate(poses)}
    first, edge_pose, edge_cam, obs, w, included = [0], [], [], [], [], []
    for l in sorted([l for l in range(len(mps)) if not mps[l]["bad"]], key=lambda l: mps[l]["id"]):
        n = 0
        for i in sorted(observers[l], key=lambda i: kfs[i]["id"]):
            if kfs[i]["bad"] or kfs[i]["id"] > max_id:
                continue
            x, y, octave, ur, cam, _ = kfs[i]["feats"][observers[l][i]]
            edge_pose.append(pose_of[i]); edge_cam.append(cam); obs.append([x, y, ur]); w.append(M["levels"][octave]); n += 1
        if n:
            included.append(l); first.append(len(edge_pose))
    R12 = np.asarray(M["Rcam12"], np.float32); t12 = np.asarray(M["tcam12"], np.float32).reshape(3, 1)
    T21 = np.zeros((4, 4), np.float32); R21 = R12.T.copy(); T21[:3, :3] = R21; T21[3, 3] = 1.0
    for r in range(3):      # `-Rcam21 * tcam21`: cv::gemm's small path, float products and sums left to right, alpha = -1 in double
        t = np.float32(np.float32(R21[r, 0] * t12[0, 0]) + np.float32(R21[r, 1] * t12[1, 0]))
        t = np.float32(t + np.float32(R21[r, 2] * t12[2, 0]))
        T21[r, 3] = np.float32(float(t) * -1.0)
    P = m.LocalBAProblem(len(free), np.array([kfs[i]["Tcw"] for i in poses], np.float32).reshape(-1, 16),
                         np.array([kfs[i]["K"] for i in poses], np.float32).reshape(-1, 5), np.array([mps[l]["pos"] for l in included], np.float32).reshape(-1, 3),
                         np.asarray(first, np.int32), np.asarray(edge_pose, np.int32), np.asarray(edge_cam, np.uint8),
                         np.asarray(obs, np.float32).reshape(-1, 3), np.asarray(w, np.float32), np.stack([np.eye(4, dtype=np.float32), T21]))
    stop = None if M["stop"] < 0 else (lambda: M["stop"] > 0)
    R = run(P, iterations, robust, stop)
    zero16, zero3 = np.zeros(16, np.float32), np.zeros(3, np.float32)
    row = {l: k for k, l in enumerate(included)}
    want_kf, want_mp, calls = [], [], []
    for i, K in enumerate(kfs):                               # vpKFs' order
        pose, gba, mark = np.asarray(K["Tcw"], np.float32), zero16, 0
        if not K["bad"]:
            if loop_kf == 0:
                pose = R.Tcw[pose_of[i]]; calls.append(("SetPose", K["id"], 0))
            else:
                gba, mark = R.Tcw[pose_of[i]], loop_kf
        want_kf.append((K["id"], mark, pose.tobytes(), gba.tobytes()))
    for l, Pt in enumerate(mps):                              # vpMP's order, not that of the vertex ids
        pos, gba, mark = np.asarray(Pt["pos"], np.float32), zero3, 0
        if l in row and not Pt["bad"]:
            if loop_kf == 0:
                pos = R.point_f[row[l]]; calls.append(("SetWorldPos", Pt["id"], 0))
            else:
                gba, mark = R.point_f[row[l]], loop_kf
        want_mp.append((Pt["id"], mark, pos.tobytes(), gba.tobytes()))
    if loop_kf == 0:                                          # UpdateNormalAndDepth, batched behind the last SetWorldPos
        calls += [("SetNormalAndDepth", mps[l]["id"], 0) for l in range(len(mps)) if l in row and not mps[l]["bad"]]
    return want_kf, want_mp, calls, R, P


def drive(M, iterations, robust, tmp_path, driver=DRIVER, env=None):
    path = str(tmp_path / "map.txt")
    lbc.write_map(M, path)
    out = subprocess.run([driver, path, str(iterations), "1" if robust else "0"], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, (out.returncode, out.stderr[-3000:])
    got_kf, got_mp, got_calls = [], [], []
    bits = lambda t: np.array([int(v, 16) for v in t], np.uint32).view(np.float32).tobytes()
    for line in out.stdout.splitlines():
        t = line.split()
        if t[0] == "KF":
            got_kf.append((int(t[1]), int(t[2]), bits(t[3:19]), bits(t[19:35])))
        elif t[0] == "MP":
            got_mp.append((int(t[1]), int(t[2]), bits(t[3:6]), bits(t[6:9])))
        elif t[0] == "CALL":
            got_calls.append((t[1], int(t[2]), int(t[3])))
    return got_kf, got_mp, got_calls, out.stdout + out.stderr


def check(M, iterations, robust, tmp_path, run, **kw):
    want_kf, want_mp, want_calls, R, P = transcription(M, iterations, robust, run)
    got_kf, got_mp, got_calls, _ = drive(M, iterations, robust, tmp_path, **kw)
    assert len(got_kf) == len(want_kf) and len(got_mp) == len(want_mp)
    for g, w in zip(got_kf, want_kf):
        assert g == w, ("keyframe", g[:2], w[:2], g[2] == w[2], g[3] == w[3])
    for g, w in zip(got_mp, want_mp):
        assert g == w, ("point", g[:2], w[:2], g[2] == w[2], g[3] == w[3])
    first_diff = next((k for k, (g, w) in enumerate(zip(got_calls, want_calls)) if g != w), None)
    assert first_diff is None and len(got_calls) == len(want_calls), (first_diff, len(got_calls), len(want_calls),
                                                                        got_calls[first_diff or 0:(first_diff or 0) + 3], want_calls[first_diff or 0:(first_diff or 0) + 3])
    return R, P, want_calls


def host_route(P, iterations, robust, stop):
    assert P.n_edges < HOST_BELOW
    return m.bundle_adjust_host(P, iterations, robust, m.POSE_ORDER_DEVICE, stop=stop)


def small_world():
    # 15 points, one of them bad: fewer points than REFRESH_HOST_BELOW (16), so that RefreshMapPoints too takes its host routine and the
    # whole sequence of calls is the same with and without a device
    return gw.make_world(5, 15, 61, "mixed", 0.1, 4, True, "off")


CASES = {"tracking": (0, 20, True, {}), "loop": (7, 10, False, {"stop": 0}), "bad_keyframe": (0, 10, True, {"bad_kf": True}),
         "loop_bad_keyframe": (3, 10, False, {"bad_kf": True}), "no_keyframe_0": (0, 5, True, {"with_kf0": False}),
         "flag_set": (0, 10, True, {"stop": 1})}


@pytest.mark.parametrize("case", list(CASES))
def test_the_class_on_the_host_route(case, tmp_path):
    loop_kf, iterations, robust, kw = CASES[case]
    M = make_map(small_world(), 5, loop_kf, **kw)
    R, P, calls = check(M, iterations, robust, tmp_path, host_route)
    n_good = sum(1 for K in M["kfs"] if not K["bad"])
    assert P.n_poses == n_good and P.n_free == n_good - (0 if case == "no_keyframe_0" else 1)
    assert R.optimised == 1 and (R.polls > 0) == ("stop" in kw)
    kinds = [c[0] for c in calls]
    if loop_kf:
        assert calls == []
    else:
        assert kinds.count("SetPose") == n_good and kinds.count("SetWorldPos") == kinds.count("SetNormalAndDepth") == P.n_points > 0
        assert kinds.index("SetWorldPos") > max(k for k, v in enumerate(kinds) if v == "SetPose")
        assert "lock" not in kinds                              # the reference takes no map mutex here
    if case == "flag_set":
        assert R.polls == 1 and R.round["iterations"][0] == 0   # the estimates reached so far -- the start -- are written all the same
        assert kinds.count("SetPose") == n_good
    if "bad_kf" in kw:
        assert any(K["bad"] for K in M["kfs"]) and P.n_edges < sum(1 for K in M["kfs"] for f in K["feats"] if f[5] >= 0 and not M["mps"][f[5]]["bad"])


def test_the_class_under_asan_and_ubsan(tmp_path):
    """The sanitized stand-alone driver (host/Makefile: test_global_ba_san) on the host route: GlobalBA.cc's filtering, flattening and
    recovery, MapPointRefresh.cc and the driver itself under AddressSanitizer + UndefinedBehaviorSanitizer; the same answers."""
    subprocess.check_call(["make", "-s", "-C", HOST, "test_global_ba_san"], timeout=900)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    for case in ("tracking", "loop_bad_keyframe"):
        loop_kf, iterations, robust, kw = CASES[case]
        M = make_map(small_world(), 5, loop_kf, **kw)
        check(M, iterations, robust, tmp_path, host_route, driver=DRIVER + "_san", env=env)
        out = drive(M, iterations, robust, tmp_path, driver=DRIVER + "_san", env=env)[3]
        assert not any(mk in out for mk in ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:"))


@pytest.mark.gpu
def test_the_class_on_the_device(tmp_path):
    W = gw.make_world(12, 900, 62, "mixed", 0.1, 6, True, "off")
    mt = m.Matcher(0.8, True)
    try:
        def device_route(P, iterations, robust, stop):
            assert P.n_edges >= HOST_BELOW
            R = mt.bundle_adjust(P, iterations, robust, stop=stop)
            assert mt.last_bundle_adjust()[0] == 0
            return R
        for loop_kf, iterations, robust in ((0, 20, True), (9, 10, False)):
            M = make_map(W, 6, loop_kf, stop=0)
            R, P, calls = check(M, iterations, robust, tmp_path, device_route)
            assert R.optimised == 1 and P.n_free == 12 and (len(calls) > 1000) == (loop_kf == 0)
    finally:
        mt.close()
