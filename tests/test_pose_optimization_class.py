"""Optimizer::PoseOptimization (host/Optimizer.h) through its driver host/test_pose: stand-in frames built from the worlds of
tests/pose_worlds.py; mvbOutlier, the return value and mTcw against the model.  Below POSE_HOST_BELOW edges a single call takes the
library's host routine (no device needed); from there on, and for every batched call, the device."""
import os
import subprocess

import numpy as np
import pytest

import pose_model as pm
import pose_worlds as pw
from test_pose_model import ORDER_DIFF_TRANSLATION, POSE_MARGIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "multi_orb_slam_amd", "host", "test_pose")
WORLD = dict(pw.worlds())


def hexf(a):
    return " ".join("%08x" % v for v in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32))


def frame_lines(P, n_total, unmatched):
    """A stand-in frame whose features with a map point are the world's edges; `unmatched` features (no point) are strewn between them."""
    lines = ["%d %d" % (P["n_cam0"], n_total), hexf(P["Tcw"]), hexf([P["fx"], P["fy"], P["cx"], P["cy"], P["bf"]]),
             hexf(P["Rcam12"]), hexf(P["tcam12"]), "%d" % len(P["inv_level_sigma2"]), hexf(P["inv_level_sigma2"])]
    at = {int(f): e for e, f in enumerate(P["feat"])}
    for i in range(n_total):
        if i in at and i not in unmatched:
            e = at[i]
            lines.append("%s %d %s 1 %s" % (hexf(P["obs"][e, :2]), P["octave"][e], hexf(P["obs"][e, 2]), hexf(P["pos"][e])))
        else:
            lines.append("%s 0 %s 0 %s" % (hexf([10.0, 20.0]), hexf(-1.0), hexf([0, 0, 0])))
    return lines


def spread(P, every=5):
    """The same world with its edges moved to feature indices that leave every fifth feature without a map point (camera split kept)."""
    n = len(P["feat"])
    n0 = int((P["feat"] < P["n_cam0"]).sum())
    idx = np.array([i for i in range(2 * n + 10) if i % every != 0], np.int32)
    Q = dict(P)
    cam0 = idx[:n0]
    new_n_cam0 = int(cam0[-1]) + 2 if n0 else 0
    cam1 = idx[idx >= new_n_cam0][:n - n0]
    Q["feat"] = np.concatenate([cam0, cam1]).astype(np.int32)
    Q["n_cam0"] = new_n_cam0
    n_total = int(Q["feat"].max()) + 3 if n else 4
    if P["mode"] == pm.CAM0:
        Q["n_cam0"] = n_total                                    # (one camera: every feature is camera 1's)
    return Q, n_total


def run_driver(tmp_path, problems, batch=False):
    allcams = int(problems[0][0]["mode"] == pm.ALL_CAMS)
    lines = ["%d %d" % (len(problems), allcams)]
    for P, n_total in problems:
        lines += frame_lines(P, n_total, ())
    f = tmp_path / "frames.txt"
    f.write_text("\n".join(lines) + "\n")
    p = subprocess.run(["timeout", "-k", "10", "120", DRIVER, str(f)] + (["batch"] if batch else []), capture_output=True, text=True, timeout=150)
    assert p.returncode == 0, p.stderr[-2000:]
    out = []
    for line in p.stdout.splitlines():
        t = line.split()
        out.append((int(t[0]), np.array([int(x, 16) for x in t[1:17]], np.uint32).view(np.float32), np.array([c == "1" for c in t[17]])))
    assert len(out) == len(problems)
    return out


def check_against_model(P, n_total, got, exact_pose):
    ret, Tcw, outlier = got
    rec, flags = pm.optimize(P, "device")                       # (what the library computes, bit for bit)
    irec, iflags = pm.optimize(P, "index")
    assert ret == rec["n_inliers"] == irec["n_inliers"]
    want = np.ones(n_total, bool)                                # the driver starts every flag at true: only edges are written
    want[P["feat"]] = flags != 0                                 # (false for every edge when fewer than 3: set while the edges are built)
    assert np.array_equal(outlier, want) and np.array_equal(flags, iflags)
    assert Tcw.tobytes() == rec["Tcw"].tobytes()
    if rec["n_initial"] >= 3:
        assert np.abs(Tcw.reshape(4, 4)[:3, 3].astype(np.float64) - irec["t"]).max() <= POSE_MARGIN * ORDER_DIFF_TRANSLATION + 2.0 ** -22 * np.abs(irec["t"]).max()


@pytest.mark.parametrize("name", ["two/cam0", "nine/cam0", "nine/all", "exact/cam0", "all_outliers/all"])
def test_class_on_small_problems_takes_the_host_routine(tmp_path, name):
    P, n_total = spread(WORLD[name])
    assert len(P["feat"]) < 16
    (got,) = run_driver(tmp_path, [(P, n_total)])
    check_against_model(P, n_total, got, True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mixed_400/cam0", "rig_400/all", "stereo_2000/cam0", "rig_2000/all", "rig_8000_mono/all", "behind/all"])
def test_class_on_the_device(tmp_path, name):
    import torch  # noqa: F401
    P, n_total = spread(WORLD[name])
    (got,) = run_driver(tmp_path, [(P, n_total)])
    check_against_model(P, n_total, got, True)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["cam0", "all"])
def test_batched_static_equals_eight_single_calls(tmp_path, mode):
    import torch  # noqa: F401
    names = ["mono_60", "stereo_60", "mixed_400", "mono_400_far", "rig_400", "mixed_2000", "nine", "two"]
    problems = [spread(WORLD["%s/%s" % (n, mode)]) for n in names]
    single = run_driver(tmp_path, problems, batch=False)
    batched = run_driver(tmp_path, problems, batch=True)
    for n, a, b, (P, n_total) in zip(names, single, batched, problems):
        assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2]), n
        check_against_model(P, n_total, b, True)
