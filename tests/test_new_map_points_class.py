"""TriangulateMatches (host/NewMapPoints.h) through its driver host/test_new_points: stand-in keyframes built from a generated world, the
verdict and the point of every pair against the NumPy model.  Below TRIANGULATE_HOST_BELOW pairs the class takes the library's host
routine (no device needed); from there on the device call."""
import os
import subprocess

import numpy as np
import pytest

import triangulate_model as tm
import triangulate_worlds as tw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "multi_orb_slam_amd", "host", "test_new_points")


def hexf(a):
    return " ".join("%08x" % v for v in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32))


def write_world(path, w, pairs):
    lines = ["%d %d %d" % (len(pairs), w.cam_enabled[0], w.cam_enabled[1])]
    for kf in (w.kf1, w.kf2):
        lines += ["%d %d" % (kf.n, kf.n_cam1), hexf(kf.Tcw[0]), hexf(kf.Tcw[1]),
                  hexf([kf.fx, kf.fy, kf.cx, kf.cy, kf.invfx, kf.invfy, kf.mbf, kf.mb, kf.scale_factors[1]]),
                  "%d" % len(kf.scale_factors), hexf(kf.scale_factors), hexf(kf.level_sigma2), hexf(kf.Rcam12), hexf(kf.tcam12)]
        for i in range(kf.n):
            lines.append("%s %d %s %d" % (hexf([kf.x[i], kf.y[i], kf.xd[i], kf.yd[i]]), kf.octave[i], hexf([kf.uright[i], kf.depth[i]]), kf.cam_of[i]))
    lines += ["%d %d" % (a, b) for a, b in pairs]
    path.write_text("\n".join(lines) + "\n")


def run_class(tmp_path, w, pairs):
    """-> (records as the class returned them, the world with the centres and Twc the class read from its stand-in keyframes)"""
    f = tmp_path / "world.txt"
    write_world(f, w, pairs)
    p = subprocess.run(["timeout", "-k", "10", "120", DRIVER, str(f)], capture_output=True, text=True, timeout=150)
    assert p.returncode == 0, p.stderr[-2000:]
    out = p.stdout.splitlines()
    seen = tw.World(w.kf1, w.kf2, pairs, cam_enabled=tuple(w.cam_enabled))
    seen.kf1, seen.kf2 = [tw.KF.__new__(tw.KF) for _ in range(2)]
    for kf, src, line in ((seen.kf1, w.kf1, out[0]), (seen.kf2, w.kf2, out[1])):
        kf.__dict__.update(src.__dict__)
        v = np.array([int(t, 16) for t in line.split()[1:]], np.uint32).view(np.float32)
        # the stand-in KeyFrame derives its centres and Twc from Tcw in float (the reference's SetPose does the same); the model takes them
        kf.centre = v[:6].reshape(2, 3).copy(); kf.Twc = v[6:].reshape(3, 4).copy()
        assert np.abs(kf.centre - src.centre).max() < 1e-5 and np.abs(kf.Twc - src.Twc).max() < 1e-5
    rec = np.zeros(len(pairs), tm.RECORD)
    has_point = np.zeros(len(pairs), bool)
    for i, line in enumerate(out[2:]):
        t = line.split()
        rec["outcome"][i] = int(t[0])
        assert int(t[1]) == (int(t[0]) == tm.ACCEPTED)
        if t[2] != "-":
            has_point[i] = True
            rec["x3D"][i] = np.array([int(x, 16) for x in t[2:5]], np.uint32).view(np.float32)
    return rec, has_point, seen


def compare(tmp_path, name, n):
    w, _ = tw.world_and_model(name)
    pairs = w.pairs[:n]
    rec, has_point, seen = run_class(tmp_path, w, pairs)
    want = seen.model(pairs)
    assert np.array_equal(rec["outcome"], want["outcome"])
    assert np.array_equal(has_point, want["path"] != tm.PATH_NONE)
    assert rec["x3D"].tobytes() == want["x3D"].tobytes()
    return want


def test_class_on_a_small_batch_takes_the_host_routine(tmp_path):
    want = compare(tmp_path, "5cm", 15)
    assert (want["outcome"] == tm.ACCEPTED).sum() >= 5 and len(set(want["path"])) >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(tw.WORLDS))
def test_class_on_the_generated_worlds(tmp_path, name):
    import torch  # noqa: F401
    want = compare(tmp_path, name, tw.N_PAIRS)
    assert (want["outcome"] == tm.ACCEPTED).sum() > 2000
