"""Optimizer::OptimizeSim3_cam1 and OptimizeSim3Batch (host/Optimizer.h) through their driver host/test_sim3opt: stand-in keyframes and
map points built from the worlds of tests/sim3opt_worlds.py; the return value, g2oS12 and vpMatches1 against the library's host routine
in DEVICE order (what the device computes, bit for bit).  Below SIM3OPT_HOST_BELOW correspondences a single call takes the host routine
(no device needed); from there on, and for every batched call, the device."""
import os
import subprocess

import numpy as np
import pytest

import multi_orb_slam_amd as m
import pose_model as pm
import sim3opt_worlds as sw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "multi_orb_slam_amd", "host")
DRIVER = os.path.join(HOST, "test_sim3opt")
EYE = np.eye(4, dtype=np.float32)


def hexf(a):
    return " ".join("%08x" % v for v in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32))


def case_lines(W, extra):
    """The world as two keyframes at the identity pose (R*X + t of the class is then X, bit for bit) whose features with a matched map
    point are the world's correspondences; `extra`: entries of vpMatches1 the reference's filtering must drop, strewn between them:
    a null match, a null point in keyframe 1, a bad point on either side, a matched point keyframe 2 does not observe."""
    n = W["n"]
    kinds = ["ok"] * n
    for j, kind in enumerate(extra):
        kinds.insert(min(len(kinds), 3 * j + 1), kind)
    N = len(kinds)
    sig1, sig2 = W["inv_level_sigma2_1"], W["inv_level_sigma2_2"]
    lines = ["%s %d" % (hexf(W["th2"]), int(W["fix_scale"])), hexf(W["R"]), hexf(W["t"]), hexf(W["s"])]
    kf1 = [hexf(EYE), hexf(W["K1"]), "%d" % len(sig1), hexf(sig1), "%d" % N]
    kf2 = [hexf(EYE), hexf(W["K2"]), "%d" % len(sig2), hexf(sig2), "%d" % (n + 1)]
    entries, where = [], []
    e = 0
    for i, kind in enumerate(kinds):
        if kind == "ok":
            kf1.append("%s %d" % (hexf(W["obs1"][e]), W["octave1"][e]))
            entries.append("1 0 %s 1 0 %d %s" % (hexf(W["x3dc1"][e]), e, hexf(W["x3dc2"][e])))
            where.append(i)
            e += 1
        else:
            kf1.append("%s 0" % hexf([11.0, 12.0]))
            p = hexf([0.1, 0.2, 3.0])
            entries.append({"null_match": "1 0 %s 0 0 -1 %s", "null_point1": "0 0 %s 1 0 %d %s" % ("%s", n, "%s"), "bad1": "1 1 %s 1 0 %d %s" % ("%s", n, "%s"),
                            "bad2": "1 0 %s 1 1 %d %s" % ("%s", n, "%s"), "not_in_kf2": "1 0 %s 1 0 -1 %s"}[kind] % (p, p))
    for k in range(n):
        kf2.append("%s %d" % (hexf(W["obs2"][k]), W["octave2"][k]))
    kf2.append("%s 0" % hexf([13.0, 14.0]))
    return lines + kf1 + kf2 + ["%d" % N] + entries, where, kinds


def run_driver(tmp_path, worlds, extra=(), batch=False, driver=DRIVER, env=None):
    lines = ["%d" % len(worlds)]
    meta = []
    for W in worlds:
        ls, where, kinds = case_lines(W, extra)
        lines += ls
        meta.append((where, kinds))
    f = tmp_path / "cases.txt"
    f.write_text("\n".join(lines) + "\n")
    p = subprocess.run(["timeout", "-k", "10", "120", driver, str(f)] + (["batch"] if batch else []), capture_output=True, text=True, timeout=150, env=env)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    out = []
    for line in p.stdout.splitlines():
        t = line.split()
        out.append((int(t[0]), np.array([int(x, 16) for x in t[1:9]], np.uint64).view(np.float64), np.array([c == "1" for c in t[9]]) if t[9] != "-" else np.zeros(0, bool)))
    assert len(out) == len(worlds)
    return out, meta


def as_the_class_passes_it(W):
    """g2oS12 = g2o::Sim3(Matrix3d(R), Vector3d(t), s) from the float start; the class hands the library rotation().toRotationMatrix()
    rounded to float."""
    R = np.asarray(W["R"], np.float32).reshape(3, 3)
    q = pm.quat_from_matrix([[float(v) for v in row] for row in R])
    V = dict(W)
    V["R"] = np.array(pm.quat_to_matrix(q), np.float64).astype(np.float32).reshape(9)
    return V, q


def check(W, got, meta):
    ret, s12, matches = got
    where, kinds = meta
    V, q0 = as_the_class_passes_it(W)
    (rec, flags), = m.sim3_optimize_host([sw.to_problem(m, V)], m.POSE_ORDER_DEVICE)
    assert ret == rec["n_inliers"]
    want = np.array([k in ("ok", "null_point1", "bad1", "bad2", "not_in_kf2") for k in kinds])   # (only a null match is null beforehand)
    want[np.asarray(where, np.int64)[flags != 0]] = False
    assert np.array_equal(matches, want)
    if rec["written"]:
        assert s12.tobytes() == np.concatenate([rec["q"], rec["t"], [rec["s"]]]).tobytes()
    else:                                                            # g2oS12 as it came: the quaternion of the constructor, not a round trip
        assert list(s12[:4]) == q0 and list(s12[4:7]) == [float(v) for v in W["t"]] and s12[7] == float(W["s"])
    return rec


SMALL = ["zero", "survivors_9", "survivors_10", "survivors_11", "nine_clean", "some_bad", "branches_fixed"]
EXTRA = ("null_match", "null_point1", "bad1", "bad2", "not_in_kf2")


@pytest.mark.parametrize("name", SMALL)
def test_class_on_small_problems_takes_the_host_routine(tmp_path, name):
    W, expect = sw.exit_cases()[name]
    assert W["n"] < 450
    (got,), (meta,) = run_driver(tmp_path, [W], EXTRA)
    rec = check(W, got, meta)
    for k, v in expect.items():
        assert rec[k] == v, (name, k)


def test_class_under_the_sanitizers_on_the_host_path(tmp_path):
    """The stand-alone driver built with AddressSanitizer and UndefinedBehaviorSanitizer over Optimizer.cc, g2o_compat.h, cv_compat.h and
    itself (`make san`), on the problems that need no device: the same lines as the plain driver."""
    subprocess.check_call(["make", "-s", "-C", HOST, "test_sim3opt_san"], timeout=900)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    worlds = [sw.exit_cases()[n][0] for n in SMALL]
    plain, _ = run_driver(tmp_path, worlds, EXTRA)
    san, meta = run_driver(tmp_path, worlds, EXTRA, driver=DRIVER + "_san", env=env)
    for W, a, b, mt in zip(worlds, plain, san, meta):
        assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2])
        check(W, b, mt)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n600_fixed_wrong20_noise_off", "n1000_free10_noise_near", "n2000_free07_wrong20_noise", "n8192_fixed_noise"])
def test_class_on_the_device(tmp_path, name):
    import torch  # noqa: F401
    W = sw.world(name)
    assert W["n"] >= 450                                             # SIM3OPT_HOST_BELOW: below it a single call stays on the host
    (got,), (meta,) = run_driver(tmp_path, [W], EXTRA)
    rec = check(W, got, meta)
    assert rec["written"] == 1 and rec["n_inliers"] >= 20


@pytest.mark.gpu
@pytest.mark.parametrize("fix_scale", [False, True])
def test_batched_static_equals_the_single_calls(tmp_path, fix_scale):
    import torch  # noqa: F401
    worlds = sw.candidates(81, 120, 6, fix_scale)
    for W in worlds[1:]:                                             # (the batched static has ONE current keyframe)
        assert all(np.array_equal(W[k], worlds[0][k]) for k in ("x3dc1", "obs1", "octave1", "inv_level_sigma2_1")) and W["K1"] == worlds[0]["K1"]
    single, meta = run_driver(tmp_path, worlds, EXTRA, batch=False)
    batched, _ = run_driver(tmp_path, worlds, EXTRA, batch=True)
    for W, a, b, mt in zip(worlds, single, batched, meta):
        assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2])
        check(W, b, mt)
    assert any(a[0] >= 20 for a in batched)
