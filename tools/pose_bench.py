#!/usr/bin/env python3
"""Timings of the pose optimisation on the device (orbm_pose_optimize, orbm_pose_optimize_resident) next to the library's own host
routine for the same job (orbm_pose_optimize_host in the device's order: the same statements, one edge after the other on one CPU
core), same problems, same box, same run.  The host routine is NOT g2o: the reference's own cost per call (a heap-built graph, one
`new` per edge and per robust kernel) has never been measured in this project, g2o cannot be built here.  Informational: bench.py's
contract is untouched.

    python tools/pose_bench.py [--out profiles/r10/pose_bench.json]   all legs, alternated five times

Problems: mixed mono / stereo worlds of tests/pose_worlds.py (10 % outliers, start 5 cm / 2 degrees off), 50 .. 8 000 edges, two cameras,
all-cameras mode.  Legs, per size:
  a   orbm_pose_optimize, batch 1       (edges through the staging buffer, one launch of one workgroup, one synchronisation)
  b   orbm_pose_optimize_host, batch 1
  a8  orbm_pose_optimize, batch 8       (eight problems of that size, eight workgroups, one synchronisation)
  b8  orbm_pose_optimize_host, batch 8
  r   orbm_pose_optimize_resident       (the same edges read from a resident frame and a resident point table: 4 bytes per edge go up)
Every call is synchronised inside the timed window (the entry points return when the results are on the host).  Every leg goes through
ctypes with every argument prepared beforehand.  The size below which b wins is where host/Optimizer.cc (POSE_HOST_BELOW) switches."""
import argparse
import ctypes as C
import json
import os
import sys
import time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402,F401  (first: torch ships its own HIP runtime)
import multi_orb_slam_amd as m  # noqa: E402
from multi_orb_slam_amd import _lib  # noqa: E402
from multi_orb_slam_amd import matcher as mm  # noqa: E402
import pose_model as pm  # noqa: E402
import pose_worlds as pw  # noqa: E402

SIZES = (50, 100, 200, 400, 800, 1600, 3200, 8000)


def leg(fn, seconds):
    n, t0 = 0, time.perf_counter()
    while True:
        fn(); n += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n * 1e6


def spread(v):
    return {"median_us": round(float(np.median(v)), 2), "min_us": round(float(min(v)), 2), "max_us": round(float(max(v)), 2), "runs": len(v)}


class Legs:
    def __init__(self, mt, worlds):
        self.L = _lib.lib(); self.mt = mt
        probs = [pw.to_problem(m, P) for P in worlds]
        self.B = len(probs)
        self.recs, self.first, self.feat, self.pos, self.obs, self.octave = mm._pose_pack(probs)
        ne = int(self.first[-1])
        self.flags_a = np.zeros(max(ne, 1), np.uint8); self.flags_b = np.zeros(max(ne, 1), np.uint8)
        self.res_a = np.zeros(self.B, m.POSE_RESULT_DTYPE); self.res_b = np.zeros(self.B, m.POSE_RESULT_DTYPE)
        self.args = [_lib.ptr(x) for x in (self.first, self.feat, self.pos, self.obs, self.octave)]

    def a(self):
        _lib.check(self.L.orbm_pose_optimize(self.mt._h, _lib.ptr(self.recs), self.B, *self.args, _lib.ptr(self.flags_a), _lib.ptr(self.res_a)))

    def b(self):
        _lib.check(self.L.orbm_pose_optimize_host(_lib.ptr(self.recs), self.B, *self.args, m.POSE_ORDER_DEVICE, _lib.ptr(self.flags_b),
                                                  _lib.ptr(self.res_b)))


class ResidentLeg:
    """The world as a resident frame (one feature per edge) and a resident point table (one row per edge)."""

    def __init__(self, mt, P):
        self.L = _lib.lib(); self.mt = mt
        n = len(P["feat"]); n0 = int(P["n_cam0"])
        rng = np.random.default_rng(1)
        descs = [rng.integers(0, 256, (n0, 32), dtype=np.uint8), rng.integers(0, 256, (n - n0, 32), dtype=np.uint8)]
        cam_of = (np.arange(n) >= n0).astype(np.int32)
        local_of = np.where(cam_of == 0, np.arange(n), np.arange(n) - n0).astype(np.int32)
        # (positions clipped into the image bounds the grid is built for; the optimisation reads them as they are)
        fd = m.FrameData(np.clip(P["obs"][:, 0], 0, pw.W - 1).astype(np.float32), np.clip(P["obs"][:, 1], 0, pw.H - 1).astype(np.float32),
                         P["octave"], np.zeros(n, np.float32), P["obs"][:, 2].copy(), cam_of, local_of, descs, (0.0, 0.0, float(pw.W), float(pw.H)))
        self.F = mt.frame(fd)
        self.pts = m.LocalPoints(mt, n)
        rows = np.zeros(n, m.POINT_DTYPE); rows["pos"] = P["pos"]
        self.pts.write(0, rows)
        Q = dict(P)
        Q["obs"] = np.stack([fd.un_x, fd.un_y, P["obs"][:, 2]], axis=1)
        self.world = Q
        self.prob = pw.to_problem(m, Q)
        self.pof = np.arange(n, dtype=np.int32)
        self.flags = np.zeros(n, np.uint8); self.res = np.zeros(1, m.POSE_RESULT_DTYPE)

    def r(self):
        _lib.check(self.L.orbm_pose_optimize_resident(self.mt._h, _lib.ptr(self.prob.rec), self.F._h, self.pts._h, _lib.ptr(self.pof),
                                                      _lib.ptr(self.flags), _lib.ptr(self.res)))

    def close(self):
        self.pts.close(); self.F.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    results = []
    mt = m.Matcher()
    for n in SIZES:
        worlds = [pw.generate(seed=700 + n + k, n=n, kind="mixed", outliers=0.1, start=(0.05, 2.0), two_cams=True) for k in range(8)]
        one, eight, res = Legs(mt, worlds[:1]), Legs(mt, worlds), ResidentLeg(mt, worlds[0])
        legs = {"a": one.a, "b": one.b, "a8": eight.a, "b8": eight.b, "r": res.r}
        for fn in legs.values():
            fn()
        for lg in (one, eight):                                         # the two sides do the same job
            assert lg.res_a.tobytes() == lg.res_b.tobytes() and np.array_equal(lg.flags_a, lg.flags_b), n
        (hrec, hflags), = m.pose_optimize_host([res.prob], order=m.POSE_ORDER_DEVICE)
        assert res.res[0].tobytes() == hrec.tobytes() and np.array_equal(res.flags, hflags), n
        for _ in range(3):                                              # warm-up: buffers grown, clocks up
            for fn in legs.values():
                fn()
        t = {k: [] for k in legs}
        for _ in range(a.runs):                                         # alternated in one process
            for k, fn in legs.items():
                t[k].append(leg(fn, a.seconds))
        rec = one.res_a[0]
        results.append({"edges": n, "inliers": int(rec["n_inliers"]), "iterations": [int(x) for x in rec["round"]["iterations"]],
                        "trials": [int(x) for x in rec["round"]["trials"]],
                        "a_device_batch1": spread(t["a"]), "b_host_batch1": spread(t["b"]), "a8_device_batch8": spread(t["a8"]),
                        "b8_host_batch8": spread(t["b8"]), "r_device_resident": spread(t["r"]),
                        "b_over_a": round(float(np.median(t["b"]) / np.median(t["a"])), 3),
                        "b8_over_a8": round(float(np.median(t["b8"]) / np.median(t["a8"])), 3)})
        res.close()
    mt.close()
    for row in results:
        print(json.dumps(row))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
