#!/usr/bin/env python3
"""Timings of the Sim3 refinement on the device (orbm_sim3_optimize) next to the library's own host routine for the same job
(orbm_sim3_optimize_host in DEVICE order: the same statements, one correspondence after the other on one CPU core), same problems, same
box, same run.  The host routine is NOT g2o (a graph on the heap per call, two edges and two robust kernels per correspondence, a
virtual call per numeric-Jacobian evaluation), whose cost has never been measured in this project: g2o cannot be built here.  Every
figure this tool prints compares the device with THIS LIBRARY'S host routine and nothing else.  Informational: bench.py's contract is
untouched.

    python tools/sim3opt_bench.py [--out profiles/r14/sim3opt_bench.json]   all legs, alternated five times

Problems: worlds of tests/sim3opt_worlds.py (20 % wrong correspondences, one pixel of noise, a start a little off, free scale), N in
{20, 50, 100, 200, 500, 2 000} correspondences, B in {1, 4, 16} problems per call.  Legs, per (N, B):
  a   orbm_sim3_optimize        (staging, one kernel, one synchronisation)
  b   orbm_sim3_optimize_host
Every call is synchronised inside the timed window (the entry points return when the results are on the host).  Every leg goes through
ctypes with every argument prepared beforehand.  The number of correspondences where b stops winning for a single problem is where
host/Optimizer.cc (SIM3OPT_HOST_BELOW) switches."""
import argparse
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
from multi_orb_slam_amd.matcher import _sim3opt_pack  # noqa: E402
import sim3opt_worlds as sw  # noqa: E402

SIZES = (20, 50, 100, 200, 500, 2000)
BATCHES = (1, 4, 16)


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
        probs = [sw.to_problem(m, W) for W in worlds]
        self.B = len(probs)
        self.recs, self.first, self.arrays, self.flags_a, self.res_a = _sim3opt_pack(probs)   # (kept alive here)
        self.flags_b, self.res_b = self.flags_a.copy(), self.res_a.copy()
        self.args = [_lib.ptr(self.recs), self.B, _lib.ptr(self.first)] + [_lib.ptr(a) for a in self.arrays]

    def a(self):
        _lib.check(self.L.orbm_sim3_optimize(self.mt._h, *self.args, _lib.ptr(self.flags_a), _lib.ptr(self.res_a)))

    def b(self):
        _lib.check(self.L.orbm_sim3_optimize_host(*self.args, m.POSE_ORDER_DEVICE, _lib.ptr(self.flags_b), _lib.ptr(self.res_b)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    results = []
    mt = m.Matcher()
    for n in SIZES:
        worlds = [sw.generate(900 + n + k, n, s=(0.7, 1.0, 1.4)[k % 3], wrong=0.2, noise=1.0, grade=2) for k in range(max(BATCHES))]
        for B in BATCHES:
            lg = Legs(mt, worlds[:B])
            legs = {"a": lg.a, "b": lg.b}
            for fn in legs.values():
                fn()
            assert lg.res_a.tobytes() == lg.res_b.tobytes() and lg.flags_a.tobytes() == lg.flags_b.tobytes(), (n, B)   # the two sides do the same job
            for _ in range(3):                                          # warm-up: buffers grown, clocks up
                for fn in legs.values():
                    fn()
            t = {k: [] for k in legs}
            for _ in range(a.runs):                                     # alternated in one process
                for k, fn in legs.items():
                    t[k].append(leg(fn, a.seconds))
            passes = int((lg.res_a["round"]["trials"] + lg.res_a["round"]["iterations"]).sum())
            results.append({"correspondences": n, "problems": B, "passes_over_the_edges": passes,
                            "inliers": [int(v) for v in lg.res_a["n_inliers"]][:4], "a_device": spread(t["a"]), "b_host": spread(t["b"]),
                            "b_over_a": round(float(np.median(t["b"]) / np.median(t["a"])), 3),
                            "compared_with": "this library's host routine (orbm_sim3_optimize_host, DEVICE order), not g2o"})
    mt.close()
    for row in results:
        print(json.dumps(row))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
