#!/usr/bin/env python3
"""Timings of the local bundle adjustment on the device (orbm_local_ba) next to the library's own host routine for the same job
(orbm_local_ba_host in DEVICE order: the same statements on one CPU core), same problems, same box, same run.  The host routine is NOT
g2o (a graph on the heap per call, a sparse Cholesky behind an ordering), whose cost has never been measured in this project: g2o cannot
be built here.  Every figure this tool prints compares the device with THIS LIBRARY'S host routine and nothing else.  Informational:
bench.py's contract is untouched.

    python tools/local_ba_bench.py [--out profiles/r20/local_ba_bench.json]   all legs, alternated

Problems: worlds of tests/lba_worlds.py (10 % wrong observations, noise, a start 5 cm / 2 degrees off, mixed mono / stereo, both
cameras), 5 / 15 / 40 / 64 free keyframes (as many fixed ones up to 40) with 500 to 20 000 points, up to 8 observations per point.
Legs, per world:
  a   orbm_local_ba        (staging, the kernel chains, one synchronisation per Levenberg trial)
  b   orbm_local_ba_host
Every call is synchronised inside the timed window (the entry points return when the results are on the host), no stop function.
Every leg goes through ctypes with every argument prepared beforehand.  The number of edges where b stops winning is where
host/LocalBA.cc (LBA_HOST_BELOW) switches."""
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
import lba_worlds as lw  # noqa: E402

WORLDS = ((5, 5, 500), (5, 5, 2000), (15, 15, 2000), (15, 15, 5000), (40, 40, 5000), (40, 40, 20000), (64, 40, 5000), (64, 40, 20000))


def spread(v):
    return {"median_ms": round(float(np.median(v)) * 1e3, 3), "min_ms": round(float(min(v)) * 1e3, 3), "max_ms": round(float(max(v)) * 1e3, 3),
            "runs": len(v)}


class Legs:
    def __init__(self, mt, W):
        self.L = _lib.lib(); self.mt = mt
        self.prob = lw.to_problem(m, W)
        self.P = self.prob.native()
        self.res_a, self.res_b = m.LocalBAResult(self.prob), m.LocalBAResult(self.prob)
        self.Ra, self.Rb = self.res_a.native(), self.res_b.native()
        self.no_stop = _lib.LBA_STOP_FN()

    def a(self):
        _lib.check(self.L.orbm_local_ba(self.mt._h, C.byref(self.P), self.no_stop, None, C.byref(self.Ra)))

    def b(self):
        _lib.check(self.L.orbm_local_ba_host(C.byref(self.P), self.no_stop, None, m.POSE_ORDER_DEVICE, C.byref(self.Rb)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--worlds", type=int, default=len(WORLDS))
    a = ap.parse_args()
    results = []
    mt = m.Matcher()
    for f, x, n in WORLDS[:a.worlds]:
        W = lw.make_world(f, x, n, 700 + f + n, "mixed", 0.1, "off", 8)
        lg = Legs(mt, W)
        legs = {"a": lg.a, "b": lg.b}
        for fn in legs.values():
            fn()
        ra, rb = lg.res_a.take(lg.Ra), lg.res_b.take(lg.Rb)
        assert ra.same_bytes(rb) is None, (f, x, n, ra.same_bytes(rb))   # the two sides do the same job
        last = mt.last_local_ba()
        lg.a()                                                          # warm-up: buffers grown, clocks up
        t = {k: [] for k in legs}
        for _ in range(a.runs):                                         # alternated in one process, one call per sample
            for k, fn in legs.items():
                t0 = time.perf_counter(); fn(); t[k].append(time.perf_counter() - t0)
        results.append({"free": f, "fixed": x, "points": n, "edges": lg.prob.n_edges, "iterations": ra.rounds["iterations"].tolist(),
                        "trials": ra.rounds["trials"].tolist(), "kernel_launches": last[1], "synchronisations": last[2],
                        "a_device": spread(t["a"]), "b_host": spread(t["b"]),
                        "b_over_a": round(float(np.median(t["b"]) / np.median(t["a"])), 3),
                        "compared_with": "this library's host routine (orbm_local_ba_host, DEVICE order), not g2o"})
        print(json.dumps(results[-1]), flush=True)
    mt.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
