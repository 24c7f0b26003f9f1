#!/usr/bin/env python3
"""Timings of the essential graph on the device (orbm_essential_graph) next to the library's own host routine for the same job
(orbm_essential_graph_host in DEVICE order: the same statements on one CPU core, its system solved by the dense sequential LDL^T), same
problems, same box, same run.  The host routine is NOT g2o (a graph on the heap per call, a sparse Cholesky behind an ordering), whose
cost has never been measured in this project: g2o cannot be built here.  Every figure this tool prints compares the device with THIS
LIBRARY'S host routine and nothing else.  Informational: bench.py's contract is untouched.

    python tools/essential_graph_bench.py [--out profiles/r22/essential_graph_bench.json]   all legs, alternated

Problems: the rings of tests/eg_worlds.py (drifted odometry, loop edges from the truth, a free scale), 20 / 30 / 40 / 50 / 100 / 200 / 400 / 800
free keyframes at about 5 edges per keyframe, 25 points per keyframe, 20 iterations (LoopClosing::CorrectLoop's call).
Legs, per world:
  a   orbm_essential_graph        (staging, the kernel chains, one synchronisation per Levenberg trial, the points)
  b   orbm_essential_graph_host   only up to --host-max-free keyframes: its dense factorisation grows with the cube of the keyframes
Every call is synchronised inside the timed window (the entry points return when the results are on the host).  Every leg goes through
ctypes with every argument prepared beforehand.  The number of edges where b stops winning is where host/EssentialGraph.cc
(EG_HOST_BELOW) switches."""
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
import eg_worlds as ew  # noqa: E402

WORLDS = (20, 30, 40, 50, 100, 200, 400, 800)
ITERATIONS = 20


def spread(v):
    return {"median_ms": round(float(np.median(v)) * 1e3, 3), "min_ms": round(float(min(v)) * 1e3, 3), "max_ms": round(float(max(v)) * 1e3, 3),
            "runs": len(v)}


class Legs:
    def __init__(self, mt, W):
        self.L = _lib.lib(); self.mt = mt
        self.prob = ew.make_problem(m, W)
        self.P = self.prob.native()
        self.res_a, self.res_b = m.EssentialGraphResult(self.prob), m.EssentialGraphResult(self.prob)
        self.Ra, self.Rb = self.res_a.native(), self.res_b.native()

    def a(self):
        _lib.check(self.L.orbm_essential_graph(self.mt._h, C.byref(self.P), ITERATIONS, C.byref(self.Ra)))

    def b(self):
        _lib.check(self.L.orbm_essential_graph_host(C.byref(self.P), ITERATIONS, m.POSE_ORDER_DEVICE, C.byref(self.Rb)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--only", type=int, default=0, help="one world: this many free keyframes")
    ap.add_argument("--host-max-free", type=int, default=200)
    a = ap.parse_args()
    results = []
    mt = m.Matcher()
    for f in ([a.only] if a.only else WORLDS):
        W = ew.ring(f, 900 + f, n_points=25 * f, covis=3, doubles=f // 10)
        lg = Legs(mt, W)
        legs = {"a": lg.a}
        if f <= a.host_max_free:
            legs["b"] = lg.b
        for fn in legs.values():
            fn()
        ra = lg.res_a.take(lg.Ra)
        if "b" in legs:
            rb = lg.res_b.take(lg.Rb)
            assert ra.same_bytes(rb) is None, (f, ra.same_bytes(rb))        # the two sides do the same job
        last = mt.last_essential_graph()
        assert last[0] == 0
        lg.a()                                                          # warm-up: buffers grown, clocks up
        t = {k: [] for k in legs}
        for _ in range(a.runs):                                         # alternated in one process, one call per sample
            for k, fn in legs.items():
                t0 = time.perf_counter(); fn(); t[k].append(time.perf_counter() - t0)
        row = {"free": f, "points": 25 * f, "edges": lg.prob.n_edges, "rows": 7 * f, "iterations": int(ra.round["iterations"][0]),
               "trials": int(ra.round["trials"][0]), "kernel_launches": last[1], "synchronisations": last[2], "block_pairs_computed": last[4],
               "block_pairs_possible": last[5], "panels": last[6], "a_device": spread(t["a"]),
               "compared_with": "this library's host routine (orbm_essential_graph_host, DEVICE order), not g2o"}
        if "b" in legs:
            row["b_host"] = spread(t["b"]); row["b_over_a"] = round(float(np.median(t["b"]) / np.median(t["a"])), 3)
        else:
            row["b_host"] = None                                        # no host figure at this size (see --host-max-free)
        results.append(row)
        print(json.dumps(row), flush=True)
    mt.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
