#!/usr/bin/env python3
"""Timings of the PnP RANSAC on the device (orbm_pnp_ransac) next to the library's own host routine for the same job
(orbm_pnp_ransac_host: the same statements, one hypothesis after the other on one CPU core), same problems, same box, same run.  The
host routine is NOT the reference's PnPsolver (heap CvMats per iteration, OpenCV's SVDs), whose cost has never been measured in this
project: OpenCV cannot be built here.  Every figure this tool prints compares the device with THIS LIBRARY'S host routine and nothing
else.  Informational: bench.py's contract is untouched.

    python tools/pnp_bench.py [--out profiles/r15/pnp_bench.json]   all legs, alternated five times

Problems: worlds of tests/pnp_worlds.py (30 % wrong correspondences, one pixel of noise, every octave), N in {20, 50, 100, 200, 500,
2 000} correspondences, B in {1, 4, 16} problems per call, 300 hypotheses each; and 10 / 30 / 100 hypotheses at 20 correspondences, for
the crossing point.  Legs, per (N, B, H):
  a   orbm_pnp_ransac        (staging, four kernels, one synchronisation, the copy back)
  b   orbm_pnp_ransac_host
Every call is synchronised inside the timed window (the entry points return when the results are on the host).  Every leg goes through
ctypes with every argument prepared beforehand."""
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
from multi_orb_slam_amd.matcher import _pnp_pack  # noqa: E402
import pnp_worlds as pw  # noqa: E402

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
    def __init__(self, mt, worlds, H):
        self.L = _lib.lib(); self.mt = mt
        self.probs = [pw.problem(m, W, quads=W["quads"][:H]) for W in worlds]
        self.args_a, self.out_a = _pnp_pack(self.probs)   # (the arrays behind the pointers are kept alive by the tuples)
        self.args_b, self.out_b = _pnp_pack(self.probs)
        self.keep = []

    def a(self):
        _lib.check(self.L.orbm_pnp_ransac(self.mt._h, *self.args_a))

    def b(self):
        _lib.check(self.L.orbm_pnp_ransac_host(*self.args_b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    results = []
    mt = m.Matcher()
    plan = [(n, B, 300) for n in SIZES for B in BATCHES] + [(20, 1, H) for H in (10, 30, 100)]
    for n, B, H in plan:
        worlds = [pw.world(n, 0.3, 1.0, seed=900 + n + k, H=H) for k in range(B)]
        lg = Legs(mt, worlds, H)
        legs = {"a": lg.a, "b": lg.b}
        for fn in legs.values():
            fn()
        for x, y in zip(lg.out_a[1:], lg.out_b[1:]):                # the two sides do the same job
            assert x.tobytes() == y.tobytes(), (n, B, H)
        for _ in range(3):                                          # warm-up: buffers grown, clocks up
            for fn in legs.values():
                fn()
        t = {k: [] for k in legs}
        for _ in range(a.runs):                                     # alternated in one process
            for k, fn in legs.items():
                t[k].append(leg(fn, a.seconds))
        results.append({"correspondences": n, "problems": B, "hypotheses": H, "records": [int(v) for v in lg.out_a[3]][:4],
                        "a_device": spread(t["a"]), "b_host": spread(t["b"]), "b_over_a": round(float(np.median(t["b"]) / np.median(t["a"])), 3),
                        "compared_with": "this library's host routine (orbm_pnp_ransac_host), not the reference's PnPsolver"})
    mt.close()
    for row in results:
        print(json.dumps(row))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
