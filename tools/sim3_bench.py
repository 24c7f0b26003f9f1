#!/usr/bin/env python3
"""Timings of the Sim3 RANSAC on the device (orbm_sim3_ransac) next to the library's own host routine for the same job
(orbm_sim3_ransac_host in DEVICE order: the same statements, one hypothesis and one correspondence after the other on one CPU core),
same problems, same box, same run.  The host routine is NOT the reference's cv::Mat code (every vector its own matrix on the heap),
whose cost has never been measured in this project: OpenCV cannot be built here.  Informational: bench.py's contract is untouched.

    python tools/sim3_bench.py [--out profiles/r11/sim3_bench.json]   all legs, alternated five times

Problems: worlds of tests/sim3_worlds.py (30 % wrong correspondences, one pixel of noise, both cameras), N in {20, 100, 500, 2 000}
correspondences, B in {1, 4, 16} problems per call, 300 hypotheses each (N = 20, B = 1 also with 10, 30 and 100).  Legs, per (N, B):
  a   orbm_sim3_ransac        (staging, two kernels back to back, one synchronisation)
  b   orbm_sim3_ransac_host
Every call is synchronised inside the timed window (the entry points return when the results are on the host).  Every leg goes through
ctypes with every argument prepared beforehand.  hypotheses x correspondences where b stops winning is where host/Sim3Solver.cc
(SIM3_HOST_BELOW) switches."""
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
import sim3_worlds as sw  # noqa: E402

SIZES = (20, 100, 500, 2000)
BATCHES = (1, 4, 16)
HYPOTHESES = 300


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
    def __init__(self, mt, worlds, hypotheses=HYPOTHESES):
        self.L = _lib.lib(); self.mt = mt
        probs = [sw.to_problem(m, W, W["triples"][:hypotheses]) for W in worlds]
        self.B = len(probs)
        # (_sim3_pack returns ctypes pointers into arrays it made: keep the arrays alive by packing by hand)
        self.keep = []
        hold = lambda a: (self.keep.append(a), _lib.ptr(a))[1]
        cat = lambda name, dt, shape: np.ascontiguousarray(np.concatenate([getattr(p, name) for p in probs]).reshape(shape), dt)
        first = np.zeros(self.B + 1, np.int32); its = np.zeros(self.B + 1, np.int32)
        first[1:] = np.cumsum([p.n for p in probs]); its[1:] = np.cumsum([p.h for p in probs])
        self.args = [hold(np.concatenate([p.rec for p in probs])), self.B, hold(first), hold(cat("x3dc1", np.float32, (-1, 3))),
                     hold(cat("x3dc2", np.float32, (-1, 3))), hold(cat("cam1", np.int32, (-1,))), hold(cat("cam2", np.int32, (-1,))),
                     hold(cat("max_err1", np.float32, (-1,))), hold(cat("max_err2", np.float32, (-1,))), hold(its), hold(cat("triples", np.int32, (-1, 3)))]
        words = int(sum(p.h * p.w for p in probs))
        self.hyp_a = np.zeros(int(its[-1]), m.SIM3_HYP_DTYPE); self.hyp_b = np.zeros(int(its[-1]), m.SIM3_HYP_DTYPE)
        self.mask_a = np.zeros(words, np.uint64); self.mask_b = np.zeros(words, np.uint64)

    def a(self):
        _lib.check(self.L.orbm_sim3_ransac(self.mt._h, *self.args, _lib.ptr(self.hyp_a), _lib.ptr(self.mask_a)))

    def b(self):
        _lib.check(self.L.orbm_sim3_ransac_host(*self.args, m.SIM3_MATH_DEVICE, _lib.ptr(self.hyp_b), _lib.ptr(self.mask_b)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    results = []
    mt = m.Matcher()
    for n in SIZES:
        worlds = [sw.generate(900 + n + k, n, s=(0.7, 1.0, 1.4)[k % 3], wrong=0.3, noise=1.0, cams=(0.2, 0.2), H=HYPOTHESES) for k in range(max(BATCHES))]
        # (N = 20 also with fewer hypotheses, as a solver with few correspondences runs: where the host routine stops winning)
        for B, H in [(B, HYPOTHESES) for B in BATCHES] + ([(1, 10), (1, 30), (1, 100)] if n == SIZES[0] else []):
            lg = Legs(mt, worlds[:B], H)
            legs = {"a": lg.a, "b": lg.b}
            for fn in legs.values():
                fn()
            assert lg.hyp_a.tobytes() == lg.hyp_b.tobytes() and lg.mask_a.tobytes() == lg.mask_b.tobytes(), (n, B)   # the two sides do the same job
            for _ in range(3):                                          # warm-up: buffers grown, clocks up
                for fn in legs.values():
                    fn()
            t = {k: [] for k in legs}
            for _ in range(a.runs):                                     # alternated in one process
                for k, fn in legs.items():
                    t[k].append(leg(fn, a.seconds))
            results.append({"correspondences": n, "problems": B, "hypotheses": H, "work": n * B * H,
                            "best_inliers": int(lg.hyp_a["n_inliers"].max()), "a_device": spread(t["a"]), "b_host": spread(t["b"]),
                            "b_over_a": round(float(np.median(t["b"]) / np.median(t["a"])), 3)})
    mt.close()
    for row in results:
        print(json.dumps(row))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
