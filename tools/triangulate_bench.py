#!/usr/bin/env python3
"""Timings of the triangulation stage on the device (orbv_triangulate_pairs, orbv_create_new_points_resident) next to the library's own
host routine for the same job (orbv_triangulate_pairs_host: the same statements, one pair after the other on one CPU core), same
batches, same box, same run.  Informational: bench.py's contract is untouched.

    python tools/triangulate_bench.py [--out profiles/r09/triangulate_bench.json]   all legs, alternated five times

Batches: the pairs of the 25 cm world of tests/triangulate_worlds.py (two keyframes of 3 000 features), cut to 16 .. 3 000 pairs, and
a 4 000-pair world.  Legs, per batch:
  a  orbv_triangulate_pairs        (both keyframes' arrays and the pairs through the pinned stage, one launch, one synchronisation)
  b  orbv_triangulate_pairs_host
and on two synthetic keyframes of about 2 000 features (the ones of tests/test_gpu_triangulate.py):
  c  orbv_create_new_points_resident                                   (search + triangulation, one synchronisation)
  d  orbv_search_for_triangulation_resident, then orbv_triangulate_pairs_host on its pairs   (what a caller did before this stage existed)
Every leg goes through ctypes with every argument prepared beforehand (d builds its pair list from match[] with NumPy inside the timed
region: that is part of the sequence).  The batch size below which b wins is where host/NewMapPoints.cc (TRIANGULATE_HOST_BELOW)
switches; d minus c is the per-neighbour saving of the fused call."""
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
import triangulate_worlds as tw  # noqa: E402

SIZES = (16, 32, 64, 128, 256, 512, 1024, 2048, 3000, 4000)


def leg(fn, seconds):
    n, t0 = 0, time.perf_counter()
    while True:
        fn(); n += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n * 1e6


def spread(v):
    return {"median_us": round(float(np.median(v)), 2), "min_us": round(float(min(v)), 2), "max_us": round(float(max(v)), 2), "runs": len(v)}


class PairLegs:
    def __init__(self, search, world, n):
        self.L = _lib.lib(); self.S = search
        self.k1, self.k2 = world.kf1.native(), world.kf2.native()
        self.c1, self.c2 = self.k1.c(), self.k2.c()
        self.en = np.array([1, 1], np.uint8)
        self.pairs = np.ascontiguousarray(world.pairs[:n]); self.n = n
        self.ratio = float(world.ratio_factor)
        self.out_a = np.zeros(n, m.TRI_OUT_DTYPE); self.out_b = np.zeros(n, m.TRI_OUT_DTYPE)

    def a(self):
        _lib.check(self.L.orbv_triangulate_pairs(self.S._h, C.byref(self.c1), C.byref(self.c2), _lib.ptr(self.en), _lib.ptr(self.pairs), self.n,
                                                 self.ratio, _lib.ptr(self.out_a)))

    def b(self):
        _lib.check(self.L.orbv_triangulate_pairs_host(C.byref(self.c1), C.byref(self.c2), _lib.ptr(self.en), _lib.ptr(self.pairs), self.n,
                                                      self.ratio, _lib.ptr(self.out_b)))


class FusedLegs:
    def __init__(self, search):
        import test_gpu_triangulate as t
        self.L = _lib.lib(); self.S = search
        a, b, self.kf1, self.kf2 = t.synthetic_keyframes()
        self.KA, self.KB = search.keyframe(t.to_side(a)), search.keyframe(t.to_side(b))
        for K, kf in ((self.KA, self.kf1), (self.KB, self.kf2)):
            K.set_geometry(kf.uright, kf.depth, kf.cos_stereo, kf.xd, kf.yd)
        self.T, self.keep = search._tri(t.F12, t.EX, t.EY, t.SF, t.S2)
        self.k1, self.k2 = self.kf1.native(), self.kf2.native()
        self.c1, self.c2 = self.k1.c(), self.k2.c()
        self.G = _lib.TriGeometry(); self.G.kf1, self.G.kf2 = self.k1.c(), self.k2.c()
        self.G.cam_enabled[0] = self.G.cam_enabled[1] = 1
        self.G.ratio_factor = float(np.float32(1.5) * t.SF[1])
        self.en = np.array([1, 1], np.uint8)
        n = self.KA.n
        self.match_c = np.full(n, -1, np.int32); self.match_d = np.full(n, -1, np.int32)
        self.out_c = np.zeros(n, m.TRI_OUT_DTYPE); self.out_d = np.zeros(n, m.TRI_OUT_DTYPE)
        self.acc = C.c_int(); self.nm = C.c_int()
        self.pairs = 0

    def c(self):
        _lib.check(self.L.orbv_create_new_points_resident(self.S._h, self.KA._h, None, self.KB._h, None, C.byref(self.T), C.byref(self.G), 50, 1,
                                                          _lib.ptr(self.match_c), _lib.ptr(self.out_c), C.byref(self.acc)))

    def d(self):
        _lib.check(self.L.orbv_search_for_triangulation_resident(self.S._h, self.KA._h, None, self.KB._h, None, C.byref(self.T), 50, 1,
                                                                 _lib.ptr(self.match_d), C.byref(self.nm)))
        idx = np.flatnonzero(self.match_d >= 0).astype(np.int32)
        pairs = np.ascontiguousarray(np.stack([idx, self.match_d[idx]], 1))
        rec = np.zeros(max(len(idx), 1), m.TRI_OUT_DTYPE)
        _lib.check(self.L.orbv_triangulate_pairs_host(C.byref(self.c1), C.byref(self.c2), _lib.ptr(self.en), _lib.ptr(pairs), len(idx),
                                                      self.G.ratio_factor, _lib.ptr(rec)))
        self.out_d[:] = 0; self.out_d[idx] = rec[:len(idx)]
        self.pairs = len(idx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    results = []
    S = m.BowSearch()
    base = tw.make_world("25cm")
    big = tw.make_world("25cm", 4000)
    for n in SIZES:
        lg = PairLegs(S, big if n > len(base.pairs) else base, n)
        lg.a(); lg.b()
        assert lg.out_a.tobytes() == lg.out_b.tobytes(), n              # the two sides do the same job
        for _ in range(3):                                              # warm-up: buffers grown, clocks up
            lg.a(); lg.b()
        t = {"a": [], "b": []}
        for _ in range(a.runs):                                         # alternated in one process
            for k in ("a", "b"):
                t[k].append(leg(getattr(lg, k), a.seconds))
        results.append({"batch": "pairs_%d" % n, "pairs": n, "features": [lg.k1.n, lg.k2.n], "a_triangulate_pairs_device": spread(t["a"]),
                        "b_triangulate_pairs_host": spread(t["b"]), "b_over_a": round(float(np.median(t["b"]) / np.median(t["a"])), 3)})
    fl = FusedLegs(S)
    fl.c(); fl.d()
    assert np.array_equal(fl.match_c, fl.match_d) and fl.out_c.tobytes() == fl.out_d.tobytes()
    for _ in range(3):
        fl.c(); fl.d()
    t = {"c": [], "d": []}
    for _ in range(a.runs):
        for k in ("c", "d"):
            t[k].append(leg(getattr(fl, k), a.seconds))
    results.append({"batch": "fused_2000_features", "features": [fl.KA.n, fl.KB.n], "pairs": fl.pairs, "accepted": fl.acc.value,
                    "c_create_new_points_resident": spread(t["c"]), "d_search_then_host_routine": spread(t["d"]),
                    "d_minus_c_us": round(float(np.median(t["d"]) - np.median(t["c"])), 2)})
    fl.KA.close(); fl.KB.close(); S.close()
    for row in results:
        print(json.dumps(row))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
