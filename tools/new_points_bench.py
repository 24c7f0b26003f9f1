#!/usr/bin/env python3
"""What one enqueue for all neighbours of a keyframe saves: orbv_create_new_points_keyframe next to the loop it replaces, one
orbv_create_new_points_resident per neighbour with the flags of the current keyframe updated on the host between two of them (one
synchronisation, one flag upload and one pass over the records per neighbour).  The loop stays in the library; both legs run in one
process, alternated, on the same resident keyframes.  Informational: bench.py's contract is untouched.

    python tools/new_points_bench.py [--out profiles/r19/new_points_bench.json]

Worlds: tests/new_points_worlds.py at 2 000 features x 15 neighbours (the reference's nn = 15) and at 600 x 5.  Both legs go through
ctypes with every argument prepared beforehand; the loop's flag update is three NumPy operations per neighbour inside the timed region,
because that is part of the sequence.  Every call of either leg synchronises before it returns, inside the timed window.  Before any
timing the two legs must return the same bytes."""
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
import new_points_worlds as nw  # noqa: E402

SHAPES = ((2000, 15), (600, 5))


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
    def __init__(self, search, world):
        self.L = _lib.lib(); self.S = search; self.w = world
        n, K = world.n, world.K
        self.n, self.K = n, K

        def resident(side, kf):
            fv = m.FeatureVector(side["node_id"], side["node_start"], side["items"])
            k = search.keyframe(m.BowSide(side["desc"], side["angle"], fv, side["flags"], side["x"], side["y"], side["octave"], side["cam_of"]))
            k.set_geometry(kf.uright, kf.depth, kf.cos_stereo, kf.xd, kf.yd)
            return k
        self.KA = resident(world.side_a, world.kf_a)
        self.KB = [resident(b.side, b.kf) for b in world.nb]
        self.keep = [world.kf_a.native()] + [b.kf.native() for b in world.nb]
        self.R = (_lib.NewPointsRound * K)()
        self.flags_b = [np.ascontiguousarray(b.side["flags"]) for b in world.nb]
        for k, b in enumerate(world.nb):
            T, kp = search._tri(b.F12, b.ex, b.ey, nw.SF, nw.S2)
            self.keep.append(kp)
            r = self.R[k]
            r.b = self.KB[k]._h; r.flags_b = self.flags_b[k].ctypes.data; r.t = T
            r.geometry.kf1, r.geometry.kf2 = self.keep[0].c(), self.keep[1 + k].c()
            r.geometry.cam_enabled[0], r.geometry.cam_enabled[1] = int(b.cam_enabled[0]), int(b.cam_enabled[1])
            r.geometry.ratio_factor = float(nw.RATIO)
        self.flags_a = np.ascontiguousarray(world.side_a["flags"])
        self.on = [b.cam_enabled[world.kf_a.cam_of].astype(np.uint8) for b in world.nb]
        self.keepbits = (self.flags_a & 0xFE).astype(np.uint8)
        self.match = [np.full((K, n), -1, np.int32) for _ in range(2)]
        self.out = [np.zeros((K, n), m.TRI_OUT_DTYPE) for _ in range(2)]
        self.nm = np.zeros(K, np.int32); self.acc = np.zeros(K, np.int32); self.acc1 = C.c_int()

    def chained(self):
        _lib.check(self.L.orbv_create_new_points_keyframe(self.S._h, self.KA._h, _lib.ptr(self.flags_a), self.R, self.K, 50, 1, _lib.ptr(self.match[0]),
                                                          _lib.ptr(self.out[0]), _lib.ptr(self.nm), _lib.ptr(self.acc)))

    def loop(self):
        free = self.flags_a & 1
        for k in range(self.K):
            r = self.R[k]
            fa = self.keepbits | (free & self.on[k])
            _lib.check(self.L.orbv_create_new_points_resident(self.S._h, self.KA._h, _lib.ptr(fa), r.b, r.flags_b, C.byref(r.t), C.byref(r.geometry), 50, 1,
                                                              self.match[1][k].ctypes.data, self.out[1][k].ctypes.data, C.byref(self.acc1)))
            free = free & (self.out[1][k]["outcome"] != 1)

    def close(self):
        for k in [self.KA] + self.KB:
            k.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    results = []
    S = m.BowSearch()
    for n, K in SHAPES:
        lg = Legs(S, nw.make_world(n, K))
        lg.chained(); lg.loop()
        assert np.array_equal(lg.match[0], lg.match[1]) and lg.out[0].tobytes() == lg.out[1].tobytes(), (n, K)   # the two legs do the same job
        call = S.last_keyframe_call
        lg.chained(); counts = call()
        for _ in range(5):                                              # warm-up of both: buffers grown, clocks up
            lg.chained(); lg.loop()
        t = {"chained": [], "loop": []}
        for _ in range(a.runs):                                         # alternated in one process
            for k in ("chained", "loop"):
                t[k].append(leg(getattr(lg, k), a.seconds))
        c, l = float(np.median(t["chained"])), float(np.median(t["loop"]))
        results.append({"features": n, "neighbours": K, "matches": lg.nm.tolist(), "accepted": lg.acc.tolist(),
                        "rounds_enqueued": counts[1], "kernel_launches": counts[2], "synchronisations": counts[3],
                        "chained_call": spread(t["chained"]), "loop_of_fused_calls": spread(t["loop"]),
                        "loop_minus_chained_us": round(l - c, 2), "per_neighbour_us": round((l - c) / K, 2), "loop_over_chained": round(l / c, 3)})
        lg.close()
    S.close()
    for row in results:
        print(json.dumps(row))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
