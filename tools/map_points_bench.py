#!/usr/bin/env python3
"""Timings of the map-point refresh on the device (orbm_refresh_points, host/MapPointRefresh.h) next to the library's own host
routine for the same job (orbm_refresh_points_host: the same statements, one point after the other on one CPU core), same
batches, same box, same run.  Informational: bench.py's contract is untouched.

    python tools/map_points_bench.py [--out profiles/r08/map_points_bench.json]   all legs, alternated five times
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o mp -- python tools/map_points_bench.py --trace-plan
                                                                      only the device calls, for a kernel trace
    python tools/map_points_bench.py --kernel-trace DIR/.../mp_kernel_trace.csv [--trace-only] --out ...   adds the kernels' own times

Batches: tests/mappoint_worlds.py -- the generated worlds of the GPU test (500, 4 000 and 20 000 points; a new keyframe brings
1 000 - 2 000), a 2 000-point world, and batches of 1, 16 and 128 ordinary points cut from it (rows behind the forced ones).  Legs, per batch:
  a  orbm_refresh_points        (pack into the staging block, up to three launches, one synchronisation, records copied out)
  b  orbm_refresh_points_host
  c  RefreshMapPoints (host/MapPointRefresh.h)                                        } host/test_refresh time: one process, alternated,
  d  ComputeDistinctiveDescriptors + UpdateNormalAndDepth per point on cv::Mat types  } on a map of its own (1 500 points)
a and b go through ctypes with every argument prepared beforehand; a ends with the stream synchronised.  The batch size below
which b wins is where host/MapPointRefresh.cc (REFRESH_HOST_BELOW) switches."""
import argparse
import csv
import ctypes as C
import json
import os
import subprocess
import sys
import time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import multi_orb_slam_amd as m  # noqa: E402
from multi_orb_slam_amd import _lib  # noqa: E402
import mappoint_worlds as mw  # noqa: E402

DRIVER = os.path.join(ROOT, "multi_orb_slam_amd", "host", "test_refresh")
SMALL = (1, 2, 4, 8, 16, 32, 64, 128)
WORLDS = (500, 2000, 4000, 20000)
TRACE_REPS = 40


def batches():
    base, _ = mw.make_world(2000, 2000)
    out = [("cut_%d" % n, base.subset(np.arange(32, 32 + n))) for n in SMALL]
    for n in WORLDS:
        out.append(("world_%d" % n, base if n == 2000 else mw.make_world(n, n)[0]))
    return out


class Legs:
    def __init__(self, mt, batch):
        self.mt = mt; self.nb = batch.native()
        self.out_a = np.zeros(max(batch.n_points, 1), _lib.REFRESH_DTYPE); self.out_b = np.zeros(max(batch.n_points, 1), _lib.REFRESH_DTYPE)
        self.L = _lib.lib()

    def a(self):
        _lib.check(self.L.orbm_refresh_points(self.mt._h, C.byref(self.nb.c), _lib.ptr(self.out_a)))

    def b(self):
        _lib.check(self.L.orbm_refresh_points_host(C.byref(self.nb.c), _lib.ptr(self.out_b)))


def leg(fn, seconds):
    n, t0 = 0, time.perf_counter()
    while True:
        fn(); n += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n * 1e6


def spread(v):
    return {"median_us": round(float(np.median(v)), 2), "min_us": round(float(min(v)), 2), "max_us": round(float(max(v)), 2), "pairs": len(v)}


def read_trace(path):
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"].split("(")[0]
            grid = r.get("Grid_Size") or r.get("Grid_Size_X") or "?"
            rows.setdefault((name, grid), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return [{"kernel": name, "grid": grid, "dispatches": len(v), "median_us": round(float(np.median(v)), 2)}
            for (name, grid), v in sorted(rows.items()) if "k_refresh" in name]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--trace-plan", action="store_true")
    ap.add_argument("--kernel-trace")
    ap.add_argument("--trace-only", action="store_true", help="with --kernel-trace: only summarise the trace (no device needed)")
    ap.add_argument("--seconds", type=float, default=0.4)
    ap.add_argument("--pairs", type=int, default=5)
    a = ap.parse_args()
    results = []
    if not a.trace_only:
        mt = m.Matcher(0.6, True)
        for name, batch in batches():
            lg = Legs(mt, batch)
            lg.a(); lg.b()
            assert lg.out_a.tobytes() == lg.out_b.tobytes(), name          # the two sides do the same job
            if a.trace_plan:
                if name.startswith("world"):
                    for _ in range(TRACE_REPS):
                        lg.a()
                continue
            t = {"a": [], "b": []}
            for _ in range(a.pairs):                                       # alternated in one process
                for k in ("a", "b"):
                    t[k].append(leg(getattr(lg, k), a.seconds))
            results.append({"batch": name, "points": batch.n_points, "observations": batch.n_obs, "paths": list(mt.last_refresh()),
                            "a_refresh_points_device": spread(t["a"]), "b_refresh_points_host": spread(t["b"]),
                            "b_over_a": round(float(np.median(t["b"]) / np.median(t["a"])), 3)})
        mt.close()
        if a.trace_plan:
            return
        r = subprocess.run(["timeout", "-k", "10", "300", DRIVER, "time", "1500", str(a.seconds)], capture_output=True, text=True, timeout=330)
        if r.returncode != 0:
            raise SystemExit("test_refresh time failed (%d): %s" % (r.returncode, r.stderr[-1000:]))
        legs = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
        c = [x["us_per_call"] for x in legs if x["leg"] == "class"]; d = [x["us_per_call"] for x in legs if x["leg"] == "per_point"]
        results.append({"batch": "class_map_1500", "points": 1500, "c_class_refresh_map_points": spread(c),
                        "d_per_point_on_cv_mat_types": spread(d), "d_over_c": round(float(np.median(d) / np.median(c)), 3)})
    if a.kernel_trace:
        results.append({"kernel_trace": read_trace(a.kernel_trace)})
    for row in results:
        print(json.dumps(row))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
