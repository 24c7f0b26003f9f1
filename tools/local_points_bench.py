#!/usr/bin/env python3
"""Timings of local-map tracking on the device (orbm_search_local_points, host/LocalMapSearch.h) next to what the library offered
before it for the same job, same worlds, same box, same run.  Informational: bench.py's contract is untouched.

    python tools/local_points_bench.py [--out profiles/r08/local_points_bench.json]   all legs, alternated five times
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o lp -- python tools/local_points_bench.py --trace-plan
                                                                      only the device calls, for a kernel trace
    python tools/local_points_bench.py --kernel-trace DIR/.../lp_kernel_trace.csv [--trace-only] --out ...   adds the kernels' own times

Worlds: tests/frustum_worlds.py, 2 000 and 8 000 points against a frame of [1000, 500] features, th = 3; the point table is
written once and stays unchanged between calls.  Legs, per world:
  a  orbm_search_local_points                                    (table in HBM; pose, skip and occupied flags in)
  b  orbm_frustum_host + compaction + orbm_search_by_projection_points   (what a caller had to do before: frustum test per point
     on the host -- here already the library's scalar restatement, not cv::Mat algebra, with the level thresholds built once
     before the timed region -- the visible points' queries compacted into a preallocated buffer, one 68-byte query per visible
     point through the staging block)
  e  orbm_search_by_projection_points alone, fed with the ready-made queries of b (the search without any frustum work)
  c  SearchLocalPoints (host/LocalMapSearch.h)                   } host/test_local_points time: one process,
  d  Frame::isInFrustum per point + ORBmatcher::SearchByProjection } alternated
a, b and e go through ctypes with every argument prepared beforehand; each call ends with the stream synchronised."""
import argparse
import csv
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import multi_orb_slam_amd as m  # noqa: E402
from multi_orb_slam_amd import _lib  # noqa: E402
import frustum_worlds as fw  # noqa: E402

DRIVER = os.path.join(ROOT, "multi_orb_slam_amd", "host", "test_local_points")
SIZES = (2000, 8000)
TRACE_REPS = 40


class Legs:
    def __init__(self, npts):
        self.w = w = fw.make_world(npts, [1000, 500], 640, 480, npts, 3.0)
        self.mt = m.Matcher(0.8, True)
        self.F = self.mt.frame(m.FrameData(**w["fr"]))
        self.pts = m.LocalPoints(self.mt, npts)
        self.pts.write(0, w["points"])
        self.view = w["view"].native()
        self.n = npts; nf = self.F.data.n_total
        self.points = np.ascontiguousarray(w["points"])
        self.mo = np.zeros(nf, np.int32); self.track = np.zeros(npts, _lib.TRACK_DTYPE); self.q = np.zeros(npts, _lib.QUERY_DTYPE)
        self.ntm = C.c_int(); self.nm = C.c_int()
        self.L = _lib.lib()
        self.mask = np.zeros(npts, bool); self.ready_buf = np.zeros(npts, _lib.QUERY_DTYPE); self.ready = self.ready_buf[:0]
        self.b()                                   # (builds the level thresholds orbm_frustum_host keeps per thread; leaves the queries for e)

    def a(self):
        _lib.check(self.L.orbm_search_local_points(self.mt._h, self.F._h, self.pts._h, self.n, C.byref(self.view.c), None, None, 0.8, 100,
                                                   _lib.ptr(self.track), _lib.ptr(self.mo), C.byref(self.ntm), C.byref(self.nm)))
        return self.ntm.value, self.nm.value

    def b(self):
        _lib.check(self.L.orbm_frustum_host(_lib.ptr(self.points), self.n, C.byref(self.view.c), None, _lib.ptr(self.track), _lib.ptr(self.q),
                                            C.byref(self.ntm)))
        np.not_equal(self.track["in_view"], 0, out=self.mask)          # compaction into a buffer allocated once
        self.ready = self.ready_buf[:self.ntm.value]
        np.compress(self.mask, self.q, out=self.ready)
        return self.ntm.value, self.e()[1]

    def e(self):
        _lib.check(self.L.orbm_search_by_projection_points(self.mt._h, self.F._h, _lib.ptr(self.ready), len(self.ready), None, 0.8, 100,
                                                           _lib.ptr(self.mo), C.byref(self.nm)))
        return len(self.ready), self.nm.value

    def close(self):
        self.pts.close(); self.F.close(); self.mt.close()


def leg(fn, seconds):
    n, t0 = 0, time.perf_counter()
    while True:
        fn(); n += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n * 1e6


def spread(v):
    return {"median_us": round(float(np.median(v)), 2), "min_us": round(float(min(v)), 2), "max_us": round(float(max(v)), 2), "pairs": len(v)}


def trace_plan():
    for npts in SIZES:
        lg = Legs(npts)
        for fn in (lg.a, lg.e):
            for _ in range(TRACE_REPS + 3):
                fn()
        lg.close()


def read_trace(path):
    """-> [{kernel, grid, dispatches, median_us}]: the kernels of the plan by name and grid size (k_project's grid tells the legs apart:
    one wave per table row in a, one per visible point in e)."""
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"].split("(")[0]
            grid = r.get("Grid_Size") or r.get("Grid_Size_X") or "?"
            rows.setdefault((name, grid), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = []
    for (name, grid), v in sorted(rows.items()):
        if any(k in name for k in ("k_frustum", "k_project", "k_resolve", "k_rs_")):
            out.append({"kernel": name, "grid": grid, "dispatches": len(v), "median_us": round(float(np.median(v)), 2)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--trace-plan", action="store_true")
    ap.add_argument("--kernel-trace")
    ap.add_argument("--trace-only", action="store_true", help="with --kernel-trace: only summarise the trace (no device needed)")
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--pairs", type=int, default=5)
    a = ap.parse_args()
    if a.trace_plan:
        trace_plan()
        return
    results = []
    for npts in (() if a.trace_only else SIZES):
        lg = Legs(npts)
        ra, rb = lg.a(), lg.b()
        assert ra == rb, (ra, rb)                      # the two sides do the same job
        t = {"a": [], "b": [], "e": []}
        for _ in range(a.pairs):                       # alternated in one process
            for k in ("a", "b", "e"):
                t[k].append(leg(getattr(lg, k), a.seconds))
        row = {"points": npts, "features": lg.F.data.n_total, "in_view": ra[0], "matches": ra[1], "resolve": list(lg.mt.last_resolve()),
               "a_search_local_points": spread(t["a"]), "b_host_frustum_plus_points_search": spread(t["b"]),
               "e_points_search_ready_queries": spread(t["e"]),
               "b_over_a": round(float(np.median(t["b"]) / np.median(t["a"])), 3),
               "frustum_share_of_a_against_e": round(float(1 - np.median(t["e"]) / np.median(t["a"])), 3)}
        lg.close()
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "world.bin")
            fw.write_driver_world(path, lg.w)
            r = subprocess.run(["timeout", "-k", "10", "300", DRIVER, "time", path, str(a.seconds)], capture_output=True, text=True, timeout=330)
            if r.returncode != 0:
                raise SystemExit("test_local_points time failed (%d): %s" % (r.returncode, r.stderr[-1000:]))
        legs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
        c = [l["us_per_call"] for l in legs if l["leg"] == "search_local_points"]
        d = [l["us_per_call"] for l in legs if l["leg"] == "host_frustum_then_search"]
        row["c_class_search_local_points"] = spread(c); row["d_class_isinfrustum_plus_search"] = spread(d)
        row["d_over_c"] = round(float(np.median(d) / np.median(c)), 3)
        results.append(row)
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
