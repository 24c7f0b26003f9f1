#!/usr/bin/env python3
"""Timings of the local map on the device (orbm_map_vote, orbm_map_local_points, host/LocalMap.h) next to the host routines that do the
same job on plain arrays, same maps, same box, same run.  Informational: bench.py's contract is untouched.

    python tools/local_map_bench.py [--out profiles/r24/local_map_bench.json]   all legs, alternated five times

Maps: 200 and 2 000 keyframes of 2 000 features at five observations per point (keyframe k sees a window of 2 000 consecutive points
that moves on by 400 per keyframe: 80 000 / 800 000 points, 400 000 / 4 000 000 observation records), a frame of 2 000 features of
which 70 % hold a point of the newest keyframes' windows, and the local keyframes that follow from its votes (every keyframe with a
vote, then their neighbours in keyframe order up to 80).  The map is written once and stays unchanged between calls.  Legs, per map:
  a  orbm_map_vote                  (records in HBM; the frame's point slots in, the votes out)
  b  orbm_local_map_vote_host       (the same sum on the host over the same record slab)
  c  orbm_map_local_points          (rows in HBM; the local keyframes' slots in, the list out)
  d  orbm_local_map_points_host     (the same walk on the host over the same rows)
  e  UpdateLocalMap + SearchLocalPoints over a ResidentMap (host/LocalMap.h)             } host/test_local_map time: one process,
  f  the reference's UpdateLocalKeyFrames / UpdateLocalPoints transcribed + the existing } alternated, on the frustum worlds of
     SearchLocalPoints over a per-thread point table (what the parent commit ran)        } 2 000 and 8 000 points
a to d go through ctypes with every argument prepared beforehand; a and c end with the stream synchronised inside the call.  b and d
are NOT the reference's loops over std::map copies (leg f has those): they are this library's own host routines on flat arrays."""
import argparse
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

DRIVER = os.path.join(ROOT, "multi_orb_slam_amd", "host", "test_local_map")
SIZES = (200, 2000)
FEATURES, STEP, WORLD_CASES = 2000, 400, (1, 3)


class Legs:
    def __init__(self, n_kfs):
        rng = np.random.default_rng(n_kfs)
        self.n_kfs = n_kfs; self.n_points = n_points = STEP * (n_kfs - 1) + FEATURES
        rows = np.empty((n_kfs, FEATURES), np.int32)
        for k in range(n_kfs):
            rows[k] = STEP * k + rng.permutation(FEATURES)
        self.rows = rows; self.count = np.full(n_kfs, FEATURES, np.int32)
        self.flags = (rng.random(n_points) < 0.03).astype(np.uint8)
        obs = np.zeros(n_kfs * FEATURES, _lib.OBS_DTYPE)
        obs["point"] = rows.reshape(-1); obs["keyframe"] = np.repeat(np.arange(n_kfs, dtype=np.int32), FEATURES)
        self.obs = obs[rng.permutation(len(obs))]                      # (records lie in the slab in the order they were made, not by keyframe)
        newest = STEP * (n_kfs - 3)
        self.fp = np.where(rng.random(FEATURES) < 0.7, newest + rng.integers(0, FEATURES, FEATURES), -1).astype(np.int32)
        self.mt = m.Matcher(0.8, True)
        self.rm = rm = m.ResidentMap(self.mt, n_kfs, n_points, len(obs), FEATURES)
        rm.write_points(np.arange(n_points), np.zeros(n_points, m.POINT_DTYPE), self.flags)
        rm.write_observations(np.arange(len(obs)), self.obs)
        for k in range(n_kfs):
            rm.write_keyframe(k, rows[k])
        self.L = _lib.lib()
        self.votes = np.zeros(n_kfs, np.int32); self.votes_h = np.zeros(n_kfs, np.int32)
        self.list = np.zeros(m.MAX_POINTS, np.int32); self.list_h = np.zeros(m.MAX_POINTS, np.int32); self.nl = C.c_int()
        self.a()
        k1 = np.nonzero(self.votes > 0)[0]
        voted = set(k1.tolist())
        near = [k for k in range(n_kfs - 1, -1, -1) if k not in voted]
        self.local = np.concatenate([k1, near[:max(0, 80 - len(k1))]]).astype(np.int32)

    def a(self):
        _lib.check(self.L.orbm_map_vote(self.mt._h, self.rm._h, _lib.ptr(self.fp), len(self.fp), _lib.ptr(self.votes)))
        return self.votes

    def b(self):
        _lib.check(self.L.orbm_local_map_vote_host(_lib.ptr(self.obs), len(self.obs), _lib.ptr(self.flags), self.n_points, _lib.ptr(self.fp),
                                                   len(self.fp), self.n_kfs, _lib.ptr(self.votes_h)))
        return self.votes_h

    def c(self):
        _lib.check(self.L.orbm_map_local_points(self.mt._h, self.rm._h, _lib.ptr(self.local), len(self.local), _lib.ptr(self.list), C.byref(self.nl)))
        return self.list[:self.nl.value]

    def d(self):
        _lib.check(self.L.orbm_local_map_points_host(_lib.ptr(self.rows), _lib.ptr(self.count), self.n_kfs, FEATURES, _lib.ptr(self.flags),
                                                     self.n_points, _lib.ptr(self.local), len(self.local), _lib.ptr(self.list_h), m.MAX_POINTS,
                                                     C.byref(self.nl)))
        return self.list_h[:self.nl.value]

    def close(self):
        self.rm.close(); self.mt.close()


def leg(fn, seconds):
    n, t0 = 0, time.perf_counter()
    while True:
        fn(); n += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n * 1e6


def spread(v):
    return {"median_us": round(float(np.median(v)), 2), "min_us": round(float(min(v)), 2), "max_us": round(float(max(v)), 2), "pairs": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--pairs", type=int, default=5)
    a = ap.parse_args()
    results = []
    for n_kfs in SIZES:
        lg = Legs(n_kfs)
        assert np.array_equal(lg.a(), lg.b()) and lg.votes.sum() > 0          # the two sides do the same job
        assert np.array_equal(lg.c(), lg.d()) and lg.nl.value > 0
        stats = lg.mt.last_local_map(lg.rm)
        t = {k: [] for k in "abcd"}
        for _ in range(a.pairs):                                               # alternated in one process
            for k in "abcd":
                t[k].append(leg(getattr(lg, k), a.seconds))
        results.append({"keyframes": n_kfs, "points": lg.n_points, "records": len(lg.obs), "frame_features": FEATURES,
                        "keyframes_voted": int((lg.votes > 0).sum()), "local_keyframes": len(lg.local), "candidates": stats[2], "points_kept": stats[3],
                        "a_map_vote": spread(t["a"]), "b_vote_host": spread(t["b"]), "c_map_local_points": spread(t["c"]),
                        "d_local_points_host": spread(t["d"])})
        lg.close()
    for case_index in WORLD_CASES:
        case = fw.CASES[case_index]
        w = fw.make_world(*case)
        n, N = case[0], case[1][0]
        rng = np.random.default_rng(case_index + 900)
        pre = list(zip(rng.permutation(N)[: N // 10].tolist(), rng.permutation(n)[: N // 10].tolist()))
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "world.bin")
            fw.write_driver_world(path, w, np.zeros(n, np.int32), pre)
            r = subprocess.run(["timeout", "-k", "10", "300", DRIVER, "time", path, str(a.seconds)], capture_output=True, text=True, timeout=330)
            if r.returncode != 0:
                raise SystemExit("test_local_map time failed (%d): %s" % (r.returncode, r.stderr[-1000:]))
        legs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
        e = [l["us_per_call"] for l in legs if l["leg"] == "resident_map_update_and_search"]
        f = [l["us_per_call"] for l in legs if l["leg"] == "reference_update_then_point_table_search"]
        results.append({"world_points": n, "frame_features": len(w["fr"]["un_x"]), "local_points": legs[0]["local_points"],
                        "in_view": legs[0]["in_view"], "matches": legs[0]["matches"],
                        "e_resident_map_update_and_search": spread(e), "f_reference_update_then_point_table_search": spread(f)})
    for row in results:
        print(json.dumps(row))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
