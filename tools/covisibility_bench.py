#!/usr/bin/env python3
"""Timings of the covisibility and culling counts on the device (orbm_map_covisibility, orbm_map_culling_counts, host/Covisibility.h)
next to the host routines that do the same job on plain arrays, same maps, same box, same run.  Informational: bench.py's contract
is untouched.

    python tools/covisibility_bench.py [--out profiles/r25/covisibility_bench.json]   all legs, alternated five times

Maps: the two of tools/local_map_bench.py -- 200 and 2 000 keyframes of 2 000 features, keyframe k seeing a window of 2 000 consecutive
points that moves on by 400 per keyframe: 400 000 / 4 000 000 observation records, five observers per point -- with levels 0 to 3,
a tenth of the features far, 1 400 camera-1 features per keyframe and n_obs between the number of observers and twice it.  1, 20 and
100 keyframes per call, from the middle of the map.  Legs, per map and call size:
  a  orbm_map_covisibility              (index clean)          b  orbm_local_map_covisibility_host
  c  orbm_map_culling_counts            (index clean)          d  orbm_local_map_culling_host
  i  one record written again + orbm_map_culling_counts, which rebuilds the index        j  the record write alone   (i - j: the build)
  e  CovisibilityCounts / KeyFrameCulling over a ResidentMap (host/Covisibility.h)     } host/test_covisibility time: one process,
  f  the reference's loops transcribed with their std::map copies, on stand-in types   } alternated, on seeded maps of the same sizes
a to d, i and j go through ctypes with every argument prepared beforehand; the device calls end with the stream synchronised inside the
call.  b and d are NOT the reference's loops (leg f has those, as a transcription on stand-in types, not the reference binary): they
are this library's own host routines on flat arrays, which index the records by point on every call."""
import argparse
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

DRIVER = os.path.join(ROOT, "multi_orb_slam_amd", "host", "test_covisibility")
SIZES = (200, 2000)
LISTED = (1, 20, 100)
FEATURES, STEP, N_CAM1 = 2000, 400, 1400


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
        feat = np.tile(np.arange(FEATURES, dtype=np.int32), n_kfs)
        order = rng.permutation(len(obs))                              # (records lie in the slab in the order they were made, not by keyframe)
        self.obs = obs[order]; self.obs_feat = np.ascontiguousarray(feat[order])
        self.kf_feat = (rng.integers(0, 4, (n_kfs, FEATURES)) | np.where(rng.random((n_kfs, FEATURES)) < 0.1, _lib.FEATURE_FAR, 0)).astype(np.uint8)
        self.ncam1 = np.full(n_kfs, N_CAM1, np.int32)
        seen = np.bincount(obs["point"], minlength=n_points)
        self.n_obs = (seen + (seen * rng.random(n_points)).astype(np.int64)).astype(np.int32)
        self.mt = m.Matcher(0.8, True)
        self.rm = rm = m.ResidentMap(self.mt, n_kfs, n_points, len(obs), FEATURES)
        rm.write_points(np.arange(n_points), np.zeros(n_points, m.POINT_DTYPE), self.flags)
        rm.write_point_nobs(np.arange(n_points), self.n_obs)
        rm.write_observations(np.arange(len(obs)), self.obs)
        rm.write_observation_features(np.arange(len(obs)), self.obs_feat)
        for k in range(n_kfs):
            rm.write_keyframe(k, rows[k]); rm.write_keyframe_features(k, self.kf_feat[k], N_CAM1)
        self.L = _lib.lib()
        self.cap = 100 * n_kfs
        self.first = np.zeros(101, np.int32); self.first_h = np.zeros(101, np.int32)
        self.ent = np.zeros(self.cap, m.COVIS_DTYPE); self.ent_h = np.zeros(self.cap, m.COVIS_DTYPE)
        self.counts = np.zeros((100, 2), np.int32); self.counts_h = np.zeros((100, 2), np.int32)
        self.slot0 = np.zeros(1, np.int32); self.rec0 = self.obs[:1].copy()
        self.listed(1)

    def listed(self, n):
        self.kfs = (self.n_kfs // 2 + 3 * np.arange(n)).astype(np.int32) % self.n_kfs
        assert len(np.unique(self.kfs)) == n

    def a(self):
        _lib.check(self.L.orbm_map_covisibility(self.mt._h, self.rm._h, _lib.ptr(self.kfs), len(self.kfs), _lib.ptr(self.first), _lib.ptr(self.ent), self.cap))
        return self.ent[:self.first[len(self.kfs)]]

    def b(self):
        _lib.check(self.L.orbm_local_map_covisibility_host(_lib.ptr(self.obs), _lib.ptr(self.obs_feat), len(self.obs), _lib.ptr(self.flags), self.n_points,
                                                           _lib.ptr(self.rows), _lib.ptr(self.count), _lib.ptr(self.ncam1), self.n_kfs, FEATURES,
                                                           _lib.ptr(self.kfs), len(self.kfs), _lib.ptr(self.first_h), _lib.ptr(self.ent_h), self.cap))
        return self.ent_h[:self.first_h[len(self.kfs)]]

    def c(self):
        _lib.check(self.L.orbm_map_culling_counts(self.mt._h, self.rm._h, _lib.ptr(self.kfs), len(self.kfs), 0, _lib.ptr(self.counts)))
        return self.counts[:len(self.kfs)]

    def d(self):
        _lib.check(self.L.orbm_local_map_culling_host(_lib.ptr(self.obs), _lib.ptr(self.obs_feat), len(self.obs), _lib.ptr(self.flags), _lib.ptr(self.n_obs),
                                                      self.n_points, _lib.ptr(self.rows), _lib.ptr(self.count), _lib.ptr(self.kf_feat), self.n_kfs, FEATURES,
                                                      _lib.ptr(self.kfs), len(self.kfs), 0, _lib.ptr(self.counts_h)))
        return self.counts_h[:len(self.kfs)]

    def j(self):
        _lib.check(self.L.orbm_map_write_observations(self.mt._h, self.rm._h, _lib.ptr(self.slot0), 1, _lib.ptr(self.rec0)))

    def i(self):
        self.j()
        self.c()

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
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--no-class", action="store_true")
    a = ap.parse_args()
    results = []
    for n_kfs in a.sizes:
        lg = Legs(n_kfs)
        for n in LISTED:
            lg.listed(n)
            assert np.array_equal(lg.a(), lg.b()) and len(lg.a()) > 0           # the two sides do the same job
            assert lg.rm.last_covisibility()[:2] == (1, 0)                      # ... on the device, over a clean index
            assert np.array_equal(lg.c(), lg.d()) and lg.counts[:n, 1].sum() > 0
            lg.i()
            assert lg.rm.last_covisibility()[:2] == (1, 1)                      # a record write makes the next call rebuild the index
            t = {k: [] for k in "abcdij"}
            for _ in range(a.pairs):                                            # alternated in one process
                for k in "abcdij":
                    t[k].append(leg(getattr(lg, k), a.seconds))
            lg.c()
            results.append({"keyframes": n_kfs, "points": lg.n_points, "records": len(lg.obs), "listed": n, "entries": int(lg.first[n]),
                            "counted_points": int(lg.counts[:n, 0].sum()), "redundant": int(lg.counts[:n, 1].sum()),
                            "a_map_covisibility": spread(t["a"]), "b_covisibility_host": spread(t["b"]), "c_map_culling_counts": spread(t["c"]),
                            "d_culling_host": spread(t["d"]), "i_write_one_record_then_culling_counts_with_index_build": spread(t["i"]),
                            "j_write_one_record": spread(t["j"])})
            print(json.dumps(results[-1]), flush=True)
        lg.close()
    if not a.no_class:
        for n_kfs in a.sizes:
            n_points = STEP * (n_kfs - 1) + FEATURES
            for n in LISTED:
                r = subprocess.run(["timeout", "-k", "10", "400", DRIVER, "time", str(n_kfs), str(n_points), "6", str(n), str(a.seconds)],
                                   capture_output=True, text=True, timeout=430)
                if r.returncode != 0:
                    raise SystemExit("test_covisibility time failed (%d): %s" % (r.returncode, r.stderr[-1000:]))
                legs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
                row = {"class_keyframes": n_kfs, "points": n_points, "records": legs[0]["records"], "listed": n}
                for what in ("covisibility", "culling"):
                    for route, key in (("class", "e_class"), ("transcription", "f_reference_loops_transcribed")):
                        v = [1e3 * l["ms_per_call"] for l in legs if l["what"] == what and l["route"] == route]
                        sums = {l["checksum"] for l in legs if l["what"] == what}
                        assert len(sums) == 1, (what, sums)                    # both routes count the same
                        row["%s_%s" % (what, key)] = spread(v)
                results.append(row)
                print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
