#!/usr/bin/env python3
"""Timings of the loop correction over the resident map (orbm_map_correct_sim3, orbm_map_correct_rigid) next to the host routines that
do the same job on plain arrays, same maps, same box, same run.  Informational: bench.py's contract is untouched.

    python tools/loop_correction_bench.py [--out profiles/r26/loop_correction_bench.json]   all legs, alternated five times

Whole calls with the synchronisation inside, through ctypes with every argument prepared beforehand.  Legs, per call and size:
  a  the device call: rows and mirror corrected in place
  b  the library's host routine on the same arrays (positions packed n x 3)
  c  b, then orbm_map_write_points of every changed row, gathered from a host copy of the rows: what keeps a resident map consistent
     without the calls of leg a
Sizes: the Sim3 call over a loop's neighbourhood -- 30 keyframes of 2 000 features, a window of 2 000 points that moves on by 1 300 per
keyframe, about 40 000 kept points; the rigid call over a whole map of 100 000 and 1 000 000 points under 2 000 keyframes, 70 % of the
points with a position from global BA, the rest carried through their reference keyframe.  So that a thousand repetitions leave the map
where it was, the Sim3 legs run with CorrectedSim3 == NonCorrectedSim3 and the rigid legs with GetPoseInverse() the inverse of
mTcwBefGBA: the statements executed are the same, the points stay put to rounding.
The two drop-ins (host/LoopCorrection.h) against their transcriptions are NOT measured here: host/test_loop_correction has no timing
mode yet."""
import argparse
import ctypes as C
import json
import os
import sys
import time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import multi_orb_slam_amd as m  # noqa: E402
from multi_orb_slam_amd import _lib  # noqa: E402
import loopcorrect_worlds as lw  # noqa: E402

P = _lib.ptr


class Sim3Legs:
    KFS, FEATURES, STEP = 30, 2000, 1300

    def __init__(self, mt):
        rng = np.random.default_rng(1)
        self.mt = mt; self.L = _lib.lib()
        n_kfs, F = self.KFS, self.FEATURES
        self.n_points = n = self.STEP * (n_kfs - 1) + F
        self.kf_rows = np.stack([self.STEP * k + rng.permutation(F) for k in range(n_kfs)]).astype(np.int32)
        self.kf_count = np.full(n_kfs, F, np.int32)
        self.flags = (rng.random(n) < 0.03).astype(np.uint8)
        self.rows = np.zeros(n, m.POINT_DTYPE); self.rows["pos"] = rng.uniform(-10, 10, (n, 3))
        self.kfs = rng.permutation(n_kfs).astype(np.int32)
        self.before = lw.random_sim3(rng, n_kfs, True); self.after = self.before.copy()
        self.already = rng.permutation(n)[:n // 50].astype(np.int32)
        self.rm = m.ResidentMap(mt, n_kfs, n, 1, F)
        self.rm.write_points(np.arange(n), self.rows, self.flags)
        for k in range(n_kfs):
            self.rm.write_keyframe(k, self.kf_rows[k])
        self.cap = n
        self.ent = np.zeros(n, m.CORRECT_DTYPE); self.out = np.zeros((n, 3), np.float32); self.tiw = np.zeros((n_kfs, 16), np.float32)
        self.ent_h = self.ent.copy(); self.out_h = self.out.copy(); self.n = C.c_int(); self.n_h = C.c_int()
        self.pos = np.ascontiguousarray(self.rows["pos"])

    def a(self):
        _lib.check(self.L.orbm_map_correct_sim3(self.mt._h, self.rm._h, P(self.kfs), len(self.kfs), P(self.before), P(self.after), P(self.already),
                                                len(self.already), P(self.ent), P(self.out), self.cap, C.byref(self.n), P(self.tiw)))

    def b(self):
        _lib.check(self.L.orbm_local_map_correct_sim3_host(P(self.kf_rows), P(self.kf_count), self.KFS, self.FEATURES, P(self.flags), P(self.pos), 3,
                                                           self.n_points, P(self.kfs), len(self.kfs), P(self.before), P(self.after), P(self.already),
                                                           len(self.already), P(self.ent_h), P(self.out_h), self.cap, C.byref(self.n_h), P(self.tiw)))

    def c(self):
        self.b()
        slots = np.ascontiguousarray(self.ent_h["point"][:self.n_h.value])
        self.rows["pos"][slots] = self.out_h[:self.n_h.value]
        changed = self.rows[slots]                                    # the gather of the rows that travel
        _lib.check(self.L.orbm_map_write_points(self.mt._h, self.rm._h, P(slots), len(slots), P(changed), P(self.flags[slots])))

    def check(self):
        self.a(); self.b()
        k = self.n.value
        assert k == self.n_h.value > 30000 and self.rm.last_correction()[0] == 1
        assert self.ent[:k].tobytes() == self.ent_h[:k].tobytes()
        return {"keyframes": self.KFS, "candidates": int(self.kf_count.sum()), "kept": k}

    def close(self):
        self.rm.close()


class RigidLegs:
    KFS = 2000

    def __init__(self, mt, n):
        rng = np.random.default_rng(n)
        self.mt = mt; self.L = _lib.lib(); self.n_points = n
        self.flags = (rng.random(n) < 0.03).astype(np.uint8)
        self.rows = np.zeros(n, m.POINT_DTYPE); self.rows["pos"] = rng.uniform(-10, 10, (n, 3))
        self.ref = rng.integers(-1, self.KFS, n).astype(np.int32)
        self.corrected = (rng.random(self.KFS) < 0.9).astype(np.uint8)
        Tb = lw.random_pose_rows(rng, self.KFS).reshape(-1, 3, 4)
        Ta = np.zeros_like(Tb)                                        # the inverse pose: [R^T | -R^T t]
        Ta[:, :, :3] = Tb[:, :, :3].transpose(0, 2, 1)
        Ta[:, :, 3] = -np.einsum("kij,kj->ki", Ta[:, :, :3], Tb[:, :, 3])
        self.Tb = np.ascontiguousarray(Tb.reshape(-1, 12)); self.Ta = np.ascontiguousarray(Ta.reshape(-1, 12))
        self.gba_slots = rng.permutation(n)[:int(0.7 * n)].astype(np.int32)
        self.gba_pos = np.ascontiguousarray(self.rows["pos"][self.gba_slots])
        self.rm = m.ResidentMap(mt, 4, n, 1, 4)
        self.rm.write_points(np.arange(n), self.rows, self.flags)
        self.rm.write_point_ref(np.arange(n), self.ref)
        self.st = np.zeros(n, np.uint8); self.out = np.zeros((n, 3), np.float32); self.st_h = self.st.copy(); self.out_h = self.out.copy()
        self.pos = np.ascontiguousarray(self.rows["pos"])

    def a(self):
        _lib.check(self.L.orbm_map_correct_rigid(self.mt._h, self.rm._h, None, self.n_points, P(self.corrected), P(self.Tb), P(self.Ta), self.KFS,
                                                 P(self.gba_slots), P(self.gba_pos), len(self.gba_slots), P(self.st), P(self.out)))

    def b(self):
        _lib.check(self.L.orbm_local_map_correct_rigid_host(P(self.pos), 3, P(self.flags), P(self.ref), self.n_points, None, self.n_points,
                                                            P(self.corrected), P(self.Tb), P(self.Ta), self.KFS, P(self.gba_slots), P(self.gba_pos),
                                                            len(self.gba_slots), P(self.st_h), P(self.out_h)))

    def c(self):
        self.b()
        slots = np.nonzero(self.st_h)[0].astype(np.int32)
        self.rows["pos"][slots] = self.out_h[slots]
        changed = self.rows[slots]
        _lib.check(self.L.orbm_map_write_points(self.mt._h, self.rm._h, P(slots), len(slots), P(changed), P(self.flags[slots])))

    def check(self):
        self.a(); self.b()
        assert np.array_equal(self.st, self.st_h) and self.rm.last_correction()[0] == 1
        return {"points": self.n_points, "keyframes": self.KFS, "given": int((self.st == 1).sum()), "moved": int((self.st == 2).sum())}

    def close(self):
        self.rm.close()


def leg(fn, seconds):
    n, t0 = 0, time.perf_counter()
    while True:
        fn(); n += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n * 1e6


def spread(v):
    return {"median_us": round(float(np.median(v)), 1), "min_us": round(float(min(v)), 1), "max_us": round(float(max(v)), 1), "pairs": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--rigid", type=int, nargs="*", default=[100000, 1000000])
    a = ap.parse_args()
    mt = m.Matcher(0.8, True)
    results = []
    for what, make in [("correct_sim3", lambda: Sim3Legs(mt))] + [("correct_rigid", (lambda n: lambda: RigidLegs(mt, n))(n)) for n in a.rigid]:
        lg = make()
        row = {"call": what}; row.update(lg.check())
        t = {k: [] for k in "abc"}
        for _ in range(a.pairs):                                      # alternated in one process
            for k in "abc":
                t[k].append(leg(getattr(lg, k), a.seconds))
        row.update({"a_device_call": spread(t["a"]), "b_host_routine": spread(t["b"]), "c_host_routine_then_write_points": spread(t["c"])})
        results.append(row)
        print(json.dumps(row), flush=True)
        lg.close()
    mt.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
