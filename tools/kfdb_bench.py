#!/usr/bin/env python3
"""Timings of the resident keyframe database (orbv_db_query, KeyFrameDatabase::DetectRelocalizationCandidates) next to the reference's
algorithm on the host (`host/test_kfdb`: inverted files as lists + ORBVocabulary::score), same worlds, same box, same run.
Informational: bench.py's contract is untouched.

    python tools/kfdb_bench.py [--out profiles/r07/kfdb_bench.json]     all legs, every leg >= 0.5 s, alternated five times
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o kfdb -- python tools/kfdb_bench.py --trace-plan
                                                                         only the query calls, in a fixed order, for a kernel trace
    python tools/kfdb_bench.py --kernel-trace DIR/.../kfdb_kernel_trace.csv --out ...   adds k_db_query's own time per configuration

Worlds: K keyframes of ~1 500 words (tests/kfdb_model.py's generator).  Algorithmic bytes of one query = alive words x 12 B (ids + values
read once) + 24 B per entry and query of output, the budget the interface was specified with; the kernel writes 16 B of them (score,
common, first word), and the figure with 16 B is reported beside it.  Over the kernel's time either is a share of the HBM peak
(8.0 TB/s) -- computed from shapes, not a measured traffic figure."""
import argparse
import csv
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
import kfdb_model as km  # noqa: E402

DRIVER = os.path.join(ROOT, "multi_orb_slam_amd", "host", "test_kfdb")
KS = (1000, 10000)
QS = (1, 8)
TRACE_REPS = 40
HBM_PEAK = 8.0e12


def world(K):
    w = km.World(K, seed=K, words=(1450, 1550), stride=200, window=4000)
    for k in w.kfs:
        k.bow1 = k.bow        # the database under test holds the whole ~1 500-word vectors (the camera-1 file of the class)
    lap = K // 2
    asking = [lap + (j * 37 + 11) % (lap - 10) for j in range(8)]
    return w, asking


def fill(w, asking):
    db = m.KeyFrameDatabase(w.n_words)
    words = 0
    for t, k in enumerate(w.kfs):
        if t not in asking:
            db.add(k.mnId, k.bow1); words += len(k.bow1[0])
    return db, words


def leg(fn, seconds=0.5):
    """calls of fn for at least `seconds` (each call ends with the stream synchronised, inside the timed window) -> us per call"""
    n, t0 = 0, time.perf_counter()
    while True:
        fn(); n += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n * 1e6


def spread(v):
    return {"median_us": round(float(np.median(v)), 2), "min_us": round(float(min(v)), 2), "max_us": round(float(max(v)), 2)}


def trace_plan():
    for K in KS:
        w, asking = world(K)
        db, _ = fill(w, asking)
        qs = [w.kfs[t].bow1 for t in asking]
        for Q in QS:
            for _ in range(TRACE_REPS + 3):
                db.query(qs[:Q])
        db.close()


def read_trace(path):
    """k_db_query dispatches in time order, cut into the runs trace_plan() makes (3 warm-up calls dropped per run) -> {(K, Q): [us]}"""
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            if "k_db_query" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    rows.sort()
    per = TRACE_REPS + 3
    assert len(rows) == per * len(KS) * len(QS), (len(rows), per)
    out, i = {}, 0
    for K in KS:
        for Q in QS:
            out[(K, Q)] = [us for _, us in rows[i + 3:i + per]]
            i += per
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--trace-plan", action="store_true")
    ap.add_argument("--kernel-trace")
    ap.add_argument("--seconds", type=float, default=0.5)
    a = ap.parse_args()
    if a.trace_plan:
        trace_plan()
        return
    kernel = read_trace(a.kernel_trace) if a.kernel_trace else {}
    results = []
    for K in KS:
        w, asking = world(K)
        db, words = fill(w, asking)
        qs = [w.kfs[t].bow1 for t in asking]
        for Q in QS:
            db.query(qs[:Q])
        gpu = {Q: [] for Q in QS}
        for _ in range(5):                      # legs alternated five times
            for Q in QS:
                gpu[Q].append(leg(lambda: db.query(qs[:Q]), a.seconds))
        entries = len(db)
        db.close()
        # the class and the host restatement: one process, five alternations (host/test_kfdb time)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "world.bin")
            ops = [("add_cam1", t, 0, 0.0) for t in range(K) if t not in asking] + [("reloc", t, 0, 0.0) for t in asking]
            for k in w.kfs:
                k.bow = (k.bow[0][:0], k.bow[1][:0])      # only the camera-1 file is used (it holds the whole vectors): keep the world file small
            km.write_world(path, w.n_words, w.kfs, ops)
            r = subprocess.run(["timeout", "-k", "10", "500", DRIVER, "time", path, str(a.seconds)], capture_output=True, text=True, timeout=540)
            if r.returncode != 0:
                raise SystemExit("test_kfdb time failed (%d): %s" % (r.returncode, r.stderr[-1000:]))
        legs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
        host = [l["us_per_call"] for l in legs if l["leg"] == "host"]
        cls = [l["us_per_call"] for l in legs if l["leg"] == "class"]
        for Q in QS:
            row = {"K": K, "alive_entries": entries, "alive_words": words, "Q": Q, "query_call": spread(gpu[Q]),
                   "query_call_us_per_query": round(float(np.median(gpu[Q])) / Q, 2)}
            bytes_alg = words * 12 + 24 * entries * Q
            bytes_written = words * 12 + 16 * entries * Q
            row["algorithmic_bytes"] = bytes_alg
            row["algorithmic_bytes_with_16B_out"] = bytes_written
            if (K, Q) in kernel:
                ku = float(np.median(kernel[(K, Q)]))
                row["k_db_query_us"] = round(ku, 2)
                row["algorithmic_bytes_over_kernel_time_share_of_hbm_peak"] = round(bytes_alg / (ku * 1e-6) / HBM_PEAK, 4)
                row["with_16B_out_over_kernel_time_share_of_hbm_peak"] = round(bytes_written / (ku * 1e-6) / HBM_PEAK, 4)
            results.append(row)
        results.append({"K": K, "detect_relocalization_candidates": {"class_on_device": spread(cls), "host_lists": spread(host),
                                                                       "host_over_class": round(float(np.median(host) / np.median(cls)), 2)},
                        "checksums": r.stderr.strip().splitlines()[-1]})
    for row in results:
        print(json.dumps(row))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
