"""bench.py as the driver runs it: a plain run warms up, times exactly --steps steps and does nothing else, and --dump-outputs
writes what the last timed step computed -- held here against the oracle fed the same synthetic stream."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
import multi_orb_slam_amd as m
from multi_orb_slam_amd import synth
from oracle_pipeline import OracleFrontEnd

pytestmark = pytest.mark.gpu
BENCH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py")


@pytest.mark.timeout(300, method="thread")
def test_plain_run_times_exactly_steps_and_dumps_the_last_step(tmp_path):
    steps, warmup = 25, 6
    env = dict(os.environ, MORB_BENCH_WATCHDOG_S="240")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path)],
                       env=env, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["metric"] == "frames/sec (N-cam extract+match)" and line["unit"] == "frames/s" and line["higher_is_better"] is True
    assert line["dtype"] == "u8" and line["steps"] == steps and line["warmup"] == warmup and line["full"] is False
    assert line["timing"]["blocks"] == 1 and line["timing"]["step_ms"]["n"] == steps
    assert line["ms_per_step"] > 0 and abs(line["value"] * line["ms_per_step"] / 1e3 - 1.0) < 0.01   # one rig: value = 1 / step time
    assert not any(k in line for k in ("parity", "roofline", "roofline_m1", "dropin", "cpu_baseline", "latency_ms_isolated", "c_abi_loop"))
    names = {p.name[:-4] for p in tmp_path.iterdir()}
    assert names == set(line["dumped_outputs"]) and sum(p.stat().st_size for p in tmp_path.iterdir()) <= bench.DUMP_LIMIT_BYTES

    # the oracle over the same stream up to the last timed step (timestep warmup + steps - 1)
    P = bench.plan_for(1, 1, 0)
    W, H, gcam = P["width"], P["height"], P["global_cams"]
    ofe = OracleFrontEnd([m.ExtractorParams(nfeatures=P["nfeatures"])] * len(gcam), W, H, gcam, cam_threads=True)
    frames = [[synth.image(g, t, W, H) for g in gcam] for t in range(P["ring"])]
    for t in range(warmup + steps):
        exp = ofe.step(frames[t % P["ring"]])
    if ofe.pool is not None:
        ofe.pool.shutdown()
    got = {n: np.load(tmp_path / (n + ".npy")) for n in names}
    for n, v in got.items():
        assert v.dtype in (np.float32, np.float64), n
    assert got["counts"].tolist() == exp["counts"] and got["n_temporal"][0] == exp["n_temporal"] and got["n_cross"][0] == exp["n_cross"]
    for f in exp["kps"].dtype.names:
        assert np.array_equal(got["kps_" + f], exp["kps"][f]) and got["kps_" + f].dtype.itemsize >= exp["kps"][f].dtype.itemsize, f
    assert got["kps_x"].tobytes() == exp["kps"]["x"].tobytes() and got["kps_angle"].tobytes() == exp["kps"]["angle"].tobytes()
    assert np.array_equal(got["desc"], exp["desc"])
    for n in ("uright", "depth", "un_x", "un_y"):
        assert got[n].tobytes() == np.asarray(exp[n], np.float32).tobytes(), n
    assert np.array_equal(got["match_of_feature"], exp["match_of_feature"]) and exp["n_temporal"] > 100
    for n, v in zip(("cross_best_idx", "cross_best_dist", "cross_second_dist"), exp["cross"]):
        assert np.array_equal(got[n], v), n
