"""The N > 1 job as PROCESSES on one GPU: every rank a fresh process (tests/mp_rank.py), gloo control plane on
127.0.0.1, the exchange as direct writes between the processes' IPC-mapped arenas (orbf_exchange_peer_*), every step of every rank
held against the oracle; and a rank that dies makes every survivor's step return ORB_E_TIMEOUT well inside 30 s.  (RCCL refuses two
ranks on one GPU, so its world > 1 path stays unmeasured here -- the driver's 8-GPU run is the first.)"""
import os
import socket
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _spawn(world, rig_cams, w, h, nf, steps, ahead, extra=(), env_extra=None, timeout=240):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **(env_extra or {}))
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "mp_rank.py")] + [str(x) for x in (world, r, port, rig_cams, w, h, nf, steps, ahead, 0)] + list(extra),
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    t0 = time.time()
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=max(1.0, timeout - (time.time() - t0)))
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            out, _ = p.communicate()
            out += b"\n[killed by the test after %d s]" % timeout
        outs.append(out.decode("utf-8", "replace"))
    return [p.returncode for p in procs], outs, time.time() - t0


@pytest.mark.timeout(400, method="thread")
@pytest.mark.parametrize("world,rig_cams,w,h,nf,ahead", [(2, 2, 640, 480, 1000, 0), (2, 2, 640, 480, 1000, 3), (2, 4, 640, 480, 1000, 2), (4, 4, 320, 240, 300, 3)])
def test_rank_processes_exchange_through_ipc_arenas_bit_exact(world, rig_cams, w, h, nf, ahead):
    """configs[1]'s two cameras as two processes (isolated steps and three announced ahead), configs[3]'s four cameras as two processes
    with two cameras each, four processes with one camera each -- overlapping cameras on a photograph, every rank's every step vs the oracle."""
    rcs, outs, _dt = _spawn(world, rig_cams, w, h, nf, steps=7, ahead=ahead)
    assert rcs == [0] * world, "\n".join(o[-1500:] for o in outs)
    assert "bit-exact vs the oracle" in outs[0]


@pytest.mark.timeout(200, method="thread")
def test_a_dead_rank_is_a_timeout_error_on_every_survivor():
    """rank 1 of three exits without a word before step 3: ranks 0 and 2 must come back from a step with ORB_E_TIMEOUT (the peer
    transport names rank 1) -- within the exchange's timeout (3 s here) plus margins, far inside 30 s, nobody hangs."""
    rcs, outs, dt = _spawn(3, 3, 320, 240, 300, steps=8, ahead=2, extra=("die_at=3:1",), env_extra={"MORB_EXCHANGE_TIMEOUT_MS": "3000"}, timeout=120)
    assert rcs[1] == 0 and rcs[0] == 3 and rcs[2] == 3, "\n".join(o[-1500:] for o in outs)
    assert "rank(s) 1 did not deliver" in outs[0] and "rank(s) 1 did not deliver" in outs[2]
    assert dt < 60.0


@pytest.mark.timeout(300, method="thread")
def test_bench_runs_two_rank_processes_on_this_one_gpu():
    """`python bench.py --gpus 2 --config 3` on a box with ONE GPU: the launcher starts two rank processes (the parent never touches the
    GPU), they share device 0, gloo is the control plane, the peer transport the exchange; each rank runs the parity gate against the
    OTHER rank's cameras (--full), blocks are timed with barriers on both sides and MAX-reduced, rank 0 relays the one JSON line -- which
    says n_ranks 2 on n_gpus 1: a rehearsal, not a scaling measurement."""
    import json
    root = os.path.dirname(HERE)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MORB_BENCH_WATCHDOG_S="240")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--config", "3", "--steps", "60", "--warmup", "20", "--min-time", "0.05",
                        "--full", "--no-roofline", "--no-cpu"], env=env, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_ranks"] == 2 and line["n_gpus"] == 1 and line["value"] > 0 and line["scaling"] == "strong"
    assert "bit-exact vs oracle" in line["parity"] and "peer transport" in line["exchange"]


@pytest.mark.timeout(300, method="thread")
@pytest.mark.parametrize("max_keys, expected_redos", [(16384, 1), (4096, 7)], ids=["one_step_falls_back", "every_step_falls_back"])
def test_reshipped_blocks_and_unequal_look_ahead_between_rank_processes(max_keys, expected_redos):
    """ADVICE r05's scenario between PROCESSES: three ranks with DIFFERENT look-ahead (0, 1 and 3 steps); extractions fall back to the
    host path AFTER their blocks went out (more level-0 candidates than the device quadtree takes: the limit is lowered here), the
    blocks carry the mark, and every rank ships its final block a second time (the peer transport's second region).
    one_step_falls_back: camera 1 sees noise in step 2 (27 703 candidates > 16 384).  every_step_falls_back: the photograph itself
    (10 049 candidates at 640x480) is over a limit of 4096 on every rank in every step.
    This is the test that found the round-6 ordering bug: a step's exchange ends in a wait for the other ranks and stands on the
    stream of the step's extraction chain; the rank that ran ahead dropped its steps in flight and then had the waits for steps 1..3
    IN FRONT of the re-extraction of step 0, whose re-shipment the rank without look-ahead was waiting for -- every rank sat out the
    timeout.  Dropped runs are now forgotten instead of completed (orbx_discard) and, until the dropped exchanges have been answered,
    the handle extracts on a spare extractor that works on the matcher's stream (frontend.hip: x_spare_until).
    Every step of every rank is held against the oracle; every rank counts the same re-shipments."""
    rcs, outs, _dt = _spawn(3, 3, 640, 480, 500, steps=7, ahead=0, extra=("aheads=0,1,3", "noise_at=2:1"),
                            env_extra={"MORB_OCT_MAX_KEYS": str(max_keys), "MORB_EXCHANGE_TIMEOUT_MS": "10000"})
    assert rcs == [0, 0, 0], "\n".join(o[-1500:] for o in outs)
    assert "bit-exact vs the oracle" in outs[0]
    import re
    redos = [int(x) for x in re.findall(r"\(\d+, \[[^\]]*\], \d+, \d+, (\d+)\)", outs[0])]
    assert redos == [expected_redos] * 3, outs[0][-800:]


@pytest.mark.timeout(300, method="thread")
def test_a_slow_rank_never_sees_a_block_overwritten():
    """Three ranks three steps ahead, rank 1 sleeps 40 ms before every step: the fast ranks run into their look-ahead limit, ship the
    blocks of up to three future steps into rank 1's arena while it is still busy with an old one, and wait; the eight slots per rank
    must keep every block intact until its step (why eight suffice).  16 steps = two trips round the slots, every
    step of every rank against the oracle."""
    rcs, outs, _dt = _spawn(3, 3, 320, 240, 300, steps=16, ahead=3, extra=("slow=1:40",))
    assert rcs == [0, 0, 0], "\n".join(o[-1500:] for o in outs)
    assert "bit-exact vs the oracle" in outs[0]
