"""Child process of tests/test_gpu_loop_correction.py, started with MORB_HOST_RESOLVE=1 (read in orbm_create): the two corrections
through their host route -- the host routines over the map's mirror, the new positions then sent to their rows -- against the model,
with the rows read back from HBM.  Prints 'loop_correction_leg ok'."""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)
import multi_orb_slam_amd as m  # noqa: E402
import loopcorrect_worlds as lw  # noqa: E402
import test_gpu_loop_correction as t  # noqa: E402


def main():
    assert os.environ.get("MORB_HOST_RESOLVE") == "1"
    mt = m.Matcher(0.8, True)
    w, exp = lw.sim3_case(257)
    rm, rows0 = t.sim3_map_of(mt, w)
    ent, out, Tiw = rm.correct_sim3(w["kfs"], w["before"], w["after"], w["already"])
    assert rm.last_correction() == (0, int(w["kf_count"][w["kfs"]].sum()), 257, len(w["kfs"]))   # the host route ran
    assert np.array_equal(t.entries2(ent), exp[0]) and np.array_equal(t.bits(out), t.bits(exp[1])) and np.array_equal(t.bits(Tiw), t.bits(exp[2]))
    t.assert_rows(rm, rows0, exp[3])
    try:
        rm.correct_sim3(w["kfs"], w["before"], w["after"], (), cap=3)
    except m.OrbError as e:
        assert e.code == m._lib.ORB_E_CAPACITY and e.needed > 257
    else:
        raise AssertionError("a list of 3 took more than 257 points")
    t.assert_rows(rm, rows0, exp[3])
    rm.close()
    w, exp = lw.rigid_case(257)
    for slots in (None, np.random.default_rng(1).permutation(w["n_points"])[:200].astype(np.int32)):
        e = exp if slots is None else lw.model.correct_rigid(w["pos"], w["flags"], w["ref"], slots, w["kf_corrected"], w["Tb"], w["Ta"],
                                                             w["gba_slots"], w["gba_pos"])
        rm, rows0 = t.rigid_map_of(mt, w)
        st, pos = rm.correct_rigid(slots, w["kf_corrected"], w["Tb"], w["Ta"], w["gba_slots"], w["gba_pos"])
        assert rm.last_correction()[0] == 0 and rm.last_correction()[2] == int((e[0] != 0).sum()) > 20
        assert np.array_equal(st, e[0]) and np.array_equal(t.bits(pos), t.bits(e[1]))
        t.assert_rows(rm, rows0, e[2])
        rm.close()
    mt.close()
    print("loop_correction_leg ok")


if __name__ == "__main__":
    main()
