"""GPU parity of the loop correction over the resident map (orbm_map_correct_sim3, orbm_map_correct_rigid, orbm_map_write_positions,
orbm_map_write_point_ref): the device against the library's host routines and the NumPy model of the reference's statements on the
worlds and hand-built cases of tests/loopcorrect_worlds.py.  Every comparison is equality of integers or of raw bytes; the rows are
read back from HBM (orbm_debug_map_read_points), the mirror through a rigid call that corrects nothing (its pos_out is the mirror's)."""
import numpy as np
import pytest

import loopcorrect_model as model
import loopcorrect_worlds as lw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher():
    import multi_orb_slam_amd as m
    mt = m.Matcher(0.8, True)
    yield mt
    mt.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def random_rows(n, pos, seed):
    """Rows whose every field beside the position is random: a correction must leave those bytes alone."""
    import multi_orb_slam_amd as m
    rng = np.random.default_rng(seed)
    rows = np.frombuffer(rng.bytes(n * m.POINT_DTYPE.itemsize), m.POINT_DTYPE).copy()
    rows["pos"] = pos
    return rows


def sim3_map_of(mt, w):
    import multi_orb_slam_amd as m
    rm = m.ResidentMap(mt, w["n_kfs"], w["n_points"], 1, w["stride"])
    rows = random_rows(w["n_points"], w["pos"], 1)
    rm.write_points(np.arange(w["n_points"]), rows, w["flags"])
    for k in range(w["n_kfs"]):
        rm.write_keyframe(k, w["kf_rows"][k, :w["kf_count"][k]])
    return rm, rows


def rigid_map_of(mt, w):
    import multi_orb_slam_amd as m
    rm = m.ResidentMap(mt, w["n_kfs"], w["n_points"], 1, 4)
    rows = random_rows(w["n_points"], w["pos"], 2)
    rm.write_points(np.arange(w["n_points"]), rows, w["flags"])
    rm.write_point_ref(np.arange(w["n_points"]), w["ref"])
    return rm, rows


def mirror_positions(rm):
    st, pos = rm.correct_rigid(None, [], [], [])
    assert not st.any()
    return pos


def assert_rows(rm, rows0, new_pos):
    """HBM holds rows0 with the positions new_pos and nothing else changed; the mirror holds the same positions."""
    hbm = rm.read_points(np.arange(len(rows0)))
    assert np.array_equal(bits(hbm["pos"]), bits(new_pos))
    exp = rows0.copy(); exp["pos"] = new_pos
    assert hbm.tobytes() == exp.tobytes()
    assert np.array_equal(bits(mirror_positions(rm)), bits(new_pos))


def entries2(ent):
    return np.stack([ent["point"], ent["position"]], axis=1).reshape(-1, 2)


def host_sim3(w):
    import multi_orb_slam_amd as m
    return m.local_map_correct_sim3_host(w["kf_rows"], w["kf_count"], w["flags"], w["pos"], w["kfs"], w["before"], w["after"], w["already"])


def sim3_device_case(mt, w, exp):
    e_ent, e_out, e_Tiw, e_new = exp
    rm, rows0 = sim3_map_of(mt, w)
    try:
        ent, out, Tiw = rm.correct_sim3(w["kfs"], w["before"], w["after"], w["already"])
        cand = int(w["kf_count"][w["kfs"]].sum())
        print("correct_sim3: %d keyframes, %d candidates -> %d kept" % (len(w["kfs"]), cand, len(ent)))
        assert rm.last_correction() == (1, cand, len(e_ent), len(w["kfs"]))
        assert np.array_equal(entries2(ent), e_ent) and np.array_equal(bits(out), bits(e_out)) and np.array_equal(bits(Tiw), bits(e_Tiw))
        h_ent, h_out, h_Tiw, h_new = host_sim3(w)
        assert ent.tobytes() == h_ent.tobytes() and out.tobytes() == h_out.tobytes() and Tiw.tobytes() == h_Tiw.tobytes()
        assert np.array_equal(bits(h_new), bits(e_new))
        assert_rows(rm, rows0, e_new)
    finally:
        rm.close()


def test_hand_built_sim3_case(matcher):
    h = lw.hand_sim3()
    h.update(n_kfs=2, n_points=6, stride=5)
    exp = model.correct_sim3(h["kf_rows"], h["kf_count"], h["flags"], h["pos"], h["kfs"], h["before"], h["after"], h["already"])
    assert np.array_equal(exp[0], h["exp_entries"]) and np.array_equal(exp[1], h["exp_pos"])
    sim3_device_case(matcher, h, exp)


@pytest.mark.parametrize("kept", lw.KEPT)
def test_sim3_worlds(matcher, kept):
    w, exp = lw.sim3_case(kept)
    sim3_device_case(matcher, w, exp)


@pytest.mark.parametrize("variant", ["fixed", "same"])
def test_sim3_scale_one_and_equal_transforms(matcher, variant):
    w, exp = lw.sim3_case(257, variant)
    sim3_device_case(matcher, w, exp)


@pytest.mark.parametrize("kept", [1, 65, 257])
def test_sim3_capacity_one_short_changes_nothing(matcher, kept):
    import multi_orb_slam_amd as m
    from multi_orb_slam_amd import _lib
    w, exp = lw.sim3_case(kept)
    rm, rows0 = sim3_map_of(matcher, w)
    try:
        with pytest.raises(m.OrbError) as e:
            rm.correct_sim3(w["kfs"], w["before"], w["after"], w["already"], cap=kept - 1)
        assert e.value.code == _lib.ORB_E_CAPACITY and e.value.needed == kept and str(kept) in str(e.value)
        assert_rows(rm, rows0, w["pos"])                            # no row and no mirror entry changed
        ent, out, _ = rm.correct_sim3(w["kfs"], w["before"], w["after"], w["already"], cap=kept)
        assert np.array_equal(entries2(ent), exp[0]) and np.array_equal(bits(out), bits(exp[1]))
        assert_rows(rm, rows0, exp[3])
    finally:
        rm.close()


def test_sim3_second_call_does_not_see_the_marks_of_the_first(matcher):
    """Two calls on one map with different lists: the first skips `already` and claims through kfs[:3]; the second, with nothing to
    skip and the whole list, claims what the first skipped or never met, and moves what the first moved once more."""
    w, _ = lw.sim3_case(257)
    rm, rows0 = sim3_map_of(matcher, w)
    try:
        a = slice(0, 3)
        e1 = model.correct_sim3(w["kf_rows"], w["kf_count"], w["flags"], w["pos"], w["kfs"][a], w["before"][a], w["after"][a], w["already"])
        e2 = model.correct_sim3(w["kf_rows"], w["kf_count"], w["flags"], e1[3], w["kfs"][::-1], w["before"][::-1], w["after"][::-1], ())
        g1 = rm.correct_sim3(w["kfs"][a], w["before"][a], w["after"][a], w["already"])
        assert np.array_equal(entries2(g1[0]), e1[0]) and np.array_equal(bits(g1[1]), bits(e1[1]))
        g2 = rm.correct_sim3(w["kfs"][::-1].copy(), w["before"][::-1].copy(), w["after"][::-1].copy(), ())
        assert np.array_equal(entries2(g2[0]), e2[0]) and np.array_equal(bits(g2[1]), bits(e2[1]))
        done = w["already"][w["already"] >= 0]
        assert np.isin(done, e2[0][:, 0]).any() and not np.isin(done, e1[0][:, 0]).any()   # skipped then, claimed now
        assert np.isin(e1[0][:, 0], e2[0][:, 0]).all() and len(e2[0]) > len(e1[0]) > 0
        assert_rows(rm, rows0, e2[3])
    finally:
        rm.close()


# ---- the update after global BA

def rigid_device_case(mt, w, slots, exp):
    import multi_orb_slam_amd as m
    rm, rows0 = rigid_map_of(mt, w)
    try:
        st, out = rm.correct_rigid(slots, w["kf_corrected"], w["Tb"], w["Ta"], w["gba_slots"], w["gba_pos"])
        n = w["n_points"] if slots is None else len(slots)
        print("correct_rigid: %d slots -> %d given, %d moved" % (n, int((st == 1).sum()), int((st == 2).sum())))
        assert rm.last_correction() == (1, n, int((exp[0] != 0).sum()), w["n_kfs"])
        assert np.array_equal(st, exp[0]) and np.array_equal(bits(out), bits(exp[1]))
        h_st, h_out, h_new = m.local_map_correct_rigid_host(w["pos"], w["flags"], w["ref"], slots, w["kf_corrected"], w["Tb"], w["Ta"],
                                                            w["gba_slots"], w["gba_pos"])
        assert st.tobytes() == h_st.tobytes() and out.tobytes() == h_out.tobytes() and np.array_equal(bits(h_new), bits(exp[2]))
        assert_rows(rm, rows0, exp[2])
    finally:
        rm.close()


def test_hand_built_rigid_case(matcher):
    h = lw.hand_rigid()
    h.update(n_points=7, n_kfs=3)
    exp = model.correct_rigid(h["pos"], h["flags"], h["ref"], None, h["kf_corrected"], h["Tb"], h["Ta"], h["gba_slots"], h["gba_pos"])
    assert np.array_equal(exp[0], h["exp_status"]) and np.array_equal(exp[1], h["exp_pos"])
    rigid_device_case(matcher, h, None, exp)


@pytest.mark.parametrize("changed", lw.KEPT)
def test_rigid_worlds(matcher, changed):
    w, exp = lw.rigid_case(changed)
    rigid_device_case(matcher, w, None, exp)


def test_rigid_over_a_list_of_slots_and_twice_in_a_row(matcher):
    """A scattered half of the slots, then the other half with another list of given positions: the second call does not see the
    marks the first left for its given points."""
    import multi_orb_slam_amd as m
    w, _ = lw.rigid_case(257)
    rng = np.random.default_rng(9)
    order = rng.permutation(w["n_points"]).astype(np.int32)
    first, second = order[:len(order) // 2], order[len(order) // 2:]
    e1 = model.correct_rigid(w["pos"], w["flags"], w["ref"], first, w["kf_corrected"], w["Tb"], w["Ta"], w["gba_slots"], w["gba_pos"])
    e2 = model.correct_rigid(e1[2], w["flags"], w["ref"], second, w["kf_corrected"], w["Tb"], w["Ta"], (), ())
    rigid_device_case(matcher, w, first, e1)
    rm, rows0 = rigid_map_of(matcher, w)
    try:
        g1 = rm.correct_rigid(first, w["kf_corrected"], w["Tb"], w["Ta"], w["gba_slots"], w["gba_pos"])
        g2 = rm.correct_rigid(second, w["kf_corrected"], w["Tb"], w["Ta"])
        assert np.array_equal(g1[0], e1[0]) and np.array_equal(g2[0], e2[0]) and np.array_equal(bits(g2[1]), bits(e2[1]))
        given = w["gba_slots"][w["gba_slots"] >= 0]
        assert (e1[0] == 1).any() and not (e2[0] == 1).any() and np.isin(second, given).any()
        assert_rows(rm, rows0, e2[2])
    finally:
        rm.close()


def test_positions_and_references_written_alone(matcher):
    import multi_orb_slam_amd as m
    from multi_orb_slam_amd import _lib
    rng = np.random.default_rng(4)
    n = 1000
    rows0 = random_rows(n, rng.uniform(-5, 5, (n, 3)).astype(np.float32), 3)
    with m.ResidentMap(matcher, 2, n, 1, 4) as rm:
        rm.write_points(np.arange(n), rows0)
        assert rm.points == n
        slots = np.concatenate([rng.permutation(n)[:300], [7, 7]]).astype(np.int32)      # slot 7 twice more: its last entry counts
        pos = rng.uniform(-5, 5, (len(slots), 3)).astype(np.float32)
        rm.write_positions(slots, pos)
        new = rows0["pos"].copy()
        for s, p in zip(slots.tolist(), pos):
            new[s] = p
        assert np.array_equal(new[7], pos[-1])
        assert_rows(rm, rows0, new)
        with pytest.raises(m.OrbError) as e:
            rm.write_positions([3, n], np.zeros((2, 3), np.float32))
        assert e.value.code == _lib.ORB_E_CAPACITY
        with pytest.raises(m.OrbError) as e:
            rm.write_point_ref([n], [0])
        assert e.value.code == _lib.ORB_E_CAPACITY
        assert_rows(rm, rows0, new)                                  # nothing written
        # a reference never written is -1: with every keyframe corrected only the points whose reference was written move
        Tb = lw.random_pose_rows(rng, 2); Ta = lw.random_pose_rows(rng, 2)
        rm.write_point_ref([5, 6, 8], [0, 1, 2])
        st, _ = rm.correct_rigid(None, [1, 1], Tb, Ta)
        assert np.nonzero(st)[0].tolist() == [5, 6] and st[5] == st[6] == 2
        ref = np.full(n, -1, np.int32); ref[[5, 6, 8]] = [0, 1, 2]
        exp = model.correct_rigid(new, np.zeros(n, np.uint8), ref, None, [1, 1], Tb, Ta)
        assert_rows(rm, rows0, exp[2])
        with pytest.raises(m.OrbError) as e:
            rm.correct_rigid([1, 2, 1], [1, 1], Tb, Ta)
        assert e.value.code == _lib.ORB_E_ARG
        assert_rows(rm, rows0, exp[2])


def test_point_list_survives_a_correction_and_the_search_reads_the_new_positions(matcher):
    """orbm_map_local_points, orbm_map_correct_rigid, orbm_map_search_local_points: the same as the search on a fresh map written with
    the corrected rows."""
    import multi_orb_slam_amd as m
    import frustum_worlds as fw
    n = 2000
    w = fw.make_world(n, [1000, 500], 640, 480, 2, 3.0)
    rng = np.random.default_rng(21)
    slots = rng.permutation(3 * n)[:n].astype(np.int32)
    flags = (rng.random(n) < 0.05).astype(np.uint8)
    n_kfs = 3
    kf_rows = [slots[rng.permutation(n)][:900] for _ in range(n_kfs)]
    ref = rng.integers(-1, n_kfs + 1, n).astype(np.int32)
    # a correction of a few centimetres: keyframe r was at a small translation, and is now at another one
    Tb = np.tile(np.eye(3, 4, dtype=np.float32), (n_kfs, 1, 1)); Ta = Tb.copy()
    Tb[:, :, 3] = rng.uniform(-0.05, 0.05, (n_kfs, 3)); Ta[:, :, 3] = rng.uniform(-0.05, 0.05, (n_kfs, 3))
    corrected = np.array([1, 0, 1], np.uint8)
    given = slots[rng.permutation(n)[:200]]
    F = matcher.frame(m.FrameData(**w["fr"]))
    view = w["view"].native()
    with m.ResidentMap(matcher, n_kfs, 3 * n, 1, 1000) as rm, m.ResidentMap(matcher, n_kfs, 3 * n, 1, 1000) as fresh:
        rm.write_points(slots, w["points"], flags); rm.write_point_ref(slots, ref)
        for k in range(n_kfs):
            rm.write_keyframe(k, kf_rows[k]); fresh.write_keyframe(k, kf_rows[k])
        lst = rm.local_points([2, 0, 1])
        before = rm.search(F, view, n_list=len(lst))
        lst = rm.local_points([2, 0, 1])
        gba_pos = (rm.read_points(given)["pos"] + rng.uniform(-0.03, 0.03, (len(given), 3))).astype(np.float32)
        st, pos = rm.correct_rigid(slots, corrected, Tb.reshape(n_kfs, 12), Ta.reshape(n_kfs, 12), given, gba_pos)
        assert (st == 1).sum() > 100 and (st == 2).sum() > 300 and (st == 0).sum() > 300
        got = rm.search(F, view, n_list=len(lst))
        rows = w["points"].copy(); rows["pos"] = pos
        fresh.write_points(slots, rows, flags)
        assert np.array_equal(fresh.local_points([2, 0, 1]), lst)
        exp = fresh.search(F, view, n_list=len(lst))
        print("search after the correction: %d listed, in view %d, matches %d (before: %d, %d)" % (len(lst), got[0], got[1], before[0], before[1]))
        assert got[:2] == exp[:2] and got[1] > 20
        assert got[2].tobytes() == exp[2].tobytes() and got[3].tobytes() == exp[3].tobytes()
        assert got[3].tobytes() != before[3].tobytes()              # the positions the search read are the new ones
    F.close()


def test_host_route_of_the_correction_gives_the_same_bytes():
    """MORB_HOST_RESOLVE=1 (read in orbm_create, hence a fresh child process): both calls through the host routines over the mirror, the
    new positions then sent to HBM (tests/loop_correction_leg.py)."""
    import os
    import subprocess
    import sys
    leg = os.path.join(os.path.dirname(os.path.abspath(__file__)), "loop_correction_leg.py")
    out = subprocess.run([sys.executable, leg], env=dict(os.environ, MORB_HOST_RESOLVE="1"), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "loop_correction_leg ok" in out.stdout, out.stdout + out.stderr
