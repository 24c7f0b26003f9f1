"""The library's two host routines of the loop correction (orbm_local_map_correct_sim3_host, orbm_local_map_correct_rigid_host) against
the NumPy model of the reference's statements (tests/loopcorrect_model.py), bit for bit: the hand-built cases, whose expected values
are worked out by hand, and seeded worlds of 0 to 70 000 kept points that hold every class of point the loops distinguish
(tests/loopcorrect_worlds.py asserts that they do).  No GPU: the routines run on plain arrays."""
import numpy as np
import pytest

import loopcorrect_model as model
import loopcorrect_worlds as lw


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def host_sim3(w, cap=None):
    import multi_orb_slam_amd as m
    return m.local_map_correct_sim3_host(w["kf_rows"], w["kf_count"], w["flags"], w["pos"], w["kfs"], w["before"], w["after"], w["already"], cap)


def host_rigid(w, slots=None):
    import multi_orb_slam_amd as m
    return m.local_map_correct_rigid_host(w["pos"], w["flags"], w["ref"], slots, w["kf_corrected"], w["Tb"], w["Ta"], w["gba_slots"], w["gba_pos"])


def same_sim3(got, exp):
    ent, out, Tiw, new = got[:4]
    e_ent, e_out, e_Tiw, e_new = exp
    assert np.array_equal(np.stack([ent["point"], ent["position"]], axis=1).reshape(-1, 2), e_ent)
    assert np.array_equal(bits(out), bits(e_out)) and np.array_equal(bits(Tiw), bits(e_Tiw)) and np.array_equal(bits(new), bits(e_new))


def test_hand_built_sim3_case():
    h = lw.hand_sim3()
    ent, out, Tiw, new = model.correct_sim3(h["kf_rows"], h["kf_count"], h["flags"], h["pos"], h["kfs"], h["before"], h["after"], h["already"])
    assert np.array_equal(ent, h["exp_entries"]) and np.array_equal(out, h["exp_pos"]) and np.array_equal(Tiw, h["exp_Tiw"])
    assert np.array_equal(new[[1, 3]], h["pos"][[1, 3]])          # the bad point and the one already corrected stay
    same_sim3(host_sim3(h), (ent, out, Tiw, new))


def test_hand_built_rigid_case():
    h = lw.hand_rigid()
    st, out, new = model.correct_rigid(h["pos"], h["flags"], h["ref"], None, h["kf_corrected"], h["Tb"], h["Ta"], h["gba_slots"], h["gba_pos"])
    assert np.array_equal(st, h["exp_status"]) and np.array_equal(out, h["exp_pos"]) and np.array_equal(new, h["exp_pos"])
    g_st, g_out, g_new = host_rigid(h)
    assert np.array_equal(g_st, st) and np.array_equal(bits(g_out), bits(out)) and np.array_equal(bits(g_new), bits(new))


def test_model_inverse_and_map_compose_to_the_identity():
    """The model's own sanity: S.inverse().map(S.map(P)) is P to rounding, for any scale."""
    rng = np.random.default_rng(0)
    S = lw.random_sim3(rng, 50, False); P = rng.uniform(-10, 10, (50, 3))
    back = model.sim3_map(model.sim3_inverse(S), model.sim3_map(S, P))
    assert np.max(np.abs(back - P)) < 1e-12


@pytest.mark.parametrize("kept", lw.KEPT)
def test_sim3_worlds(kept):
    w, exp = lw.sim3_case(kept)
    got = host_sim3(w)
    print("sim3 world: %d keyframes listed, %d candidates, %d kept" % (len(w["kfs"]), int(w["kf_count"][w["kfs"]].sum()), len(got[0])))
    same_sim3(got, exp)


@pytest.mark.parametrize("variant", ["fixed", "same"])
def test_sim3_scale_one_and_equal_transforms(variant):
    """Scale 1 (the stereo loop's fixed scale) and before == after: equal to the MODEL, which need not return the input."""
    w, exp = lw.sim3_case(257, variant)
    assert np.all(w["after"][:, 7] == 1.0)
    same_sim3(host_sim3(w), exp)


@pytest.mark.parametrize("kept", [1, 65, 257])
def test_sim3_capacity_one_short_changes_nothing(kept):
    import multi_orb_slam_amd as m
    from multi_orb_slam_amd import _lib
    w, exp = lw.sim3_case(kept)
    with pytest.raises(m.OrbError) as e:
        host_sim3(w, cap=kept - 1)
    assert e.value.code == _lib.ORB_E_CAPACITY and e.value.needed == kept and str(kept) in str(e.value)
    # the wrapper works on a copy; the routine itself must leave ITS array alone: call it on one we keep
    from multi_orb_slam_amd._lib import ptr
    import ctypes as C
    P = w["pos"].copy(); n = C.c_int(); ent = np.zeros(kept, m.CORRECT_DTYPE); out = np.zeros((kept, 3), np.float32)
    tiw = np.zeros((len(w["kfs"]), 16), np.float32)
    rc = _lib.lib().orbm_local_map_correct_sim3_host(ptr(w["kf_rows"]), ptr(w["kf_count"]), w["n_kfs"], w["stride"], ptr(w["flags"]), ptr(P), 3,
                                                     w["n_points"], ptr(w["kfs"]), len(w["kfs"]), ptr(w["before"]), ptr(w["after"]),
                                                     ptr(w["already"]), len(w["already"]), ptr(ent), ptr(out), kept - 1, C.byref(n), ptr(tiw))
    assert rc == _lib.ORB_E_CAPACITY and n.value == kept and np.array_equal(bits(P), bits(w["pos"]))
    same_sim3(host_sim3(w, cap=kept), exp)                       # and exactly enough room is enough


@pytest.mark.parametrize("changed", lw.KEPT)
def test_rigid_worlds(changed):
    w, exp = lw.rigid_case(changed)
    st, out, new = host_rigid(w)
    print("rigid world: %d points, %d changed (%d given, %d moved)" % (w["n_points"], int((st != 0).sum()), int((st == 1).sum()), int((st == 2).sum())))
    assert np.array_equal(st, exp[0]) and np.array_equal(bits(out), bits(exp[1])) and np.array_equal(bits(new), bits(exp[2]))


def test_rigid_over_a_list_of_slots():
    """A scattered list of slots: status and pos_out follow the list, points outside it stay."""
    w, _ = lw.rigid_case(257)
    rng = np.random.default_rng(9)
    slots = rng.permutation(w["n_points"])[:w["n_points"] // 2].astype(np.int32)
    exp = model.correct_rigid(w["pos"], w["flags"], w["ref"], slots, w["kf_corrected"], w["Tb"], w["Ta"], w["gba_slots"], w["gba_pos"])
    st, out, new = host_rigid(w, slots)
    assert (st != 0).sum() > 50 and np.array_equal(st, exp[0]) and np.array_equal(bits(out), bits(exp[1])) and np.array_equal(bits(new), bits(exp[2]))
    rest = np.setdiff1d(np.arange(w["n_points"]), slots)
    assert np.array_equal(bits(new[rest]), bits(w["pos"][rest]))


def test_argument_errors_of_the_host_routines():
    import multi_orb_slam_amd as m
    from multi_orb_slam_amd import _lib
    h = lw.hand_rigid()
    with pytest.raises(m.OrbError) as e:                            # a slot named twice
        host_rigid(h, [0, 1, 0])
    assert e.value.code == _lib.ORB_E_ARG
    with pytest.raises(m.OrbError) as e:                            # a slot outside the points
        host_rigid(h, [7])
    assert e.value.code == _lib.ORB_E_ARG
    s = lw.hand_sim3()
    with pytest.raises(m.OrbError) as e:                            # a keyframe outside the rows
        m.local_map_correct_sim3_host(s["kf_rows"], s["kf_count"], s["flags"], s["pos"], [2], s["before"][:1], s["after"][:1], cap=8)
    assert e.value.code == _lib.ORB_E_ARG
