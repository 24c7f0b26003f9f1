"""The NumPy model of the map-point refresh (tests/mappoint_model.py) against the library's host routine
(orbm_refresh_points_host: the statement sequence the kernels share), bit for bit, and against known answers.  No device needed."""
import ctypes as C
import numpy as np
import pytest

import mappoint_model as mm
import mappoint_worlds as mw


def host(batch):
    import multi_orb_slam_amd as m
    return m.refresh_points_host(batch.native())


def one_point(descs, alive=None, what=3, centres=None, pos=(1.0, 2.0, 3.0), ref=(0.0, 0.0, 0.0), level=2):
    n = len(descs)
    centres = np.zeros((n, 3), np.float32) if centres is None else centres
    return mw.Batch([0, n], np.asarray(descs, np.uint8).reshape(n, 32), centres, np.ones(n, np.uint8) if alive is None else alive,
                    [pos], [ref], [level], [what], mw.scale_factors())


def with_bits(k, start=0):
    """A descriptor with bits start .. start+k-1 set."""
    bits = np.zeros(256, np.uint8); bits[start:start + k] = 1
    return np.packbits(bits)


@pytest.mark.parametrize("n_points,seed", [(500, 1), (4000, 2), (20000, 3)])
def test_model_equals_the_host_routine_on_the_generated_worlds(n_points, seed):
    b, forced = mw.make_world(n_points, seed)
    rec, n_alive, tied = mm.refresh(b)
    print(mw.check_conditions(b, forced, rec, n_alive, tied))
    got = host(b)
    for k in rec.dtype.names:
        assert got[k].tobytes() == rec[k].tobytes(), k
    assert got.tobytes() == rec.tobytes()
    # the same lists in another order: same bytes again, and the order does decide between tied rows
    pb, perm = b.permuted(np.random.default_rng(seed + 100))
    prec, _, ptied = mm.refresh(pb)
    assert host(pb).tobytes() == prec.tobytes()
    produced = ((b.what & 1) != 0) & (rec["best_obs"] >= 0)
    old_index = perm[pb.first[:-1][produced] + prec["best_obs"][produced]] - b.first[:-1][produced]
    moved = old_index != rec["best_obs"][produced]
    assert moved.any() and tied[produced][moved].all()         # another winner only where the least median was tied
    assert np.array_equal(prec["best_median"], rec["best_median"])


def test_one_and_two_observations_the_first_wins_with_median_zero():
    """N = 1 and N = 2: the median index (int)(0.5*(N-1)) is 0, every sorted row starts with its own zero."""
    a, b = with_bits(40), with_bits(90, 100)
    for descs in ([a], [a, b], [b, a]):
        bt = one_point(descs, centres=np.array([[0, 0, 0]] * len(descs), np.float32))
        for rec in (mm.refresh(bt)[0], host(bt)):
            assert rec["best_obs"][0] == 0 and rec["best_median"][0] == 0
            assert rec["desc"][0].tobytes() == descs[0].tobytes()


def test_known_answer_three_on_a_line():
    """Distances 10 / 30 / 40: the medians (index 1 of each sorted row) are 10, 10, 30 -- rows 0 and 1 tie, the lower index wins."""
    descs = [with_bits(10), with_bits(0), with_bits(30, 10)]          # d01 = 10, d12 = 30, d02 = 40
    assert mm.hamming_matrix(descs).tolist() == [[0, 10, 40], [10, 0, 30], [40, 30, 0]]
    assert mm.row_medians(descs).tolist() == [10, 10, 30]
    bt = one_point(descs)
    for rec in (mm.refresh(bt)[0], host(bt)):
        assert rec["best_obs"][0] == 0 and rec["best_median"][0] == 10
    bt = one_point([descs[2], descs[1], descs[0]])                     # reversed: medians 30, 10, 10 -> row 1
    for rec in (mm.refresh(bt)[0], host(bt)):
        assert rec["best_obs"][0] == 1 and rec["best_median"][0] == 10 and rec["desc"][0].tobytes() == descs[1].tobytes()
    # a dead observation takes no part: of the line only 10 / 40 remain, N = 2, the first ALIVE one wins, reported by list position
    bt = one_point([descs[1], descs[0], descs[2]], alive=np.array([0, 1, 1], np.uint8))
    for rec in (mm.refresh(bt)[0], host(bt)):
        assert rec["best_obs"][0] == 1 and rec["best_median"][0] == 0


def test_normal_and_depth_known_answers():
    """One observer on the x axis: the normal is the unit x vector; 3-4-5 triangle to the reference camera."""
    s = mw.scale_factors()
    bt = one_point([with_bits(1)], centres=np.array([[-4.0, 2.0, 3.0]], np.float32), pos=(1.0, 2.0, 3.0), ref=(1.0, -1.0, 7.0), level=3)
    for rec in (mm.refresh(bt)[0], host(bt)):
        assert rec["normal"][0].tolist() == [1.0, 0.0, 0.0]
        assert rec["max_dist"][0] == np.float32(5.0) * s[3] and rec["min_dist"][0] == np.float32(np.float32(5.0) * s[3]) / s[7]
    # two observers at right angles: (1, 0, 0) + (0, 1, 0), halved
    bt = one_point([with_bits(1), with_bits(2)], centres=np.array([[-1.0, 2.0, 3.0], [1.0, -2.0, 3.0]], np.float32))
    for rec in (mm.refresh(bt)[0], host(bt)):
        assert rec["normal"][0].tolist() == [0.5, 0.5, 0.0]
    # jobs that were not asked for leave zeros
    for what, zero in ((1, ("normal", "min_dist", "max_dist")), (2, ("desc", "best_obs", "best_median")), (0, rec.dtype.names)):
        bt = one_point([with_bits(1), with_bits(2)], what=what, centres=np.array([[-1.0, 2.0, 3.0], [1.0, -2.0, 3.0]], np.float32))
        m_rec, h_rec = mm.refresh(bt)[0], host(bt)
        assert m_rec.tobytes() == h_rec.tobytes()
        for k in zero:
            assert not np.asarray(h_rec[k]).any(), (what, k)


def test_argument_errors_of_the_host_routine():
    import multi_orb_slam_amd as m
    from multi_orb_slam_amd import _lib
    L = _lib.lib()
    b, _ = mw.make_world(64, 5)
    out = np.zeros(b.n_points, m.REFRESH_DTYPE)

    def rc(change):
        nb = m.RefreshBatch(*[a.copy() for a in b.args()]); change(nb)      # (copies: the changes stay in this call)
        return L.orbm_refresh_points_host(C.byref(nb.c), _lib.ptr(out))
    assert rc(lambda nb: None) == _lib.ORB_OK
    assert L.orbm_refresh_points_host(None, _lib.ptr(out)) == _lib.ORB_E_ARG
    assert L.orbm_refresh_points_host(C.byref(b.native().c), None) == _lib.ORB_E_ARG
    assert rc(lambda nb: setattr(nb.c, "n_points", -1)) == _lib.ORB_E_ARG
    assert rc(lambda nb: setattr(nb.c, "n_obs", nb.c.n_obs - 1)) == _lib.ORB_E_ARG          # first[P] != n_obs
    assert rc(lambda nb: setattr(nb.c, "obs_desc", None)) == _lib.ORB_E_ARG
    assert rc(lambda nb: setattr(nb.c, "n_levels", 0)) == _lib.ORB_E_ARG
    assert rc(lambda nb: setattr(nb.c, "n_levels", 33)) == _lib.ORB_E_ARG
    assert rc(lambda nb: setattr(nb.c, "scale_factors", None)) == _lib.ORB_E_ARG

    def bad_first(nb):
        nb.first[3], nb.first[4] = nb.first[4] + 1, nb.first[3]
    assert rc(bad_first) == _lib.ORB_E_ARG

    def bad_level(nb):
        nb.ref_level[20] = mw.N_LEVELS
        nb.what[20] = 3
    assert rc(bad_level) == _lib.ORB_E_ARG

    def bad_what(nb):
        nb.what[7] = 4
    assert rc(bad_what) == _lib.ORB_E_ARG
    assert "what[7]" in L.orb_last_error().decode()
    # no points at all is legal
    e = mw.Batch([0], np.zeros((0, 32), np.uint8), np.zeros((0, 3), np.float32), np.zeros(0, np.uint8), np.zeros((0, 3), np.float32),
                 np.zeros((0, 3), np.float32), np.zeros(0, np.int32), np.zeros(0, np.uint8), mw.scale_factors())
    assert len(host(e)) == 0
