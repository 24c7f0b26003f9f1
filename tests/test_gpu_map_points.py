"""GPU parity of the map-point refresh (orbm_refresh_points: MapPoint::ComputeDistinctiveDescriptors + UpdateNormalAndDepth for a
batch of points in one device call) with the model of tests/mappoint_model.py.  Every comparison is bit for bit on the whole
record array, every point, none left out; the conditions a world must meet are asserted on the model first."""
import ctypes as C
import os
import struct
import subprocess
import numpy as np
import pytest

import mappoint_model as mm
import mappoint_worlds as mw

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
WORLDS = [(500, 1), (4000, 2), (20000, 3)]


@pytest.fixture(scope="module")
def matcher():
    import multi_orb_slam_amd as m
    mt = m.Matcher(0.8, True)
    yield mt
    mt.close()


def expected_paths(b):
    counts = b.first[1:] - b.first[:-1]
    idle = (counts == 0) | (b.what == 0)
    return (int((~idle & (counts <= 16)).sum()), int((~idle & (counts > 16) & (counts <= 64)).sum()),
            int((~idle & (counts > 64) & (counts <= mw.CAP)).sum()), int((~idle & (counts > mw.CAP)).sum()), int(idle.sum()))


def run_and_compare(mt, b, rec):
    got = mt.RefreshPoints(b.native())
    paths = mt.last_refresh()
    print("refresh: %d points, %d observations -> paths (16-lane, wavefront, workgroup, host, idle) %s" % (b.n_points, b.n_obs, paths))
    assert paths == expected_paths(b)                    # the device for everything up to the cap, the host only beyond it
    for k in rec.dtype.names:
        bad = np.nonzero([got[k][i].tobytes() != rec[k][i].tobytes() for i in range(b.n_points)])[0]
        assert len(bad) == 0, (k, len(bad), bad[:8], got[k][bad[:3]], rec[k][bad[:3]], (b.first[1:] - b.first[:-1])[bad[:8]])
    assert got.tobytes() == rec.tobytes()
    return got


@pytest.mark.parametrize("n_points,seed", WORLDS)
def test_generated_worlds(matcher, n_points, seed):
    """500 / 4 000 / 20 000 points, observation counts 1 + geometric(0.12) capped at 300 with 0, 1, 2, 3, 16, 17, 64, 65, cap and cap + 1
    forced in, next to all-identical descriptors, a point whose observations are all dead, a camera centre equal to the position
    (a non-finite normal: the same bytes on both sides) and reference levels 0 and n_levels - 1."""
    b, forced = mw.make_world(n_points, seed)
    rec, n_alive, tied = mm.refresh(b)
    print(mw.check_conditions(b, forced, rec, n_alive, tied))            # before anything is compared
    paths = expected_paths(b)
    assert min(paths[:4]) >= 1 and paths[3] == int(((b.first[1:] - b.first[:-1]) > mw.CAP)[b.what != 0].sum())
    run_and_compare(matcher, b, rec)
    assert not np.isfinite(rec["normal"][forced["centre_at_pos"]]).any()
    # a second call on the same handle with other sizes in the scratch: the same bytes again
    small, sf = mw.make_world(64, seed + 10)
    run_and_compare(matcher, small, mm.refresh(small)[0])
    run_and_compare(matcher, b, rec)


def test_single_jobs_and_every_small_count(matcher):
    """Each job on its own over every observation count 0 .. 70 and around the cap, all alive and with dead ones."""
    rng = np.random.default_rng(9)
    counts = np.array(list(range(0, 71)) + [127, 128, 129, 255, 256, 257, 300], np.int64)
    for what in (1, 2, 3):
        for dead in (0.0, 0.3):
            b, _ = mw.make_world(len(counts), 40 + what)
            first = np.zeros(len(counts) + 1, np.int64); first[1:] = np.cumsum(counts)
            n_obs = int(first[-1])
            src = rng.integers(0, b.n_obs, n_obs)
            owner = np.repeat(np.arange(len(counts)), counts)
            nb = mw.Batch(first, b.obs_desc[src], b.pos[owner] + rng.normal(size=(n_obs, 3)).astype(np.float32) * 5, rng.random(n_obs) >= dead,
                          b.pos, b.ref_centre, b.ref_level, np.full(len(counts), what, np.uint8), b.scale_factors)
            rec = mm.refresh(nb)[0]
            run_and_compare(matcher, nb, rec)


def test_a_permuted_observation_list_changes_the_winner_of_a_tied_point(matcher):
    b, _ = mw.make_world(4000, 2)
    rec, _, tied = mm.refresh(b)
    got = run_and_compare(matcher, b, rec)
    pb, perm = b.permuted(np.random.default_rng(77))
    prec = mm.refresh(pb)[0]
    pgot = run_and_compare(matcher, pb, prec)
    produced = ((b.what & 1) != 0) & (got["best_obs"] >= 0)
    old_index = perm[pb.first[:-1][produced] + pgot["best_obs"][produced]] - b.first[:-1][produced]
    moved = old_index != got["best_obs"][produced]
    assert moved.sum() >= 10 and tied[produced][moved].all()             # the order did decide, and only between tied rows
    assert np.array_equal(pgot["best_median"], got["best_median"])


def test_device_equals_the_host_routine_and_argument_errors(matcher):
    import multi_orb_slam_amd as m
    from multi_orb_slam_amd import _lib
    b, _ = mw.make_world(500, 7)
    nb = b.native()
    assert matcher.RefreshPoints(nb).tobytes() == m.refresh_points_host(nb).tobytes()
    L = _lib.lib()
    out = np.zeros(b.n_points, m.REFRESH_DTYPE)
    assert L.orbm_refresh_points(None, C.byref(nb.c), _lib.ptr(out)) == _lib.ORB_E_ARG
    assert L.orbm_refresh_points(matcher._h, None, _lib.ptr(out)) == _lib.ORB_E_ARG
    assert L.orbm_refresh_points(matcher._h, C.byref(nb.c), None) == _lib.ORB_E_ARG
    for field, value in (("n_points", -1), ("n_obs", b.n_obs + 1), ("first", None), ("obs_centre", None), ("n_levels", 0), ("n_levels", 33),
                         ("ref_level", None)):
        bad = m.RefreshBatch(*[a.copy() for a in b.args()]); setattr(bad.c, field, value)
        assert L.orbm_refresh_points(matcher._h, C.byref(bad.c), _lib.ptr(out)) == _lib.ORB_E_ARG, field
    bad = m.RefreshBatch(*[a.copy() for a in b.args()]); bad.ref_level[30] = -1; bad.what[30] = 2
    assert L.orbm_refresh_points(matcher._h, C.byref(bad.c), _lib.ptr(out)) == _lib.ORB_E_ARG
    # no points, and points without any observation
    e = mw.Batch([0], np.zeros((0, 32), np.uint8), np.zeros((0, 3), np.float32), np.zeros(0, np.uint8), np.zeros((0, 3), np.float32),
                 np.zeros((0, 3), np.float32), np.zeros(0, np.int32), np.zeros(0, np.uint8), mw.scale_factors())
    assert len(matcher.RefreshPoints(e.native())) == 0
    e = mw.Batch([0, 0, 0, 0], np.zeros((0, 32), np.uint8), np.zeros((0, 3), np.float32), np.zeros(0, np.uint8), np.ones((3, 3), np.float32),
                 np.zeros((3, 3), np.float32), np.zeros(3, np.int32), np.array([1, 2, 3], np.uint8), mw.scale_factors())
    got = matcher.RefreshPoints(e.native())
    assert got["best_obs"].tolist() == [-1, 0, -1] and got.tobytes() == mm.refresh(e)[0].tobytes()
    assert matcher.last_refresh() == (0, 0, 0, 0, 3)
    # and after all that the handle still works
    run_and_compare(matcher, b, mm.refresh(b)[0])


# ---- the C++ class path (host/MapPointRefresh.h) ---------------------------------------------------------------------------------
def write_driver_world(path, b, ref_obs, bad_points):
    """The little-endian file host/test_refresh reads (format: the head of host/test_refresh.cc): the arrays of a Batch, one keyframe
    per observation; ref_obs[p] = the observation whose keyframe is the point's reference keyframe, or -1."""
    with open(path, "wb") as f:
        f.write(struct.pack("<iii", b.n_points, b.n_obs, len(b.scale_factors)))
        f.write(b.scale_factors.astype("<f4").tobytes())
        f.write(b.first.astype("<i4").tobytes()); f.write(np.asarray(ref_obs, "<i4").tobytes())
        f.write(b.obs_desc.tobytes()); f.write(b.obs_centre.astype("<f4").tobytes()); f.write(b.obs_alive.tobytes())
        f.write(b.pos.astype("<f4").tobytes()); f.write(b.ref_centre.astype("<f4").tobytes()); f.write(b.ref_level.astype("<i4").tobytes())
        f.write(np.asarray(bad_points, np.uint8).tobytes())


def test_cpp_driver_check(tmp_path):
    """host/test_refresh check on its own small map: RefreshMapPoints against a per-point restatement of the two reference functions."""
    drv = os.path.join(os.path.dirname(HERE), "multi_orb_slam_amd", "host", "test_refresh")
    assert os.path.exists(drv), "host driver not built (build())"
    out = subprocess.run([drv, "check"], capture_output=True, text=True, timeout=600)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "refresh check ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.parametrize("n_points,seed,what", [(500, 1, 3), (4000, 2, 3), (4000, 4, 1), (4000, 5, 2)])
def test_cpp_class_fills_the_map_points_with_the_models_bytes(tmp_path, n_points, seed, what):
    """RefreshMapPoints on a map built from a generated world: mDescriptor, mNormalVector, mfMinDistance and mfMaxDistance of every
    point are the model's bytes; a bad point and a point whose job did not run keep what they held."""
    drv = os.path.join(os.path.dirname(HERE), "multi_orb_slam_amd", "host", "test_refresh")
    assert os.path.exists(drv), "host driver not built (build())"
    b, forced = mw.make_world(n_points, seed)
    b.what[:] = what                                                     # the class runs the same jobs on every point of a call
    rng = np.random.default_rng(seed + 500)
    # the reference keyframe observes the point where the world's reference centre is the centre of one of its camera-1 observations
    # (the driver puts observation o into camera o % 2); otherwise a keyframe of its own (`observations[pRefKF]` inserts index 0)
    ref_obs = np.full(b.n_points, -1, np.int32)
    for p in range(b.n_points):
        hit = [o for o in range(b.first[p], b.first[p + 1]) if o % 2 == 0 and np.array_equal(b.obs_centre[o], b.ref_centre[p])]
        if hit:
            ref_obs[p] = hit[0]
    assert (ref_obs >= 0).sum() > 0.2 * b.n_points and (ref_obs < 0).sum() > 0.2 * b.n_points
    bad = (rng.random(b.n_points) < 0.05).astype(np.uint8)
    wpath = str(tmp_path / "world.bin"); opath = str(tmp_path / "out.bin")
    write_driver_world(wpath, b, ref_obs, bad)
    out = subprocess.run([drv, "world", wpath, opath, str(what)], capture_output=True, text=True, timeout=600)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "refresh world ok" in out.stdout, out.stdout + out.stderr
    rec = mm.refresh(b)[0]
    got = np.fromfile(opath, np.dtype([("desc", "u1", (32,)), ("normal", "<f4", (3,)), ("min_dist", "<f4"), ("max_dist", "<f4")]))
    assert len(got) == b.n_points
    counts = b.first[1:] - b.first[:-1]
    # what the driver put into every point beforehand and the reference leaves alone: descriptor of 0xAB bytes, normal (7, 8, 9), distances 11 / 12
    keep_desc = (bad != 0) | ((what & 1) == 0) | (rec["best_obs"] < 0)
    keep_nd = (bad != 0) | ((what & 2) == 0) | (counts == 0)
    exp = got.copy()
    exp["desc"] = np.where(keep_desc[:, None], np.uint8(0xAB), rec["desc"])
    exp["normal"] = np.where(keep_nd[:, None], np.array([7, 8, 9], np.float32)[None, :], rec["normal"])
    exp["min_dist"] = np.where(keep_nd, np.float32(11), rec["min_dist"]); exp["max_dist"] = np.where(keep_nd, np.float32(12), rec["max_dist"])
    assert (what & 1) == 0 or (~keep_desc).sum() > 0.8 * b.n_points
    assert (what & 2) == 0 or (~keep_nd).sum() > 0.8 * b.n_points
    for k in exp.dtype.names:
        assert got[k].tobytes() == exp[k].tobytes(), k


def test_the_staged_block_grows_and_is_reused_on_a_fresh_matcher():
    """A handle of its own, so that the staged block is reallocated inside the test: one point with one observation and the descriptor
    job alone, its per-point arrays of the normal / depth job ABSENT (NULL); then 300 points over the three size classes; then the
    first again.  Every call byte for byte the host routine, the two small calls each other."""
    import multi_orb_slam_amd as m
    b, _ = mw.make_world(300, 21)
    counts = b.first[1:] - b.first[:-1]
    one = b.subset([int(np.flatnonzero(counts >= 1)[0])])
    small = mw.Batch([0, 1], one.obs_desc[:1], one.obs_centre[:1], [1], one.pos, one.ref_centre, one.ref_level, [1], one.scale_factors).native()
    small.c.pos = None; small.c.ref_centre = None; small.c.ref_level = None
    large = b.native()
    paths = expected_paths(b)
    assert min(paths[:3]) >= 1                                           # <= 16, <= 64 and > 64 observations are all there
    mt = m.Matcher(0.8, True)
    try:
        want_small = m.refresh_points_host(small)
        first = mt.RefreshPoints(small)
        assert mt.last_refresh() == (1, 0, 0, 0, 0)
        assert first.tobytes() == want_small.tobytes() and first["best_obs"][0] == 0
        got = mt.RefreshPoints(large)
        assert mt.last_refresh() == paths
        assert got.tobytes() == m.refresh_points_host(large).tobytes() == mm.refresh(b)[0].tobytes()
        again = mt.RefreshPoints(small)
        assert again.tobytes() == want_small.tobytes() == first.tobytes()
    finally:
        mt.close()
