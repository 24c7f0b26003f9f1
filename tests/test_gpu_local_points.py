"""GPU parity of local-map tracking on the device (orbm_search_local_points over an HBM-resident point table) with the model
of tests/frustum_model.py and the CPU oracle's SearchByProjection(F, vpMapPoints, th) fed with the model's queries in table
order.  Every comparison is bit for bit: orbm_track as raw bytes, match_of_feature, both counts.  No point is left out of a
comparison (the records of points that are not in view are all zero on both sides)."""
import os
import subprocess
import sys
import numpy as np
import pytest

import oracle
import frustum_model as fm
import frustum_worlds as fw

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def matcher():
    import multi_orb_slam_amd as m
    mt = m.Matcher(0.8, True)
    yield mt
    mt.close()


def run_and_compare(mt, F, OF, pts, points, view, skip=None, occupied=None, n=None, want_device_path=True):
    """One call against model + oracle; returns what was expected (n_to_match, nmatches, match_of_feature, track, verdict)."""
    n = len(points) if n is None else n
    exp = fm.expected_search(OF, points[:n], view, None if skip is None else skip[:n], occupied, mt.nnratio, 100)
    e_ntm, e_nm, e_mo, e_track, _ = exp
    ntm, nm, mo, track = mt.SearchLocalPoints(F, pts, view.native(), skip, occupied, n=n)
    print("local points: n %d features %d -> in view %d (expected %d), matches %d (expected %d), resolve %s"
          % (n, OF.n_total, ntm, e_ntm, nm, e_nm, mt.last_resolve()))
    if want_device_path and n > 0 and OF.n_total > 0:
        assert mt.last_resolve()[0] == 0, mt.last_resolve()          # resolved on the device, not by the host fallback
    assert ntm == e_ntm and nm == e_nm
    assert np.array_equal(track["in_view"], e_track["in_view"])
    assert track.tobytes() == e_track.tobytes()
    assert np.array_equal(mo, e_mo)
    return exp


@pytest.mark.parametrize("case", fw.CASES, ids=lambda c: "%dpts_%dx%d_th%g" % (c[0], c[1][0], c[1][1], c[5]))
def test_generated_worlds(matcher, case):
    """500 / 2 000 / 8 000 / 16 384 points against frames of [1000, 500] and [2000, 2000] features, th 1, 3, 5: points made by
    back-projecting frame features at random depth with perturbed descriptors, plus points behind the camera, outside the image,
    out of the distance band and at grazing normals."""
    import multi_orb_slam_amd as m
    w = fw.make_world(*case)
    OF = oracle.FrameData(**w["fr"])
    fw.check_conditions(w, *fm.expected_search(OF, w["points"], w["view"], None, None, matcher.nnratio, 100))   # before anything is compared
    F = matcher.frame(m.FrameData(**w["fr"]))
    with m.LocalPoints(matcher, case[0]) as pts:
        pts.write(0, w["points"])
        assert pts.count == case[0]
        run_and_compare(matcher, F, OF, pts, w["points"], w["view"])
        # skip, occupied and a different ratio in use; the same table, a second call
        rng = np.random.default_rng(case[4] + 50)
        skip = (rng.random(case[0]) < 0.15).astype(np.uint8)
        occ = (rng.random(OF.n_total) < 0.15).astype(np.uint8)
        matcher.nnratio = 0.6
        try:
            e = run_and_compare(matcher, F, OF, pts, w["points"], w["view"], skip, occ)
            assert (e[4] == fm.SKIPPED).sum() > 0
            assert e[1] >= 0.25 * min(e[0], int((occ[:case[1][0]] == 0).sum()))   # the floor of the conditions, over the features left free
            assert not np.any(occ[e[2] >= 0])                       # an occupied feature takes no point
        finally:
            matcher.nnratio = 0.8
    F.close()


@pytest.mark.parametrize("th", [1.0, 3.0])
def test_points_on_every_decision_boundary(matcher, th):
    """Points the model has moved onto its own decision boundaries, both sides of each (one ulp apart): image edges, both ends of
    the distance band, the viewing-angle limit, the radius class, the depth sign (where the projection overflows: the documented
    deviation), and max_dist within +-2 ulps of where the ratio crosses every level threshold."""
    import multi_orb_slam_amd as m
    b = fw.make_boundary_world([1000, 500], 640, 480, 11, th)
    verdict, track, _, keep = fm.frustum(b["points"], b["view"])
    kinds = set(b["kinds"].tolist())
    assert {"u_min", "u_max", "v_min", "v_max", "too_near", "too_far", "grazing", "radius", "behind"} <= kinds
    for k in range(fw.N_LEVELS - 1):
        assert set(track["level"][b["kinds"] == "level%d" % k].tolist()) == {k, k + 1}
    assert (verdict == fm.NONFINITE).sum() > 0
    OF = oracle.FrameData(**b["fr"]); F = matcher.frame(m.FrameData(**b["fr"]))
    fw.check_conditions(b, *fm.expected_search(OF, b["points"], b["view"], None, None, matcher.nnratio, 100))
    with m.LocalPoints(matcher, len(b["points"])) as pts:
        pts.write(0, b["points"])
        run_and_compare(matcher, F, OF, pts, b["points"], b["view"])
    F.close()


def test_contested_features_go_to_the_first_point_in_table_order(matcher):
    """Six points onto each of 150 features, descriptors at different distances: whoever comes first in the TABLE claims the feature
    (reference src/ORBmatcher.cc:143 seen by later points at :107-109), so the reversed table gives a different assignment."""
    import multi_orb_slam_amd as m
    w = fw.make_world(2000, [1000, 500], 640, 480, 21, 3.0)
    verdict = fm.frustum(w["points"], w["view"])[0]
    good = np.nonzero(verdict == fm.IN_VIEW)[0][:150]
    base = w["points"][good]
    rng = np.random.default_rng(5)
    tab = np.repeat(base, 6)
    flips = rng.integers(0, 256, (len(tab), 3))
    for i in range(len(tab)):                                   # up to three flipped bits: near-ties between the six
        for bit in flips[i][: i % 4]:
            tab["desc"][i][bit // 8] ^= np.uint8(1 << (bit % 8))
    tab["blocks"] = 1
    tab = tab[rng.permutation(len(tab))]
    OF = oracle.FrameData(**w["fr"]); F = matcher.frame(m.FrameData(**w["fr"]))
    with m.LocalPoints(matcher, len(tab)) as pts:
        pts.write(0, tab)
        fwd = run_and_compare(matcher, F, OF, pts, tab, w["view"])
        pts.write(0, tab[::-1].copy())
        rev = run_and_compare(matcher, F, OF, pts, tab[::-1].copy(), w["view"])
    matched = fwd[2] >= 0
    assert matched.sum() >= 40
    assert np.any((len(tab) - 1 - rev[2][matched]) != fwd[2][matched])   # the order did decide
    F.close()


def test_partial_writes_smaller_n_empty_inputs(matcher):
    import multi_orb_slam_amd as m
    w = fw.make_world(2000, [1000, 500], 640, 480, 31, 3.0)
    w2 = fw.make_world(2000, [1000, 500], 640, 480, 32, 3.0)       # (same frame size, other points)
    OF = oracle.FrameData(**w["fr"]); F = matcher.frame(m.FrameData(**w["fr"]))
    with m.LocalPoints(matcher, 2500) as pts:
        assert pts.count == 0
        pts.write(0, w["points"])
        first = run_and_compare(matcher, F, OF, pts, w["points"], w["view"])
        # rows 300..899 and 1500..1503 replaced between two calls == a fresh table with the same content
        mixed = w["points"].copy()
        mixed[300:900] = w2["points"][300:900]; mixed[1500:1504] = w2["points"][10:14]
        pts.write(300, mixed[300:900]); pts.write(1500, mixed[1500:1504])
        assert pts.count == 2000
        second = run_and_compare(matcher, F, OF, pts, mixed, w["view"])
        assert not np.array_equal(first[2], second[2])
        with m.LocalPoints(matcher, 2000) as fresh:
            fresh.write(0, mixed)
            got = matcher.SearchLocalPoints(F, fresh, w["view"].native())
        assert got[0] == second[0] and got[1] == second[1] and np.array_equal(got[2], second[2]) and got[3].tobytes() == second[3].tobytes()
        # n smaller than the table: the rows beyond n do not exist for the call
        for n in (1, 777, 1999):
            run_and_compare(matcher, F, OF, pts, mixed, w["view"], n=n)
        # n = 0
        ntm, nm, mo, track = matcher.SearchLocalPoints(F, pts, w["view"].native(), n=0)
        assert (ntm, nm) == (0, 0) and np.all(mo == -1) and len(track) == 0
        # rows written beyond the old high-water mark, with a gap: the gap reads as zeroed points (never in view)
        pts.write(2100, w2["points"][:50])
        assert pts.count == 2150
        gap = np.concatenate([mixed, np.zeros(100, mixed.dtype), w2["points"][:50]])
        run_and_compare(matcher, F, OF, pts, gap, w["view"])
        # an empty frame: the frustum half still runs
        empty = dict(w["fr"]); n0 = 0
        for k in ("un_x", "un_y", "octave", "angle", "uright", "cam_of", "local_of"):
            empty[k] = empty[k][:0]
        empty["descs"] = [d[:0] for d in empty["descs"]]
        FE = matcher.frame(m.FrameData(**empty))
        ntm, nm, mo, track = matcher.SearchLocalPoints(FE, pts, w["view"].native(), n=2000)
        e_track = fm.frustum(mixed, w["view"])[1]
        assert ntm == second[0] and nm == 0 and len(mo) == 0 and track.tobytes() == e_track.tobytes()
        FE.close()
    F.close()


def test_zero_depth_point_is_out_of_view_and_changes_nothing_else(matcher):
    """PcZ == 0: u, v are infinite or NaN; the reference lets them through its bound checks into an int cast.  Here the point is
    out of view, and every other row is what it is with a point behind the camera in its place."""
    import multi_orb_slam_amd as m
    w = fw.make_world(2000, [1000, 500], 640, 480, 41, 3.0)
    V = w["view"]
    tab = w["points"].copy()
    # points in the camera's z = 0 plane: P = Ow + a * (row 0 of R) + b * (row 1 of R), rounded; keep those whose PcZ is exactly 0
    R = V.Rcw.astype(np.float64)
    cands = []
    rng = np.random.default_rng(3)
    for _ in range(4000):
        a, b_ = rng.uniform(-3, 3, 2)
        P = (V.Ow.astype(np.float64) + a * R[0] + b_ * R[1]).astype(np.float32)
        t = np.float32(np.float32(V.Rcw[2, 0] * P[0] + V.Rcw[2, 1] * P[1]) + np.float32(V.Rcw[2, 2] * P[2]))
        if np.float32(np.float64(t) + np.float64(V.tcw[2])) == 0.0:
            cands.append(P)
    cands.append(V.Ow.copy())                                         # the camera centre itself, if its PcZ rounds to 0
    rows = np.arange(100, 100 + len(cands))
    tab["pos"][rows] = np.array(cands, np.float32)
    tab["min_dist"][rows] = 0.0; tab["max_dist"][rows] = 100.0
    verdict = fm.frustum(tab, V)[0]
    assert (verdict[rows] == fm.NONFINITE).sum() >= 1, "no point with PcZ == 0 could be constructed"
    zero = rows[verdict[rows] == fm.NONFINITE]
    OF = oracle.FrameData(**w["fr"]); F = matcher.frame(m.FrameData(**w["fr"]))
    with m.LocalPoints(matcher, len(tab)) as pts:
        pts.write(0, tab)
        with_zero = run_and_compare(matcher, F, OF, pts, tab, V)
        assert np.all(with_zero[3]["in_view"][zero] == 0)
        ref = tab.copy()
        ref["pos"][zero] = w["points"]["pos"][np.nonzero(fm.frustum(w["points"], V)[0] == fm.BEHIND)[0][0]]
        pts.write(0, ref)
        without = run_and_compare(matcher, F, OF, pts, ref, V)
    assert with_zero[0] == without[0] and with_zero[1] == without[1]
    assert np.array_equal(with_zero[2], without[2]) and with_zero[3].tobytes() == without[3].tobytes()
    F.close()


def test_argument_errors(matcher):
    import ctypes as C
    import multi_orb_slam_amd as m
    from multi_orb_slam_amd import _lib
    w = fw.make_world(500, [1000, 500], 640, 480, 1, 3.0)
    F = matcher.frame(m.FrameData(**w["fr"]))
    L = _lib.lib()
    with pytest.raises(m.OrbError) as e:
        m.LocalPoints(matcher, 65536)
    assert e.value.code == _lib.ORB_E_CAPACITY
    with pytest.raises(m.OrbError) as e:
        m.LocalPoints(matcher, -1)
    assert e.value.code == _lib.ORB_E_ARG
    with m.LocalPoints(matcher, 600) as pts:
        pts.write(0, w["points"])
        with pytest.raises(m.OrbError) as e:
            pts.write(200, w["points"])                              # 200 + 500 > 600
        assert e.value.code == _lib.ORB_E_CAPACITY
        with pytest.raises(m.OrbError) as e:
            pts.write(-1, w["points"][:3])
        assert e.value.code == _lib.ORB_E_ARG
        assert pts.count == 500
        view = w["view"].native()
        with pytest.raises(m.OrbError) as e:                          # more points than were ever written: loud, not truncated
            matcher.SearchLocalPoints(F, pts, view, n=501)
        assert e.value.code == _lib.ORB_E_CAPACITY
        with pytest.raises(m.OrbError) as e:
            matcher.SearchLocalPoints(F, pts, view, n=-1)
        assert e.value.code == _lib.ORB_E_ARG
        mo = np.zeros(F.data.n_total, np.int32); a = C.c_int(); b = C.c_int()
        args = lambda v, ntm=C.byref(a): (matcher._h, F._h, pts._h, 500, v, None, None, C.c_float(0.8), 100, None, _lib.ptr(mo), ntm, C.byref(b))
        assert L.orbm_search_local_points(*args(None)) == _lib.ORB_E_ARG                  # no view
        assert L.orbm_search_local_points(*args(C.byref(view.c), None)) == _lib.ORB_E_ARG  # no n_to_match
        for levels in (0, 33):
            bad = w["view"].native(); bad.c.n_levels = levels
            assert L.orbm_search_local_points(*args(C.byref(bad.c))) == _lib.ORB_E_ARG
        bad = w["view"].native(); bad.c.log_scale_factor = 0.0
        assert L.orbm_search_local_points(*args(C.byref(bad.c))) == _lib.ORB_E_ARG
        bad = w["view"].native(); bad.c.scale_factors = None
        assert L.orbm_search_local_points(*args(C.byref(bad.c))) == _lib.ORB_E_ARG
        other = m.Matcher(0.8, True)                                  # a table belongs to the handle that made it
        try:
            with pytest.raises(m.OrbError) as e:
                other.SearchLocalPoints(F, pts, view)
            assert e.value.code == _lib.ORB_E_ARG
        finally:
            other.close()
        # and after all that the table still works
        OF = oracle.FrameData(**w["fr"])
        run_and_compare(matcher, F, OF, pts, w["points"], w["view"])
    F.close()


@pytest.mark.parametrize("case_index", [1])
def test_host_fallback_gives_the_same_bytes(case_index):
    """The exact fallback search_finish takes when the device resolve does not converge, forced with MORB_HOST_RESOLVE=1 (read in
    orbm_create, hence a fresh child process): the queries are rebuilt on the host from the table's mirror."""
    out = subprocess.run([sys.executable, os.path.join(HERE, "local_points_leg.py"), str(case_index)],
                         env=dict(os.environ, MORB_HOST_RESOLVE="1"), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "local_points_leg ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.parametrize("case_index", [1, 3])
def test_cpp_class_against_host_restatement_and_model(tmp_path, case_index):
    """host/test_local_points check: SearchLocalPoints (LocalMapSearch.h) against Frame::isInFrustum per point + the existing
    ORBmatcher::SearchByProjection(F, points, th) -- every scratch field, mnVisible, F.mvpMapPoints, both counts, on two frames -- and
    what the class left behind against the model + oracle as well.  Bad points and points the frame already holds are in use."""
    drv = os.path.join(os.path.dirname(HERE), "multi_orb_slam_amd", "host", "test_local_points")
    assert os.path.exists(drv), "host driver not built (build())"
    case = fw.CASES[case_index]
    w = fw.make_world(*case)
    n = case[0]; N = case[1][0]
    rng = np.random.default_rng(case_index + 900)
    bad = (rng.random(n) < 0.05).astype(np.int32)
    feats = rng.permutation(N)[: N // 10]; owners = rng.permutation(n)[: N // 10]
    pre = list(zip(feats.tolist(), owners.tolist()))
    wpath = str(tmp_path / "world.bin"); opath = str(tmp_path / "out.bin")
    fw.write_driver_world(wpath, w, bad, pre)
    out = subprocess.run([drv, "check", wpath, opath], capture_output=True, text=True, timeout=600)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "local_points check ok" in out.stdout, out.stdout + out.stderr
    # the same under the model: loop 1 nulls the bad pre-matched points and takes the others out of the search
    skip = bad.astype(np.uint8).copy()
    occ = np.zeros(len(w["fr"]["un_x"]), np.uint8)
    held = np.full(N, -1, np.int32)
    for g, p in pre:
        if not bad[p]:
            skip[p] = 1; held[g] = p
            occ[g] = 1 if w["points"]["blocks"][p] else 0
    e_ntm, e_nm, e_mo, e_track, _ = fm.expected_search(oracle.FrameData(**w["fr"]), w["points"], w["view"], skip, occ, 0.8, 100)
    ntm, nm, pts, feat = fw.read_driver_out(opath, n, N)
    assert (ntm, nm) == (e_ntm, e_nm) and e_nm > 0
    live = skip == 0
    assert np.array_equal(pts["in_view"][live], e_track["in_view"][live])
    iv = live & (e_track["in_view"] != 0)
    for k in ("proj_x", "proj_y", "proj_xr", "view_cos", "level"):
        assert pts[k][iv].tobytes() == e_track[k][iv].tobytes(), k
    exp_feat = np.where(e_mo[:N] >= 0, e_mo[:N], held)
    assert np.array_equal(feat, exp_feat)
    # mnVisible: 1 at construction, +1 for a point the frame held, +1 for a point in view
    exp_vis = 1 + iv.astype(np.int32)
    for g, p in pre:
        if not bad[p]:
            exp_vis[p] += 1
    assert np.array_equal(pts["visible"], exp_vis)
