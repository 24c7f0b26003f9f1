"""The NumPy model of the triangulation stage (tests/triangulate_model.py) against the library's host routine
(orbv_triangulate_pairs_host: the statement sequence the kernel shares), byte for byte, against known answers, and -- the model's SVD
only -- against LAPACK.  No device needed."""
import ctypes as C

import numpy as np
import pytest

import triangulate_model as tm
import triangulate_worlds as tw


def lib():
    from multi_orb_slam_amd import _lib
    return _lib


def test_record_layout_is_the_abi_struct():
    import multi_orb_slam_amd as m
    assert m.TRI_OUT_DTYPE.itemsize == 20 and m.TRI_OUT_DTYPE == tm.RECORD
    assert [m.TRI_OUT_DTYPE.fields[k][1] for k in ("x3D", "outcome", "path")] == [0, 12, 16]


def test_the_worlds_meet_their_condition():
    print(tw.check_conditions([tw.world_and_model(name)[1] for name in tw.WORLDS]))


@pytest.mark.parametrize("name", list(tw.WORLDS))
def test_model_equals_the_host_routine_on_the_generated_worlds(name):
    w, rec = tw.world_and_model(name)
    got = w.host()
    for k in rec.dtype.names:
        assert got[k].tobytes() == rec[k].tobytes(), k
    assert got.tobytes() == rec.tobytes()
    # the same pairs in another order: pairs are independent, the records move with them
    perm = np.random.default_rng(5).permutation(len(w.pairs))
    assert w.host(w.pairs[perm]).tobytes() == rec[perm].tobytes()
    assert w.model(w.pairs[perm[:200]]).tobytes() == rec[perm[:200]].tobytes()


@pytest.mark.parametrize("enabled", [(1, 0), (0, 1)])
def test_exactly_one_camera_off(enabled):
    w, rec = tw.world_and_model("25cm")
    off = tw.World(w.kf1, w.kf2, w.pairs, cam_enabled=enabled)
    got = off.host()
    cam = w.kf1.cam_of[w.pairs[:, 0]]
    dropped = cam == (0 if enabled[0] == 0 else 1)
    assert dropped.any() and (~dropped).any()
    assert (got["outcome"][dropped] == tm.CAM_OFF).all() and not got["x3D"][dropped].any() and not got["path"][dropped].any()
    assert got[~dropped].tobytes() == rec[~dropped].tobytes()
    assert off.model(w.pairs[:300]).tobytes() == got[:300].tobytes()


def test_hand_built_pairs_reach_the_two_degenerate_exits():
    for name, (w, outcome, path) in tw.hand_built().items():
        for rec in (w.model(), w.host()):
            assert (rec["outcome"][0], rec["path"][0]) == (outcome, path), name
        assert w.model().tobytes() == w.host().tobytes(), name
    w = tw.w_zero_world()
    assert w.host()["x3D"][0].tolist() == [1.0, 0.0, 0.0]          # the null vector itself: (1, 0, 0, 0)


def test_known_answer_exact_integer_geometry():
    """The point (1, 2, 4) seen from the origin and from 1/32 m to its right, f = 512: a stereo feature of keyframe 1 is unprojected
    to exactly (1, 2, 4) and passes every gate with zero error; seen from 1/4 m the linear triangulation runs and lands within float
    rounding of it."""
    for rec in (tw.exact_world().model(), tw.exact_world().host()):
        assert rec["x3D"][0].tolist() == [1.0, 2.0, 4.0] and rec["outcome"][0] == tm.ACCEPTED and rec["path"][0] == tm.PATH_UNPROJECT1
    # no depth in keyframe 1, depth in keyframe 2: unprojected from there, (0.96875, 2, 4) + its centre (0.03125, 0, 0)
    w = tw.exact_world(stereo1=False, stereo2=True)
    for rec in (w.model(), w.host()):
        assert rec["x3D"][0].tolist() == [1.0, 2.0, 4.0] and rec["outcome"][0] == tm.ACCEPTED and rec["path"][0] == tm.PATH_UNPROJECT2
    # no depth at all and rays this close to parallel (cos > 0.9998): "no stereo and very low parallax"
    w = tw.exact_world(stereo1=False, stereo2=False)
    for rec in (w.model(), w.host()):
        assert rec["outcome"][0] == tm.LOW_PARALLAX and rec["path"][0] == tm.PATH_NONE and not rec["x3D"][0].any()
    w = tw.exact_world(stereo1=False, stereo2=False, baseline=0.25)
    for rec in (w.model(), w.host()):
        assert rec["outcome"][0] == tm.ACCEPTED and rec["path"][0] == tm.PATH_SVD
        assert np.abs(rec["x3D"][0] - np.array([1, 2, 4], np.float32)).max() <= 4 * 2.0 ** -21    # 4 ulp of 4.0
    # the reprojection gates are strict `>`: one pixel off in keyframe 2 is 1 > 5.991 false (kept), three pixels 9 > 5.991 (rejected)
    for shift, outcome in ((1.0, tm.ACCEPTED), (3.0, tm.REPROJ2)):
        w = tw.exact_world()
        w.kf2.y[0] += shift
        for rec in (w.model(), w.host()):
            assert rec["outcome"][0] == outcome, shift
    w = tw.exact_world()
    w.kf1.uright[0] += 3.0                                           # the right coordinate enters keyframe 1's test: 9 > 7.8
    for rec in (w.model(), w.host()):
        assert rec["outcome"][0] == tm.REPROJ1
    # scale consistency: ratioDist = 4.5757 / 4.5826 = 0.9985 and ratioFactor = 1.8; octaves 7 / 4 give ratioOctave = 1.2^3 = 1.728,
    # below 0.9985 * 1.8 = 1.797 (kept); octaves 7 / 3 give 1.2^4 = 2.07, above it (rejected)
    for octave2, outcome in ((4, tm.ACCEPTED), (3, tm.SCALE)):
        w = tw.exact_world()
        w.kf1.octave[0], w.kf2.octave[0] = 7, octave2
        for rec in (w.model(), w.host()):
            assert rec["outcome"][0] == outcome, octave2


def test_known_answer_unprojection_at_the_principal_point():
    """A pixel at the principal point unprojects to (0, 0, z) in its camera: Twc's third column times z plus its translation for a
    first-camera feature; through mRcam12 * (0, 0, z) + mtcam12 = (z + 0.1, 0, 0) (a quarter turn about y, 10 cm lever arm) for a
    second-camera feature, picked by i >= N of the feature's OWN keyframe."""
    kf1 = tw.KF(np.eye(3), (-1.0, -2.0, -3.0), 1)                     # centre (1, 2, 3)
    kf2 = tw.KF(np.eye(3), (-1.0, -2.0, -3.0), 1)
    # distorted keypoint at the principal point, the undistorted one elsewhere: UnprojectStereo reads the distorted one
    kf1.set_features([300.0, 300.0], [200.0, 200.0], [tw.CX, tw.CX], [tw.CY, tw.CY], [0, 0], [100.0, 100.0], [2.0, 2.0])
    xc = tm.unproject_stereo(kf1, 0)
    assert [float(v) for v in xc] == [1.0, 2.0, 5.0]
    xc = tm.unproject_stereo(kf1, 1)                                  # i >= N: the second camera
    assert np.allclose([float(v) for v in xc], [1.0 + 2.1, 2.0, 3.0], atol=1e-6)
    # through the library: make the unprojection the chosen path (stereo parallax larger than the rays') and read x3D of the record
    kf2.set_features([300.0, 300.0], [200.0, 200.0], [300.0, 300.0], [200.0, 200.0], [0, 0], [-1.0, -1.0], [-1.0, -1.0])
    w = tw.World(kf1, kf2, [[0, 0], [1, 1]])
    rec, host = w.model(), w.host()
    assert rec.tobytes() == host.tobytes()
    assert (host["path"] == tm.PATH_UNPROJECT1).all()
    assert host["x3D"][0].tolist() == [1.0, 2.0, 5.0] and np.allclose(host["x3D"][1], [3.1, 2.0, 3.0], atol=1e-6)


def test_known_answer_camera_two_pair_takes_the_first_cameras_rotations_for_its_rays():
    """Both first cameras look the same way while the second cameras' [R|t] are 20 degrees apart: a camera-2 pair of features without
    depth at the same pixel has parallel rays by the reference's statement (Rwc1 / Rwc2 are the first camera's) and leaves as "low
    parallax" -- rays from the second cameras' rotations would be 20 degrees apart and the triangulation would run.  Turning the FIRST
    camera of keyframe 2 instead, with identical second-camera matrices, enters the linear triangulation."""
    def world(turn_first, turn_second):
        kf1 = tw.KF(np.eye(3), (0, 0, 0), 0)
        kf2 = tw.KF(tw.rotation((0, 1, 0), 20.0) if turn_first else np.eye(3), (-0.3, 0, 0), 0)
        if turn_second:
            kf2.Tcw[1, :, :3] = (tw.rotation((0, 1, 0), 20.0) @ kf1.Tcw[1, :, :3].astype(np.float64)).astype(np.float32)
        else:
            kf2.Tcw[1, :, :3] = kf1.Tcw[1, :, :3]
        for kf in (kf1, kf2):
            kf.set_features([400.0], [260.0], [400.0], [260.0], [0], [-1.0], [-1.0])
        return tw.World(kf1, kf2, [[0, 0]])
    w = world(False, True)
    for rec in (w.model(), w.host()):
        assert rec["outcome"][0] == tm.LOW_PARALLAX and rec["path"][0] == tm.PATH_NONE
    w = world(True, False)
    for rec in (w.model(), w.host()):
        assert rec["path"][0] == tm.PATH_SVD
    assert w.model().tobytes() == w.host().tobytes()


def test_cos_stereo_helper():
    """orbv_cos_stereo is cosf(2*atan2f(mb/2, depth)).  Held against the same expression in double: atan2f and cosf are each within one
    ulp.  The doubled angle is at most pi, so its error is at most 2^-22 absolute (the doubling is exact); the cosine's slope is at most 1
    and its own rounding adds at most 2^-24.  2^-21 + 2^-24 bounds the difference with a factor of two to spare."""
    import multi_orb_slam_amd as m
    depth = np.concatenate([np.exp(np.linspace(np.log(0.05), np.log(80.0), 4000)), [0.0384615]]).astype(np.float32)
    mb = np.float32(40.0) / np.float32(520.0)
    got = m.cos_stereo(mb, depth)
    want = np.cos(2 * np.arctan2(np.float64(mb / np.float32(2)), depth.astype(np.float64)))
    assert got.dtype == np.float32 and np.abs(got - want).max() <= 2.0 ** -21 + 2.0 ** -24
    assert m.cos_stereo(mb, depth).tobytes() == got.tobytes()
    assert abs(float(m.cos_stereo(np.float32(2.0), np.array([1.0], np.float32))[0])) < 1e-7      # atan2(1, 1) = pi/4: cos(pi/2)


def test_model_svd_null_vector_against_lapack():
    """The model's Jacobi SVD (float, OpenCV's sweep order, the hypot replacement) against numpy.linalg.svd of the same matrix in float64:
    the last right singular vector, up to sign, largest component difference.  Measured over the 6 271 linear triangulations of the three
    worlds: 6.4e-6 (the 90 cm world; medians 7e-8 .. 1.5e-7, 99th percentiles 2.5e-7 .. 1.4e-6 -- the tail belongs to pairs whose two
    smallest singular values lie close together).  Tolerance: that largest deviation times a margin of 4 for inputs not seen, 2.6e-5.
    This holds the MODEL against LAPACK; the library is held against the model, never against itself."""
    tolerance = 4 * 6.4e-6
    worst = 0.0
    for name in tw.WORLDS:
        w, rec = tw.world_and_model(name)
        for p in np.flatnonzero(rec["path"] == tm.PATH_SVD):
            _, _, A = tm.system_matrix(w.kf1, w.kf2, int(w.pairs[p, 0]), int(w.pairs[p, 1]))
            v = np.array(tm.jacobi_vt(A)[3], np.float64)
            ref = np.linalg.svd(np.array(A, np.float64))[2][3]
            if np.dot(ref, v) < 0:
                ref = -ref
            worst = max(worst, float(np.abs(ref - v).max()))
    print("largest deviation of the model's null vector from LAPACK: %.3g (tolerance %.3g)" % (worst, tolerance))
    assert worst <= tolerance


def test_argument_errors_of_the_host_routine():
    import multi_orb_slam_amd as m
    _lib = lib()
    L = _lib.lib()
    w, _ = tw.world_and_model("5cm")
    pairs = w.pairs[:64].copy()
    out = np.zeros(64, m.TRI_OUT_DTYPE)
    en = np.array([1, 1], np.uint8)

    def rc(change=None, pairs=pairs, **kw):
        k1, k2 = w.kf1.native(**kw.get("kf1", {})), w.kf2.native(**kw.get("kf2", {}))
        c1, c2 = k1.c(), k2.c()
        if change:
            change(c1, c2)
        return L.orbv_triangulate_pairs_host(C.byref(c1), C.byref(c2), _lib.ptr(en), _lib.ptr(pairs), len(pairs), float(w.ratio_factor), _lib.ptr(out))
    err = lambda: L.orb_last_error().decode()
    assert rc() == _lib.ORB_OK
    k1 = w.kf1.native().c()
    assert L.orbv_triangulate_pairs_host(None, C.byref(k1), _lib.ptr(en), _lib.ptr(pairs), 64, 1.8, _lib.ptr(out)) == _lib.ORB_E_ARG
    assert L.orbv_triangulate_pairs_host(C.byref(k1), None, _lib.ptr(en), _lib.ptr(pairs), 64, 1.8, _lib.ptr(out)) == _lib.ORB_E_ARG
    k2 = w.kf2.native().c()
    assert L.orbv_triangulate_pairs_host(C.byref(k1), C.byref(k2), None, _lib.ptr(pairs), 64, 1.8, _lib.ptr(out)) == _lib.ORB_E_ARG
    assert "cam_enabled" in err()
    assert L.orbv_triangulate_pairs_host(C.byref(k1), C.byref(k2), _lib.ptr(en), None, 64, 1.8, _lib.ptr(out)) == _lib.ORB_E_ARG
    assert L.orbv_triangulate_pairs_host(C.byref(k1), C.byref(k2), _lib.ptr(en), _lib.ptr(pairs), 64, 1.8, None) == _lib.ORB_E_ARG
    assert L.orbv_triangulate_pairs_host(C.byref(k1), C.byref(k2), _lib.ptr(en), _lib.ptr(pairs), -1, 1.8, _lib.ptr(out)) == _lib.ORB_E_ARG
    assert L.orbv_triangulate_pairs_host(C.byref(k1), C.byref(k2), _lib.ptr(en), None, 0, 1.8, None) == _lib.ORB_OK      # no pairs is legal
    for name in ("x", "yd", "octave", "uright", "depth", "cos_stereo"):
        assert rc(lambda c1, c2: setattr(c2, name, None)) == _lib.ORB_E_ARG and "kf2" in err()
    assert rc(lambda c1, c2: setattr(c1, "scale_factors", None)) == _lib.ORB_E_ARG
    assert rc(lambda c1, c2: setattr(c1, "n_levels", 0)) == _lib.ORB_E_ARG
    assert rc(lambda c1, c2: setattr(c2, "n_levels", 33)) == _lib.ORB_E_ARG
    # an index out of range, on either side, names the pair and the index
    bad = pairs.copy(); bad[5, 0] = w.kf1.n
    assert rc(pairs=bad) == _lib.ORB_E_ARG and "pair 5" in err() and "index %d" % w.kf1.n in err() and "kf1" in err()
    bad = pairs.copy(); bad[9, 1] = -1
    assert rc(pairs=bad) == _lib.ORB_E_ARG and "pair 9" in err() and "kf2" in err()
    # an octave outside n_levels
    oc = w.kf2.octave.copy(); oc[pairs[3, 1]] = tw.N_LEVELS
    assert rc(kf2=dict(octave=oc)) == _lib.ORB_E_ARG and "pair 3" in err() and "octave %d" % tw.N_LEVELS in err()
    oc = w.kf1.octave.copy(); oc[pairs[4, 0]] = -1
    assert rc(kf1=dict(octave=oc)) == _lib.ORB_E_ARG and "pair 4" in err()
    # a camera id outside cam_enabled
    cam = w.kf1.cam_of.copy(); cam[pairs[7, 0]] = 2
    assert rc(kf1=dict(cam_of=cam)) == _lib.ORB_E_ARG and "pair 7" in err() and "camera 2" in err()
    assert rc(kf1=dict(cam_of=w.kf1.cam_of)) == _lib.ORB_OK
    # a stereo feature without a positive depth (the reference's UnprojectStereo returns an empty matrix there)
    stereo = np.flatnonzero(w.kf1.uright[pairs[:, 0]] >= 0)[0]
    dp = w.kf1.depth.copy(); dp[pairs[stereo, 0]] = 0.0
    assert rc(kf1=dict(depth=dp)) == _lib.ORB_E_ARG and "pair %d" % stereo in err() and "depth" in err()


def test_an_explicit_camera_array_equals_the_default():
    w, rec = tw.world_and_model("5cm")
    import multi_orb_slam_amd as m
    got = m.triangulate_pairs_host(w.kf1.native(cam_of=w.kf1.cam_of), w.kf2.native(), w.cam_enabled, w.pairs, w.ratio_factor)
    assert got.tobytes() == rec.tobytes()
