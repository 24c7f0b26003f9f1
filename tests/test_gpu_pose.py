"""GPU parity of the pose optimisation on the device (orbm_pose_optimize: one workgroup per problem, resident for the whole call) with
the library's host routine in the device's summation order -- byte for byte: result records and outlier flags -- and with the
index-order model of tests/pose_model.py: flags and return value identical, the pose within the tolerance derived on the CPU
(tests/test_pose_model.py).  The resident form (observations from the resident frame, positions from the resident point table)
against the plain form, byte for byte."""
import numpy as np
import pytest

import frustum_worlds as fw
import pose_model as pm
import pose_worlds as pw
from test_pose_model import ORDER_DIFF_TRANSLATION, ORDER_DIFF_QUATERNION, POSE_MARGIN

pytestmark = pytest.mark.gpu
WORLD = dict(pw.worlds())
NAMES = list(WORLD)


@pytest.fixture(scope="module")
def matcher():
    import multi_orb_slam_amd as m
    mt = m.Matcher(0.8, True)
    yield mt
    mt.close()


def same(got, want, what):
    (rec, flags), (hrec, hflags) = got, want
    for k in hrec.dtype.names:
        assert rec[k].tobytes() == hrec[k].tobytes(), (what, k, rec[k], hrec[k])
    assert rec.tobytes() == hrec.tobytes(), what
    assert np.array_equal(flags, hflags), (what, "flags", int((flags != hflags).sum()))


def device_and_host(mt, names_or_problems):
    import multi_orb_slam_amd as m
    probs = [pw.to_problem(m, WORLD[p]) if isinstance(p, str) else p for p in names_or_problems]
    dev = mt.PoseOptimization(probs)
    hst = m.pose_optimize_host(probs, order=m.POSE_ORDER_DEVICE)
    for i, (d, h) in enumerate(zip(dev, hst)):
        same(d, h, (i, names_or_problems[i] if isinstance(names_or_problems[i], str) else probs[i].n))
    return dev


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_host_routine_in_device_order(matcher, name):
    (rec, flags), = device_and_host(matcher, [name])
    assert matcher.last_pose() == (1, 0)
    # against the index-order model: flags and return value identical, the pose within the CPU-derived tolerance
    mrec, mflags, _ = pw.evaluate("index")[name]
    assert np.array_equal(flags, mflags) and rec["n_inliers"] == mrec["n_inliers"] and rec["n_bad"] == mrec["n_bad"]
    dt = float(np.abs(rec["t"] - mrec["t"]).max())
    dq = float(min(np.abs(rec["q"] - mrec["q"]).max(), np.abs(rec["q"] + mrec["q"]).max()))
    print("%s: device against the index-order model: translation %.3e, quaternion %.3e" % (name, dt, dq))
    assert dt <= POSE_MARGIN * ORDER_DIFF_TRANSLATION and dq <= POSE_MARGIN * ORDER_DIFF_QUATERNION


@pytest.mark.parametrize("B", [1, 2, 8, 64])
def test_batches_of_problems_of_unequal_length(matcher, B):
    names = [NAMES[(7 * i + B) % len(NAMES)] for i in range(B)]
    if B >= 8:
        names[3] = "two/cam0"; names[5] = "mixed_8000/all"; names[6] = "all_outliers/all"
    device_and_host(matcher, names)
    assert matcher.last_pose() == (B, 0)


def sized(n, seed=50, two_cams=True):
    import multi_orb_slam_amd as m
    return pw.to_problem(m, pw.generate(seed=seed + n % 97, n=n, kind="mixed", outliers=0.1, start=(0.05, 2.0), two_cams=two_cams))


def test_edge_counts_around_the_wave_and_the_capacity(matcher):
    import multi_orb_slam_amd as m
    counts = [0, 1, 9, 10, 11, 63, 64, 65, m.POSE_CAP, m.POSE_CAP + 1]        # (9, 10, 11: `n < 10` ends the call after one round)
    probs = [sized(n) for n in counts]
    got = device_and_host(matcher, probs)
    assert matcher.last_pose() == (len(counts) - 1, 1)             # one problem beyond the device capacity: the host routine took it
    assert [int(r["n_initial"]) for r, _ in got] == counts
    for p in probs[:-1]:
        device_and_host(matcher, [p])
        assert matcher.last_pose() == (1, 0)
    device_and_host(matcher, [probs[-1]])
    assert matcher.last_pose() == (0, 1)


@pytest.mark.parametrize("kind", ["mono", "stereo", "mixed"])
def test_nine_ten_and_eleven_edges(matcher, kind):
    """The counts either side of `if (S.n < 10 || S.round == 3)`: 9 edges end after the first round, 10 and 11 run all four."""
    import multi_orb_slam_amd as m
    counts = [9, 10, 11]
    probs = [pw.to_problem(m, pw.generate(seed=70 + n, n=n, kind=kind, outliers=0.1, start=(0.02, 1.0))) for n in counts]
    got = device_and_host(matcher, probs)
    assert matcher.last_pose() == (3, 0)
    assert [(int(r["n_initial"]), int(r["rounds"])) for r, _ in got] == [(9, 1), (10, 4), (11, 4)]
    for p in probs:
        device_and_host(matcher, [p])
        assert matcher.last_pose() == (1, 0)


def test_the_call_made_twice_gives_identical_bytes(matcher):
    names = ["mixed_8000/all", "rig_2000/all", "stereo_2000/cam0", "mono_60/cam0"]
    a = device_and_host(matcher, names)
    b = device_and_host(matcher, names)
    for x, y, n in zip(a, b, names):
        same(x, y, n)


@pytest.mark.parametrize("mode", [pm.CAM0, pm.ALL_CAMS])
def test_resident_form_equals_the_plain_form(matcher, mode):
    """The frame uploaded as the search tests do it, a point table written with orbm_points_write, point_of_feature from an actual
    orbm_search_local_points call on one of frustum_worlds' worlds."""
    import multi_orb_slam_amd as m
    w = fw.make_world(2000, [1000, 500], 640, 480, 2, 3.0)
    fr, V, points = w["fr"], w["view"], w["points"]
    F = matcher.frame(m.FrameData(**fr))
    with m.LocalPoints(matcher, len(points)) as pts:
        pts.write(0, points)
        _, nmatches, match_of_feature, _ = matcher.SearchLocalPoints(F, pts, V.native())
        assert nmatches > 100
        N = len(match_of_feature)
        n_cam0 = 1000
        Tcw = np.eye(4, dtype=np.float32)
        Tcw[:3, :3] = V.Rcw
        Tcw[:3, 3] = V.tcw
        inv_sigma2 = (1.0 / (V.scale_factors * V.scale_factors)).astype(np.float32)
        R12 = pw.rot([0.1, 1.0, 0.05], 0.6).astype(np.float32)
        g = np.nonzero(match_of_feature >= 0)[0]
        if mode == pm.CAM0:
            g = g[g < n_cam0]
        rows = match_of_feature[g]
        obs = np.stack([fr["un_x"][g], fr["un_y"][g], fr["uright"][g]], axis=1)
        prob = m.PoseProblem(Tcw, V.fx, V.fy, V.cx, V.cy, V.mbf, inv_sigma2, g, points["pos"][rows], obs, fr["octave"][g], mode=mode,
                             n_cam0=n_cam0, Rcam12=R12, tcam12=[0.3, 0.0, 0.05])
        assert (obs[:, 2] < 0).any() and (obs[:, 2] >= 0).any()
        (prec, pflags), = matcher.PoseOptimization([prob])
        (hrec, hflags), = m.pose_optimize_host([prob], order=m.POSE_ORDER_DEVICE)
        same((prec, pflags), (hrec, hflags), "plain")
        rrec, rflags = matcher.PoseOptimizationResident(prob, F, pts, match_of_feature)
        assert matcher.last_pose() == (1, 0)
        assert rrec.tobytes() == prec.tobytes()
        per_feature = np.zeros(N, np.uint8)
        per_feature[g] = pflags
        assert np.array_equal(rflags, per_feature)
        assert 0 < int(prec["n_inliers"]) and prec["rounds"] == 4
        print("resident form: %d edges, %d inliers" % (len(g), int(prec["n_inliers"])))
        # no point at all: the early return, the pose untouched
        rrec, rflags = matcher.PoseOptimizationResident(prob, F, pts, np.full(N, -1, np.int32))
        assert rrec["n_inliers"] == 0 and rrec["rounds"] == 0 and rrec["Tcw"].tobytes() == Tcw.tobytes() and not rflags.any()
    F.close()


def test_the_staged_block_grows_and_is_reused_on_a_fresh_matcher():
    """A handle of its own, so that the staged block is reallocated inside the test: 1 problem of 2 edges, then 8 problems of 400
    edges, then the first again.  Every call byte for byte the host routine in device order, the two small calls each other."""
    import multi_orb_slam_amd as m
    mt = m.Matcher(0.8, True)
    try:
        small, large = [sized(2)], [sized(400, seed=50 + 3 * i) for i in range(8)]
        first = device_and_host(mt, small)
        assert mt.last_pose() == (1, 0)
        device_and_host(mt, large)
        assert mt.last_pose() == (8, 0)
        again = device_and_host(mt, small)
        same(first[0], again[0], "the small call before and after the large one")
    finally:
        mt.close()
