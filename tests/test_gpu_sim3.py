"""GPU parity of the Sim3 RANSAC on the device (orbm_sim3_ransac: one lane per hypothesis for the Horn alignment, one wave per
hypothesis for the inlier masks) with the library's host routine in DEVICE order -- byte for byte: hypothesis records, inlier counts
and mask words."""
import numpy as np
import pytest

import sim3_model as sm
import sim3_worlds as sw

pytestmark = pytest.mark.gpu
WORLD = dict(sw.worlds())
NAMES = list(WORLD)


@pytest.fixture(scope="module")
def matcher():
    import multi_orb_slam_amd as m
    mt = m.Matcher(0.8, True)
    yield mt
    mt.close()


def same(got, want, what):
    (rec, masks), (hrec, hmasks) = got, want
    for k in hrec.dtype.names:
        assert rec[k].tobytes() == hrec[k].tobytes(), (what, k, np.nonzero((rec[k] != hrec[k]).reshape(len(rec), -1).any(axis=1))[0][:5])
    assert rec.tobytes() == hrec.tobytes(), what
    assert masks.shape == hmasks.shape and masks.tobytes() == hmasks.tobytes(), (what, "masks")


def device_and_host(mt, names_or_problems):
    import multi_orb_slam_amd as m
    probs = [sw.to_problem(m, WORLD[p]) if isinstance(p, str) else p for p in names_or_problems]
    dev = mt.Sim3Ransac(probs)
    hst = m.sim3_ransac_host(probs, order=m.SIM3_MATH_DEVICE)
    for i, (d, h) in enumerate(zip(dev, hst)):
        same(d, h, (i, names_or_problems[i] if isinstance(names_or_problems[i], str) else (probs[i].n, probs[i].h)))
    return dev


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_host_routine_in_device_order(matcher, name):
    (rec, masks), = device_and_host(matcher, [name])
    over = len(WORLD[name]["x3dc1"]) > sm.CAP
    assert matcher.last_sim3() == ((0, 1) if over else (1, 0))
    # and the model in libm order: counts and masks identical (the guard band), the same elements non-finite
    mrec, mmasks, _, _ = sw.evaluate("libm")[name]
    assert np.array_equal(rec["n_inliers"], mrec["n_inliers"]) and masks.tobytes() == mmasks.tobytes()
    assert np.array_equal(np.isfinite(rec["T12"]), np.isfinite(mrec["T12"]))


def sized(n, h, seed=60, **kw):
    import multi_orb_slam_amd as m
    W = sw.generate(seed + n % 89, max(n, 3), wrong=0.3, noise=1.0, cams=(0.2, 0.2), H=max(h, 1), **kw)
    keep = lambda a: a[:n]
    tri = W["triples"][:h] if n >= 3 else np.zeros((0, 3), np.int32)
    return m.Sim3Problem(W["K1"], W["K2"], keep(W["x3dc1"]), keep(W["x3dc2"]), keep(W["cam1"]), keep(W["cam2"]), keep(W["max_err1"]),
                         keep(W["max_err2"]), tri, fix_scale=W["fix_scale"], calib=W["calib"])


@pytest.mark.parametrize("B", [1, 2, 8, 64])
def test_batches_of_problems_of_unequal_length(matcher, B):
    import multi_orb_slam_amd as m
    shapes = [(0, 0), (3, 1), (63, 5), (64, 64), (65, 65), (200, 0), (129, 300), (1000, 7), (m.SIM3_CAP, 3), (m.SIM3_CAP + 1, 2),
              (20, m.SIM3_MAX_ITS), (500, 300)]
    probs = [sized(*shapes[(5 * i + B) % len(shapes)], fix_scale=bool(i & 1)) for i in range(B)]
    if B >= 8:
        probs[3] = sw.to_problem(m, WORLD["degenerate_and_repeated"]); probs[5] = sw.to_problem(m, WORLD["depth_zero"])
        probs[6] = sw.to_problem(m, WORLD["n300_fixed_wide"])
    device_and_host(matcher, probs)
    n_host = sum(p.n > m.SIM3_CAP for p in probs)
    assert matcher.last_sim3() == (B - n_host, n_host)


def test_counts_around_the_wave_the_capacity_and_the_iteration_limit(matcher):
    import multi_orb_slam_amd as m
    shapes = [(0, 0), (3, 4), (63, 9), (64, 9), (65, 9), (m.SIM3_CAP, 5), (m.SIM3_CAP + 1, 5), (40, m.SIM3_MAX_ITS), (40, 0)]
    probs = [sized(n, h) for n, h in shapes]
    got = device_and_host(matcher, probs)
    assert matcher.last_sim3() == (len(shapes) - 1, 1)             # one problem beyond the device capacity: the host routine took it
    assert [(len(r), mk.shape[1]) for r, mk in got] == [(h if n >= 3 else 0, (n + 63) // 64) for n, h in shapes]
    for p in probs:
        device_and_host(matcher, [p])
        assert matcher.last_sim3() == ((0, 1) if p.n > m.SIM3_CAP else (1, 0))


def test_the_call_made_twice_gives_identical_bytes(matcher):
    names = ["n2000_fixed_wrong30", "n128_free_0.7_both", "rotation_zero", "n500_free_1.4_wrong60"]
    a = device_and_host(matcher, names)
    b = device_and_host(matcher, names)
    for x, y, n in zip(a, b, names):
        same(x, y, n)


def test_a_call_after_an_unrelated_search_on_the_same_matcher(matcher):
    import multi_orb_slam_amd as m
    import frustum_worlds as fw
    w = fw.make_world(2000, [1000, 500], 640, 480, 2, 3.0)
    F = matcher.frame(m.FrameData(**w["fr"]))
    with m.LocalPoints(matcher, len(w["points"])) as pts:
        pts.write(0, w["points"])
        _, nmatches, _, _ = matcher.SearchLocalPoints(F, pts, w["view"].native())
        assert nmatches > 100
        device_and_host(matcher, ["n1000_free_1.0_wrong30", "n40_free_0.7_wrong30"])
    F.close()


def test_a_matcher_closes_its_frames_before_itself():
    """orbm_frame_destroy hands the frame's buffers back to its matcher: a frame that is still open when the matcher closes (the
    test above failing before its F.close(), the frame kept alive by the traceback) must be closed by the matcher, not after it."""
    import multi_orb_slam_amd as m
    import frustum_worlds as fw
    w = fw.make_world(2000, [1000, 500], 640, 480, 2, 3.0)
    mt = m.Matcher(0.8, True)
    F = mt.frame(m.FrameData(**w["fr"]))
    assert F._h
    mt.close()
    assert F._h is None and mt._h is None
    F.close()


def test_the_staged_block_grows_and_is_reused_on_a_fresh_matcher():
    """A handle of its own, so that the staged block is reallocated inside the test: (n, h) = (3, 1), then (1000, 300) next to a
    problem without a hypothesis, then (3, 1) again.  Every call byte for byte the host routine in device order, the two small calls
    each other."""
    import multi_orb_slam_amd as m
    mt = m.Matcher(0.8, True)
    try:
        small, large = [sized(3, 1)], [sized(1000, 300), sized(200, 0)]
        first = device_and_host(mt, small)
        assert mt.last_sim3() == (1, 0)
        got = device_and_host(mt, large)
        assert mt.last_sim3() == (2, 0) and [len(r) for r, _ in got] == [300, 0]
        again = device_and_host(mt, small)
        same(first[0], again[0], "the small call before and after the large one")
    finally:
        mt.close()
