"""The frustum model (tests/frustum_model.py) against answers worked out by hand, the level-threshold table against direct
logf evaluation, and the library's host restatement of the kernel (orbm_frustum_host: the arithmetic the exact fallback of
orbm_search_local_points runs) against the model.  No GPU."""
import numpy as np
import pytest

import frustum_model as fm
import frustum_worlds as fw

f32, f64 = np.float32, np.float64


def simple_view(th=3.0, bounds=(0.0, 0.0, 640.0, 480.0), limit=0.5):
    sf, lsf = fw.scale_pyramid()
    return fm.View(np.eye(3), np.zeros(3), np.zeros(3), 500.0, 500.0, 320.0, 240.0, 40.0, bounds, sf, lsf, th, limit)


def one_point(pos, normal=(0, 0, 1), min_dist=1.0, max_dist=8.0, blocks=1):
    p = fm.make_points(1)
    p["pos"][0] = pos; p["normal"][0] = normal; p["min_dist"] = min_dist; p["max_dist"] = max_dist; p["blocks"] = blocks
    p["desc"][0] = np.arange(32)
    return p


def up(x):
    return np.nextafter(f32(x), f32(np.inf))


def down(x):
    return np.nextafter(f32(x), f32(-np.inf))


def test_point_on_the_optical_axis():
    # Pc = (0, 0, 4): invz = 0.25, u = 320, v = 240, dist = 4, viewCos = 1, ratio = 2 -> ceil(log 2 / log 1.2) = ceil(3.80) = 4
    V = simple_view(th=3.0)
    verdict, track, q, keep = fm.frustum(one_point((0, 0, 4)), V)
    assert verdict[0] == fm.IN_VIEW and keep.tolist() == [0]
    t = track[0]
    assert (t["proj_x"], t["proj_y"], t["proj_xr"], t["view_cos"], t["level"], t["in_view"]) == (320.0, 240.0, 310.0, 1.0, 4, 1)
    sf4 = f32(f32(f32(f32(1.2) * f32(1.2)) * f32(1.2)) * f32(1.2))
    assert q["radius"][0] == f32(f32(f32(2.5) * f32(3.0)) * sf4)          # viewCos > 0.998: 2.5, times th, times the level's scale
    assert (q["u"][0], q["v"][0], q["ur"][0], q["min_level"][0], q["max_level"][0], q["cam"][0], q["blocks"][0]) == (320, 240, 310, 3, 4, 0, 1)
    assert q["desc"][0].tolist() == list(range(32)) and q["angle"][0] == 0


def test_th_one_leaves_the_radius_alone_and_oblique_views_get_the_wide_window():
    # normal tilted so that viewCos = 0.6 <= 0.998: r = 4.0; th == 1.0: no factor
    V = simple_view(th=1.0)
    _, track, q, _ = fm.frustum(one_point((0, 0, 4), normal=(0.8, 0, 0.6)), V)
    assert track["view_cos"][0] == f32(f64(4.0) * f64(f32(0.6)) / f64(4.0)) and track["level"][0] == 4
    sf4 = V.scale_factors[4]
    assert q["radius"][0] == f32(f32(4.0) * sf4)


@pytest.mark.parametrize("kwargs,reason", [
    (dict(pos=(0, 0, -4)), fm.BEHIND),                          # PcZ < 0
    (dict(pos=(4, 0, 4)), fm.OUTSIDE),                          # u = 500 * 4 * 0.25 + 320 = 820 > 640
    (dict(pos=(0, -4, 4)), fm.OUTSIDE),                         # v = 240 - 500 < 0
    (dict(pos=(0, 0, 4), min_dist=6.0), fm.TOO_NEAR),           # 4 < 0.8 * 6
    (dict(pos=(0, 0, 4), max_dist=3.0), fm.TOO_FAR),            # 4 > 1.2 * 3
    (dict(pos=(0, 0, 4), normal=(1, 0, 0)), fm.GRAZING),        # viewCos = 0 < 0.5
    (dict(pos=(1, 0, 0)), fm.NONFINITE),                        # PcZ == 0: u infinite (the documented deviation)
    (dict(pos=(0, 0, 0), min_dist=0.0), fm.NONFINITE),          # 0 * inf
])
def test_one_case_per_rejection(kwargs, reason):
    verdict, track, q, keep = fm.frustum(one_point(**kwargs), simple_view())
    assert verdict[0] == reason and len(q) == 0 and len(keep) == 0
    assert track[0].tobytes() == bytes(24)


def test_skip_is_neither_tested_nor_searched():
    verdict, track, q, _ = fm.frustum(one_point((0, 0, 4)), simple_view(), skip=np.array([1], np.uint8))
    assert verdict[0] == fm.SKIPPED and track["in_view"][0] == 0 and len(q) == 0


def test_equalities_pass():
    # u == min_x: Pc = (-2.5, 0, 4): u = 500 * -2.5 * 0.25 + 320 = 7.5 exactly
    p = one_point((-2.5, 0, 4))
    assert fm.frustum(p, simple_view(bounds=(7.5, 0.0, 640.0, 480.0)))[0][0] == fm.IN_VIEW
    assert fm.frustum(p, simple_view(bounds=(up(7.5), 0.0, 640.0, 480.0)))[0][0] == fm.OUTSIDE
    # u == max_x, v == min_y, v == max_y the same way
    assert fm.frustum(p, simple_view(bounds=(0.0, 0.0, 7.5, 480.0)))[0][0] == fm.IN_VIEW
    assert fm.frustum(p, simple_view(bounds=(0.0, 0.0, down(7.5), 480.0)))[0][0] == fm.OUTSIDE
    assert fm.frustum(p, simple_view(bounds=(0.0, 240.0, 640.0, 240.0)))[0][0] == fm.IN_VIEW
    assert fm.frustum(p, simple_view(bounds=(0.0, up(240.0), 640.0, 480.0)))[0][0] == fm.OUTSIDE
    # dist == 1.2f * max_dist: the point at exactly that depth on the axis (sqrt of a float's square in double is the float)
    edge = f32(f32(1.2) * f32(5.0))
    assert fm.frustum(one_point((0, 0, edge), max_dist=5.0), simple_view())[0][0] == fm.IN_VIEW
    assert fm.frustum(one_point((0, 0, up(edge)), max_dist=5.0), simple_view())[0][0] == fm.TOO_FAR
    # dist == 0.8f * min_dist
    edge = f32(f32(0.8) * f32(5.0))
    assert fm.frustum(one_point((0, 0, edge), min_dist=5.0), simple_view())[0][0] == fm.IN_VIEW
    assert fm.frustum(one_point((0, 0, down(edge)), min_dist=5.0), simple_view())[0][0] == fm.TOO_NEAR
    # viewCos == limit: PO = (0, 0, 4), Pn = (0, 0, 0.5): 4 * 0.5 / 4 = 0.5
    assert fm.frustum(one_point((0, 0, 4), normal=(0, 0, 0.5)), simple_view())[0][0] == fm.IN_VIEW
    assert fm.frustum(one_point((0, 0, 4), normal=(0, 0, down(0.5))), simple_view())[0][0] == fm.GRAZING
    # PcZ == +0 is not "behind" (0 < 0 is false); it is rejected as a non-finite projection instead
    assert fm.frustum(one_point((1, 0, 0.0)), simple_view())[0][0] == fm.NONFINITE


def test_dot_product_accumulates_in_double():
    # PO = Pn = (1, 2^-12, 2^-12): the products are 1, 2^-24, 2^-24.  In float 1 + 2^-24 rounds back to 1 twice: viewCos = 1.0.
    # In double the sum is 1 + 2^-23, dist = (float)sqrt(1 + 2^-23) = 1.0, and viewCos = (float)(1 + 2^-23) = 0x3f800001.
    e = 2.0 ** -12
    assert f32(f32(f32(1) + f32(e * e)) + f32(e * e)) == f32(1.0)
    V = simple_view(bounds=(0.0, 0.0, 1e7, 1e7))
    verdict, track, _, _ = fm.frustum(one_point((1, e, e), normal=(1, e, e), min_dist=0.5, max_dist=1.0), V)
    assert verdict[0] == fm.IN_VIEW
    assert track["view_cos"][:1].view(np.uint32)[0] == 0x3F800001
    assert track["level"][0] == 0 and track["proj_x"][0] == f32(500 * 4096 + 320)


def test_camera_centre_is_a_float_product_with_weight_minus_one():
    # R = rotation by 90 degrees about z, t = (1, 2, 3): Rt * t = (2, -1, 3), Ow = (-2, 1, -3)
    R = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], f32)
    assert fm.camera_centre(R, [1, 2, 3]).tolist() == [-2.0, 1.0, -3.0]
    # a case where float and double accumulation differ: column (1, 2^-24, 2^-24) against t = (1, 1, 1)
    e = 2.0 ** -24
    R = np.array([[1, 0, 0], [e, 1, 0], [e, 0, 1]], f32)
    assert fm.camera_centre(R, [1, 1, 1])[0] == f32(-1.0)          # in double the sum is 1 + 2^-23: -1.0000001 after rounding


@pytest.mark.parametrize("scale_factor,n_levels", [(1.2, 8), (2.0, 8), (1.05, 11), (1.5, 6)])
def test_threshold_table_against_direct_logf(scale_factor, n_levels):
    import multi_orb_slam_amd as m
    lsf = f32(np.log(f64(f32(scale_factor))))
    T = m.level_thresholds(lsf, n_levels)
    assert len(T) == n_levels - 1 and np.all(np.diff(T) > 0)

    def by_table(r):
        return (r[:, None] > T[None, :]).sum(1).astype(np.int32)

    rng = np.random.default_rng(7)
    top = float(scale_factor) ** n_levels * 1.5
    r = np.concatenate([rng.uniform(0.2, top, 600000), np.exp(rng.uniform(np.log(1e-6), np.log(1e6), 400000))]).astype(f32)
    assert len(r) >= 10 ** 6
    assert np.array_equal(by_table(r), fm.predict_level(r, lsf, n_levels))
    for t in T:    # the +-4096 ulp neighbourhood of every threshold
        bits = np.arange(-4096, 4097, dtype=np.int64) + int(np.array([t], f32).view(np.uint32)[0])
        near = bits.astype(np.uint32).view(f32)
        assert np.array_equal(by_table(near), fm.predict_level(near, lsf, n_levels))
    # what the reference leaves undefined, settled the same way on both sides
    odd = np.array([0.0, -1.0, np.inf, np.nan, 1e-45], f32)
    assert by_table(odd).tolist() == [0, 0, n_levels - 1, 0, 0] == fm.predict_level(odd, lsf, n_levels).tolist()


def test_threshold_table_argument_errors():
    import multi_orb_slam_amd as m
    for lsf, n in ((0.0, 8), (-0.2, 8), (float("nan"), 8), (0.18, 0), (0.18, 33), (1000.0, 8)):
        with pytest.raises(m.OrbError) as e:
            m.level_thresholds(lsf, n)
        assert e.value.code == -1


@pytest.mark.parametrize("case", fw.CASES[:3])
def test_host_restatement_equals_model_on_generated_worlds(case):
    import multi_orb_slam_amd as m
    w = fw.make_world(*case)
    skip = (np.random.default_rng(case[4]).random(case[0]) < 0.1).astype(np.uint8)
    for sk in (None, skip):
        verdict, track, q, keep = fm.frustum(w["points"], w["view"], sk)
        cnt, htrack, hq = m.frustum_host(w["points"], w["view"].native(), sk)
        assert cnt == len(keep) and htrack.tobytes() == track.tobytes()
        assert hq[keep].tobytes() == q.tobytes()
        assert np.all(hq["cam"][track["in_view"] == 0] == -1)       # no window: such a query has no candidates


def test_host_restatement_equals_model_on_every_boundary():
    import multi_orb_slam_amd as m
    b = fw.make_boundary_world([1000, 500], 640, 480, 11, 3.0)
    verdict, track, q, keep = fm.frustum(b["points"], b["view"])
    kinds = set(b["kinds"].tolist())
    assert {"u_min", "u_max", "v_min", "v_max", "too_near", "too_far", "grazing", "radius", "behind"} <= kinds
    assert all("level%d" % k in kinds for k in range(fw.N_LEVELS - 1))
    for k in kinds - {"plain"}:      # both sides of every boundary are there
        sel = b["kinds"] == k
        if k.startswith("level"):
            lv = int(k[5:]); assert set(track["level"][sel].tolist()) == {lv, lv + 1}
        elif k == "radius":
            vc = track["view_cos"][sel].astype(f64); assert (vc > 0.998).any() and (vc <= 0.998).any()
        elif k == "behind":
            assert (verdict[sel] == fm.BEHIND).any() and (verdict[sel] != fm.BEHIND).any()
        else:
            assert (verdict[sel] == fm.IN_VIEW).any() and (verdict[sel] != fm.IN_VIEW).any()
    cnt, htrack, hq = m.frustum_host(b["points"], b["view"].native())
    assert cnt == len(keep) and htrack.tobytes() == track.tobytes() and hq[keep].tobytes() == q.tobytes()


def test_generated_worlds_meet_their_conditions():
    """The GPU tests assert these again before they compare anything; here they are held without a device."""
    import oracle
    for case in fw.CASES[:3]:
        w = fw.make_world(*case)
        got = fm.expected_search(oracle.FrameData(**w["fr"]), w["points"], w["view"], None, None, 0.8, 100)
        fw.check_conditions(w, *got)
