"""The boundary worlds of the extractor (tests/extractor_boundary_worlds.py) hold what they are for, and the CPU oracle equals the plain
reference on every one of them: this is what gives the oracle its authority over records and descriptors in
tests/test_gpu_extractor_boundaries.py.  CPU only; every comparison is equality of integers or bytes."""
import numpy as np
import pytest

import oracle
import extractor_boundary_worlds as W

FAMILIES = sorted(W.FAMILIES)


def _accepted(family):
    return [w for w in W.FAMILIES[family]() if not w.refused]


@pytest.mark.parametrize("family", FAMILIES)
def test_family_holds_both_sides_of_its_boundaries(family):
    W.CHECKS[family]()


@pytest.mark.parametrize("family", FAMILIES)
def test_oracle_pyramid_equals_the_plain_resize_chain(family):
    for w in _accepted(family):
        p = w.params
        sizes = W.plain_level_sizes(w.image.shape[1], w.image.shape[0], p["scale_factor"], p["nlevels"])
        assert oracle.level_sizes(w.image.shape[1], w.image.shape[0], p["scale_factor"], p["nlevels"]) == sizes, w.name
        got = oracle.pyramid(w.image, p["scale_factor"], p["nlevels"])
        assert len(got) == len(w.levels)
        for l, (a, b) in enumerate(zip(got, w.levels)):
            assert a.shape == b.shape and np.array_equal(a, b), (w.name, l)


@pytest.mark.parametrize("family", FAMILIES)
def test_oracle_cell_candidates_equal_the_plain_cells(family):
    n = 0
    for w in _accepted(family):
        for l, level in enumerate(w.levels):
            c = oracle.cell_candidates(level, w.params["ini_th"], w.params["min_th"])
            got = [(int(k["x"]), int(k["y"]), int(k["response"])) for k in c]
            assert got == w.candidates(l), (w.name, l)
            assert all(float(k["x"]) == int(k["x"]) and float(k["response"]) == int(k["response"]) for k in c)
            n += len(got)
    assert n > 0 or family == "pyramid"


@pytest.mark.parametrize("family", ["edges", "angles", "saturation"])
def test_oracle_blur_and_moments_equal_the_plain_ones_at_the_keypoints(family):
    n = 0
    for w in _accepted(family):
        kps, _ = oracle.extract(w.image, nfeatures=w.params["nfeatures"], scale_factor=w.params["scale_factor"], nlevels=w.params["nlevels"],
                                ini_th=w.params["ini_th"], min_th=w.params["min_th"])
        kept = {(int(k["x"]), int(k["y"])) for k in kps if k["octave"] == 0}
        for l, level in enumerate(w.levels):
            assert np.array_equal(oracle.gaussian_blur7(level), W.plain_blur(level)), (w.name, l)
            for (x, y, _) in w.candidates(l):
                _, m01, m10 = oracle.ic_angle(level, x + W.BORDER, y + W.BORDER)
                assert (m10, m01) == W.plain_moments(level, x + W.BORDER, y + W.BORDER), (w.name, l, x, y)
                n += 1
        # the stamps are not only candidates: the quadtree keeps them, so the describe stage sees them
        for st in w.stamps:
            assert (st["x"], st["y"]) in kept, (w.name, st)
    assert n >= 12


def test_oracle_orientation_at_zero_and_equal_moments():
    """fast_atan2 where one moment is zero or both are equal in size: the eight directions come out 45 degrees apart to within the
    polynomial's published error (0.3 degrees), the axes exactly, and m10 == m01 == 0 gives 0."""
    (w,) = W.angles()
    ang = {}
    for st in w.stamps:
        a, m01, m10 = oracle.ic_angle(w.image, st["x"], st["y"])
        assert (m10, m01) == W.plain_moments(w.image, st["x"], st["y"])
        ang[st["kind"]] = (float(a), m10, m01)
    assert ang["dot"][0] == 0.0
    for k in range(4):
        a, m10, m01 = ang["sym%d" % k]
        assert a == {(1, 0): 0.0, (0, 1): 90.0, (-1, 0): 180.0, (0, -1): 270.0}[(int(np.sign(m10)), int(np.sign(m01)))]
        a, m10, m01 = ang["diag%d" % k]
        want = {(1, 1): 45.0, (-1, 1): 135.0, (-1, -1): 225.0, (1, -1): 315.0}[(int(np.sign(m10)), int(np.sign(m01)))]
        assert abs(a - want) < 0.3


def test_quotas_and_tables_equal_the_plain_ones():
    for w in W.tiny() + W.pyramid() + W.edges():
        p = w.params
        t = oracle.tables(p["nfeatures"], p["scale_factor"], p["nlevels"], p["ini_th"], p["min_th"])
        assert t["quota"].tolist() == W.plain_quotas(p["nfeatures"], p["scale_factor"], p["nlevels"]), w.name
        assert [np.float32(s).view(np.uint32) for s in t["scale"]] == [s.view(np.uint32) for s in W.plain_scales(p["scale_factor"], p["nlevels"])]
        assert t["umax"].tolist() == W.plain_umax()


def test_saturated_blur_is_where_the_clamp_decides():
    """(x * 257 * 257 + 32768) >> 16 is 257 for x = 255: without the clamp the byte would wrap to 1."""
    dark, _ = W.saturation()
    pre = W.plain_blur(dark.image, preclamp=True)
    got = oracle.gaussian_blur7(dark.image)
    assert (pre > 255).any() and (got[pre > 255] == 255).all() and np.array_equal(got[pre <= 255], pre[pre <= 255].astype(np.uint8))
