"""The extractor's kernels on their decision boundaries, in every form: the constructed worlds of tests/extractor_boundary_worlds.py
through k_pyramid_* / k_resize, k_fast_cells, k_octree and k_describe.  Every pyramid level byte for byte against the plain resize chain,
every level's candidate list (x, y, response, order) against the plain cell loop and the oracle, keypoint records and descriptors bit for
bit against oracle.extract (which tests/test_extractor_boundary_worlds.py holds to the plain reference on these very worlds).

The forms of the kernels are chosen once per process (MORB_FAST_FORM, MORB_PYR_CHAIN, the large-rig tile plan), so the tests of this file
run in the default forms in this process and once more per other form in a child pytest process (test_every_world_once_more_in_form)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import extractor_boundary_worlds as W

pytestmark = pytest.mark.gpu

REFUSAL = "too small for the 30-px detection grid"
_ORACLE = {}


def _params(w):
    import multi_orb_slam_amd as m
    p = w.params
    return m.ExtractorParams(nfeatures=p["nfeatures"], scale_factor=p["scale_factor"], nlevels=p["nlevels"], ini_th_fast=p["ini_th"],
                             min_th_fast=p["min_th"])


def _oracle(w):
    """(keypoints, descriptors, [candidates per level]) of the oracle: computed once per world"""
    if w.name not in _ORACLE:
        p = w.params
        kps, desc = oracle.extract(w.image, nfeatures=p["nfeatures"], scale_factor=p["scale_factor"], nlevels=p["nlevels"], ini_th=p["ini_th"],
                                   min_th=p["min_th"])
        _ORACLE[w.name] = (kps, desc, [oracle.cell_candidates(lv, p["ini_th"], p["min_th"]) for lv in w.levels])
    return _ORACLE[w.name]


def _make(worlds):
    import multi_orb_slam_amd as m
    return m.Extractor([_params(w) for w in worlds], max(64, max(w.image.shape[1] for w in worlds)), max(64, max(w.image.shape[0] for w in worlds)))


def _assert_form(ex, worlds):
    want = os.environ.get("MORB_EXPECT_PYRAMID_FORM")   # (a child of test_every_world_once_more_in_form: the form it forced did run)
    if want:
        # the large-rig tile launches need a second level to build; a rig of one-level cameras takes the per-level chain (nothing to launch)
        want = 2 if int(want) == 3 and max(w.params["nlevels"] for w in worlds) < 2 else int(want)
        assert ex.pyramid_form() == want, (ex.pyramid_form(), want, [w.name for w in worlds])


def _assert_world(ex, cam, w, kps, desc, path=0):
    okps, odesc, ocands = _oracle(w)
    for l, ref in enumerate(w.levels):
        got = ex.debug_level(cam, l)
        assert got.shape == ref.shape and np.array_equal(got, ref), (w.name, "level %d" % l)
        cand = ex.debug_candidates(cam, l)
        assert [(int(k["x"]), int(k["y"]), int(k["response"])) for k in cand] == w.candidates(l), (w.name, "candidates of level %d" % l)
        for f in ("x", "y", "response"):
            assert np.array_equal(cand[f].view(np.uint32), ocands[l][f].view(np.uint32)), (w.name, l, f)
    assert len(kps) == len(okps), (w.name, len(kps), len(okps))
    for f in kps.dtype.names:
        a, b = kps[f], okps[f]
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b), (w.name, f)
    assert np.array_equal(desc, odesc), w.name
    assert ex.last_path() == path, (w.name, ex.last_path())


def _expected_path(worlds):
    """0: the device quadtree, the path under test.  It takes up to four root nodes; a level with candidates and more roots (the strips:
    26 and 55) sends the launch through the host quadtree (2), like a level beyond the device's candidate limit."""
    wide = any(W.plain_roots(lv.shape[1], lv.shape[0]) > 4 and w.candidates(l) for w in worlds for l, lv in enumerate(w.levels))
    return 2 if wide else 0


def _run(worlds, path=None):
    """the worlds as the cameras of one launch"""
    path = _expected_path(worlds) if path is None else path
    ex = _make(worlds)
    try:
        out = ex.extract([w.image for w in worlds])
        _assert_form(ex, worlds)
        for c, w in enumerate(worlds):
            _assert_world(ex, c, w, out[c][0], out[c][1], path)
    finally:
        ex.close()


@pytest.mark.parametrize("family", sorted(W.FAMILIES))
def test_family_equals_the_plain_reference_and_the_oracle(family):
    """Two worlds per launch, so that the cells next to a world's in the grid of k_fast_cells, and the blocks next to its own in every
    other kernel, belong to another world with other parameters or another size."""
    ws = [w for w in W.FAMILIES[family]() if not w.refused]
    for i in range(0, len(ws), 2):
        _run(ws[i:i + 2])


def test_worlds_of_different_families_and_sizes_share_a_launch():
    by = {w.name: w for w in W.all_worlds()}
    _run([by["lanes_strip_813_empty_last_column"], by["tiny_62x62_l1"], by["nms_pairs"]])
    _run([by["edges_rims_and_corners"], by["angles_dihedral_and_zero_moments"], by["saturation_dark_on_255"], by["pyramid_checker_127x93"]])
    _run([by["thresholds_255_255_c0_0"], by["thresholds_1_1_c100_0"], by["thresholds_128_127_c100_0"], by["survivors_every_pixel"]])


def test_a_handle_serves_the_worlds_of_a_family_one_after_the_other():
    """the geometry is re-derived per size and nothing of the previous image is left behind (flat worlds after busy ones)"""
    ws = [w for w in W.tiny() if not w.refused and w.params["nlevels"] == 1 and w.params["nfeatures"] == 50]
    ex = _make(ws)
    try:
        for w in ws[::-1] + ws:
            kps, desc = ex.extract([w.image] + [None] * (len(ws) - 1))[0]
            p = w.params
            okps, odesc = oracle.extract(w.image, nfeatures=ex.params[0].nfeatures, scale_factor=p["scale_factor"], nlevels=p["nlevels"],
                                         ini_th=p["ini_th"], min_th=p["min_th"])
            assert kps.tobytes() == okps.tobytes() and np.array_equal(desc, odesc), w.name
            assert len(ex.debug_candidates(0, 0)) == w.n_corners and len(kps) <= w.n_corners and (len(kps) > 0) == (w.n_corners > 0)
    finally:
        ex.close()


def test_refused_sizes_raise_the_plans_error_and_leave_the_handle_usable():
    """One pixel below the smallest level that still has a 30-pixel cell (62 wide or high): the plan's error, and the next call works."""
    from multi_orb_slam_amd._lib import OrbError
    ws = W.tiny()
    by = {w.name: w for w in ws}
    good = {2: by["tiny_74x74_l2"], 1: by["tiny_62x62_l1"]}
    bad = [w for w in ws if w.refused]
    assert len(bad) == len(W.TINY_REFUSED)
    for w in bad:
        g = good[w.params["nlevels"]]
        ex = _make([w, g])
        try:
            with pytest.raises(OrbError, match=REFUSAL):
                ex.extract([w.image, None])
            with pytest.raises(OrbError, match=REFUSAL):     # (as the second camera of a launch whose first one is fine)
                ex.extract([g.image, w.image])
            out = ex.extract([g.image, g.image])
            for c in range(2):
                _assert_world(ex, c, g, out[c][0], out[c][1])
        finally:
            ex.close()


@pytest.mark.parametrize("family", ["tiny", "nms"])
def test_host_quadtree_path_on_the_smallest_worlds(family):
    """MORB_HOST_OCTREE=1 (read at create): the candidates of the same kernels through the host quadtree and the list form of k_describe"""
    ws = [w for w in W.FAMILIES[family]() if not w.refused]
    os.environ["MORB_HOST_OCTREE"] = "1"
    try:
        exs = [_make(ws[i:i + 2]) for i in range(0, len(ws), 2)]
    finally:
        os.environ.pop("MORB_HOST_OCTREE")
    for k, ex in enumerate(exs):
        pair = ws[2 * k:2 * k + 2]
        try:
            out = ex.extract([w.image for w in pair])
            for c, w in enumerate(pair):
                _assert_world(ex, c, w, out[c][0], out[c][1], path=2)
        finally:
            ex.close()


# form -> (pyramid form the child must see, environment).  MORB_TEST_PYRAMID_PLAN = "tile_w,tile_h,split" is read by tests/conftest.py.
FORMS = {
    "fast_latency_form": (None, {"MORB_FAST_FORM": "1"}),
    "fast_throughput_form_large_rig_pyramid": (3, {"MORB_FAST_FORM": "2", "MORB_PYR_CHAIN": "1"}),
    "generic_chain": (2, {"MORB_PYR_CHAIN": "2"}),
    "large_rig_pyramid_small_tiles": (3, {"MORB_PYR_CHAIN": "1", "MORB_TEST_PYRAMID_PLAN": "32,16,0"}),
}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_every_world_once_more_in_form(form):
    """k_fast_cells<256, 4> and <128, 8>, the one-launch tile pyramid, the large-rig tile launches (at their default and at small tiles
    with ragged last rows and columns) and the per-level chain: the tests above in a fresh process per form."""
    want, extra = FORMS[form]
    env = {k: v for k, v in os.environ.items() if k not in ("MORB_FAST_FORM", "MORB_PYR_CHAIN", "MORB_TEST_PYRAMID_PLAN", "MORB_EXPECT_PYRAMID_FORM")}
    env.update(extra)
    if want is not None:
        env["MORB_EXPECT_PYRAMID_FORM"] = str(want)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "not once_more_in_form"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    tail = r.stdout.decode()[-3000:]
    assert r.returncode == 0 and " passed" in tail, tail
