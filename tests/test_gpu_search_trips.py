"""The search chain's prologues after they were reshaped to one trip to memory per stage (csrc/project_dev.h: the motion path of
project_wave gathers its query with ONE vector load and takes the camera from a ballot; csrc/search.hip: k_resolve_mono issues every
set-up load with clamped indices before its first wait).  Nothing of that may show in a result: every case is bit-exact against the
oracle's sequential search / front end.

Resolve set-up, through the matcher's query-record search on synthetic frames:
  * nq at the lane, slot, register and worklist boundaries of T = 1024 threads with RQ = 2 queries each;
  * frame capacities of 1, 1 024, 1 025 and 2 048 features (zero, one, one-and-a-bit and two rounds of the table initialisation);
  * the last query and the last feature carry a pick of their own (`pin_last`): a clamped load that leaked into a neighbour's slot
    would bring that pick along.
Motion prologue, through front-end steps on small images (three steps ahead: k_project; isolated: k_project_side):
  * one to four cameras, one camera blank at the first, a middle and the last position, totals that are no multiple of four,
    octave 0 and the highest octave, a 16-level pyramid (both ends of the scale select), features without depth."""
import functools

import numpy as np
import pytest

import helpers
import oracle

pytestmark = pytest.mark.gpu

T_THREADS, RQ = 1024, 2


# ---------------------------------------------------------------------------------------------------------------- resolve set-up
def pin_last(fr, q):
    """The last feature of the frame moves inside the image; the last query (and the one before it, which then takes the feature
    first: it blocks) becomes an exact copy of it -- distance 0, every level, rotation 0."""
    n = len(fr["un_x"])
    g = n - 1
    fr["un_x"][g] = np.float32(100.5); fr["un_y"][g] = np.float32(80.25)
    desc = np.concatenate(fr["descs"])[g]
    for i in range(max(len(q) - 2, 0), len(q)):
        q["u"][i] = fr["un_x"][g]; q["v"][i] = fr["un_y"][g]
        q["radius"][i] = np.float32(15.0)
        q["ur"][i] = fr["uright"][g] if fr["uright"][g] > 0 else q["u"][i] - np.float32(20.0)
        q["min_level"][i] = 0; q["max_level"][i] = -1
        q["cam"][i] = fr["cam_of"][g]; q["blocks"][i] = 1
        q["angle"][i] = fr["angle"][g]
        q["desc"][i] = desc


@pytest.fixture(scope="module")
def matcher():
    import multi_orb_slam_amd as m
    mt = m.Matcher(0.8, True)
    yield mt
    mt.close()


@functools.lru_cache(maxsize=None)
def _world(n_per_cam, nq_max, seed):
    fr = helpers.make_frame_arrays(list(n_per_cam), 640, 480, seed)
    q = helpers.make_queries(fr, nq_max, seed + 40, th=15.0, blocks=2)
    return fr, q


def _search_equals_oracle(matcher, fr, q, want_forms):
    import multi_orb_slam_amd as m
    F = matcher.frame(m.FrameData(**fr)); OF = oracle.FrameData(**fr)
    n = len(fr["un_x"])
    try:
        for check_ori in (True, False):
            matcher.check_orientation = check_ori
            got_n, got = matcher.SearchByProjection(F, q)
            assert matcher.last_resolve_form()[0] in want_forms, matcher.last_resolve_form()
            exp_n, exp = oracle.search_by_projection_frames(OF, q, 100, check_ori)
            assert got_n == exp_n and np.array_equal(got, exp)
        assert exp[n - 1] >= len(q) - 2 and exp[n - 1] >= 0      # (without the rotation check: the pinned pick is somebody's match)
    finally:
        matcher.check_orientation = True
        F.close()


@pytest.mark.parametrize("nq", [1, 63, 64, 65, T_THREADS - 1, T_THREADS, T_THREADS + 1, RQ * T_THREADS - 1, RQ * T_THREADS,
                                RQ * T_THREADS + 1])
def test_resolve_setup_at_the_query_boundaries(matcher, nq):
    from multi_orb_slam_amd import matcher as mm
    fr0, q0 = _world((700, 500), RQ * T_THREADS + 1, 3)
    fr = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in fr0.items()}
    q = q0[:nq].copy()
    pin_last(fr, q)
    forms = (mm.FORM_MONO2_ANG,) if nq <= RQ * T_THREADS else (mm.FORM_MONO4_WORKLIST, mm.FORM_MONO4_WAVES)
    _search_equals_oracle(matcher, fr, q, forms)


@pytest.mark.parametrize("capacity", [1, T_THREADS, T_THREADS + 1, 2 * T_THREADS])
def test_resolve_setup_at_the_table_initialisation_rounds(matcher, capacity):
    from multi_orb_slam_amd import matcher as mm
    n_per_cam = (capacity,) if capacity == 1 else (capacity // 2, capacity - capacity // 2)
    fr0, q0 = _world(n_per_cam, 301, 7 + capacity)
    fr = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in fr0.items()}
    q = q0.copy()
    pin_last(fr, q)
    assert len(fr["un_x"]) == capacity
    _search_equals_oracle(matcher, fr, q, (mm.FORM_MONO2_ANG,))


# ---------------------------------------------------------------------------------------------------------------- motion prologue
W, H, STEPS = 320, 240, 5
BLANK = -1   # (a camera that sees a uniform image: no features, two equal consecutive camera starts)

# name -> (width, height, per camera (nfeatures, scale_factor, nlevels), blank camera or None)
RIGS = {
    "1cam": (W, H, ((150, 1.2, 8),), None),
    "2cams": (W, H, ((150, 1.2, 8), (100, 1.2, 8)), None),
    "3cams": (W, H, ((150, 1.2, 8), (100, 1.2, 8), (120, 1.2, 8)), None),
    "4cams": (W, H, ((150, 1.2, 8),) * 4, None),
    "blank_first": (W, H, ((150, 1.2, 8),) * 3, 0),
    "blank_middle": (W, H, ((150, 1.2, 8),) * 3, 1),
    "blank_last": (W, H, ((150, 1.2, 8),) * 3, 2),
    "16levels": (480, 360, ((400, 1.12, 16), (200, 1.12, 16)), None),
}


def _frames(name):
    from multi_orb_slam_amd import synth
    w, h, cams, blank = RIGS[name]
    return [[np.full((h, w), 128, np.uint8) if c == blank else synth.image(c, t, w, h) for c in range(len(cams))] for t in range(STEPS)]


def _params(name):
    import multi_orb_slam_amd as m
    return [m.ExtractorParams(nfeatures=nf, scale_factor=sf, nlevels=nl) for nf, sf, nl in RIGS[name][2]]


@functools.lru_cache(maxsize=None)
def _oracle_steps(name):
    from oracle_pipeline import OracleFrontEnd
    w, h, _, _ = RIGS[name]
    ofe = OracleFrontEnd(_params(name), w, h)
    return [ofe.step(imgs) for imgs in _frames(name)]


@pytest.mark.parametrize("ahead", [3, 0], ids=["three_ahead", "isolated"])
@pytest.mark.parametrize("name", list(RIGS))
def test_motion_prologue_steps_equal_oracle(name, ahead):
    import torch  # noqa: F401  (before libmorb, as in test_gpu_frontend.py)
    from multi_orb_slam_amd import pipeline
    from oracle_pipeline import assert_same_step
    w, h, cams, blank = RIGS[name]
    exp = _oracle_steps(name)
    # what the case is for, read off the oracle's steps (the queries of step t are the features of step t - 1)
    sources = exp[:-1]
    assert all(sum(s["counts"]) > 100 for s in sources)
    if blank is not None:
        assert all(s["counts"][blank] == 0 for s in exp)
    assert any(sum(s["counts"]) % 4 != 0 for s in sources)                       # the last workgroup has idle waves
    nlevels = cams[0][2]
    assert all(s["kps"]["octave"].min() == 0 and s["kps"]["octave"].max() == nlevels - 1 for s in sources)
    assert all((s["depth"] <= 0).any() and (s["depth"] > 0).any() for s in sources)
    assert exp[-1]["n_temporal"] > 50
    frames = _frames(name)
    fe = pipeline.FrontEnd(_params(name), w, h)
    try:
        announced = 0
        for t in range(STEPS):
            while announced < min(t + ahead, STEPS - 1):
                announced += 1
                fe.announce(frames[announced])
            announced = max(announced, t)
            assert_same_step(fe.step(frames[t]), exp[t])
    finally:
        fe.close()
