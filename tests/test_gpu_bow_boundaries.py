"""GPU half of the boundary tests of the BoW-gated searches: every world of tests/bow_boundary_worlds.py through k_bow_join / k_bow_finish
(csrc/bow.hip) in every form of the join -- one wave per node, four waves, four waves with more than two rounds per stripe, the largest
node that is staged whole in LDS, the smallest with a tail read from HBM, the smallest whose tail reaches a third stripe -- and in all
three modes (SearchByBoW(KF, F), SearchByBoW(KF, KF), SearchForTriangulation), through the plain calls and through resident keyframes,
every match word against the oracle: the number of differing words is zero, no island is left out.  The node sizes of the forms come
from enqueue_join's arithmetic restated in bow_boundary_worlds.join_form, and every call asserts the form it ran through
BowSearch.last_join(): a moved threshold fails the test instead of quietly running another kernel.  The worlds are built and checked on
the CPU (tests/test_bow_boundary_worlds.py); a mismatch is reported by the groups and sides of the islands that differ.  Every call is
made twice on the same workspace."""
import functools
import numpy as np
import pytest
import torch  # noqa: F401  (first: torch ships its own HIP runtime)
import multi_orb_slam_amd as m
import oracle
import bow_boundary_worlds as bw

pytestmark = pytest.mark.gpu
SIZES = bw.form_sizes()


@pytest.fixture(scope="module")
def search():
    S = m.BowSearch()
    yield S
    S.close()


def to_side(s):
    fv = m.FeatureVector(s["node_id"], s["node_start"], s["items"])
    return m.BowSide(s["desc"], s["angle"], fv, s["flags"], s["x"], s["y"], s["octave"], s["cam_of"])


@functools.lru_cache(None)
def expected(kind, size, nnratio, th, population, mode):
    """The oracle's answer: computed once, shared by the plain and the resident runs, never written to."""
    w = world(kind, size, nnratio, th, population)
    nm, match = bw.run(oracle.search_by_bow, oracle.search_for_triangulation, w, mode)
    match.setflags(write=False)
    return nm, match


def world(kind, size, nnratio=None, th=None, population=None):
    return bw.bow_world(size, nnratio, th) if kind == "bow" else bw.rotation_world(population, size) if kind == "rotation" else bw.tri_world(size)


def device(S, w, mode, A, B, resident, flags_a=None, flags_b=None):
    th, r = w["th"], w["nnratio"]
    if mode == 2:
        T = w.get("tri") or bw.tri_params()
        args = (T["F12"], T["ex"], T["ey"], T["sf"], T["s2"])
        got = S.search_for_triangulation_resident(A, B, *args, flags_a, flags_b, th, True) if resident else S.search_for_triangulation(A, B, *args, th, True)
    else:
        got = S.search_by_bow_resident(A, B, mode, flags_a, flags_b, th, r, True) if resident else S.search_by_bow(A, B, mode, th, r, True)
    waves, lds = bw.join_form(w["size"])
    assert S.last_join() == (waves, w["size"], lds, mode), (S.last_join(), w["size"], mode)      # the form this world was built for
    return got


def run_worlds(S, cases, modes):
    """cases: [(name, key of expected() without the mode)].  Plain and resident, each twice -> the differences, by island."""
    differing, islands, words = [], 0, 0
    for name, key in cases:
        w = world(*key)
        sa, sb = to_side(w["a"]), to_side(w["b"])
        ka, kb = S.keyframe(sa), S.keyframe(sb)
        for mode in modes:
            onm, omatch = expected(*key, mode)
            for resident in (False, True):
                for again in (0, 1):
                    nm, match = device(S, w, mode, ka if resident else sa, kb if resident else sb, resident)
                    bad = int((match != omatch).sum())
                    if bad or nm != onm:
                        differing.append("%s mode %d %s call %d: %d words, nmatches %d vs %d: %s" % (
                            name, mode, "resident" if resident else "plain", again, bad, nm, onm, bw.kinds_of_differences(w, mode, match, omatch)))
            islands += len(w["islands"]); words += len(omatch)
        ka.close(); kb.close()
    print("%d islands, %d match words per run" % (islands, words))
    return differing


def bow_cases(key):
    return [("bow_%s_%g" % (key, r), ("bow", SIZES[key], r, 30 if r == bw.RATIOS[0] else 50, None)) for r in bw.RATIOS + (bw.TIE_RATIO,)]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("key", list(SIZES))
def test_search_by_bow_boundaries(search, key, mode):
    differing = run_worlds(search, bow_cases(key), (mode,))
    assert not differing, differing


@pytest.mark.parametrize("key", list(SIZES))
def test_search_for_triangulation_boundaries(search, key):
    differing = run_worlds(search, [("tri_%s" % key, ("tri", SIZES[key], None, None, None))], (2,))
    assert not differing, differing


@pytest.mark.parametrize("key", list(SIZES))
def test_rotation_boundaries(search, key):
    """The nine histogram populations, each in all three modes: the bins' edges, the wrap to 360, the 0.1f edges of ComputeThreeMaxima."""
    cases = [("rotation_%s_%s" % (p, key), ("rotation", SIZES[key], None, None, p)) for p in bw.POPULATIONS]
    differing = run_worlds(search, cases, (0, 1, 2))
    assert not differing, differing


@pytest.mark.parametrize("key", ["one_wave", "tail"])
def test_flags_of_the_call_replace_the_uploaded_ones(search, key):
    """Keyframes uploaded with every feature usable and monocular; the calls carry the worlds' own flags."""
    differing = []
    for name, wkey, modes in ((bow_cases(key)[1] + ((0, 1),)), ("tri_%s" % key, ("tri", SIZES[key], None, None, None), (2,))):
        w = world(*wkey)
        blank = lambda s: dict(s, flags=np.ones(len(s["flags"]), np.uint8))
        assert (w["a"]["flags"] != 1).any() and (w["b"]["flags"] != 1).any()
        ka, kb = search.keyframe(to_side(blank(w["a"]))), search.keyframe(to_side(blank(w["b"])))
        for mode in modes:
            onm, omatch = expected(*wkey, mode)
            for again in (0, 1):
                nm, match = device(search, w, mode, ka, kb, True, w["a"]["flags"], w["b"]["flags"])
                if nm != onm or not np.array_equal(match, omatch):
                    differing.append("%s mode %d call %d: %s" % (name, mode, again, bw.kinds_of_differences(w, mode, match, omatch)))
            # ... and without them the uploaded flags hold: another answer, the oracle's for the blank flags
            bnm, bmatch = bw.run(oracle.search_by_bow, oracle.search_for_triangulation, w, mode, True, blank(w["a"]), blank(w["b"]))
            nm, match = device(search, w, mode, ka, kb, True)
            assert not np.array_equal(bmatch, omatch)
            if nm != bnm or not np.array_equal(match, bmatch):
                differing.append("%s mode %d uploaded flags: %d words" % (name, mode, int((match != bmatch).sum())))
        ka.close(); kb.close()
    assert not differing, differing
