"""orbm_pnp_ransac on the device against orbm_pnp_ransac_host, byte for byte: every hypothesis record, count and mask word, every refined
record and its mask.  The shapes are the smallest at which the three kernels can go wrong: N around the 64 correspondences of a mask
word, H around the 16 hypotheses of a k_pnp_hyp workgroup (and the 32 / 64 of the other forms the kernel could have taken), refine sets
from 4 points to the whole problem, 0 .. ORBM_PNP_MAX_RECORDS + 1 records, unequal batches with empty problems, the host path for a
problem beyond ORBM_PNP_CAP, repeated calls and the growth of the staged block."""
import numpy as np
import pytest
import multi_orb_slam_amd as m
import pnp_worlds as pw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher():
    mt = m.Matcher(device=0)
    yield mt
    mt.close()


def same(dev, host):
    assert len(dev) == len(host)
    for b, (d, h) in enumerate(zip(dev, host)):
        for k, (x, y) in enumerate(zip(d, h)):
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), (b, ("hyp", "words", "refined", "refined_words")[k])


def both(matcher, problems):
    dev = matcher.pnp_ransac(problems)
    host = m.pnp_ransac_host(problems)
    same(dev, host)
    return dev


def cut(w, H, best_start=None, min_inliers=None):
    w = dict(w)
    if min_inliers is not None:
        w["min_inliers"] = min_inliers
    return pw.problem(m, w, best_start=best_start, quads=w["quads"][:H])


@pytest.mark.parametrize("N", [4, 63, 64, 65, 300])
def test_sizes_around_a_mask_word(matcher, N):
    # 30 % wrong correspondences (none among four), 1 px of noise, min_inliers low enough for records: refine sets between 4 points and
    # most of N
    w = pw.world(N, 0.0 if N == 4 else 0.3, 1.0, seed=200 + N, H=40, min_inliers=4)
    dev = both(matcher, [pw.problem(m, w)])
    assert len(dev[0][2]) >= 1 and matcher.last_pnp()[:2] == (1, 0)


@pytest.mark.parametrize("H", [0, 1, 15, 16, 17, 31, 32, 33, 64, 65, 300, 1024])
def test_hypothesis_counts_around_the_workgroup(matcher, H):
    w = pw.world(65, 0.3, 0.0, seed=300, H=max(H, 1))
    dev = both(matcher, [cut(w, H)])
    assert len(dev[0][0]) == H


def test_refine_sets_from_four_points_to_all(matcher):
    sizes = set()
    probs = []
    for N, bad, mi in ((4, 0.0, 4), (5, 0.0, 4), (64, 0.0, 4), (65, 0.0, 4), (300, 0.0, 4), (300, 0.6, 4), (20, 0.75, 4)):
        probs.append(pw.problem(m, pw.world(N, bad, 0.0, seed=400 + N + int(bad * 100), H=24, min_inliers=mi)))
    dev = both(matcher, probs)
    for d in dev:
        sizes |= set(int(x) for x in d[2]["n_set"])
    assert {4, 5, 64, 65, 300} <= sizes, sizes


def test_hand_built_cases(matcher):
    worlds = pw.hand_built()
    dev = both(matcher, [pw.problem(m, w) for w in worlds])
    by = {w["name"]: d for w, d in zip(worlds, dev)}
    for name in ("coplanar", "collinear", "two_coincident", "four_coincident"):
        assert by[name][0]["flags"][0] & m.PNP_FLAG_RANDOM_SVD, name


def test_record_counts_and_the_host_tail(matcher):
    w = pw.many_records()
    host = m.pnp_ransac_host([pw.problem(m, w)])[0]
    rec = [int(h) for h in host[2]["hyp"]]
    assert len(rec) > m.PNP_MAX_RECORDS + 1
    for n_rec in (0, 1, m.PNP_MAX_RECORDS, m.PNP_MAX_RECORDS + 1):
        H = rec[n_rec - 1] + 1 if n_rec else rec[0]          # the hypotheses up to and including record n_rec - 1
        dev = both(matcher, [cut(w, H)])
        assert len(dev[0][2]) == n_rec
        assert matcher.last_pnp() == (1, 0, min(n_rec, m.PNP_MAX_RECORDS), max(0, n_rec - m.PNP_MAX_RECORDS))
    # best_start above every count: no record at all
    dev = both(matcher, [cut(w, len(w["quads"]), best_start=10 ** 6)])
    assert len(dev[0][2]) == 0 and matcher.last_pnp()[2:] == (0, 0)
    # a continuation block: best_start inside the range of the counts
    both(matcher, [cut(w, len(w["quads"]), best_start=int(np.median(host[0]["n_inliers"])))])


@pytest.mark.parametrize("B", [1, 2, 8, 64])
def test_batches_of_unequal_problems(matcher, B):
    sizes = [65, 0, 4, 300, 63, 17, 64, 130]
    probs = []
    for b in range(B):
        N = sizes[b % len(sizes)]
        H = 0 if N == 0 else (1 + (7 * b) % 23)
        probs.append(cut(pw.world(max(N, 4), 0.3, 1.0, seed=500 + b, H=max(H, 1), min_inliers=4), H) if N else
                     m.PnPProblem(pw.K, np.zeros((0, 3)), np.zeros((0, 2)), np.zeros(0), np.zeros((0, 4)), 4))
    both(matcher, probs)
    assert matcher.last_pnp()[:2] == (B, 0)


def test_a_problem_beyond_the_capacity_takes_the_host_path(matcher):
    big = cut(pw.world(m.PNP_CAP + 1, 0.3, 0.0, seed=600, H=3), 3)
    small = cut(pw.world(65, 0.3, 0.0, seed=601, H=20), 20)
    both(matcher, [small, big])
    assert matcher.last_pnp()[:2] == (1, 1)
    both(matcher, [big])
    assert matcher.last_pnp() == (0, 1, 0, 0)


def test_repeated_calls_growth_and_an_unrelated_search_between():
    matcher = m.Matcher(device=0)               # its own: nothing is allocated before the first call
    assert matcher.pnp_buffers() == (0, 0, 0)
    small = [cut(pw.world(63, 0.3, 1.0, seed=700, H=9, min_inliers=4), 9)]
    large = [cut(pw.world(300, 0.3, 1.0, seed=701 + b, H=70, min_inliers=4), 70) for b in range(3)]
    first = both(matcher, small)
    b_small = matcher.pnp_buffers()
    assert all(v > 0 for v in b_small)
    both(matcher, large)                        # the staged block, the device block and the mapped block grow
    b_large = matcher.pnp_buffers()
    assert all(l > s for l, s in zip(b_large, b_small)), (b_small, b_large)
    again = both(matcher, small)                # ... and are reused by a smaller call
    assert matcher.pnp_buffers() == b_large
    same(first, again)
    # an unrelated search on the same matcher, then the same call once more
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    matcher.hamming_matrix(a, a)
    same(first, matcher.pnp_ransac(small))
    assert matcher.pnp_buffers() == b_large
    matcher.close()
