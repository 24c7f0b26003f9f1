"""PnPsolver on the host: orbm_pnp_ransac_host, orbm_pnp_walk, orbm_pnp_parameters and the three hooks against tests/pnp_model.py, the
NumPy model written from the reference's PnPsolver.cc and OpenCV's semantics.  Records, counts, mask words and refined records are
compared byte for byte; the model's own coverage (how the call sequences end, which branches the hand-built cases reach) is asserted
so that nothing passes vacuously.  No device is needed."""
import numpy as np
import pytest
import multi_orb_slam_amd as m
from multi_orb_slam_amd._lib import ORB_E_ARG
import pnp_model as pm
import pnp_worlds as pw

_cache = {}


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def solved(key, make):
    """(worlds, model results, host results) of a world set, computed once and shared."""
    if key not in _cache:
        worlds = make()
        model = pm.ransac_multi(worlds)
        host = []
        for k in range(0, len(worlds), m.PNP_MAX_BATCH):
            host += m.pnp_ransac_host([pw.problem(m, w) for w in worlds[k:k + m.PNP_MAX_BATCH]])
        _cache[key] = (worlds, model, host)
    return _cache[key]


def assert_same(w, mod, got):
    """Every field of every hypothesis record, every count and mask word, every refined record and its mask."""
    hyp, words, ref, rwords = got
    name = w["name"]
    assert len(hyp) == len(w["quads"]), name
    for f, k in (("R", "R"), ("t", "t"), ("rep_error", "err")):
        wd = {"R": 9, "t": 3, "rep_error": 1}[f]
        diff = (bits(hyp[f]).reshape(len(hyp), wd) != bits(mod[k]).reshape(len(hyp), wd)).any(axis=1)
        assert not diff.any(), (name, f, np.nonzero(diff)[0][:5])
    assert (hyp["choice"] == mod["choice"]).all(), name
    assert (hyp["flags"] == mod["flags"]).all(), name
    assert (hyp["reserved"] == 0).all(), name
    assert (hyp["n_inliers"] == mod["n_inliers"]).all(), name
    assert (words == mod["words"]).all(), name
    assert list(ref["hyp"]) == list(mod["rec"]), name
    assert (ref["n_set"] == mod["ref_n_set"]).all() and (ref["n_inliers"] == mod["ref_n_inliers"]).all() and (ref["flags"] == mod["ref_flags"]).all(), name
    assert (bits(ref["R"]).reshape(len(ref), 9) == bits(mod["ref_R"]).reshape(len(ref), 9)).all(), name
    assert (bits(ref["t"]).reshape(len(ref), 3) == bits(mod["ref_t"]).reshape(len(ref), 3)).all(), name
    assert (rwords == mod["ref_words"]).all(), name


def model_sequence(w, mod):
    """Every iterate(5, ...) of a fresh solver until bNoMore or a success, on the model -> (how it ended, records refined on the way)."""
    N = len(w["p3dw"])
    max_its = min(pm.parameters(N)[0], len(w["quads"]))
    it = pm.IterateModel(N, w["min_inliers"], max_its)
    refined = {h: int(n) for h, n in zip(mod["rec"], mod["ref_n_inliers"])}
    tried = []

    def refine(h):
        if h not in tried:
            tried.append(h)
        return refined[h]
    while True:
        ans, no_more, idx = it.iterate(5, mod["n_inliers"], refine)
        if ans != "nothing" or no_more:
            return ans, tried


SETS = [("seeded", pw.seeded_worlds), ("decoy", pw.decoy_worlds), ("hand", pw.hand_built), ("many", lambda: [pw.many_records()])]


@pytest.mark.parametrize("key,make", SETS, ids=[s[0] for s in SETS])
def test_host_routine_equals_model(key, make):
    worlds, model, host = solved(key, make)
    for w, mod, got in zip(worlds, model, host):
        assert_same(w, mod, got)


def test_seeded_worlds_cover_every_ending():
    endings = set()
    for key, make in SETS[:2]:
        worlds, model, _ = solved(key, make)
        for w, mod in zip(worlds, model):
            ans, tried = model_sequence(w, mod)
            if ans == "refined":
                endings.add("refined_first" if len(tried) == 1 else "refined_later")
            else:
                endings.add(ans)
    assert endings == {"refined_first", "refined_later", "best", "nothing"}, endings


def test_seeded_worlds_reach_every_choice_and_octave():
    worlds, model, _ = solved(*SETS[0])
    choices = set()
    for mod in model:
        choices |= set(int(c) for c in mod["choice"])
    assert choices == {1, 2, 3}
    assert all(len(set(w["max_err"].tolist())) == min(len(w["p3dw"]), pw.LEVELS) for w in worlds)


def test_hand_built_cases_reach_their_branches():
    worlds, model, host = solved(*SETS[2])
    by = {w["name"]: (w, mod) for w, mod in zip(worlds, model)}
    # exactly degenerate quadruples: a singular value is exactly zero and cvSVD completes U with random vectors
    for name in ("coplanar", "collinear", "two_coincident", "four_coincident"):
        assert by[name][1]["flags"][0] & pm.FLAG_RANDOM_SVD, name
    # a general quadruple in the same problem does not
    assert not by["coplanar"][1]["flags"][2] & pm.FLAG_RANDOM_SVD
    # the point at depth 0 is no inlier of a finite pose, and nothing else of its row is disturbed
    w, mod = by["depth_zero"]
    assert mod["n_inliers"][0] == 11 and not (int(mod["words"][0, 0]) >> 11) & 1
    # behind the camera first: solve_for_sign makes pcs[2] -- the depth of the quadruple's FIRST point -- positive.  The order that
    # starts with a point in front of the camera recovers the pose (and leaves point 0 behind the camera, at its true depth of -3); the
    # order that starts with the point behind the camera is forced onto the mirrored configuration and cannot fit.  Both branches of
    # the sign test are taken among the approximations, and differently in the two orders.
    w, mod = by["behind_first"]
    assert np.isfinite(mod["R"]).all()
    depth = lambda h, i: float(mod["R"][h][2] @ w["p3dw"][i].astype(np.float64) + mod["t"][h][2])
    assert mod["err"][1] < 1e-3 and depth(1, 1) > 0 and abs(depth(1, 0) + 3.0) < 1e-3
    assert mod["err"][0] > 1.0
    q = w["quads"]
    sign = pm.compute_pose(w["p3dw"][q].astype(np.float64), w["p2d"][q].astype(np.float64),
                           np.tile([float(np.float32(k)) for k in w["K"]], (len(q), 1)))["neg"]
    assert sign.any() and not sign.all() and (sign[0] != sign[1]).any()
    # N below, at and one above min_inliers: records need n_inliers >= 8
    assert by["N7_min8"][1]["rec"] == [] and max(by["N7_min8"][1]["n_inliers"]) <= 7
    assert len(by["N8_min8"][1]["rec"]) >= 1 and len(by["N9_min8"][1]["rec"]) >= 1
    assert (by["N8_min8"][1]["ref_n_inliers"] == 8).all()      # Refine() cannot succeed: 8 > 8 is false
    assert (by["N9_min8"][1]["ref_n_inliers"] == 9).any()
    worlds, model, host = solved(*SETS[3])
    assert len(model[0]["rec"]) > m.PNP_MAX_RECORDS
    assert len(host[0][2]) == len(model[0]["rec"])


def test_walk_equals_the_transcription_of_iterate():
    rng = np.random.default_rng(3)
    for trial in range(300):
        N = int(rng.integers(4, 60)); min_inl = int(rng.integers(4, 12)); max_its = int(rng.integers(1, 40)); n_it = int(rng.integers(1, 8))
        total = max_its + 60
        counts = rng.integers(0, N + 1, total).astype(np.int32)
        counts[rng.random(total) < 0.6] = rng.integers(0, min_inl)       # most hypotheses fail
        refined_of = {h: int(rng.integers(max(0, min_inl - 2), min_inl + (3 if rng.random() < 0.3 else 1))) for h in range(total)}
        it = pm.IterateModel(N, min_inl, max_its)
        st = m.pnp_walk_state()
        block = int(rng.integers(3, 50))        # hypotheses evaluated per block: the first block holds max_its of them
        start, size = 0, max_its
        calls = 0
        while calls < 12:
            calls += 1
            want = it.iterate(n_it, counts, lambda h: refined_of[h])
            while True:
                cnt = counts[start:start + size]
                rec = pm.records(cnt, min_inl, int(st["best_inliers"][0]) if start else 0)
                got = m.pnp_walk(cnt, start, rec, [refined_of[start + h] for h in rec], N, min_inl, max_its, n_it, st)
                if not st["exhausted"][0]:
                    break
                start, size = start + size, block      # a continuation block, best_start = the current best
                st["best_record"] = -1
            name = {m.PNP_WALK_NOTHING: "nothing", m.PNP_WALK_REFINED: "refined", m.PNP_WALK_BEST: "best"}[got]
            assert (name, bool(st["no_more"][0])) == want[:2], (trial, calls)
            assert int(st["iterations"][0]) == it.iterations and int(st["best_inliers"][0]) == it.best_inliers and int(st["best_hyp"][0]) == it.best_hyp
            if name != "nothing":
                assert want[2] == int(st["best_hyp"][0])
            if it.iterations + n_it + 1 >= total - block:
                break


def test_parameters_equal_the_model():
    for N in list(range(0, 70)) + [100, 125, 300, 1000, 2000, 8200]:
        for min_inl in (4, 8, 10, 25):
            for eps in (0.4, 0.5, 0.25):
                got = m.pnp_parameters(N, 0.99, min_inl, 300, 4, eps)
                want = pm.parameters(N, 0.99, min_inl, 300, 4, eps)
                assert got[:2] == want[:2] and np.float32(got[2]).tobytes() == np.float32(want[2]).tobytes(), (N, min_inl, eps, got, want)
    assert m.pnp_parameters(8)[:2] == (1, 8)            # N == minInliers
    assert m.pnp_parameters(20, epsilon=0.5)[1] == 10   # N*epsilon exactly integral
    assert m.pnp_parameters(4)[:2] == (1, 8)            # N = 4: below the minimum; ceil of a NaN, converted as x86 does


def test_qr_solve_hook_and_its_singular_return():
    rng = np.random.default_rng(9)
    for _ in range(50):
        A = rng.normal(size=(6, 4)); b = rng.normal(size=6)
        x, sing = m.pnp_qr_solve(A, b)
        mx, ms = pm.qr_solve(A[None], b[None], np.zeros((1, 4)))
        assert not sing and not ms[0] and bits(x).tolist() == bits(mx[0]).tolist()
        assert np.allclose(x, np.linalg.lstsq(A, b, rcond=None)[0], rtol=1e-9, atol=1e-12)
    # an all-zero column: the return leaves x as it was (the definition of include/orbm.h), and the flag says so
    A = rng.normal(size=(6, 4)); A[:, 2] = 0
    x0 = np.array([1.5, -2.5, 3.5, -4.5])
    x, sing = m.pnp_qr_solve(A, rng.normal(size=6), x0)
    assert sing and bits(x).tolist() == bits(x0).tolist()
    mx, ms = pm.qr_solve(A[None], np.ones((1, 6)), x0[None])
    assert ms[0] and bits(mx[0]).tolist() == bits(x0).tolist()
    # the first loop never looks at the last row: a column that is zero but for its last element is singular too
    A = rng.normal(size=(6, 4)); A[:5, 0] = 0
    assert m.pnp_qr_solve(A, np.ones(6))[1] and pm.qr_solve(A[None], np.ones((1, 6)), np.zeros((1, 4)))[1][0]


def test_compute_pose_hook_equals_model():
    rng = np.random.default_rng(10)
    for n in (4, 5, 17, 100):
        w = pw.world(max(n, 4), 0.0, 1.0, seed=50 + n)
        pws = w["p3dw"][:n].astype(np.float64); us = w["p2d"][:n].astype(np.float64)
        R, t, err, choice, flags = m.pnp_compute_pose(pws, us, [float(np.float32(k)) for k in w["K"]])
        mod = pm.compute_pose(pws[None], us[None], np.array([[float(np.float32(k)) for k in w["K"]]]))
        assert bits(R).tolist() == bits(mod["R"][0]).tolist() and bits(t).tolist() == bits(mod["t"][0]).tolist()
        assert bits(err).tolist() == bits(mod["err"][0]).tolist() and choice == mod["choice"][0] and flags == mod["flags"][0]


def test_bad_arguments_are_refused_and_the_edges_accepted():
    """The checks the port shares with Sim3 (ransac_validate, csrc/ransac_dev.h), on the smallest shapes: every refusal one step beyond
    its limit, and the limit itself accepted, so that a `<` turned `<=` fails on one side or the other."""
    w = pw.world(4, 0.0, 0.0, seed=31, H=1)
    run = lambda quads, copies=1: m.pnp_ransac_host([pw.problem(m, w, quads=np.asarray(quads, np.int32))] * copies)
    tile = lambda H: np.tile(np.array([0, 1, 2, 3], np.int32), (H, 1))
    for refused in (lambda: run([[0, 1, 2, -1]]),                    # a position before the problem
                    lambda: run([[0, 1, 2, 4]]),                     # position n
                    lambda: run(tile(1), m.PNP_MAX_BATCH + 1),
                    lambda: run(tile(m.PNP_MAX_ITS + 1))):
        with pytest.raises(m.OrbError) as e:
            refused()
        assert e.value.code == ORB_E_ARG
    (hyp, words, _, _), = run([[3, 2, 1, 0]])                        # position n - 1
    assert len(hyp) == 1 and words.shape == (1, 1) and np.isfinite(hyp["R"]).all()
    one, = run(tile(1))
    batch = run(tile(1), m.PNP_MAX_BATCH)
    assert len(batch) == m.PNP_MAX_BATCH
    assert all(got[0].tobytes() == one[0].tobytes() and got[1].tobytes() == one[1].tobytes() for got in batch)
    (hyp, words, _, _), = run(tile(m.PNP_MAX_ITS))
    assert len(hyp) == m.PNP_MAX_ITS and words.shape == (m.PNP_MAX_ITS, 1)
    assert hyp.tobytes() == one[0].tobytes() * m.PNP_MAX_ITS and (words == one[1][0, 0]).all()
