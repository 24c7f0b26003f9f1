"""The resident keyframe database on the MI355X against the model (tests/kfdb_model.py) and the oracle's L1 score: everything bit-exact
(== on integers, .tobytes() on doubles).  The fixtures' non-vacuity is asserted on the model alone in tests/test_kfdb_model.py."""
import os
import subprocess
import numpy as np
import pytest
import multi_orb_slam_amd as m
from multi_orb_slam_amd import synth
import kfdb_model as km
import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "multi_orb_slam_amd", "host", "test_kfdb")


def same_doubles(a, b):
    return np.asarray(a, np.float64).tobytes() == np.asarray(b, np.float64).tobytes()


class Mirror:
    """Drives the device database and the model's inverted file with the same operations (camera-1 file of the model)."""

    def __init__(self, n_words):
        self.db = m.KeyFrameDatabase(n_words)
        self.model = km.ModelDatabase(n_words)
        self.n_words = n_words
        self.frames = 0

    def add(self, k):
        self.db.add(k.mnId, k.bow1); self.model.add_cam1(k)

    def erase(self, k):
        self.db.erase(k.mnId); self.model.erase(k)

    def clear(self):
        self.db.clear(); self.model.clear()

    def check(self, queries, batch=True):
        """Every query as a relocalisation frame with a fresh id: sharing order, common of every entry, score of every entry above
        the reference's threshold -- and, stronger, the score of EVERY returned entry against the oracle."""
        frames = [km.FrameOf(10 ** 9 + self.frames + i, k) for i, k in enumerate(queries)]     # a fresh id each: nothing is "already met"
        self.frames += len(frames)
        got = self.db.query([f.bow1 for f in frames]) if batch else [self.db.query([f.bow1])[0] for f in frames]
        for f, (keys, common, score) in zip(frames, got):
            _, tr = self.model.detect_reloc(f)
            assert keys.tolist() == tr["met"] == tr["sharing"]
            assert common.tolist() == [tr["common"][i] for i in tr["sharing"]]
            by_key = dict(zip(keys.tolist(), score))
            assert len(tr["scored"]) > 0 or not tr["sharing"]
            for i, d in tr["scored"].items():
                assert same_doubles(by_key[i], d), (i, by_key[i], d)
        return got


@pytest.mark.parametrize("K", [120, 2000, 10000])
def test_query_equals_the_model_on_generated_worlds(K):
    w = km.World(K, seed=K)
    mr = Mirror(w.n_words)
    lap = K // 2
    asking = [w.kfs[lap + (j * 37 + 11) % (lap - 10)] for j in range(6)]
    skip = set(id(k) for k in asking)
    for k in w.kfs:
        if id(k) not in skip:
            mr.add(k)
    assert len(mr.db) == K - len(skip)
    got = mr.check(asking)
    assert min(len(g[0]) for g in got) >= 10
    # all scores of one query against the oracle, whatever their common count
    keys, _, score = got[0]
    by_id = {k.mnId: k for k in w.kfs}
    for key, s in zip(keys.tolist(), score):
        assert same_doubles(s, oracle.bow_score_l1(asking[0].bow1, by_id[key].bow1))


def test_interleaved_add_erase_readd_clear():
    w = km.World(200, seed=5)
    mr = Mirror(w.n_words)
    q = [w.kfs[150], w.kfs[161]]
    rest = [k for k in w.kfs if k not in q]
    for k in rest[:120]:
        mr.add(k)
    mr.check(q)
    for k in rest[10:120:3]:
        mr.erase(k)
    mr.check(q)
    for k in rest[10:120:6][::-1]:     # re-added in another order: they now come last among ties
        mr.add(k)
    for k in rest[120:]:
        mr.add(k)
    mr.check(q)
    mr.erase(w.kfs[150])               # unknown key: no-op
    mr.clear()
    assert len(mr.db) == 0
    assert [len(g[0]) for g in mr.db.query([q[0].bow1])] == [0]
    for k in rest[40:90]:
        mr.add(k)
    mr.check(q)


def test_across_arena_growth_and_compaction():
    # the arena starts at 65 536 words and doubles; ~800 words per keyframe: 400 keyframes cross two doublings
    w = km.World(420, seed=9)
    mr = Mirror(w.n_words)
    q = [w.kfs[300], w.kfs[333]]
    rest = [k for k in w.kfs if k not in q]
    total = 0
    for i, k in enumerate(rest):
        mr.add(k)
        total += len(k.bow1[0])
        if i in (60, 61, 130, 131, 300):
            mr.check(q[:1])
    assert total > 4 * 65536 // 2
    # erase until dead words exceed half of the arena (a compaction), checking on both sides of it
    for i, k in enumerate(rest[::2] + rest[1::4]):
        mr.erase(k)
        if i % 50 == 49:
            mr.check(q)
    mr.check(q)
    for k in rest[::2][:40]:
        mr.add(k)
    mr.check(q)


def test_one_query_and_eight_in_one_call_give_the_same_rows():
    w = km.World(300, seed=21)
    mr = Mirror(w.n_words)
    q = [w.kfs[i] for i in range(200, 280, 10)]
    for k in w.kfs:
        if k not in q:
            mr.add(k)
    a = mr.check(q, batch=True)
    b = mr.check(q, batch=False)
    assert len(a) == len(b) == 8
    for x, y in zip(a, b):
        assert x[0].tolist() == y[0].tolist() and x[1].tolist() == y[1].tolist() and x[2].tobytes() == y[2].tobytes()


def _random_bow(n, n_words, seed, scale=1.0):
    ids = np.sort(np.argsort(km._h(seed, 7, n_words), kind="stable")[:n]).astype(np.uint32)
    v = (1.0 + (km._h(seed, 8, n) % np.uint32(997)).astype(np.float64))
    return ids, v / v.sum() * scale


LENGTHS = [1, 63, 64, 65, 1500, 20000]


def test_entry_and_query_lengths_and_the_empty_query():
    # queries up to 4 096 words run from LDS, longer ones from global memory: 20 000 takes the general form
    n_words = 60000
    mr = Mirror(n_words)
    kfs = [km.KF(100 + i, _random_bow(n, n_words, 31 + i)) for i, n in enumerate(LENGTHS)]
    kfs += [km.KF(200 + i, _random_bow(n, n_words, 77 + i)) for i, n in enumerate(LENGTHS)]
    for k in kfs:
        mr.add(k)
    queries = [km.KF(900 + i, _random_bow(n, n_words, 131 + i)) for i, n in enumerate(LENGTHS)]
    for q in queries:
        got = mr.check([q])
        keys, common, score = got[0]
        for key, c, s in zip(keys.tolist(), common.tolist(), score):
            e = next(k for k in kfs if k.mnId == key)
            assert c == len(np.intersect1d(q.bow1[0], e.bow1[0]))
            assert same_doubles(s, oracle.bow_score_l1(q.bow1, e.bow1))
    got = mr.check(queries)      # mixed lengths in one call (the longest decides the form)
    assert sum(len(g[0]) for g in got) > 12
    empty = (np.zeros(0, np.uint32), np.zeros(0, np.float64))
    assert [len(g[0]) for g in mr.db.query([empty])] == [0]
    assert [len(g[0]) for g in mr.db.query([empty, queries[4].bow1])][0] == 0
    assert mr.db.query([]) == []


def test_a_query_that_shares_exactly_one_word_with_one_entry():
    mr = Mirror(1000)
    a = km.KF(1, (np.array([3, 500, 900], np.uint32), np.array([0.25, 0.5, 0.25])))
    b = km.KF(2, (np.array([4, 501, 901], np.uint32), np.array([0.5, 0.25, 0.25])))
    mr.add(a); mr.add(b)
    q = km.KF(9, (np.array([2, 5, 500, 902], np.uint32), np.array([0.125, 0.125, 0.5, 0.25])))
    keys, common, score = mr.check([q])[0]
    assert keys.tolist() == [1] and common.tolist() == [1]
    assert same_doubles(score[0], oracle.bow_score_l1(q.bow1, a.bow1)) and score[0] == 0.5


def test_tiny_values_keep_their_bits():
    # terms next to the double denormal range: |v - w| - |v| - |w| with v, w down to 1e-300 and below (5e-324 is the smallest denormal)
    n_words = 5000
    mr = Mirror(n_words)
    ids = np.arange(0, 4000, 2, dtype=np.uint32)
    tiny = np.array([1e-300, 3e-308, 2.2250738585072014e-308, 1e-310, 5e-324, 7e-320])
    va = np.where(np.arange(len(ids)) % 3 == 0, tiny[np.arange(len(ids)) % 6], 1e-3 / (1 + np.arange(len(ids))))
    vb = np.where(np.arange(len(ids)) % 2 == 0, tiny[(np.arange(len(ids)) + 1) % 6], 1e-305 * (1 + np.arange(len(ids))))
    e1, e2 = km.KF(1, (ids, va)), km.KF(2, (ids[::3], tiny[np.arange(len(ids[::3])) % 6]))
    mr.add(e1); mr.add(e2)
    q = km.KF(9, (ids, vb))
    keys, common, score = mr.check([q])[0]
    assert keys.tolist() == [1, 2] and common.tolist() == [len(ids), len(ids[::3])]
    for key, s in zip(keys.tolist(), score):
        exp = oracle.bow_score_l1(q.bow1, (e1 if key == 1 else e2).bow1)
        assert same_doubles(s, exp) and s != 0.0


def test_score_of_named_entries_generated_and_from_the_vocabulary():
    w = km.World(150, seed=3)
    db = m.KeyFrameDatabase(w.n_words)
    for k in w.kfs[:140]:
        db.add(k.mnId, k.bow)
    q = w.kfs[145]
    keys = [70, 71, 3, 139, 0, 72]
    got = db.score(q.bow, keys)
    assert same_doubles(got, [oracle.bow_score_l1(q.bow, w.kfs[i].bow) for i in keys])
    assert len(db.score(q.bow, [])) == 0
    with pytest.raises(m.OrbError) as e:
        db.score(q.bow, [70, 145])
    assert e.value.code == -1
    # BowVectors of the real producer: Vocabulary.bow_vectors on a synthetic tree
    voc = synth.vocabulary(10, 3)
    v = m.Vocabulary(voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"], voc["L"])
    nw = v.info()["n_words"]
    bows = [v.bow_vectors(synth.vocabulary_words(voc, 400 + 50 * i, seed=i % 4 + 1, flip_p=0.03 + 0.01 * (i % 3)))[0] for i in range(12)]
    db2 = m.KeyFrameDatabase(nw)
    for i, b in enumerate(bows[:10]):
        db2.add(i, b)
    for qb in bows[10:]:
        got = db2.score(qb, list(range(10)))
        assert same_doubles(got, [oracle.bow_score_l1(qb, b) for b in bows[:10]])
        assert same_doubles(got, [m.score_l1(qb, b) for b in bows[:10]])
        keys, common, score = db2.query([qb])[0]
        assert len(keys) >= 5
        for key, c, s in zip(keys.tolist(), common.tolist(), score):
            assert c == len(np.intersect1d(qb[0], bows[key][0])) and same_doubles(s, got[key])


def test_argument_errors_are_loud():
    db = m.KeyFrameDatabase(100)
    ok = (np.array([1, 5, 9], np.uint32), np.array([0.5, 0.25, 0.25]))
    db.add(7, ok)
    for bad in (lambda: db.add(7, ok),                                                              # duplicate key
                lambda: db.add(8, (np.array([5, 1, 9], np.uint32), ok[1])),                         # unsorted
                lambda: db.add(8, (np.array([1, 5, 5], np.uint32), ok[1])),                         # duplicate id
                lambda: db.add(8, (np.array([1, 5, 100], np.uint32), ok[1])),                       # id >= n_words
                lambda: db.query([(np.array([9, 5], np.uint32), np.array([0.5, 0.5]))]),            # unsorted query
                lambda: db.query([ok], capacity=0)):                                                # capacity too small
        with pytest.raises(m.OrbError) as e:
            bad()
        assert e.value.code == -1
    assert len(db) == 1
    db.add(8, ok)
    with pytest.raises(m.OrbError):
        db.query([ok], capacity=1)
    assert [g[0].tolist() for g in db.query([ok], capacity=2)] == [[7, 8]]


# --------------------------------------------------------------------------------------------------------- the C++ class
def run_driver(mode, world, out, timeout=120):
    r = subprocess.run(["timeout", "-k", "10", str(timeout), DRIVER, mode, str(world), str(out)], capture_output=True, text=True, timeout=timeout + 30)
    assert r.returncode == 0, (mode, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r


def class_against_model(tmp_path, n_words, kfs, ops, name):
    world, out_gpu, out_cpu = tmp_path / (name + ".bin"), tmp_path / (name + "_gpu.bin"), tmp_path / (name + "_cpu.bin")
    km.write_world(world, n_words, kfs, ops)
    exp = km.expected_out(km.run_script(n_words, kfs, ops))
    run_driver("run", world, out_gpu)
    run_driver("cpu", world, out_cpu)
    got, cpu = km.read_out(out_gpu, len(kfs)), km.read_out(out_cpu, len(kfs))
    assert len(got) == len(cpu) == len(exp) > 0
    for i, (g, c, e) in enumerate(zip(got, cpu, exp)):
        assert g[0] == e[0] == c[0], (i, g[0], e[0], c[0])
        assert g[1] == e[1], i
        assert c[1] == e[1], i
    return exp


@pytest.mark.parametrize("K", [120, 400])
def test_class_equals_model_and_host_restatement_on_generated_worlds(tmp_path, K):
    w = km.World(K, seed=K)
    exp = class_against_model(tmp_path, w.n_words, w.kfs, w.script(), "world%d" % K)
    assert max(len(ids) for ids, _ in exp) >= 2


def test_class_quirks(tmp_path):
    for name, (n_words, kfs, ops) in km.quirk_cases().items():
        class_against_model(tmp_path, n_words, kfs, ops, name)


def test_two_threads_through_the_class_mutex(tmp_path):
    # one thread adds 500 keyframes (camera 1), another asks for relocalisation candidates all the while; compared is only what does not
    # depend on the interleaving: both finish, and a query made after the join equals the model's.  The asking thread's frames look at
    # places 0..149 of the world, the last query at place 250: no keyframe the last query meets was marked or scored by the other thread
    # (the reference adds a marked neighbour's stale mRelocScore, so that would make the answer depend on the interleaving).
    w = km.World(520, seed=17)
    adds = [("add_cam1", t, 0, 0.0) for t in range(500)]
    last = [("reloc", 510, 777, 0.0)]
    world, out = tmp_path / "mt.bin", tmp_path / "mt_out.bin"
    km.write_world(world, w.n_words, w.kfs, adds + [("reloc", t, 0, -1.0) for t in range(0, 150, 7)] + last)
    r = run_driver("threads", world, out)
    assert "500 adds" in r.stderr
    exp = km.expected_out(km.run_script(w.n_words, w.kfs, adds + last))
    got = km.read_out(out, len(w.kfs))
    assert len(got) == 1 and got[0][0] == exp[0][0] and len(exp[0][0]) >= 1
    listed = 0
    for g, e in zip(got[0][1], exp[0][1]):
        if e[3] == 777:
            assert g[3:] == e[3:]
            listed += 1
    assert listed >= 10


def test_relocalisation_candidates_feed_search_by_bow(tmp_path):
    """The chain that motivated the database: DetectRelocalizationCandidates -> SearchByBoW per candidate (src/Tracking.cc:1979-2011).
    Keyframes are built on the device from the front end's resident features (a camera pair sliding over the synthetic scene); the
    candidates the class returns equal the model's, and the resident search on each equals the oracle's SearchByBoW."""
    from multi_orb_slam_amd import pipeline
    voc = synth.vocabulary(10, 3, seed=12)
    v = m.Vocabulary(voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"], voc["L"])
    ov = oracle.Vocabulary(voc)
    nw = v.info()["n_words"]
    bs = m.BowSearch()
    fe = pipeline.FrontEnd([m.ExtractorParams(nfeatures=600), m.ExtractorParams(nfeatures=400)], 320, 240)
    n_kf = 9
    sides, dev, bows = [], [], []
    for t in range(n_kf):
        got = fe.step([synth.image(c, 2 * t, 320, 240) for c in range(2)])
        feats = fe.fe.export_features()
        dev.append(bs.keyframe_from_device(v, feats, levelsup=2))
        b, _ = v.bow_vectors(got["desc"], 2)
        ob, (onid, onstart, oitems) = ov.bow_vectors(got["desc"], 2)
        assert b[0].tolist() == ob[0].tolist() and b[1].tobytes() == ob[1].tobytes()
        bows.append(b)
        sides.append(dict(desc=got["desc"], angle=got["kps"]["angle"], flags=(1 | ((got["uright"] >= 0) << 1)).astype(np.uint8), node_id=onid,
                          node_start=onstart, items=oitems))
    kfs = [km.KF(i + 1, bows[i], bows[i]) for i in range(n_kf)]
    for i, k in enumerate(kfs):
        k.cov = k.cov1 = [kfs[j] for j in (i - 1, i + 1, i - 2, i + 2) if 0 <= j < n_kf]
    lost = 4     # the frame to relocalise: the view of keyframe 4, which is not in the database
    ops = [("add_cam1", i, 0, 0.0) for i in range(n_kf) if i != lost] + [("reloc", lost, 5000, 0.0)]
    exp = class_against_model(tmp_path, nw, kfs, ops, "chain")
    cands = exp[0][0]
    assert len(cands) >= 1
    for c in cands:
        n, match = bs.search_by_bow_resident(dev[c - 1], dev[lost], 0, None, None, 50, 0.8, True)
        on, omatch = oracle.search_by_bow(sides[c - 1], sides[lost], 0, 50, 0.8, True)
        assert n == on and np.array_equal(match, omatch)
        assert n > 30
    fe.close()
