"""The checker of the keyframe database: a line-by-line Python restatement of the reference's KeyFrameDatabase (src/KeyFrameDatabase.cc)
with real inverted lists and the per-keyframe scratch fields, and a seeded world generator for its tests.

Written from the reference's behaviour, cited by line; the score is oracle.bow_score_l1 (double), every float step is numpy.float32:
    add / add_cam1   :41-57     one push_back per word of the BowVector
    erase            :63-97     first occurrence out of every list of both files; relative order kept
    clear            :99-105
    DetectLoopCandidates[_cam1]      :119-255 / :269-402
    DetectRelocalizationCandidates   :415-543
A detect call returns (ids, trace); the trace holds every intermediate list, so a test can compare stage by stage."""
import struct
import numpy as np
import oracle
from multi_orb_slam_amd import synth

F32 = np.float32


class KF:
    """The members of KeyFrame / Frame the database reads or writes."""

    def __init__(self, mnId, bow, bow1=None, cov=(), cov1=(), conn=(), conn1=()):
        self.mnId = int(mnId)
        self.bow = (np.ascontiguousarray(bow[0], np.uint32), np.ascontiguousarray(bow[1], np.float64))
        b1 = bow if bow1 is None else bow1
        self.bow1 = (np.ascontiguousarray(b1[0], np.uint32), np.ascontiguousarray(b1[1], np.float64))
        self.cov, self.cov1 = list(cov), list(cov1)        # KF objects, best covisibility first
        self.conn, self.conn1 = list(conn), list(conn1)    # KF objects (a set in the reference)
        # src/KeyFrame.cc:35: mnLoopQuery(0), mnLoopWords(0), mnRelocQuery(0), mnRelocWords(0); the two scores are not initialised
        # there -- canonical choice of this project: 0
        self.mnLoopQuery = 0; self.mnLoopWords = 0; self.mLoopScore = F32(0)
        self.mnRelocQuery = 0; self.mnRelocWords = 0; self.mRelocScore = F32(0)

    def fields(self):
        return (self.mnLoopQuery, self.mnLoopWords, float(self.mLoopScore), self.mnRelocQuery, self.mnRelocWords, float(self.mRelocScore))


def score(a, b):
    return oracle.bow_score_l1(a, b)


class ModelDatabase:
    def __init__(self, n_words):
        self.n_words = n_words
        self.clear()

    def add(self, kf):                                   # :41-48
        for w in kf.bow[0]:
            self.inv.setdefault(int(w), []).append(kf)

    def add_cam1(self, kf):                              # :51-57
        for w in kf.bow1[0]:
            self.inv1.setdefault(int(w), []).append(kf)

    def erase(self, kf):                                 # :63-97
        for inv, bow in ((self.inv, kf.bow), (self.inv1, kf.bow1)):
            for w in bow[0]:
                l = inv.get(int(w), [])
                for i, x in enumerate(l):
                    if x is kf:
                        del l[i]
                        break

    def clear(self):                                     # :99-105
        self.inv, self.inv1 = {}, {}

    # ------------------------------------------------------------------------------------------------------------------
    def detect_loop(self, q, min_score, cam1=False):     # :119-255, :269-402
        min_score = F32(min_score)
        inv = self.inv1 if cam1 else self.inv
        qbow = q.bow1 if cam1 else q.bow
        bow_of = (lambda k: k.bow1) if cam1 else (lambda k: k.bow)
        cov_of = (lambda k: k.cov1) if cam1 else (lambda k: k.cov)
        connected = set(id(k) for k in (q.conn1 if cam1 else q.conn))
        tr = dict(met=[], raw_common={}, first_word={}, sharing=[], common={}, min_common=None, scored={}, matches=[], groups=[])
        sharing = []
        for w in qbow[0]:                                # :132-154
            for k in inv.get(int(w), []):
                if k.mnId not in tr["raw_common"]:
                    tr["met"].append(k.mnId); tr["raw_common"][k.mnId] = 0; tr["first_word"][k.mnId] = int(w)
                tr["raw_common"][k.mnId] += 1
                if k.mnLoopQuery != q.mnId:
                    k.mnLoopWords = 0
                    if id(k) not in connected:
                        k.mnLoopQuery = q.mnId
                        sharing.append(k)
                k.mnLoopWords += 1
        tr["sharing"] = [k.mnId for k in sharing]
        if not sharing:                                  # :157
            return [], tr
        max_common = 0                                   # :164-169
        for k in sharing:
            if k.mnLoopWords > max_common:
                max_common = k.mnLoopWords
        min_common = int(F32(max_common) * F32(0.8))     # :171  int = int * float
        tr["min_common"] = min_common
        tr["common"] = {k.mnId: k.mnLoopWords for k in sharing}
        matches = []
        for k in sharing:                                # :177-193
            if k.mnLoopWords > min_common:
                d = score(qbow, bow_of(k))
                tr["scored"][k.mnId] = d
                si = F32(d)
                k.mLoopScore = si
                if si >= min_score:
                    matches.append((si, k))
        tr["matches"] = [(float(s), k.mnId) for s, k in matches]
        if not matches:                                  # :195
            return [], tr
        acc_and_match = []
        best_acc = min_score                             # :199
        for s, k in matches:                             # :205-230
            best, acc, best_kf = s, s, k
            for k2 in cov_of(k)[:10]:
                if k2.mnLoopQuery == q.mnId and k2.mnLoopWords > min_common:
                    acc = F32(acc + k2.mLoopScore)
                    if k2.mLoopScore > best:
                        best_kf = k2
                        best = k2.mLoopScore
            acc_and_match.append((acc, best_kf))
            tr["groups"].append((float(acc), best_kf.mnId, k.mnId))
            if acc > best_acc:
                best_acc = acc
        retain = F32(F32(0.75) * best_acc)               # :233
        out, seen = [], set()
        for acc, k in acc_and_match:                     # :240-251
            if acc > retain and id(k) not in seen:
                out.append(k.mnId); seen.add(id(k))
        return out, tr

    def detect_reloc(self, f):                           # :415-543 (f: anything with mnId and bow1)
        tr = dict(met=[], raw_common={}, first_word={}, sharing=[], common={}, min_common=None, scored={}, matches=[], groups=[])
        sharing = []
        for w in f.bow1[0]:                              # :429-447
            for k in self.inv1.get(int(w), []):
                if k.mnId not in tr["raw_common"]:
                    tr["met"].append(k.mnId); tr["raw_common"][k.mnId] = 0; tr["first_word"][k.mnId] = int(w)
                tr["raw_common"][k.mnId] += 1
                if k.mnRelocQuery != f.mnId:
                    k.mnRelocWords = 0
                    k.mnRelocQuery = f.mnId
                    sharing.append(k)
                k.mnRelocWords += 1
        tr["sharing"] = [k.mnId for k in sharing]
        if not sharing:
            return [], tr
        max_common = 0
        for k in sharing:
            if k.mnRelocWords > max_common:
                max_common = k.mnRelocWords
        min_common = int(F32(max_common) * F32(0.8))     # :461
        tr["min_common"] = min_common
        tr["common"] = {k.mnId: k.mnRelocWords for k in sharing}
        matches = []
        for k in sharing:                                # :469-481
            if k.mnRelocWords > min_common:
                d = score(f.bow1, k.bow1)
                tr["scored"][k.mnId] = d
                si = F32(d)
                k.mRelocScore = si
                matches.append((si, k))
        tr["matches"] = [(float(s), k.mnId) for s, k in matches]
        if not matches:
            return [], tr
        acc_and_match = []
        best_acc = F32(0)                                # :487
        for s, k in matches:                             # :493-519
            best, acc, best_kf = s, s, k
            for k2 in k.cov1[:10]:
                if k2.mnRelocQuery != f.mnId:
                    continue
                acc = F32(acc + k2.mRelocScore)
                if k2.mRelocScore > best:
                    best_kf = k2
                    best = k2.mRelocScore
            acc_and_match.append((acc, best_kf))
            tr["groups"].append((float(acc), best_kf.mnId, k.mnId))
            if acc > best_acc:
                best_acc = acc
        retain = F32(F32(0.75) * best_acc)               # :523
        out, seen = [], set()
        for acc, k in acc_and_match:
            if acc > retain and id(k) not in seen:
                out.append(k.mnId); seen.add(id(k))
        return out, tr


# ------------------------------------------------------------------------------------------------------------------ worlds
def _h(seed, a, n):
    return synth.hash32(np.arange(n, dtype=np.uint64) + np.uint64(((seed * 0x9E3779B1) ^ (a * 0x85EBCA6B)) & 0xFFFFFFFF))


def bow_from(ids, weights):
    """Sorted unique ids with L1-normalised positive values (what BowVector::normalize leaves)."""
    ids = np.asarray(ids, np.uint32)
    order = np.argsort(ids, kind="stable")
    ids, weights = ids[order], np.asarray(weights, np.float64)[order]
    keep = np.concatenate([[True], ids[1:] != ids[:-1]]) if len(ids) else np.zeros(0, bool)
    ids, weights = ids[keep], weights[keep]
    return ids, weights / weights.sum() if len(ids) else weights


class World:
    """K keyframes along a trajectory through places that own overlapping windows of a word permutation; the second half of the
    trajectory is a second lap over the same places.  Covisibility = nearest in time (ordered), connected = within `reach` in time."""

    def __init__(self, K, seed=1, words=(300, 1200), stride=100, window=2000, reach=6):
        lap = max(K // 2, 1)
        self.n_words = lap * stride + window
        perm = np.argsort(_h(seed, 1, self.n_words), kind="stable").astype(np.uint32)
        span = words[1] - words[0]
        sal = _h(seed, 3, self.n_words) % np.uint32(window)       # every word's salience: low values are seen by whoever passes
        jit = _h(seed, 2, K) % np.uint32(41)
        self.kfs = []
        for t in range(K):
            place = t % lap
            # the number of words drifts along the trajectory (texture-rich and texture-poor stretches), with a little jitter
            nw = int(words[0] + span * (0.5 + 0.5 * np.sin(place / 9.0))) + int(jit[t]) - 20
            h = _h(seed, 1000 + t, window)
            own = sal[place * stride:place * stride + window] < np.uint32(int(0.8 * nw))     # what the place shows
            noise = h % np.uint32(window) < np.uint32(int(0.25 * nw))                        # what only this view picked up
            pick = np.flatnonzero(own | noise)
            ids = perm[place * stride + pick]
            wts = 1.0 + (_h(seed, 500000 + t, window)[pick] % np.uint32(1000)).astype(np.float64)
            bow = bow_from(ids, wts)
            c1 = (_h(seed, 900000 + t, window)[pick] & np.uint32(3)) != 0     # camera 1 sees three quarters of the words
            bow1 = bow_from(ids[c1], wts[c1])
            self.kfs.append(KF(t, bow, bow1))
        for t, k in enumerate(self.kfs):
            near = [t + d * s for d in range(1, 9) for s in (-1, 1)]
            k.cov = [self.kfs[i] for i in near if 0 <= i < K][:12]
            k.cov1 = [self.kfs[i] for i in near[::-1] if 0 <= i < K][:12][::-1] if t % 3 else k.cov[:7]
            k.conn = [self.kfs[i] for i in range(max(0, t - reach), min(K, t + reach + 1)) if i != t]
            k.conn1 = k.conn[:max(1, len(k.conn) - 2)]
        self.K = K

    def script(self, n_detect=6):
        """Operations (name, keyframe index, frame id, minScore): the first lap and most of the second are added, a few keyframes are
        erased and some re-added (so add order != id order), then keyframes of the second lap ask for loop / relocalisation candidates."""
        K = self.K
        lap = K // 2
        asking = [lap + (j * 37 + 11) % max(lap - 10, 1) for j in range(n_detect)]
        out = set(a + d for a in asking for d in (0, 5, 9)) | {lap + 3}     # who asks is not in the database yet (LoopClosing.cc:140-173)
        ops = [(name, t, 0, 0.0) for t in range(K) if t not in out for name in ("add", "add_cam1")]
        victims = [t for t in range(3, K, max(K // 12, 5)) if t not in out]
        ops += [("erase", t, 0, 0.0) for t in victims]
        ops += [(name, t, 0, 0.0) for t in victims[::2] for name in ("add", "add_cam1")]
        frame_id = 1000000
        for j, t in enumerate(asking):
            ops.append(("loop", t, 0, 0.004))
            ops.append(("loop_cam1", (t + 5) % K, 0, 0.004))
            ops.append(("reloc", (t + 9) % K, frame_id + j, 0.0))
        ops.append(("loop", lap + 3, 0, 0.9))     # nothing scores that high: lScoreAndMatch stays empty
        return ops


class FrameOf:
    """A Frame for relocalisation: an id of its own and the camera-1 BowVector of a keyframe."""

    def __init__(self, mnId, kf):
        self.mnId = int(mnId); self.bow1 = kf.bow1


def run_script(n_words, kfs, ops):
    """-> per detect call (name, returned ids, trace, fields of every keyframe after the call)."""
    db = ModelDatabase(n_words)
    out = []
    for name, t, fid, ms in ops:
        k = kfs[t]
        if name == "add": db.add(k)
        elif name == "add_cam1": db.add_cam1(k)
        elif name == "erase": db.erase(k)
        elif name == "clear": db.clear()
        elif name in ("loop", "loop_cam1"):
            ids, tr = db.detect_loop(k, ms, cam1=(name == "loop_cam1"))
            out.append((name, ids, tr, [x.fields() for x in kfs]))
        elif name == "reloc":
            ids, tr = db.detect_reloc(FrameOf(fid, k))
            out.append((name, ids, tr, [x.fields() for x in kfs]))
        else:
            raise ValueError(name)
    return out


# ----------------------------------------------------------------------------------------------------- hand-built cases
def B(ids, vals=None):
    """A small hand-made BowVector: the given ids, equal values that sum to 1 unless values are given."""
    ids = np.asarray(sorted(ids), np.uint32)
    vals = np.full(len(ids), 1.0 / max(len(ids), 1)) if vals is None else np.asarray(vals, np.float64)
    return ids, vals


def quirk_cases():
    """name -> (n_words, keyframes, operations): the scratch-field quirks of the reference, as scripts the C++ class and the host
    restatement run too."""
    cases = {}
    # 1. the same keyframe asks twice: the second walk finds every keyframe marked -> counted on top, none listed
    kfs = [KF(1, B(range(0, 6))), KF(2, B(range(2, 11))), KF(3, B(list(range(5, 10)) + [50])), KF(9, B(range(10)))]
    kfs[0].cov = [kfs[1]]; kfs[1].cov = [kfs[0], kfs[2]]
    for k in kfs:
        k.cov1 = k.cov
    ops = [(n, t, 0, 0.0) for t in range(3) for n in ("add", "add_cam1")] + [("loop", 3, 0, 0.0), ("loop", 3, 0, 0.0), ("loop_cam1", 3, 0, 0.0)]
    cases["twice"] = (100, kfs, ops)
    # 2. keyframe 0 asks: fresh keyframes carry mnLoopQuery 0 already (src/KeyFrame.cc:35) -> none listed; one that an earlier query (7) marked
    #    is listed, and its unmarked-by-this-walk neighbours contribute to its group with whatever they hold
    kfs = [KF(0, B(range(10))), KF(1, B(range(0, 8))), KF(2, B(range(1, 10))), KF(3, B(range(1, 8))), KF(7, B(range(3, 10)))]
    kfs[1].cov = [kfs[2], kfs[3]]; kfs[2].cov = [kfs[1]]; kfs[3].cov = [kfs[2], kfs[1]]
    for k in kfs:
        k.cov1 = k.cov
    ops = [(n, t, 0, 0.0) for t in (1, 2, 3) for n in ("add", "add_cam1")]
    ops += [("loop", 0, 0, 0.0),            # nothing listed
            ("loop", 4, 0, 0.0),            # keyframe 7 marks 1, 2, 3 and scores them
            ("erase", 2, 0, 0.0), ("add", 2, 0, 0.0), ("add_cam1", 2, 0, 0.0),
            ("loop", 0, 0, 0.0),            # all three are listed now (marked 7); their scores are rewritten
            ("reloc", 0, 0, 0.0)]           # a frame with mnId 0 meets mnRelocQuery 0 everywhere: none listed
    cases["zero"] = (100, kfs, ops)
    # 3. connected keyframes: counted to 1, not marked; they still take part in groups if an earlier query with the same id marked them -- here
    #    they do not, and the group of keyframe 3 has no contributing neighbour
    kfs = [KF(1, B(range(0, 7))), KF(2, B(range(1, 9))), KF(3, B(range(2, 10))), KF(9, B(range(10)))]
    kfs[3].conn = [kfs[0], kfs[1]]
    kfs[2].cov = [kfs[0], kfs[1]]
    ops = [(n, t, 0, 0.0) for t in range(3) for n in ("add", "add_cam1")] + [("loop", 3, 0, 0.0), ("loop_cam1", 3, 0, 0.0)]
    cases["connected"] = (100, kfs, ops)
    # 4. relocalisation adds a marked neighbour's STALE score: frame 5 scores keyframe 2 high; frame 6 lists keyframe 2 below the threshold
    #    (not scored now) and scores keyframe 1, whose best covisible keyframe is 2 -> the group's best is 2 with the score of frame 5
    kfs = [KF(1, B(list(range(0, 8)) + list(range(40, 46)))), KF(2, B(list(range(6, 9)) + list(range(20, 30)))),
           KF(50, B(range(20, 30))), KF(51, B(range(0, 10)))]
    kfs[0].cov1 = [kfs[1]]
    ops = [("add_cam1", 0, 0, 0.0), ("add_cam1", 1, 0, 0.0), ("reloc", 2, 5, 0.0), ("reloc", 3, 6, 0.0), ("reloc", 3, 6, 0.0)]
    cases["stale"] = (100, kfs, ops)
    return cases


# ------------------------------------------------------------------------------------------------ files of the C++ driver
OPS = ("add", "add_cam1", "erase", "clear", "loop", "loop_cam1", "reloc")
MAGIC = 0x4B464442


def write_world(path, n_words, kfs, ops):
    """WORLD.bin of host/test_kfdb.cc (little endian): header, keyframes, operations."""
    index = {id(k): i for i, k in enumerate(kfs)}
    with open(path, "wb") as f:
        f.write(struct.pack("<iiii", MAGIC, n_words, len(kfs), len(ops)))
        for k in kfs:
            lists = [np.array([index[id(x)] for x in l], np.int32) for l in (k.cov, k.cov1, k.conn, k.conn1)]
            f.write(struct.pack("<Qiiiiii", k.mnId, len(k.bow[0]), len(k.bow1[0]), *[len(l) for l in lists]))
            f.write(k.bow[0].tobytes()); f.write(k.bow[1].tobytes()); f.write(k.bow1[0].tobytes()); f.write(k.bow1[1].tobytes())
            for l in lists:
                f.write(l.tobytes())
        for name, t, fid, ms in ops:
            f.write(struct.pack("<iiQf", OPS.index(name), t, fid, ms))


def read_out(path, n_kf):
    """OUT.bin -> per detect call (returned ids, fields of every keyframe)."""
    blob = open(path, "rb").read()
    pos, out = 0, []
    rec = struct.Struct("<QifQif")
    while pos < len(blob):
        n, = struct.unpack_from("<i", blob, pos); pos += 4
        ids = list(struct.unpack_from("<%dQ" % n, blob, pos)); pos += 8 * n
        fields = [rec.unpack_from(blob, pos + i * rec.size) for i in range(n_kf)]; pos += rec.size * n_kf
        out.append((ids, fields))
    return out


def expected_out(results):
    """What read_out returns for a run that agrees with the model (floats through float32, as the file stores them)."""
    return [(ids, [(a, b, float(F32(c)), d, e, float(F32(g))) for a, b, c, d, e, g in fields]) for _, ids, _, fields in results]
