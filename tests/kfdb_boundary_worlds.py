"""Boundary worlds of the keyframe database's query kernel (k_db_query, multi_orb_slam_amd/csrc/kfdb.hip) and a plain restatement of
what it computes.

A world is a script over one database: ("add", key, bow), ("erase", key), ("query", [bows]) and ("refused", [bows]); a bow is
(ids uint32 strictly ascending, values float64).  play() runs a script against anything with add / erase / query / score / last_query --
ModelDB here, the device database in tests/test_gpu_kfdb_boundaries.py -- and returns a transcript that two backends must share byte for
byte: every query alone and all of an operation's queries in one call, keys, common counts, score bits, the score of every query
against every alive key, and the launch (form, entries per workgroup, workgroups, queries).

The model is a Python loop over IEEE doubles written from DBoW2's L1Scoring::score (ScoringObject.cpp:23-68) and the list walk of
KeyFrameDatabase::DetectRelocalizationCandidates (src/KeyFrameDatabase.cc:429-446): the intersection, fabs(v - w) - fabs(v) - fabs(w)
added one by one in ascending word id from 0.0, then -s / 2; a keyframe's place in the list is its smallest shared word, then its add
order.  It walks an entry 64 words at a time only so that the wrong rules -- each the slip one line of the kernel could make -- have a
place to stand; with rules=() the chunks change nothing.  tests/kfdb_model.py's inverted file stands beside it for the order
(inverted_file_order).

Groups: switch (LDS | global at 4096 | 4097 query words, the 65 535 cap), chunk (entry lengths around 64 and 128, the shared word's lane,
chunks that share nothing), search (where the binary search ends), grid (entries per workgroup, partly filled workgroups, query counts),
values (zeros, equal values, denormals, sums that tell the summation order), order (ties on the first shared word, erase and re-add)."""
import numpy as np
import kfdb_model as km

LDS_WORDS, MAX_WORDS, MAX_QUERIES, CHUNK = 4096, 65535, 1024, 64
FORM_LDS, FORM_GLOBAL = 1, 2
RULES = ("padding_lane_counted", "first_from_last_chunk", "tree_sum", "descending_sum", "plus_zero", "le_at_qn")
RULE_GROUP = {"padding_lane_counted": "search", "first_from_last_chunk": "chunk", "tree_sum": "values", "descending_sum": "values",
              "plus_zero": "values", "le_at_qn": "search"}


class Refused(Exception):
    pass


def epb_of(Q, E):
    """run_query's entries per workgroup"""
    return min(64, max(4, (Q * E) // 1024))


def launch_of(lengths, E):
    """(form, entries per workgroup, workgroups per query, queries) of the launch run_query makes"""
    epb = epb_of(len(lengths), E)
    return (FORM_LDS if max(lengths) <= LDS_WORDS else FORM_GLOBAL, epb, (E + epb - 1) // epb, len(lengths))


def _val(w, salt):
    h = (np.asarray(w, np.uint64) * np.uint64(2654435761) + np.uint64(salt * 40503)) % np.uint64(1000)
    return 1.0 / (3.0 + h.astype(np.float64))


def bow(ids, vals=None, salt=1):
    ids = np.ascontiguousarray(ids, np.uint32)
    assert len(ids) < 2 or (ids[1:] > ids[:-1]).all()
    vals = _val(ids, salt) if vals is None else np.ascontiguousarray(vals, np.float64)
    assert len(vals) == len(ids)
    return ids, vals


# ------------------------------------------------------------------------------------------------------------------- the model
def ascending_sum(terms):
    s = 0.0
    for t in terms:
        s += t
    return s


def descending_sum(terms):
    return ascending_sum(terms[::-1])


def tree_sum(terms):
    t = list(terms) or [0.0]
    while len(t) > 1:
        t = [t[i] + t[i + 1] if i + 1 < len(t) else t[i] for i in range(0, len(t), 2)]
    return t[0]


def shared_terms(q, e):
    """the terms of the words both vectors hold, ascending word id"""
    pos = {int(w): k for k, w in enumerate(q[0])}
    out = []
    for i, w in enumerate(e[0]):
        k = pos.get(int(w))
        if k is not None:
            v, x = float(q[1][k]), float(e[1][i])
            out.append(abs(v - x) - abs(v) - abs(x))
    return out


_POS = {}


def _positions(q):
    hit = _POS.get(id(q[0]))
    if hit is None or hit[0] is not q[0]:
        hit = (q[0], {int(w): k for k, w in enumerate(q[0])})
        _POS[id(q[0])] = hit
    return hit[1]


def pair(q, e, rules=(), after=None):
    """(common, first shared word, score) of query q against entry e.  `after`: the (id, value) that follows the query's words in the
    packed block of its call (the next query's first word), which only the rule "le_at_qn" ever looks at."""
    pos = _positions(q)
    qn, n = len(q[0]), len(e[0])
    top = int(q[0][-1]) if qn else -1
    common, first, terms = 0, 0, []
    for base in range(0, n, CHUNK):
        found = []                                        # (word, term) of the lanes that hold a shared word, ascending lane
        for lane in range(CHUNK):
            i = base + lane
            if i >= n:                                    # a lane behind the entry's end carries w = 0 and must find nothing
                if "padding_lane_counted" in rules and qn and int(q[0][0]) == 0:
                    v = float(q[1][0])
                    found.append((0, abs(v - 0.0) - abs(v) - 0.0))
                continue
            w = int(e[0][i])
            k = pos.get(w)
            if k is not None:
                v, x = float(q[1][k]), float(e[1][i])
            elif "le_at_qn" in rules and after is not None and w > top and after[0] == w:     # lo == qn, and ids[qn] is read
                v, x = float(after[1]), float(e[1][i])
            else:
                continue
            found.append((w, abs(v - x) - abs(v) - abs(x)))
        if not found:
            continue
        if common == 0 or "first_from_last_chunk" in rules:
            first = found[0][0]
        common += len(found)
        terms += [t for _, t in found]
    s = tree_sum(terms) if "tree_sum" in rules else descending_sum(terms) if "descending_sum" in rules else ascending_sum(terms)
    return common, first, (0.0 - s / 2.0) if "plus_zero" in rules else -s / 2.0


class ModelDB:
    """The database as a list in add order; query() as orbv_db_query returns it."""

    def __init__(self, n_words, rules=()):
        assert all(r in RULES for r in rules)
        self.n_words, self.rules, self.entries, self.launch, self.cache = n_words, tuple(rules), [], (0, 0, 0, 0), {}

    def add(self, key, b):
        assert all(k != key for k, _ in self.entries) and len(b[0]) <= MAX_WORDS and (len(b[0]) == 0 or int(b[0][-1]) < self.n_words)
        self.entries.append((key, b))

    def erase(self, key):
        self.entries = [(k, b) for k, b in self.entries if k != key]

    def __len__(self):
        return len(self.entries)

    def _pair(self, q, e, after):
        a = after if "le_at_qn" in self.rules else None
        ck = (id(q[0]), id(e[0]), None if a is None else a[0])
        if ck not in self.cache:
            self.cache[ck] = pair(q, e, self.rules, a)
        return self.cache[ck]

    def _check(self, bows):
        if len(bows) > MAX_QUERIES or any(len(b[0]) > MAX_WORDS for b in bows):
            raise Refused()

    def query(self, bows):
        self._check(bows)
        out, memo = [], {}
        for qi, q in enumerate(bows):
            after = None
            if "le_at_qn" in self.rules:
                nxt = next((b for b in bows[qi + 1:] if len(b[0])), None)
                after = None if nxt is None else (int(nxt[0][0]), float(nxt[1][0]))
            mk = (id(q[0]), after)
            if mk not in memo:                            # (a call may repeat one query a thousand times)
                rows = [(key,) + self._pair(q, b, after) for key, b in self.entries]
                hits = [r for r in rows if r[1] > 0]
                hits.sort(key=lambda r: r[2])             # stable: the add order among equal first words
                memo[mk] = (np.array([r[0] for r in hits], np.uint64), np.array([r[1] for r in hits], np.int32),
                            np.array([r[3] for r in hits], np.float64))
            out.append(memo[mk])
        if bows and self.entries:
            self.launch = launch_of([len(b[0]) for b in bows], len(self.entries))
        return out

    def score(self, q, keys):
        self._check([q])
        by = dict(self.entries)
        if len(keys):
            self.launch = launch_of([len(q[0])], len(keys))
        return np.array([self._pair(q, by[int(k)], None)[2] for k in keys], np.float64)

    def last_query(self):
        return self.launch


def inverted_file_order(entries, q):
    """keys and common counts as the reference's list walk meets them (tests/kfdb_model.py), for entries in add order"""
    db = km.ModelDatabase(0)
    for key, b in entries:
        db.add_cam1(km.KF(key, b))
    _, tr = db.detect_reloc(km.FrameOf(10 ** 9, km.KF(0, q)))
    return tr["met"], [tr["raw_common"][k] for k in tr["met"]]


def _distinct(bows):
    seen, out = set(), []
    for b in bows:
        if id(b[0]) not in seen:
            seen.add(id(b[0])); out.append(b)
    return out


def _pack(rows):
    return [(r[0].tolist(), r[1].tolist(), np.asarray(r[2], np.float64).tobytes()) for r in rows]


def play(world, db, refusal=Refused):
    """The transcript of a world on a database (see the module's docstring)."""
    out = []
    for op in world["ops"]:
        if op[0] == "add":
            db.add(op[1], op[2])
        elif op[0] == "erase":
            db.erase(op[1])
        elif op[0] == "refused":
            try:
                db.query(op[1])
                out.append(("refused", False))
            except refusal:
                out.append(("refused", True))
        elif op[0] == "query":
            rec = {"n": len(op[1]), "entries": len(db), "alone": [], "alone_launch": [], "scores": []}
            keys = [k for k in world["keys_after"][len(out)]]
            for q in _distinct(op[1]):
                rec["alone"] += _pack(db.query([q])); rec["alone_launch"].append(db.last_query())
                rec["scores"].append(np.asarray(db.score(q, keys), np.float64).tobytes()); rec["alone_launch"].append(db.last_query())
            rec["batch"] = _pack(db.query(op[1])); rec["batch_launch"] = db.last_query()
            out.append(("query", rec))
        else:
            raise ValueError(op[0])
    return out


def differences(a, b):
    """where two transcripts part: [(operation, what)]"""
    out = []
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        if x[0] == "refused":
            if x != y:
                out.append((k, "refused"))
            continue
        for what in ("alone", "batch", "scores", "alone_launch", "batch_launch"):
            if x[1][what] != y[1][what]:
                out.append((k, what))
    return out


# ------------------------------------------------------------------------------------------------------------------ the worlds
def _finish(name, group, n_words, ops, **more):
    """records the alive keys at every transcript position (play scores every query against all of them)"""
    alive, after = [], []
    for op in ops:
        if op[0] == "add":
            alive.append(op[1])
        elif op[0] == "erase":
            alive = [k for k in alive if k != op[1]]
        else:
            after.append(list(alive))
    return dict(name=name, group=group, n_words=n_words, ops=ops, keys_after=after, **more)


def _odd(n, start=1):
    return start + 2 * np.arange(n, dtype=np.int64)


def entry_with(length, shared, salt):
    """An entry of `length` words: odd filler ids (no query of these worlds holds an odd id below 4000) with the even words shared[p] put at
    position p, ascending throughout."""
    ids, nxt = [], 1
    for p in range(length):
        if p in shared:
            assert shared[p] >= nxt and shared[p] % 2 == 0
            ids.append(shared[p]); nxt = shared[p] + 1
        else:
            ids.append(nxt); nxt += 2
    return bow(ids, salt=salt)


def switch_world():
    n_words = 70000
    ents = [bow(np.arange(0, 70000, 7), salt=2), bow(np.arange(5, 69000, 345), salt=3), bow([0], salt=4), bow([69999], salt=5),
            bow(np.arange(4090 * 16, 4100 * 16, 8), salt=6), bow([], salt=7), bow(np.arange(3, 65538), salt=8)]
    q = {n: bow(np.arange(n, dtype=np.int64) * 16 + 3, salt=10 + n % 7) for n in (4095, 4096, 4097)}
    q[65535] = bow(np.arange(65535) + 3, salt=9)
    q[65536] = bow(np.arange(65536) + 3, salt=9)
    ops = [("add", 100 + i, e) for i, e in enumerate(ents)]
    ops += [("query", [q[4095], q[4096]]), ("query", [q[4096], q[4097]]), ("query", [q[4097], q[4095], q[4096]]), ("query", [q[65535]]),
            ("refused", [q[65536]]), ("refused", [q[4095], q[65536]]), ("query", [q[4095]])]
    return _finish("switch", "switch", n_words, ops, lengths=(4095, 4096, 4097, 65535))


CHUNK_LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129)


def chunk_world():
    """query: the even ids 1000, 1010, ...; every entry shares exactly the words put into it, at the positions named"""
    n_words = 10000
    q = bow(np.arange(1000, 3000, 10), salt=1)
    ents, names, word = [], [], iter(range(2990, 1000, -10))      # later entries share SMALLER words: list order != add order
    for L in CHUNK_LENGTHS:
        ents.append(entry_with(L, {}, 20 + L)); names.append("len%d_none" % L)
        for p in sorted({0, 63, 64, L - 1, 127, 128}):
            if 0 <= p < L:
                ents.append(entry_with(L, {p: next(word)}, 30 + L + p)); names.append("len%d_only_at_%d" % (L, p))
    # two shared words, chunks that share nothing before, between and behind them
    ents.append(entry_with(200, {5: 1000, 130: 1500}, 50)); names.append("chunks_0_and_2")
    ents.append(entry_with(129, {64: 1100}, 51)); names.append("behind_one_empty_chunk")
    ents.append(entry_with(193, {128: 1050, 192: 1300}, 52)); names.append("behind_two_empty_chunks")
    ents.append(entry_with(65, {3: 1020}, 53)); names.append("after_it")
    ops = [("add", 1 + i, e) for i, e in enumerate(ents)] + [("query", [q])]
    return _finish("chunk", "chunk", n_words, ops, names=names, entries=ents, q=q)


def search_world():
    n_words = 5000
    q1 = bow(list(range(0, 1000, 10)) + [4999], salt=1)               # word 0 at position 0, word n_words - 1 at position qn - 1
    q2 = bow(np.arange(2000, 3001, 10), salt=2)
    q3 = bow([3001, 3005], salt=3)                                    # follows q2 in the packed block: its first id is an entry's word
    ents = dict(
        zero_len1=bow([0], salt=4), zero_len65=bow([0] + list(_odd(64)), salt=5),
        pad_len1_no_zero=bow([7], salt=6), pad_len65_no_zero=bow(list(_odd(65)), salt=7),
        last_len1=bow([4999], salt=8), last_len65=bow(list(_odd(64, 4001)) + [4999], salt=9),
        below_q2=bow(_odd(100), salt=10), above_q2=bow(_odd(70, 3001), salt=11),
        ends_q2=bow([1999, 2000, 2001, 2999, 3000, 3001], salt=12), first_q2=bow([2000], salt=13), lastw_q2=bow([3000, 4000], salt=14),
        between=bow(np.arange(2005, 3000, 10), salt=15))
    ops = [("add", 1 + i, e) for i, e in enumerate(ents.values())] + [("query", [q1]), ("query", [q2, q3]), ("query", [q1, q2])]
    return _finish("search", "search", n_words, ops, names=list(ents), entries=list(ents.values()), q=(q1, q2, q3))


T53 = 2.0 ** -53


def values_world():
    n_words = 1000
    ids = np.arange(10, 14)
    q_order = bow(ids, [4.0, 4.0, 4.0, 4.0])
    e_order = bow(ids, [0.5, T53, T53, T53])                      # terms -1, -2^-53 three times: three orders, three sums
    wide = np.arange(100, 160)
    q_wide, e_wide = bow(wide, salt=22), bow(wide, salt=25)
    zq = bow([200, 201, 202, 203], [0.0, 0.25, 0.0, 0.5])
    ents = dict(order=e_order, wide=e_wide,
                zero_entry=bow([201], [0.0]), zero_query=bow([200], [0.75]), zero_both=bow([202], [0.0]), zero_all=bow([200, 201, 202], [0.5, 0.0, 0.0]),
                zero_and_one=bow([200, 203], [0.125, 0.5]),
                equal=bow([201, 203], [0.25, 0.5]),
                denormal=bow([300, 301, 302, 303], [5e-324, 1e-310, 2.2250738585072014e-308, 3e-308]))
    q_den = bow([300, 301, 302, 303], [1e-310, 5e-324, 2.2250738585072009e-308, 2.2250738585072014e-308])
    ops = [("add", 1 + i, e) for i, e in enumerate(ents.values())] + [("query", [q_order]), ("query", [q_wide]), ("query", [zq]), ("query", [q_den]),
                                                                       ("query", [q_order, q_wide, zq, q_den])]
    return _finish("values", "values", n_words, ops, names=list(ents), pairs=dict(order=(q_order, e_order), wide=(q_wide, e_wide)), zq=zq,
                   entries=ents)


def order_world():
    n_words = 100
    q = bow([5, 10, 20, 30, 40, 50], salt=1)
    ents = [(5, bow([10, 20], salt=2)), (3, bow([10, 60], salt=3)), (9, bow([10, 30, 40], salt=4)), (1, bow([9, 10, 11], salt=5)),
            (7, bow([5, 99], salt=6)), (8, bow([50], salt=7)), (2, bow([20, 50], salt=8)), (6, bow([20, 21], salt=9)), (4, bow([61, 62], salt=10))]
    ops = [("add", k, b) for k, b in ents] + [("query", [q])]
    ops += [("erase", 3), ("query", [q]), ("add", 3, ents[1][1]), ("query", [q])]                   # key 3 now comes last among the ties on word 10
    ops += [("erase", 5), ("erase", 9), ("erase", 1), ("erase", 7), ("erase", 2), ("query", [q])]  # more than half of the arena dead: a compaction
    ops += [("add", 9, ents[2][1]), ("add", 5, ents[0][1]), ("query", [q])]
    return _finish("order", "order", n_words, ops)


GRID_E = tuple(range(1, 67))


def grid_world():
    """The database grows one entry at a time; at every size 1024 and 1023 queries go out in one call each (Q x E either side of every
    multiple of 1024 at which entries-per-workgroup changes: 1024 E against 1023 E), and 1, 2, 3 and 5 queries."""
    n_words = 2000
    distinct = [bow(sorted({(3 * j + i) % 11 for i in range(4)} | {100 + j}), salt=40 + j) for j in range(8)]
    ops = []
    for E in GRID_E:
        ops.append(("add", 1000 + E, bow([E % 11, 100 + E % 8, 200 + E], salt=60 + E)))
        for Q in (1024, 1023) + ((1, 2, 3, 5) if E in (1, 2, 3, 4, 5, 6, 9, 64, 65, 66) else ()):
            ops.append(("query", [distinct[i % 8] for i in range(Q)]))
    ops.append(("refused", [distinct[i % 8] for i in range(1025)]))
    ops.append(("query", [distinct[0], distinct[1]]))
    return _finish("grid", "grid", n_words, ops)


def worlds():
    return [switch_world(), chunk_world(), search_world(), values_world(), order_world(), grid_world()]


N_WORLDS = 6
GROUPS = ("switch", "chunk", "search", "grid", "values", "order")


# -------------------------------------------------------------------------------------------------------------- the conditions
def check_conditions(w):
    """What each group promises, asserted on the model alone.  -> number of conditions checked"""
    n = 0
    g = w["group"]
    queries = [op[1] for op in w["ops"] if op[0] == "query"]
    if g == "switch":
        lens = {len(b[0]) for qs in queries for b in qs}
        assert lens == {4095, 4096, 4097, 65535} and LDS_WORDS == 4096 and MAX_WORDS == 65535
        forms = [launch_of([len(b[0]) for b in qs], 7)[0] for qs in queries]
        assert forms == [FORM_LDS, FORM_GLOBAL, FORM_GLOBAL, FORM_GLOBAL, FORM_LDS]
        assert [sorted(len(b[0]) for b in qs) for qs in queries[:2]] == [[4095, 4096], [4096, 4097]]      # the longest decides for all
        refused = [op[1] for op in w["ops"] if op[0] == "refused"]
        assert [max(len(b[0]) for b in qs) for qs in refused] == [65536, 65536]
        for qs in queries:                                                                                # every query meets entries
            for q in qs:
                assert sum(pair(q, op[2])[0] > 0 for op in w["ops"] if op[0] == "add") >= 3
        n += 5
    elif g == "chunk":
        lens = sorted({len(e[0]) for e in w["entries"]})
        assert set(CHUNK_LENGTHS) <= set(lens)
        by = dict(zip(w["names"], w["entries"]))
        for name, e in by.items():
            c, first, _ = pair(w["q"], e)
            if name.endswith("_none"):
                assert c == 0
            elif "_only_at_" in name:
                p = int(name.rsplit("_", 1)[1])
                assert c == 1 and int(e[0][p]) == first and first % 10 == 0; n += 1
        lanes = {(int(nm.split("_")[0][3:]), int(nm.rsplit("_", 1)[1])) for nm in by if "_only_at_" in nm}
        assert {(64, 0), (64, 63), (65, 64), (65, 0), (127, 126), (129, 128), (129, 64), (128, 127), (1, 0), (63, 62)} <= lanes
        assert pair(w["q"], by["chunks_0_and_2"])[:2] == (2, 1000) and pair(w["q"], by["chunks_0_and_2"], ("first_from_last_chunk",))[1] == 1500
        assert pair(w["q"], by["behind_one_empty_chunk"])[:2] == (1, 1100) and pair(w["q"], by["behind_two_empty_chunks"])[:2] == (2, 1050)
        n += 3
    elif g == "search":
        q1, q2, q3 = w["q"]
        by = dict(zip(w["names"], w["entries"]))
        assert int(q1[0][0]) == 0 and int(q1[0][-1]) == w["n_words"] - 1
        assert pair(q1, by["zero_len1"])[:2] == (1, 0) and pair(q1, by["zero_len65"])[:2] == (1, 0) and len(by["zero_len65"][0]) == 65
        assert pair(q1, by["pad_len1_no_zero"])[0] == 0 and pair(q1, by["pad_len1_no_zero"], ("padding_lane_counted",))[0] == 63
        assert pair(q1, by["last_len1"])[:2] == (1, 4999) and pair(q1, by["last_len65"])[:2] == (1, 4999)
        assert int(by["below_q2"][0][-1]) < int(q2[0][0]) and int(by["above_q2"][0][0]) > int(q2[0][-1])
        assert pair(q2, by["below_q2"])[0] == pair(q2, by["above_q2"])[0] == 0
        assert pair(q2, by["above_q2"], ("le_at_qn",), (int(q3[0][0]), float(q3[1][0])))[0] == 1
        assert pair(q2, by["ends_q2"])[:2] == (2, 2000) and pair(q2, by["first_q2"])[0] == 1 and pair(q2, by["lastw_q2"])[:2] == (1, 3000)
        assert pair(q2, by["between"])[0] == 0
        n += 8
    elif g == "values":
        for name, (q, e) in w["pairs"].items():
            t = shared_terms(q, e)
            sums = {np.float64(f(t)).tobytes() for f in (ascending_sum, descending_sum, tree_sum)}
            assert len(sums) == 3, name      # the inputs can tell "one by one in ascending word id" from the other two orders
            n += 1
        assert shared_terms(*w["pairs"]["order"]) == [-1.0, -T53, -T53, -T53]
        E = w["entries"]; zq = w["zq"]
        for name in ("zero_entry", "zero_query", "zero_both", "zero_all"):
            c, _, s = pair(zq, E[name])
            assert c >= 1 and s == 0.0 and np.signbit(s), name      # -0.0: a term of 0 and the sign of -s / 2
            assert not np.signbit(pair(zq, E[name], ("plus_zero",))[2])
            n += 1
        assert pair(zq, E["zero_and_one"])[2] == 0.5 and pair(zq, E["equal"])[2] == 0.75
    elif g == "order":
        t = play(w, ModelDB(w["n_words"]))
        firsts = [t[k][1]["batch"][0][0] for k in range(5)]
        assert firsts[0][:5] == [7, 5, 3, 9, 1] and firsts[1][:4] == [7, 5, 9, 1] and firsts[2][:5] == [7, 5, 9, 1, 3]
        assert firsts[3] == [3, 6, 8] and firsts[4] == [3, 9, 5, 6, 8]
        n += 5
    elif g == "grid":
        seen, partial = set(), 0
        E = 0
        for op in w["ops"]:
            if op[0] == "add":
                E += 1
            elif op[0] == "query":
                Q = len(op[1])
                epb = epb_of(Q, E)
                seen.add((Q, E, epb))
                partial += E % epb == 1 and E > epb
        for k in range(5, 65):               # either side of every value of Q x E at which epb changes
            assert (1024, k, k) in seen and (1023, k, k - 1 if k > 5 else 4) in seen
        assert (1024, 4, 4) in seen and (1024, 3, 4) in seen and (1024, 65, 64) in seen and (1023, 65, 64) in seen and (1023, 64, 63) in seen
        assert {(q, e) for q, e, _ in seen} >= {(q, e) for q in (1, 2, 1024) for e in (1, 2, 3, 5)} and partial >= 60
        assert [len(op[1]) for op in w["ops"] if op[0] == "refused"] == [1025]
        n += 4
    assert n > 0
    return n
