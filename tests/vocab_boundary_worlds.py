"""Boundary worlds of the vocabulary descent and the device-built FeatureVector (k_bow_transform, k_fv_count, k_fv_offsets, k_fv_fill:
multi_orb_slam_amd/csrc/bow.hip) and a plain restatement of what they compute.

A world is a (tree, features, levelsup) triple with a group name.  Trees are hand-built parent / is_leaf / desc / weight arrays over node
ids as synth.vocabulary returns them (fan-out is free: orbv_create puts no cap on k); features sit an exact number of flipped bits from
chosen children.  Groups:
    tie     equal distances (two, three, all children; different lanes, one lane across passes: children c, c + 16, c + 32; first against
            last child), distance 0, distance 256 as the best, the only and a tied distance
    fanout  k = 1, 2, 15, 16, 17, 20, 32, 33
    depth   L = 1 .. 6, levelsup 0, 1, L - 1, L, L + 2; ragged trees whose leaves lie above, at and below the FeatureVector's level
    ids     node ids not grouped by parent and not breadth-first (shuffled, reversed): rank by NodeId differs from position
    stop    words of weight 0 and below, all stopped, one kept, a stopped word in the only non-root bin
    bins    1, 2, 1024, 1025, 1026, 2048, 2049, 4096, 4097 bins (nodes at the FeatureVector's level plus the root's) and 4098, refused
    fill    which bins are occupied (none, the root's only, the last only, the first and last of each chunk of 1024, every, every other,
            one bin with everything), feature counts around 16, 64 and 256, and one world of ~5000 features

model(tree, features, levelsup, rules=()) is written from DBoW2's statements: TemplatedVocabulary::transform (TemplatedVocabulary.h:
1219-1260: the descent with strict '<' so the first child wins, nid taken at nid_level = L - levelsup, 0 when nid_level <= 0 -- and, this
project's canonical choice for the variable the reference leaves uninitialised, 0 when the path has no node there), the word's weight,
FeatureVector::addFeature as a map ordered by NodeId with the features appended in index order, BowVector::addWeight one by one in
feature order with stopped words (weight <= 0) skipped (:1152-1160), then BowVector::normalize(L1).  numpy.argmin returns the FIRST
minimum: that is the strict '<' of the loop.  `rules` names one wrong rule at a time (RULES)."""
import numpy as np
from multi_orb_slam_amd import synth

RULES = ("last_child_wins", "second_pass_dropped", "nid_one_level_late", "bins_by_position", "items_descending", "stopped_kept",
         "root_bin_dropped", "chunk_base_not_carried")
RULE_GROUP = {"last_child_wins": "tie", "second_pass_dropped": "fanout", "nid_one_level_late": "depth", "bins_by_position": "ids",
              "items_descending": "fill", "stopped_kept": "stop", "root_bin_dropped": "depth", "chunk_base_not_carried": "bins"}
GROUPS = ("tie", "fanout", "depth", "ids", "stop", "bins", "fill")
MAX_BINS, CHUNK = 4097, 1024


# ---------------------------------------------------------------------------------------------------------------- descriptors
def flip(d, bits):
    out = np.array(d, np.uint8).copy()
    for b in bits:
        out[(b % 256) // 8] ^= np.uint8(1 << (b % 8))
    return out


def run(count, start):
    return [(start + j) % 256 for j in range(count)]


def ham(rows, f):
    return np.unpackbits(np.bitwise_xor(rows, f), axis=1).sum(1).astype(np.int64)


def _h(seed, n):
    return synth.hash32(np.arange(n, dtype=np.uint64) + np.uint64((seed * 0x9E3779B1) & 0xFFFFFFFF))


def _weights(n, seed):
    return 0.5 + (_h(seed + 977, n) % np.uint32(1000)).astype(np.float64) / 997.0


# ---------------------------------------------------------------------------------------------------------------------- trees
class Prepared:
    def __init__(self, tree):
        parent = np.asarray(tree["parent"], np.int64)
        n = len(parent)
        kids = [[] for _ in range(n)]
        for i in range(1, n):
            kids[parent[i]].append(i)                     # ascending id: the loader's push_back order
        self.children = [np.array(k, np.int64) for k in kids]
        self.word_of = np.zeros(n, np.int64)
        self.word_of[np.flatnonzero(np.asarray(tree["is_leaf"])[1:]) + 1] = np.arange(int(np.asarray(tree["is_leaf"])[1:].sum()))
        self.depth = np.zeros(n, np.int64)
        self.order = [0]                                  # breadth-first, children ascending
        for h in self.order:
            for c in kids[h]:
                self.depth[c] = self.depth[h] + 1
                self.order.append(c)
        assert len(self.order) == n, "every node is reachable"
        self.position = np.zeros(n, np.int64); self.position[self.order] = np.arange(n)
        self.depths = int(self.depth.max()) + 1
        self.level_ids = [np.sort(np.flatnonzero(self.depth == d)) for d in range(self.depths)]
        for i in range(1, n):                             # the flagged nodes are exactly the childless ones
            assert bool(tree["is_leaf"][i]) == (len(kids[i]) == 0)
        self.desc = np.ascontiguousarray(tree["desc"], np.uint8)


_PREP = {}


def prepared(tree):
    hit = _PREP.get(id(tree))
    if hit is None or hit[0] is not tree:
        hit = (tree, Prepared(tree))
        _PREP[id(tree)] = hit
    return hit[1]


def n_bins(tree, levelsup):
    T = prepared(tree)
    lvl = tree["L"] - levelsup
    return 1 + (len(T.level_ids[lvl]) if 1 <= lvl < T.depths else 0)


def _tree(parent, leaf, desc, weight, L):
    parent = np.array(parent, np.int32); leaf = np.array(leaf, np.uint8)
    weight = np.array(weight, np.float64)
    k = int(np.bincount(parent[1:], minlength=len(parent)).max())
    return dict(parent=parent, is_leaf=leaf, desc=np.ascontiguousarray(np.array(desc, np.uint8).reshape(-1, 32)), weight=weight, k=k, L=L)


def flat_tree(f0, dists, weights=None):
    """L = 1: the root's children are words; child c lies dists[c] flipped bits from f0 (its own run of bits, so equal distances are
    different descriptors unless the distance is 0 or 256)"""
    k = len(dists)
    desc = [np.zeros(32, np.uint8)] + [flip(f0, run(d, 11 * c)) for c, d in enumerate(dists)]
    w = _weights(k, k + sum(dists)) if weights is None else weights
    return _tree([0] * (k + 1), [0] + [1] * k, desc, [0.0] + list(w), 1)


def grow(fan, L, seed, flips=20):
    """Breadth-first growth: fan(level, index in the level, node id) children for a node of `level` < L (0: a leaf already)."""
    parent, leaf, desc, weight = [0], [0], [np.zeros(32, np.uint8)], [0.0]
    frontier = [0]
    for level in range(L):
        nxt = []
        for idx, node in enumerate(frontier):
            k = fan(level, idx, node)
            if node and k == 0:
                continue
            base = synth.descriptors(k, seed + 1) if node == 0 else None
            for c in range(k):
                cid = len(parent)
                d = base[c] if node == 0 else flip(desc[node], [int(x) % 256 for x in _h(seed + 31 * cid, flips)])
                parent.append(node); leaf.append(0); desc.append(d); weight.append(0.0)
                nxt.append(cid)
        frontier = nxt
    has_child = np.bincount(np.array(parent[1:]), minlength=len(parent)) > 0
    w = _weights(len(parent), seed)
    for i in range(1, len(parent)):
        if not has_child[i]:
            leaf[i] = 1; weight[i] = float(w[i])
    return _tree(parent, leaf, desc, weight, L)


def wide_root(m, seed):
    """L = 1 with m words under the root (any m: the odd bin counts)"""
    return _tree([0] * (m + 1), [0] + [1] * m, np.concatenate([np.zeros((1, 32), np.uint8), synth.descriptors(m, seed)]),
                 [0.0] + list(_weights(m, seed)), 1)


def renumber(tree, perm):
    """perm: new id -> old id (perm[0] == 0).  The same tree under other node ids."""
    perm = np.asarray(perm, np.int64)
    assert perm[0] == 0 and sorted(perm.tolist()) == list(range(len(perm)))
    inv = np.empty(len(perm), np.int64); inv[perm] = np.arange(len(perm))
    parent = inv[np.asarray(tree["parent"], np.int64)[perm]].astype(np.int32); parent[0] = 0
    return dict(parent=parent, is_leaf=tree["is_leaf"][perm].copy(), desc=tree["desc"][perm].copy(), weight=tree["weight"][perm].copy(),
                k=tree["k"], L=tree["L"])


FILL_INNER, FILL_LEAVES, FILL_ROOT_LEAVES = 64, 64, (1, 30, 67)


def _code(j):
    return [b for b in range(6) if (j >> b) & 1] + [6 + b for b in range(6) if not (j >> b) & 1]


def fill_tree(stopped=()):
    """67 children of the root: three words (ids 1, 30, 67: their features have no node at level 2 -- the root's bin) and 64 inner nodes
    with 64 words each: 4096 nodes at level 2, 4097 bins, four full chunks of 1024 and one bin more.  Word (p, j) = its parent's
    descriptor with the six-of-twelve code of j flipped in: a feature equal to a word's descriptor descends to exactly that word.
    Level-2 ids are breadth-first, so the bin of word (p, j) is 1 + 64 p + j."""
    top = synth.descriptors(67, 4242)
    parent, leaf, desc, weight = [0], [0], [np.zeros(32, np.uint8)], [0.0]
    inner = []
    for c in range(67):
        parent.append(0); desc.append(top[c]); weight.append(0.0)
        if c + 1 in FILL_ROOT_LEAVES:
            leaf.append(1)
        else:
            leaf.append(0); inner.append(c + 1)
    assert len(inner) == FILL_INNER
    for p in inner:
        for j in range(FILL_LEAVES):
            parent.append(p); leaf.append(1); desc.append(flip(desc[p], _code(j))); weight.append(0.0)
    w = _weights(len(parent), 99)
    weight = [float(w[i]) if leaf[i] else 0.0 for i in range(len(parent))]
    for i in stopped:
        assert leaf[i]
        weight[i] = 0.0
    return _tree(parent, leaf, desc, weight, 2)


def fill_word(tree, b):
    """node id of the word whose bin (levelsup 0) is b >= 1; b = 0, -1, -2: the three words under the root"""
    if b <= 0:
        return FILL_ROOT_LEAVES[-b]
    return int(prepared(tree).level_ids[2][b - 1])


# ---------------------------------------------------------------------------------------------------------------------- model
def descend(tree, f, rules=(), trace=None):
    """-> (leaf node id, [node id chosen at level 1, 2, ...])"""
    T = prepared(tree)
    cur, path = 0, []
    while True:
        kids = T.children[cur]
        if "second_pass_dropped" in rules:
            kids = kids[:16]                              # (a lane's children c + 16, c + 32, ... never looked at)
        d = ham(T.desc[kids], f)
        best = len(d) - 1 - int(np.argmin(d[::-1])) if "last_child_wins" in rules else int(np.argmin(d))
        if trace is not None:
            trace.append(d.tolist())
        cur = int(kids[best]); path.append(cur)
        if len(T.children[cur]) == 0:
            return cur, path


def device_layout(bins, nbins, level_ids, carry=True):
    """k_fv_count / k_fv_offsets / k_fv_fill restated on arrays: counts per bin, the non-empty bins compacted chunk by chunk of 1024 with
    the running base carried from chunk to chunk, every bin's features in ascending index.  carry=False is the wrong rule: the base of a
    chunk is what the chunk before it alone counted."""
    counts = np.bincount(bins[bins >= 0], minlength=nbins)
    node_id, node_start, b2n = np.zeros(nbins + 1, np.uint32), np.zeros(nbins + 1, np.int32), np.full(nbins, -1, np.int64)
    base_n = base_i = 0
    for b0 in range(0, nbins, CHUNK):
        c = counts[b0:b0 + CHUNK]
        nodes, items = np.cumsum(c > 0), np.cumsum(c)
        for t in np.flatnonzero(c > 0):
            nd = base_n + nodes[t] - 1
            node_id[nd] = 0 if b0 + t == 0 else level_ids[b0 + t - 1]
            node_start[nd] = base_i + items[t] - c[t]
            b2n[b0 + t] = nd
        if carry:
            base_n += int(nodes[-1]); base_i += int(items[-1])
        else:
            base_n, base_i = int(nodes[-1]), int(items[-1])
    node_start[base_n] = base_i
    out = np.zeros(max(len(bins), 1), np.uint32)
    for b in np.flatnonzero(b2n >= 0):
        mine = np.flatnonzero(bins == b)
        pos = node_start[b2n[b]]
        out[pos:pos + len(mine)] = mine[:max(0, len(out) - pos)]
    return node_id[:base_n].copy(), node_start[:base_n + 1].copy(), out[:base_i].copy(), int(counts.max()) if len(counts) else 0


def model(tree, features, levelsup, rules=(), trace=None):
    """-> dict(word, node, weight per feature; bow = (ids, values); fv = (node_id, node_start, items); bins, nbins, largest)"""
    assert all(r in RULES for r in rules)
    T = prepared(tree)
    feats = np.ascontiguousarray(features, np.uint8).reshape(-1, 32)
    n = len(feats)
    nid_level = tree["L"] - levelsup
    at = nid_level + (1 if "nid_one_level_late" in rules else 0)
    word, node, weight = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.float64)
    for i in range(n):
        tr = [] if trace is not None else None
        leaf, path = descend(tree, feats[i], rules, tr)
        if trace is not None:
            trace[i] = tr
        word[i] = T.word_of[leaf]
        node[i] = path[at - 1] if 1 <= at <= len(path) else 0
        weight[i] = tree["weight"][leaf]
    kept = [i for i in range(n) if weight[i] > 0 or "stopped_kept" in rules]
    # BowVector::addWeight, one by one in feature order; normalize(L1)
    bv = {}
    for i in kept:
        w = int(word[i])
        if w in bv:
            bv[w] += float(weight[i])
        else:
            bv[w] = float(weight[i])
    ids = sorted(bv)
    vals = [bv[w] for w in ids]
    norm = 0.0
    for v in vals:
        norm += abs(v)
    if norm > 0.0:
        vals = [v / norm for v in vals]
    # FeatureVector::addFeature: a map ordered by NodeId, push_back in index order
    fv = {}
    for i in kept:
        if "root_bin_dropped" in rules and node[i] == 0:
            continue
        fv.setdefault(int(node[i]), []).append(i)
    keys = sorted(fv, key=(lambda k: T.position[k]) if "bins_by_position" in rules else None)
    if "bins_by_position" in rules and 0 in fv:
        keys = [0] + [k for k in keys if k]
    starts, items = [0], []
    for k in keys:
        items += fv[k][::-1] if "items_descending" in rules else fv[k]
        starts.append(len(items))
    fvec = (np.array(keys, np.uint32), np.array(starts, np.int32), np.array(items, np.uint32))
    # the device's bins: 0 the root's, else 1 + rank by NodeId among the nodes of the level; -1 a stopped word
    nbins = n_bins(tree, levelsup)
    lvl = T.level_ids[nid_level] if nbins > 1 else np.zeros(0, np.int64)
    kept_set = set(kept)
    bins = np.array([(-1 if i not in kept_set else 0 if node[i] == 0 else 1 + int(np.searchsorted(lvl, node[i]))) for i in range(n)], np.int64)
    if "chunk_base_not_carried" in rules and nbins <= MAX_BINS:
        a, b, c, _ = device_layout(bins, nbins, lvl, carry=False)
        fvec = (a, b, c)
    largest = max([starts[j + 1] - starts[j] for j in range(len(keys))] + [0])
    return dict(word=word, node=node, weight=weight, bow=(np.array(ids, np.uint32), np.array(vals, np.float64)), fv=fvec, bins=bins, nbins=nbins,
                largest=largest, items=len(items))


def differing(a, b, keys=("word", "node", "weight", "bow", "fv")):
    """names of the outputs in which two answers differ, byte for byte"""
    out = []
    for k in keys:
        x, y = a[k], b[k]
        x, y = (x, y) if isinstance(x, tuple) else ((x,), (y,))
        if len(x) != len(y) or any(np.asarray(p).dtype != np.asarray(q).dtype or np.asarray(p).tobytes() != np.asarray(q).tobytes() for p, q in zip(x, y)):
            out.append(k)
    return out


# --------------------------------------------------------------------------------------------------------------------- worlds
def _world(name, group, tree, feats, levelsup, **promise):
    return dict(name=name, group=group, tree=tree, feats=np.ascontiguousarray(np.array(feats, np.uint8).reshape(-1, 32)), levelsup=levelsup,
                promise=promise)


def near_words(tree, n, seed, flips=6):
    """n features a few flipped bits from hashed words of the tree, every third one a fresh random descriptor"""
    leaves = np.flatnonzero(np.asarray(tree["is_leaf"]))
    pick = leaves[_h(seed, n) % np.uint32(len(leaves))]
    rnd = synth.descriptors(n, seed + 7)
    out = [rnd[i] if i % 3 == 2 else flip(tree["desc"][pick[i]], [int(x) % 256 for x in _h(seed * 131 + i, flips)]) for i in range(n)]
    return np.array(out, np.uint8).reshape(-1, 32)


F0 = synth.descriptors(1, 777)[0]


def tie_worlds():
    cases = [   # name, distances of the root's children from the first feature, the children that tie for the best
        ("two_lanes", [40, 30, 50, 30, 60], (1, 3)), ("three_lanes", [40, 30, 30, 50, 30], (1, 2, 4)),
        ("first_last_k2", [33, 33], (0, 1)), ("first_last_k20", [30] + [60] * 18 + [30], (0, 19)),
        ("second_pass_k17", [30] + [60] * 15 + [30], (0, 16)), ("second_pass_k20", [60] * 3 + [30] + [60] * 15 + [30], (3, 19)),
        ("third_pass_k33", [30] + [60] * 15 + [30] + [60] * 15 + [30], (0, 16, 32)), ("second_pass_k33_lane1", [60, 30] + [60] * 15 + [30] + [60] * 15, (1, 17)),
        ("all_equal_k17", [50] * 17, tuple(range(17))), ("all_equal_k33", [77] * 33, tuple(range(33))), ("all_equal_k5", [128] * 5, tuple(range(5))),
        ("zero_best", [10, 0, 20], (1,)), ("zero_tie", [10, 0, 0], (1, 2)), ("zero_tie_second_pass", [10] * 16 + [0, 10, 0], (16, 18)),
        ("complement_only", [256], (0,)), ("complement_tie", [256, 256, 256], (0, 1, 2)), ("complement_tie_k17", [256] * 17, tuple(range(17))),
        ("complement_loses", [256, 255, 256], (1,)), ("best_255_tie", [256, 255, 255], (1, 2))]
    out = []
    for name, dists, tie in cases:
        tree = flat_tree(F0, dists)
        feats = [F0] + [tree["desc"][1 + c] for c in range(len(dists))] + list(synth.descriptors(3, len(dists)))
        out.append(_world("tie_" + name, "tie", tree, feats, 0, tie=tie, dist=min(dists)))
    return out


def fanout_worlds():
    out = []
    for k in (1, 2, 15, 16, 17, 20, 32, 33):
        tree = grow(lambda level, idx, node, k=k: k if level == 0 else max(1, min(k, 1 + (idx + k) % 3)), 2, 50 + k)
        feats = list(near_words(tree, 40, k)) + [tree["desc"][i] for i in range(1, k + 1)]
        out.append(_world("fanout_k%d" % k, "fanout", tree, feats, 1, k=k))
    # the best child is one only a later pass of its lane sees
    for k, best in ((17, 16), (20, 17), (33, 32), (33, 20)):
        tree = flat_tree(F0, [60 + c % 5 for c in range(best)] + [30] + [64] * (k - best - 1))
        out.append(_world("fanout_best_%d_of_%d" % (best, k), "fanout", tree, [F0] + list(synth.descriptors(5, k)), 0, k=k, best=best))
    return out


def depth_worlds():
    out = []
    for L in range(1, 7):
        tree = grow(lambda level, idx, node: 2 + (level == 0), L, 300 + L)
        feats = near_words(tree, 30, L)
        for levelsup in sorted({0, 1, L - 1, L, L + 2}):
            out.append(_world("depth_L%d_up%d" % (L, levelsup), "depth", tree, feats, levelsup, L=L))
    # ragged: the FeatureVector's level is 2 (declared L = 3, levelsup 1); words at depth 1 (above: the root's bin), 2 (at) and 3 (below)
    ragged = grow(lambda level, idx, node: (4, (0, 3, 2, 3)[idx % 4], (0, 2, 3)[idx % 3])[level], 3, 77)
    T = prepared(ragged)
    feats = [ragged["desc"][i] for i in range(1, len(ragged["parent"])) if ragged["is_leaf"][i]] + list(near_words(ragged, 20, 5))
    for levelsup in (0, 1, 2, 3):
        out.append(_world("depth_ragged_up%d" % levelsup, "depth", ragged, feats, levelsup, ragged=True,
                          leaf_depths=sorted({int(T.depth[i]) for i in range(1, len(T.depth)) if ragged["is_leaf"][i]})))
    return out


def ids_worlds():
    base = grow(lambda level, idx, node: 6 if level == 0 else 2 + (idx % 4), 3, 21)
    n = len(base["parent"])
    shuffled = np.concatenate([[0], 1 + np.argsort(synth.hash32(np.arange(n - 1, dtype=np.uint64) + np.uint64(99)))])
    # (reversing ALL ids keeps every level in breadth-first order: parents and children turn round together.  Reversing the ids of the even
    # levels alone turns the children's blocks round against their parents.)
    T = prepared(base)
    reverse = np.arange(n)
    for d in range(2, T.depths, 2):
        reverse[T.level_ids[d]] = T.level_ids[d][::-1]
    feats = near_words(base, 120, 8)
    out = []
    for name, perm in (("shuffled", shuffled), ("reversed", reverse)):
        tree = renumber(base, perm)
        for levelsup in ((0, 1) if name == "shuffled" else (1,)):     # (level 1 is always in id order: its nodes share one parent)
            out.append(_world("ids_%s_up%d" % (name, levelsup), "ids", tree, feats, levelsup))
    # by hand: two inner nodes 2 and 1 (the first child has the larger id... ids ascending decide the child order, so give the LEVEL-2
    # nodes ids that run against their breadth-first position: children of node 1 are 5 and 6, children of node 2 are 3 and 4)
    d = synth.descriptors(2, 5)
    desc = [np.zeros(32, np.uint8), d[0], d[1], flip(d[1], run(9, 0)), flip(d[1], run(9, 40)), flip(d[0], run(9, 0)), flip(d[0], run(9, 40))]
    hand = _tree([0, 0, 0, 2, 2, 1, 1], [0, 0, 0, 1, 1, 1, 1], desc, [0, 0, 0, 1.25, 0.75, 2.5, 1.0], 2)
    feats = [desc[5], desc[3], desc[6], desc[4], desc[5], desc[4]]
    out.append(_world("ids_hand_reversed", "ids", hand, feats, 0, order=[3, 4, 5, 6]))
    return out


def stop_worlds():
    out = []
    k = 6
    dists = [20 + 3 * c for c in range(k)]
    own = lambda tree: [tree["desc"][1 + c] for c in (0, 1, 2, 3, 4, 5, 2, 0, 5)]
    for name, w in (("zero_and_negative", [1.5, 0.0, 2.0, -0.75, 0.25, -0.0]), ("all_stopped", [0.0, -1.0, 0.0, -0.0, 0.0, -2.5]),
                    ("one_kept", [0.0, 0.0, 3.5, 0.0, -1.0, 0.0])):
        tree = flat_tree(F0, dists, w)
        out.append(_world("stop_" + name, "stop", tree, own(tree), 0, weights=w))
    # one node at level 1 (the only non-root bin) whose two words are one stopped, one not; then both stopped
    d = synth.descriptors(1, 9)[0]
    for name, w in (("in_the_only_bin", [0.0, 2.0]), ("the_only_bin_all_stopped", [0.0, -1.0])):
        desc = [np.zeros(32, np.uint8), d, flip(d, run(5, 0)), flip(d, run(5, 100))]
        tree = _tree([0, 0, 1, 1], [0, 0, 1, 1], desc, [0, 0] + w, 2)
        out.append(_world("stop_" + name, "stop", tree, [desc[2], desc[3], desc[2], desc[3], desc[3]], 1, weights=w))
    return out


def _binary(depth, seed):
    return grow(lambda level, idx, node: 2, depth, seed, flips=24)


def bins_worlds():
    out = []
    out.append(_world("bins_1_level_zero", "bins", wide_root(5, 1), synth.descriptors(20, 3), 1, nbins=1))
    out.append(_world("bins_1_no_such_level", "bins", wide_root(5, 1), synth.descriptors(20, 3), -2, nbins=1))
    t1 = grow(lambda level, idx, node: (1, 3)[level], 2, 14)
    out.append(_world("bins_2", "bins", t1, near_words(t1, 20, 2), 1, nbins=2))
    for m in (1023, 1025, 2047, 4095, 4097):
        tree = wide_root(m, m)
        picks = sorted({0, 1, m // 2, m - 2, m - 1} | {int(x) % m for x in _h(m, 40)} | ({1022, 1023, 1024} if m > 1024 else set()))
        feats = [tree["desc"][1 + c] for c in picks] + list(synth.descriptors(10, m))
        out.append(_world("bins_%d_wide" % (m + 1), "bins", tree, feats, 0, nbins=m + 1, refused=m + 1 > MAX_BINS))
    for depth in (10, 11, 12):
        tree = _binary(depth, 600 + depth)
        feats = list(near_words(tree, 150, depth, flips=3)) + [tree["desc"][-1], tree["desc"][-2 ** depth]]
        out.append(_world("bins_%d_binary" % (2 ** depth + 1), "bins", tree, feats, 0, nbins=2 ** depth + 1))
    for k in (32, 64):
        tree = grow(lambda level, idx, node, k=k: k, 2, 700 + k)
        feats = list(near_words(tree, 150, k, flips=3)) + [tree["desc"][-1], tree["desc"][-k * k]]
        out.append(_world("bins_%d_k%d" % (k * k + 1, k), "bins", tree, feats, 0, nbins=k * k + 1))
    return out


FILL_COUNTS = (0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257)


def fill_worlds():
    tree = fill_tree()
    word = lambda b: tree["desc"][fill_word(tree, b)]
    out = []
    occ = dict(none=[], root_only=[0, -1, 0, -2], last_only=[4096, 4096, 4096], chunk_edges=[1024, 1023, 2048, 2047, 1023, 2048],
               more_chunk_edges=[4096, 3072, 3071, 4095, 1, 0, 1024, 3072],
               every=list(range(4096, -1, -1)), every_other=list(range(0, 4097, 2)), one_bin_all=[2500] * 300, first_bin_all=[1] * 130)
    for name, bins in occ.items():
        out.append(_world("fill_" + name, "fill", tree, [word(b) for b in bins], 0, bins=[max(b, 0) for b in bins],
                          largest=(300 if name == "one_bin_all" else 130 if name == "first_bin_all" else None)))
    for n in FILL_COUNTS + (5000,):
        spread = 37 if n < 1000 else 700
        bins = [int(x) for x in (_h(n + 5, n) % np.uint32(spread)) * np.uint32(4097 // spread)]
        out.append(_world("fill_n%d" % n, "fill", tree, [word(b) for b in bins], 0, bins=bins, n=n))
    stopped = fill_tree(stopped=[fill_word(tree, b) for b in (0, 1024, 2048)])
    bins = [0, 1023, 1024, 1025, 2048, 2049, 1024, 4096]
    out.append(_world("fill_stopped_at_the_chunk_edges", "fill", stopped, [stopped["desc"][fill_word(stopped, b)] for b in bins], 0,
                      bins=[b for b in bins if b not in (0, 1024, 2048)]))
    return out


def worlds():
    return tie_worlds() + fanout_worlds() + depth_worlds() + ids_worlds() + stop_worlds() + bins_worlds() + fill_worlds()


N_WORLDS = 19 + 12 + 31 + 4 + 5 + 13 + 22


# ----------------------------------------------------------------------------------------------------------------- conditions
def check_conditions(w):
    """What the world's group promises, asserted on the model alone.  -> number of conditions checked"""
    p, tree, g = w["promise"], w["tree"], w["group"]
    T = prepared(tree)
    trace = {}
    ans = model(tree, w["feats"], w["levelsup"], trace=trace)
    n = 0
    if g == "tie":
        d = trace[0][0]                                   # distances of the first feature to the root's children
        assert min(d) == p["dist"] and tuple(i for i, x in enumerate(d) if x == min(d)) == p["tie"]
        assert int(ans["word"][0]) == p["tie"][0]         # L = 1: word c is child c
        if len(p["tie"]) > 1:
            assert int(model(tree, w["feats"], w["levelsup"], ("last_child_wins",))["word"][0]) == p["tie"][-1]
        n += 2
    elif g == "fanout":
        assert tree["k"] == p["k"] == max(len(c) for c in T.children)
        if "best" in p:
            assert int(np.argmin(trace[0][0])) == p["best"] >= 16 and int(ans["word"][0]) == p["best"]
        n += 1
    elif g == "depth":
        if p.get("ragged"):
            assert p["leaf_depths"] == [1, 2, 3]
            lvl = tree["L"] - w["levelsup"]
            lens = {len(trace[i]) for i in trace}
            assert lens == {1, 2, 3}
            if lvl == 2:
                assert {len(trace[i]) for i in trace if ans["node"][i] == 0} == {1} and 0 in ans["fv"][0]
        else:
            assert T.depths == p["L"] + 1 == tree["L"] + 1 and all(len(trace[i]) == p["L"] for i in trace)
            lvl = tree["L"] - w["levelsup"]
            assert (ans["node"] == 0).all() == (lvl <= 0)
        n += 1
    elif g == "ids":
        lvl = tree["L"] - w["levelsup"]
        ids = T.level_ids[lvl]
        by_pos = sorted(ids, key=lambda i: T.position[i])
        assert list(ids) != by_pos                        # rank by NodeId is not the breadth-first position
        assert any(tree["parent"][i] > i for i in range(1, len(tree["parent"]))) or "reversed" in w["name"]
        if "order" in p:
            assert ans["fv"][0].tolist() == p["order"] and by_pos == [5, 6, 3, 4]
        n += 2
    elif g == "stop":
        stopped = sum(1 for x in ans["weight"] if not x > 0)
        assert stopped > 0 and ans["items"] == len(w["feats"]) - stopped
        if "all_stopped" in w["name"]:
            assert ans["items"] == 0 and len(ans["bow"][0]) == 0 and len(ans["fv"][0]) == 0
        if w["name"] == "stop_one_kept":
            assert len(ans["bow"][0]) == 1 and ans["bow"][1].tolist() == [1.0]
        if w["name"] == "stop_in_the_only_bin":
            assert ans["nbins"] == 2 and len(ans["fv"][0]) == 1 and ans["fv"][0][0] != 0 and 0 < ans["items"] < len(w["feats"])
        n += 2
    elif g == "bins":
        assert ans["nbins"] == p["nbins"] == n_bins(tree, w["levelsup"])
        assert bool(p.get("refused")) == (ans["nbins"] > MAX_BINS)
        if ans["nbins"] > CHUNK and not p.get("refused"):
            occupied = set(ans["bins"].tolist())
            assert any(b >= CHUNK for b in occupied) and any(0 <= b < CHUNK for b in occupied)      # nodes on both sides of a chunk edge
        n += 2
    elif g == "fill":
        got = sorted(b for b in ans["bins"].tolist() if b >= 0)
        assert got == sorted(p["bins"]) and ans["nbins"] == MAX_BINS
        if p.get("largest"):
            assert ans["largest"] == p["largest"] == len(w["feats"])
        if "n" in p:
            assert len(w["feats"]) == p["n"]
        n += 2
    # the device's layout, restated, is the map's on every world that the device accepts
    if ans["nbins"] <= MAX_BINS:
        lvl = T.level_ids[tree["L"] - w["levelsup"]] if ans["nbins"] > 1 else np.zeros(0, np.int64)
        a, b, c, largest = device_layout(ans["bins"], ans["nbins"], lvl)
        assert a.tobytes() == ans["fv"][0].tobytes() and b.tobytes() == ans["fv"][1].tobytes() and c.tobytes() == ans["fv"][2].tobytes()
        assert largest == ans["largest"]
        n += 1
    return n
