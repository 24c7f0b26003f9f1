"""Boundary worlds of the BoW-gated searches (csrc/bow.hip: k_bow_join MODE 0 SearchByBoW(KF, F), MODE 1 SearchByBoW(KF, KF), MODE 2
SearchForTriangulation; k_bow_finish): two sides whose every query sits on a decision of oracle/bow_oracle.cpp, both sides of it.

A vocabulary node is a natural ISLAND: a query sees the candidates of its own node and nothing else, and both sides take a hand-built
FeatureVector.  Every island is a node of its own; a world is a set of nodes.  An island's descriptors are a random 256-bit code with an
exact number of its first bits flipped (search_boundary_worlds._Builder.desc restated in `flip`), so every distance that matters is
chosen: a candidate "at d" lies d bits from the island's probe query, two candidates at d1 and d2 lie |d1 - d2| apart.  FILLERS are
candidates at 226 .. 256 bits from the probe (the code's complement with a few bits flipped back): farther than every threshold in
use and than every intended runner-up, they only make the node -- and with the largest node the FORM of the whole call -- what the
world's `size` says.  `check_isolation` asserts exactly that before anything is compared.

The forms come from enqueue_join's arithmetic, restated in `join_form` (one wave per node / four, fully staged in LDS / a stage of
`lds_cand` candidates and a tail read from HBM); `form_sizes` derives the node sizes either side of each threshold from it.  Float
boundary values come from bisection over float32 bit patterns (`cross` of search_boundary_worlds) on the model's own intermediates
(tests/bow_model.py); none is typed in.

This is input generation only: what is expected of a device comes from the oracle."""
import functools
import numpy as np
import bow_model as bm
import search_boundary_worlds as sbw
from search_boundary_worlds import POPULATIONS, RATIOS, cross, ratio_pairs, ratio_rejects, rot_bin, rot_of, round_half_away  # noqa: F401

f32 = np.float32
JOIN_LDS_BYTES, WIDE_FROM = 65536, 128      # csrc/bow.hip: JOIN_LDS_BYTES; enqueue_join `wide = max_nc >= 128`
TIE_RATIO = 1.5                             # the one ratio above 1: two equal candidates are accepted, the FIRST of them (modes 0 / 1)
BIG_RATIOS = (RATIOS[0], RATIOS[1])         # 0.6 (at th 30) and 0.7 (at th 50)
FAR = 30                                    # fillers lie 256 - FAR .. 256 bits from the probe


def join_form(max_nc):
    """enqueue_join's arithmetic -> (waves per node, lds_cand)."""
    claimed = (max_nc + 63) & ~63
    lds = max(0, min(max_nc, (JOIN_LDS_BYTES - claimed) // 40))
    if lds < max_nc:
        lds &= ~63
    return (4 if max_nc >= WIDE_FROM else 1), lds


@functools.lru_cache(None)
def form_sizes():
    """-> dict(one_wave, four_waves, rounds, staged, tail, long_tail): the largest node of one wave, the smallest of four, one in which four
    stripes take more than two rounds (three candidates of one lane), the largest that is staged whole, the smallest with a tail (one
    partial round of the first stripe), and the smallest whose tail reaches into a third stripe."""
    one = max(n for n in range(1, 4096) if join_form(n)[0] == 1)
    staged = max(n for n in range(1, 4096) if join_form(n)[1] == n)
    assert join_form(one + 1)[0] == 4 and join_form(staged + 1)[1] < staged + 1 and join_form(4095)[1] < 4095
    long_tail = min(n for n in range(staged + 1, 4096) if n - join_form(n)[1] >= 2 * 64 + 36)   # the tail reaches into a third stripe
    return dict(one_wave=one, four_waves=one + 1, rounds=2 * 256 + 64 + 5, staged=staged, tail=staged + 1, long_tail=long_tail)


def flip(base, d):
    """`base` with its first d bits flipped."""
    out = base.copy()
    full, rest = divmod(int(d), 8)
    out[:full] ^= 0xFF
    if rest:
        out[full] ^= np.uint8((1 << rest) - 1)
    return out


def bow_accepts(best, second, nnratio, double=False):
    """(float)best < nnratio * (float)second: the searches here ACCEPT on `<` (the projection searches reject on `>`: ratio_rejects)."""
    if double:
        return float(best) < float(f32(nnratio)) * float(second)
    return bool(f32(best) < f32(f32(nnratio) * f32(second)))


def float_double_pairs(nnratio, th=256):
    """Every (best, second) within the threshold that the float product accepts and the double product does not, or the other way."""
    return [(b, s) for s in range(1, 257) for b in range(1, min(s, th) + 1) if bow_accepts(b, s, nnratio) != bow_accepts(b, s, nnratio, True)]


# ------------------------------------------------------------------------------------------------ the builder
class _Builder:
    def __init__(self, kind, size, th, nnratio, seed):
        self.kind, self.size, self.th, self.nnratio = kind, size, th, nnratio
        self.rng = np.random.default_rng(seed)
        self.waves, self.lds = join_form(size)
        self.A = dict(desc=[], angle=[], flags=[], x=[], y=[], octave=[], cam_of=[])
        self.B = dict(desc=[], angle=[], flags=[], x=[], y=[], octave=[], cam_of=[])
        self.a_items, self.b_items = [], []          # per node
        self.islands = []
        self.role_b = []                             # per feature of b: "" (filler) or the candidate's role
        self.owner_a, self.owner_b = [], []          # island of every feature

    def _feat(self, S, desc, ang=0.0, flags=3, x=100.0, y=100.0, octave=0, cam=0):
        S["desc"].append(desc); S["angle"].append(f32(ang)); S["flags"].append(flags); S["x"].append(f32(x)); S["y"].append(f32(y))
        S["octave"].append(octave); S["cam_of"].append(cam)
        return len(S["desc"]) - 1

    def island(self, group, side, cands, queries=None, nc=None, far=FAR, probe=None, note=""):
        """One node.  cands: dicts(d, role[, j][, feature fields]) -- `j` is the position in the node (default: the next free one);
        queries: dicts(d[, role][, feature fields]) in the node's order, default one probe at d = 0 (`probe`: its feature fields).  The
        LAST query is the probe: the one whose answer the island is about.  nc: candidates of the node, fillers included."""
        D = self.rng.integers(0, 256, 32, dtype=np.uint8)
        isl = len(self.islands)
        queries = [dict(d=0, **(probe or {}))] if queries is None else [dict(q) for q in queries]
        qa = []
        for q in queries:
            q = dict(q); d = q.pop("d"); q.pop("role", None)
            qa.append(self._feat(self.A, flip(D, d), **q)); self.owner_a.append(isl)
        nc = max(nc or 0, len(cands))
        at = {}
        free = iter([j for j in range(nc) if j not in {c["j"] for c in cands if "j" in c}])
        for c in cands:
            j = c["j"] if "j" in c else next(free)
            assert 0 <= j < nc and j not in at, (group, side, j, nc)
            at[j] = c
        items, cand_of = [], {}
        fill_d = (256 - self.rng.integers(0, far + 1, nc)) if far else np.full(nc, 256)
        fill_desc = {}
        for j in range(nc):
            if j in at:
                c = dict(at[j]); d = c.pop("d"); role = c.pop("role"); c.pop("j", None)
                g = self._feat(self.B, flip(D, d), **c); cand_of[role] = g; self.role_b.append(role)
            else:
                k = int(fill_d[j])
                if k not in fill_desc:
                    fill_desc[k] = flip(D, k)
                g = self._feat(self.B, fill_desc[k]); self.role_b.append("")
            self.owner_b.append(isl); items.append(g)
        self.a_items.append(qa); self.b_items.append(items)
        self.islands.append(dict(group=group, side=side, node=isl, queries=qa, probe=qa[-1], cands=cand_of, note=note,
                                 cand_d=sorted(c["d"] for c in cands), query_d=[q["d"] for q in queries]))
        return self.islands[-1]

    def finish(self, **extra):
        def side(S, items):
            n = len(S["desc"])
            start = np.concatenate([[0], np.cumsum([len(i) for i in items])]).astype(np.int32)
            return dict(desc=np.array(S["desc"], np.uint8).reshape(n, 32), angle=np.array(S["angle"], f32), flags=np.array(S["flags"], np.uint8),
                        x=np.array(S["x"], f32), y=np.array(S["y"], f32), octave=np.array(S["octave"], np.int32),
                        cam_of=np.array(S["cam_of"], np.int32), node_id=(10 * (1 + np.arange(len(items)))).astype(np.uint32),
                        node_start=start, items=np.array([g for i in items for g in i], np.uint32))
        w = dict(kind=self.kind, size=self.size, th=self.th, nnratio=self.nnratio, a=side(self.A, self.a_items), b=side(self.B, self.b_items),
                 islands=self.islands, role_b=np.array(self.role_b), owner_a=np.array(self.owner_a), owner_b=np.array(self.owner_b),
                 form=(self.waves, max(len(i) for i in self.b_items), self.lds))
        w.update(extra)
        return w


def check_isolation(w):
    """For every query, every candidate of its node that is not of its island's cast lies farther than th_low and than every candidate of
    the cast (so farther than the intended runner-up, whoever has been claimed); the largest node is the world's size.  -> fillers checked"""
    a, b = w["a"], w["b"]
    checked = 0
    assert max(np.diff(b["node_start"])) == w["size"] == w["form"][1]
    for isl in w["islands"]:
        items = b["items"][b["node_start"][isl["node"]]:b["node_start"][isl["node"] + 1]]
        fillers = items[w["role_b"][items] == ""]
        if not len(fillers):
            continue
        for q, dq in zip(isl["queries"], isl["query_d"]):
            d = bm.distances(a["desc"][q], b["desc"][fillers])
            bound = max([w["th"]] + [min(abs(c - dq), 255) for c in isl["cand_d"]])
            assert d.min() > bound or d.min() == 256, (isl["group"], isl["side"], int(d.min()), bound)   # (256 is never best nor second)
            checked += len(fillers)
    return checked


# ------------------------------------------------------------------------------------------------ placements in a node
def placements(nc, waves, lds):
    """Where best (b), runner-up (s) and a third candidate (t) of one query sit in a node of nc candidates: name -> dict(b, s[, t]).
    Candidate j belongs to lane j % 64 and, with four waves, to stripe (j / 64) % 4: one lane sees j, j + 64 * waves, ..."""
    period = 64 * waves
    staged = min(nc, lds)
    P = {"same_lane_best_first": dict(b=5, s=5 + period), "same_lane_second_first": dict(b=5 + period, s=5),
         "same_lane_third_first": dict(t=5, s=5 + period, b=5 + 2 * period), "same_lane_third_last": dict(b=5, s=5 + period, t=5 + 2 * period),
         "same_lane_third_between": dict(b=5, t=5 + period, s=5 + 2 * period),
         "other_lane": dict(b=5, s=6), "other_lane_reversed": dict(b=6, s=5), "other_stripe": dict(b=5, s=70), "other_stripe_reversed": dict(b=133, s=5),
         "first_and_63": dict(b=0, s=63), "63_and_first": dict(b=63, s=0), "64_and_first": dict(b=64, s=0), "63_and_64": dict(b=63, s=64),
         "last_and_first": dict(b=nc - 1, s=0), "first_and_last": dict(b=0, s=nc - 1),
         "stage_end_and_after": dict(b=staged - 1, s=staged), "after_and_stage_end": dict(b=staged, s=staged - 1),
         "staged_and_tail_same_lane": dict(b=5, s=staged + 5), "tail_and_staged_same_lane": dict(b=staged + 5, s=5),
         "both_in_tail": dict(b=staged + 9, s=staged + 40), "both_in_tail_reversed": dict(b=nc - 1, s=staged),
         "tail_second_stripe_and_first": dict(b=staged + 64 + 9, s=staged + 5), "tail_first_and_third_stripe": dict(b=staged + 5, s=staged + 128 + 9),
         "tail_second_stripe_and_staged": dict(b=staged + 64 + 9, s=9), "tail_same_lane_two_stripes": dict(b=staged + 128 + 5, s=staged + 64 + 5)}
    out = {}
    for name, p in P.items():
        js = list(p.values())
        if all(0 <= j < nc for j in js) and len(set(js)) == len(js):
            if ("tail" in name or "after" in name) and staged == nc:
                continue                                 # (no tail in this form)
            out[name] = p
    return out


# ------------------------------------------------------------------------------------------------ SearchByBoW (modes 0 and 1)
def _refused_pair(nnratio, th):
    """(best, second) with best <= th - 1 that the ratio test refuses while (best - 1, second) passes: the first of ratio_pairs' edges."""
    for b, s in ratio_pairs(nnratio, th)[0]:
        for bb in (b, b + 1):
            if bb < th and bb < s and not bow_accepts(bb, s, nnratio) and bow_accepts(bb - 1, s, nnratio):
                return bb, s
    raise AssertionError("no ratio edge under the threshold")


def _bow_groups(B):
    th, r, size = B.th, B.nnratio, B.size
    # ---- distance threshold: one candidate, no runner-up
    for d, side in ((th - 1, "below"), (th, "at"), (th + 1, "above")):
        B.island("threshold", side, [dict(d=d, role="a")])
    if r == TIE_RATIO:
        B.island("tie", "equal_first_wins", [dict(d=20, role="a"), dict(d=20, role="b")])
        B.island("tie", "equal_first_wins_far_apart", [dict(d=20, role="a", j=3), dict(d=20, role="b", j=size - 2)], nc=size)
        B.island("tie", "second_nearer", [dict(d=20, role="a"), dict(d=19, role="b")])
        return
    # ---- ratio: the edges of ratio_pairs (largest best the projection searches' `>` lets through), moved to this search's `<`
    edges, differ = ratio_pairs(r, th)
    picks = [(b, s, "edge") for b, s in edges] + [(b, s, "float_equal") for b, s in differ[:1] + differ[len(differ) // 2:len(differ) // 2 + 1] + differ[-1:]]
    fd = float_double_pairs(r, th)
    picks += [(b, s, "float_double") for b, s in fd[:1] + fd[-1:]]
    for b, s, why in picks:
        for bb in (b - 1, b, b + 1):
            if 1 <= bb <= min(th - 1, s):
                side = "%s_%d_%d" % ("accepted" if bow_accepts(bb, s, r) else "refused", bb, s)
                B.island("ratio_" + why, side, [dict(d=bb, role="a"), dict(d=s, role="b")])
                B.island("ratio_" + why, side + "_rev", [dict(d=s, role="b"), dict(d=bb, role="a")])
    rb, rs = _refused_pair(r, th)
    B.refused = (rb, rs)
    B.island("ratio_runner_up", "absent", [dict(d=rb, role="a")])                                        # second stays 256
    B.island("ratio_runner_up", "at_256", [dict(d=rb, role="a"), dict(d=256, role="b")], far=0)
    B.island("ratio_runner_up", "at_256_with_fillers_at_256", [dict(d=rb, role="a"), dict(d=256, role="b")], nc=70, far=0)
    B.island("ratio_runner_up", "present", [dict(d=rb, role="a"), dict(d=rs, role="b")])
    B.island("ratio_runner_up", "equal_to_best", [dict(d=rb - 1, role="a"), dict(d=rb - 1, role="b")])    # always refused at ratio <= 1
    # ---- placement of best and runner-up: (rb, rs) is refused, (rb - 1, rs) accepted -- a runner-up that is missed or doubled shows
    # (the groups that fill whole nodes stand in the worlds of BIG_RATIOS only, one per threshold: they do not depend on the ratio)
    full = r in BIG_RATIOS
    for name, p in placements(size, B.waves, B.lds).items() if full else ():
        for best, side in ((rb, "refused"), (rb - 1, "accepted")):
            cands = [dict(d=best, role="a", j=p["b"]), dict(d=rs, role="b", j=p["s"])]
            if "t" in p:
                cands.append(dict(d=rs + 7, role="c", j=p["t"]))
            B.island("placement", "%s_%s" % (name, side), cands, nc=size)
    # ---- claims
    cast = [dict(d=5, role="a"), dict(d=19, role="b"), dict(d=40, role="c")]
    assert bow_accepts(19, 40, r) and bow_accepts(5, 19, r) and not bow_accepts(7, 7, r)
    blocker = dict(d=5)                                  # its descriptor IS candidate a's: it takes a at distance 0
    B.island("claim", "taken", cast, queries=[blocker, dict(d=0)])                                         # queries 0 and 1 of the node
    B.island("claim", "free", cast)
    B.island("claim", "first_refused", cast, queries=[dict(d=12), dict(d=0)])                               # 7 against 7: refused, leaves a alone
    far_q = [dict(d=256 - k % 7) for k in range(63)]     # 63 queries that match nothing, then the pair: numbers 63 and 64 of the node
    B.island("claim", "taken_across_the_block", cast, queries=far_q + [blocker, dict(d=0)], far=0)
    B.island("claim", "free_across_the_block", cast, queries=far_q + [dict(d=12), dict(d=0)], far=0)
    stage = min(size, B.lds)
    big = lambda ja: [dict(cast[0], j=ja), dict(cast[1], j=(ja + 64) % size), dict(cast[2], j=(ja + 129) % size)]
    if full:
        B.island("claim", "taken_staged", big(7), queries=[blocker, dict(d=0)], nc=size)
        B.island("claim", "taken_last_staged", big(stage - 1), queries=[blocker, dict(d=0)], nc=size)
    if full and stage < size:
        B.island("claim", "taken_in_tail", big(stage + 11), queries=[blocker, dict(d=0)], nc=size)
        B.island("claim", "runner_up_in_tail", [dict(cast[0], j=3), dict(cast[1], j=size - 1), dict(cast[2], j=stage)], queries=[blocker, dict(d=0)], nc=size)
        for st in (1, 2):                                # ... and in the tail of another stripe than the first, where the tail is that long
            if stage + 64 * st + 7 < size:
                B.island("claim", "taken_in_tail_stripe_%d" % st, big(stage + 64 * st + 7), queries=[blocker, dict(d=0)], nc=size)
    # the claimed candidate in another stripe than the first (four waves: the claim is written by wave 0 and read by the wave of that stripe)
    for st in (1, 2, 3):
        if 64 * st + 10 <= size:
            B.island("claim", "taken_in_stripe_%d" % st, [dict(cast[0], j=64 * st + 7), dict(cast[1], j=3), dict(cast[2], j=40)], queries=[blocker, dict(d=0)], nc=64 * st + 10)
    if 64 * 3 + 10 <= size:
        B.island("claim", "chain_over_the_stripes", [dict(cast[0], j=64 + 7), dict(cast[1], j=128 + 9), dict(cast[2], j=192 + 1)],
                 queries=[blocker, dict(d=19), dict(d=0)], nc=64 * 3 + 10)
    B.island("claim", "chain_of_three", cast, queries=[blocker, dict(d=19), dict(d=0)])                    # a and b go: the probe is left c alone
    # the first query's match goes to the rotation filter (180 degrees: a bin of its own) and still hides the candidate
    B.island("claim", "taken_then_filtered", cast, queries=[dict(d=5, ang=180.0), dict(d=0)])
    # usable flags (bit 0): of the best candidate (mode 0 takes it, mode 1 skips it), of a query
    B.island("usable", "b_cleared_on_best", [dict(cast[0], flags=2), cast[1], cast[2]])
    if full:
        B.island("usable", "b_cleared_on_best_big", [dict(cast[0], flags=2, j=size - 1), dict(cast[1], j=0), dict(cast[2], j=64 % size)], nc=size)
    B.island("usable", "b_cleared_on_runner_up", [dict(d=rb, role="a"), dict(d=rs, role="b", flags=2)])     # mode 1: the runner-up is gone, accepted
    B.island("usable", "a_cleared_on_blocker", cast, queries=[dict(d=5, flags=2), dict(d=0)])
    B.island("usable", "a_cleared_on_probe", cast, queries=[dict(d=0, flags=2)])


@functools.lru_cache(None)
def bow_world(size, nnratio, th):
    B = _Builder("bow", size, th, nnratio, seed=size * 7 + int(nnratio * 100))
    _bow_groups(B)
    if not any(len(i) == size for i in B.b_items):       # (nothing of its own fills a node: the form comes from a node nobody asks)
        B.island("form", "ballast", [dict(d=256, role="x")], nc=size, far=0, queries=[dict(d=0, flags=2)])
    return B.finish(refused=getattr(B, "refused", None))


def bow_worlds():
    """[(name, world)]: every ratio of RATIOS (0.6 at th 30, the others at th 50) and the tie ratio, at every size of form_sizes()."""
    out = []
    for key, size in form_sizes().items():
        for r in RATIOS + (TIE_RATIO,):
            th = 30 if r == RATIOS[0] else 50
            out.append(("bow_%s_%g_th%d" % (key, r, th), bow_world(size, r, th)))
    return out


# ------------------------------------------------------------------------------------------------ rotation populations
class _RotationAdapter:
    """What search_boundary_worlds._rotation needs of a builder (group, island with one candidate and one probe angle), onto _Builder:
    every micro-island is a node of its own -- the histogram is filled by atomics of as many workgroups."""

    def __init__(self, B):
        self.B, self.th, self.kinds = B, B.th, []

    def group(self, kind, paired=True):
        self.kinds.append(kind)
        return len(self.kinds) - 1

    def island(self, kind, g, side, cands, probe=None, **_):
        (d, role, extra), = cands
        self.B.island(kind, side, [dict(d=d, role=role, ang=extra["ang"])], probe=dict(ang=probe["ang"]))


@functools.lru_cache(None)
def rotation_world(population, size):
    B = _Builder("rotation", size, 50, 0.7, seed=size + POPULATIONS.index(population))
    R = _RotationAdapter(B)
    sbw._rotation(R, population)
    B.island("form", "ballast", [dict(d=256, role="x")], nc=size, far=0, queries=[dict(d=0, flags=2)])
    return B.finish(population=population, rot_half_exact=getattr(R, "rot_half_exact", 0))


def rotation_worlds():
    return [("rotation_%s_%s" % (p, key), rotation_world(p, size)) for key, size in form_sizes().items() for p in POPULATIONS]


# ------------------------------------------------------------------------------------------------ SearchForTriangulation (mode 2)
ROWS = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], f32)                   # epipolar lines = image rows: dsqr = (y2 - y1)^2
SLANT = np.array([1e-5, 0, 0.004, 0, 2e-5, -1, -0.004, 1, 0.3], f32)   # a general matrix: every term of the line and the numerator rounds
N_LEVELS, L_ZERO, L_FMA, L_FLOAT = 11, 8, 9, 10                      # pyramid levels 0 .. 7 and three whose sigma2 a case places


def tri_tables():
    sf = (f32(1.2) ** np.arange(N_LEVELS)).astype(f32)
    return sf, (sf * sf).astype(f32)


def _tri_groups(B, T):
    th, size = B.th, B.size
    sf, s2 = T["sf"], T["s2"]
    EX, EY = f32(T["ex"][0]), f32(T["ey"][0])
    Y1 = f32(100.0)
    mono, stereo = 1, 3
    ok = dict(x=130.0, y=Y1, flags=stereo)               # on the query's row, a stereo point: every gate passes
    q0 = dict(d=0, x=100.0, y=Y1, flags=stereo)
    for d, side in ((th - 1, "below"), (th, "at"), (th + 1, "above")):
        B.island("threshold", side, [dict(ok, d=d, role="a")], queries=[q0])
    # ---- dsqr against 3.84 * sigma2[octave]: one float of y2 either side
    la, lb, lc = bm.epipolar_line(ROWS, 100.0, Y1)
    for o in (0, 3, 7):
        passes = lambda y: bm.dsqr_passes(bm.epipolar_dsqr(la, lb, lc, 130.0, y)[0], s2[o])
        for sgn in (1, -1):
            inside, outside = cross(passes, Y1, f32(Y1 + sgn * 40.0))
            B.island("dsqr", "pass_o%d%+d" % (o, sgn), [dict(ok, d=10, role="a", y=inside, octave=o)], queries=[q0])
            B.island("dsqr", "reject_o%d%+d" % (o, sgn), [dict(ok, d=10, role="a", y=outside, octave=o)], queries=[q0])
    # dsqr == 0 against sigma2 == 0 (a level of the caller's table): the only exact equality `<` against `<=` has
    B.island("dsqr_equal", "zero_sigma_reject", [dict(ok, d=10, role="a", octave=L_ZERO)], queries=[q0])
    B.island("dsqr_equal", "unit_sigma_pass", [dict(ok, d=10, role="a", octave=0)], queries=[q0])
    # the float / double compare and the contracted numerator: cases found by T's search (tri_world), their sigma2 placed between the two values
    for key, lvl in (("float", L_FLOAT), ("fma", L_FMA)):
        c = T[key]
        B.island("dsqr_" + key, "at_placed_sigma", [dict(d=10, role="a", x=c["x2"], y=c["y2"], octave=lvl, cam=1, flags=stereo)],
                 queries=[dict(d=0, x=c["x1"], y=c["y1"], cam=1, flags=stereo)])
        B.island("dsqr_" + key, "at_unit_sigma", [dict(d=10, role="a", x=c["x2"], y=c["y2"], octave=0, cam=1, flags=stereo)],
                 queries=[dict(d=0, x=c["x1"], y=c["y1"], cam=1, flags=stereo)])
    # ---- the epipole gate: dex^2 + dey^2 against 100 * scale[octave], both monocular; the candidate sits on the query's row
    qm = lambda y: dict(d=0, x=100.0, y=y, flags=mono)
    y8 = f32(EY - f32(8.0))
    assert bm.epipole_rejects(EX, EY, f32(EX - f32(6.0)), y8, sf[0]) == (False, f32(100.0), f32(100.0))
    B.island("epipole", "equal_6_8_pass", [dict(d=10, role="a", x=f32(EX - f32(6.0)), y=y8, flags=mono, octave=0)], queries=[qm(y8)])
    for o in (0, 3, 7):
        for sgn in (1, -1):
            rej = lambda x: bm.epipole_rejects(EX, EY, x, y8, sf[o])[0]
            inside, outside = cross(rej, EX, f32(EX + sgn * 60.0))
            B.island("epipole", "reject_o%d%+d" % (o, sgn), [dict(d=10, role="a", x=inside, y=y8, flags=mono, octave=o)], queries=[qm(y8)])
            B.island("epipole", "pass_o%d%+d" % (o, sgn), [dict(d=10, role="a", x=outside, y=y8, flags=mono, octave=o)], queries=[qm(y8)])
    for fq, nq in ((mono, "mono"), (stereo, "stereo")):
        for fc, ncn in ((mono, "mono"), (stereo, "stereo")):
            for x, where in ((f32(EX + f32(1.0)), "inside"), (f32(EX + f32(50.0)), "outside")):
                B.island("epipole_flags", "%s_%s_%s" % (nq, ncn, where), [dict(d=10, role="a", x=x, y=EY, flags=fc)], queries=[dict(d=0, x=100.0, y=EY, flags=fq)])
    # ---- den == 0 (camera 2: an all-zero F12), camera mismatch, usable flags
    B.island("den", "zero", [dict(ok, d=10, role="a", cam=2)], queries=[dict(q0, cam=2)])
    B.island("den", "rows", [dict(ok, d=10, role="a", cam=0)], queries=[q0])
    B.island("camera", "other_is_nearer", [dict(ok, d=5, role="a", cam=3), dict(ok, d=20, role="b")], queries=[q0])
    B.island("camera", "same", [dict(ok, d=5, role="a"), dict(ok, d=20, role="b")], queries=[q0])
    B.island("camera", "only_other", [dict(ok, d=5, role="a", cam=3)], queries=[q0])
    B.island("usable", "b_cleared_on_best", [dict(ok, d=5, role="a", flags=2), dict(ok, d=20, role="b")], queries=[q0])
    B.island("usable", "a_cleared", [dict(ok, d=5, role="a")], queries=[dict(q0, flags=2)])
    # ---- equal distances: the LAST candidate that passes the gates wins; a nearer one that fails hides nothing
    bad = dict(ok, y=f32(Y1 + f32(40.0)))                # 40 rows off: fails dsqr at every level
    B.island("ties", "two_equal", [dict(ok, d=10, role="a"), dict(ok, d=10, role="b")], queries=[q0])
    B.island("ties", "three_equal", [dict(ok, d=10, role="a"), dict(ok, d=10, role="b"), dict(ok, d=10, role="c")], queries=[q0])
    B.island("ties", "later_equal_fails", [dict(ok, d=10, role="a"), dict(bad, d=10, role="b")], queries=[q0])
    B.island("ties", "later_nearer_fails", [dict(ok, d=10, role="a"), dict(bad, d=5, role="b")], queries=[q0])
    B.island("ties", "earlier_nearer_fails", [dict(bad, d=5, role="a"), dict(ok, d=10, role="b")], queries=[q0])
    B.island("ties", "nearer_fails_epipole", [dict(d=5, role="a", x=f32(EX + f32(1.0)), y=EY, flags=mono), dict(d=10, role="b", x=f32(EX + f32(50.0)), y=EY, flags=mono)],
             queries=[dict(d=0, x=100.0, y=EY, flags=mono)])
    for name, p in placements(size, 1, B.lds).items():   # (mode 2: every wave takes whole queries -- a lane sees j, j + 64, ...)
        cands = [dict(ok, d=10, role="a", j=p["b"]), dict(ok, d=10, role="b", j=p["s"])]
        if "t" in p:
            cands.append(dict(bad, d=10, role="c", j=p["t"]))
        B.island("tie_placement", name, cands, queries=[q0], nc=size)
    # four queries of one node (with four waves: one per wave), the 64th and 65th too
    B.island("queries", "five_in_a_node", [dict(ok, d=10, role="a"), dict(ok, d=12, role="b")], queries=[dict(q0, d=k) for k in (4, 3, 2, 1, 0)])
    B.island("queries", "across_the_block", [dict(ok, d=10, role="a", j=size - 1), dict(ok, d=10, role="b", j=0)], queries=[dict(q0, d=k % 9) for k in range(66)] + [q0], nc=size)


def _find_float_double_case():
    """A pair under SLANT whose dsqr is a float D, and a sigma2 with D < 3.84 * sigma2 in double but not in float."""
    rng = np.random.default_rng(5)
    for _ in range(4000):
        x1, y1, x2 = (f32(v) for v in rng.uniform(50, 500, 3))
        la, lb, lc = bm.epipolar_line(SLANT, x1, y1)
        y_on = f32(-(float(la) * float(x2) + float(lc)) / float(lb))
        y2 = f32(y_on + f32(rng.uniform(1.0, 3.0)))
        D, _ = bm.epipolar_dsqr(la, lb, lc, x2, y2)
        if D is None or not 0.5 < D < 50:
            continue
        s_rej, s_ok = cross(lambda s: not bm.dsqr_passes(D, s), f32(D / 8), f32(D))
        if not bm.dsqr_passes(D, s_ok, ("dsqr_float",)):
            return dict(x1=x1, y1=y1, x2=x2, y2=y2, sigma2=s_ok, dsqr=D)
    raise AssertionError("no pair on which the float and the double compare decide differently")


def _find_fma_case():
    """A pair under SLANT whose numerator rounds differently when a * x2 + b * y2 is contracted, and a sigma2 between the two dsqr."""
    rng = np.random.default_rng(6)
    for _ in range(4000):
        x1, y1, x2 = (f32(v) for v in rng.uniform(50, 500, 3))
        la, lb, lc = bm.epipolar_line(SLANT, x1, y1)
        y_on = f32(-(float(la) * float(x2) + float(lc)) / float(lb))
        y2 = f32(y_on + f32(rng.uniform(1.0, 3.0)))
        D, _ = bm.epipolar_dsqr(la, lb, lc, x2, y2)
        Df, _ = bm.epipolar_dsqr(la, lb, lc, x2, y2, ("num_fma",))
        if D is None or D == Df or not 0.5 < D < 50:
            continue
        for s in cross(lambda s: not bm.dsqr_passes(D, s), f32(D / 8), f32(D)):
            if bm.dsqr_passes(D, s) != bm.dsqr_passes(Df, s):
                return dict(x1=x1, y1=y1, x2=x2, y2=y2, sigma2=s, dsqr=D, dsqr_fma=Df)
    raise AssertionError("no pair whose contracted numerator decides differently")


@functools.lru_cache(None)
def tri_params():
    sf, s2 = tri_tables()
    fd, fma = _find_float_double_case(), _find_fma_case()
    s2 = s2.copy(); s2[L_ZERO] = 0.0; s2[L_FLOAT] = fd["sigma2"]; s2[L_FMA] = fma["sigma2"]
    F12 = np.stack([ROWS, SLANT, np.zeros(9, f32), ROWS])
    return dict(F12=F12, ex=np.array([300.0, -50.0, 300.0, 300.0], f32), ey=np.array([200.0, 240.0, 200.0, 200.0], f32), sf=sf, s2=s2, float=fd, fma=fma)


@functools.lru_cache(None)
def tri_world(size, th=50):
    T = tri_params()
    B = _Builder("tri", size, th, 0.0, seed=size * 3 + 1)
    _tri_groups(B, T)
    return B.finish(tri=T)


def tri_worlds():
    return [("tri_%s" % key, tri_world(size)) for key, size in form_sizes().items()]


# ------------------------------------------------------------------------------------------------ answers
def run(fn_bow, fn_tri, w, mode, check_ori=True, a=None, b=None):
    """One search of world w in `mode` through search functions of the oracle's signatures -> (nmatches, match)."""
    a = w["a"] if a is None else a; b = w["b"] if b is None else b
    if mode == 2:
        T = w.get("tri") or tri_params()
        return fn_tri(a, b, T["F12"], T["ex"], T["ey"], T["sf"], T["s2"], w["th"], check_ori)
    return fn_bow(a, b, mode, w["th"], w["nnratio"], check_ori)


def answers(w, mode, match):
    """Per island: the roles its queries got, in the node's order ("" nothing, "?" a filler) -- of the probe last."""
    match = np.asarray(match)
    if mode == 0:
        got = np.full(len(w["a"]["desc"]), -1, np.int64)
        for g in np.flatnonzero(match >= 0):
            got[match[g]] = g
    else:
        got = match
    role = lambda g: "" if g < 0 else (w["role_b"][g] or "?")
    return [[role(got[q]) for q in isl["queries"]] for isl in w["islands"]]


def kinds_of_differences(w, mode, got, expected):
    """Groups (with sides) of the islands that own a differing match word."""
    bad = np.flatnonzero(np.asarray(got) != np.asarray(expected))
    owner = w["owner_b"] if mode == 0 else w["owner_a"]
    return sorted({"%s[%s]" % (w["islands"][owner[g]]["group"], w["islands"][owner[g]]["side"]) for g in bad})
