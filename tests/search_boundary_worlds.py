"""Boundary worlds of the projection searches: frames, queries, second windows and occupied flags whose every case sits on a decision
of the oracle's search loops (oracle/orb_oracle.cpp: features_in_area, orc_search_by_projection_frames / _points / _loop2,
orc_project_best, three_maxima), both sides of it.

Every case is an ISLAND: a handful of features and queries in grid cells of their own, farther from every other island than any of
its windows reaches, so that what one island decides depends on nothing else in the world.  A decision comes as a GROUP of islands
that differ in one quantity only (below / at / above a threshold, one ulp inside / on a window's edge, ...); the probe query of each
member carries the group's number, and `paired[group]` says whether the members must get different answers from the oracle
(tests/test_search_boundary_worlds.py checks that against the oracle alone, before any device sees the world).

Boundary values are computed here in float32 arithmetic, the oracle's operation order restated, and found by bisection over the float
bit patterns (as frustum_worlds.bisect_field does) -- none is typed in.  Descriptor distances are exact by construction: a candidate's
descriptor is the island's base descriptor with its first d bits flipped.

This is input generation only: what is expected of a device comes from the oracle."""
import numpy as np
import helpers

f32 = np.float32
GRID_COLS, GRID_ROWS, HISTO_LENGTH = 64, 48, 30       # Frame.h:37-38, ORBmatcher.cc:39
RESOLVE_K = 6                                         # csrc/matcher_internal.h: the shortlist k_project keeps per query
FIRST_CAP = 64                                        # csrc/search.hip search_common: first capacity of a candidate list
RATIOS = (0.6, 0.7, 0.75, 0.8, 0.9)
# rotation populations (frame search, orientation check on): which bins the ballast fills, and what sits on their edges
POPULATIONS = ("edges_a", "edges_b", "wrap", "ten_one_one", "eleven_one_one", "two_equal", "three_equal", "four_equal", "empty")
LEVEL_K = 3


def inv_sigma2_table(n=8):
    return (1.0 / (f32(1.2) ** np.arange(n)) ** 2).astype(f32)


# ------------------------------------------------------------------------------------------------ float32 helpers
def _key(v):
    """float32 -> integer that orders like the float (bisection over bit patterns across zero)."""
    b = int(np.asarray(v, f32).view(np.uint32))
    return b if b < 0x80000000 else -(b & 0x7fffffff) - 1


def _unkey(k):
    b = k if k >= 0 else ((-(k + 1)) | 0x80000000)
    return np.array([b], np.uint32).view(f32)[0]


def cross(pred, a, b):
    """pred(a) holds, pred(b) does not: bisect the float32 bit patterns between them -> (last value where it holds, its neighbour
    where it does not), one ulp apart."""
    a = f32(a); b = f32(b)
    assert pred(a) and not pred(b), (a, b)
    lo, hi = _key(a), _key(b)
    while abs(hi - lo) > 1:
        mid = lo + (hi - lo) // 2
        if pred(_unkey(mid)):
            lo = mid
        else:
            hi = mid
    x, y = _unkey(lo), _unkey(hi)
    assert y == np.nextafter(x, y) or (x == 0 and y == 0)
    return x, y


def round_half_away(v):
    """std::round / roundf of a float."""
    v = float(v)
    return int(np.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def rot_of(q_angle, f_angle):
    """rot as the searches compute it (float subtraction, `rot < 0.0` -> += 360.0f)."""
    rot = f32(f32(q_angle) - f32(f_angle))
    if rot < 0.0:
        rot = f32(rot + f32(360.0))
    return rot


def rot_bin(rot, rnd=round_half_away):
    b = rnd(f32(rot * f32(f32(1.0) / f32(HISTO_LENGTH))))
    return 0 if b == HISTO_LENGTH else b


def ratio_rejects(best, second, nnratio, double=False):
    """(float)best > nnratio * (float)second, nnratio a float; `double`: the wrong rule that widens the product."""
    if double:
        return float(best) > float(f32(nnratio)) * float(second)
    return bool(f32(best) > f32(f32(nnratio) * f32(second)))


def ratio_pairs(nnratio, th):
    """-> (edges, differ): edges = [(largest accepted best, second)] for a few seconds; differ = pairs within the threshold that the
    float compare accepts and a double compare rejects (or the other way round)."""
    edges = []
    for second in (10, 20, 50, 110, 140):
        acc = [b for b in range(1, min(second, th) + 1) if not ratio_rejects(b, second, nnratio)]
        if acc and acc[-1] + 1 <= th and acc[-1] + 1 <= second:
            edges.append((acc[-1], second))
    differ = [(b, s) for s in range(1, 257) for b in range(1, min(s, th) + 1)
              if ratio_rejects(b, s, nnratio) != ratio_rejects(b, s, nnratio, True)]
    return edges, differ


class Grid:
    """Bounds -> cells, with the oracle's float operations (make_view, build_grid, features_in_area)."""

    def __init__(self, bounds):
        self.minX, self.minY, self.maxX, self.maxY = (f32(b) for b in bounds)
        self.invW = f32(f32(GRID_COLS) / f32(self.maxX - self.minX))
        self.invH = f32(f32(GRID_ROWS) / f32(self.maxY - self.minY))

    def px(self, cx):
        return f32(self.minX + f32(f32(cx) / self.invW))

    def py(self, cy):
        return f32(self.minY + f32(f32(cy) / self.invH))

    def posx(self, x):
        return f32(f32(f32(x) - self.minX) * self.invW)

    def posy(self, y):
        return f32(f32(f32(y) - self.minY) * self.invH)

    def edgex(self, x, r, sign):
        """(x - minX -/+ r) * invW"""
        t = f32(f32(x) - self.minX)
        return f32((f32(t - f32(r)) if sign < 0 else f32(t + f32(r))) * self.invW)


# ------------------------------------------------------------------------------------------------ the builder
class _Builder:
    def __init__(self, search, bounds, n_cams, seed):
        from multi_orb_slam_amd._lib import QUERY_DTYPE, WINDOW_DTYPE
        self.search = search; self.G = Grid(bounds); self.bounds = tuple(float(f32(b)) for b in bounds)
        self.n_cams = n_cams
        self.rng = np.random.default_rng(seed)
        self.feats = [[] for _ in range(n_cams)]        # per camera: dict(x, y, oct, ang, ur, desc, role, occ)
        self.qs = []; self.w2 = []; self.kinds = []; self.groups = []; self.sides = []
        self.paired = []; self.group_kind = []
        self.QD, self.WD = QUERY_DTYPE, WINDOW_DTYPE
        cams = [0] if search == "points" else list(range(min(n_cams, 2)))
        self._small = [(c, cx, cy) for cy in range(2, 23, 2) for cx in range(2, 61, 2) for c in cams]
        self._large = [(c, cx, cy) for cy in (28, 32) for cx in (4, 10, 16, 22, 28, 34) for c in cams]
        self._huge = [(c, cx, 28) for cx in (44, 56) for c in cams]
        self.dropped = 0                                # islands a filter left out: none can be, and the tests assert it
        self.level_lo, self.level_hi = (-1, 0) if search == "loop2" else (-1, -1)

    # -- placement
    def slot(self, size="small", cam=None):
        pool = {"small": self._small, "large": self._large, "huge": self._huge}[size]
        for k, s in enumerate(pool):
            if cam is None or s[0] == cam:
                c, cx, cy = pool.pop(k)
                return c, self.G.px(cx), self.G.py(cy), cx, cy
        raise AssertionError("no %s slot left in the %s world" % (size, self.search))

    def desc(self, base, d):
        """`base` with its first d bits flipped: Hamming distance exactly d from it, |i - j| between two of them."""
        out = base.copy()
        full, rest = divmod(int(d), 8)
        out[:full] ^= 0xFF
        if rest:
            out[full] ^= np.uint8((1 << rest) - 1)
        return out

    def base(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def feat(self, cam, x, y, desc, role, octave=0, ang=0.0, ur=-1.0, occ=False):
        self.feats[cam].append(dict(x=f32(x), y=f32(y), oct=int(octave), ang=f32(ang), ur=f32(ur), desc=desc, role=role, occ=bool(occ)))

    def group(self, kind, paired=True):
        self.paired.append(paired); self.group_kind.append(kind)
        return len(self.paired) - 1

    def query(self, kind, cam, u, v, r, desc, group=-1, side="", ur=np.nan, lo=None, hi=None, blocks=1, ang=0.0, win2=None):
        q = np.zeros(1, self.QD)[0]
        q["u"] = u; q["v"] = v; q["radius"] = r; q["ur"] = ur
        q["min_level"] = self.level_lo if lo is None else lo; q["max_level"] = self.level_hi if hi is None else hi
        q["cam"] = cam; q["blocks"] = blocks; q["angle"] = ang; q["desc"] = desc
        w = np.zeros(1, self.WD)[0]
        w["cam"] = -1
        if win2 is not None:
            w["cam"], w["u"], w["v"], w["radius"], w["min_level"], w["max_level"] = win2
        self.qs.append(q); self.w2.append(w); self.kinds.append(kind); self.groups.append(group); self.sides.append(side)
        return len(self.qs) - 1

    # -- the simplest island: candidates (distance, role[, dict of feature fields]) around one centre, blockers, one probe
    def island(self, kind, group, side, cands, size="small", r=1.0, blockers=(), probe=None, cam=None, offsets=None):
        c, x0, y0, cx, cy = self.slot(size, cam)
        D = self.base()
        for k, cd in enumerate(cands):
            d, role = cd[0], cd[1]
            extra = dict(cd[2]) if len(cd) > 2 else {}
            if self.search == "loop2" and not kind.startswith("level"):
                extra.pop("octave", None)                # (no ratio test to keep out of a tie there, and a level gate of two octaves)
            dx, dy = offsets[k] if offsets else (f32(0.125) * (k % 5), f32(0.125) * (k // 5))
            self.feat(c, f32(x0 + f32(dx)), f32(y0 + f32(dy)), self.desc(D, d), role, **extra)
        for d, blocks in blockers:                       # earlier queries whose descriptor IS candidate d's: they take it at distance 0
            if self.search == "loop2" and not blocks:    # (the loop search has no such flag -- every match hides its feature: no claim instead)
                continue
            self.query(kind + ":blocker", c, x0, y0, r, self.desc(D, d), blocks=blocks)
        kw = dict(probe or {})
        return self.query(kind, c, kw.pop("u", x0), kw.pop("v", y0), kw.pop("r", r), D, group, side, **kw), (c, x0, y0, cx, cy)


O1, O2 = dict(octave=1), dict(octave=2)       # candidates that tie carry different octaves: the ratio test of the points form (equal
                                              # levels only) then leaves the tie to the visiting order, as the other searches do


def _threshold(B, th):
    g = B.group("threshold")
    for d, side in ((th - 1, "below"), (th, "at"), (th + 1, "above")):
        B.island("threshold", g, side, [(d, "a")])
    # the first candidate in visiting order lies over the threshold, the one behind it under it
    g = B.group("threshold_second")
    B.island("threshold_second", g, "under", [(th + 1, "a"), (th - 1, "b", O1)])
    B.island("threshold_second", g, "over", [(th + 1, "a"), (th + 1, "b", O1)])
    B.island("threshold_second", g, "at", [(th + 1, "a"), (th, "b", O1)])
    # short_th: the only candidates under the threshold are all claimed
    g = B.group("short_th")
    B.island("short_th", g, "claimed", [(5, "a"), (7, "b"), (th + 1, "c")], blockers=[(5, 1), (7, 1)])
    B.island("short_th", g, "open", [(5, "a"), (7, "b"), (th + 1, "c")], blockers=[(5, 1), (7, 0)])


def _ties(B):
    g = B.group("tie_cell")                              # same cell: ascending index decides
    B.island("tie_cell", g, "equal", [(10, "a"), (10, "b", O1)])
    B.island("tie_cell", g, "second", [(10, "a"), (9, "b", O1)])
    B.island("tie_cell", g, "equal3", [(10, "a"), (10, "b", O1), (10, "c", O2)])
    B.island("tie_cell", g, "third", [(10, "a"), (10, "b", O1), (9, "c", O2)])
    # different cells: the visiting order is column-major (ix outer, iy inner); the features are added against it
    cw = f32(1.0) / B.G.invW; ch = f32(1.0) / B.G.invH
    r = f32(1.3) * max(cw, ch)
    off3 = [(cw, 0), (0, ch), (0, 0)]                    # a: next column; b: next row of the same column; c: the centre's cell
    g = B.group("tie_cells")
    B.island("tie_cells", g, "equal3", [(10, "a"), (10, "b", O1), (10, "c", O2)], "large", r, offsets=off3)      # c, visited first
    B.island("tie_cells", g, "equal2", [(10, "a"), (10, "b", O1), (11, "c", O2)], "large", r, offsets=off3)      # b: its column comes first
    B.island("tie_cells", g, "last", [(9, "a"), (10, "b", O1), (10, "c", O2)], "large", r, offsets=off3)         # a, strictly nearer


def _occupancy(B):
    g = B.group("occupied")
    B.island("occupied", g, "occupied", [(5, "a", dict(occ=True)), (20, "b")])
    B.island("occupied", g, "free", [(5, "a"), (20, "b")])
    if B.search == "best":                               # (no claims there: every point on its own)
        return
    g = B.group("claimed")
    B.island("claimed", g, "blocking", [(5, "a"), (20, "b")], blockers=[(5, 1)])
    if B.search != "loop2":                              # (the two-window search has no such flag: every match hides its feature)
        B.island("claimed", g, "overwritten", [(5, "a"), (20, "b")], blockers=[(5, 0)])
    B.island("claimed", g, "unclaimed", [(5, "a"), (20, "b")])


def _shortlist(B, th):
    far = min(20, th)
    cands = [(d, "f%d" % d) for d in range(1, RESOLVE_K + 1)]
    blk = [(d, 1) for d in range(1, RESOLVE_K + 1)]
    g = B.group("shortlist")
    B.island("shortlist", g, "k", cands, blockers=blk)                                    # exactly RESOLVE_K eligible, all claimed
    B.island("shortlist", g, "k+1", cands + [(far, "seventh")], blockers=blk)             # ... and a seventh behind them: a rescan
    B.island("shortlist", g, "k+1_open", cands + [(far, "seventh")], blockers=blk[:-1] + [(RESOLVE_K, 0)])
    B.island("shortlist", g, "k+1_at_th", cands + [(th, "seventh")], blockers=blk)        # the rescan's own compare with the threshold
    B.island("shortlist", g, "k+1_over_th", cands + [(th + 1, "seventh")], blockers=blk)
    # candidate lists around the first capacity and around the retry that rounds up to a multiple of 64: the winner is the LAST entry
    g = B.group("capacity")
    for n in (FIRST_CAP - 1, FIRST_CAP, FIRST_CAP + 1, 2 * FIRST_CAP, 2 * FIRST_CAP + 1):
        zero = [(0, 0)] * n
        B.island("capacity", g, "last_%d" % n, [(30, "first")] + [(30, "mid")] * (n - 2) + [(10, "last")], offsets=zero)
        B.island("capacity", g, "first_%d" % n, [(30, "first")] + [(30, "mid")] * (n - 2) + [(30, "last")], offsets=zero)


def _levels(B):
    k = LEVEL_K
    if B.search == "loop2":                              # the inclusive [lo, hi] gate of :704-707 (hi = the predicted level >= 0)
        g = B.group("level2")
        for lo, hi, side in ((k, k - 1, "lo>hi"), (k - 1, k, "lo<hi"), (k, k, "lo==hi")):
            for o in (k - 1, k, k + 1):
                B.island("level2", g, "%s_o%d" % (side, o), [(5, "a", dict(octave=o))], probe=dict(lo=lo, hi=hi))
        return
    for lo in (-1, 0, 1, k):
        for hi in (-1, 0, k):
            g = B.group("level", paired=not ((lo <= 0 and hi < 0) or (lo >= 1 and hi == 0)))   # (no check at all / nothing passes)
            for o in (0, k - 1, k, k + 1):
                B.island("level", g, "min%d_max%d_o%d" % (lo, hi, o), [(5, "a", dict(octave=o))], probe=dict(lo=lo, hi=hi))


def _window(B):
    G = B.G
    one = f32(1.0)
    far_up, far_down = f32(1e9), f32(-1e9)
    cw = f32(1.0) / G.invW; ch = f32(1.0) / G.invH
    for axis in ("x", "y"):
        for sgn in (1, -1):
            g = B.group("window_edge")
            for side in ("inside", "on"):
                for attempt in range(8):                 # (a centre next to a power of two has no float exactly r away: the next slot)
                    cc, x0, y0, _, _ = B.slot("small")
                    c0 = x0 if axis == "x" else y0
                    # |f - c0| < r in float: the last coordinate inside, and its neighbour, where the difference is exactly r
                    inside, on = cross(lambda f: abs(f32(f - c0)) < one, c0, f32(c0 + sgn * f32(2.0)))
                    if abs(f32(on - c0)) == one:
                        break
                assert abs(f32(on - c0)) == one and abs(f32(inside - c0)) < one
                f = inside if side == "inside" else on
                D = B.base()
                B.feat(cc, f if axis == "x" else x0, f if axis == "y" else y0, B.desc(D, 5), "a")
                B.query("window_edge", cc, x0, y0, one, D, g, "%s_%s%+d" % (side, axis, sgn))
    # r = 0 against the smallest positive radius, the feature exactly at the centre
    g = B.group("window_r0")
    B.island("window_r0", g, "zero", [(5, "a")], probe=dict(r=f32(0.0)))
    B.island("window_r0", g, "tiny", [(5, "a")], probe=dict(r=np.nextafter(f32(0), f32(1))))
    # query centres whose (x - minX -/+ r) * invW is an exact integer, and their neighbours one ulp either side: the floor / ceil of the
    # cell range.  Under the right rule all of them find the feature just inside that edge (unpaired: only wrong arithmetic differs).
    g = B.group("window_cells", paired=False)
    B.cells_exact = 0
    for sgn in (-1, 1):
        cc, x0, y0, cx, cy = B.slot("large")
        k = cx - 1 if sgn < 0 else cx + 1
        for j in range(200):                             # about one cell: the edge lands on an integer next to the neighbouring cell's centre
            r = f32(cw * f32(1.0 + 0.001 * j))           # (not every radius has a centre whose product is that integer exactly: the next one)
            pred = (lambda x: G.edgex(x, r, -1) < k) if sgn < 0 else (lambda x: G.edgex(x, r, 1) <= k)
            below, above = cross(pred, f32(x0 - 4), f32(x0 + 4))
            near = [below, above]
            for _ in range(6):
                near = [np.nextafter(near[0], far_down)] + near + [np.nextafter(near[-1], far_up)]
            exact = [x for x in near if G.edgex(x, r, sgn) == k]
            if exact:
                break
        assert exact, "no centre puts the window's edge on cell %d exactly" % k
        B.cells_exact += len(exact)
        xs = [np.nextafter(exact[0], far_down), exact[0], np.nextafter(exact[-1], far_up)]
        assert G.edgex(xs[0], r, sgn) < k < G.edgex(xs[2], r, sgn)
        fx = f32(x0 + sgn * f32(0.97) * r)               # just inside the edge in question for all three centres
        for x, side in zip(xs, ("below", "exact", "above")):
            assert abs(f32(fx - x)) < r
            D = B.base()
            B.feat(cc, fx, y0, B.desc(D, 5), "a")
            B.query("window_cells", cc, x, y0, r, D, g, "%s%+d" % (side, sgn))
    # the round() of the insertion: a feature whose (x - minX) * invW crosses k + 0.5 changes column, and with it the visiting order:
    # `a` (lower index) and `b` tie; b sits in cell k.  a in cell k as well -> a wins; a in column / row k + 1 -> b is visited first.
    B.half_exact = 0
    for axis in ("x", "y"):
        g = B.group("insert_round")
        pos = G.posx if axis == "x" else G.posy
        cell = cw if axis == "x" else ch
        for side in ("below", "at"):
            cc, x0, y0, cx, cy = B.slot("large")
            kc = cx if axis == "x" else cy
            c0 = x0 if axis == "x" else y0
            low, up = cross(lambda f: round_half_away(pos(f)) <= kc, c0, f32(c0 + cell))
            B.half_exact += int(pos(up) == f32(kc + 0.5))
            f = low if side == "below" else up
            D = B.base()
            B.feat(cc, f if axis == "x" else x0, f if axis == "y" else y0, B.desc(D, 10), "a")
            B.feat(cc, x0, y0, B.desc(D, 10), "b", **O1)
            B.query("insert_round", cc, x0, y0, f32(1.3) * cell, D, g, "%s_%s" % (side, axis))
    # ... and the feature that rounds into column 64 / row 48 and is never found
    for axis in ("x", "y"):
        g = B.group("insert_last")
        n = GRID_COLS if axis == "x" else GRID_ROWS
        pos = G.posx if axis == "x" else G.posy
        for side in ("kept", "lost"):
            if axis == "x":
                o0 = G.py(14 if side == "kept" else 18)
                kept, lost = cross(lambda f: round_half_away(pos(f)) < n, G.px(n - 1), G.px(n))
            else:
                o0 = G.px(62.5 if side == "kept" else 57)
                kept, lost = cross(lambda f: round_half_away(pos(f)) < n, G.py(n - 1), G.py(n))
            f = kept if side == "kept" else lost
            D = B.base()
            B.feat(0, f if axis == "x" else o0, f if axis == "y" else o0, B.desc(D, 5), "a")
            B.query("insert_last", 0, f if axis == "x" else o0, f if axis == "y" else o0, one, D, g, "%s_%s" % (side, axis))
    # windows partly and wholly outside the bounds, on each side; the feature sits just inside the bounds
    for name, fx, fy, dx, dy in (("left", G.px(0) + f32(0.5), G.py(26), -1, 0), ("right", G.px(63), G.py(26), 1, 0),
                                 ("top", G.px(30), G.py(0) + f32(0.5), 0, -1), ("bottom", G.px(60), G.py(47), 0, 1)):
        g = B.group("window_outside")
        for side, step in (("inside", 0.0), ("partly", 0.6), ("beyond", 1.5), ("wholly", 2.5 if name in ("left", "top") else 4.0)):
            D = B.base()                                 # (a feature and a descriptor base per query: nothing is shared but the place)
            B.feat(0, f32(fx), f32(fy), B.desc(D, 5), "a")
            B.query("window_outside", 0, f32(fx + f32(dx * step) * cw), f32(fy + f32(dy * step) * ch), cw if dx else ch, D, g,
                    "%s_%s" % (name, side))


def _huge(B):
    """A window of more than 64 cells: k_project takes its cells in chunks of 64.  The nearest candidate lies in the last column."""
    G = B.G
    cw = f32(1.0) / G.invW; ch = f32(1.0) / G.invH
    g = B.group("window_chunks")
    for side, da in (("last_chunk", 9), ("tie", 10)):
        c, x0, y0, cx, cy = B.slot("huge")
        r = f32(4.2) * max(cw, ch)
        ncells = (int(np.ceil(G.edgex(x0, r, 1))) - int(np.floor(G.edgex(x0, r, -1))) + 1) ** 2
        assert ncells > 64
        D = B.base()
        B.feat(c, f32(x0 + f32(3.9) * cw), f32(y0 + f32(3.9) * ch), B.desc(D, da), "a")     # last column, last row: the last chunk
        B.feat(c, f32(x0 - f32(3.9) * cw), f32(y0 - f32(3.9) * ch), B.desc(D, 10), "b", **O1)     # first column, first row
        B.feat(c, x0, y0, B.desc(D, 10), "c", **O2)
        B.query("window_chunks", c, x0, y0, r, D, g, side)


def _right_gate(B):
    one = f32(1.0); U = f32(50.0)
    g = B.group("right_edge")                            # |ur - uright| == r passes, one ulp more does not
    for sgn in (1, -1):
        ok, out = cross(lambda v: not (abs(f32(v - U)) > one), U, f32(U + sgn * f32(3.0)))
        assert abs(f32(ok - U)) == one
        B.island("right_edge", g, "on%+d" % sgn, [(5, "a", dict(ur=U))], probe=dict(ur=ok))
        B.island("right_edge", g, "out%+d" % sgn, [(5, "a", dict(ur=U))], probe=dict(ur=out))
    g = B.group("right_sign")                            # the gate reads `uright > 0`
    tiny = np.nextafter(f32(0), f32(1))
    for ur, side in ((f32(0.0), "zero"), (f32(-0.0), "minus_zero"), (f32(-1.0), "minus_one"), (tiny, "smallest_positive")):
        B.island("right_sign", g, side, [(5, "a", dict(ur=ur))], probe=dict(ur=f32(1000.0)))
    g = B.group("right_nan")                             # a NaN never closes the gate
    B.island("right_nan", g, "nan", [(5, "a", dict(ur=U))], probe=dict(ur=f32(np.nan)))
    B.island("right_nan", g, "far", [(5, "a", dict(ur=U))], probe=dict(ur=f32(1000.0)))


def chi2_value(ex, ey, er, sg, double=False):
    """e2 * inv_sigma2[level] as orc_project_best forms it: float sums of float squares, a FLOAT product (widened for the compare);
    `double`: the wrong rule that widens the factors first."""
    e2 = f32(f32(f32(ex) * f32(ex)) + f32(f32(ey) * f32(ey)))
    if er is not None:
        e2 = f32(e2 + f32(f32(er) * f32(er)))
    return float(e2) * float(sg) if double else float(f32(e2 * f32(sg)))


def _chi2(B):
    """Gate 2 of project_best: `e2 * inv_sigma2[level]`, a float product widened to double, against 7.8 (the feature has a right
    coordinate >= 0) and 5.99.  The level table is the caller's, so the crossing is placed with IT: for offsets whose squares are
    exact, bisect inv_sigma2 to the two neighbouring floats either side of the limit, and keep offsets on which a double product
    decides differently from the float product for one of the two (searched for here, asserted by the tests).  -> the table."""
    sg = inv_sigma2_table()
    B.float_double_chi2 = 0
    level = 1
    for limit, stereo in ((5.99, False), (7.8, True)):
        g = B.group("chi2_stereo" if stereo else "chi2_mono")
        er = f32(0.5) if stereo else None
        hits = []
        for kx in range(8, 41):
            for ky in range(0, 17, 2):
                ex, ey = f32(kx / 8.0), f32(ky / 8.0)
                e2 = chi2_value(ex, ey, er, 1.0)
                if not 1.0 < limit / e2 < 6.0:
                    continue
                ok, out = cross(lambda v: not (chi2_value(ex, ey, er, v) > limit), f32(0.9 * limit / e2), f32(1.1 * limit / e2))
                nd = sum((chi2_value(ex, ey, er, v) > limit) != (chi2_value(ex, ey, er, v, True) > limit) for v in (ok, out))
                if nd:
                    hits.append((ex, ey, ok, out))
        assert hits, "no offset on which the float and the double product decide differently"
        B.float_double_chi2 += len(hits)
        for ex, ey, ok, out in hits[:1]:
            for v, side in ((ok, "pass"), (out, "reject")):
                sg[level] = v
                c, x0, y0, _, _ = B.slot("small")
                fx, fy = f32(np.round(x0 * 8) / 8), f32(np.round(y0 * 8) / 8)          # (eighths: the offsets stay exact)
                assert f32(f32(fx + ex) - fx) == ex and f32(f32(fy + ey) - fy) == ey
                D = B.base()
                B.feat(c, fx, fy, B.desc(D, 5), "a", octave=level, ur=f32(50.0) if stereo else f32(-1.0))
                B.query("chi2", c, f32(fx + ex), f32(fy + ey), f32(8.0), D, g, "%s_%g" % (side, limit), ur=f32(50.5) if stereo else f32(0.0))
                level += 1
    # uright == 0 takes the stereo branch (`>= 0`): ex^2 = 6.5 passes 7.8 there and fails 5.99 in the other branch
    g = B.group("chi2_branch")
    ex = f32(np.sqrt(6.5))
    for ur, side in ((f32(0.0), "zero"), (f32(-0.0), "minus_zero"), (f32(-1.0), "minus_one"), (-np.nextafter(f32(0), f32(1)), "largest_negative")):
        c, x0, y0, _, _ = B.slot("small")
        D = B.base()
        B.feat(c, x0, y0, B.desc(D, 5), "a", ur=ur)
        B.query("chi2_branch", c, f32(x0 + ex), y0, f32(8.0), D, g, side, ur=f32(0.0))
    B.inv_sigma2 = sg


def _ratio(B, nnratio, th):
    edges, differ = ratio_pairs(nnratio, th)
    assert edges
    B.float_double_ratio = len(differ)
    picks = [(b, s, "edge") for b, s in edges] + [(b, s, "float_double") for b, s in differ[:1] + differ[len(differ) // 2:len(differ) // 2 + 1] + differ[-1:]]
    for b, s, why in picks:
        g = B.group("ratio_" + why)
        assert not ratio_rejects(b, s, nnratio)
        B.island("ratio", g, "accepted_%d_%d" % (b, s), [(b, "a"), (s, "b")])
        B.island("ratio", g, "accepted_rev_%d_%d" % (b, s), [(s, "b"), (b, "a")])            # the second is visited first
        if b + 1 <= min(th, s) and ratio_rejects(b + 1, s, nnratio):
            B.island("ratio", g, "rejected_%d_%d" % (b + 1, s), [(b + 1, "a"), (s, "b")])
            B.island("ratio", g, "rejected_rev_%d_%d" % (b + 1, s), [(s, "b"), (b + 1, "a")])
    b, s = edges[0]
    rej = (b + 1, s)
    g = B.group("ratio_levels")                          # the test applies only when bestLevel == bestLevel2
    B.island("ratio", g, "equal_levels", [(rej[0], "a", dict(octave=2)), (rej[1], "b", dict(octave=2))])
    B.island("ratio", g, "unequal_levels", [(rej[0], "a", dict(octave=2)), (rej[1], "b", dict(octave=3))])
    g = B.group("ratio_second_hidden")                   # a second neighbour that is occupied or claimed does not count
    B.island("ratio", g, "second_counts", [(rej[0], "a"), (rej[1], "b")])
    B.island("ratio", g, "second_occupied", [(rej[0], "a"), (rej[1], "b", dict(occ=True))])
    B.island("ratio", g, "second_claimed", [(rej[0], "a"), (rej[1], "b")], blockers=[(rej[1], 1)])
    B.island("ratio", g, "second_overwritable", [(rej[0], "a"), (rej[1], "b")], blockers=[(rej[1], 0)])
    g = B.group("ratio_single")                          # one candidate: best2 = 256, bestLevel2 = -1
    B.island("ratio", g, "single", [(rej[0], "a")])
    B.island("ratio", g, "two", [(rej[0], "a"), (rej[1], "b")])


def _loop2_windows(B):
    """Equal candidates across the two windows of a loop point: camera 1's are visited first, one strict `<` runs over both."""
    g = B.group("tie_windows")
    for side, d0, d1, first in (("equal", 10, 10, True), ("second_nearer", 10, 9, True), ("only_second", 10, 10, False)):
        c0, x0, y0, _, _ = B.slot("small", 0)
        c1, x1, y1, _, _ = B.slot("small", 1)
        D = B.base()
        B.feat(0, x0, y0, B.desc(D, d0), "a")
        B.feat(1, x1, y1, B.desc(D, d1), "b"); B.feat(1, f32(x1 + f32(0.25)), y1, B.desc(D, d1), "c")
        B.query("tie_windows", 0 if first else -1, x0, y0, f32(1.0), D, g, side, win2=(1, x1, y1, f32(1.0), -1, 0))


def _rotation(B, population):
    """One histogram population.  Micro-islands (one feature, one query, rot = query angle - feature angle): `ballast` fills bins at their
    centres, the boundary triples sit one ulp either side of 15 + 30 k.  -> nothing; the probes' sides name their bin."""
    def pair(kind, g, side, q_ang, f_ang, d=5):
        B.island(kind, g, side, [(d, "a", dict(ang=f_ang))], probe=dict(ang=q_ang))

    def ballast(bins_counts):
        for b, n in bins_counts:
            g = B.group("hist_bin", paired=False)
            for _ in range(n):
                pair("hist_ballast", g, "bin%d" % b, f32(30.0 * b), f32(0.0))

    def edge(k, wrap=False):
        g = B.group("rot_edge")
        mid = f32(15 + 30 * k)
        if not wrap:
            lo, up = cross(lambda a: rot_bin(rot_of(a, f32(0))) <= k, f32(mid - 5), f32(mid + 5))
            # (where rot * factor is exactly k + 0.5, roundf and round-to-even disagree: counted, the tests assert that some are)
            B.rot_half_exact = getattr(B, "rot_half_exact", 0) + int(f32(up * f32(f32(1.0) / f32(HISTO_LENGTH))) == f32(k + 0.5))
            vals = sorted(set(float(v) for v in (lo, up, mid, np.nextafter(mid, f32(0)), np.nextafter(mid, f32(1e9)))))
            for a in vals:
                a = f32(a)
                pair("rot_edge", g, "%s_%d_bin%d" % ("below" if a < mid else "at" if a == mid else "above", 15 + 30 * k, rot_bin(a)), a, f32(0.0))
        else:                                            # through the negative wrap: 0 - f_ang + 360
            up, lo = cross(lambda f: rot_bin(rot_of(f32(0), f)) > k, f32(360 - mid - 5), f32(360 - mid + 5))
            for f, side in ((lo, "below"), (up, "at_or_above")):
                assert rot_of(f32(0), f) > 0 and f32(f32(0) - f) < 0
                pair("rot_wrap", g, "%s_%d_bin%d" % (side, 15 + 30 * k, rot_bin(rot_of(f32(0), f))), f32(0.0), f)

    if population in ("edges_a", "edges_b"):
        first = 0 if population == "edges_a" else 6
        ballast([(first + 1, 12), (first + 3, 11), (first + 5, 10)])
        for k in range(first, first + 6):
            edge(k)
        edge(first, wrap=True); edge(first + 3, wrap=True)
    elif population == "wrap":
        ballast([(0, 12), (6, 11), (9, 10)])
        g = B.group("rot_zero")
        tiny = np.nextafter(f32(0), f32(1))
        pair("rot_zero", g, "plus_zero", f32(0.0), f32(0.0))                   # bin 0, kept
        pair("rot_zero", g, "minus_zero", f32(-0.0), f32(0.0))
        pair("rot_zero", g, "to_360", f32(0.0), tiny)                          # -tiny + 360 rounds to 360.0f: bin 12
        pair("rot_zero", g, "to_360_from_one", f32(1.0), np.nextafter(f32(1), f32(2)))
        assert rot_of(f32(0.0), tiny) == f32(360.0) and rot_bin(f32(360.0)) == 12
    elif population == "ten_one_one":
        ballast([(2, 10), (5, 1), (8, 1)])
    elif population == "eleven_one_one":
        ballast([(2, 11), (5, 1), (8, 1)])
    elif population == "two_equal":
        ballast([(2, 4), (5, 4), (8, 2), (10, 2)])
    elif population == "three_equal":
        ballast([(2, 3), (5, 3), (8, 3), (10, 1)])
    elif population == "four_equal":
        ballast([(2, 3), (5, 3), (8, 3), (10, 3)])
    elif population == "empty":
        g = B.group("hist_bin", paired=False)
        for _ in range(4):
            pair("hist_ballast", g, "unmatched", f32(0.0), f32(0.0), d=B.th + 1)
    else:
        raise ValueError(population)


SEARCHES = ("frames", "points", "loop2", "best")


def make_search_world(search, bounds, th=100, nnratio=0.8, population=None, fillers=(), filler_queries=0, seed=1, filler_th=3.0):
    """-> dict(fr, q, w2, occ, kinds, groups, sides, paired, group_kind, roles, n_island_queries, dropped, ...).

    search: "frames" (SearchByProjection between frames), "points" (the ratio-test form, camera 0 only), "loop2" (two windows),
    "best" (project_best, all gates).  population: one of POPULATIONS -- then the world holds that rotation-histogram population and
    nothing else (frame search); None: every other kind, all rotations 0 (the population "all matches in one bin").
    fillers: ordinary features per camera (helpers.make_frame_arrays) in the rows below the islands; filler_queries: ordinary queries
    (helpers.make_queries) onto them, appended behind the islands' queries.  In a population world the filler features' descriptors are
    all zeros and the filler queries' all ones: candidates, none of them ever accepted, so the population stays what its name says."""
    assert search in SEARCHES
    n_cams = max(2, len(fillers))
    B = _Builder(search, bounds, n_cams, seed)
    B.th = th
    if population is not None:
        assert search == "frames"
        _rotation(B, population)
    else:
        if search != "best":
            _threshold(B, th)
            _shortlist(B, th)
        _ties(B); _occupancy(B); _levels(B)
        if search == "loop2":
            _loop2_windows(B)
        if search != "loop2":
            _window(B); _huge(B); _right_gate(B)
        if search == "points":
            _ratio(B, nnratio, th)
        if search == "best":
            _chi2(B)
    n_island_q = len(B.qs)
    # ---- fillers: below the islands (rows 36 and up, columns up to 54), far from any island's window
    G = B.G
    fill = None
    if any(fillers):
        fw = float(G.px(54) - G.px(0)); fh = float(G.py(47) - G.py(36))
        fill = helpers.make_frame_arrays(list(fillers), fw - 20, fh - 20, seed + 500)
        fill["un_x"] = (fill["un_x"] + f32(10) + G.px(0)).astype(f32); fill["un_y"] = (fill["un_y"] + f32(10) + G.py(36)).astype(f32)
        fill["uright"] = np.where(fill["uright"] > 0, fill["uright"] + f32(10) + G.px(0), fill["uright"]).astype(f32)
        if population is not None:
            for d in fill["descs"]:
                d[:] = 0
    # ---- assemble, camera-major
    cols = dict(un_x=[], un_y=[], octave=[], angle=[], uright=[], cam_of=[], local_of=[])
    descs = []; roles = []; occ = []
    fill_global = []                                     # global index of every filler feature, in the filler frame's order
    for c in range(n_cams):
        fs = B.feats[c]
        nf = int(fillers[c]) if c < len(fillers) else 0
        sel = np.flatnonzero(fill["cam_of"] == c) if fill is not None else np.zeros(0, np.int64)
        assert len(sel) == nf
        base = sum(len(x) for x in cols["un_x"])
        cols["un_x"].append(np.concatenate([np.array([f["x"] for f in fs], f32), fill["un_x"][sel] if nf else np.zeros(0, f32)]))
        cols["un_y"].append(np.concatenate([np.array([f["y"] for f in fs], f32), fill["un_y"][sel] if nf else np.zeros(0, f32)]))
        cols["octave"].append(np.concatenate([np.array([f["oct"] for f in fs], np.int32), fill["octave"][sel] if nf else np.zeros(0, np.int32)]))
        cols["angle"].append(np.concatenate([np.array([f["ang"] for f in fs], f32), fill["angle"][sel] if nf else np.zeros(0, f32)]))
        cols["uright"].append(np.concatenate([np.array([f["ur"] for f in fs], f32), fill["uright"][sel] if nf else np.zeros(0, f32)]))
        n_c = len(fs) + nf
        cols["cam_of"].append(np.full(n_c, c, np.int32)); cols["local_of"].append(np.arange(n_c, dtype=np.int32))
        d = np.array([f["desc"] for f in fs], np.uint8).reshape(-1, 32)
        descs.append(np.ascontiguousarray(np.concatenate([d, fill["descs"][c]]) if nf else d))
        roles += [f["role"] for f in fs] + [""] * nf
        occ += [f["occ"] for f in fs] + [False] * nf
        fill_global.append(base + len(fs) + np.arange(nf))
    fr = {k: np.concatenate(v) for k, v in cols.items()}
    fr["descs"] = descs; fr["bounds"] = B.bounds
    q = np.array(B.qs, B.QD) if B.qs else np.zeros(0, B.QD)
    w2 = np.array(B.w2, B.WD) if B.w2 else np.zeros(0, B.WD)
    kinds = list(B.kinds); groups = list(B.groups); sides = list(B.sides)
    if filler_queries:
        assert fill is not None
        fq = helpers.make_queries(fill, filler_queries, seed + 600, th=filler_th, blocks=2)
        if search == "points":
            fq["u"] = np.where(fq["cam"] == 0, fq["u"], f32(-1.0e6))     # (camera 0 only: a query made from another camera's feature sees nothing)
            fq["cam"] = 0
        if search == "loop2":
            lvl = np.maximum(fq["max_level"], 0)
            fq["ur"] = np.nan; fq["blocks"] = 1; fq["min_level"] = lvl - 1; fq["max_level"] = lvl
        if population is not None:
            fq["desc"] = 255                             # (against all-zero filler features, below: distance 256 to every one of them)
        fw2 = np.zeros(filler_queries, B.WD); fw2["cam"] = -1
        q = np.concatenate([q, fq]); w2 = np.concatenate([w2, fw2])
        kinds += ["filler"] * filler_queries; groups += [-1] * filler_queries; sides += [""] * filler_queries
    occ = np.array(occ, np.uint8)
    return dict(fr=fr, q=np.ascontiguousarray(q), w2=np.ascontiguousarray(w2) if search == "loop2" else None, occ=occ, kinds=np.array(kinds),
                groups=np.array(groups, np.int64), sides=np.array(sides), paired=np.array(B.paired, bool), group_kind=np.array(B.group_kind),
                roles=np.array(roles), n_island_queries=n_island_q, dropped=B.dropped, search=search, th=th, nnratio=nnratio,
                population=population, float_double_ratio=getattr(B, "float_double_ratio", None),
                float_double_chi2=getattr(B, "float_double_chi2", None), half_exact=getattr(B, "half_exact", None),
                cells_exact=getattr(B, "cells_exact", None), rot_half_exact=getattr(B, "rot_half_exact", 0),
                inv_sigma2=getattr(B, "inv_sigma2", inv_sigma2_table()))


# ------------------------------------------------------------------------------------------------ answers, by query
def answers(world, match_of_feature, unfiltered=None):
    """What each query got, as the role of its feature inside its island: "" nothing, a role, or role + "/rejected" when the rotation
    histogram took the match back (`unfiltered`: match_of_feature of the same search without the orientation check)."""
    out = np.array([""] * len(world["q"]), dtype=object)
    src = match_of_feature if unfiltered is None else unfiltered
    for g in np.flatnonzero(src >= 0):
        out[src[g]] = world["roles"][g] + ("/rejected" if match_of_feature[g] == -2 else "")
    return out


def kinds_of_differences(world, got, expected):
    """Kinds (with sides) of the queries involved in a mismatch of two match_of_feature arrays: the owners on either side of every
    differing feature."""
    bad = np.flatnonzero(np.asarray(got) != np.asarray(expected))
    names = set()
    for g in bad:
        for owner in (got[g], expected[g]):
            if owner >= 0:
                names.add("%s[%s]" % (world["kinds"][owner], world["sides"][owner]))
        if got[g] < 0 and expected[g] < 0:
            names.add("feature %d (%s): %d vs %d" % (g, world["roles"][g], got[g], expected[g]))
    return sorted(names)
