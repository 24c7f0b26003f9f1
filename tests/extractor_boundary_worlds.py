"""Constructed inputs that sit ON the decision boundaries of the extractor's kernels, and a plain restatement of every operation they
exercise.  CPU only; imports neither the package nor the oracle (tests/test_extractor_boundary_worlds.py holds the oracle to this file,
tests/test_gpu_extractor_boundaries.py the kernels to both).

Plain reference: each operation straight from its published definition on NumPy integers -- FAST-9/16 score as "max over the 16 arcs of
the min over 9" (S+ and S-, minus 1), the reference's cell loop (src/ORBextractor.cc:766-830) with strict 8-neighbour maxima that see 0
outside the cell's scored rectangle, the intensity-centroid moments over the umax disc, the 7 x 7 sigma-2 blur in 8.8 fixed point with
BORDER_REFLECT_101, and OpenCV's 11-bit fixed-point bilinear resize.  Nothing here is shared with oracle/ or the kernels.

Worlds: small uint8 images with the parameter set they are meant for and, where a family places stamps, each stamp's stand-alone known
answer.  A stamp is a 7 x 7 patch on a flat canvas of the centre's value c: `n` contiguous ring pixels from ring index `start` on are
c + pol * d.  Alone, its centre scores d - 1 when n >= 9 and -1 when n == 8.  check_<family>() asserts on the CPU, from the plain
reference, that a family holds both sides of every boundary it names and that no stamp's answer was changed by anything else in its image.
"""
import functools
import numpy as np

# (dx, dy) of the Bresenham circle of radius 3, in the order cv::FAST walks it
RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1),
        (-2, 2), (-1, 3)]
EDGE = 19          # EDGE_THRESHOLD: first scored column / row of a level
BORDER = 16        # candidate coordinates are relative to (16, 16)
GAUSS = [18, 34, 49, 55, 49, 34, 18]   # getGaussianKernel(7, 2) in 8.8 fixed point: sums to 257


# ====================================================================================================================== plain reference
def plain_scores(level):
    """max(S+, S-) - 1 per pixel (int32; -1 on the 3-pixel rim, which has no ring): S+ = max over the 16 arcs of 9 contiguous ring pixels
    of min(c - r), S- the same of min(r - c).  A pixel is a corner at threshold t exactly when this is >= t."""
    a = np.asarray(level).astype(np.int32)
    h, w = a.shape
    S = np.full((h, w), -1, np.int32)
    if h < 7 or w < 7:
        return S
    c = a[3:h - 3, 3:w - 3]
    d = [c - a[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in RING]
    sp = np.full(c.shape, -256, np.int32)
    sm = np.full(c.shape, -256, np.int32)
    for k in range(16):
        lo_p = d[k]
        lo_m = -d[k]
        for i in range(1, 9):
            lo_p = np.minimum(lo_p, d[(k + i) % 16])
            lo_m = np.minimum(lo_m, -d[(k + i) % 16])
        sp = np.maximum(sp, lo_p)
        sm = np.maximum(sm, lo_m)
    S[3:h - 3, 3:w - 3] = np.maximum(sp, sm) - 1
    return S


def plain_cells(w, h):
    """The reference's cell grid (:774-807) as scored rectangles [(i, j, x0, y0, x1, y1)], cell-major, empty ones included (x1 <= x0:
    the cells the reference skips or hands to FAST less than seven pixels wide).  None when the level has no 30-pixel cell."""
    width, height = w - 2 * BORDER, h - 2 * BORDER
    ncols, nrows = width // 30, height // 30        # (int)(float / 30.f): exact for these magnitudes
    if ncols < 1 or nrows < 1:
        return None
    wc, hc = -(-width // ncols), -(-height // nrows)
    out = []
    for i in range(nrows):
        for j in range(ncols):
            x0, y0 = EDGE + j * wc, EDGE + i * hc
            out.append((i, j, x0, y0, min(x0 + wc, w - EDGE), min(y0 + hc, h - EDGE)))
    return out


def plain_cell_candidates(level, ini_th, min_th):
    """[(x - 16, y - 16, response)] in the order the reference hands them to DistributeOctTree: cells row by row, pixels row-major
    inside a cell; strict 8-neighbour maxima of the scores >= min_th inside the cell's scored rectangle (0 outside it); the maxima
    >= ini_th alone when the cell has any, all of them otherwise."""
    level = np.asarray(level)
    h, w = level.shape
    S = plain_scores(level)
    out = []
    for (_, _, x0, y0, x1, y1) in plain_cells(w, h):
        if x1 <= x0 or y1 <= y0:
            continue
        Z = np.zeros((y1 - y0 + 2, x1 - x0 + 2), np.int32)
        sc = S[y0:y1, x0:x1]
        Z[1:-1, 1:-1] = np.where(sc >= min_th, sc, 0)
        mid = Z[1:-1, 1:-1]
        is_max = mid > 0
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dx or dy:
                    is_max &= mid > Z[1 + dy:Z.shape[0] - 1 + dy, 1 + dx:Z.shape[1] - 1 + dx]
        ys, xs = np.nonzero(is_max)                 # row-major
        loc = [(int(x0 + x - BORDER), int(y0 + y - BORDER), int(mid[y, x])) for y, x in zip(ys, xs)]
        strong = [k for k in loc if k[2] >= ini_th]
        out += strong if strong else loc
    return out


def plain_quick_survivors(level, min_th):
    """The high-speed test every FAST implementation may run first (a necessary condition for a score >= min_th): with T = min_th + 1,
    every one of the four antipodal pairs (ring 0/8, 2/10, 4/12, 6/14) has a pixel darker than c by T, or every one a brighter one."""
    a = np.asarray(level).astype(np.int32)
    h, w = a.shape
    c = a[3:h - 3, 3:w - 3]
    d = [c - a[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in RING]
    T = min_th + 1
    bright = np.ones(c.shape, bool)
    dark = np.ones(c.shape, bool)
    for k in (0, 2, 4, 6):
        bright &= (d[k] >= T) | (d[k + 8] >= T)
        dark &= (d[k] <= -T) | (d[k + 8] <= -T)
    out = np.zeros((h, w), bool)
    out[3:h - 3, 3:w - 3] = bright | dark
    return out


def packed_quick_value(level, x, y, first_of_four):
    """What the byte-packed form of the same test compares with K = 256 min_th + 1 (it passes at >= K; 0 <= min_th <= 127): every ring
    pixel rides in the HIGH byte of a 16-bit lane whose low byte is the pixel to its left (0 for ring 12 of the first pixel of a group of
    four), the extrema over the pairs are unsigned 16-bit ones, and the centre is c << 8 on the bright side, c << 8 | 255 on the dark one:
    max(sat(C0 - A'), sat(B' - C1)).  The low bytes cost up to 255: a difference of exactly T passes with nothing to spare when the
    selected lane's low byte is 255 (bright side) or 0 (dark side).  check_arcs uses this to show that the junk worlds sit ON K."""
    a = np.asarray(level).astype(np.int64)
    lane = {}
    for k in range(0, 16, 2):
        dx, dy = RING[k]
        lane[k] = (a[y + dy, x + dx] << 8) | (0 if k == 12 and first_of_four else a[y + dy, x + dx - 1])
    A = max(min(lane[k], lane[k + 8]) for k in (0, 2, 4, 6))
    B = min(max(lane[k], lane[k + 8]) for k in (0, 2, 4, 6))
    c = int(a[y, x])
    return int(max(0, (c << 8) - A, B - ((c << 8) | 255)))


def plain_umax():
    """Half-widths of the orientation disc's rows (reference :452-470): round(sqrt(15^2 - v^2)) up to v = 11, the rest mirrored."""
    vmax = int(np.floor(15 * np.sqrt(2.0) / 2 + 1))
    vmin = int(np.ceil(15 * np.sqrt(2.0) / 2))
    umax = [0] * 16
    for v in range(vmax + 1):
        umax[v] = int(round(float(np.sqrt(225.0 - v * v))))
    v0 = 0
    for v in range(15, vmin - 1, -1):
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0
        v0 += 1
    return umax


def plain_moments(level, x, y):
    """(m10, m01) = sum of u I(x + u, y + v) and of v I(x + u, y + v) over the disc |u| <= umax[|v|], |v| <= 15: exact integers."""
    a = np.asarray(level)
    umax = plain_umax()
    m10 = m01 = 0
    for v in range(-15, 16):
        for u in range(-umax[abs(v)], umax[abs(v)] + 1):
            p = int(a[y + v, x + u])
            m10 += u * p
            m01 += v * p
    return m10, m01


def plain_blur(level, preclamp=False):
    """7 x 7 Gaussian, taps 18 34 49 55 49 34 18 per axis, BORDER_REFLECT_101, (sum + 32768) >> 16, clamped to 255 (`preclamp`: the
    value in front of the clamp, which reaches 256 and 257 on saturated patches because the taps sum to 257, not 256)."""
    a = np.pad(np.asarray(level).astype(np.int64), 3, mode="reflect")
    h, w = a.shape[0] - 6, a.shape[1] - 6
    acc = np.zeros((h, w), np.int64)
    for j in range(7):
        for i in range(7):
            acc += GAUSS[j] * GAUSS[i] * a[j:j + h, i:i + w]
    v = (acc + 32768) >> 16
    return v if preclamp else np.minimum(v, 255).astype(np.uint8)


def resize_taps(dn, sn):
    """One axis of cv::resize(INTER_LINEAR) on 8-bit images: per destination index (source index, coefficient of it, coefficient of the
    next one) in 11-bit fixed point, computed in float32 like OpenCV does."""
    scale = 1.0 / (dn / sn)
    out = []
    for d in range(dn):
        f = np.float32((d + 0.5) * scale - 0.5)
        s = int(np.floor(f))
        f = np.float32(f - np.float32(s))
        out.append((s, int(np.rint(np.float32((np.float32(1) - f) * np.float32(2048)))), int(np.rint(np.float32(f * np.float32(2048))))))
    return out


def plain_resize(level, dw, dh):
    """The 11-bit fixed-point formula: horizontal pass to 19 bits, vertical pass with two truncating products, + 2 >> 2.  Along x an
    index outside the row takes the border pixel with weight 1; along y each tap's row is clipped and the weights stay."""
    a = np.asarray(level).astype(np.int64)
    sh, sw = a.shape
    x0, x1, a0, a1 = [], [], [], []
    for s, c0, c1 in resize_taps(dw, sw):
        if s < 0:
            s, c0, c1 = 0, 2048, 0
        if s >= sw - 1:
            s, c0, c1 = sw - 1, 2048, 0
        x0.append(s); x1.append(min(s + 1, sw - 1)); a0.append(c0); a1.append(c1)
    x0, x1, a0, a1 = (np.array(v, np.int64) for v in (x0, x1, a0, a1))
    out = np.zeros((dh, dw), np.int64)
    for dy, (s, b0, b1) in enumerate(resize_taps(dh, sh)):
        r0, r1 = a[min(max(s, 0), sh - 1)], a[min(max(s + 1, 0), sh - 1)]
        h0 = r0[x0] * a0 + r0[x1] * a1
        h1 = r1[x0] * a0 + r1[x1] * a1
        out[dy] = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def plain_scales(scale_factor, nlevels):
    """mvScaleFactor in float32, each from the previous one times the double-stored factor (reference :416-423)."""
    sc = [np.float32(1)]
    for _ in range(1, nlevels):
        sc.append(np.float32(np.float64(sc[-1]) * np.float64(np.float32(scale_factor))))
    return sc


def plain_level_sizes(W, H, scale_factor, nlevels):
    """cvRound(float(size) * mvInvScaleFactor[level]) (reference :1113-1114); round() rounds halves to even like cvRound."""
    out = []
    for s in plain_scales(scale_factor, nlevels):
        inv = np.float32(1) / s
        out.append((int(round(float(np.float32(W) * inv))), int(round(float(np.float32(H) * inv)))))
    return out


def plain_pyramid(img, scale_factor, nlevels):
    """Level l is level l - 1 (the quantised bytes) resized."""
    levels = [np.ascontiguousarray(img, np.uint8)]
    for (w, h) in plain_level_sizes(img.shape[1], img.shape[0], scale_factor, nlevels)[1:]:
        levels.append(plain_resize(levels[-1], w, h))
    return levels


def plain_roots(w, h):
    """Root nodes of DistributeOctTree on a level (reference :540): round((maxX - minX) / (maxY - minY))."""
    return int(np.floor(float(np.float32(w - 2 * BORDER) / np.float32(h - 2 * BORDER)) + 0.5))


def plain_quotas(nfeatures, scale_factor, nlevels):
    """mnFeaturesPerLevel (reference :431-441), float32 arithmetic."""
    f32 = np.float32
    factor = f32(1.0 / np.float64(f32(scale_factor)))
    desired = f32(f32(f32(nfeatures) * f32(f32(1) - factor)) / f32(f32(1) - f32(np.float64(factor) ** nlevels)))
    out, total = [], 0
    for _ in range(nlevels - 1):
        out.append(int(round(float(desired))))
        total += out[-1]
        desired = f32(desired * factor)
    out.append(max(nfeatures - total, 0))
    return out


# ============================================================================================================================= worlds
class World:
    def __init__(self, family, name, image, stamps=(), refused=False, **params):
        self.family, self.name, self.image, self.stamps, self.refused = family, name, np.ascontiguousarray(image, np.uint8), list(stamps), refused
        self.params = dict(nfeatures=500, scale_factor=1.2, nlevels=1, ini_th=20, min_th=7)
        self.params.update(params)

    def __repr__(self):
        return "World(%s)" % self.name

    @property
    def levels(self):
        """the plain pyramid (computed once; nobody may write into it)"""
        if not hasattr(self, "_levels"):
            self._levels = plain_pyramid(self.image, self.params["scale_factor"], self.params["nlevels"])
            for lv in self._levels:
                lv.setflags(write=False)
        return self._levels

    def candidates(self, l):
        if not hasattr(self, "_cands"):
            self._cands = {}
        if l not in self._cands:
            self._cands[l] = plain_cell_candidates(self.levels[l], self.params["ini_th"], self.params["min_th"])
        return self._cands[l]


def texture(w, h, base=100):
    """A canvas that is nowhere flat and nowhere a corner: six grey levels, so every FAST score is below the lowest threshold used."""
    y, x = np.mgrid[0:h, 0:w]
    return (base + (x * 7 + y * 13 + (x * y) % 5) % 6).astype(np.uint8)


# the pixels whose bytes ride along in the packed quick test's 16-bit lanes: the left neighbours of ring 0, 2, 4, 6, 8, 10, 12, 14
# (those that are ring pixels themselves -- the left neighbours of ring 0 and 8 -- are left to the arc)
JUNK = [(dx - 1, dy) for k, (dx, dy) in enumerate(RING) if k % 2 == 0 and (dx - 1, dy) not in RING]


def put_stamp(img, x, y, c, d, pol, start, n, junk=None):
    """-> the stamp's record, with its stand-alone answer for a cell that holds nothing stronger"""
    assert 0 <= c + pol * d <= 255
    if junk is not None:
        for dx, dy in JUNK:
            img[y + dy, x + dx] = junk
    img[y, x] = c
    for k in range(n):
        dx, dy = RING[(start + k) % 16]
        img[y + dy, x + dx] = c + pol * d
    return dict(x=x, y=y, c=c, d=d, pol=pol, start=start, n=n, junk=junk, score=d - 1 if n >= 9 else -1, present=None)


def put_dot(img, x, y, v):
    """one pixel of value v on a canvas of (about) c: all sixteen ring pixels differ; on a flat canvas the score is |v - c| - 1"""
    c = int(img[y, x])
    flat = bool((img[y - 3:y + 4, x - 3:x + 4] == c).all())
    img[y, x] = v
    st = dict(x=x, y=y, c=c, d=abs(v - c), pol=0, start=0, n=16, junk=None, present=True)
    if flat:
        st["score"] = abs(v - c) - 1
    return st


def _usable_cells(w, h, need=16):
    return [c for c in plain_cells(w, h) if c[4] - c[2] >= need and c[5] - c[3] >= need]


def _arc_specs(ini_th, min_th, lengths=(8, 9, 10, 16), starts=range(16), pols=(1, -1)):
    ds = sorted({d for d in (min_th, min_th + 1, ini_th, ini_th + 1) if d <= 255})
    return [(pol, s, n, d) for pol in pols for n in lengths for d in ds for s in starts]


def _stamp_worlds(family, name, specs, canvas_of, ini_th, min_th, junk=None, nlevels=1):
    """One stamp per cell, stamps grouped by the canvas value they need; the centre walks through the lane residues of its cell."""
    groups = {}
    for sp in specs:
        groups.setdefault(canvas_of(*sp), []).append(sp)
    out = []
    for c in sorted(groups):
        todo = groups[c]
        part = 0
        while todo:
            w, h = (320, 240) if len(todo) > 20 else (192, 160)
            cells = _usable_cells(w, h, 26)
            img = np.full((h, w), c, np.uint8)
            stamps = []
            for k, ((pol, s, n, d), cell) in enumerate(zip(todo, cells)):
                x, y = cell[2] + 5 + k % 8, cell[3] + 5 + (k // 8) % 8
                st = put_stamp(img, x, y, c, d, pol, s, n, junk)
                st["present"] = n >= 9 and d - 1 >= min_th
                stamps.append(st)
            todo = todo[len(cells):]
            out.append(World(family, "%s_c%d_%d" % (name, c, part), img, stamps, ini_th=ini_th, min_th=min_th, nlevels=nlevels))
            part += 1
    return out


def _mid_canvas(ini_th):
    """mid-grey where the largest difference fits, the end of the byte range where it does not"""
    dmax = min(ini_th + 1, 255)
    return lambda pol, s, n, d: min(100, 255 - dmax) if pol > 0 else max(155, dmax)


def arcs_at(family, ini_th, min_th, tag, nlevels=1):
    return _stamp_worlds(family, "%s_%s" % (family, tag), _arc_specs(ini_th, min_th), _mid_canvas(ini_th), ini_th, min_th, nlevels=nlevels)


@functools.lru_cache(None)
def arcs():
    ini, mn = 20, 7
    out = arcs_at("arcs", ini, mn, "mid")
    # centres at the ends of the byte range (c - T or c + T leaves it) and ring values of exactly 0 and 255
    short = _arc_specs(ini, mn, lengths=(8, 9), starts=range(0, 16, 3))
    out += _stamp_worlds("arcs", "arcs_end", short, lambda pol, s, n, d: (0 if pol > 0 else 255), ini, mn)
    out += _stamp_worlds("arcs", "arcs_near_end", short, lambda pol, s, n, d: (3 if pol > 0 else 252), ini, mn)
    out += _stamp_worlds("arcs", "arcs_ring_end", short, lambda pol, s, n, d: (255 - d if pol > 0 else d), ini, mn)
    # the quick test's junk bytes at both extremes.  A junk pixel is a strong corner of its own, so these run with ini_th == min_th:
    # then the cell's threshold choice cannot drop a stamp and its answer stays the stand-alone one.
    for junk in (0, 255):
        for th in (7, 20):
            specs = _arc_specs(th, th, lengths=(8, 9, 16), starts=range(16))
            out += _stamp_worlds("arcs", "arcs_junk%d_t%d" % (junk, th), specs, lambda pol, s, n, d: 100 if pol > 0 else 155, th, th, junk=junk)
    return out


THRESHOLDS = [(20, 7), (1, 1), (127, 127), (128, 128), (128, 127), (254, 254), (255, 255)]


@functools.lru_cache(None)
def thresholds():
    out = []
    for ini, mn in THRESHOLDS:
        out += arcs_at("thresholds", ini, mn, "%d_%d" % (ini, mn), nlevels=2 if (ini, mn) == (20, 7) else 1)
        if ini == mn and ini in (1, 127, 128):   # the junk bytes on both sides of the packed / unpacked switch
            for junk in (0, 255):
                specs = _arc_specs(ini, mn, lengths=(8, 9), starts=range(0, 16, 2))
                out += _stamp_worlds("thresholds", "thresholds_%d_junk%d" % (ini, junk), specs,
                                     lambda pol, s, n, d: 255 - (ini + 1) - 40 if pol > 0 else ini + 1 + 40, ini, mn, junk=junk)
    return out


LAST_WIDTHS = (1, 3, 4, 5, 8, 9)
STRIP_WIDTHS = (813, 1681)


def last_cell_width(w, h=126):
    cells = plain_cells(w, h)
    return cells[-1][4] - cells[-1][2]


@functools.lru_cache(None)
def lanes():
    out = []
    w, h = 320, 240
    cells = plain_cells(w, h)
    img = np.full((h, w), 100, np.uint8)
    stamps = []

    def strong(x, y, start=0, pol=1):
        st = put_stamp(img, x, y, 100, 40, pol, start, 9)
        st["present"] = True
        stamps.append(st)

    inner = [c for c in cells if 0 < c[0] < 5 and 0 < c[1] < 8]      # interior cells of 32 x 35
    for r in range(8):                                               # every residue of (x - x0) mod 8
        c = inner[r]
        strong(c[2] + 8 + r, c[3] + 16, start=r, pol=1 if r % 2 else -1)
    c = inner[8]                                                     # first / last scored column and row of a cell
    strong(c[2], c[3] + 8); strong(c[4] - 1, c[3] + 18, start=8); strong(c[2] + 10, c[3], start=4); strong(c[2] + 20, c[5] - 1, start=12)
    # first / last scored column and row of the level, and its four corners
    strong(EDGE, 70); strong(w - EDGE - 1, 60, start=8); strong(70, EDGE, start=4); strong(100, h - EDGE - 1, start=12)
    strong(EDGE, EDGE, start=2); strong(w - EDGE - 1, EDGE, start=6); strong(EDGE, h - EDGE - 1, start=10); strong(w - EDGE - 1, h - EDGE - 1, start=14)
    out.append(World("lanes", "lanes_residues_and_rims", img, stamps))
    # last cell column 1, 3, 4, 5, 8 and 9 scored pixels wide: a dot in each of its columns (the tail mask of the row's last group)
    for want in LAST_WIDTHS:
        w = next(w for w in range(94, 2000) if last_cell_width(w) == want)   # (narrow last columns need many columns: 500 to 800 wide)
        h = 232                                    # (tall enough for at most four quadtree roots on both levels)
        img = np.full((h, w), 100, np.uint8)
        x0 = plain_cells(w, h)[-1][2]
        stamps = [put_dot(img, x0 + k, EDGE + 2 + 9 * k, 200 - k) for k in range(want)]
        stamps += [put_dot(img, x0 - 1, h - EDGE - 1, 180), put_dot(img, EDGE, EDGE, 170), put_dot(img, x0 - 9, EDGE + 40, 30)]
        out.append(World("lanes", "lanes_last_width_%d" % want, img, stamps, nlevels=2))
    # the strips: their last cell column starts where the scored area ends (cw <= 0): the first width at which the reference's grid does
    # that, and the widest the family holds
    for w in STRIP_WIDTHS:
        h = 62
        img = np.full((h, w), 100, np.uint8)
        xs = (EDGE, 45, w // 2, w // 2 + 300, w - 51, w - 50, w - 31, w - EDGE - 1)
        stamps = [put_dot(img, x, EDGE + 3 + (k * 5) % 20, 210 - k) for k, x in enumerate(xs)]
        out.append(World("lanes", "lanes_strip_%d_empty_last_column" % w, img, stamps))
    return out


def all_pass_pattern(w, h):
    """0 / 255 such that EVERY pixel passes the quick test: f = ((x + 2 y) mod 4 < 2).  Three columns or rows away the value differs
    on one side at least, and (2, 2) / (2, -2) away it always does."""
    y, x = np.mgrid[0:h, 0:w]
    return np.where((x + 2 * y) % 4 < 2, 255, 0).astype(np.uint8)


@functools.lru_cache(None)
def survivors():
    w, h = 192, 160
    cells = plain_cells(w, h)
    img = np.full((h, w), 100, np.uint8)
    stamps = []
    counts = {}
    for k, n in enumerate((0, 1, 2, 3, 9, 13)):      # isolated pixels: each is the one survivor of its neighbourhood
        c = cells[k + 5]
        for q in range(n):
            stamps.append(put_dot(img, c[2] + 4 + 7 * (q % 4), c[3] + 4 + 7 * (q // 4), 160 + q))
        counts[(c[0], c[1])] = n
    a = World("survivors", "survivors_counts", img, stamps)
    a.survivor_counts = counts
    img = np.full((h, w), 100, np.uint8)
    pat = all_pass_pattern(w, h)
    full = []
    for c in (cells[6], cells[-1]):                  # a whole cell and the ragged last one, with the rim their rings reach
        img[c[3] - 3:c[5] + 3, c[2] - 3:c[4] + 3] = pat[c[3] - 3:c[5] + 3, c[2] - 3:c[4] + 3]
        full.append((c[0], c[1]))
    b = World("survivors", "survivors_every_pixel", img, nlevels=2)
    b.full_cells = full
    return [a, b]


NMS_DIRS = {"h": (1, 0), "v": (0, 1), "d": (1, 1), "a": (-1, 1)}


@functools.lru_cache(None)
def nms():
    w, h = 192, 160
    cells = {(c[0], c[1]): c for c in plain_cells(w, h)}
    img = np.full((h, w), 100, np.uint8)
    stamps = []

    def pair(x, y, dxy, va, vb, pa, pb):
        for (px, py, v, p) in ((x, y, va, pa), (x + dxy[0], y + dxy[1], vb, pb)):
            st = put_dot(img, px, py, v)
            st["present"] = p
            stamps.append(st)

    for k, (name, dxy) in enumerate(sorted(NMS_DIRS.items())):
        c = cells[(0, k)]                                                  # equal inside one cell: both removed
        pair(c[2] + 10, c[3] + 10, dxy, 200, 200, False, False)
        pair(c[2] + 22, c[3] + 10, dxy, 200, 199, True, False)             # one grey level, each way
        pair(c[2] + 10, c[3] + 22, dxy, 199, 200, False, True)
    # equal across a cell boundary, in each direction: both stay
    c = cells[(2, 1)]
    pair(c[2] - 1, c[3] + 12, NMS_DIRS["h"], 200, 200, True, True)
    pair(c[2] + 12, c[3] - 1, NMS_DIRS["v"], 200, 200, True, True)
    c = cells[(2, 3)]
    pair(c[2] - 1, c[3] - 1, NMS_DIRS["d"], 200, 200, True, True)          # cells (1, 2) and (2, 3) across the junction
    c = cells[(3, 2)]
    pair(c[4], c[3] - 1, NMS_DIRS["a"], 200, 200, True, True)              # (2, 3) and (3, 2)
    return [World("nms", "nms_pairs", img, stamps, nfeatures=300)]


@functools.lru_cache(None)
def fallback():
    ini, mn = 20, 7
    w, h = 192, 160
    cells = _usable_cells(w, h, 26)
    img = np.full((h, w), 100, np.uint8)
    stamps = []
    #            first stamp (d, present)   second stamp (d, present) in the same cell
    plan = [((12, True), None),             # only weak: kept
            ((12, False), (40, True)),      # weak and strong: the weak one dropped
            ((12, False), (ini + 1, True)),   # a score of exactly ini_th is strong
            ((12, True), (ini, True)),        # ini_th - 1 is not: both kept
            ((mn + 1, True), None),           # exactly min_th alone: kept
            ((mn, False), None)]              # min_th - 1: no corner at all
    for k, (a, b) in enumerate(plan):
        c = cells[2 * k + 1]
        for (spec, off) in ((a, 6), (b, 19)):
            if spec:
                st = put_stamp(img, c[2] + off, c[3] + off, 100, spec[0], 1 if k % 2 else -1, 3 * k, 9)
                st["present"] = spec[1]
                stamps.append(st)
    return [World("fallback", "fallback_cells", img, stamps, ini_th=ini, min_th=mn)]


@functools.lru_cache(None)
def edges():
    w, h = 160, 120
    img = texture(w, h)
    stamps = []
    for k in range(4):          # keypoints 19 .. 22 pixels from each edge: the patch (half-size 22) crosses it, touches it, stays inside
        stamps.append(put_dot(img, EDGE + k, 32 + 12 * k, 230))
        stamps.append(put_dot(img, w - 1 - EDGE - k, 32 + 12 * k, 20))
        stamps.append(put_dot(img, 40 + 12 * k, EDGE + k, 225))
        stamps.append(put_dot(img, 40 + 12 * k, h - 1 - EDGE - k, 25))
    for (x, y) in ((EDGE, EDGE), (w - 1 - EDGE, EDGE), (EDGE, h - 1 - EDGE), (w - 1 - EDGE, h - 1 - EDGE)):
        stamps.append(put_dot(img, x, y, 240))
    return [World("edges", "edges_rims_and_corners", img, stamps, nlevels=3)]


def _corner_patch(kind):
    """31 x 31 boolean patterns with their apex at the centre"""
    dy, dx = np.mgrid[-15:16, -15:16]
    if kind == "base":      # no symmetry at all
        return (dx >= 0) & (dy >= 0) & (dy <= 4)
    if kind == "sym":       # mirror-symmetric about the x axis: m01 == 0
        return (dx >= 0) & (abs(dy) <= 2)
    if kind == "diag":      # symmetric about the diagonal: m10 == m01
        return (dx >= 0) & (dy >= 0)
    raise KeyError(kind)


def dihedral(p):
    return [np.rot90(q, k) for q in (p, np.fliplr(p)) for k in range(4)]


@functools.lru_cache(None)
def angles():
    w, h = 192, 160
    cells = plain_cells(w, h)
    img = np.full((h, w), 100, np.uint8)
    pats = [("base%d" % k, p) for k, p in enumerate(dihedral(_corner_patch("base")))]
    pats += [("sym%d" % k, np.rot90(_corner_patch("sym"), k)) for k in range(4)]
    pats += [("diag%d" % k, np.rot90(_corner_patch("diag"), k)) for k in range(4)]
    stamps = []
    for (name, p), c in zip(pats, cells):
        x, y = c[2] + 13, c[3] + 13
        sub = img[y - 15:y + 16, x - 15:x + 16]
        sub[p] = 200
        img[y, x] = 215                                  # the apex alone is the strict maximum of its corner
        stamps.append(dict(x=x, y=y, kind=name, present=True))
    c = cells[len(pats)]
    st = put_dot(img, c[2] + 13, c[3] + 13, 220)         # a symmetric patch: m10 == m01 == 0
    st["kind"] = "dot"
    stamps.append(st)
    return [World("angles", "angles_dihedral_and_zero_moments", img, stamps)]


@functools.lru_cache(None)
def saturation():
    out = []
    for name, canvas, lo, apex in (("dark_on_255", 255, 40, 20), ("bright_on_0", 0, 215, 235)):
        w, h = 192, 160
        cells = plain_cells(w, h)
        img = np.full((h, w), canvas, np.uint8)
        stamps = []
        for k, p in enumerate(dihedral(_corner_patch("base"))[:4] + [np.rot90(_corner_patch("diag"), k) for k in range(4)]):
            c = cells[k]
            x, y = c[2] + 13, c[3] + 13
            img[y - 15:y + 16, x - 15:x + 16][p] = lo
            img[y, x] = apex
            stamps.append(dict(x=x, y=y, kind="corner%d" % k, present=True))
        for k in range(4):
            c = cells[10 + k]
            stamps.append(put_dot(img, c[2] + 8 + k, c[3] + 9, 255 - canvas))
        out.append(World("saturation", "saturation_" + name, img, stamps))
    return out


TINY_OK = [(74, 100, 2), (100, 74, 2), (74, 74, 2), (62, 62, 1), (62, 90, 1)]
TINY_REFUSED = [(73, 100, 2), (100, 73, 2), (73, 73, 2), (61, 62, 1), (62, 61, 1)]


@functools.lru_cache(None)
def tiny():
    out = []
    for (w, h, nl) in TINY_OK + TINY_REFUSED:
        img = texture(w, h)
        stamps = [put_dot(img, EDGE, EDGE, 220), put_dot(img, w - 1 - EDGE, h - 1 - EDGE, 30), put_dot(img, w // 2, h // 2, 200)]
        out.append(World("tiny", "tiny_%dx%d_l%d" % (w, h, nl), img, stamps, refused=(w, h, nl) in TINY_REFUSED, nlevels=nl, nfeatures=100))
    for n in (0, 1, 2, 5):           # exactly n corners overall
        img = np.full((100, 100), 90, np.uint8)
        stamps = [put_dot(img, 25 + 11 * k, 30 + 9 * k, 180 + k) for k in range(n)]
        wd = World("tiny", "tiny_%d_corners" % n, img, stamps, nfeatures=50)
        wd.n_corners = n
        out.append(wd)
    for nf in (1, 2, 3):             # quotas of 0 and 1 on some level
        img = texture(160, 120)
        stamps = [put_dot(img, 25 + 10 * k, 25 + 6 * k, 200 + k) for k in range(12)]
        out.append(World("tiny", "tiny_quota_nf%d" % nf, img, stamps, nfeatures=nf, nlevels=3))
    return out


@functools.lru_cache(None)
def pyramid():
    out = []
    for (w, h, nl) in ((74, 74, 2), (127, 93, 3), (641, 479, 8)):
        y, x = np.mgrid[0:h, 0:w]
        for name, img in (("checker", (x + y) % 2 * 255), ("vstripes", x % 2 * 255), ("hstripes", y % 2 * 255)):
            out.append(World("pyramid", "pyramid_%s_%dx%d" % (name, w, h), img.astype(np.uint8), nlevels=nl, nfeatures=300))
    return out


FAMILIES = dict(arcs=arcs, thresholds=thresholds, lanes=lanes, survivors=survivors, nms=nms, fallback=fallback, edges=edges, angles=angles,
                saturation=saturation, tiny=tiny, pyramid=pyramid)


def all_worlds():
    return [w for f in FAMILIES.values() for w in f()]


# ============================================================================================================================= checks
def _check_stamps(world):
    """Every stamp's plain result is its stand-alone known answer: the centre's score, and present / absent with that response."""
    S = plain_scores(world.image)
    cands = {(x, y): r for x, y, r in world.candidates(0)}
    for st in world.stamps:
        x, y = st["x"], st["y"]
        if "score" in st:
            assert S[y, x] == st["score"], (world.name, st, int(S[y, x]))
        got = cands.get((x - BORDER, y - BORDER))
        assert (got is not None) == st["present"], (world.name, st, got)
        if st["present"] and "score" in st:
            assert got == st["score"], (world.name, st, got)


def _check_arc_family(worlds, sets):
    for wd in worlds:
        _check_stamps(wd)
    for (ini, mn) in sets:
        sts = [st for wd in worlds if (wd.params["ini_th"], wd.params["min_th"]) == (ini, mn) for st in wd.stamps]
        # both sides of the arc length, for both polarities and every arc start
        for pol in (1, -1):
            for start in range(16):
                mine = [st for st in sts if st["pol"] == pol and st["start"] == start]
                if mn < 255:
                    assert any(st["n"] == 8 and not st["present"] and st["d"] > mn for st in mine), (ini, mn, pol, start)
                    assert any(st["n"] == 9 and st["present"] for st in mine), (ini, mn, pol, start)
        # both sides of each threshold: d - 1 == th - 1 (no) and d - 1 == th (yes); nothing reaches a score of 255
        for th in {ini, mn}:
            assert any(st["n"] >= 9 and st["d"] == th and st["score"] == th - 1 for st in sts), (ini, mn, th)
            if th < 255:
                assert any(st["n"] >= 9 and st["d"] == th + 1 and st["score"] == th and st["present"] for st in sts), (ini, mn, th)
        if mn == 255:
            assert not any(st["present"] for st in sts)
        else:
            assert any(st["present"] for st in sts) and any(not st["present"] and st["n"] >= 9 for st in sts)


def _check_junk_sits_on_k(worlds):
    """In the packed quick test a stamp with d == min_th + 1 and the worst junk byte passes with NOTHING to spare (value == K) and one
    with d == min_th misses; both polarities' worst byte (255 under a brighter centre, 0 under a darker one) occur."""
    on_k = set()
    for w in worlds:
        mn = w.params["min_th"]
        K = 256 * mn + 1
        cells = plain_cells(w.image.shape[1], w.image.shape[0])
        for st in w.stamps:
            x0 = next(c[2] for c in cells if c[2] <= st["x"] < c[4] and c[3] <= st["y"] < c[5])
            v = packed_quick_value(w.image, st["x"], st["y"], (st["x"] - x0) % 4 == 0)
            assert (v >= K) == (st["n"] >= 9 and st["d"] > mn) or st["n"] == 8, (w.name, st, v, K)   # (with 8 the test may pass: it is only necessary)
            if st["present"] and v == K:
                on_k.add((st["junk"], st["pol"]))
    assert {(255, -1), (0, 1)} <= on_k, on_k


def check_arcs():
    ws = arcs()
    _check_arc_family([w for w in ws if "junk" not in w.name], [(20, 7)])
    junk = [w for w in ws if "junk" in w.name]
    _check_arc_family(junk, [(7, 7), (20, 20)])
    for jv in (0, 255):   # the junk bytes are in place, at both extremes, under a stamp on each side of the threshold
        sts = [st for w in junk for st in w.stamps if st["junk"] == jv]
        assert any(st["present"] and st["d"] == w.params["min_th"] + 1 for w in junk for st in w.stamps if st["junk"] == jv)
        assert any(not st["present"] and st["n"] >= 9 for st in sts)
        for w in junk:
            for st in w.stamps:
                if st["junk"] == jv:
                    assert all(w.image[st["y"] + dy, st["x"] + dx] == jv for dx, dy in JUNK)
    _check_junk_sits_on_k(junk)
    ends = [st for w in ws if "end" in w.name for st in w.stamps]
    assert {0, 3, 252, 255} <= {st["c"] for st in ends} and {0, 255} <= {st["c"] + st["pol"] * st["d"] for st in ends if st["c"] not in (0, 255)}
    assert any(st["present"] for st in ends) and any(not st["present"] for st in ends)
    assert any(st["c"] - st["d"] < 0 and st["pol"] > 0 for st in ends) and any(st["c"] + st["d"] > 255 and st["pol"] < 0 for st in ends)


def check_thresholds():
    ws = thresholds()
    assert {(w.params["ini_th"], w.params["min_th"]) for w in ws} == set(THRESHOLDS)
    _check_arc_family([w for w in ws if "junk" not in w.name], THRESHOLDS)
    for w in ws:
        if "junk" in w.name:
            _check_stamps(w)
            assert any(st["present"] for st in w.stamps) and any(not st["present"] and st["n"] >= 9 for st in w.stamps)
    _check_junk_sits_on_k([w for w in ws if "junk" in w.name and w.params["min_th"] <= 127])


def check_lanes():
    ws = lanes()
    for w in ws:
        _check_stamps(w)
    a = ws[0]
    h, w = a.image.shape
    cells = plain_cells(w, h)
    cell_of = lambda st: next(c for c in cells if c[2] <= st["x"] < c[4] and c[3] <= st["y"] < c[5])
    assert {(st["x"] - cell_of(st)[2]) % 8 for st in a.stamps[:8]} == set(range(8))
    xs, ys = {st["x"] for st in a.stamps}, {st["y"] for st in a.stamps}
    assert {EDGE, w - EDGE - 1} <= xs and {EDGE, h - EDGE - 1} <= ys
    c = a.stamps[8:12]
    assert c[0]["x"] == cell_of(c[0])[2] and c[1]["x"] == cell_of(c[1])[4] - 1 and c[2]["y"] == cell_of(c[2])[3] and c[3]["y"] == cell_of(c[3])[5] - 1
    for want, wd in zip(LAST_WIDTHS, ws[1:1 + len(LAST_WIDTHS)]):
        hh, ww = wd.image.shape
        last = plain_cells(ww, hh)[-1]
        assert last[4] - last[2] == want and last[4] == ww - EDGE
        assert {st["x"] for st in wd.stamps} >= set(range(last[2], last[4]))
    for sw, strip in zip(STRIP_WIDTHS, ws[-len(STRIP_WIDTHS):]):
        assert strip.image.shape == (62, sw)
        last = plain_cells(sw, 62)[-1]
        assert last[4] - last[2] <= 0
        assert any(st["x"] == sw - EDGE - 1 for st in strip.stamps)
    for ww in range(62, STRIP_WIDTHS[0]):     # no narrower level has an empty last cell column
        assert last_cell_width(ww, 62) > 0, ww


def check_survivors():
    a, b = survivors()
    _check_stamps(a)
    q = plain_quick_survivors(a.image, a.params["min_th"])
    h, w = a.image.shape
    got = {(c[0], c[1]): int(q[c[3]:c[5], c[2]:c[4]].sum()) for c in plain_cells(w, h)}
    for cell, n in a.survivor_counts.items():
        assert got[cell] == n, (cell, n, got[cell])
    assert {0, 1, 2, 3} <= set(got.values()) and any(n % 2 == 1 and n >= 9 for n in got.values())
    q = plain_quick_survivors(b.image, b.params["min_th"])
    cells = {(c[0], c[1]): c for c in plain_cells(w, h)}
    for cell in b.full_cells:
        c = cells[cell]
        assert q[c[3]:c[5], c[2]:c[4]].all()


def check_nms():
    (w,) = nms()
    _check_stamps(w)
    S = plain_scores(w.image)
    pairs = list(zip(w.stamps[0::2], w.stamps[1::2]))
    kinds = set()
    for a, b in pairs:
        sa, sb = int(S[a["y"], a["x"]]), int(S[b["y"], b["x"]])
        assert abs(a["x"] - b["x"]) <= 1 and abs(a["y"] - b["y"]) <= 1
        kinds.add(((b["x"] - a["x"], b["y"] - a["y"]), sa - sb, a["present"], b["present"]))
    for d in NMS_DIRS.values():
        assert {(d, 0, False, False), (d, 0, True, True), (d, 1, True, False), (d, -1, False, True)} <= kinds, d


def check_fallback():
    (w,) = fallback()
    _check_stamps(w)
    ini, mn = w.params["ini_th"], w.params["min_th"]
    sc = [(st["score"], st["present"]) for st in w.stamps]
    assert (ini, True) in sc and (ini - 1, True) in sc and (mn, True) in sc and (mn - 1, False) in sc
    assert sum(1 for s, p in sc if mn <= s < ini and not p) >= 2 and sum(1 for s, p in sc if mn <= s < ini and p) >= 2


def check_edges():
    (w,) = edges()
    _check_stamps(w)
    hh, ww = w.image.shape
    xs, ys = {st["x"] for st in w.stamps}, {st["y"] for st in w.stamps}
    assert set(range(19, 23)) <= xs and set(range(19, 23)) <= ys
    assert {ww - 1 - k for k in range(19, 23)} <= xs and {hh - 1 - k for k in range(19, 23)} <= ys
    at = {(st["x"], st["y"]) for st in w.stamps}
    assert {(19, 19), (ww - 20, 19), (19, hh - 20), (ww - 20, hh - 20)} <= at
    assert plain_scores(texture(ww, hh)).max() < w.params["min_th"]


def check_angles():
    (w,) = angles()
    _check_stamps(w)
    m = {st["kind"]: plain_moments(w.image, st["x"], st["y"]) for st in w.stamps}
    assert m["dot"] == (0, 0)
    base = [m["base%d" % k] for k in range(8)]
    assert len(set(base)) == 8 and all(a and b and abs(a) != abs(b) for a, b in base)
    sym = [m["sym%d" % k] for k in range(4)]
    assert {(np.sign(a), np.sign(b)) for a, b in sym} == {(1, 0), (-1, 0), (0, 1), (0, -1)}
    diag = [m["diag%d" % k] for k in range(4)]
    assert all(abs(a) == abs(b) > 0 for a, b in diag) and {(np.sign(a), np.sign(b)) for a, b in diag} == {(1, 1), (1, -1), (-1, 1), (-1, -1)}


def check_saturation():
    dark, bright = saturation()
    for w in (dark, bright):
        _check_stamps(w)
    pre = plain_blur(dark.image, preclamp=True)
    seen = set()
    for st in dark.stamps:       # inside the blurred patch of a keypoint (half-size 19) the clamp bites
        seen |= set(np.unique(pre[st["y"] - 19:st["y"] + 20, st["x"] - 19:st["x"] + 20]).tolist())
    assert {256, 257} <= seen and min(seen) < 200
    assert plain_blur(bright.image, preclamp=True).max() <= 255


def check_tiny():
    ws = tiny()
    for w in ws:
        p = w.params
        sizes = plain_level_sizes(w.image.shape[1], w.image.shape[0], p["scale_factor"], p["nlevels"])
        if w.refused:
            assert all(plain_cells(*s) is not None for s in sizes[:-1]) and plain_cells(*sizes[-1]) is None and min(sizes[-1]) == 61
        else:
            assert all(plain_cells(*s) is not None for s in sizes)
            _check_stamps(w)
    ok = [plain_level_sizes(w, h, 1.2, nl)[-1] for (w, h, nl) in TINY_OK]
    assert any(s[0] == 62 < s[1] for s in ok) and any(s[1] == 62 < s[0] for s in ok) and (62, 62) in ok
    for w in ws:
        if hasattr(w, "n_corners"):
            assert len(w.candidates(0)) == w.n_corners
    quotas = [q for w in ws if "quota" in w.name for q in plain_quotas(w.params["nfeatures"], 1.2, w.params["nlevels"])]
    assert 0 in quotas and 1 in quotas


def check_pyramid():
    ws = pyramid()
    assert {w.image.shape for w in ws} == {(74, 74), (93, 127), (479, 641)}
    for w in ws:
        assert set(np.unique(w.image).tolist()) == {0, 255}
        assert plain_cells(*plain_level_sizes(w.image.shape[1], w.image.shape[0], 1.2, w.params["nlevels"])[-1]) is not None
    assert min(plain_level_sizes(74, 74, 1.2, 2)[-1]) == 62
    # the rounding of the resize is exercised over the whole byte range
    vals = set()
    for w in ws[:6]:
        for lv in w.levels[1:]:
            vals |= set(np.unique(lv).tolist())
    assert {0, 255} <= vals and len(vals) > 16


CHECKS = dict(arcs=check_arcs, thresholds=check_thresholds, lanes=check_lanes, survivors=check_survivors, nms=check_nms,
              fallback=check_fallback, edges=check_edges, angles=check_angles, saturation=check_saturation, tiny=check_tiny,
              pyramid=check_pyramid)
