"""Boundary worlds of the frame assembly: keypoints, depth images and camera layouts whose every case sits on a decision of Frame merge,
ComputeStereoFromRGBD and PosInGrid / AssignFeaturesToGrid (reference src/Frame.cc:191-395, :632-642, :959-986), both sides of it in the
same world -- and a plain numpy MODEL of the three operations, which is what every form of the assembly on the device is held to.

A world is a dict: `cams` (per-camera KP_DTYPE records), `descs` (per-camera uint8[n, 32], every row of the world different), `depth`
(None, or one float32 image [rows + 1, stride] that every camera reads; only [:rows, :depth_width] is the image, the rest is padding
that only a WRONG rule ever reads), `mbf`, `bounds` (minX, minY, maxX, maxY), `calib` (None or the nine floats) and `marks`
(label -> global indices of the features that sit on the world's decisions).

Boundary values are found by bisection over float32 bit patterns in the reference's operation order (float subtract, float multiply,
round half away from zero, convert to int, compare); none is typed in.  np.round rounds halves to even, so the rounding is written out.

`model(world, rules)` carries the RIGHT rules by default; tests/test_frame_boundary_worlds.py swaps wrong ones in to show that each is
caught by the group named for it, and holds the oracle to the model on every world.  Pure numpy: neither the GPU nor the library."""
import numpy as np
from multi_orb_slam_amd._lib import KP_DTYPE

f32, f64 = np.float32, np.float64
COLS, ROWS = 64, 48
CELLS = COLS * ROWS
W, H = 640, 480
SMALL_MAX, SMALL_CAMS, GRID_CAM_MAX, HEAD_CAMS = 8192, 4, 16384, 32      # csrc/frame.hip: the sizes at which the assembly changes form
ROUND_BOUNDS = (0.0, 0.0, 640.0, 480.0)
POSITIVE_BOUNDS = (16.0, 12.0, 656.0, 492.0)
MULTI_YAML = (522.6309776476671, 521.2605910670696, 325.2888863142117, 234.2819617198055,      # reference OtherFiles/multi.yaml:7-16
              -0.01682098888100379, -0.06786658266284684, -0.008326822638637795, 0.003629888382443059, 0.0)

# the rules of the reference; every other value of a key is a WRONG rule
RIGHT = dict(round="away",          # "even": rintf; "trunc": (int) without rounding
             below_first=False,     # True: `x < minX` refused before the rounding
             exit_le=False,         # True: `px <= 64`, `py <= 48` still inside
             pick="trunc",          # "round": the keypoint rounded before the depth lookup
             depth_at="distorted",  # "undistorted": the depth read at the undistorted pixel
             dv_ge=False,           # True: `dv >= 0`
             flush=False,           # True: denormal depths read as zero
             cam_gt=False,          # True: `g > base + n` in the camera lookup
             order="index")         # "arrival": the items of a cell in the order they were dealt, not ascending


# ------------------------------------------------------------------------------------------------ float32 helpers
def _key(v):
    b = int(np.asarray(v, f32).view(np.uint32))
    return b if b < 0x80000000 else -(b & 0x7fffffff) - 1


def _unkey(k):
    b = k if k >= 0 else ((-(k + 1)) | 0x80000000)
    return np.array([b], np.uint32).view(f32)[0]


def cross(pred, a, b):
    """pred(a) holds, pred(b) does not: bisect the float32 bit patterns between them -> (last value where it holds, its neighbour where
    it does not), one ulp apart."""
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
    assert y == np.nextafter(x, y)
    return x, y


def roundf(v, how="away"):
    """roundf / rintf / truncation of float32 values, as float64 integers."""
    v = np.asarray(v, f32).astype(f64)
    if how == "away":
        return np.copysign(np.floor(np.abs(v) + 0.5), v)      # (|v| + 0.5 is exact in double for every float32 that has a fraction)
    return np.rint(v) if how == "even" else np.trunc(v)


class Grid:
    def __init__(self, bounds):
        self.minX, self.minY, self.maxX, self.maxY = (f32(b) for b in bounds)
        self.invW = f32(f32(COLS) / f32(self.maxX - self.minX))       # reference src/Frame.cc:271-272
        self.invH = f32(f32(ROWS) / f32(self.maxY - self.minY))

    def pos(self, v, axis):
        lo, inv = (self.minX, self.invW) if axis == 0 else (self.minY, self.invH)
        with np.errstate(over="ignore", invalid="ignore"):
            return (np.asarray(v, f32) - lo).astype(f32) * inv

    def index(self, v, axis, how="away"):
        return roundf(self.pos(v, axis), how).astype(np.int64)

    def centre(self, k, axis):
        """a coordinate well inside column / row k"""
        lo, inv = (self.minX, self.invW) if axis == 0 else (self.minY, self.invH)
        v = f32(lo + f32(f32(k + 0.25) / inv))                      # (k + 0.25: rounding to even and truncation find it in k too)
        assert int(self.index(v, axis)) == k and 0.2 < float(self.pos(v, axis)) - k < 0.3
        return v


def undistort(calib, xs, ys):
    """cv::undistortPoints(pts, K, dist, noArray(), K) as the reference's OpenCV evaluates it: CV_32F parameters promoted to double,
    five iterations, left to right without contraction; a copy when k1 == 0 (src/Frame.cc:676)."""
    xs = np.asarray(xs, f32); ys = np.asarray(ys, f32)
    if calib is None or f32(calib[4]) == 0:
        return xs.copy(), ys.copy()
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = [f64(f32(c)) for c in calib]
    ifx, ify = 1.0 / fx, 1.0 / fy
    x = (xs.astype(f64) - cx) * ifx; y = (ys.astype(f64) - cy) * ify
    x0, y0 = x, y
    for _ in range(5):
        r2 = x * x + y * y
        icdist = 1.0 / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x = (x0 - dx) * icdist; y = (y0 - dy) * icdist
    xx = fx * x + 0.0 * y + cx; yy = 0.0 * x + fy * y + cy; ww = 1.0 / (0.0 * x + 0.0 * y + 1.0)
    return (xx * ww).astype(f32), (yy * ww).astype(f32)


def image_bounds(calib, cols=W, rows=H):
    """Frame::ComputeImageBounds (src/Frame.cc:743-778)"""
    ux, uy = undistort(calib, [0, cols, 0, cols], [0, 0, rows, rows])
    return (float(min(ux[0], ux[2])), float(min(uy[0], uy[1])), float(max(ux[1], ux[3])), float(max(uy[2], uy[3])))


BOUNDS = {"round": lambda: ROUND_BOUNDS, "calibrated": lambda: image_bounds(MULTI_YAML), "positive": lambda: POSITIVE_BOUNDS}


# ------------------------------------------------------------------------------------------------ the model
def camera_of(counts, rules=RIGHT):
    """the camera of every global index, as the merge finds it: `while (c + 1 < n_cams && g >= base[c] + n[c]) ++c`"""
    counts = np.asarray(counts, np.int64); n = int(counts.sum())
    g = np.arange(n, dtype=np.int64)
    ends = np.cumsum(counts)                                       # base[c] + n[c]
    if not rules["cam_gt"]:
        c = np.searchsorted(ends, g, side="right")                 # the number of cameras with end <= g, walked from the front ...
    else:
        c = np.searchsorted(ends, g, side="left")                  # ... with end < g
    # (the walk stops at the first camera whose test fails; ends ascend, so the count is that camera)
    return np.minimum(c, len(counts) - 1).astype(np.int32)


def model(world, rules=RIGHT):
    """-> dict: per feature `cell` (or -1), `uright`, `depth`, `ux`, `uy`; for the frame `cell_start`, `items` (ascending global index
    inside a cell) and `cam_start`."""
    G = Grid(world["bounds"])
    counts = [len(k) for k in world["cams"]]
    n_cams = len(counts); n = sum(counts)
    kps = np.concatenate(world["cams"]) if n else np.zeros(0, KP_DTYPE)
    x, y = kps["x"], kps["y"]
    ux, uy = undistort(world["calib"], x, y)
    cam = camera_of(counts, rules)
    # ComputeStereoFromRGBD: imDepth.at<float>(v, u) of the DISTORTED keypoint, float -> int by truncation; uRight from the undistorted x
    uright = np.full(n, -1.0, f32); depth = np.full(n, -1.0, f32)
    D = world["depth"]
    if D is not None and n:
        sx, sy = (x, y) if rules["depth_at"] == "distorted" else (ux, uy)
        how = "trunc" if rules["pick"] == "trunc" else "away"
        iu = roundf(sx, how).astype(np.int64); iv = roundf(sy, how).astype(np.int64)
        if rules == RIGHT:
            assert iu.min() >= 0 and iu.max() < world["depth_width"] and iv.min() >= 0 and iv.max() < D.shape[0] - 1   # the device reads here
        dv = D[np.clip(iv, 0, D.shape[0] - 1), np.clip(iu, 0, D.shape[1] - 1)]
        if rules["flush"]:
            dv = np.where(np.abs(dv) < np.finfo(f32).tiny, f32(0), dv)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            ok = (dv >= 0) if rules["dv_ge"] else (dv > 0)
            q = (f32(world["mbf"]) / dv).astype(f32)
            ur = (ux - q).astype(f32)
        uright = np.where(ok, ur, f32(-1)).astype(f32); depth = np.where(ok, dv, f32(-1)).astype(f32)
    # PosInGrid: round((x - minX) * invW), inside while 0 <= px < 64 and 0 <= py < 48
    px = G.index(ux, 0, rules["round"]); py = G.index(uy, 1, rules["round"])
    inside = (px >= 0) & (py >= 0) & ((px <= COLS) & (py <= ROWS) if rules["exit_le"] else (px < COLS) & (py < ROWS))
    if rules["below_first"]:
        inside &= ~((ux < G.minX) | (uy < G.minY))
    cell = np.where(inside, (cam.astype(np.int64) * COLS + px) * ROWS + py, -1)
    ncell = n_cams * CELLS
    cell = np.where(cell >= ncell, -1, cell).astype(np.int32)       # (a wrong rule's cell behind the last camera has no list to go to)
    # AssignFeaturesToGrid: camera after camera in index order
    ins = np.flatnonzero(cell >= 0)
    order = ins[np.argsort(cell[ins], kind="stable")]
    if rules["order"] == "arrival" and len(ins):
        deal = np.random.default_rng(7).permutation(len(ins))       # some order that is not the ascending one
        order = ins[deal][np.argsort(cell[ins][deal], kind="stable")]
    cell_start = np.zeros(ncell + 1, np.int32)
    cell_start[1:] = np.cumsum(np.bincount(cell[ins], minlength=ncell))
    cam_start = np.zeros(n_cams + 1, np.int32); cam_start[1:] = np.cumsum(counts)
    return dict(cell=cell, uright=uright, depth=depth, ux=ux, uy=uy, cell_start=cell_start, items=order.astype(np.int32), cam_start=cam_start,
                kps=kps, descs=np.concatenate(world["descs"]) if n else np.zeros((0, 32), np.uint8), cam=cam)


def features_in_area(world, M, cam, x, y, r):
    """Frame::GetFeaturesInArea over the model's grid, walked in the reference's order (columns, then rows, then the cell's items)."""
    G = Grid(world["bounds"]); x = f32(x); y = f32(y); r = f32(r)
    x0 = max(0, int(np.floor(f32(f32(f32(x - G.minX) - r) * G.invW))))
    x1 = min(COLS - 1, int(np.ceil(f32(f32(f32(x - G.minX) + r) * G.invW))))
    y0 = max(0, int(np.floor(f32(f32(f32(y - G.minY) - r) * G.invH))))
    y1 = min(ROWS - 1, int(np.ceil(f32(f32(f32(y - G.minY) + r) * G.invH))))
    out = []
    if x0 >= COLS or x1 < 0 or y0 >= ROWS or y1 < 0:
        return np.zeros(0, np.int32)
    cs, items = M["cell_start"], M["items"]
    for ix in range(x0, x1 + 1):
        for iy in range(y0, y1 + 1):
            c = (cam * COLS + ix) * ROWS + iy
            for g in items[cs[c]:cs[c + 1]]:
                if abs(f32(M["ux"][g] - x)) < r and abs(f32(M["uy"][g] - y)) < r:
                    out.append(g)
    return np.array(out, np.int32)


def frame_data(world, M):
    """The FrameData arrays of the host-built forms (orbm_frame_create / _resident): the model's undistorted positions and uRight."""
    kps = M["kps"]
    return dict(un_x=M["ux"], un_y=M["uy"], octave=kps["octave"], angle=kps["angle"], uright=M["uright"], cam_of=M["cam"],
                local_of=np.concatenate([np.arange(len(k), dtype=np.int32) for k in world["cams"]] + [np.zeros(0, np.int32)]),
                descs=world["descs"], bounds=world["bounds"])


# ------------------------------------------------------------------------------------------------ the builder
def records(x, y, first):
    n = len(x); g = first + np.arange(n)
    k = np.zeros(n, KP_DTYPE)
    k["x"] = x; k["y"] = y; k["size"] = 31.0; k["angle"] = (g * 37 % 360).astype(f32); k["response"] = g.astype(f32)
    k["octave"] = g % 8; k["class_id"] = -1
    return k


def descriptors(n, first, seed):
    d = np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)
    d[:, :4] = (first + np.arange(n, dtype=np.uint32)).astype("<u4").view(np.uint8).reshape(n, 4)      # every row of the world different
    return d


class _World:
    def __init__(self, name, group, bounds, n_cams, calib=None):
        self.name, self.group, self.bounds, self.calib = name, group, tuple(float(f32(b)) for b in bounds), calib
        self.G = Grid(bounds)
        self.x = [[] for _ in range(n_cams)]; self.y = [[] for _ in range(n_cams)]; self.n = [0] * n_cams
        self.marks = {}; self.notes = {}

    def add(self, cam, x, y, mark=None):
        x = np.atleast_1d(np.asarray(x, f32)); y = np.atleast_1d(np.asarray(y, f32))
        if mark:
            self.marks.setdefault(mark, []).extend((cam, self.n[cam] + i) for i in range(len(x)))
        self.x[cam].append(x); self.y[cam].append(y); self.n[cam] += len(x)

    def in_cell(self, cam, cell, mark=None, count=1):
        """`count` features of camera `cam` in its cell `cell` (column-major, as the grid numbers them)"""
        self.add(cam, np.full(count, self.G.centre(cell // ROWS, 0)), np.full(count, self.G.centre(cell % ROWS, 1)), mark)

    def done(self, depth=None, depth_width=0, mbf=40.0):
        base = np.concatenate([[0], np.cumsum(self.n)])
        cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, f32)
        cams = [records(cat(self.x[c]), cat(self.y[c]), int(base[c])) for c in range(len(self.n))]
        descs = [descriptors(self.n[c], int(base[c]), 1000 + c) for c in range(len(self.n))]
        marks = {k: np.array(sorted(int(base[c]) + l for c, l in v), np.int64) for k, v in self.marks.items()}
        return dict(name=self.name, group=self.group, cams=cams, descs=descs, depth=depth, depth_width=depth_width, mbf=float(mbf),
                    bounds=self.bounds, calib=self.calib, marks=marks, notes=self.notes)


CELL_COLS = (0, 1, 31, 62, 63)
CELL_ROWS = (0, 1, 23, 46, 47)


def world_cell_round(bounds_name):
    """The edge between column k and k + 1 (rows alike) for every listed column that has a right-hand neighbour inside the grid, and the
    edge below it: the last float that stays and the first that moves on.  notes: how many of the movers land on k + 0.5 exactly."""
    B = _World("cell_round/" + bounds_name, "cell_round", BOUNDS[bounds_name](), 2)
    G = B.G; ties = 0; cases = 0
    for axis, listed, n_axis in ((0, CELL_COLS, COLS), (1, CELL_ROWS, ROWS)):
        edges = sorted(set([k for k in listed if k + 1 < n_axis] + [k - 1 for k in listed if k >= 1]))
        for i, k in enumerate(edges):
            stay, move = cross(lambda v: int(G.index(v, axis)) <= k, G.centre(k, axis), G.centre(k + 1, axis))
            ties += int(float(G.pos(move, axis)) == k + 0.5); cases += 1
            other = G.centre(3 + 5 * i, 1 - axis)                # every case on a row (column) of its own
            for v, mark in ((stay, "stay"), (move, "move")):
                B.add(cases % 2, v if axis == 0 else other, other if axis == 0 else v, mark)
                if float(G.pos(v, axis)) == k + 0.5:
                    B.marks.setdefault("tie", []).append((cases % 2, B.n[cases % 2] - 1))
    B.notes = dict(cases=cases, exact_ties=ties)
    return B.done()


def world_grid_exit(bounds_name):
    """Column 63 | 64 and row 47 | 48, the maximum itself, the lower edge (the last float with pos > -0.5 is cell 0, the first at or
    below is outside) and the minimum itself.  Two cameras, the cases in camera 0: a cell index one column too far lies in camera 1."""
    B = _World("grid_exit/" + bounds_name, "grid_exit", BOUNDS[bounds_name](), 2)
    G = B.G; cases = 0; ties = 0
    for axis, n_axis, lo, hi in ((0, COLS, G.minX, G.maxX), (1, ROWS, G.minY, G.maxY)):
        span = f32(hi - lo)
        last_in, first_out = cross(lambda v: int(G.index(v, axis)) <= n_axis - 1, G.centre(n_axis - 1, axis), f32(hi + span / f32(64)))
        low_out, low_in = cross(lambda v: int(G.index(v, axis)) < 0, f32(lo - span / f32(32)), G.centre(0, axis))
        assert float(G.pos(low_in, axis)) > -0.5 >= float(G.pos(low_out, axis))
        ties += int(float(G.pos(first_out, axis)) == n_axis - 0.5) + int(float(G.pos(low_out, axis)) == -0.5)
        for i, (v, mark) in enumerate(((last_in, "in"), (first_out, "out"), (hi, "out"), (low_in, "in"), (low_out, "out"), (lo, "in"))):
            other = G.centre(5 + 6 * i + axis, 1 - axis)
            B.add(0, v if axis == 0 else other, other if axis == 0 else v, mark)
            if mark == "in" and v < lo:
                B.marks.setdefault("below_min_in", []).append((0, B.n[0] - 1))
            cases += 1
    B.in_cell(1, 0); B.in_cell(1, CELLS - 1); B.in_cell(0, 1500)
    B.notes = dict(cases=cases, exact_ties=ties)
    return B.done()


STRIDE = 704


def depth_image(stride=STRIDE):
    """every pixel (the padding included) different from every other: truncation, rounding and swapped axes each read another value"""
    idx = np.arange((H + 1) * stride, dtype=f64).reshape(H + 1, stride)
    D = (1.0 + idx / 65536.0).astype(f32)
    assert len(np.unique(D)) == D.size
    return D


def world_depth_pick(calibrated):
    """Fractional keypoint coordinates next to an integer, the last column and row, a stride larger than the width; `calibrated`: k1 != 0,
    the depth read at the distorted pixel and uRight from the undistorted x, at keypoints where the two pixels differ."""
    calib = MULTI_YAML if calibrated else None
    B = _World("depth_pick/" + ("k1" if calibrated else "plain"), "depth_pick", image_bounds(calib), 2, calib)
    pts = [(100, 50), (317, 201), (5, 470), (630, 7)]
    for i, (u, v) in enumerate(pts):
        c = i % 2
        B.add(c, np.nextafter(f32(u + 1), f32(0)), v, "frac"); B.add(c, u, np.nextafter(f32(v + 1), f32(0)), "frac")
        B.add(c, f32(u + 0.999), v, "frac"); B.add(c, u, f32(v + 0.999), "frac"); B.add(c, f32(u + 0.5), f32(v + 0.5), "frac")
        B.add(c, u, v, "whole")
    for c, (u, v) in enumerate([(W - 1, 33), (40, H - 1)]):
        B.add(c, u, v, "last"); B.add(c, f32(u + 0.75) if u == W - 1 else u, f32(v + 0.75) if v == H - 1 else v, "last")
    B.add(1, W - 1, H - 1, "last"); B.add(0, np.nextafter(f32(W), f32(0)), np.nextafter(f32(H), f32(0)), "last")
    if calibrated:
        for u, v in [(20.25, 30.5), (610.5, 25.25), (30.75, 450.5), (600.25, 440.75), (322.5, 12.25), (8.5, 240.75), (560.5, 400.25), (90.25, 80.5)]:
            ux, uy = undistort(calib, [u], [v])
            if 0 <= ux[0] < W and 0 <= uy[0] < H and (int(ux[0]), int(uy[0])) != (int(u), int(v)):
                B.add(0, u, v, "moved")
        assert len(B.marks.get("moved", [])) >= 3
    return B.done(depth_image(), W)


DEPTH_VALUES = [("+0", 0.0), ("-0", -0.0), ("denorm_min", 1e-45), ("denorm_max", 1.1754942e-38), ("flt_min", 1.17549435e-38), ("-1", -1.0),
                ("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf), ("1e-38", 1e-38), ("0.3", 0.3), ("0.7", 0.7), ("3", 3.0), ("4.1", 4.1),
                ("65.3", 65.3)]


def world_depth_value():
    """One keypoint per listed depth value, each on a pixel and a cell of its own, and a fractional undistorted x so that the
    subtraction rounds.  uRight / depth are -1 / -1 unless dv > 0."""
    B = _World("depth_value", "depth_value", ROUND_BOUNDS, 2)
    D = depth_image()
    with np.errstate(over="ignore"):
        vals = [(name, f32(v)) for name, v in DEPTH_VALUES]
    assert vals[2][1] == np.nextafter(f32(0), f32(1)) and vals[3][1] == np.nextafter(np.finfo(f32).tiny, f32(0)) and vals[4][1] == np.finfo(f32).tiny
    inexact = 0
    for i, (name, v) in enumerate(vals):
        u, w = 21 + 37 * i, 17 + 29 * i
        D[w, u] = v
        B.add(i % 2, f32(u + 0.3), f32(w + 0.6), "positive" if v > 0 else "refused")
        if v > 0 and np.isfinite(v):
            with np.errstate(over="ignore"):
                inexact += int(f64(f32(f32(40.0) / v)) != 40.0 / f64(v))
    B.notes = dict(cases=len(vals), inexact_quotients=inexact)
    return B.done(D, W, 40.0)


CAMERA_LAYOUTS = {"one": [7], "empty_first": [0, 5], "empty_last": [5, 0], "empty_middle_and_single": [3, 0, 1, 4], "all_but_one_empty": [0, 0, 6, 0],
                  "five": [2, 0, 3, 1, 0],
                  "c32": [(c * 5 + 2) % 4 for c in range(32)], "c33": [(c * 3 + 1) % 4 for c in range(33)], "c64": [(c * 7 + 3) % 5 for c in range(64)]}


def world_cameras(layout):
    """Every feature in a cell of its own; the first and the last feature of every camera are marked: a camera lookup wrong by one at
    base + n puts them into the neighbouring camera's cells."""
    counts = CAMERA_LAYOUTS[layout]
    B = _World("cameras/" + layout, "cameras", ROUND_BOUNDS, len(counts))
    for c, n in enumerate(counts):
        for l in range(n):
            mark = "first" if l == 0 else "last" if l == n - 1 else None
            if l == 0 and n == 1:
                B.marks.setdefault("single", []).append((c, 0))
            B.in_cell(c, (c * 211 + l * 997 + 5) % CELLS, mark)
    B.notes = dict(counts=counts)
    return B.done()


def world_occupancy(kind):
    B = _World("occupancy/" + kind, "occupancy", ROUND_BOUNDS, {"full_a": 2, "full_b": 3, "full_c": 2, "every_cell": 2, "first_last": 3, "all_outside": 2}[kind])
    rng = np.random.default_rng(11)
    if kind == "full_a":           # all features of a camera in one cell: 1025 in cell 0, 65 in the last cell
        B.in_cell(0, 0, "full", 1025); B.in_cell(1, CELLS - 1, "full", 65)
    elif kind == "full_b":         # 64 in a middle cell, 2 in cell 0, 1 in the last cell
        B.in_cell(0, 1500, "full", 64); B.in_cell(1, 0, "full", 2); B.in_cell(2, CELLS - 1, "full", 1)
    elif kind == "full_c":         # 65 in a middle cell, 1025 in the last cell of the last camera
        B.in_cell(0, 1501, "full", 65); B.in_cell(1, CELLS - 1, "full", 1025)
    elif kind == "every_cell":     # each of the 3072 cells of a camera holds exactly one feature, dealt in a shuffled order
        for c in range(2):
            cells = rng.permutation(CELLS)
            B.add(c, [B.G.centre(k // ROWS, 0) for k in cells], [B.G.centre(k % ROWS, 1) for k in cells], "full")
    elif kind == "first_last":     # only the first and the last cell of every camera, alternating
        for c in range(3):
            for l in range(20):
                B.in_cell(c, 0 if (l + c) % 2 else CELLS - 1, "full")
    else:                          # nothing inside the grid
        for c in range(2):
            B.add(c, np.where(np.arange(20) % 2 == 0, f32(700.0), f32(-40.0)), rng.uniform(0, 480, 20).astype(f32), "outside")
    return B.done()


def world_spread(name, counts, seed, group="sizes"):
    """`counts` features per camera spread over the grid in a shuffled order, about one in ten outside it"""
    B = _World(name, group, ROUND_BOUNDS, len(counts))
    rng = np.random.default_rng(seed)
    for c, n in enumerate(counts):
        x = rng.uniform(-2.0, 638.0, n).astype(f32); y = rng.uniform(-2.0, 478.0, n).astype(f32)
        out = rng.random(n) < 0.1
        x = np.where(out & (np.arange(n) % 2 == 0), f32(641.0) + x / f32(16), x); y = np.where(out & (np.arange(n) % 2 == 1), f32(-3.0) - y / f32(16), y)
        B.add(c, x, y)
    return B.done()


def world_sizes(total):
    counts = [total] if total <= 1 else [total // 3, total - total // 3]
    return world_spread("sizes/total_%d" % total, counts, 100 + total)


def world_camera_size(n):
    return world_spread("sizes/camera_%d" % n, [100, n], 200 + n)


TOTALS = (1, 1023, 1024, 1025, 8191, 8192, 8193)
CAMERA_SIZES = (16383, 16384, 16385)

# name -> builder; the worlds are built on demand and kept (tests share them and leave them unchanged)
BUILDERS = {}
for _b in BOUNDS:
    BUILDERS["cell_round/" + _b] = (lambda b=_b: world_cell_round(b))
    BUILDERS["grid_exit/" + _b] = (lambda b=_b: world_grid_exit(b))
BUILDERS["depth_pick/plain"] = lambda: world_depth_pick(False)
BUILDERS["depth_pick/k1"] = lambda: world_depth_pick(True)
BUILDERS["depth_value"] = world_depth_value
for _l in CAMERA_LAYOUTS:
    BUILDERS["cameras/" + _l] = (lambda l=_l: world_cameras(l))
for _k in ("full_a", "full_b", "full_c", "every_cell", "first_last", "all_outside"):
    BUILDERS["occupancy/" + _k] = (lambda k=_k: world_occupancy(k))
for _t in TOTALS:
    BUILDERS["sizes/total_%d" % _t] = (lambda t=_t: world_sizes(t))
for _n in CAMERA_SIZES:
    BUILDERS["sizes/camera_%d" % _n] = (lambda n=_n: world_camera_size(n))
BUILDERS["sizes/zero"] = lambda: world_spread("sizes/zero", [0, 0], 1)
GROUPS = ("cell_round", "grid_exit", "depth_pick", "depth_value", "cameras", "occupancy", "sizes")

_worlds, _models = {}, {}


def world(name):
    if name not in _worlds:
        _worlds[name] = BUILDERS[name]()
    return _worlds[name]


def expected(name):
    """the model of a world under the RIGHT rules, computed once"""
    if name not in _models:
        _models[name] = model(world(name))
    return _models[name]


def names(group=None):
    return [n for n in BUILDERS if group is None or n.split("/")[0] == group]


def widen(w, n_cams, front=2, filler=True):
    """The same world inside a larger rig: `front` cameras in front (three features each, one of them outside the grid unless the world has a depth image; `filler` False:
    empty), the world's cameras, empty cameras behind, `n_cams` in all.  The marks move with their features."""
    extra = n_cams - len(w["cams"])
    assert extra >= front >= 0
    if extra == 0:
        return w
    fr = []
    G = Grid(w["bounds"])
    for c in range(front):
        # (a world with a depth image keeps every keypoint inside the image: the lookup has no bounds check, as in the reference)
        x = np.array([G.centre(3 + c, 0), G.centre(40, 0), f32(G.maxX + f32(50)) if w["depth"] is None else G.centre(50, 0)], f32); y = np.array([G.centre(7, 1), G.centre(30 + c, 1), G.centre(9, 1)], f32)
        fr.append(records(x, y, 900000 + 3 * c) if filler else np.zeros(0, KP_DTYPE))
    fd = [descriptors(len(k), 900000 + 3 * c, 77 + c) for c, k in enumerate(fr)]
    back = extra - front
    shift = sum(len(k) for k in fr)
    out = dict(w)
    out["name"] = "%s@%d+%d" % (w["name"], n_cams, front)
    out["cams"] = fr + list(w["cams"]) + [np.zeros(0, KP_DTYPE) for _ in range(back)]
    out["descs"] = fd + list(w["descs"]) + [np.zeros((0, 32), np.uint8) for _ in range(back)]
    out["marks"] = {k: v + shift for k, v in w["marks"].items()}
    return out
