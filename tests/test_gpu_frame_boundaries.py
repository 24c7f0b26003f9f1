"""GPU parity on the boundary worlds of tests/frame_boundary_worlds.py: every form of the frame assembly, on every world its size limits
admit, equal to the plain model byte for byte -- the grid (cell_start, items), the merged keypoints and descriptors, uRight and depth as
bit patterns, and GetFeaturesInArea around the features that sit on the world's decisions.  (That the oracle agrees with the model is
the business of tests/test_frame_boundary_worlds.py.)

The forms, and how a world is brought to each:
  host            matcher.frame(data): the grid computed on the host (the anchor)
  resident_*      matcher.frame(data, resident=...): k_frame_build_small with the staged fill; all / no / every other camera resident
                  (beyond 8192 features or 4 cameras it hands over to the host form)
  device          Matcher.frame_from_device on the world as it is
  device@N        ... on the world inside a rig of N cameras (frame_boundary_worlds.widen): large by camera count
  counts_small    Matcher.frame_from_device_counts, the counts read on the device: k_frame_build_small with d_counts
  counts@5, @32   k_frame_fill_head + k_grid_cam(cell_cnt = NULL)
  counts_three@5  one capacity of 16385: k_frame_head + k_frame_fill(n_dev) + k_scan_cells / k_scatter_cells / k_sort_cells
  counts@33, @64  k_cams_from_counts + k_frame_fill + k_grid_cam;  counts_three@33: ... + the three launches
`dispatch` restates frame_from_device_impl's conditions once, from the sizes; every form asserts that they send it where its name says,
so a moved limit fails the test instead of quietly running another kernel.

With the counts on the device every capacity exceeds its count (count + 1, count + 300, one empty camera of capacity 500 or 16385), the
keypoint slots beyond the count hold recognisable garbage inside the grid, and the frame's buffers come from the pool dirty: a lane that
runs past the count shows in cell_start or items.  Every world is built twice on one matcher with another frame in between; the second
result must equal the first."""
import time

import numpy as np
import pytest

import frame_boundary_worlds as fw

pytestmark = pytest.mark.gpu

LDS_LIMIT = 150 * 1024
SMALL, FILL_HEAD = "k_frame_build_small", "k_frame_fill_head+k_grid_cam"


def dispatch(caps, counts_on_device):
    """frame_from_device_impl's choice (csrc/frame.hip), from the per-camera sizes it is given"""
    n, n_cams = sum(caps), len(caps)
    lds_small = 2 * (n_cams * fw.CELLS + 1) * 4 + fw.SMALL_MAX * 2
    if 0 < n <= fw.SMALL_MAX and n_cams <= fw.SMALL_CAMS and lds_small <= LDS_LIMIT:
        return SMALL
    grid_cam = max(caps) <= fw.GRID_CAM_MAX
    if counts_on_device and n_cams <= fw.HEAD_CAMS:
        if grid_cam and n:
            return FILL_HEAD
        head = "k_frame_head"
    else:
        head = "k_cams_from_counts" if counts_on_device else "host table"
    return head + "+k_frame_fill+" + ("k_grid_cam" if grid_cam else "three launches")


def resident_runs_on_device(n, n_cams):
    return 0 < n <= fw.SMALL_MAX and n_cams <= fw.SMALL_CAMS


@pytest.fixture(scope="module")
def matcher():
    import multi_orb_slam_amd as m
    mt = m.Matcher(0.8, True)
    yield mt
    mt.close()


# ------------------------------------------------------------------------------------------------ worlds on the device
_wide, _models, _uploads, _areas = {}, {}, {}, {}
GARBAGE_XY = (123.0, 45.0)          # inside every set of bounds and inside the depth image


def wide(name, n_cams, front):
    key = (name, n_cams, front)
    if key not in _wide:
        _wide[key] = fw.widen(fw.world(name), n_cams, front)
    return _wide[key]


def model_of(w):
    if w["name"] not in _models:
        _models[w["name"]] = fw.expected(w["name"]) if w["name"] in fw.BUILDERS else fw.model(w)
    return _models[w["name"]]


class Uploaded:
    """a world's per-camera arrays in HBM, capacity-sized and one slot more: the slots beyond a camera's count hold garbage"""

    def __init__(self, w, caps):
        from multi_orb_slam_amd import rt
        self.bufs = []; self.cams = []; self.desc_ptrs = []
        counts = [len(k) for k in w["cams"]]
        depth = None
        if w["depth"] is not None:
            depth = rt.DeviceBuffer(w["depth"].nbytes); depth.upload(w["depth"]); self.bufs.append(depth)
        for c, (k, d) in enumerate(zip(w["cams"], w["descs"])):
            cap = caps[c]
            assert cap >= len(k)
            kk = np.zeros(cap + 1, fw.KP_DTYPE); kk["x"], kk["y"] = GARBAGE_XY; kk["octave"] = 99; kk["angle"] = 777.0
            kk[:len(k)] = k
            dd = np.full((cap + 1, 32), 0xEE, np.uint8); dd[:len(d)] = d
            bk = rt.DeviceBuffer(kk.nbytes); bk.upload(kk); bd = rt.DeviceBuffer(dd.nbytes); bd.upload(dd)
            self.bufs += [bk, bd]
            self.cams.append((bk.ptr, bd.ptr, cap, depth.ptr if depth else 0, w["depth"].shape[1] if depth else 0))
            self.desc_ptrs.append(bd.ptr)
        cnt = np.array(counts + [0], np.int32)                     # the counts, then the extractor's status word
        self.counts = counts
        self.d_counts = rt.DeviceBuffer(cnt.nbytes); self.d_counts.upload(cnt); self.bufs.append(self.d_counts)

    def free(self):
        for b in self.bufs:
            b.free()


def uploaded(w, caps):
    key = (w["name"], tuple(caps))
    if key not in _uploads:
        if len(_uploads) > 24:                                     # (keep HBM use small: the oldest go)
            for k in list(_uploads)[:12]:
                _uploads.pop(k).free()
        _uploads[key] = Uploaded(w, caps)
    return _uploads[key]


def other_world(n_cams, n):
    """a different, larger world of the same rig: built and closed before and between the two builds of a world, it leaves the pool's
    buffers full of another frame's cells, items and cursors"""
    per = max(200, (n + 500 + n_cams - 1) // n_cams)
    per = (per + 1023) // 1024 * 1024 if per > 1024 else per       # (few distinct sizes: the worlds are cached)
    name = "other/%d/%d" % (n_cams, per)
    if name not in _wide:
        _wide[name] = fw.world_spread(name, [per] * n_cams, 5)
    return _wide[name]


def dirty_pool(matcher, n_cams, n):
    o = other_world(n_cams, n)
    U = uploaded(o, [len(k) for k in o["cams"]])
    matcher.set_calibration(None)
    F = matcher.frame_from_device(U.cams, 40.0, o["bounds"])
    F.grid()
    F.close()


# ------------------------------------------------------------------------------------------------ comparison
def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def compare(matcher, F, w, M, device_built, what):
    cs, items = F.grid()
    assert cs[-1] == M["cell_start"][-1], "%s: %d features in the grid, the model has %d" % (what, cs[-1], M["cell_start"][-1])
    bad = np.flatnonzero(cs != M["cell_start"])
    assert len(bad) == 0, "%s: cell_start differs from cell %d on (camera %d)" % (what, bad[0], bad[0] // fw.CELLS)
    bad = np.flatnonzero(items != M["items"])
    assert len(bad) == 0, "%s: items differ at %s: %s, the model has %s" % (what, bad[:8], items[bad[:8]], M["items"][bad[:8]])
    if device_built:
        k, d, ur, dp = F.download()
        assert k.tobytes() == M["kps"].tobytes(), what + ": keypoints"
        assert np.array_equal(u32(dp), u32(M["depth"])), "%s: depth differs at %s" % (what, np.flatnonzero(u32(dp) != u32(M["depth"]))[:8])
    else:
        _, d, ur, _ = F.download(kps=False, depth=False)
    assert np.array_equal(d, M["descs"]), what + ": descriptors"
    assert np.array_equal(u32(ur), u32(M["uright"])), "%s: uRight differs at %s" % (what, np.flatnonzero(u32(ur) != u32(M["uright"]))[:8])
    for label, idx in w["marks"].items():
        for g in (idx if len(idx) <= 40 else idx[:4]):             # (every boundary feature; of a full cell's thousand, the first few)
            got = matcher.features_in_area(F, int(M["cam"][g]), float(M["ux"][g]), float(M["uy"][g]), 13.0)
            if (w["name"], int(g)) not in _areas:
                _areas[(w["name"], int(g))] = fw.features_in_area(w, M, int(M["cam"][g]), M["ux"][g], M["uy"][g], 13.0)
            exp = _areas[(w["name"], int(g))]
            assert np.array_equal(got, exp), "%s: GetFeaturesInArea around %s feature %d" % (what, label, g)
    return cs, items


def capacities(counts, big=None):
    """count + 1 / count + 300, and the last empty camera 500 (or `big`); without an empty camera `big` goes on top of the last one"""
    caps = [n + (1 if c % 2 == 0 else 300) for c, n in enumerate(counts)]
    empty = [c for c, n in enumerate(counts) if n == 0]
    if empty:
        caps[empty[-1]] = big or 500
    elif big:
        caps[-1] = big
    return caps


def forms_of(name):
    """-> [(form, world, capacities or None, kernels it must run)] for every form the world's size admits"""
    w0 = fw.world(name)
    nc = len(w0["cams"]); counts0 = [len(k) for k in w0["cams"]]
    out = [("host", w0, None, None), ("resident_all", w0, None, None), ("resident_none", w0, None, None), ("resident_mixed", w0, None, None),
           ("device", w0, None, dispatch(counts0, False))]
    for t in (5, 33, 64):
        if nc + 2 <= t:
            w = wide(name, t, 2)
            out.append(("device@%d" % t, w, None, "host table+k_frame_fill+" + ("k_grid_cam" if max(counts0) <= fw.GRID_CAM_MAX else "three launches")))
    # the counts on the device
    def target(t):
        return w0 if nc == t else wide(name, t, min(2, t - nc - 1)) if nc < t else None
    ts = nc if (nc == 4 or 0 in counts0 or nc > 4) else nc + 1
    w = target(ts)
    caps = capacities([len(k) for k in w["cams"]])
    if len(caps) <= fw.SMALL_CAMS and sum(caps) <= fw.SMALL_MAX:
        out.append(("counts_small", w, caps, SMALL))
    for t in (5, 32):
        w = target(t)
        if w is not None:
            caps = capacities([len(k) for k in w["cams"]])
            if max(caps) <= fw.GRID_CAM_MAX:
                out.append(("counts@%d" % t, w, caps, FILL_HEAD))
    w = target(5) or target(32)
    if w is not None:
        out.append(("counts_three@%d" % len(w["cams"]), w, capacities([len(k) for k in w["cams"]], fw.GRID_CAM_MAX + 1), "k_frame_head+k_frame_fill+three launches"))
    for t in (33, 64):
        w = target(t)
        if w is not None:
            caps = capacities([len(k) for k in w["cams"]])
            out.append(("counts@%d" % t, w, caps, "k_cams_from_counts+k_frame_fill+" + ("k_grid_cam" if max(caps) <= fw.GRID_CAM_MAX else "three launches")))
    w = target(33)
    if w is not None and max(counts0) <= fw.GRID_CAM_MAX:
        out.append(("counts_three@33", w, capacities([len(k) for k in w["cams"]], fw.GRID_CAM_MAX + 1), "k_cams_from_counts+k_frame_fill+three launches"))
    return out


def build(matcher, form, w, M, caps):
    import multi_orb_slam_amd as m
    counts = [len(k) for k in w["cams"]]
    if form == "host" or form.startswith("resident"):
        data = m.FrameData(**fw.frame_data(w, M))
        if form == "host":
            return matcher.frame(data), False
        U = uploaded(w, counts)
        res = {"resident_all": [p for p in U.desc_ptrs], "resident_none": [0] * len(counts),
               "resident_mixed": [p if c % 2 == 0 else 0 for c, p in enumerate(U.desc_ptrs)]}[form]
        return matcher.frame(data, resident=res), False
    matcher.set_calibration(w["calib"])
    try:
        if caps is None:
            U = uploaded(w, counts)
            return matcher.frame_from_device(U.cams, w["mbf"], w["bounds"]), True
        U = uploaded(w, caps)
        return matcher.frame_from_device_counts(U.cams, U.d_counts.ptr, U.counts, w["mbf"], w["bounds"]), True
    finally:
        matcher.set_calibration(None)


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("name", fw.names())
def test_every_form_equals_the_model(matcher, name):
    t0 = time.time()
    ran = []
    for form, w, caps, kernels in forms_of(name):
        M = model_of(w)
        counts = [len(k) for k in w["cams"]]
        n, n_cams = sum(counts), len(counts)
        what = "%s [%s]" % (w["name"], form)
        if form.startswith("resident"):
            kernels = SMALL + " (staged)" if resident_runs_on_device(n, n_cams) else "host grid"
        elif form != "host":
            assert dispatch(caps or counts, caps is not None) == kernels, "%s: the dispatch no longer sends it to %s" % (what, kernels)
        first = None
        for rnd in (0, 1):
            dirty_pool(matcher, n_cams, sum(caps) if caps else n)
            F, device_built = build(matcher, form, w, M, caps)
            try:
                got = compare(matcher, F, w, M, device_built, "%s, build %d" % (what, rnd + 1))
            finally:
                F.close()
            if first is not None:
                assert got[0].tobytes() == first[0].tobytes() and got[1].tobytes() == first[1].tobytes(), what + ": the second build differs"
            first = got
        ran.append("%s=%s" % (form, kernels or "host grid"))
    print("frame boundaries %s: %.2f s; %s" % (name, time.time() - t0, "; ".join(ran)))


def test_dispatch_at_the_size_limits():
    """the worlds of the `sizes` group straddle the limits: 8192 | 8193 features, a camera of 16384 | 16385"""
    n = lambda name: [len(k) for k in fw.world(name)["cams"]]
    assert dispatch(n("sizes/total_8192"), False) == SMALL and dispatch(n("sizes/total_8193"), False) == "host table+k_frame_fill+k_grid_cam"
    assert dispatch(n("sizes/camera_16384"), False) == "host table+k_frame_fill+k_grid_cam"
    assert dispatch(n("sizes/camera_16385"), False) == "host table+k_frame_fill+three launches"
    assert resident_runs_on_device(8192, 2) and not resident_runs_on_device(8193, 2) and not resident_runs_on_device(10, 5)
    assert dispatch([1] * 32, True) == FILL_HEAD and dispatch([1] * 33, True) == "k_cams_from_counts+k_frame_fill+k_grid_cam"
    assert dispatch([1] * 4, False) == SMALL and dispatch([1] * 5, False) == "host table+k_frame_fill+k_grid_cam"
    forms = {name: [f[0] for f in forms_of(name)] for name in fw.names()}
    for group in fw.GROUPS:                              # every form runs on at least one world of every group its limits admit
        have = set(f for name in fw.names(group) for f in forms[name])
        want = {"host", "resident_all", "resident_none", "resident_mixed", "device", "device@5", "device@33", "device@64", "counts_small", "counts@5", "counts@32",
                "counts_three@5", "counts@33", "counts@64", "counts_three@33"}
        assert want <= have, (group, want - have)


def test_frame_sink_places_extracted_ties_as_the_model_does():
    """The extractor's describe kernel has its own copy of PosInGrid (the frame sink of rigs up to 4 cameras) and cannot be fed chosen
    keypoints.  Level-0 keypoints are integers, and with the bounds (0, 0, 640, 480) every tenth integer is an exact k + 0.5 tie: one
    front-end step on synth images has dozens.  The step's grid must be the model's on the step's own keypoints, cell for cell."""
    import multi_orb_slam_amd as m
    from multi_orb_slam_amd import synth
    from multi_orb_slam_amd.frontend import NativeFrontEnd
    fe = NativeFrontEnd([m.ExtractorParams(nfeatures=1500), m.ExtractorParams(nfeatures=1000)], fw.W, fw.H)
    try:
        r = fe.step([synth.image(c, 0, fw.W, fw.H) for c in range(2)])
        form, cs, items = fe.last_frame_grid()
    finally:
        fe.close()
    assert form == 1, "the step's frame was not filled through the frame sink (form %d)" % form
    counts = r["counts"]; start = np.concatenate([[0], np.cumsum(counts)])
    assert sum(counts) <= fw.SMALL_MAX and len(counts) <= fw.SMALL_CAMS
    w = dict(name="sink", cams=[r["kps"][start[c]:start[c + 1]] for c in range(2)], descs=[r["desc"][start[c]:start[c + 1]] for c in range(2)],
             depth=None, depth_width=0, mbf=40.0, bounds=fw.ROUND_BOUNDS, calib=None, marks={})
    M = fw.model(w)
    G = fw.Grid(fw.ROUND_BOUNDS)
    px, py = G.pos(M["ux"], 0), G.pos(M["uy"], 1)
    ties = np.flatnonzero((px - np.floor(px) == 0.5) | (py - np.floor(py) == 0.5))
    inside = M["cell"] >= 0
    last = np.flatnonzero(inside & ((M["cell"] % fw.CELLS // fw.ROWS == fw.COLS - 1) | (M["cell"] % fw.ROWS == fw.ROWS - 1)))
    print("frame sink: %d features, %d on an exact tie, %d in column 63 or row 47, %d outside the grid; largest x %.2f, y %.2f" %
          (len(px), len(ties), len(last), (~inside).sum(), M["ux"].max(), M["uy"].max()))
    assert len(ties) >= 20
    # Column 63 and row 47 are out of the extractor's reach with these bounds: it keeps a border of EDGE_THRESHOLD = 19 pixels
    # (reference src/ORBextractor.cc:767-771), so x <= 640 - 20 and y <= 480 - 20 at level 0 (and, scaled back, at every level), while
    # column 63 begins at x = 625 and row 47 at y = 465.  What CAN be held here: nothing lies beyond the border, and the highest
    # column and row the extraction does reach (62 and 46) are occupied.  Column 63 | 64 itself is the `grid_exit` worlds' business.
    assert len(last) == 0 and M["ux"].max() < 625 - 1 and M["uy"].max() < 465 - 1 and M["ux"].min() >= 19 and M["uy"].min() >= 19
    cols = M["cell"][inside] % fw.CELLS // fw.ROWS; rows = M["cell"][inside] % fw.ROWS
    assert cols.max() == fw.COLS - 2 and rows.max() == fw.ROWS - 2 and inside.all()
    assert r["un_x"].tobytes() == M["ux"].tobytes() and r["un_y"].tobytes() == M["uy"].tobytes()
    got_cell = np.full(len(px), -1, np.int32)
    got_cell[items] = np.repeat(np.arange(len(cs) - 1, dtype=np.int32), np.diff(cs))
    bad = ties[got_cell[ties] != M["cell"][ties]]
    assert len(bad) == 0, "tie features %s: cells %s, the model has %s" % (bad[:8], got_cell[bad[:8]], M["cell"][bad[:8]])
    assert cs.tobytes() == M["cell_start"].tobytes() and items.tobytes() == M["items"].tobytes()


def teardown_module(module):
    for U in _uploads.values():
        U.free()
    _uploads.clear()
