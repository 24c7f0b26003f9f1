"""GPU parity on the boundary worlds of tests/search_boundary_worlds.py: every projection search, in every resolve form, equal to the
oracle -- match_of_feature and nmatches, best_idx and best_dist of project_best, the candidate lists of project_candidates.

The islands of a world are a few hundred queries; FILLERS (ordinary features and queries of helpers, below the islands) carry them to
the sizes at which search_enqueue changes form.  The filler counts are the smallest that cross each limit, derived below from
search_enqueue's own arithmetic (`select_form`), and every test asserts the form it names through Matcher.last_resolve_form(): a moved
limit fails the test instead of quietly running another kernel.

The switches MORB_RESOLVE_MONO, MORB_RS_PER_CAMERA and MORB_HOST_RESOLVE are read once per process: the last test of the file runs the
boundary tests again in one child pytest per switch value, one after the other."""
import contextlib
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import oracle
import search_boundary_worlds as sw
from multi_orb_slam_amd import matcher as _mm
from test_search_boundary_worlds import BOUNDS, TH

pytestmark = pytest.mark.gpu

# ---- search_enqueue's arithmetic (csrc/search.hip), restated: the limits the filler counts are derived from
LDS_LIMIT = 150 * 1024
K = sw.RESOLVE_K
RSC_RQ = 4
MONO_MODE = int(os.environ.get("MORB_RESOLVE_MONO", "2"))
CAM_ENV = int(os.environ.get("MORB_RS_PER_CAMERA", "1"))
HOST = os.environ.get("MORB_HOST_RESOLVE", "0") not in ("0", "")
# (the library's codes: tests/test_abi.py holds matcher.FORM_* against ORBM_FORM_* of include/orb_debug.h)
F_HOST, MONO2_ANG, MONO2, MONO4_WORKLIST, MONO4_WAVES = _mm.FORM_HOST, _mm.FORM_MONO2_ANG, _mm.FORM_MONO2, _mm.FORM_MONO4_WORKLIST, _mm.FORM_MONO4_WAVES
JACOBI_LDSQ, JACOBI, CAMS, SWEEPS = _mm.FORM_JACOBI_LDSQ, _mm.FORM_JACOBI, _mm.FORM_CAMS, _mm.FORM_SWEEPS
FORM_NAMES = {_mm.FORM_NONE: "none", F_HOST: "host_resolve", MONO2_ANG: "k_resolve_mono<2,true>", MONO2: "k_resolve_mono<2,false>",
              MONO4_WORKLIST: "k_resolve_mono<4> worklist", MONO4_WAVES: "k_resolve_mono<4> per wave", JACOBI_LDSQ: "k_resolve<.,true>",
              JACOBI: "k_resolve<.,false>", CAMS: "k_resolve_cams", SWEEPS: "k_rs_sweep chain"}


def lds_tables(n, nq):
    return 2 * n * 4 + ((nq + 1) // 2) * 4


def lds_cam(nf_cap):
    return 8 * nf_cap + 2 * RSC_RQ * 1024


def lds_jacobi_q(n, nq):
    return lds_tables(n, nq) + nq * (4 + 4 + K * 4 + 1) + n * 4 + 16


def lds_mono(n, nq, ang):
    nq2 = (nq + 1) & ~1
    return n * 8 + nq2 * 4 + K * nq2 * 2 + ((nq + 3) & ~3) + ((nq + n) * 4 if ang else 0) + nq2 * 2 + 16


def select_form(n_per_cam, q_per_cam, nq, points, win2):
    n = sum(n_per_cam)
    if HOST:
        return F_HOST
    multi = lds_tables(n, nq) > LDS_LIMIT
    cams_want = CAM_ENV and not points and not win2 and (multi or (len(n_per_cam) >= 2 and CAM_ENV > 1 and nq >= CAM_ENV))
    cams_fit = cams_want and max(n_per_cam) > 0 and 0 < max(q_per_cam) <= RSC_RQ * 1024 and nq < 65536 and lds_cam(max(n_per_cam)) <= LDS_LIMIT
    if multi:
        return CAMS if cams_fit else SWEEPS
    if cams_fit:
        return CAMS
    if not points and MONO_MODE != 0 and n < 65535 and lds_mono(n, nq, False) <= LDS_LIMIT:
        if nq <= 2048:
            return MONO2_ANG if lds_mono(n, nq, True) <= LDS_LIMIT else MONO2
        return MONO4_WORKLIST if MONO_MODE == 2 else MONO4_WAVES
    return JACOBI_LDSQ if lds_jacobi_q(n, nq) <= LDS_LIMIT and n < 65535 else JACOBI


def named_form(search, scenario):
    """The form each scenario is FOR, by name (select_form, from the sizes, must say the same)."""
    if HOST:
        return F_HOST
    per_camera = search == "frames"                      # (one window per query and no ratio test)
    if scenario in ("cams", "sweeps"):                   # the frame's tables are beyond one workgroup
        return CAMS if scenario == "cams" and per_camera and CAM_ENV != 0 else SWEEPS
    if per_camera and CAM_ENV > 1:
        return CAMS
    if search != "points" and MONO_MODE != 0:
        return {"small": MONO2_ANG, "bare": MONO2_ANG, "no_angles": MONO2, "worklist": MONO4_WORKLIST if MONO_MODE == 2 else MONO4_WAVES}[scenario]
    return JACOBI if scenario == "no_angles" else JACOBI_LDSQ


def smallest(pred, lo=1, hi=1 << 20):
    """smallest integer in (lo, hi] for which pred holds (pred is monotone)"""
    assert not pred(lo) and pred(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if pred(mid) else (mid, hi)
    return hi


def plan(scenario, isl_per_cam, isl_q):
    """-> (filler features per camera, filler queries, filler th) that carry a world of isl_per_cam island features and isl_q island
    queries to the scenario's form: the smallest counts that cross the limit in question."""
    if scenario == "bare":
        return (), 0, 3.0
    if scenario == "small":                              # a few hundred features and queries, two cameras
        return (300, 200), 300, 3.0
    nq = isl_q + 300
    if scenario == "no_angles":                          # the angles no longer fit beside the tables (nq <= 2048)
        assert nq <= 2048
        n = smallest(lambda n: lds_mono(n, nq, True) > LDS_LIMIT)
        assert lds_mono(n, nq, False) <= LDS_LIMIT and lds_tables(n, nq) <= LDS_LIMIT
        assert 11000 < n < 13000                         # "about 12 000"
        a = n // 2
        return (a - isl_per_cam[0], n - a - isl_per_cam[1]), 300, 2.0
    if scenario == "worklist":                           # nq just above 2048
        return (1000, 1000), 2049 - isl_q, 3.0
    n = smallest(lambda n: lds_tables(n, nq) > LDS_LIMIT)                      # the whole frame's tables beyond a workgroup's LDS
    assert 19000 < n < 19300                             # "more than about 19 200"
    if scenario == "cams":                               # ... over two cameras that each fit one
        a = (n + 1) // 2
        assert lds_cam(a) <= LDS_LIMIT
        return (a - isl_per_cam[0], n - a - isl_per_cam[1]), 300, 2.0
    assert scenario == "sweeps"                          # ... one camera beyond a workgroup's LDS
    cap = smallest(lambda c: lds_cam(c) > LDS_LIMIT)
    c1 = isl_per_cam[1] + 500                            # (a second, small camera)
    c0 = max(cap, n - c1)
    return (c0 - isl_per_cam[0], c1 - isl_per_cam[1]), 300, 2.0


# ------------------------------------------------------------------------------------------------ worlds, shared
_cache = {}


def world(search, bounds_name, scenario, th=None, nnratio=0.8, population=None):
    key = (search, bounds_name, scenario, th, nnratio, population)
    if key not in _cache:
        th_ = TH[search] if th is None else th
        bare = sw.make_search_world(search, BOUNDS[bounds_name](), th=th_, nnratio=nnratio, population=population)
        cam = np.asarray(bare["fr"]["cam_of"])
        fillers, fq, fth = plan(scenario, [int((cam == 0).sum()), int((cam == 1).sum())], len(bare["q"]))
        w = bare if not any(fillers) else sw.make_search_world(search, BOUNDS[bounds_name](), th=th_, nnratio=nnratio, population=population,
                                                              fillers=fillers, filler_queries=fq, filler_th=fth)
        assert w["dropped"] == 0 and w["n_island_queries"] == bare["n_island_queries"]
        w["OF"] = oracle.FrameData(**w["fr"])
        w["expected"] = {}
        _cache[key] = w
    return _cache[key]


def expected(w, what, fn):
    if what not in w["expected"]:
        w["expected"][what] = fn()
    return w["expected"][what]


@pytest.fixture(scope="module")
def matcher():
    import multi_orb_slam_amd as m
    mt = m.Matcher(0.8, True)
    yield mt
    mt.close()


@contextlib.contextmanager
def device_frame(matcher, w):
    import multi_orb_slam_amd as m
    F = matcher.frame(m.FrameData(**w["fr"]))
    try:
        yield F
    finally:
        F.close()


def expected_form(w, search, scenario):
    cam = np.asarray(w["fr"]["cam_of"]); qc = np.asarray(w["q"]["cam"])
    n_per_cam = [int((cam == c).sum()) for c in range(len(w["fr"]["descs"]))]
    q_per_cam = [int((qc == c).sum()) for c in range(len(n_per_cam))] if search != "points" else [len(qc)] + [0] * (len(n_per_cam) - 1)
    want = named_form(search, scenario)
    assert select_form(n_per_cam, q_per_cam, len(qc), search == "points", search == "loop2") == want, \
        "search_enqueue's arithmetic no longer sends %s / %s to %s" % (search, scenario, FORM_NAMES[want])
    return want


def check_form(matcher, w, search, scenario, long_lists=True):
    want = expected_form(w, search, scenario)
    form, retries = matcher.last_resolve_form()
    assert form == want, "%s / %s ran %s, the test is for %s" % (search, scenario, FORM_NAMES[form], FORM_NAMES[want])
    # the islands' lists of 65, 128 and 129 candidates overflow the first capacity once; the retry rounds up to a multiple of 64
    if form != F_HOST:
        if long_lists:
            assert retries == 1 and matcher.last_resolve()[3] >= 2 * sw.FIRST_CAP + 1, (retries, matcher.last_resolve())
        elif scenario == "bare":
            assert retries == 0, retries


def same_matches(w, got, exp, what):
    (n, mo), (en, emo) = got, exp
    t = "%s: " % (what,)
    assert np.array_equal(mo, emo), t + "differing queries: %s" % sw.kinds_of_differences(w, mo, emo)
    assert n == en, t + "nmatches %d, expected %d" % (n, en)


FRAME_SCENARIOS = ["small", "no_angles", "worklist", "cams", "sweeps"]
POINT_SCENARIOS = ["small", "no_angles", "sweeps"]


# ------------------------------------------------------------------------------------------------ the searches
@pytest.mark.parametrize("bounds_name", list(BOUNDS))
@pytest.mark.parametrize("scenario", FRAME_SCENARIOS)
def test_boundary_frames(matcher, scenario, bounds_name):
    """SearchByProjection between frames: threshold 100 and 64, orientation check on and off."""
    t0 = time.time()
    for th in (100, 64):
        w = world("frames", bounds_name, scenario, th=th)
        with device_frame(matcher, w) as F:
            for ori in (True, False):
                matcher.check_orientation = ori
                try:
                    got = matcher.SearchByProjection(F, w["q"], th, w["occ"])
                finally:
                    matcher.check_orientation = True
                exp = expected(w, ("frames", ori), lambda: oracle.search_by_projection_frames(w["OF"], w["q"], th, ori, w["occ"]))
                same_matches(w, got, exp, "th %d, orientation %s" % (th, ori))
                check_form(matcher, w, "frames", scenario)
                assert exp[0] > 50
    print("boundary frames %s %s: %.2f s" % (scenario, bounds_name, time.time() - t0))


# every copy of the rotation binning and of ComputeThreeMaxima gets every population: alone (`bare`: k_resolve_mono<2,true>; under the
# switches k_resolve<false,true>, k_resolve_cams, host_resolve) and among fillers none of whose queries is ever accepted, at the sizes of
# the other forms -- `no_angles` (the angles read from HBM: k_resolve_mono<2,false>, k_resolve<false,false>'s reject pass), `worklist`
# (both schedules of k_resolve_mono<4>), `cams` (k_resolve_cams' meeting over several workgroups), `sweeps` (k_rs_owner / k_rs_reject)
HISTOGRAM_SCENARIOS = ["bare", "no_angles", "worklist", "cams", "sweeps"]


@pytest.mark.parametrize("bounds_name", list(BOUNDS))
@pytest.mark.parametrize("population", sw.POPULATIONS)
@pytest.mark.parametrize("scenario", HISTOGRAM_SCENARIOS)
def test_boundary_histogram(matcher, scenario, population, bounds_name):
    """One rotation-histogram population per world: bin edges one ulp either side, the wrap, the edges of ComputeThreeMaxima."""
    w = world("frames", bounds_name, scenario, population=population)
    with device_frame(matcher, w) as F:
        got = matcher.SearchByProjection(F, w["q"], 100, w["occ"])
    exp = expected(w, ("frames", True), lambda: oracle.search_by_projection_frames(w["OF"], w["q"], 100, True, w["occ"]))
    same_matches(w, got, exp, population)
    check_form(matcher, w, "frames", scenario, long_lists=False)
    assert (population == "empty") == (exp[0] == 0)
    assert (population in ("ten_one_one", "empty")) == (not np.any(exp[1] == -2))


@pytest.mark.parametrize("bounds_name", list(BOUNDS))
@pytest.mark.parametrize("scenario", POINT_SCENARIOS)
def test_boundary_points(matcher, scenario, bounds_name):
    """SearchByProjection(F, vpMapPoints, th): the ratio test at the five ratios, each with the pairs on ITS boundary."""
    t0 = time.time()
    for ratio in sw.RATIOS:
        w = world("points", bounds_name, scenario, nnratio=ratio)
        matcher.nnratio = ratio
        try:
            with device_frame(matcher, w) as F:
                got = matcher.SearchByProjectionPoints(F, w["q"], w["occ"])
        finally:
            matcher.nnratio = 0.8
        exp = expected(w, "points", lambda: oracle.search_by_projection_points(w["OF"], w["q"], w["occ"], ratio, 100))
        same_matches(w, got, exp, "nnratio %g" % ratio)
        check_form(matcher, w, "points", scenario)
        assert exp[0] > 50
    print("boundary points %s %s: %.2f s" % (scenario, bounds_name, time.time() - t0))


@pytest.mark.parametrize("bounds_name", list(BOUNDS))
@pytest.mark.parametrize("scenario", ["small", "worklist", "cams"])
def test_boundary_two_windows(matcher, scenario, bounds_name):
    """The two-window loop search, th_low = 50 (`cams`: a frame beyond a workgroup's LDS; two windows never resolve per camera)."""
    w = world("loop2", bounds_name, scenario)
    with device_frame(matcher, w) as F:
        got = matcher.SearchByProjectionWindows(F, w["q"], w["w2"], 50, w["occ"])
    exp = expected(w, "loop2", lambda: oracle.search_by_projection_loop2(w["OF"], w["q"], w["w2"], w["occ"], 50))
    same_matches(w, got, exp, "two windows")
    check_form(matcher, w, "loop2", scenario)
    assert exp[0] > 20


@pytest.mark.parametrize("bounds_name", list(BOUNDS))
def test_boundary_project_best_and_candidates(matcher, bounds_name):
    """project_best with gates 0, 1 and 2 (best_idx, best_dist), and the ordered candidate lists of every island query."""
    w = world("best", bounds_name, "small")
    with device_frame(matcher, w) as F:
        for gate in (0, 1, 2):
            for occ in (None, w["occ"]):
                bi, bd = matcher.project_best(F, w["q"], occ, gate, w["inv_sigma2"])
                ebi, ebd = oracle.project_best(w["OF"], w["q"], occ, gate, w["inv_sigma2"])
                bad = np.flatnonzero((bi != ebi) | (bd != ebd))
                assert len(bad) == 0, "gate %d: differing queries %s" % (gate, sorted(set("%s[%s]" % (w["kinds"][i], w["sides"][i]) for i in bad)))
    for search in ("best", "frames"):
        w = world(search, bounds_name, "small")
        nq = w["n_island_queries"]; q = w["q"][:nq]; fr = w["fr"]
        with device_frame(matcher, w) as F:
            idx, dist, cnt = matcher.project_candidates(F, q, 4 * sw.FIRST_CAP)
        alld = np.concatenate(fr["descs"])
        for i in range(nq):
            cand = oracle.features_in_area(w["OF"], int(q["cam"][i]), float(q["u"][i]), float(q["v"][i]), float(q["radius"][i]),
                                           int(q["min_level"][i]), int(q["max_level"][i]))
            ur = fr["uright"][cand]
            with np.errstate(invalid="ignore"):
                cand = cand[~((ur > 0) & (np.abs(np.float32(q["ur"][i]) - ur) > q["radius"][i]))]
            what = "%s[%s]" % (w["kinds"][i], w["sides"][i])
            assert cnt[i] == len(cand) and np.array_equal(idx[i, :cnt[i]], cand), what
            d = np.unpackbits(np.bitwise_xor(alld[cand], q["desc"][i][None, :]), axis=1).sum(1) if len(cand) else np.zeros(0)
            assert np.array_equal(dist[i, :cnt[i]], d.astype(np.uint16)), what
        assert cnt.max() == 2 * sw.FIRST_CAP + 1 or search == "best"


@pytest.mark.parametrize("bounds_name", list(BOUNDS))
def test_boundary_insertion_on_the_resident_frame(matcher, bounds_name):
    """The frame built a second time by orbm_frame_create_resident, every camera's descriptors resident: its grid is computed by
    k_frame_build_small (the host-built frame's by the host), so the k + 0.5 ties of `insert_round` and column 64 / row 48 of
    `insert_last` reach a kernel.  Same grid, same answers."""
    import multi_orb_slam_amd as m
    from multi_orb_slam_amd import rt
    w = world("frames", bounds_name, "small")
    fr = w["fr"]
    cam = np.asarray(fr["cam_of"])
    assert np.all(np.diff(cam) >= 0) and len(cam) <= 8192 and len(fr["descs"]) <= 4      # (what keeps the resident form on the device)
    bufs = []
    for d in fr["descs"]:
        d = np.ascontiguousarray(d, np.uint8)
        b = rt.DeviceBuffer(max(d.nbytes, 32)); b.upload(d); bufs.append(b)
    exp = expected(w, ("frames", True), lambda: oracle.search_by_projection_frames(w["OF"], w["q"], 100, True, w["occ"]))
    with device_frame(matcher, w) as F:
        cs, items = F.grid()
        host_built = matcher.SearchByProjection(F, w["q"], 100, w["occ"])
    FR = matcher.frame(m.FrameData(**fr), resident=[b.ptr for b in bufs])
    try:
        rcs, ritems = FR.grid()
        resident = matcher.SearchByProjection(FR, w["q"], 100, w["occ"])
    finally:
        FR.close()
        for b in bufs:
            b.free()
    ocs, oitems = oracle.grid_csr(w["OF"])
    assert rcs.tobytes() == cs.tobytes() == ocs.tobytes() and ritems.tobytes() == items.tobytes() == oitems.tobytes()
    same_matches(w, resident, exp, "resident frame")
    same_matches(w, resident, host_built, "resident against host-built")
    probes = np.flatnonzero(np.isin(w["kinds"], ("insert_round", "insert_last")))
    assert len(probes) >= 8 and np.isin(probes, resident[1]).sum() >= 4           # the insertion probes did find their features


def points_of_queries(q, V):
    """Map points whose projection through view V lands where the queries look: back-projected at depth 4 in double, facing the camera
    (radius class 2.5), max_dist = 1.1 x distance (predicted level 1, window of octaves 0 and 1).  The model projects them again in the
    reference's number formats; what it gets is what the search behind k_frustum is held to."""
    from multi_orb_slam_amd._lib import POINT_DTYPE
    f64 = np.float64
    R = V.Rcw.astype(f64); t = V.tcw.astype(f64); Ow = V.Ow.astype(f64)
    z = 4.0
    with np.errstate(invalid="ignore"):
        Pc = np.stack([(q["u"].astype(f64) - f64(V.cx)) / f64(V.fx) * z, (q["v"].astype(f64) - f64(V.cy)) / f64(V.fy) * z, np.full(len(q), z)], 1)
    P = ((Pc - t) @ R).astype(np.float32)
    PO = P.astype(f64) - Ow
    dist = np.linalg.norm(PO, axis=1)
    pts = np.zeros(len(q), POINT_DTYPE)
    pts["pos"] = P
    pts["normal"] = (PO / dist[:, None]).astype(np.float32)
    pts["max_dist"] = (1.1 * dist).astype(np.float32); pts["min_dist"] = (1.1 * dist / 1.2 ** 7).astype(np.float32)
    pts["blocks"] = q["blocks"]; pts["desc"] = q["desc"]
    return pts


@pytest.mark.parametrize("bounds_name", list(BOUNDS))
@pytest.mark.parametrize("ratio", [0.9, 0.6])
def test_boundary_local_points(matcher, ratio, bounds_name):
    """SearchLocalPoints: the islands of the points world as map points in front of a frustum_worlds view, so that k_frustum feeds the
    same search.  The windows are the model's (radius 2.5 x the level's scale, levels 0 and 1), so the islands that sit on a WINDOW's
    edge are ordinary here; every decision on descriptor distances -- threshold, ratio pairs, ties, occupancy, shortlist, list
    capacity -- is the island's own, and the result is the model's frustum + the oracle's search, bit for bit."""
    import multi_orb_slam_amd as m
    import frustum_model as fm
    import frustum_worlds as fw
    w = world("points", bounds_name, "small", nnratio=ratio)
    V0 = fw.make_view(640, 480, 3, 1.0)
    V = fm.View(V0.Rcw, V0.tcw, V0.Ow, V0.fx, V0.fy, V0.cx, V0.cy, V0.mbf, BOUNDS[bounds_name](), V0.scale_factors, V0.log_scale_factor, 1.0)
    points = points_of_queries(w["q"], V)
    matcher.nnratio = ratio
    try:
        with device_frame(matcher, w) as F, m.LocalPoints(matcher, len(points)) as pts:
            pts.write(0, points)
            ntm, nm, mo, track = matcher.SearchLocalPoints(F, pts, V.native(), None, w["occ"], n=len(points))
    finally:
        matcher.nnratio = 0.8
    e_ntm, e_nm, e_mo, e_track, verdict = fm.expected_search(w["OF"], points, V, None, w["occ"], ratio, 100)
    assert track.tobytes() == e_track.tobytes() and ntm == e_ntm
    same_matches(w, (nm, mo), (e_nm, e_mo), "local points, nnratio %g" % ratio)      # (table row i is query i of the world)
    want = F_HOST if HOST else JACOBI_LDSQ
    assert matcher.last_resolve_form()[0] == want, FORM_NAMES[matcher.last_resolve_form()[0]]
    assert HOST or matcher.last_resolve()[0] == 0
    # the islands did decide something: among the ratio islands' probes in view, some took their feature and some were refused
    got = sw.answers(w, e_mo)
    ratio_probes = np.flatnonzero((w["kinds"] == "ratio") & (verdict == fm.IN_VIEW))
    assert len(ratio_probes) >= 20 and (got[ratio_probes] != "").sum() >= 5 and (got[ratio_probes] == "").sum() >= 5
    assert e_nm > 50 and (verdict[:w["n_island_queries"]] == fm.IN_VIEW).mean() > 0.9


# ------------------------------------------------------------------------------------------------ the other switch values
CHILDREN = [("MORB_RESOLVE_MONO", "0", "boundary_frames and (small or no_angles) or boundary_histogram and (bare or no_angles) or boundary_two_windows and small", 300),
            ("MORB_RESOLVE_MONO", "1", "(boundary_frames or boundary_two_windows or boundary_histogram) and worklist", 240),
            ("MORB_RS_PER_CAMERA", "2", "boundary_frames and small or boundary_histogram and bare", 180),
            ("MORB_RS_PER_CAMERA", "0", "(boundary_frames or boundary_histogram) and (cams or sweeps)", 300),
            ("MORB_HOST_RESOLVE", "1", "(boundary_frames or boundary_points or boundary_two_windows) and small or boundary_histogram and bare", 240)]


def test_boundaries_under_every_switch_value():
    """k_resolve's Jacobi sweeps (MORB_RESOLVE_MONO=0), the per-wave schedule (=1), k_resolve_cams at the small size
    (MORB_RS_PER_CAMERA=2), the per-sweep chain for every large frame (=0) and host_resolve (MORB_HOST_RESOLVE=1): the switches are read
    once per process, so one child pytest per value runs the boundary tests of this file that reach the form in question -- one after the
    other, each under its own time limit; the tests assert the form themselves."""
    if any(k in os.environ for k in ("MORB_RESOLVE_MONO", "MORB_RS_PER_CAMERA", "MORB_HOST_RESOLVE")):
        return                                           # (a child of this test)
    for var, val, select, limit in CHILDREN:
        t0 = time.time()
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "-k", select],
                           env=dict(os.environ, **{var: val}), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=limit)
        tail = r.stdout.decode()[-3000:]
        assert r.returncode == 0 and " passed" in tail, "%s=%s:\n%s" % (var, val, tail)
        print("boundary tests under %s=%s: %.1f s" % (var, val, time.time() - t0))
