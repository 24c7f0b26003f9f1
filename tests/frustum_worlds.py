"""Synthetic local maps for the local-points tests and the bench: a frame (helpers.make_frame_arrays), a pose, and a table
of map points most of which were made by back-projecting the frame's camera-1 features, so that the search behind the frustum
test has something to find.  Also the boundary worlds: points moved by the model onto its own decision boundaries.

Everything here is input generation; what is expected of the device comes from frustum_model + the oracle alone."""
import numpy as np
import helpers
import frustum_model as fm
from multi_orb_slam_amd import synth
from multi_orb_slam_amd._lib import POINT_DTYPE

f32, f64 = np.float32, np.float64
N_LEVELS = 8

# (points, features per camera, width, height, seed, th): the sizes of the GPU tests
CASES = [(500, [1000, 500], 640, 480, 1, 3.0), (2000, [1000, 500], 640, 480, 2, 3.0), (2000, [1000, 500], 640, 480, 3, 1.0),
         (8000, [2000, 2000], 1280, 720, 4, 5.0), (16384, [2000, 2000], 1280, 720, 5, 3.0)]


def scale_pyramid(scale_factor=1.2, n_levels=N_LEVELS):
    """mvScaleFactors / mfLogScaleFactor as ORBextractor and Frame compute them (float products, log in double rounded to float)."""
    sf = np.ones(n_levels, f32)
    for i in range(1, n_levels):
        sf[i] = f32(sf[i - 1] * f32(scale_factor))
    return sf, f32(np.log(f64(f32(scale_factor))))


def make_view(W, H, seed, th, angle=0.3):
    rng = np.random.default_rng(seed + 1000)
    a = rng.normal(size=3); a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = (np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K).astype(f32)
    t = rng.normal(size=3).astype(f32)
    sf, lsf = scale_pyramid()
    return fm.View(R, t, fm.camera_centre(R, t), 525.0 * W / 640, 525.0 * W / 640, W / 2 - 0.5, H / 2 - 0.5, 40.0,
                   (0.0, 0.0, float(W), float(H)), sf, lsf, th)


def make_world(npts, n_per_cam, W, H, seed, th):
    """-> dict(fr, view, points, target): `target[i]` is the camera-1 feature point i was made from."""
    rng = np.random.default_rng(seed)
    fr = helpers.make_frame_arrays(n_per_cam, W, H, seed)
    N = n_per_cam[0]
    V = make_view(W, H, seed, th)
    R = V.Rcw.astype(f64); t = V.tcw.astype(f64); Ow = V.Ow.astype(f64)
    # a consistent stereo coordinate for the camera-1 features: uright = x - mbf / depth
    zg = rng.uniform(1.0, 8.0, N)
    has_r = rng.random(N) < 0.6
    fr["uright"][:N] = np.where(has_r, fr["un_x"][:N].astype(f64) - f64(V.mbf) / zg, -1.0).astype(f32)
    kind = rng.choice(6, npts, p=[0.58, 0.08, 0.12, 0.06, 0.06, 0.10])   # fine, behind, outside, too near, too far, grazing
    g = rng.integers(0, N, npts)
    u = fr["un_x"][g].astype(f64) + rng.uniform(-3, 3, npts)
    v = fr["un_y"][g].astype(f64) + rng.uniform(-3, 3, npts)
    z = zg[g] * (1 + rng.uniform(-0.002, 0.002, npts))
    out = kind == 2
    u[out] = np.where(rng.random(out.sum()) < 0.5, -rng.uniform(5, 200, out.sum()), W + rng.uniform(5, 200, out.sum()))
    z[kind == 1] *= -1
    Pc = np.stack([(u - f64(V.cx)) / f64(V.fx) * z, (v - f64(V.cy)) / f64(V.fy) * z, z], 1)
    P = ((Pc - t) @ R).astype(f32)                                       # R^T (Pc - t)
    PO = P.astype(f64) - Ow
    dist = np.linalg.norm(PO, axis=1)
    level = np.clip(fr["octave"][g] + rng.integers(0, 2, npts), 0, N_LEVELS - 1)
    maxd = dist * 1.2 ** (level - 0.5)
    maxd[level == 0] = dist[level == 0] * 0.95
    mind = maxd / 1.2 ** 7
    near = kind == 3; far = kind == 4
    maxd[near] *= 4; mind[near] = dist[near] * 1.5
    maxd[far] = dist[far] / 1.5; mind[far] = maxd[far] / 3.6
    d = PO / dist[:, None]
    tilt = np.where(kind == 5, rng.uniform(62, 89, npts),
                    np.where(rng.random(npts) < 0.5, rng.uniform(0, 3.0, npts), rng.uniform(5, 55, npts))) * np.pi / 180
    r = rng.normal(size=(npts, 3)); r -= (r * d).sum(1)[:, None] * d; r /= np.linalg.norm(r, axis=1)[:, None]
    pts = np.zeros(npts, POINT_DTYPE)
    pts["pos"] = P
    pts["normal"] = (np.cos(tilt)[:, None] * d + np.sin(tilt)[:, None] * r).astype(f32)
    pts["min_dist"] = mind.astype(f32); pts["max_dist"] = maxd.astype(f32)
    pts["blocks"] = (rng.random(npts) < 0.85).astype(np.int32)
    pts["desc"] = synth.perturbed_queries(fr["descs"][0][g], seed + 3, 0.06)
    return dict(fr=fr, view=V, points=pts, target=g)


def check_conditions(world, n_to_match, nmatches, match_of_feature, track, verdict):
    """What keeps a comparison on this world from passing vacuously; properties of the inputs under the model and the oracle alone."""
    n = len(world["points"]); N = int((np.asarray(world["fr"]["cam_of"]) == 0).sum())
    assert 0.2 * n <= n_to_match <= 0.8 * n, (n_to_match, n)
    for reason in fm.REJECTIONS:
        assert (verdict == reason).sum() > 0, reason
    vc = track["view_cos"][track["in_view"] != 0].astype(f64)
    assert (vc > 0.998).sum() > 0 and (vc <= 0.998).sum() > 0
    assert len(np.unique(track["level"][track["in_view"] != 0])) >= 5
    assert nmatches >= 0.25 * min(n_to_match, N), (nmatches, n_to_match, N)
    # contested features, under the model: the target of an in-view point is the camera-1 feature nearest to where the MODEL projects it
    # (inside its search window), not the feature the generator made it from
    iv = np.nonzero(track["in_view"] != 0)[0]
    fx_ = np.asarray(world["fr"]["un_x"], f32)[:N].astype(f64); fy_ = np.asarray(world["fr"]["un_y"], f32)[:N].astype(f64)
    radius = np.where(track["view_cos"][iv].astype(f64) > 0.998, 2.5, 4.0) * (float(world["view"].th) if float(world["view"].th) != 1.0 else 1.0) \
        * world["view"].scale_factors[track["level"][iv]].astype(f64)
    targets = np.full(len(iv), -1, np.int64)
    for a in range(0, len(iv), 1024):
        sel = iv[a:a + 1024]
        dx = np.abs(track["proj_x"][sel].astype(f64)[:, None] - fx_[None, :]); dy = np.abs(track["proj_y"][sel].astype(f64)[:, None] - fy_[None, :])
        d2 = dx * dx + dy * dy
        d2[(dx >= radius[a:a + 1024, None]) | (dy >= radius[a:a + 1024, None])] = np.inf
        best = d2.argmin(1)
        targets[a:a + 1024] = np.where(np.isfinite(d2[np.arange(len(sel)), best]), best, -1)
    uniq, c = np.unique(targets[targets >= 0], return_counts=True)
    multi = np.zeros(len(world["fr"]["un_x"]), bool); multi[uniq[c >= 2]] = True
    matched = np.nonzero(match_of_feature >= 0)[0]
    assert multi[matched].sum() >= 0.01 * max(len(matched), 1), (multi[matched].sum(), len(matched))


# ------------------------------------------------------------------------------------------------ boundary worlds
def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32).astype(np.int64)


def _floats(b):
    return b.astype(np.uint32).view(f32)


def bisect_field(points, view, field, comp, other, pred):
    """Per row: bisection over the float bit patterns of points[field][:, comp] (or points[field] when comp is None) between the
    row's own value (where pred holds) and other[i] (where it does not) until the two are adjacent floats.
    -> (rows that could be bisected, value where pred still holds, neighbouring value where it does not)."""
    def get(p):
        return p[field] if comp is None else p[field][:, comp]

    def put(p, val):
        if comp is None:
            p[field] = val
        else:
            p[field][:, comp] = val

    a = get(points).astype(f32).copy(); b = np.asarray(other, f32)
    trial = points.copy(); put(trial, b)
    ok = pred(points, view) & ~pred(trial, view) & (np.sign(a) == np.sign(b)) & (a != 0) & np.isfinite(b)
    rows = np.nonzero(ok)[0]
    base = points[rows].copy()
    lo = _bits(a[rows]); hi = _bits(b[rows])
    for _ in range(34):
        mid = lo + (hi - lo) // 2
        trial = base.copy(); put(trial, _floats(mid))
        p = pred(trial, view)
        lo = np.where(p, mid, lo); hi = np.where(p, hi, mid)
    assert np.all(np.abs(hi - lo) == 1)
    return rows, _floats(lo), _floats(hi), (np.sign(hi - lo)).astype(np.int64)


def make_boundary_world(n_per_cam, W, H, seed, th, per_kind=48):
    """A world whose points sit on the model's decision boundaries, both sides of each: the four image edges, both ends of the
    distance band, the viewing-angle limit, the radius class (viewCos against 0.998), every level threshold (ratios within +-2 ulps)
    and the sign of the depth, shuffled among 2 000 ordinary points.  `kinds[i]` names the boundary row i belongs to ("plain": none)."""
    base_world = make_world(4000, n_per_cam, W, H, seed, th)
    V = base_world["view"]; P0 = base_world["points"]
    verdict, track, _, keep = fm.frustum(P0, V)
    rng = np.random.default_rng(seed + 77)

    def in_view(p, v):
        return fm.frustum(p, v)[0] == fm.IN_VIEW

    rows_out, kinds, targets = [], [], []

    def emit(rows_src, recs, kind):
        rows_out.append(recs); kinds.extend([kind] * len(recs)); targets.append(base_world["target"][rows_src])

    good = keep[track["level"][keep] >= 2]          # (room in the distance band for a point that moves)
    good = good[:per_kind * 4]
    R = V.Rcw.astype(f64); t = V.tcw.astype(f64)
    Pc = P0["pos"][good].astype(f64) @ R.T + t
    # image edges: the same point at the same depth, re-projected a few pixels beyond an edge, gives the far end of the bisection
    for name, axis, edge in (("u_min", 0, -4.0), ("u_max", 0, W + 4.0), ("v_min", 1, -4.0), ("v_max", 1, H + 4.0)):
        Pc2 = Pc.copy()
        if axis == 0:
            Pc2[:, 0] = (edge - f64(V.cx)) / f64(V.fx) * Pc2[:, 2]
        else:
            Pc2[:, 1] = (edge - f64(V.cy)) / f64(V.fy) * Pc2[:, 2]
        far = ((Pc2 - t) @ R).astype(f32)
        src = P0[good].copy()
        src["min_dist"] = f32(0.01); src["max_dist"] = src["max_dist"] * f32(1.3)
        comp = int(np.argmax(np.abs(far - src["pos"]).mean(0)))
        rows, a, b, _ = bisect_field(src, V, "pos", comp, far[:, comp], in_view)
        rows = rows[:per_kind]; a = a[:per_kind]; b = b[:per_kind]
        for val in (a, b):
            rec = src[rows].copy(); rec["pos"][:, comp] = val
            emit(good[rows], rec, name)
    src = P0[good].copy()
    # distance band: max_dist down until the point is too far, min_dist up until it is too near
    rows, a, b, _ = bisect_field(src, V, "max_dist", None, src["max_dist"] * f32(0.25), in_view)
    for val in (a[:per_kind], b[:per_kind]):
        rec = src[rows[:per_kind]].copy(); rec["max_dist"] = val; emit(good[rows[:per_kind]], rec, "too_far")
    rows, a, b, _ = bisect_field(src, V, "min_dist", None, src["max_dist"] * f32(8.0), in_view)
    for val in (a[:per_kind], b[:per_kind]):
        rec = src[rows[:per_kind]].copy(); rec["min_dist"] = val; emit(good[rows[:per_kind]], rec, "too_near")
    # viewing angle and radius class: one component of the normal
    for name, pred in (("grazing", in_view),
                       ("radius", lambda p, v: fm.frustum(p, v)[1]["view_cos"].astype(f64) > 0.998)):
        for comp in range(3):
            other = src["normal"][:, comp] * f32(0.02 if name == "grazing" else 0.5)
            rows, a, b, _ = bisect_field(src, V, "normal", comp, other, pred)
            rows = rows[:per_kind // 2]
            for val in (a[:len(rows)], b[:len(rows)]):
                rec = src[rows].copy(); rec["normal"][:, comp] = val; emit(good[rows], rec, name)
    # level thresholds: max_dist so that the ratio crosses the threshold of level k, +-2 ulps around the crossing
    wide = P0[good].copy(); wide["min_dist"] = f32(1e-3)
    for k in range(N_LEVELS - 1):
        def at_most_k(p, v, k=k):
            vd, tr, _, _ = fm.frustum(p, v)
            return (vd == fm.IN_VIEW) & (tr["level"] <= k)
        lowv = wide.copy(); dist_now = wide["max_dist"]
        # start from a max_dist that puts the point at level <= k: scale it down to ratio ~ 0.9 * 1.2^k of its current distance
        PO = wide["pos"].astype(f64) - V.Ow.astype(f64); dist = np.linalg.norm(PO, axis=1)
        lowv["max_dist"] = (dist * 1.2 ** k * 0.93).astype(f32)
        rows, a, b, sgn = bisect_field(lowv, V, "max_dist", None, (dist * 1.2 ** k * 1.07).astype(f32), at_most_k)
        rows = rows[:per_kind // 4]; a = a[:len(rows)]
        for off in (-1, 0, 1, 2):
            rec = lowv[rows].copy(); rec["max_dist"] = _floats(_bits(a) + off); emit(good[rows], rec, "level%d" % k)
    # depth sign: a point behind the camera moved along one world coordinate until its depth changes sign
    behind = np.nonzero(verdict == fm.BEHIND)[0][:per_kind * 2]
    srcb = P0[behind].copy()
    zb = (srcb["pos"].astype(f64) @ R.T + t)[:, 2]
    for comp in range(3):
        other = (srcb["pos"][:, comp].astype(f64) - 2.0 * zb / R[2, comp]).astype(f32)
        rows, a, b, _ = bisect_field(srcb, V, "pos", comp, other, lambda p, v: fm.frustum(p, v)[0] == fm.BEHIND)
        rows = rows[:per_kind // 2]
        for val in (a[:len(rows)], b[:len(rows)]):
            rec = srcb[rows].copy(); rec["pos"][:, comp] = val; emit(behind[rows], rec, "behind")

    # ... among ordinary points, so that the search behind the test has as much to decide as in any other world
    plain = np.arange(len(P0) - 2000, len(P0))
    emit(plain, P0[plain], "plain")
    pts = np.concatenate(rows_out); target = np.concatenate(targets); kinds = np.array(kinds)
    perm = rng.permutation(len(pts))      # (table order decides contested features: do not leave it sorted by kind)
    return dict(fr=base_world["fr"], view=V, points=pts[perm], target=target[perm], kinds=kinds[perm])


# ------------------------------------------------------------------------------------------------ the C++ driver's world file
def write_driver_world(path, world, bad=None, prematched=()):
    """WORLD.bin of host/test_local_points.cc (layout in its header comment).  bad[i] != 0: MapPoint i isBad(); prematched: (feature,
    point) pairs F.mvpMapPoints holds before the call."""
    fr = world["fr"]; V = world["view"]; pts = world["points"]
    cam = np.asarray(fr["cam_of"]); N = int((cam == 0).sum()); N2 = len(cam) - N
    assert np.all(cam[:N] == 0) and len(fr["descs"]) == 2 and V.n_levels == 8
    bad = np.zeros(len(pts), np.int32) if bad is None else np.asarray(bad, np.int32)
    T = np.eye(4, dtype=f32); T[:3, :3] = V.Rcw; T[:3, 3] = V.tcw
    with open(path, "wb") as f:
        f.write(np.array([0x4C505731, N, N2, len(pts), len(prematched)], np.int32).tobytes())
        for k in ("un_x", "un_y", "angle", "uright"):
            f.write(np.ascontiguousarray(fr[k], f32).tobytes())
        f.write(np.ascontiguousarray(fr["octave"], np.int32).tobytes())
        f.write(np.ascontiguousarray(fr["descs"][0], np.uint8).tobytes()); f.write(np.ascontiguousarray(fr["descs"][1], np.uint8).tobytes())
        f.write(V.scale_factors.tobytes()); f.write(T.tobytes())
        f.write(np.array([V.fx, V.fy, V.cx, V.cy, V.mbf, V.min_x, V.min_y, V.max_x, V.max_y, V.log_scale_factor, V.th], f32).tobytes())
        rec = np.zeros(len(pts), np.dtype([("p", POINT_DTYPE), ("bad", "<i4")]))
        rec["p"] = pts; rec["bad"] = bad
        f.write(rec.tobytes())
        f.write(np.asarray(list(prematched), np.int32).reshape(-1, 2).tobytes())


def read_driver_out(path, npts, N):
    """OUT.bin of `test_local_points check` -> (nToMatch, nmatches, per-point records, point index per camera-1 feature)."""
    raw = open(path, "rb").read()
    head = np.frombuffer(raw, np.int32, 2)
    dt = np.dtype([("in_view", "<i4"), ("proj_x", "<f4"), ("proj_y", "<f4"), ("proj_xr", "<f4"), ("view_cos", "<f4"), ("level", "<i4"),
                   ("visible", "<i4")])
    pts = np.frombuffer(raw, dt, npts, 8)
    feat = np.frombuffer(raw, np.int32, N, 8 + npts * dt.itemsize)
    return int(head[0]), int(head[1]), pts, feat
