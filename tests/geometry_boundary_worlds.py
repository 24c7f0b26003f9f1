"""Boundary worlds of the three geometry ports -- the pair loop of CreateNewMapPoints (csrc/triangulate.hip), CheckInliers of the
Sim3Solver (csrc/sim3.hip) and the outlier flags of PoseOptimization (csrc/pose.hip): inputs whose every case sits ON a decision of
tri_pair, sim3_inlier or the pose classification, one float either side of it.  The complement of the guard bands of
triangulate_worlds / sim3_worlds / pose_worlds: those keep the inputs away from every decision because two summation orders may
legitimately differ; in the DEVICE order host routine, model and kernel must give identical bytes, so here the inputs can sit on the
boundaries.

The conventions are those of tests/search_boundary_worlds.py.  Every case belongs to a named GROUP (the decision) and a SIDE; no
boundary value is typed in: it is the model's own intermediate value (the `trace` of tests/triangulate_model.py, err1 / err2 of
tests/sim3_model.py, class_chi of tests/pose_model.py) moved with np.nextafter in float32, or, where the quantity is not a free input,
the end of a float32 bisection of one input through the library's HOST routine (orbv_triangulate_pairs_host, orbm_sim3_ransac_host in
device order, orbm_pose_optimize_host in device order), which ends at two adjacent floats whose answers differ.  All construction runs
on the CPU.  check_conditions() asserts, on the host routine's answers, that every group is present with the sides it names and that
each side's answer is the one its name claims; what is expected of a device is the host routine's bytes, nothing else.

Triangulation: the cases whose boundary is a per-feature quantity live in ONE world (`main`, a few hundred pairs); a boundary in a
per-keyframe quantity (the translation of [R|t] for the depth signs, the camera centre for the scale gates, a table of the exact
worlds) needs keyframes of its own, so those cases are small side worlds of one pair each.  batch_orders() carries every group of
every world onto positions 0, 63 and 64 of a launch."""
import functools
import math

import numpy as np

import pose_model as pm
import pose_worlds as pw
import sim3_model as sm
import sim3_worlds as sw
import triangulate_model as tm
import triangulate_worlds as tw
from search_boundary_worlds import cross

f32, f64 = np.float32, np.float64
INF = f32(np.inf)


def up(v):
    return np.nextafter(f32(v), INF)


def down(v):
    return np.nextafter(f32(v), -INF)


def adjacent(a, b):
    return f32(a) != f32(b) and (up(a) == f32(b) or down(a) == f32(b))


# ==================================================================================================== triangulation
QUARTER = np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], np.float64)          # X_cam1 = QUARTER * X_cam2 + t: exact in float
EXACT_SCALE = (1, 2, 4, 8, 16, 32, 64, 128)     # the power-of-two scale table of the equality cases: ratioFactor = 1.5 * 2 = 3
SVD, U1, U2, NOPATH = tm.PATH_SVD, tm.PATH_UNPROJECT1, tm.PATH_UNPROJECT2, tm.PATH_NONE


def main_make(baseline=(0.25, 0.02, 0.1)):
    """The generated worlds' poses (triangulate_worlds.make_world, "25cm")."""
    kf1 = tw.KF(tw.rotation((0.3, 1.0, 0.2), 1.5), (0.02, -0.01, 0.03), 0)
    R2 = tw.rotation((0.2, 1.0, -0.3), 3.0) @ tw.rotation((0.3, 1.0, 0.2), 1.5)
    kf2 = tw.KF(R2, -R2 @ (np.array(baseline) + kf1.centre[0].astype(f64)), 0)
    return kf1, kf2


def sideways_make(cam):
    """The main poses for a camera-1 pair; for a camera-2 pair (that camera looks along world x) keyframe 2 to ITS side, so that the
    linear triangulation of a camera-2 pair is as well conditioned as that of a camera-1 pair."""
    return main_make if cam == 0 else functools.partial(main_make, (0.1, 0.02, -0.25))


def ortho_make():
    """Keyframe 2 a quarter turn about y from keyframe 1, both rotations exact: the rays of the two principal points are at exactly
    90 degrees (the rays use the first camera's rotations whatever the pair's camera)."""
    return tw.KF(np.eye(3), (0, 0, 0), 0), tw.KF(QUARTER.T, (0.5, 0, 0.25), 0)


def exact_make(cam, baseline, scale=None):
    """triangulate_worlds.exact_world's keyframes (power-of-two intrinsics, axis-aligned poses) with an exact second camera a quarter
    turn about y at the end of a 1/8 m arm.  Keyframe 2 lies `baseline` to the side of the pair's camera: along world x for a
    camera-1 pair, along world z for a camera-2 pair (whose x axis that is)."""
    kw = dict(fx=512.0, fy=512.0, cx=320.0, cy=240.0, mbf=32.0, scale=scale)
    t12 = np.array([0.125, 0.0, 0.0])
    kfs = []
    for tcw in ((0.0, 0.0, 0.0), (-baseline, 0.0, 0.0) if cam == 0 else (0.0, 0.0, -baseline)):
        kf = tw.KF(np.eye(3), tcw, 0, **kw)
        kf.Rcam12, kf.tcam12 = QUARTER.astype(f32), t12.astype(f32)
        kf.Tcw[1, :, :3], kf.Tcw[1, :, 3] = QUARTER.T, QUARTER.T @ (np.array(tcw) - t12)
        kf.centre[1] = -QUARTER @ kf.Tcw[1, :, 3].astype(f64)                  # -Rcw2.t() * tcw2 with Rcw2 = QUARTER.t()
        kfs.append(kf)
    return kfs


def feat(kf, x, y, octave=0, depth=None, cs=None):
    """One feature: the undistorted and the distorted keypoint coincide; stereo when a depth is given (uright = x - mbf / depth)."""
    x, y = f32(x), f32(y)
    if depth is None:
        return dict(x=x, y=y, xd=x, yd=y, oct=int(octave), ur=f32(-1.0), depth=f32(-1.0), cs=cs)
    return dict(x=x, y=y, xd=x, yd=y, oct=int(octave), ur=f32(f64(x) - f64(kf.mbf) / f64(depth)), depth=f32(depth), cs=cs)


def seen(make, cam, u, v, z, oct1=0, oct2=0, stereo1=False, stereo2=False, cs=None):
    """The two features of the point that camera `cam` of keyframe 1 sees at pixel (u, v) and depth z, without noise."""
    kf1, kf2 = make()
    fx, fy, cx, cy = (f64(k) for k in (kf1.fx, kf1.fy, kf1.cx, kf1.cy))
    Xc = np.array([(u - cx) / fx * z, (v - cy) / fy * z, z])
    Xw = (Xc - kf1.Tcw[cam, :, 3].astype(f64)) @ kf1.Tcw[cam, :, :3].astype(f64)
    X2 = kf2.Tcw[cam, :, :3].astype(f64) @ Xw + kf2.Tcw[cam, :, 3].astype(f64)
    return (feat(kf1, u, v, oct1, z if stereo1 else None, cs),
            feat(kf2, fx * X2[0] / X2[2] + cx, fy * X2[1] / X2[2] + cy, oct2, X2[2] if stereo2 else None, cs))


def load(kf, feats, n_cam1, cam_of=None):
    kf.n_cam1 = int(n_cam1)
    col = lambda k: [f[k] for f in feats]
    kf.set_features(col("x"), col("y"), col("xd"), col("yd"), col("oct"), col("ur"), col("depth"), cam_of)
    for i, f in enumerate(feats):
        if f["cs"] is not None:
            kf.cos_stereo[i] = f["cs"]            # cos_stereo is a free per-feature input of the stage


def single(make, cam, f1, f2, edit=None):
    """The world of one pair of camera `cam`; edit(kf1, kf2) changes the keyframes' constants."""
    kf1, kf2 = make()
    if edit is not None:
        edit(kf1, kf2)
    load(kf1, [f1], 1 - cam); load(kf2, [f2], 1 - cam)
    return tw.World(kf1, kf2, [[0, 0]])


def host1(make, cam, f1, f2, edit=None):
    r = single(make, cam, f1, f2, edit).host()[0]
    return int(r["outcome"]), int(r["path"])


def trace1(make, cam, f1, f2, edit=None):
    traces = []
    single(make, cam, f1, f2, edit).model(traces=traces)
    return traces[0]


class Rig:
    """Keyframe constants with the cases (feature pairs) collected on them -> one world."""

    def __init__(self, name, make):
        self.name, self.make, self.cases = name, make, []

    def add(self, group, side, cam, f1, f2, outcome=None, path=None):
        self.cases.append(dict(group=group, side=side, cam=cam, f1=dict(f1), f2=dict(f2), outcome=outcome, path=path))

    def world(self):
        """Camera-1 features first in both keyframes, as the reference numbers them; pair k = case k."""
        kf1, kf2 = self.make()
        order = sorted(range(len(self.cases)), key=lambda k: self.cases[k]["cam"])          # (stable)
        n1 = sum(c["cam"] == 0 for c in self.cases)
        where = np.empty(len(order), np.int64); where[order] = np.arange(len(order))
        load(kf1, [self.cases[k]["f1"] for k in order], n1); load(kf2, [self.cases[k]["f2"] for k in order], n1)
        return tw.World(kf1, kf2, np.stack([where, where], 1))


def _stereo_flag(rig, cam):
    """`uright >= 0` on a far point (mono: low parallax), whose stereo feature is unprojected (its cosine below the rays')."""
    f1, f2 = seen(rig.make, cam, 300.0, 200.0, 25.0)
    assert host1(rig.make, cam, f1, f2) == (tm.LOW_PARALLAX, NOPATH)
    cs = down(trace1(rig.make, cam, f1, f2)["cos_rays"])
    tiny = np.finfo(f32).tiny
    values = (("-0.0", f32(-0.0), True), ("+0.0", f32(0.0), True), ("smallest positive denormal", up(0), True),
              ("smallest negative denormal", down(0), False), ("-FLT_MIN", f32(-tiny), False))
    for k in (1, 2):
        for name, ur, stereo in values:
            g = dict((f1, f2)[k - 1], ur=ur, depth=f32(25.0), cs=cs)           # depth positive: the validation demands it of a stereo feature
            pair = (g, f2) if k == 1 else (f1, g)
            rig.add("stereo flag, keyframe %d" % k, name, cam, *pair, path=(U1, U2)[k - 1] if stereo else NOPATH)


def _rays_against_stereo(rig, cam):
    """`cosParallaxRays < cosParallaxStereo` with cos_stereo[idx] at the model's cos_rays and one float either side."""
    f1, f2 = seen(rig.make, cam, 340.0, 260.0, 3.0, stereo1=True, stereo2=True)
    m1, m2 = dict(f1, ur=f32(-1.0), depth=f32(-1.0)), dict(f2, ur=f32(-1.0), depth=f32(-1.0))
    cr = trace1(rig.make, cam, m1, m2)["cos_rays"]
    for side, cs in (("below", down(cr)), ("equal", cr), ("above", up(cr))):
        rig.add("rays < stereo cosine, stereo in keyframe 1", side, cam, dict(f1, cs=cs), m2, path=SVD if side == "above" else U1)
        rig.add("rays < stereo cosine, stereo in keyframe 2 only", side, cam, m1, dict(f2, cs=cs), path=SVD if side == "above" else U2)
        # both stereo: keyframe 2's cosine is never read (`else if(bStereo2)`); it is set where reading it would change the path
        rig.add("rays < stereo cosine, both stereo", side, cam, dict(f1, cs=cs), dict(f2, cs=up(cr) if side != "above" else down(cr)),
                path=SVD if side == "above" else U1)


def _stereo_orderings(rig, cam):
    """`cosParallaxStereo1 < cosParallaxStereo2` and `2 < 1`: reached only when the triangulation is not (here: rays at 90 degrees,
    cos_rays = 0), against the other side's cos_rays + 1."""
    kf1, kf2 = rig.make()
    p1, p2 = feat(kf1, kf1.cx, kf1.cy, 0, 2.0), feat(kf2, kf2.cx, kf2.cy, 0, 2.0)
    m1, m2 = feat(kf1, kf1.cx, kf1.cy), feat(kf2, kf2.cx, kf2.cy)
    t = trace1(rig.make, cam, m1, m2)
    assert t["cos_rays"] == 0
    other = t["cos_stereo2"]                                   # cosParallaxRays + 1 of the model
    for side, cs in (("below", down(other)), ("equal", other), ("above", up(other))):
        rig.add("stereo cosine 1 < 2", side, cam, dict(p1, cs=cs), m2, path=U1 if side == "below" else NOPATH)
        rig.add("stereo cosine 2 < 1", side, cam, m1, dict(p2, cs=cs), path=U2 if side == "below" else NOPATH)
        # both stereo: keyframe 2's own cosine (set below every other) is never read, its cosParallaxStereo2 stays cos_rays + 1 -- and
        # with keyframe 1's cosine above that, it is keyframe 2's feature that is unprojected
        rig.add("stereo cosines, both stereo", side, cam, dict(p1, cs=cs), dict(p2, cs=down(down(other))),
                path={"below": U1, "equal": NOPATH, "above": U2}[side])


def _rays_positive(rig, cam):
    """`cosParallaxRays > 0` at exactly 0 and at its float neighbours, by bisecting keyframe 1's x."""
    kf1, kf2 = rig.make()
    m1, m2 = feat(kf1, kf1.cx, kf1.cy), feat(kf2, kf2.cx, kf2.cy)
    at = lambda x: dict(m1, x=f32(x), xd=f32(x))
    is_svd = lambda x: host1(rig.make, cam, at(x), m2)[1] == SVD
    far = [x for x in (kf1.cx - f32(8), kf1.cx + f32(8)) if is_svd(x)]
    assert len(far) == 1 and not is_svd(kf1.cx)
    x_pos, x_not = cross(is_svd, far[0], kf1.cx)
    x_neg = np.nextafter(kf1.cx, kf1.cx - (far[0] - kf1.cx))
    cos = lambda x: trace1(rig.make, cam, at(x), m2)["cos_rays"]
    assert cos(x_pos) > 0 and cos(kf1.cx) == 0 and cos(x_neg) < 0 and not cos(x_not) > 0
    rig.add("rays > 0", "positive", cam, at(x_pos), m2, path=SVD)
    rig.add("rays > 0", "zero", cam, m1, m2, path=NOPATH)
    if x_not != kf1.cx:
        rig.add("rays > 0", "first not positive", cam, at(x_not), m2, path=NOPATH)
    rig.add("rays > 0", "negative", cam, at(x_neg), m2, path=NOPATH)


def _rays_09998(rig, cam):
    """Both features mono: cos_rays at the two floats next to the double 0.9998, by bisecting keyframe 2's x."""
    f1, f2 = seen(rig.make, cam, 300.0, 200.0, 14.0)
    at = lambda x: dict(f2, x=f32(x), xd=f32(x))
    is_svd = lambda x: host1(rig.make, cam, f1, at(x))[1] == SVD
    xs = [f32(f2["x"] + f32(d)) for d in range(-40, 41)]
    ans = [is_svd(x) for x in xs]
    k = next(k for k in range(len(xs) - 1) if ans[k] != ans[k + 1])
    x_svd, x_low = cross(is_svd, *((xs[k], xs[k + 1]) if ans[k] else (xs[k + 1], xs[k])))
    c_svd, c_low = (trace1(rig.make, cam, f1, at(x))["cos_rays"] for x in (x_svd, x_low))
    assert f64(c_svd) < f64(0.9998) < f64(c_low) and up(c_svd) == c_low, (c_svd, c_low)
    rig.add("rays < 0.9998", "below", cam, f1, at(x_svd), path=SVD)
    rig.add("rays < 0.9998", "above", cam, f1, at(x_low), path=NOPATH)
    # a stereo pair at the same cosine: the clause must not touch it
    rig.add("rays < 0.9998", "above, stereo", cam, seen(rig.make, cam, 300.0, 200.0, 14.0, stereo1=True, cs=up(c_low))[0], at(x_low), path=SVD)


ACCEPTING = (tm.ACCEPTED, tm.SCALE, tm.ZERO_DIST)


def _reprojection(rig, cam):
    """The four gates (keyframe 1 / 2, mono 5.991 / stereo 7.8) at octaves 0, 3 and 7, by bisecting the measured x (and uright) of the
    gate's feature.  On an unprojection path (the stereo cosine set to 1/2: every stereo feature wins) the measured pixel does not
    feed the point; `svd` cases (both mono) are those where it does, and there the measured y is bisected: the baseline runs along x, so
    a change of x moves the point along its ray and leaves both errors small."""
    half = f32(0.5)
    sf = tw.scale_factors()

    def gate(group, k, f1, f2, field, path, reach=6.0):
        rejected, later = (tm.REPROJ1, tm.REPROJ2)[k - 1], ((tm.REPROJ2,) + ACCEPTING, ACCEPTING)[k - 1]
        g0 = (f1, f2)[k - 1]
        move = lambda v: dict(g0, **{field: f32(v)})
        pair = lambda v: (move(v), f2) if k == 1 else (f1, move(v))
        pred = lambda v: host1(rig.make, cam, *pair(v))[0] == rejected
        far = f32(g0[field] + f32(reach) * sf[g0["oct"]])
        v_rej, v_ok = cross(pred, far, g0[field])
        rig.add(group, "rejected", cam, *pair(v_rej), outcome=(rejected,), path=path)
        rig.add(group, "passes", cam, *pair(v_ok), outcome=later, path=path)

    for o in (0, 3, 7):
        s1, s2 = seen(rig.make, cam, 300.0 + 9 * o, 220.0, 6.0, o, o, True, True, cs=half)
        m1, m2 = dict(s1, ur=f32(-1.0), depth=f32(-1.0)), dict(s2, ur=f32(-1.0), depth=f32(-1.0))
        gate("reprojection 1 mono, octave %d, unproject 2" % o, 1, m1, s2, "x", U2)
        gate("reprojection 1 stereo x, octave %d, unproject 1" % o, 1, s1, m2, "x", U1)
        gate("reprojection 1 stereo uright, octave %d, unproject 1" % o, 1, s1, m2, "ur", U1)
        gate("reprojection 2 mono, octave %d, unproject 1" % o, 2, s1, m2, "x", U1)
        gate("reprojection 2 stereo x, octave %d, unproject 1" % o, 2, s1, s2, "x", U1)
        gate("reprojection 2 stereo uright, octave %d, unproject 1" % o, 2, s1, s2, "ur", U1)
    for o in (0, 3, 7):
        a1, a2 = seen(rig.make, cam, 350.0, 250.0 + 9 * o, 3.0, o, 7)
        gate("reprojection 1 mono, octave %d, svd" % o, 1, a1, a2, "y", SVD, 10.0)
    for o in (0, 3, 7):           # (octave 7 against octave 7 in keyframe 1: the error splits, and keyframe 2's share crosses its gate first
        a1, a2 = seen(rig.make, cam, 370.0, 250.0 + 9 * o, 3.0, 7, o)                      # between 4 and 5 scale factors)
        gate("reprojection 2 mono, octave %d, svd" % o, 2, a1, a2, "y", SVD, 8.0 if o < 7 else 5.0)


@functools.lru_cache(maxsize=None)
def main_rig():
    rig = Rig("main", main_make)
    for cam in (0, 1):
        _stereo_flag(rig, cam)
        _rays_against_stereo(rig, cam)
        _rays_09998(rig, cam)
        _reprojection(rig, cam)
    return rig


@functools.lru_cache(maxsize=None)
def ortho_rig():
    rig = Rig("ortho", ortho_make)
    for cam in (0, 1):
        _stereo_orderings(rig, cam)
        _rays_positive(rig, cam)
    return rig


# ---- side worlds: a boundary in a per-keyframe quantity ----------------------------------------------------------------------------------
def exact_pair(cam, baseline, stereo1, stereo2, scale=None, oct1=0, oct2=0):
    """The point at (1, 2, 4) of the pair's camera of keyframe 1: pixel (448, 496), disparity 8; every quantity exact in float."""
    make = functools.partial(exact_make, cam, baseline, scale)
    kf1, kf2 = make()
    u2 = 448.0 - 128.0 * baseline if cam == 0 else 448.0 + 128.0 * baseline
    return make, feat(kf1, 448.0, 496.0, oct1, 4.0 if stereo1 else None), feat(kf2, u2, 496.0, oct2, 4.0 if stereo2 else None)


def _depth_signs(cam):
    """`z1 <= 0`, `z2 <= 0` -> [(group, side, world, outcomes allowed, path, outcomes excluded)].  z = R.row(2).dot(x3D) + t(2) of the
    pair's camera.  On an unprojection path x3D does not depend on [R|t], so t(2) = -R.row(2).dot(x3D) cancels the sum exactly (the
    exact world), and the floats either side come from bisecting t(2).  On the SVD path the point moves with t(2), and z changes its
    sign where the null vector's w does, from a large positive to a large negative value: t(2) is scanned for a change between
    `behind` and an outcome that needs z > 0, and bisected there; an exact zero is not to be had."""
    out = []

    def edit(k, t):
        def apply(kf1, kf2):
            (kf1, kf2)[k - 1].Tcw[cam, 2, 3] = f32(t)
        return apply

    make, f1, f2 = exact_pair(cam, 1.0 / 32, True, False)
    for k, behind in ((1, tm.Z1), (2, tm.Z2)):
        kf = make()[k - 1]
        t0 = kf.Tcw[cam, 2, 3]
        pred = lambda t: host1(make, cam, f1, f2, edit(k, t))[0] == behind
        z = lambda t: trace1(make, cam, f1, f2, edit(k, t))["z%d" % k]
        t_zero = f32(-tm.row_dot([f32(v) for v in kf.Tcw[cam, 2, :3]], trace1(make, cam, f1, f2)["x3D"]))
        t_behind, t_front = cross(pred, t_zero, t0)
        assert t_behind == t_zero and z(t_zero) == 0 and z(t_front) > 0 and z(down(t_zero)) < 0
        for side, t in (("zero", t_zero), ("positive", t_front), ("negative", down(t_zero))):
            out.append(("z%d <= 0, unproject 1" % k, side, single(make, cam, f1, f2, edit(k, t)), None if side == "positive" else (behind,), U1,
                        (behind,) if side == "positive" else None))
    make = sideways_make(cam)
    for k, behind in ((1, tm.Z1), (2, tm.Z2)):
        in_front = (tm.REPROJ1, tm.REPROJ2, tm.ZERO_DIST, tm.SCALE, tm.ACCEPTED) + ((tm.Z2,) if k == 1 else ())
        t0 = make()[k - 1].Tcw[cam, 2, 3]
        hit = None
        for u, v, depth in ((350.0, 250.0, 3.0), (100.0, 250.0, 1.0), (560.0, 250.0, 1.0)):
            f1, f2 = seen(make, cam, u, v, depth)
            outcome = lambda t: host1(make, cam, f1, f2, edit(k, t))[0]
            ts = [f32(t0 + f32(0.125 * j)) for j in range(-48, 49)]
            outs = [outcome(t) for t in ts]
            for j in range(len(ts) - 1):
                pair = {outs[j]: ts[j], outs[j + 1]: ts[j + 1]}
                if hit is None and behind in pair and len(pair) == 2 and (set(pair) - {behind}) <= set(in_front):
                    hit = (f1, f2) + cross(lambda t: outcome(t) == behind, pair[behind], pair[(set(pair) - {behind}).pop()])
        assert hit is not None, (cam, k)
        f1, f2, t_behind, t_front = hit
        zb, zf = (trace1(make, cam, f1, f2, edit(k, t))["z%d" % k] for t in (t_behind, t_front))
        assert zb < 0 < zf
        out.append(("z%d <= 0, svd" % k, "negative", single(make, cam, f1, f2, edit(k, t_behind)), (behind,), SVD, None))
        out.append(("z%d <= 0, svd" % k, "positive", single(make, cam, f1, f2, edit(k, t_front)), in_front, SVD, None))
    return out


def _scale_gates(cam):
    """`ratioDist * ratioFactor < ratioOctave` (near) and `ratioDist > ratioOctave * ratioFactor` (far): the centre is an input of its
    own, so one component of kf2.centre is scanned for the changes accepted <-> scale and bisected at each."""
    out = []
    for oct1, oct2 in ((0, 0), (2, 5), (6, 1)):
        f1, f2 = seen(main_make, cam, 330.0, 250.0, 3.0, oct1, oct2)
        found = {}
        for comp in (2, 0, 1):
            def edit(v, comp=comp):
                def apply(kf1, kf2):
                    kf2.centre[cam, comp] = f32(v)
                return apply
            accepted = lambda v: host1(main_make, cam, f1, f2, edit(v))[0] == tm.ACCEPTED
            c0 = main_make()[1].centre[cam, comp]
            vals = [f32(c0 + f32(0.5 * k)) for k in range(-80, 81)]
            outs = [host1(main_make, cam, f1, f2, edit(v))[0] for v in vals]
            assert set(outs) <= {tm.ACCEPTED, tm.SCALE}
            for k in range(len(vals) - 1):
                if outs[k] != outs[k + 1]:
                    a, r = (vals[k], vals[k + 1]) if outs[k] == tm.ACCEPTED else (vals[k + 1], vals[k])
                    v_acc, v_rej = cross(accepted, a, r)
                    t = trace1(main_make, cam, f1, f2, edit(v_rej))
                    gate = "near" if t["low"] < t["ratio_octave"] else "far"
                    assert (gate == "far") == bool(t["ratio_dist"] > t["high"])
                    if gate not in found:
                        found[gate] = [(side, single(main_make, cam, f1, f2, edit(v))) for side, v in (("accepted", v_acc), ("rejected", v_rej))]
            if len(found) == 2:
                break
        assert sorted(found) == ["far", "near"], (cam, oct1, oct2, sorted(found))
        for gate, sides in found.items():
            for side, w in sides:
                out.append(("scale gate %s, octaves %d %d" % (gate, oct1, oct2), side, w, (tm.ACCEPTED,) if side == "accepted" else (tm.SCALE,), SVD, None))
    # exact equality: the power-of-two scale table EXACT_SCALE (ratioFactor = 3), octaves 0 and 0 (ratioOctave 1), the unprojected point
    # (1, 2, 4) of the pair's camera, the centres straight below it at exactly representable distances.  far: distances 1 and 3,
    # ratioDist = 3 == 1 * 3.  near: distances 3 and 1, ratioDist = fl(1 / 3), and fl(1 / 3) * 3 rounds to 1.0f == ratioOctave.
    for gate, o1, d1, d2 in (("near", 0, 3.0, 1.0), ("far", 0, 1.0, 3.0)):
        make, f1, f2 = exact_pair(cam, 1.0 / 32, True, False, EXACT_SCALE, o1, 0)
        x3D = np.array(trace1(make, cam, f1, f2)["x3D"], f64)

        def edit(y2):
            def apply(kf1, kf2):
                kf1.centre[cam] = x3D - (0, d1, 0)
                kf2.centre[cam] = x3D - (0, d2, 0)
                if y2 is not None:
                    kf2.centre[cam, 1] = f32(y2)
            return apply
        t = trace1(make, cam, f1, f2, edit(None))
        assert (t["low"] == t["ratio_octave"]) if gate == "near" else (t["ratio_dist"] == t["high"]), t
        y_eq = f32(x3D[1] - d2)
        accepted = lambda y: host1(make, cam, f1, f2, edit(y))[0] == tm.ACCEPTED
        y_acc, y_rej = cross(accepted, y_eq, f32(y_eq + (0.5 if gate == "near" else -0.5)))
        group = "scale gate %s, equality" % gate
        out.append((group, "equal", single(make, cam, f1, f2, edit(y_eq)), (tm.ACCEPTED,), U1, None))
        if y_acc != y_eq:
            out.append((group, "last accepted", single(make, cam, f1, f2, edit(y_acc)), (tm.ACCEPTED,), U1, None))
        out.append((group, "rejected", single(make, cam, f1, f2, edit(y_rej)), (tm.SCALE,), U1, None))
    return out


def _reprojection_equalities(cam):
    """An error of exactly 0 against a gate of exactly 0 (level_sigma2[7] set to 0 in the gate's keyframe): `0 > 0` passes.  It is the
    only equality the gates have: 5.991 * sigma2 and 7.8 * sigma2 are doubles that no float sum of squares equals otherwise."""
    out = []
    for stereo1, stereo2, path in ((True, False, U1), (False, True, U2)):
        make, f1, f2 = exact_pair(cam, 1.0 / 32, stereo1, stereo2, None, 7, 7)
        for k in (1, 2):
            def edit(sigma2, k=k):
                def apply(kf1, kf2):
                    (kf1, kf2)[k - 1].level_sigma2[7] = f32(sigma2)
                return apply
            t = trace1(make, cam, f1, f2, edit(0.0))
            assert t["err%d" % k] == 0 and t["gate%d" % k] == 0
            group = "reprojection %d %s, equality" % (k, "stereo" if (stereo1, stereo2)[k - 1] else "mono")
            out.append((group, "equal", single(make, cam, f1, f2, edit(0.0)), (tm.ACCEPTED,), path, None))
            # the other side: the measured x one float off, against the same gate of 0
            g = dict((f1, f2)[k - 1]); g["x"] = up(g["x"])
            pair = (g, f2) if k == 1 else (f1, g)
            out.append((group, "above", single(make, cam, *pair, edit(0.0)), ((tm.REPROJ1, tm.REPROJ2)[k - 1],), path, None))
    return out


def _cameras():
    """Features n_cam1 - 1 and n_cam1 with the camera taken from the index (no cam_of), from an explicit cam_of that says the same, and
    from one that says the opposite; one camera switched off, so that the pair's camera shows in the outcome."""
    out = []
    pairs = [seen(main_make, c, 320.0 + 10 * k, 240.0, 3.0) for k, c in enumerate((0, 0, 1, 1))]
    for name, cam_of, cams in (("from the index", None, (0, 1)), ("explicit", [0, 0, 1, 1], (0, 1)), ("explicit, opposite", [0, 1, 0, 1], (1, 0))):
        for enabled in ((1, 0), (0, 1)):
            kf1, kf2 = main_make()
            load(kf1, [p[0] for p in pairs], 2, cam_of); load(kf2, [p[1] for p in pairs], 2, cam_of)
            for i, side in ((1, "feature n_cam1 - 1"), (2, "feature n_cam1")):
                w = tw.World(kf1, kf2, [[i, i]], cam_enabled=enabled)
                off = not enabled[cams[i - 1]]
                out.append(("camera of a feature, %s" % name, "%s, camera %d off" % (side, 1 + enabled.index(0)), w,
                            (tm.CAM_OFF,) if off else None, None, None if off else (tm.CAM_OFF,)))
    return out


@functools.lru_cache(maxsize=None)
def tri_side_worlds():
    """[(group, side, world of one pair, outcomes allowed or None, path or None, outcomes excluded or None)]; camera-1 pairs, then
    camera-2 pairs, then the camera-of-a-feature worlds."""
    out = []
    for cam in (0, 1):
        for g, s, w, oc, pa, ex in _depth_signs(cam) + _scale_gates(cam) + _reprojection_equalities(cam):
            out.append(("%s, camera %d" % (g, cam + 1), s, w, oc, pa, ex))
    return out + _cameras()


@functools.lru_cache(maxsize=None)
def tri_worlds():
    """[(name, world, groups, sides)]: the main world, the 90-degree world, the side worlds; groups / sides per pair."""
    out = []
    for rig in (main_rig(), ortho_rig()):
        out.append((rig.name, rig.world(), ["%s, camera %d" % (c["group"], c["cam"] + 1) for c in rig.cases], [c["side"] for c in rig.cases]))
    for k, (g, s, w, _, _, _) in enumerate(tri_side_worlds()):
        out.append(("side %d: %s [%s]" % (k, g, s), w, [g], [s]))
    return out


BATCH_SLOTS = (0, 63, 64)        # first lane, last lane of the first wave, first lane of the second


def batch_orders():
    """Position in the batch: for every group of EVERY world (the main world, the 90-degree world, each side world) an order of that
    world's pairs, longer than 65, in which members of the group stand at positions 0, 63 and 64 of the launch.  A world of fewer
    than 66 pairs is repeated to that length (a pair may appear any number of times in a launch); a side world's one pair fills all
    66 positions.  -> [(index into tri_worlds(), group, order)]"""
    out = []
    for wi, (_, _, groups, _) in enumerate(tri_worlds()):
        n = len(groups)
        base = (list(range(n)) * (-(-66 // n)))[:max(n, 66)]
        for g in sorted(set(groups)):
            members = [k for k in range(n) if groups[k] == g]
            order = list(base)
            for slot, k in zip(BATCH_SLOTS, (members * 3)[:3]):
                order.append(order[slot]); order[slot] = k          # (what stood there moves to the end)
            out.append((wi, g, np.array(order)))
    return out


@functools.lru_cache(maxsize=None)
def tri_host():
    return [w.host() for _, w, _, _ in tri_worlds()]


def _tri_conditions(table):
    worlds, host = tri_worlds(), tri_host()
    seen_sides = {}
    # the rigs: expectations per case
    for (name, w, groups, sides), rec, rig in zip(worlds[:2], host[:2], (main_rig(), ortho_rig())):
        assert len(rec) == len(rig.cases) == len(groups)
        for k, c in enumerate(rig.cases):
            what = (name, groups[k], sides[k], tm.OUTCOME_NAMES[rec["outcome"][k]], tm.PATH_NAMES[rec["path"][k]])
            assert c["outcome"] is None or rec["outcome"][k] in c["outcome"], what
            assert c["path"] is None or rec["path"][k] == c["path"], what
            assert c["outcome"] is not None or c["path"] is not None, what
            seen_sides.setdefault(groups[k], []).append((sides[k], (c["outcome"], c["path"])))
    for (g, s, w, oc, pa, ex), rec in zip(tri_side_worlds(), host[2:]):
        what = (g, s, tm.OUTCOME_NAMES[rec["outcome"][0]], tm.PATH_NAMES[rec["path"][0]])
        assert len(rec) == 1
        assert oc is None or rec["outcome"][0] in oc, what
        assert ex is None or rec["outcome"][0] not in ex, what
        assert pa is None or rec["path"][0] == pa, what
        seen_sides.setdefault(g, []).append((s, (oc, pa, ex)))
    for g, members in seen_sides.items():
        assert len({answer for _, answer in members}) >= 2, ("a group needs both sides", g, members)
    # every listed decision, for a camera-1 pair and for a camera-2 pair
    required = ["stereo flag, keyframe 1", "stereo flag, keyframe 2", "rays < stereo cosine, stereo in keyframe 1",
                "rays < stereo cosine, stereo in keyframe 2 only", "rays < stereo cosine, both stereo", "stereo cosine 1 < 2", "stereo cosine 2 < 1",
                "stereo cosines, both stereo", "rays > 0", "rays < 0.9998", "z1 <= 0, svd", "z1 <= 0, unproject 1", "z2 <= 0, svd",
                "z2 <= 0, unproject 1", "scale gate near, equality", "scale gate far, equality"]
    required += ["reprojection %s, octave %d, %s" % (g, o, p) for o in (0, 3, 7) for g, p in (
        ("1 mono", "unproject 2"), ("1 stereo x", "unproject 1"), ("1 stereo uright", "unproject 1"), ("2 mono", "unproject 1"),
        ("2 stereo x", "unproject 1"), ("2 stereo uright", "unproject 1"), ("1 mono", "svd"), ("2 mono", "svd"))]
    required += ["reprojection %d %s, equality" % (k, s) for k in (1, 2) for s in ("mono", "stereo")]
    required += ["scale gate %s, octaves %d %d" % (g, a, b) for g in ("near", "far") for a, b in ((0, 0), (2, 5), (6, 1))]
    for g in required:
        for cam in (1, 2):
            assert "%s, camera %d" % (g, cam) in seen_sides, (g, cam)
    for g in ("from the index", "explicit", "explicit, opposite"):
        assert "camera of a feature, %s" % g in seen_sides
    for s in ("zero", "negative", "positive"):
        for k in (1, 2):
            for cam in (1, 2):
                assert s in [x for x, _ in seen_sides["z%d <= 0, unproject 1, camera %d" % (k, cam)]]
    # position in the batch
    orders = batch_orders()
    for wi, g, order in orders:
        assert all(worlds[wi][2][order[slot]] == g for slot in BATCH_SLOTS) and len(order) > 65
    assert {g for _, g, _ in orders} == set(seen_sides)                   # every group, not the main world's alone
    for g in sorted(seen_sides):
        table.append("  %-62s %s" % (g, ", ".join(s for s, _ in seen_sides[g])))
    table.append("triangulation: %d groups, %d cases (main world %d pairs, 90-degree world %d, %d side worlds), %d batch orders"
                 % (len(seen_sides), sum(len(v) for v in seen_sides.values()), len(host[0]), len(host[1]), len(host) - 2, len(orders)))
    return {g: len(v) for g, v in seen_sides.items()}


# ==================================================================================================== Sim3 inliers
FAR = np.finfo(f32).max
# (name, generate() arguments): sizes around the wave, both rigs, all four camera combinations, the scale fixed and free -- taken from
# sim3_worlds.generate BEFORE nudge
SIM3_BASES = (("n64_h8", dict(seed=41, n=64, s=1.0, cams=(0.0, 0.0), wrong=0.3, noise=1.0, rig="small", H=8)),
              ("n65_h16_fixed_wide", dict(seed=42, n=65, s=1.0, fix_scale=True, cams=(0.5, 0.0), wrong=0.3, noise=1.0, rig="wide", H=16)),
              ("n130_h33", dict(seed=43, n=130, s=0.7, cams=(0.0, 0.5), wrong=0.3, noise=1.0, rig="small", H=33)),
              ("n200_h64_fixed_wide", dict(seed=44, n=200, s=1.0, fix_scale=True, cams=(0.5, 0.5), wrong=0.3, noise=1.0, rig="wide", H=64)))


def sim3_host(worlds):
    import multi_orb_slam_amd as m
    return m.sim3_ransac_host([sw.to_problem(m, W) for W in worlds], order=m.SIM3_MATH_DEVICE)


def bit(masks, h, i):
    return bool((int(masks[h, i // 64]) >> (i % 64)) & 1)


def _sim3_lanes():
    """Every correspondence i carries a decision at hypothesis h(i) = i mod H: its threshold is the device-order model's err (rejected,
    `err < err`) or the next float above (accepted).  -> [(name, world, [(group, side, h, i, expected bit)])]"""
    out = []
    for name, kw in SIM3_BASES:
        W = sw.generate(**kw)
        n, H = len(W["x3dc1"]), len(W["triples"])
        _, _, e1, e2 = sm.evaluate(W, "device")
        idx = np.arange(n); h = idx % H
        for which, e in (("err1", e1[h, idx]), ("err2", e2[h, idx])):
            assert np.isfinite(e).all() and (e < FAR).all(), name
            for parity in (0, 1):
                rejected = idx % 2 == parity
                thr = np.where(rejected, e, np.nextafter(e, INF)).astype(f32)
                far = np.full(n, FAR, f32)
                Wn = dict(W, max_err1=thr if which == "err1" else far, max_err2=thr if which == "err2" else far)
                cases = [("sim3 %s at its threshold" % which, "rejected" if rejected[i] else "accepted", int(h[i]), int(i), not rejected[i])
                         for i in range(n)]
                out.append(("%s/%s/%s rejected" % (name, which, ("even", "odd")[parity]), Wn, cases))
    return out


def _sim3_integral():
    """The thresholds of the real form, F(int(9.210 * sigma2)) per octave: correspondence o (octave o in both keyframes) has one
    coordinate of x3dc2 bisected until its bit under hypothesis o flips, once with only err1 deciding and once with only err2.  The
    hypotheses are drawn from the other correspondences, so that the eight decisions do not touch each other."""
    out = []
    W0 = sw.generate(seed=45, n=40, s=1.0, noise=0.0, H=8)
    W0["triples"] = (sm.draw_triples(32, 8, sw.randi_stream(46)) + 8).astype(np.int32)
    assert (W0["octave"][:, :8] == np.arange(8)).all()
    for which in ("err1", "err2"):
        far = np.full(40, FAR, f32)
        W = dict(W0, max_err1=W0["max_err1"] if which == "err1" else far, max_err2=W0["max_err2"] if which == "err2" else far)
        inside, outside = W["x3dc2"].copy(), W["x3dc2"].copy()
        for o in range(8):
            def accepted(x, o=o):
                X = W["x3dc2"].copy(); X[o, 0] = f32(x)
                return bit(sim3_host([dict(W, x3dc2=X)])[0][1], o, o)
            x0 = W["x3dc2"][o, 0]
            inside[o, 0], outside[o, 0] = cross(accepted, x0, f32(x0 + f32(0.5)))
        group = "sim3 %s against the octave's integral threshold" % which
        out.append(("integral/%s/accepted" % which, dict(W, x3dc2=inside), [(group, "accepted, octave %d" % o, o, o, True) for o in range(8)]))
        out.append(("integral/%s/rejected" % which, dict(W, x3dc2=outside), [(group, "rejected, octave %d" % o, o, o, False) for o in range(8)]))
    return out


@functools.lru_cache(maxsize=None)
def sim3_problems():
    """[(name, world, cases)]; the last one is sim3_worlds' depth_zero (infinite and NaN errors), which carries no case of its own."""
    return _sim3_lanes() + _sim3_integral() + [("depth_zero", dict(sw.hand_built())["depth_zero"], [])]


@functools.lru_cache(maxsize=None)
def sim3_host_answers():
    return sim3_host([W for _, W, _ in sim3_problems()])


def _sim3_conditions(table):
    counts = {}
    shapes = set()
    for (name, W, cases), (rec, masks) in zip(sim3_problems(), sim3_host_answers()):
        n, H = len(W["x3dc1"]), len(W["triples"])
        assert len(rec) == H and masks.shape == (H, (n + 63) // 64)
        for group, side, h, i, expected in cases:
            assert bit(masks, h, i) == expected, (name, group, side, h, i)
            counts.setdefault(group, {}).setdefault(side.split(",")[0], 0)
            counts[group][side.split(",")[0]] += 1
        if "/err" in name and not name.startswith("integral"):
            assert len(cases) == n                     # every lane of every mask word carries a decision, the last bit of a partial word
            assert {(c[3] % 64) for c in cases} >= set(range(min(n, 64)))      # and bit 63 of a full one included
            shapes.add((n, H, bool(W["fix_scale"]), bool(W["cam1"].any()), bool(W["cam2"].any()), float(W["calib"][3, 0])))
    assert {s[0] for s in shapes} == {64, 65, 130, 200} and all(8 <= s[1] <= 64 for s in shapes)
    assert {s[2] for s in shapes} == {False, True} and len({s[5] for s in shapes}) == 2
    assert {(s[3], s[4]) for s in shapes} == {(False, False), (True, False), (False, True), (True, True)}
    for g in ("sim3 err1 at its threshold", "sim3 err2 at its threshold", "sim3 err1 against the octave's integral threshold",
              "sim3 err2 against the octave's integral threshold"):
        assert set(counts[g]) == {"accepted", "rejected"}, g
        table.append("  %-62s %s" % (g, ", ".join("%s %d" % kv for kv in sorted(counts[g].items()))))
    for g in counts:
        if "integral" in g:
            assert counts[g] == {"accepted": 8, "rejected": 8}
    table.append("sim3: %d problems, %d cases" % (len(sim3_problems()), sum(sum(c.values()) for c in counts.values())))
    return {g: sum(c.values()) for g, c in counts.items()}


# ==================================================================================================== pose flags
POSE_FLAG_WORLDS = ("mono_60", "stereo_60", "mixed_400", "rig_400")     # of pose_worlds.GENERATED; rig_400 with both cameras
EDGES_PER_WORLD = 3
EQUALITY_BUDGET = 40          # starts of the search for (float)chi2 == threshold, each one bisection of v and one model run


def pose_host(problems):
    import multi_orb_slam_amd as m
    return m.pose_optimize_host([pw.to_problem(m, P) for P in problems], order=m.POSE_ORDER_DEVICE)


def with_obs(P, edge, u=None, v=None):
    obs = P["obs"].copy()
    if u is not None:
        obs[edge, 0] = f32(u)
    if v is not None:
        obs[edge, 1] = f32(v)
    return dict(P, obs=obs)


def _pose_counts():
    """9, 10 and 11 edges: `n < 10` decides whether rounds 2 to 4 run."""
    out = []
    for kind in ("mono", "stereo", "mixed"):
        for n in (9, 10, 11):
            P = pw.generate(seed=70 + n, n=n, kind=kind, outliers=0.1, start=(0.02, 1.0))
            out.append(("%d edges, %s" % (n, kind), P, ("pose edge count", "%d %s" % (n, kind), None, 1 if n < 10 else 4)))
    return out


def _flag_source(name):
    kw = dict(pw.GENERATED)[name]
    return pw.with_mode(pw.generate(**kw), pm.ALL_CAMS if kw.get("two_cams") else pm.CAM0)


def _pose_flags():
    """For the edges whose final chi2 is nearest its threshold: the observed u bisected through the host routine until the edge's
    outlier flag flips; both adjacent problems are kept.  (The optimisation is iterative: the flip need not be monotone in u; the
    bisection ends at an adjacent differing pair all the same.)"""
    out = []
    for name in POSE_FLAG_WORLDS:
        P = _flag_source(name)
        tr = pm.Trace()
        _, flags = pm.optimize(P, "device", tr)
        sigma = 1.0 / math.sqrt(float(P["inv_level_sigma2"][0]))
        taken = 0
        for e in (int(k) for k in np.argsort(tr.margins[-1], kind="stable")):
            if taken == EDGES_PER_WORLD:
                break
            flag = lambda u, e=e: bool(pose_host([with_obs(P, e, u)])[0][1][e])
            u0 = P["obs"][e, 0]
            f0 = flag(u0)
            scale = sigma * float(f32(1.2)) ** int(P["octave"][e])
            tries = [f32(u0 + f32(d * scale)) for k in range(1, 17) for d in (0.25 * k, -0.25 * k)]
            u1 = next((u for u in tries if flag(u) != f0), None)
            if u1 is None:               # (an outlier whose error in v or uright alone exceeds the threshold: no u makes it an inlier)
                continue
            taken += 1
            u_out, u_in = cross(flag, *((u0, u1) if f0 else (u1, u0)))
            kind = "stereo" if P["obs"][e, 2] >= 0 else "mono"
            group = "pose outlier flag, %s" % kind
            out.append(("%s edge %d outlier" % (name, e), with_obs(P, e, u_out), (group, "outlier", e, None)))
            out.append(("%s edge %d inlier" % (name, e), with_obs(P, e, u_in), (group, "inlier", e, None)))
    return out


def _class_chi(P, e):
    """chi2 (double) of edge e at every classification of the call (device order)."""
    tr = pm.Trace()
    pm.optimize(P, "device", tr)
    return [float(c[e]) for c in tr.class_chi]


@functools.lru_cache(maxsize=None)
def pose_equality():
    """The optional item: a problem with (float)chi2 == 5.991f (mono) / 7.815f (stereo) at one of the four classifications of one edge,
    by a bounded search.  chi2 moves by tens to hundreds of its ulps per ulp of u, but by less than one per ulp of v once v sits at the
    edge's projection (the term in v is quadratic there).  The flag is not continuous in the observation -- an edge classified an
    outlier in an early round leaves the later rounds' optimisation -- so the round that decides is whichever crosses first: u is
    bisected to the flip of the flag, the deciding round r read off the model, v moved to the vertex of chi2_r(v) (a parabola through
    three model runs), u bisected again.  Then every start bisects v to the flip and looks at the last inlier with the model; the next
    start moves u by one float towards the projection.  -> {kind: (problem, edge) or None}, {kind: starts used}."""
    found, used = {}, {}
    for kind, name in (("mono", "mono_60"), ("stereo", "stereo_60")):
        P = _flag_source(name)
        th = f32(5.991) if kind == "mono" else f32(7.815)
        tr = pm.Trace()
        _, flags = pm.optimize(P, "device", tr)
        e = int(np.argsort(np.where(flags, np.inf, tr.margins[-1]), kind="stable")[0])          # the inlier nearest its threshold
        flag = lambda Q: bool(pose_host([Q])[0][1][e])
        scale = float(f32(1.2)) ** int(P["octave"][e])
        u0, v0 = P["obs"][e, 0], P["obs"][e, 1]
        found[kind], used[kind] = None, 0
        far_u = next((u for u in (f32(u0 + f32(6 * scale)), f32(u0 - f32(6 * scale))) if flag(with_obs(P, e, u=u))), None)
        if far_u is None or flag(P):
            continue
        u_out, u_in = cross(lambda u: flag(with_obs(P, e, u=u)), far_u, u0)
        c_out, c_in = _class_chi(with_obs(P, e, u=u_out), e), _class_chi(with_obs(P, e, u=u_in), e)
        r = next(k for k in range(4) if (f32(c_out[k]) > th) != (f32(c_in[k]) > th))
        v_star = v0
        for h in (f32(0.5), f32(0.1), f32(0.02)):                 # (the fit is repeated: chi2_r(v) is a parabola only near its vertex)
            lo, mid, hi = (_class_chi(with_obs(P, e, u=u_in, v=v), e)[r] for v in (f32(v_star - h), v_star, f32(v_star + h)))
            v_star = f32(float(v_star) - float(h) * (hi - lo) / (2 * (hi - 2 * mid + lo)))
        P = with_obs(P, e, v=v_star)
        if flag(P) or not flag(with_obs(P, e, u=far_u)):
            continue
        _, u_in = cross(lambda u: flag(with_obs(P, e, u=u)), far_u, u0)
        for start in range(EQUALITY_BUDGET):
            used[kind] = start + 1
            Q = with_obs(P, e, u=u_in)
            far_v = next((v for v in (f32(v_star + f32(0.05 * scale)), f32(v_star - f32(0.05 * scale))) if flag(with_obs(Q, e, v=v))), None)
            if far_v is not None and not flag(Q):
                _, v_in = cross(lambda v: flag(with_obs(Q, e, v=v)), far_v, v_star)
                cand = with_obs(Q, e, v=v_in)
                if th in [f32(c) for c in _class_chi(cand, e)]:
                    found[kind] = (cand, e)
                    break
            u_in = down(u_in) if u_in > u0 else up(u_in)
    return found, used


@functools.lru_cache(maxsize=None)
def pose_problems():
    """[(name, problem, (group, side, edge or None, rounds or None))]"""
    out = _pose_counts() + _pose_flags()
    for kind, hit in pose_equality()[0].items():
        if hit is not None:
            out.append(("chi2 == threshold, %s" % kind, hit[0], ("pose chi2 equal to its threshold", "equal, %s" % kind, hit[1], None)))
    return out


@functools.lru_cache(maxsize=None)
def pose_host_answers():
    return pose_host([P for _, P, _ in pose_problems()])


def _pose_conditions(table):
    counts = {}
    for (name, P, (group, side, edge, rounds)), (rec, flags) in zip(pose_problems(), pose_host_answers()):
        if rounds is not None:
            assert rec["rounds"] == rounds and rec["n_initial"] == len(P["feat"]), (name, int(rec["rounds"]))
        if side in ("outlier", "inlier"):
            assert bool(flags[edge]) == (side == "outlier"), name
        if side.startswith("equal"):
            assert not flags[edge], name                      # `chi2 > threshold`: equality is an inlier
        counts.setdefault(group, []).append(side)
    assert sorted(counts["pose edge count"]) == sorted("%d %s" % (n, k) for n in (9, 10, 11) for k in ("mono", "stereo", "mixed"))
    for kind in ("mono", "stereo"):
        sides = counts["pose outlier flag, %s" % kind]
        assert sides.count("outlier") == sides.count("inlier") >= EDGES_PER_WORLD
    # adjacent problems: one float of one observation apart
    flagged = [(n, P) for n, P, c in pose_problems() if c[1] in ("outlier", "inlier")]
    for (na, A), (nb, B) in zip(flagged[0::2], flagged[1::2]):
        d = np.flatnonzero(A["obs"].reshape(-1) != B["obs"].reshape(-1))
        assert len(d) == 1 and adjacent(A["obs"].reshape(-1)[d[0]], B["obs"].reshape(-1)[d[0]]), (na, nb)
    assert len(flagged) == 2 * EDGES_PER_WORLD * len(POSE_FLAG_WORLDS)
    found, used = pose_equality()
    for g in sorted(counts):
        table.append("  %-62s %d cases" % (g, len(counts[g])))
    for kind in found:
        table.append("  exact (float)chi2 == threshold, %s: %s after %d of %d starts" % (
            kind, "found" if found[kind] is not None else "not found", used[kind], EQUALITY_BUDGET))
    table.append("pose: %d problems" % len(pose_problems()))
    return {g: len(v) for g, v in counts.items()}


# ==================================================================================================== all of it
@functools.lru_cache(maxsize=None)
def check_conditions():
    """Asserts, on the host routine's answers, that every group is there with its sides and that each side answers what its name
    claims -> (the group and side table as text, {group: cases})."""
    table = []
    counts = dict(_tri_conditions(table))
    counts.update(_sim3_conditions(table))
    counts.update(_pose_conditions(table))
    assert all(v > 0 for v in counts.values())
    return "\n".join(table), counts
