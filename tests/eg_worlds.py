"""Seeded worlds of a closed trajectory for the essential graph (tests/test_eg_model.py, tests/test_gpu_essgraph.py): keyframes on a ring
whose odometry drifts in rotation, translation and, for the free-scale form, scale; a spanning tree (every keyframe to its predecessor),
covisibility edges to earlier keyframes, loop edges between the two ends, some pairs connected twice, ONE fixed vertex (the loop
keyframe) that is vertex 0 of some edges and vertex 1 of others, points with a reference vertex and some without.  A world is a dict of
the arrays of orbm_eg_problem; make_problem turns it into the binding's EssentialGraphProblem.

Vertices: the free ones first (ring positions 1 .. n_free, which stand for ascending mnId), then the fixed one (ring position 0)."""
import math
import numpy as np

from sim3opt_model import Sim3


def rot_sim3(axis, angle, t, s):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    h = 0.5 * angle
    return Sim3([float(a[0] * math.sin(h)), float(a[1] * math.sin(h)), float(a[2] * math.sin(h)), math.cos(h)], [float(v) for v in t], float(s))


def vec8(T):
    return list(T.q) + list(T.t) + [T.s]


def ring(n_free, seed, fix_scale=False, n_points=0, drift=1.0, consistent=False, covis=3, doubles=2, unreferenced=0.1):
    """n_free free keyframes and the fixed loop keyframe.  consistent: every measurement comes from the ground truth (the optimum has
    chi2 = 0) and the estimates start drifted; otherwise the measurements come from the drifted odometry except the loop edges, which
    come from the truth: what CorrectLoop hands over."""
    rng = np.random.default_rng(seed)
    n = n_free + 1
    radius = 5.0
    truth, drifted = [], []
    for k in range(n):                          # ring position k: Siw of a camera on the circle looking along the tangent
        ang = 2 * math.pi * k / n
        Swi = rot_sim3([0.1, 1.0, 0.05], ang, [radius * math.cos(ang), 0.2 * math.sin(3 * ang), radius * math.sin(ang)], 1.0)
        truth.append(Swi.inverse())
    acc = Sim3([0., 0., 0., 1.], [0., 0., 0.], 1.)
    for k in range(n):
        if k:
            err = rot_sim3(rng.normal(size=3), drift * 0.004 * rng.normal(), drift * 0.01 * rng.normal(size=3),
                           1.0 if fix_scale else math.exp(drift * 0.004 * rng.normal()))
            acc = err * acc
        drifted.append(acc * truth[k])
    pos = list(range(1, n)) + [0]               # vertex index -> ring position: the fixed vertex is last
    vid = {p: v for v, p in enumerate(pos)}
    est = [drifted[p] for p in pos]
    ev0, ev1, meas = [], [], []

    def add(pi, pj, source):                    # vertex 0 = Siw, vertex 1 = Sjw, the measurement Sji = Sjw * Swi
        ev0.append(vid[pi]); ev1.append(vid[pj])
        meas.append(vec8(source[pj] * source[pi].inverse()))

    src = truth if consistent else drifted
    add(n - 1, 0, truth)                        # step 3: the loop connection, the fixed vertex as vertex 1
    if n > 3:
        add(0, n - 2, truth)                    # ... and as vertex 0
    for k in range(1, n):                       # step 4
        add(k, k - 1, src)                      # spanning tree: the parent is the predecessor
        if k == n - 1 and n > 2:
            add(k, 0, truth)                    # the loop edge of the current keyframe (mnId of the loop keyframe is smaller)
        for j in rng.permutation(np.arange(max(0, k - 6), max(0, k - 1)))[:covis]:
            add(k, int(j), src)                 # covisibility edges to earlier keyframes
    for _ in range(doubles if n > 2 else 0):    # pairs connected twice, once in each direction
        k = int(rng.integers(1, n))
        add(k - 1, k, src)
    ref = rng.integers(0, n, size=n_points).astype(np.int32)
    ref[rng.random(n_points) < unreferenced] = -1
    if n_points:
        ref[0] = -1 if unreferenced > 0 else ref[0]
    points = (rng.normal(size=(n_points, 3)) * 4).astype(np.float32)
    return {"n_free": n_free, "vertex": np.array([vec8(T) for T in est]), "measurement": np.array(meas).reshape(-1, 8),
            "edge_v0": np.array(ev0, np.int32), "edge_v1": np.array(ev1, np.int32), "points": points, "point_ref": ref,
            "fix_scale": bool(fix_scale)}


def make_problem(m, W):
    return m.EssentialGraphProblem(W["n_free"], W["vertex"], W["measurement"], W["edge_v0"], W["edge_v1"], W["points"], W["point_ref"],
                                   W["fix_scale"])


def _with(W, **kw):
    out = dict(W)
    out.update(kw)
    return out


def log_branch_sims():
    """One Sim3 for each branch of Sim3::log(): (|sigma| < eps, d > 1 - eps), (|sigma| < eps), (d > 1 - eps), neither; then a rotation
    within 1e-3 of pi."""
    return [rot_sim3([1, 2, 3], 1e-4, [0.3, -0.2, 0.1], 1.0 + 1e-7), rot_sim3([1, 2, 3], 0.7, [0.3, -0.2, 0.1], 1.0 - 2e-7),
            rot_sim3([3, -1, 2], 2e-4, [0.3, -0.2, 0.1], 1.3), rot_sim3([3, -1, 2], 1.1, [0.3, -0.2, 0.1], 0.8),
            rot_sim3([0.2, 1, -0.4], math.pi - 5e-4, [0.3, -0.2, 0.1], 1.05)]


def hand_cases():
    """name -> (world, iterations)"""
    cases = {}
    sims = log_branch_sims()
    for b, T in enumerate(sims):                # two free vertices and the fixed one, the first edge's error in the wanted branch
        W = ring(2, 40 + b, n_points=3)
        v0, v1 = Sim3(*_parts(W["vertex"][W["edge_v0"][0]])), Sim3(*_parts(W["vertex"][W["edge_v1"][0]]))
        M = W["measurement"].copy()
        M[0] = vec8(T * v1 * v0.inverse())      # C * v0 * v1^-1 = T
        cases["log_branch_%d" % b if b < 4 else "near_pi"] = (_with(W, measurement=M), 3)
    W = ring(3, 51, n_points=4)
    two_fixed = _with(W, n_free=2)              # the last free vertex becomes fixed: its edges to the fixed one have no Jacobian
    cases["edge_between_fixed"] = (two_fixed, 4)
    W = ring(4, 52, n_points=4)
    V = np.concatenate([W["vertex"][:4], [vec8(rot_sim3([1, 1, 0], 0.3, [9., 9., 9.], 1.1))], W["vertex"][4:]])
    V[4][:4] *= 1.0 + 1e-9                      # not a unit quaternion: returned as it came
    shift = lambda a: np.where(a >= 4, a + 1, a).astype(np.int32)
    cases["vertex_without_edge"] = (_with(W, n_free=5, vertex=V, edge_v0=shift(W["edge_v0"]), edge_v1=shift(W["edge_v1"]),
                                          point_ref=np.array([4, -1, 5, 0], np.int32)), 4)
    W = ring(3, 53, n_points=2)
    cases["no_edges"] = (_with(W, measurement=np.zeros((0, 8)), edge_v0=np.zeros(0, np.int32), edge_v1=np.zeros(0, np.int32)), 5)
    cases["zero_iterations"] = (ring(4, 54, n_points=3), 0)
    W = ring(4, 55, n_points=3)              # every estimate and every measurement the identity: every error is exactly 0
    ident = [0., 0., 0., 1., 0., 0., 0., 1.]
    cases["exact_optimum"] = (_with(W, vertex=np.array([ident] * len(W["vertex"])), measurement=np.array([ident] * len(W["measurement"]))), 5)
    W = ring(4, 56, n_points=3)
    M = W["measurement"].copy()
    M[2][4] = float("nan")
    cases["every_solve_fails"] = (_with(W, measurement=M), 3)
    cases["fix_scale_column"] = (ring(3, 57, fix_scale=True, n_points=3), 2)
    cases["fix_scale_compute_scale"] = (ring(5, 58, fix_scale=True, n_points=3, drift=4.0), 6)
    W = ring(3, 59, n_points=6)
    pts = W["points"].copy()
    pts[2] = [-0.0, 1.5, -0.0]                  # through two identities a -0.0 comes back as +0.0
    cases["unreferenced_points"] = (_with(W, points=pts, point_ref=np.array([-1, 0, -1, 3, 2, -1], np.int32)), 2)
    return cases


def _parts(v8):
    return [float(x) for x in v8[:4]], [float(x) for x in v8[4:7]], float(v8[7])
