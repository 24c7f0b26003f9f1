"""A float64 model of Optimizer::LocalBundleAdjustment (reference src/Optimizer.cc:921-1353) from its graph on, and of the parts of g2o
it runs, written from the reference's and g2o's sources (Thirdparty/g2o/g2o/: types/types_six_dof_expmap.{h,cpp}: EdgeSE3ProjectXYZ,
EdgeStereoSE3ProjectXYZ; core/base_binary_edge.hpp: constructQuadraticForm; core/block_solver.hpp: buildSystem, setLambda,
restoreDiagonal, solve; core/optimization_algorithm_levenberg.cpp; core/sparse_optimizer.cpp: initializeOptimization, optimize) -- not
from csrc/lba.hip: the loops below are g2o's nested loops (optimize -> solve -> trials) over NumPy columns of edges, not a sequence of
steps over a view.

Every per-edge operation is an element-wise IEEE + - * / of float64 (where the reference computes in float: float32) columns, which
NumPy rounds exactly as the scalar operation; a sum whose order matters is an explicit np.add.accumulate (strictly sequential; np.sum is
pairwise and is not used) or a loop; what happens once per trial is Python float arithmetic with the C library's math functions.

order="index":  the total chi2 is summed over the active edges in ascending edge position; sin, cos and pow(., 3) from the C library.
order="device": the total chi2 in the kernels' tree (edge positions 256 k .. 256 k + 255: an xor butterfly 1 .. 32 inside each group of
                64, the four groups in order, an inactive edge counting 0.0; then the partials in ascending k); sine and cosine from the
                fixed polynomial sequence of pose_model.py, the cube by multiplication.

The stated deviations of include/orbm.h are the model's too: the reduced system is solved by a dense LDL^T without pivoting in the natural
order, every inner product sequential in ascending index, failing on a zero or non-finite pivot; Matrix3d::inverse() is the cofactor form;
the products inside Eigen's small matrix expressions run in ascending index."""
import math
import numpy as np

from pose_model import SE3, quat_rotate, quat_to_matrix, canonical, DBL_MAX, LANES, ROUND_DTYPE

ENDED_COMPLETE, ENDED_STOPPED_AT_START, ENDED_NO_SECOND = 0, 1, 2
FLAG_LEVEL1, FLAG_ERASE = 1, 2
TH_MONO, TH_STEREO = 5.991, 7.815


class Result:
    FIELDS = ("pose", "Tcw", "point", "point_f", "flags", "rounds", "ended", "optimisations", "polls", "n_level1", "n_erase", "active_poses",
              "active_points", "active_edges")


class Trace:
    def __init__(self):
        self.tests = []        # per test: (chi2 per edge, depth per edge, tested mask)
        self.exits = []        # why each iteration ended: "accepted", "qmax", "rho0", "stopped"; plus "three_bad", "max_iter", "stop_376"
        self.solve_failed = 0
        self.trials = []       # (stage, iteration, lambda, rho, ok2)


def huber_constants():
    """`const float thHuberMono = sqrt(5.991)`; rk->setDelta(th): _delta the float as a double, dsqr the float member."""
    out = []
    for th2 in (TH_MONO, TH_STEREO):
        delta = float(np.float32(math.sqrt(th2)))
        out.append((delta, float(np.float32(delta * delta))))
    return out


def inverse3(m):
    """Matrix3d::inverse(): the cofactor form; m, result: nested 3 x 3 of floats or columns."""
    def cof(i, j):
        i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
        return m[i1][j1] * m[i2][j2] - m[i1][j2] * m[i2][j1]
    c00, c10, c20 = cof(0, 0), cof(1, 0), cof(2, 0)
    det = (c00 * m[0][0] + c10 * m[1][0]) + c20 * m[2][0]
    invdet = 1.0 / det
    return [[c00 * invdet, c10 * invdet, c20 * invdet],
            [cof(0, 1) * invdet, cof(1, 1) * invdet, cof(2, 1) * invdet],
            [cof(0, 2) * invdet, cof(1, 2) * invdet, cof(2, 2) * invdet]]


def ldlt_solve(H, b):
    """The dense LDL^T without pivoting: H n x n (its upper triangle is read), -> x or None on a zero or non-finite pivot."""
    n = len(b)
    L = np.zeros((n, n)); d = np.zeros(n)
    for k in range(n):
        temp = d[:k] * L[k, :k]
        prods = L[k:, :k] * temp
        sums = np.add.accumulate(np.concatenate([np.zeros((n - k, 1)), prods], axis=1), axis=1)[:, -1]
        dk = H[k, k] - sums[0]
        if not (abs(dk) > 0) or not (abs(dk) <= DBL_MAX):
            return None
        d[k] = dk
        L[k + 1:, k] = (H[k, k + 1:] - sums[1:]) / dk
    y = np.zeros(n)
    for i in range(n):
        s = np.add.accumulate(np.concatenate([[0.0], L[i, :i] * y[:i]]))[-1]
        y[i] = b[i] - s
    y = y / d
    for i in range(n - 1, -1, -1):
        s = np.add.accumulate(np.concatenate([[0.0], L[i + 1:, i] * y[i + 1:]]))[-1]
        y[i] = y[i] - s
    return y


def ranked_sum(terms, owner, n_owner):
    """Per owner the sum of its rows of `terms` in row order, starting from 0.0 -> n_owner x K."""
    out = np.zeros((n_owner,) + terms.shape[1:])
    if len(owner) == 0:
        return out
    idx = np.argsort(owner, kind="stable")
    so = owner[idx]
    start = np.searchsorted(so, so, side="left")
    rank = np.arange(len(so)) - start
    for r in range(int(rank.max()) + 1):
        sel = idx[rank == r]
        out[owner[sel]] = out[owner[sel]] + terms[sel]
    return out


def tree_partial(leaf):
    lanes = np.zeros(LANES); lanes[:len(leaf)] = leaf
    for off in (1, 2, 4, 8, 16, 32):
        lanes = lanes + lanes[np.arange(LANES) ^ off]
    return ((lanes[0] + lanes[64]) + lanes[128]) + lanes[192]


def raw_se3(q, t):
    """An SE3Quat as it is stored: the vertex's estimate is read, not constructed again (no second normalizeRotation)."""
    T = object.__new__(SE3)
    T.q, T.t = [float(v) for v in q], [float(v) for v in t]
    return T


class Graph:
    """The constants of the edges as columns."""

    def __init__(self, W):
        self.n_free = int(W["n_free"])
        self.Tcw = np.asarray(W["Tcw"], np.float32).reshape(-1, 4, 4)
        self.K = np.asarray(W["K"], np.float32).reshape(-1, 5)
        self.first = np.asarray(W["first"], np.int64)
        self.n_poses, self.n_points, self.n_edges = len(self.Tcw), len(self.first) - 1, int(self.first[-1])
        self.edge_pose = np.asarray(W["edge_pose"], np.int64)
        self.edge_point = np.repeat(np.arange(self.n_points), np.diff(self.first))
        self.cam = np.asarray(W["edge_cam"], np.int64)
        obs = np.asarray(W["obs"], np.float32).reshape(-1, 3)
        self.stereo = ~(obs[:, 2] < 0)
        self.obs = obs.astype(np.float64)
        self.w = np.asarray(W["inv_sigma2"], np.float32).astype(np.float64)
        bad = W.get("bad")
        self.bad = np.zeros(self.n_points, bool) if bad is None else np.asarray(bad) != 0
        Kd = self.K.astype(np.float64)[self.edge_pose] if self.n_edges else np.zeros((0, 5))
        self.fx, self.fy, self.cx, self.cy, self.bf = (Kd[:, k] for k in range(5))
        self.bf32 = self.K[self.edge_pose, 4] if self.n_edges else np.zeros(0, np.float32)
        Tcim = np.asarray(W["Tcim"], np.float32).reshape(2, 4, 4)
        self.Tc = [SE3.from_cv(Tcim[c]) for c in range(2)]
        self.Rc = [quat_to_matrix(T.q) for T in self.Tc]
        self.huber = huber_constants()


def edge_pass(G, poses, points, sel, jacobian):
    """computeError (+ linearizeOplus) of the edges `sel` at the given estimates -> dict of columns."""
    ep, el = G.edge_pose[sel], G.edge_point[sel]
    q = [poses[ep, k] for k in range(4)]
    t = [poses[ep, 4 + k] for k in range(3)]
    X = [points[el, k] for k in range(3)]
    cam = G.cam[sel]; st = G.stereo[sel]
    fx, fy, cx, cy, bf = G.fx[sel], G.fy[sel], G.cx[sel], G.cy[sel], G.bf[sel]
    obs = G.obs[sel]; w = G.w[sel]
    r = quat_rotate(q, X)
    p = [r[k] + t[k] for k in range(3)]                       # v1->estimate().map(v2->estimate())
    pcs = []
    for c in range(2):                                         # Tcim_quat.map(...)
        rc = quat_rotate(G.Tc[c].q, p)
        pcs.append([rc[k] + G.Tc[c].t[k] for k in range(3)])
    pc = [np.where(cam == 0, pcs[0][k], pcs[1][k]) for k in range(3)]
    with np.errstate(all="ignore"):
        proj0, proj1 = pc[0] / pc[2], pc[1] / pc[2]            # mono: project2d, cam_project
        em = [obs[:, 0] - (proj0 * fx + cx), obs[:, 1] - (proj1 * fy + cy)]
        invz = (1.0 / pc[2]).astype(np.float32)                # stereo: `const float invz = 1.0f/trans_xyz[2]`
        r0 = pc[0] * invz.astype(np.float64) * fx + cx
        r1 = pc[1] * invz.astype(np.float64) * fy + cy
        r2 = r0 - (G.bf32[sel] * invz).astype(np.float64)      # bf*invz: a float product
        es = [obs[:, 0] - r0, obs[:, 1] - r1, obs[:, 2] - r2]
        e = [np.where(st, es[0], em[0]), np.where(st, es[1], em[1]), np.where(st, es[2], 0.0)]
        chi_m = e[0] * (w * e[0]) + e[1] * (w * e[1])
        chi2 = np.where(st, chi_m + e[2] * (w * e[2]), chi_m)
    out = {"e": e, "chi2": chi2, "zc": pc[2], "stereo": st, "w": w}
    if not jacobian:
        return out
    rm = quat_to_matrix(q)                                     # T.rotation().toRotationMatrix()
    rr = [[np.where(cam == 0, G.Rc[0][i][j], G.Rc[1][i][j]) for j in range(3)] for i in range(3)]
    x, y, z = p
    xc, yc, zc = pc
    with np.errstate(all="ignore"):
        zc_2 = zc * zc
        t100, t102 = -fx / zc, fx * xc / zc_2
        t111, t112 = -fy / zc, fy * yc / zc_2
        a1 = bf / zc_2
        t2 = [[t100 * rr[0][j] + t102 * rr[2][j] for j in range(3)], [t111 * rr[1][j] + t112 * rr[2][j] for j in range(3)]]
        t2.append([t2[0][j] - a1 * rr[2][j] for j in range(3)])
        A = [[t2[k][0] * rm[0][j] + t2[k][1] * rm[1][j] + t2[k][2] * rm[2][j] for j in range(3)] for k in range(3)]
        B = [[-t2[k][1] * z + t2[k][2] * y, t2[k][0] * z - t2[k][2] * x, -t2[k][0] * y + t2[k][1] * x, t2[k][0], t2[k][1], t2[k][2]]
             for k in range(3)]
    out["A"], out["B"] = A, B
    return out


def quadratic_form(G, ev, robust):
    """constructQuadraticForm of every evaluated edge -> bl n x 3, Hll n x 3 x 3, bp n x 6, Hpp n x 6 x 6, Hpl n x 6 x 3, rho0."""
    st, w, e, A, B, chi2 = ev["stereo"], ev["w"], ev["e"], ev["A"], ev["B"], ev["chi2"]
    n = len(w)
    with np.errstate(all="ignore"):
        rho0, rho1 = chi2.copy(), np.ones(n)
        for s, (delta, dsqr) in enumerate(G.huber):
            sel = robust & (st == bool(s)) & ~(chi2 <= dsqr)
            sq = np.sqrt(chi2)
            rho0 = np.where(sel, 2 * sq * delta - dsqr, rho0)
            rho1 = np.where(sel, delta / sq, rho1)
        omega_r = [-(w * e[k]) for k in range(3)]
        omega_r = [np.where(robust, omega_r[k] * rho1, omega_r[k]) for k in range(3)]
        rw = np.where(robust, w * rho1, w)

        def dot(a, b):
            two = a[0] * b[0] + a[1] * b[1]
            return np.where(st, two + a[2] * b[2], two)
        bl = np.stack([dot([A[k][i] for k in range(3)], omega_r) for i in range(3)], axis=1)
        Hll = np.stack([np.stack([dot([A[k][i] * rw for k in range(3)], [A[k][j] for k in range(3)]) for j in range(3)], axis=1)
                        for i in range(3)], axis=1)
        bp = np.stack([dot([B[k][r] for k in range(3)], omega_r) for r in range(6)], axis=1)
        Hpp = np.stack([np.stack([dot([B[k][r] * rw for k in range(3)], [B[k][c] for k in range(3)]) for c in range(6)], axis=1)
                        for r in range(6)], axis=1)
        # with a kernel: B^T * weightedOmega * A; without: B^T * (A^T * omega)^T
        Hpl = np.stack([np.stack([np.where(robust, dot([B[k][r] * rw for k in range(3)], [A[k][c] for k in range(3)]),
                                           dot([B[k][r] for k in range(3)], [A[k][c] * w for k in range(3)])) for c in range(3)], axis=1)
                        for r in range(6)], axis=1)
    return bl, Hll, bp, Hpp, Hpl, rho0


def schur_solve(Hll, bl, Hpp, bp, Bi, eh, lm_of, na, nl, lam):
    """setLambda on both diagonals and BlockSolver::solve (block_solver.hpp:353-486).  Hll nl x 3 x 3, bl, Hpp na x 6 x 6, bp: the undamped
    sums; Bi: the Hpl blocks (6 x 3) in active-edge order, eh / lm_of: their pose and landmark indices.  -> (xp, xl, Hschur, bschur) or
    None when the reduced system cannot be factorised."""
    with np.errstate(all="ignore"):             # (a singular landmark block divides by zero, as Eigen does)
        return _schur_solve(Hll, bl, Hpp, bp, Bi, eh, lm_of, na, nl, lam)


def _schur_solve(Hll, bl, Hpp, bp, Bi, eh, lm_of, na, nl, lam):
    n, nb = 6 * na, len(eh)
    D = Hll.copy()
    for k in range(3):
        D[:, k, k] = D[:, k, k] + lam
    Dinv = np.stack([np.stack(row, axis=1) for row in inverse3([[D[:, a, b] for b in range(3)] for a in range(3)])], axis=1) \
        if nl else np.zeros((0, 3, 3))
    db = np.stack([(Dinv[:, r, 0] * bl[:, 0] + Dinv[:, r, 1] * bl[:, 1]) + Dinv[:, r, 2] * bl[:, 2] for r in range(3)], axis=1) \
        if nl else np.zeros((0, 3))
    Hs = np.zeros((n, n)); coeff = np.zeros(n)
    Di = Dinv[lm_of] if nb else np.zeros((0, 3, 3))
    BD = np.stack([(Bi[:, :, 0] * Di[:, 0, c][:, None] + Bi[:, :, 1] * Di[:, 1, c][:, None]) + Bi[:, :, 2] * Di[:, 2, c][:, None]
                   for c in range(3)], axis=2) if nb else np.zeros((0, 6, 3))
    dbl = db[lm_of] if nb else np.zeros((0, 3))
    Bb_terms = (Bi[:, :, 0] * dbl[:, 0][:, None] + Bi[:, :, 1] * dbl[:, 1][:, None]) + Bi[:, :, 2] * dbl[:, 2][:, None]
    coeffs = ranked_sum(Bb_terms, eh, na)
    blocks_of = [np.nonzero(eh == a)[0] for a in range(na)]   # per pose: its blocks in ascending landmark
    for i1 in range(na):
        hd = Hpp[i1].copy()
        for k in range(6):
            hd[k, k] = hd[k, k] + lam
        for i2 in range(i1, na):
            b1, b2 = blocks_of[i1], blocks_of[i2]
            _, s1, s2 = np.intersect1d(lm_of[b1], lm_of[b2], assume_unique=True, return_indices=True)
            h = (0.0 + hd) if i1 == i2 else np.zeros((6, 6))
            if len(s1):
                bd, bj = BD[b1[s1]], Bi[b2[s2]]
                S = (bd[:, :, 0][:, :, None] * bj[:, :, 0][:, None, :] + bd[:, :, 1][:, :, None] * bj[:, :, 1][:, None, :]) \
                    + bd[:, :, 2][:, :, None] * bj[:, :, 2][:, None, :]
                h = np.add.accumulate(np.concatenate([h[None], -S]), axis=0)[-1]
            Hs[6 * i1:6 * i1 + 6, 6 * i2:6 * i2 + 6] = h
        coeff[6 * i1:6 * i1 + 6] = coeffs[i1]
    bschur = bp.reshape(-1) - coeff
    xp = ldlt_solve(Hs, bschur)
    if xp is None:
        return None
    cp = -xp.reshape(na, 6)
    # cl = bl; per landmark `cl += Bi^T * cp` in ascending pose index; xl = 0 + Dinv * cl
    order_pl = np.lexsort((eh, lm_of)) if nb else np.zeros(0, int)
    Bo, cpo = Bi[order_pl], cp[eh[order_pl]] if nb else np.zeros((0, 6))
    if nb:
        tt = Bo[:, 0, :] * cpo[:, 0][:, None]
        for k in range(1, 6):
            tt = tt + Bo[:, k, :] * cpo[:, k][:, None]
    else:
        tt = np.zeros((0, 3))
    cl = bl.copy()
    own = lm_of[order_pl] if nb else np.zeros(0, int)
    if len(own):
        start = np.searchsorted(own, own, side="left")
        rank = np.arange(len(own)) - start
        for r in range(int(rank.max()) + 1):
            sel = rank == r
            cl[own[sel]] = cl[own[sel]] + tt[sel]
    xl = np.stack([0.0 + ((Dinv[:, r, 0] * cl[:, 0] + Dinv[:, r, 1] * cl[:, 1]) + Dinv[:, r, 2] * cl[:, 2]) for r in range(3)],
                  axis=1) if nl else np.zeros((0, 3))
    return xp, xl.reshape(-1), Hs, bschur



def robust_chi2(G, ev, robust):
    chi2, st = ev["chi2"], ev["stereo"]
    with np.errstate(all="ignore"):
        rho0 = chi2.copy()
        for s, (delta, dsqr) in enumerate(G.huber):
            sel = robust & (st == bool(s)) & ~(chi2 <= dsqr)
            rho0 = np.where(sel, 2 * np.sqrt(chi2) * delta - dsqr, rho0)
    return rho0


def total_chi2(G, act, rho0, order):
    """activeRobustChi2 over the active edges `act` (ascending positions)."""
    if order == "index":
        return float(np.add.accumulate(np.concatenate([[0.0], rho0]))[-1])
    leaf = np.zeros(G.n_edges); leaf[act] = rho0
    chi = 0.0
    for k in range(0, G.n_edges, LANES):
        chi += tree_partial(leaf[k:k + LANES])
    return float(chi)


def optimize(W, order="index", stop=None, trace=None):
    """-> Result.  stop: None (no flag), a callable, or an int n: true from the n-th poll on."""
    G = Graph(W)
    tr = trace if trace is not None else Trace()
    polls = [0]
    if stop is None:
        poll = lambda: False
    else:
        fn = stop if callable(stop) else (lambda: polls[0] > int(stop))

        def poll():
            polls[0] += 1
            return bool(fn())
    poses = np.zeros((G.n_poses, 7))
    for p in range(G.n_poses):
        T = SE3.from_cv(G.Tcw[p])
        poses[p] = T.q + T.t
    points = np.asarray(W["points"], np.float32).reshape(-1, 3).astype(np.float64)
    flags = np.zeros(G.n_edges, np.uint8)
    last_chi2 = np.zeros(G.n_edges)            # the error the last computeActiveErrors left in each edge (0: never reached)
    x = np.zeros(6 * G.n_free + 3 * G.n_points)  # g2o's x, position by position
    R = Result()
    R.rounds = np.zeros(2, ROUND_DTYPE)
    R.ended, R.optimisations = ENDED_COMPLETE, 0
    R.active_poses, R.active_points, R.active_edges = [0, 0], [0, 0], [0, 0]

    def classify(which):
        tested = ~G.bad[G.edge_point]
        ev = edge_pass(G, poses, points, np.arange(G.n_edges), False)
        th = np.where(G.stereo, TH_STEREO, TH_MONO)
        hit = tested & ((last_chi2 > th) | ~(ev["zc"] > 0.0))
        flags[hit] |= which
        tr.tests.append((last_chi2.copy(), ev["zc"].copy(), tested))

    if poll():                                  # :1204
        R.ended = ENDED_STOPPED_AT_START
    for stage in range(2):
        if R.ended != ENDED_COMPLETE:
            break
        # initializeOptimization(0)
        act = np.nonzero((flags & FLAG_LEVEL1) == 0)[0]
        ep, el = G.edge_pose[act], G.edge_point[act]
        pose_h = np.full(G.n_poses, -1); point_h = np.full(G.n_points, -1)
        free_with_edge = np.unique(ep[ep < G.n_free])
        pose_h[free_with_edge] = np.arange(len(free_with_edge))
        pts_with_edge = np.unique(el)
        point_h[pts_with_edge] = np.arange(len(pts_with_edge))
        na, nl = len(free_with_edge), len(pts_with_edge)
        R.active_poses[stage], R.active_points[stage], R.active_edges[stage] = na, nl, len(act)
        robust = (stage == 0) | G.bad[el]
        if na + nl > 0:
            R.optimisations = stage + 1
            n = 6 * na
            eh = pose_h[ep]                     # hessian index of each active edge's pose, -1: fixed
            fe = np.nonzero(eh >= 0)[0]         # the active edges that have an Hpl block, in edge order
            lam, ni, n_bad_steps = 0.0, 2.0, 0
            rnd = R.rounds[stage]
            ok = True
            i = 0
            max_iter = 10 if stage else 5
            while i < max_iter:                 # for (int i=0; i<iterations && ! terminate() && ok; i++)
                if poll():
                    tr.exits.append("stop_376")
                    break
                if not ok:
                    break
                # solve(): computeActiveErrors, activeRobustChi2, buildSystem
                ev = edge_pass(G, poses, points, act, True)
                last_chi2[act] = ev["chi2"]
                bl_e, Hll_e, bp_e, Hpp_e, Hpl_e, rho0 = quadratic_form(G, ev, robust)
                current_chi = total_chi2(G, act, rho0, order)
                ini_chi = current_chi
                Hll = ranked_sum(Hll_e, point_h[el], nl); bl = ranked_sum(bl_e, point_h[el], nl)
                Hpp = ranked_sum(Hpp_e[fe], eh[fe], na); bp = ranked_sum(bp_e[fe], eh[fe], na)
                if i == 0:                      # computeLambdaInit
                    md = 0.0
                    for v in list(np.abs(Hpp[:, range(6), range(6)]).ravel()) + list(np.abs(Hll[:, range(3), range(3)]).ravel()):
                        if v > md:
                            md = float(v)
                    lam, ni, n_bad_steps = 1e-5 * md, 2.0, 0
                qmax = 0
                rho = 0.0
                stopped = False
                while True:
                    # push; setLambda; solve
                    sol = schur_solve(Hll, bl, Hpp, bp, Hpl_e[fe], eh[fe], point_h[el[fe]], na, nl, lam)
                    ok2 = sol is not None
                    if ok2:
                        x[:n] = sol[0]
                        x[n:n + 3 * nl] = sol[1]
                    else:
                        tr.solve_failed += 1
                    # update(x): oplus of every active vertex
                    t_poses, t_points = poses.copy(), points.copy()
                    for a, p in enumerate(free_with_edge):
                        d, _ = SE3.exp([float(v) for v in x[6 * a:6 * a + 6]], order)
                        T = d * raw_se3(poses[p, :4], poses[p, 4:])
                        t_poses[p] = T.q + T.t
                    t_points[pts_with_edge] = points[pts_with_edge] + x[n:n + 3 * nl].reshape(nl, 3)
                    # restoreDiagonal (Hll, Hpp are the undamped ones); computeActiveErrors
                    ev_t = edge_pass(G, t_poses, t_points, act, False)
                    last_chi2[act] = ev_t["chi2"]
                    temp_chi = total_chi2(G, act, robust_chi2(G, ev_t, robust), order)
                    if not ok2:
                        temp_chi = DBL_MAX
                    rho = current_chi - temp_chi
                    bfull = np.concatenate([bp.reshape(-1), bl.reshape(-1)])
                    xv = x[:n + 3 * nl]
                    scale = float(np.add.accumulate(np.concatenate([[0.0], xv * (lam * xv + bfull)]))[-1])   # computeScale
                    scale += 1e-3
                    rho /= scale
                    tr.trials.append((stage, i, lam, rho, ok2))
                    if rho > 0 and abs(temp_chi) <= DBL_MAX:
                        u = 2 * rho - 1
                        cube = math.pow(u, 3) if order == "index" else u * u * u
                        alpha = 1. - cube
                        alpha = min(alpha, 2. / 3.)
                        lam *= max(1. / 3., alpha)
                        ni = 2.0
                        current_chi = temp_chi
                        poses, points = t_poses, t_points     # discardTop
                    else:
                        lam *= ni
                        ni *= 2                                 # pop
                    qmax += 1
                    rnd["trials"] += 1
                    if not (rho < 0 and qmax < 10):
                        break
                    if poll():                                  # levenberg.cpp:149
                        stopped = True
                        break
                rnd["iterations"] += 1
                terminate = qmax == 10 or rho == 0
                tr.exits.append("stopped" if stopped else "qmax" if qmax == 10 else "rho0" if rho == 0 else "accepted")
                if not terminate:
                    n_bad_steps = n_bad_steps + 1 if (ini_chi - current_chi) * 1e3 < ini_chi else 0
                    if n_bad_steps >= 3:
                        terminate = True
                        tr.exits.append("three_bad")
                ok = not terminate
                rnd["chi2"], rnd["lambda"] = canonical(current_chi), canonical(lam)
                i += 1
                if i == max_iter:
                    tr.exits.append("max_iter")
        if stage == 0:
            if poll():                          # :1217
                R.ended = ENDED_NO_SECOND
                break
            classify(FLAG_LEVEL1)
    if R.ended != ENDED_STOPPED_AT_START:
        classify(FLAG_ERASE)
    # Converter::toCvMat
    R.pose = np.array([[canonical(float(v)) for v in row] for row in poses]).reshape(G.n_poses, 7)
    R.Tcw = np.zeros((G.n_poses, 16), np.float32)
    for p in range(G.n_poses):
        Rm = quat_to_matrix([float(v) for v in poses[p, :4]])
        M = np.zeros((4, 4), np.float32)
        with np.errstate(all="ignore"):
            for r in range(3):
                for c in range(3):
                    M[r, c] = np.float32(Rm[r][c])
                M[r, 3] = np.float32(poses[p, 4 + r])
        M[3, 3] = 1.0
        R.Tcw[p] = M.reshape(16)
    R.point = points.reshape(G.n_points, 3).copy()
    with np.errstate(all="ignore"):
        R.point_f = R.point.astype(np.float32)
    R.flags = flags
    R.polls = polls[0]
    R.n_level1, R.n_erase = int(((flags & FLAG_LEVEL1) != 0).sum()), int(((flags & FLAG_ERASE) != 0).sum())
    R.active_poses, R.active_points, R.active_edges = tuple(R.active_poses), tuple(R.active_points), tuple(R.active_edges)
    R.trace = tr
    return R
