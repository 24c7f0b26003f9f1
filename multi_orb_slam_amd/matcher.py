"""Host-side mirror of the hot part of ORB_SLAM2::ORBmatcher over the C ABI (include/orbm.h)."""
import ctypes as C
import weakref
import numpy as np
from . import _lib
from ._lib import KP_DTYPE, QUERY_DTYPE, POINT_DTYPE, TRACK_DTYPE, REFRESH_DTYPE, CamFeatures, FrameDesc, check, ptr
from ._lib import OBS_DTYPE, MAX_POINTS, COVIS_DTYPE  # noqa: F401
from ._lib import POSE_PROBLEM_DTYPE, POSE_RESULT_DTYPE, POSE_CAM0, POSE_ALL_CAMS, POSE_ORDER_INDEX, POSE_ORDER_DEVICE  # noqa: F401
from ._lib import SIM3_PROBLEM_DTYPE, SIM3_HYP_DTYPE, SIM3_WALK_DTYPE, SIM3_MATH_LIBM, SIM3_MATH_DEVICE  # noqa: F401
from ._lib import SIM3OPT_PROBLEM_DTYPE, SIM3OPT_RESULT_DTYPE  # noqa: F401
from ._lib import PNP_PROBLEM_DTYPE, PNP_HYP_DTYPE, PNP_REFINED_DTYPE, PNP_WALK_DTYPE, PNP_MAX_RECORDS  # noqa: F401

TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30  # reference src/ORBmatcher.cc:37-39
# which resolve delivered a search's result (ORBM_FORM_*, include/orb_debug.h; Matcher.last_resolve_form)
(FORM_NONE, FORM_HOST, FORM_MONO2_ANG, FORM_MONO2, FORM_MONO4_WORKLIST, FORM_MONO4_WAVES, FORM_JACOBI_LDSQ, FORM_JACOBI, FORM_CAMS,
 FORM_SWEEPS) = range(10)


def descriptor_distance(a, b):
    """static ORBmatcher::DescriptorDistance (reference src/ORBmatcher.cc:3994-4010)."""
    a = np.ascontiguousarray(a, np.uint8); b = np.ascontiguousarray(b, np.uint8)
    return _lib.lib().orbm_descriptor_distance(ptr(a), ptr(b))


def three_maxima(sizes):
    sizes = np.ascontiguousarray(sizes, np.int32); ind = np.zeros(3, np.int32)
    _lib.lib().orbm_three_maxima(ptr(sizes), len(sizes), ptr(ind))
    return tuple(int(i) for i in ind)


class View:
    """The Frame members Frame::isInFrustum reads (orbm_view): pose, intrinsics, image bounds, the scale pyramid and the
    `th` of SearchByProjection(F, vpMapPoints, th).  Rcw 3x3 row-major, tcw and Ow 3-vectors, bounds = (min_x, min_y, max_x, max_y)."""

    def __init__(self, Rcw, tcw, Ow, fx, fy, cx, cy, mbf, bounds, scale_factors, log_scale_factor, th=1.0, viewing_cos_limit=0.5):
        self.scale_factors = np.ascontiguousarray(scale_factors, np.float32)
        c = self.c = _lib.View()
        c.Rcw[:] = np.asarray(Rcw, np.float32).reshape(9).tolist()
        c.tcw[:] = np.asarray(tcw, np.float32).reshape(3).tolist()
        c.Ow[:] = np.asarray(Ow, np.float32).reshape(3).tolist()
        c.fx, c.fy, c.cx, c.cy, c.mbf = float(fx), float(fy), float(cx), float(cy), float(mbf)
        c.min_x, c.min_y, c.max_x, c.max_y = (float(b) for b in bounds)
        c.viewing_cos_limit = float(viewing_cos_limit); c.th = float(th)
        c.log_scale_factor = float(log_scale_factor); c.n_levels = len(self.scale_factors)
        c.scale_factors = self.scale_factors.ctypes.data


def level_thresholds(log_scale_factor, n_levels):
    """orbm_level_thresholds: the largest ratio of every level under the C library's logf (host only)."""
    out = np.zeros(max(n_levels - 1, 1), np.float32)
    check(_lib.lib().orbm_level_thresholds(float(log_scale_factor), int(n_levels), ptr(out)))
    return out[:max(n_levels - 1, 0)]


def frustum_host(points, view, skip=None):
    """orbm_frustum_host: the library's host restatement of the frustum kernel -> (n_to_match, track, queries)."""
    points = np.ascontiguousarray(points, POINT_DTYPE); n = len(points)
    sk = None if skip is None else np.ascontiguousarray(skip, np.uint8)
    assert sk is None or len(sk) == n
    track = np.zeros(max(n, 1), TRACK_DTYPE); q = np.zeros(max(n, 1), QUERY_DTYPE); cnt = C.c_int()
    check(_lib.lib().orbm_frustum_host(ptr(points), n, C.byref(view.c), None if sk is None else ptr(sk), ptr(track), ptr(q),
                                       C.byref(cnt)))
    return cnt.value, track[:n], q[:n]


class RefreshBatch:
    """The inputs of a map-point refresh (orbm_refresh_in): P points whose observations arrive as a CSR list.  first[P + 1];
    obs_desc n_obs x 32, obs_centre n_obs x 3 (centre of the observing camera), obs_alive n_obs (the keyframe is not bad); pos and
    ref_centre P x 3, ref_level P (octave of the point's keypoint in its reference keyframe), what P (bit 0: distinctive
    descriptor, bit 1: normal and depth); scale_factors = mvScaleFactors."""

    def __init__(self, first, obs_desc, obs_centre, obs_alive, pos, ref_centre, ref_level, what, scale_factors):
        self.first = np.ascontiguousarray(first, np.int32)
        self.n_points = len(self.first) - 1; self.n_obs = int(self.first[-1])
        self.obs_desc = np.ascontiguousarray(obs_desc, np.uint8).reshape(-1, 32)
        self.obs_centre = np.ascontiguousarray(obs_centre, np.float32).reshape(-1, 3)
        self.obs_alive = np.ascontiguousarray(obs_alive, np.uint8)
        self.pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
        self.ref_centre = np.ascontiguousarray(ref_centre, np.float32).reshape(-1, 3)
        self.ref_level = np.ascontiguousarray(ref_level, np.int32)
        self.what = np.ascontiguousarray(what, np.uint8)
        self.scale_factors = np.ascontiguousarray(scale_factors, np.float32)
        assert self.n_points >= 0 and len(self.obs_desc) == len(self.obs_centre) == len(self.obs_alive) == self.n_obs
        assert len(self.pos) == len(self.ref_centre) == len(self.ref_level) == len(self.what) == self.n_points
        self.c = _lib.RefreshIn(self.n_points, self.n_obs, *[a.ctypes.data for a in (
            self.first, self.obs_desc, self.obs_centre, self.obs_alive, self.pos, self.ref_centre, self.ref_level, self.what,
            self.scale_factors)], len(self.scale_factors))


def refresh_points_host(batch):
    """orbm_refresh_points_host: MapPoint::ComputeDistinctiveDescriptors + UpdateNormalAndDepth for every point of a RefreshBatch,
    entirely on the host (no device needed) -> REFRESH_DTYPE records."""
    out = np.zeros(max(batch.n_points, 1), REFRESH_DTYPE)
    check(_lib.lib().orbm_refresh_points_host(C.byref(batch.c), ptr(out)))
    return out[:batch.n_points]


class PoseProblem:
    """One Optimizer::PoseOptimization call from its edge list on (orbm_pose_problem + its edges): Tcw = pFrame->mTcw (float 4x4);
    fx fy cx cy bf; inv_level_sigma2 = mvInvLevelSigma2; mode POSE_CAM0 / POSE_ALL_CAMS with n_cam0 = pFrame->N and Rcam12 / tcam12;
    the edges in ascending feature index: feat n, pos n x 3 (the map points), obs n x 3 (x, y, uright; uright < 0 = monocular), octave n."""

    def __init__(self, Tcw, fx, fy, cx, cy, bf, inv_level_sigma2, feat, pos, obs, octave, mode=POSE_CAM0, n_cam0=0, Rcam12=None,
                 tcam12=None):
        rec = np.zeros(1, POSE_PROBLEM_DTYPE)
        rec["Tcw"][0] = np.asarray(Tcw, np.float32).reshape(16)
        for k, v in (("fx", fx), ("fy", fy), ("cx", cx), ("cy", cy), ("bf", bf)):
            rec[k] = np.float32(v)
        rec["Rcam12"][0] = np.eye(3, dtype=np.float32).reshape(9) if Rcam12 is None else np.asarray(Rcam12, np.float32).reshape(9)
        rec["tcam12"][0] = 0 if tcam12 is None else np.asarray(tcam12, np.float32).reshape(3)
        sig = np.asarray(inv_level_sigma2, np.float32)
        rec["inv_level_sigma2"][0, :len(sig)] = sig
        rec["n_levels"] = len(sig); rec["mode"] = int(mode); rec["n_cam0"] = int(n_cam0)
        self.rec = rec
        self.feat = np.ascontiguousarray(feat, np.int32)
        self.pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
        self.obs = np.ascontiguousarray(obs, np.float32).reshape(-1, 3)
        self.octave = np.ascontiguousarray(octave, np.int32)
        self.n = len(self.feat)
        assert len(self.pos) == len(self.obs) == len(self.octave) == self.n


def _pose_pack(problems):
    recs = np.concatenate([p.rec for p in problems])
    first = np.zeros(len(problems) + 1, np.int32)
    first[1:] = np.cumsum([p.n for p in problems])
    cat = lambda name, dt, shape: np.ascontiguousarray(np.concatenate([getattr(p, name) for p in problems]).reshape(shape), dt)
    return recs, first, cat("feat", np.int32, (-1,)), cat("pos", np.float32, (-1, 3)), cat("obs", np.float32, (-1, 3)), cat("octave", np.int32, (-1,))


def _pose_unpack(problems, first, flags, res):
    return [(res[b].copy(), flags[first[b]:first[b + 1]].copy()) for b in range(len(problems))]


def pose_optimize_host(problems, order=POSE_ORDER_INDEX):
    """orbm_pose_optimize_host: the batch entirely on the host (no device needed), sums in index order (the restatement of the
    reference) or in the kernel's order -> [(POSE_RESULT_DTYPE record, outlier flag per edge)] per problem."""
    recs, first, feat, pos, obs, octave = _pose_pack(problems)
    flags = np.zeros(max(int(first[-1]), 1), np.uint8); res = np.zeros(len(problems), POSE_RESULT_DTYPE)
    check(_lib.lib().orbm_pose_optimize_host(ptr(recs), len(problems), ptr(first), ptr(feat), ptr(pos), ptr(obs), ptr(octave), int(order),
                                             ptr(flags), ptr(res)))
    return _pose_unpack(problems, first, flags, res)


def pose_sincos(x):
    """The sine / cosine sequence of POSE_ORDER_DEVICE (orbm_pose_sincos) -> (sin, cos)."""
    s = C.c_double(); c = C.c_double()
    _lib.lib().orbm_pose_sincos(float(x), C.byref(s), C.byref(c))
    return s.value, c.value


class Sim3Problem:
    """One Sim3Solver from its constructor's vectors on (orbm_sim3_problem + its correspondences + its drawn triples): K1, K2 =
    (fx, fy, cx, cy) of mK1, mK2; x3dc1, x3dc2 n x 3 (mvX3Dc1, mvX3Dc2); cam1, cam2 n (camIdx1, camIdx2); max_err1, max_err2 n
    (mvnMaxError1/2 as floats); triples H x 3 positions 0 .. n-1; either Rcam21 / tcam21 or calib = the constructor's CalibMatrix
    (rows 0-2: Rcam12, row 3: tcam12), from which they are derived as the constructor does."""

    def __init__(self, K1, K2, x3dc1, x3dc2, cam1, cam2, max_err1, max_err2, triples, fix_scale=False, Rcam21=None, tcam21=None, calib=None):
        rec = np.zeros(1, SIM3_PROBLEM_DTYPE)
        for k, v in zip(("fx1", "fy1", "cx1", "cy1"), K1):
            rec[k] = np.float32(v)
        for k, v in zip(("fx2", "fy2", "cx2", "cy2"), K2):
            rec[k] = np.float32(v)
        if calib is not None:
            Rcam21, tcam21 = sim3_second_camera(calib)
        rec["Rcam21"][0] = np.eye(3, dtype=np.float32).reshape(9) if Rcam21 is None else np.asarray(Rcam21, np.float32).reshape(9)
        rec["tcam21"][0] = 0 if tcam21 is None else np.asarray(tcam21, np.float32).reshape(3)
        rec["fix_scale"] = 1 if fix_scale else 0
        self.rec = rec
        self.x3dc1 = np.ascontiguousarray(x3dc1, np.float32).reshape(-1, 3)
        self.x3dc2 = np.ascontiguousarray(x3dc2, np.float32).reshape(-1, 3)
        self.cam1 = np.ascontiguousarray(cam1, np.int32); self.cam2 = np.ascontiguousarray(cam2, np.int32)
        self.max_err1 = np.ascontiguousarray(max_err1, np.float32); self.max_err2 = np.ascontiguousarray(max_err2, np.float32)
        self.triples = np.ascontiguousarray(triples, np.int32).reshape(-1, 3)
        self.n = len(self.x3dc1); self.h = len(self.triples); self.w = (self.n + 63) // 64
        assert len(self.x3dc2) == len(self.cam1) == len(self.cam2) == len(self.max_err1) == len(self.max_err2) == self.n


def sim3_second_camera(calib):
    """mRcam21 = Rcam12.t(), mtcam21 = -mRcam21 * tcam12 of the constructor (reference src/Sim3Solver.cc:61-70): the transpose, then
    cv::gemm's small path with alpha = -1 -> (Rcam21 3 x 3, tcam21 3), float32."""
    calib = np.asarray(calib, np.float32)
    R21 = np.ascontiguousarray(calib[:3, :3].T)
    t12 = calib[3, :3]
    t = R21[:, 0] * t12[0] + R21[:, 1] * t12[1]
    t = t + R21[:, 2] * t12[2]
    return R21, (t.astype(np.float64) * -1.0 + 0.0 * 0.0).astype(np.float32)


def _sim3_pack(problems):
    recs = np.concatenate([p.rec for p in problems])
    first = np.zeros(len(problems) + 1, np.int32); its_first = np.zeros(len(problems) + 1, np.int32)
    first[1:] = np.cumsum([p.n for p in problems]); its_first[1:] = np.cumsum([p.h for p in problems])
    cat = lambda name, dt, shape: np.ascontiguousarray(np.concatenate([getattr(p, name) for p in problems]).reshape(shape), dt)
    words = int(sum(p.h * p.w for p in problems))
    hyp = np.zeros(max(int(its_first[-1]), 1), SIM3_HYP_DTYPE); masks = np.zeros(max(words, 1), np.uint64)
    args = (ptr(recs), len(problems), ptr(first), ptr(cat("x3dc1", np.float32, (-1, 3))), ptr(cat("x3dc2", np.float32, (-1, 3))),
            ptr(cat("cam1", np.int32, (-1,))), ptr(cat("cam2", np.int32, (-1,))), ptr(cat("max_err1", np.float32, (-1,))),
            ptr(cat("max_err2", np.float32, (-1,))), ptr(its_first), ptr(cat("triples", np.int32, (-1, 3))))
    return args, its_first, hyp, masks


def _sim3_unpack(problems, its_first, hyp, masks):
    out, w0 = [], 0
    for b, p in enumerate(problems):
        out.append((hyp[its_first[b]:its_first[b + 1]].copy(), masks[w0:w0 + p.h * p.w].reshape(p.h, p.w).copy()))
        w0 += p.h * p.w
    return out


def sim3_ransac_host(problems, order=SIM3_MATH_LIBM):
    """orbm_sim3_ransac_host: every hypothesis of every problem on the host (no device needed), atan2 / sin / cos of the C library
    (the restatement of the reference) or the device's sequences -> [(SIM3_HYP_DTYPE records H, mask words H x W uint64)] per problem."""
    args, its_first, hyp, masks = _sim3_pack(problems)
    check(_lib.lib().orbm_sim3_ransac_host(*args, int(order), ptr(hyp), ptr(masks)))
    return _sim3_unpack(problems, its_first, hyp, masks)


def sim3_walk(counts, N, min_inliers, start_iteration, n_iterations, state=None):
    """orbm_sim3_walk: Sim3Solver::iterate(n_iterations, ...) over the precomputed inlier counts of the solver's hypotheses, starting at
    mnIterations = start_iteration with state = (best_inliers, best_index) (None: a fresh solver)
    -> (hypothesis returned or -1, no_more, iterations, best_inliers, best_index)."""
    counts = np.ascontiguousarray(counts, np.int32)
    st = np.zeros(1, SIM3_WALK_DTYPE)
    st["best_inliers"], st["best_index"] = (0, -1) if state is None else state
    found = _lib.lib().orbm_sim3_walk(ptr(counts), len(counts), int(N), int(min_inliers), int(start_iteration), int(n_iterations), ptr(st))
    return int(found), bool(st["no_more"][0]), int(st["iterations"][0]), int(st["best_inliers"][0]), int(st["best_index"][0])


def sim3_iterations(probability, min_inliers, max_its, N):
    """orbm_sim3_iterations: mRansacMaxIts after SetRansacParameters(probability, min_inliers, max_its) with N correspondences."""
    return int(_lib.lib().orbm_sim3_iterations(float(probability), int(min_inliers), int(max_its), int(N)))


def sim3_atan2(y, x):
    """The atan2 sequence of SIM3_MATH_DEVICE (orbm_sim3_atan2): y >= 0, x in [-1, 1]."""
    return float(_lib.lib().orbm_sim3_atan2(float(y), float(x)))


class PnPProblem:
    """One PnPsolver from its constructor's vectors on (orbm_pnp_problem + its correspondences + its drawn quadruples): K = (fx, fy, cx,
    cy) of the frame (floats, widened to the solver's doubles); p3dw n x 3 (mvP3Dw), p2d n x 2 (mvP2D), max_err n (mvMaxError);
    quads H x 4 positions 0 .. n-1 in drawing order; min_inliers = mRansacMinInliers after SetRansacParameters; best_start =
    mnBestInliers on entry."""

    def __init__(self, K, p3dw, p2d, max_err, quads, min_inliers, best_start=0):
        rec = np.zeros(1, PNP_PROBLEM_DTYPE)
        for k, v in zip(("fu", "fv", "uc", "vc"), K):
            rec[k] = float(np.float32(v))
        rec["min_inliers"] = int(min_inliers); rec["best_start"] = int(best_start)
        self.rec = rec
        self.p3dw = np.ascontiguousarray(p3dw, np.float32).reshape(-1, 3)
        self.p2d = np.ascontiguousarray(p2d, np.float32).reshape(-1, 2)
        self.max_err = np.ascontiguousarray(max_err, np.float32).reshape(-1)
        self.quads = np.ascontiguousarray(quads, np.int32).reshape(-1, 4)
        self.n = len(self.p3dw); self.h = len(self.quads); self.w = (self.n + 63) // 64
        assert len(self.p2d) == len(self.max_err) == self.n


def _pnp_pack(problems):
    B = len(problems)
    recs = np.concatenate([p.rec for p in problems])
    first = np.zeros(B + 1, np.int32); its_first = np.zeros(B + 1, np.int32)
    first[1:] = np.cumsum([p.n for p in problems]); its_first[1:] = np.cumsum([p.h for p in problems])
    cat = lambda name, dt, shape: np.ascontiguousarray(np.concatenate([getattr(p, name) for p in problems]).reshape(shape), dt)
    words = int(sum(p.h * p.w for p in problems))
    extra = [max(0, min(p.h, p.n) - PNP_MAX_RECORDS) for p in problems]   # always enough (include/orbm.h)
    rwords = PNP_MAX_RECORDS * int(sum(p.w for p in problems)) + int(sum(e * p.w for e, p in zip(extra, problems)))
    hyp = np.zeros(max(int(its_first[-1]), 1), PNP_HYP_DTYPE); masks = np.zeros(max(words, 1), np.uint64)
    n_rec = np.zeros(B, np.int32)
    refined = np.zeros(B * PNP_MAX_RECORDS + sum(extra), PNP_REFINED_DTYPE); rmasks = np.zeros(max(rwords, 1), np.uint64)
    args = (ptr(recs), B, ptr(first), ptr(cat("p3dw", np.float32, (-1, 3))), ptr(cat("p2d", np.float32, (-1, 2))),
            ptr(cat("max_err", np.float32, (-1,))), ptr(its_first), ptr(cat("quads", np.int32, (-1, 4))), ptr(hyp), ptr(masks), ptr(n_rec),
            ptr(refined), ptr(rmasks), int(sum(extra)))
    return args, (its_first, hyp, masks, n_rec, refined, rmasks)


def _pnp_unpack(problems, out):
    """-> per problem (PNP_HYP_DTYPE records H, mask words H x W, PNP_REFINED_DTYPE records R, their mask words R x W), R = all records
    of the problem: the ORBM_PNP_MAX_RECORDS slots first, the appended ones behind."""
    its_first, hyp, masks, n_rec, refined, rmasks = out
    B = len(problems)
    res, w0 = [], 0
    xr, xw = B * PNP_MAX_RECORDS, PNP_MAX_RECORDS * int(sum(p.w for p in problems))
    rw0 = 0
    for b, p in enumerate(problems):
        nr = int(n_rec[b]); nd = min(nr, PNP_MAX_RECORDS); ne = nr - nd
        ref = np.concatenate([refined[b * PNP_MAX_RECORDS:b * PNP_MAX_RECORDS + nd], refined[xr:xr + ne]])
        rm = np.concatenate([rmasks[rw0:rw0 + nd * p.w], rmasks[xw:xw + ne * p.w]]).reshape(nr, p.w)
        # the unused slots stay zero
        assert not refined[b * PNP_MAX_RECORDS + nd:(b + 1) * PNP_MAX_RECORDS].view(np.uint8).any()
        assert not rmasks[rw0 + nd * p.w:rw0 + PNP_MAX_RECORDS * p.w].any()
        xr += ne; xw += ne * p.w; rw0 += PNP_MAX_RECORDS * p.w
        res.append((hyp[its_first[b]:its_first[b + 1]].copy(), masks[w0:w0 + p.h * p.w].reshape(p.h, p.w).copy(), ref.copy(), rm.copy()))
        w0 += p.h * p.w
    return res


def pnp_ransac_host(problems):
    """orbm_pnp_ransac_host: every hypothesis and every refined record of every problem on the host (no device needed)
    -> per problem (hypothesis records, mask words H x W, refined records, their mask words)."""
    args, out = _pnp_pack(problems)
    check(_lib.lib().orbm_pnp_ransac_host(*args))
    return _pnp_unpack(problems, out)


def pnp_walk_state():
    """The state of a fresh solver for pnp_walk."""
    st = np.zeros(1, PNP_WALK_DTYPE)
    st["best_hyp"] = -1; st["best_record"] = -1
    return st


def pnp_walk(counts, block_start, rec_hyp, rec_inliers, N, min_inliers, max_its, n_iterations, state):
    """orbm_pnp_walk: PnPsolver::iterate(n_iterations, ...) over a block of evaluated hypotheses (counts; the iterations block_start ..)
    and the block's records (position inside the block, refined n_inliers); state: PNP_WALK_DTYPE[1], updated in place
    -> PNP_WALK_NOTHING / PNP_WALK_REFINED / PNP_WALK_BEST."""
    counts = np.ascontiguousarray(counts, np.int32)
    rec_hyp = np.ascontiguousarray(rec_hyp, np.int32); rec_inliers = np.ascontiguousarray(rec_inliers, np.int32)
    ans = _lib.lib().orbm_pnp_walk(ptr(counts), len(counts), int(block_start), ptr(rec_hyp), ptr(rec_inliers), len(rec_hyp), int(N),
                                   int(min_inliers), int(max_its), int(n_iterations), ptr(state))
    assert ans >= 0, "orbm_pnp_walk: bad arguments"
    return int(ans)


def pnp_parameters(N, probability=0.99, min_inliers=8, max_its=300, min_set=4, epsilon=0.4):
    """orbm_pnp_parameters: SetRansacParameters with N correspondences -> (mRansacMaxIts, mRansacMinInliers, mRansacEpsilon float32)."""
    out = np.zeros(2, np.int32); eps = np.zeros(1, np.float32)
    assert _lib.lib().orbm_pnp_parameters(float(probability), int(min_inliers), int(max_its), int(min_set), float(np.float32(epsilon)), int(N),
                                          ptr(out), ptr(eps)) == 0
    return int(out[0]), int(out[1]), eps[0]


def pnp_svd(A):
    """cvSVD as the library restates it (orbm_pnp_svd) of an m x n float64 matrix, m >= n -> (w n, ut n x m, vt n x n, random branch)."""
    A = np.ascontiguousarray(A, np.float64)
    m_, n = A.shape
    w = np.zeros(n); ut = np.zeros((n, m_)); vt = np.zeros((n, n))
    r = _lib.lib().orbm_pnp_svd(ptr(A), m_, n, ptr(w), ptr(ut), ptr(vt))
    assert r >= 0
    return w, ut, vt, bool(r)


def pnp_qr_solve(A, b, x0=None):
    """qr_solve (orbm_pnp_qr_solve): A nr x nc, b nr -> (x, singular); x0: what x held on entry (it is left alone on a singular return)."""
    A = np.array(A, np.float64); b = np.array(b, np.float64)
    nr, nc = A.shape
    x = np.zeros(nc) if x0 is None else np.array(x0, np.float64)
    r = _lib.lib().orbm_pnp_qr_solve(ptr(A), nr, nc, ptr(b), ptr(x))
    assert r >= 0
    return x, bool(r)


def pnp_compute_pose(pws, us, K):
    """compute_pose of n points (orbm_pnp_compute_pose): pws n x 3, us n x 2 float64, K = fu fv uc vc -> (R 3 x 3, t 3, error, choice, flags)."""
    pws = np.ascontiguousarray(pws, np.float64).reshape(-1, 3); us = np.ascontiguousarray(us, np.float64).reshape(-1, 2)
    K = np.ascontiguousarray(K, np.float64)
    R = np.zeros(9); t = np.zeros(3); out = np.zeros(2, np.int32)
    err = _lib.lib().orbm_pnp_compute_pose(ptr(pws), ptr(us), len(pws), ptr(K), ptr(R), ptr(t), ptr(out))
    return R.reshape(3, 3), t, float(err), int(out[0]), int(out[1])


class Sim3OptProblem:
    """One Optimizer::OptimizeSim3_cam1 call from its correspondence list on (orbm_sim3opt_problem + its correspondences): K1, K2 =
    (fx, fy, cx, cy) of pKF1->mK, pKF2->mK; inv_level_sigma2_1 / _2 = mvInvLevelSigma2 of the two keyframes; the start g2oS12 as float
    R 3 x 3, t 3, s; th2; fix_scale; x3dc1, x3dc2 n x 3 (camera-frame points of keyframe 1 and 2), obs1, obs2 n x 2 (kpUn.pt), octave1,
    octave2 n."""

    def __init__(self, K1, K2, inv_level_sigma2_1, inv_level_sigma2_2, R, t, s, th2, fix_scale, x3dc1, x3dc2, obs1, obs2, octave1, octave2):
        rec = np.zeros(1, SIM3OPT_PROBLEM_DTYPE)
        rec["K1"][0] = np.asarray(K1, np.float32); rec["K2"][0] = np.asarray(K2, np.float32)
        s1 = np.asarray(inv_level_sigma2_1, np.float32); s2 = np.asarray(inv_level_sigma2_2, np.float32)
        rec["inv_level_sigma2_1"][0, :len(s1)] = s1; rec["inv_level_sigma2_2"][0, :len(s2)] = s2
        rec["n_levels1"] = len(s1); rec["n_levels2"] = len(s2)
        rec["R"][0] = np.asarray(R, np.float32).reshape(9); rec["t"][0] = np.asarray(t, np.float32).reshape(3)
        rec["s"] = np.float32(s); rec["th2"] = np.float32(th2); rec["fix_scale"] = 1 if fix_scale else 0
        self.rec = rec
        self.x3dc1 = np.ascontiguousarray(x3dc1, np.float32).reshape(-1, 3)
        self.x3dc2 = np.ascontiguousarray(x3dc2, np.float32).reshape(-1, 3)
        self.obs1 = np.ascontiguousarray(obs1, np.float32).reshape(-1, 2)
        self.obs2 = np.ascontiguousarray(obs2, np.float32).reshape(-1, 2)
        self.octave1 = np.ascontiguousarray(octave1, np.int32); self.octave2 = np.ascontiguousarray(octave2, np.int32)
        self.n = len(self.x3dc1)
        assert len(self.x3dc2) == len(self.obs1) == len(self.obs2) == len(self.octave1) == len(self.octave2) == self.n


def _sim3opt_pack(problems):
    recs = np.concatenate([p.rec for p in problems])
    first = np.zeros(len(problems) + 1, np.int32)
    first[1:] = np.cumsum([p.n for p in problems])
    cat = lambda name, dt, shape: np.ascontiguousarray(np.concatenate([getattr(p, name) for p in problems]).reshape(shape), dt)
    arrays = (cat("x3dc1", np.float32, (-1, 3)), cat("x3dc2", np.float32, (-1, 3)), cat("obs1", np.float32, (-1, 2)),
              cat("obs2", np.float32, (-1, 2)), cat("octave1", np.int32, (-1,)), cat("octave2", np.int32, (-1,)))
    flags = np.zeros(max(int(first[-1]), 1), np.uint8); res = np.zeros(len(problems), SIM3OPT_RESULT_DTYPE)
    return recs, first, arrays, flags, res


def _sim3opt_unpack(problems, first, flags, res):
    return [(res[b].copy(), flags[first[b]:first[b + 1]].copy()) for b in range(len(problems))]


def sim3_optimize_host(problems, order=POSE_ORDER_INDEX):
    """orbm_sim3_optimize_host: the batch entirely on the host (no device needed), sums in index order with the C library's sin / cos /
    exp (the restatement of the reference) or in the kernel's order with the device's sequences
    -> [(SIM3OPT_RESULT_DTYPE record, flag per correspondence: 0 kept, 1 removed after the first optimisation, 2 failed the final test)]."""
    recs, first, arrays, flags, res = _sim3opt_pack(problems)
    check(_lib.lib().orbm_sim3_optimize_host(ptr(recs), len(problems), ptr(first), *[ptr(a) for a in arrays], int(order), ptr(flags), ptr(res)))
    return _sim3opt_unpack(problems, first, flags, res)


def sim3opt_exp(x):
    """The exponential of the device order of the Sim3 refinement (orbm_sim3opt_exp)."""
    return float(_lib.lib().orbm_sim3opt_exp(float(x)))


def sim3opt_expmap(update, order=POSE_ORDER_INDEX):
    """g2o::Sim3(Vector7d) as the library restates it (orbm_sim3opt_expmap) -> (q 4, t 3, s, branch)."""
    u = np.ascontiguousarray(update, np.float64); out = np.zeros(8)
    assert len(u) == 7
    branch = _lib.lib().orbm_sim3opt_expmap(ptr(u), int(order), ptr(out))
    return out[:4].copy(), out[4:7].copy(), float(out[7]), int(branch)


def sim3opt_ldlt7(A, b):
    """The 7 x 7 LDLT solve of a Levenberg trial (orbm_sim3opt_ldlt7) -> (isPositive, x)."""
    A = np.array(A, np.float64).reshape(49); b = np.ascontiguousarray(b, np.float64); x = np.zeros(7)
    ok = _lib.lib().orbm_sim3opt_ldlt7(ptr(A), ptr(b), ptr(x))
    return bool(ok), x


class LocalBAProblem:
    """One Optimizer::LocalBundleAdjustment from its graph on (orbm_lba_problem): Tcw n_poses x 4 x 4 float (the free poses first, n_free
    of them), K n_poses x 5 (fx fy cx cy mbf), points n_points x 3, first n_points + 1 (the CSR of the edges per point), edge_pose,
    edge_cam, obs n_edges x 3 (u v ur; ur < 0: mono), inv_sigma2, Tcim 2 x 4 x 4, bad n_points or None."""

    def __init__(self, n_free, Tcw, K, points, first, edge_pose, edge_cam, obs, inv_sigma2, Tcim, bad=None):
        self.Tcw = np.ascontiguousarray(Tcw, np.float32).reshape(-1, 16); self.K = np.ascontiguousarray(K, np.float32).reshape(-1, 5)
        self.points = np.ascontiguousarray(points, np.float32).reshape(-1, 3); self.first = np.ascontiguousarray(first, np.int32)
        self.edge_pose = np.ascontiguousarray(edge_pose, np.int32); self.edge_cam = np.ascontiguousarray(edge_cam, np.uint8)
        self.obs = np.ascontiguousarray(obs, np.float32).reshape(-1, 3); self.inv_sigma2 = np.ascontiguousarray(inv_sigma2, np.float32)
        self.Tcim = np.ascontiguousarray(Tcim, np.float32).reshape(32)
        self.bad = None if bad is None else np.ascontiguousarray(bad, np.uint8)
        self.n_free = int(n_free); self.n_poses = len(self.Tcw); self.n_points = len(self.points); self.n_edges = len(self.edge_pose)
        assert len(self.K) == self.n_poses and len(self.first) == self.n_points + 1 and int(self.first[-1]) == self.n_edges
        assert len(self.edge_cam) == len(self.obs) == len(self.inv_sigma2) == self.n_edges
        assert self.bad is None or len(self.bad) == self.n_points

    def native(self):
        P = _lib.LbaProblem()
        P.n_free, P.n_poses, P.n_points, P.reserved = self.n_free, self.n_poses, self.n_points, 0
        for k in ("Tcw", "K", "points", "first", "edge_pose", "edge_cam", "obs", "inv_sigma2"):
            setattr(P, k, getattr(self, k).ctypes.data)
        P.bad = None if self.bad is None else self.bad.ctypes.data
        P.Tcim[:] = [float(v) for v in self.Tcim]
        return P


class LocalBAResult:
    """orbm_lba_result: pose n_poses x 7 (q x y z w, t) and Tcw n_poses x 16 (what SetPose receives), point / point_f n_points x 3, flags per
    edge (LBA_FLAG_LEVEL1 | LBA_FLAG_ERASE), rounds [(iterations, trials, chi2, lambda)] x 2, ended (LBA_ENDED_*), optimisations, polls,
    n_level1, n_erase, active_poses / active_points / active_edges of either optimisation."""
    FIELDS = ("pose", "Tcw", "point", "point_f", "flags", "rounds", "ended", "optimisations", "polls", "n_level1", "n_erase", "active_poses",
              "active_points", "active_edges")

    def __init__(self, problem):
        self.pose = np.zeros((problem.n_poses, 7)); self.Tcw = np.zeros((problem.n_poses, 16), np.float32)
        self.point = np.zeros((problem.n_points, 3)); self.point_f = np.zeros((problem.n_points, 3), np.float32)
        self.flags = np.zeros(problem.n_edges, np.uint8)
        self._pad = [np.zeros(1, a.dtype) if a.size == 0 else a for a in (self.pose, self.Tcw, self.point, self.point_f, self.flags)]

    def native(self):
        R = _lib.LbaResult()
        R.pose, R.Tcw, R.point, R.point_f, R.flags = [a.ctypes.data for a in self._pad]
        return R

    def take(self, R):
        self.rounds = np.zeros(2, _lib.POSE_ROUND_DTYPE)
        for s in range(2):
            self.rounds[s] = (R.round[s].iterations, R.round[s].trials, R.round[s].chi2, R.round[s].lambda_)
        for k in ("ended", "optimisations", "polls", "n_level1", "n_erase"):
            setattr(self, k, int(getattr(R, k)))
        for k in ("active_poses", "active_points", "active_edges"):
            setattr(self, k, (int(getattr(R, k)[0]), int(getattr(R, k)[1])))
        return self

    def same_bytes(self, other):
        """The first field that differs from `other` bit for bit, or None."""
        for k in self.FIELDS:
            a, b = getattr(self, k), getattr(other, k)
            if (a.tobytes() != b.tobytes()) if isinstance(a, np.ndarray) else (a != b):
                return k
        return None


def _lba_stop(stop):
    """stop: None (no flag: nothing is polled), a callable -> truth value, or an int n: true from the n-th poll on (n = 0: at once)."""
    if stop is None:
        return _lib.LBA_STOP_FN(), None
    if callable(stop):
        fn = stop
    else:
        state = {"polls": 0}

        def fn():
            state["polls"] += 1
            return state["polls"] > int(stop)
    cb = _lib.LBA_STOP_FN(lambda ctx: 1 if fn() else 0)
    return cb, cb


def local_ba_host(problem, order=POSE_ORDER_INDEX, stop=None):
    """orbm_local_ba_host: one local bundle adjustment entirely on the host (no device needed), in the index order with the C library's
    sin / cos / pow (the restatement of the reference) or in the device's order -> LocalBAResult."""
    res = LocalBAResult(problem); P = problem.native(); R = res.native()
    cb, keep = _lba_stop(stop)
    check(_lib.lib().orbm_local_ba_host(C.byref(P), cb, None, int(order), C.byref(R)))
    return res.take(R)


class GlobalBAResult:
    """orbm_ba_result: pose n_poses x 7 (q x y z w, t) and Tcw n_poses x 16 (what SetPose / mTcwGBA receive), point / point_f
    n_points x 3, round (iterations, trials, chi2, lambda) of the one optimize(), optimised, polls, active_poses / active_points /
    active_edges of its initializeOptimization()."""
    FIELDS = ("pose", "Tcw", "point", "point_f", "round", "optimised", "polls", "active_poses", "active_points", "active_edges")

    def __init__(self, problem):
        self.pose = np.zeros((problem.n_poses, 7)); self.Tcw = np.zeros((problem.n_poses, 16), np.float32)
        self.point = np.zeros((problem.n_points, 3)); self.point_f = np.zeros((problem.n_points, 3), np.float32)
        self._pad = [np.zeros(1, a.dtype) if a.size == 0 else a for a in (self.pose, self.Tcw, self.point, self.point_f)]

    def native(self):
        R = _lib.BaResult()
        R.pose, R.Tcw, R.point, R.point_f = [a.ctypes.data for a in self._pad]
        return R

    def take(self, R):
        self.round = np.zeros(1, _lib.POSE_ROUND_DTYPE)
        self.round[0] = (R.round.iterations, R.round.trials, R.round.chi2, R.round.lambda_)
        for k in ("optimised", "polls", "active_poses", "active_points", "active_edges"):
            setattr(self, k, int(getattr(R, k)))
        return self

    same_bytes = LocalBAResult.same_bytes


def bundle_adjust_host(problem, iterations, robust, order=POSE_ORDER_INDEX, stop=None):
    """orbm_bundle_adjust_host: Optimizer::BundleAdjustment from its graph on, entirely on the host (no device needed), in either
    order -> GlobalBAResult.  problem: a LocalBAProblem (its `bad` is ignored); stop: see local_ba_host."""
    res = GlobalBAResult(problem); P = problem.native(); R = res.native()
    cb, keep = _lba_stop(stop)
    check(_lib.lib().orbm_bundle_adjust_host(C.byref(P), int(iterations), 1 if robust else 0, cb, None, int(order), C.byref(R)))
    return res.take(R)


class EssentialGraphProblem:
    """One Optimizer::OptimizeEssentialGraph from its graph on (orbm_eg_problem): vertex n_vertices x 8 double (quaternion x y z w,
    translation, scale; the free ones first, n_free of them, in ascending mnId), measurement n_edges x 8 (Sji), edge_v0 / edge_v1 (the
    vertices of Siw and Sjw; the edge position is the active-edge order), points n_points x 3 float, point_ref per point the vertex of
    its reference keyframe or -1, fix_scale."""

    def __init__(self, n_free, vertex, measurement, edge_v0, edge_v1, points=None, point_ref=None, fix_scale=False):
        self.vertex = np.ascontiguousarray(vertex, np.float64).reshape(-1, 8)
        self.measurement = np.ascontiguousarray(measurement, np.float64).reshape(-1, 8)
        self.edge_v0 = np.ascontiguousarray(edge_v0, np.int32).reshape(-1); self.edge_v1 = np.ascontiguousarray(edge_v1, np.int32).reshape(-1)
        self.points = np.ascontiguousarray(np.zeros((0, 3)) if points is None else points, np.float32).reshape(-1, 3)
        self.point_ref = np.ascontiguousarray(np.zeros(0) if point_ref is None else point_ref, np.int32).reshape(-1)
        self.n_free = int(n_free); self.n_vertices = len(self.vertex); self.n_edges = len(self.measurement); self.n_points = len(self.points)
        self.fix_scale = bool(fix_scale)
        assert len(self.edge_v0) == len(self.edge_v1) == self.n_edges and len(self.point_ref) == self.n_points
        assert 0 <= self.n_free <= self.n_vertices

    def native(self):
        P = _lib.EgProblem()
        P.n_free, P.n_vertices, P.n_edges, P.n_points, P.fix_scale = self.n_free, self.n_vertices, self.n_edges, self.n_points, int(self.fix_scale)
        for k in ("vertex", "measurement", "edge_v0", "edge_v1", "points", "point_ref"):
            a = getattr(self, k)
            setattr(P, k, a.ctypes.data if a.size else None)
        return P


class EssentialGraphResult:
    """orbm_eg_result: estimate n_vertices x 8 (q x y z w, t, s), Tiw n_vertices x 16 (what SetPose receives), point_f n_points x 3 (what
    SetWorldPos receives), round (iterations, trials, chi2, lambda) of the one optimize(), optimised, active_vertices / active_edges of
    its initializeOptimization()."""
    FIELDS = ("estimate", "Tiw", "point_f", "round", "optimised", "active_vertices", "active_edges")

    def __init__(self, problem):
        self.estimate = np.zeros((problem.n_vertices, 8)); self.Tiw = np.zeros((problem.n_vertices, 16), np.float32)
        self.point_f = np.zeros((problem.n_points, 3), np.float32)
        self._pad = [np.zeros(1, a.dtype) if a.size == 0 else a for a in (self.estimate, self.Tiw, self.point_f)]

    def native(self):
        R = _lib.EgResult()
        R.estimate, R.Tiw, R.point_f = [a.ctypes.data for a in self._pad]
        return R

    def take(self, R):
        self.round = np.zeros(1, _lib.POSE_ROUND_DTYPE)
        self.round[0] = (R.round.iterations, R.round.trials, R.round.chi2, R.round.lambda_)
        for k in ("optimised", "active_vertices", "active_edges"):
            setattr(self, k, int(getattr(R, k)))
        return self

    same_bytes = LocalBAResult.same_bytes


def essential_graph_host(problem, iterations=20, order=POSE_ORDER_INDEX):
    """orbm_essential_graph_host: Optimizer::OptimizeEssentialGraph from its graph on, entirely on the host (no device needed), in
    either order -> EssentialGraphResult."""
    res = EssentialGraphResult(problem); P = problem.native(); R = res.native()
    check(_lib.lib().orbm_essential_graph_host(C.byref(P), int(iterations), int(order), C.byref(R)))
    return res.take(R)


def eg_edge_eval(measurement, v0, v1, fix_scale=False, order=POSE_ORDER_INDEX):
    """One edge of the essential graph at two estimates, 8 doubles each (orbm_eg_edge_eval) -> (error 7, chi2, Jacobian by vertex 0
    7 x 7, by vertex 1 7 x 7; row: the error, column: the dimension)."""
    M = np.ascontiguousarray(measurement, np.float64).reshape(8); a = np.ascontiguousarray(v0, np.float64).reshape(8)
    b = np.ascontiguousarray(v1, np.float64).reshape(8); out = np.zeros(106)
    check(_lib.lib().orbm_eg_edge_eval(ptr(M), ptr(a), ptr(b), 1 if fix_scale else 0, int(order), ptr(out)))
    return out[:7].copy(), float(out[7]), out[8:57].reshape(7, 7).copy(), out[57:106].reshape(7, 7).copy()


def sim3_log_eval(sim3, order=POSE_ORDER_INDEX):
    """g2o's Sim3::log() of (q x y z w, t, s) (orbm_sim3_log_eval) -> (omega, upsilon, sigma as 7 doubles, the branch taken)."""
    T = np.ascontiguousarray(sim3, np.float64).reshape(8); out = np.zeros(7)
    rc = _lib.lib().orbm_sim3_log_eval(ptr(T), int(order), ptr(out))
    if rc < 0:
        check(rc)
    return out, int(rc)


def pose_acos(d):
    """The arc cosine of the device order (orbm_pose_acos): d in [-1, 1]."""
    return float(_lib.lib().orbm_pose_acos(float(d)))


def pose_log(x):
    """The natural logarithm of the device order (orbm_pose_log)."""
    return float(_lib.lib().orbm_pose_log(float(x)))


def ba_ldlt(H, b):
    """The solver of the global BA's reduced system on the host (orbm_ba_ldlt: the local BA's factorisation, the backward substitution
    in descending order) -> x, or None on a zero or non-finite pivot."""
    H = np.ascontiguousarray(H, np.float64); b = np.ascontiguousarray(b, np.float64); x = np.zeros(len(b))
    rc = _lib.lib().orbm_ba_ldlt(len(b), ptr(H), ptr(b), ptr(x))
    if rc < 0:
        check(rc)
    return x if rc == 1 else None


def lba_edge_eval(Tcim, K5, pose7, point3, cam, obs3, inv_sigma2):
    """One edge of the local BA (orbm_lba_edge_eval) -> (error 3, chi2, depth, Jacobian by the point 3 x 3, by the pose 3 x 6)."""
    Tcim = np.ascontiguousarray(Tcim, np.float32).reshape(32); K5 = np.ascontiguousarray(K5, np.float32)
    pose7 = np.ascontiguousarray(pose7, np.float64); point3 = np.ascontiguousarray(point3, np.float64)
    obs3 = np.ascontiguousarray(obs3, np.float32); out = np.zeros(32)
    check(_lib.lib().orbm_lba_edge_eval(ptr(Tcim), ptr(K5), ptr(pose7), ptr(point3), int(cam), ptr(obs3), float(inv_sigma2), ptr(out)))
    return out[:3].copy(), float(out[3]), float(out[4]), out[5:14].reshape(3, 3).copy(), out[14:32].reshape(3, 6).copy()


def lba_ldlt(H, b):
    """The dense LDL^T without pivoting of the local BA's reduced system (orbm_lba_ldlt) -> x, or None on a zero or non-finite pivot."""
    H = np.ascontiguousarray(H, np.float64); b = np.ascontiguousarray(b, np.float64); x = np.zeros(len(b))
    return x if _lib.lib().orbm_lba_ldlt(len(b), ptr(H), ptr(b), ptr(x)) == 1 else None


def lba_controller_trace(chi, hdiag6, b6, max_iter, order=POSE_ORDER_INDEX):
    """The local BA's controller and lm_step on one stream of chi2 values (orbm_lba_controller_trace) -> (steps x 3 of the local BA,
    steps x 3 of lm_step): lambda, ni, verdict (1 a trial follows, 2 the next iteration, 3 optimize() returned)."""
    chi = np.ascontiguousarray(chi, np.float64); h = np.ascontiguousarray(hdiag6, np.float64); b = np.ascontiguousarray(b6, np.float64)
    a = np.zeros((len(chi) + 1, 3)); l = np.zeros((len(chi) + 1, 3))
    n = _lib.lib().orbm_lba_controller_trace(ptr(chi), len(chi), ptr(h), ptr(b), int(max_iter), int(order), len(chi), ptr(a), ptr(l))
    if n < 0:
        raise AssertionError("the two controllers took a different number of steps (%d)" % (-1 - n))
    return a[:n].copy(), l[:n].copy()


class LocalPoints:
    """A table of map points resident in HBM (orbm_points): what isInFrustum and the search read of each MapPoint."""

    def __init__(self, matcher, capacity):
        self._m = matcher; self.capacity = int(capacity)
        self._h = C.c_void_p()
        check(_lib.lib().orbm_points_create(matcher._h, self.capacity, C.byref(self._h)))

    def write(self, first, points):
        """Rows [first, first + len(points)) of the table (POINT_DTYPE); any sub-range."""
        points = np.ascontiguousarray(points, POINT_DTYPE)
        check(_lib.lib().orbm_points_write(self._m._h, self._h, int(first), len(points), ptr(points)))

    @property
    def count(self):
        """High-water mark: one past the last row ever written (orbm_points_count)."""
        n = int(_lib.lib().orbm_points_count(self._h))
        if n < 0:
            raise _lib.OrbError(n, "orbm_points_count on a closed table")
        return n

    def close(self):
        if getattr(self, "_h", None):
            try:
                _lib.lib().orbm_points_destroy(self._h)
            except Exception:
                pass
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def _i32(a):
    return np.ascontiguousarray(a, np.int32).reshape(-1)


def local_map_vote_host(obs, point_flags, frame_points, n_kfs):
    """orbm_local_map_vote_host: keyframeCounter of UpdateLocalKeyFrames (reference src/Tracking.cc:1838-1855) on plain arrays: obs
    OBS_DTYPE records (point -1 = free), point_flags one byte per point slot (bit 0 = bad), frame_points the point slot of every
    feature of the frame or -1 -> votes[n_kfs]."""
    obs = np.ascontiguousarray(obs, OBS_DTYPE); fl = np.ascontiguousarray(point_flags, np.uint8); fp = _i32(frame_points)
    votes = np.zeros(max(int(n_kfs), 1), np.int32)
    check(_lib.lib().orbm_local_map_vote_host(ptr(obs), len(obs), ptr(fl), len(fl), ptr(fp), len(fp), int(n_kfs), ptr(votes)))
    return votes[:int(n_kfs)]


def local_map_points_host(kf_rows, kf_count, point_flags, local_kfs, list_cap=MAX_POINTS):
    """orbm_local_map_points_host: UpdateLocalPoints (reference src/Tracking.cc:1794-1824) on plain arrays: kf_rows n_kfs x stride point
    slots (-1 = none), kf_count the features of every keyframe, local_kfs the local keyframes in order -> the kept slots in order."""
    rows = np.ascontiguousarray(kf_rows, np.int32); assert rows.ndim == 2
    cnt = _i32(kf_count); fl = np.ascontiguousarray(point_flags, np.uint8); lk = _i32(local_kfs)
    assert len(cnt) == rows.shape[0]
    out = np.zeros(max(int(list_cap), 1), np.int32); n = C.c_int()
    check(_lib.lib().orbm_local_map_points_host(ptr(rows), ptr(cnt), rows.shape[0], max(rows.shape[1], 1), ptr(fl), len(fl), ptr(lk),
                                                len(lk), ptr(out), int(list_cap), C.byref(n)))
    return out[:n.value].copy()


def _split_covisibility(first, entries):
    return [entries[first[j]:first[j + 1]].copy() for j in range(len(first) - 1)]


def local_map_covisibility_host(obs, obs_feature, point_flags, kf_rows, kf_count, kf_n_cam1, kfs):
    """orbm_local_map_covisibility_host: KFcounter / KFcounter_cam1 of KeyFrame::UpdateConnections (reference src/KeyFrame.cc:512-552) on
    plain arrays: obs OBS_DTYPE records with obs_feature their feature indices, kf_rows n_kfs x stride point slots, kf_n_cam1 the
    camera-1 feature count of every keyframe -> one COVIS_DTYPE array per listed keyframe (all > 0, ascending keyframe slot)."""
    obs = np.ascontiguousarray(obs, OBS_DTYPE); of = _i32(obs_feature); fl = np.ascontiguousarray(point_flags, np.uint8)
    rows = np.ascontiguousarray(kf_rows, np.int32); assert rows.ndim == 2
    cnt = _i32(kf_count); nc = _i32(kf_n_cam1); ks = _i32(kfs)
    assert len(of) == len(obs) and len(cnt) == rows.shape[0] == len(nc)
    first = np.zeros(len(ks) + 1, np.int32)
    cap = max(len(ks) * rows.shape[0], 1)   # a keyframe has at most one entry per other keyframe
    ent = np.zeros(cap, COVIS_DTYPE)
    check(_lib.lib().orbm_local_map_covisibility_host(ptr(obs), ptr(of), len(obs), ptr(fl), len(fl), ptr(rows), ptr(cnt), ptr(nc),
                                                      rows.shape[0], max(rows.shape[1], 1), ptr(ks), len(ks), ptr(first), ptr(ent), cap))
    return _split_covisibility(first, ent)


def local_map_culling_host(obs, obs_feature, point_flags, point_n_obs, kf_rows, kf_count, kf_feature_bytes, kfs, mono=False):
    """orbm_local_map_culling_host: nMPs and nRedundantObservations of LocalMapping::KeyFrameCulling (reference src/LocalMapping.cc:990-1032)
    on plain arrays: kf_feature_bytes n_kfs x stride (bits 0-4 the level, bit 7 far), point_n_obs MapPoint::Observations() of every
    point slot -> counts[len(kfs), 2]."""
    obs = np.ascontiguousarray(obs, OBS_DTYPE); of = _i32(obs_feature); fl = np.ascontiguousarray(point_flags, np.uint8); no = _i32(point_n_obs)
    rows = np.ascontiguousarray(kf_rows, np.int32); fb = np.ascontiguousarray(kf_feature_bytes, np.uint8)
    assert rows.ndim == 2 and fb.shape == rows.shape and len(no) == len(fl) and len(of) == len(obs)
    cnt = _i32(kf_count); ks = _i32(kfs)
    assert len(cnt) == rows.shape[0]
    out = np.zeros((max(len(ks), 1), 2), np.int32)
    check(_lib.lib().orbm_local_map_culling_host(ptr(obs), ptr(of), len(obs), ptr(fl), ptr(no), len(fl), ptr(rows), ptr(cnt), ptr(fb),
                                                 rows.shape[0], max(rows.shape[1], 1), ptr(ks), len(ks), int(bool(mono)), ptr(out)))
    return out[:len(ks)]


def _f32(a, cols):
    a = np.ascontiguousarray(a, np.float32)
    return a.reshape(-1, cols)


def _f64(a, cols):
    return np.ascontiguousarray(a, np.float64).reshape(-1, cols)


def _raise_needed(rc, needed):
    """check(rc), the number an ORB_E_CAPACITY call reports attached to the exception as .needed."""
    if rc != _lib.ORB_OK:
        e = _lib.OrbError(rc, _lib.lib().orb_last_error().decode("utf-8", "replace"))
        e.needed = int(needed)
        raise e


def local_map_correct_sim3_host(kf_rows, kf_count, point_flags, pos, kfs, sim3_before, sim3_after, already=(), cap=None):
    """orbm_local_map_correct_sim3_host: step 4.2 of LoopClosing::CorrectLoop (reference src/LoopClosing.cc:678-710) on plain arrays: pos
    n_points x 3 float32 (not modified), kfs the keyframes in CorrectedSim3's order with their NonCorrectedSim3 / CorrectedSim3 as rows of
    8 doubles (quaternion x y z w, translation, scale), already the point slots to skip -> (entries CORRECT_DTYPE, pos_out k x 3, Tiw n x
    4 x 4, the new n_points x 3 positions).  cap None: room for every candidate.  Beyond cap: OrbError with .needed."""
    rows = np.ascontiguousarray(kf_rows, np.int32); assert rows.ndim == 2
    cnt = _i32(kf_count); fl = np.ascontiguousarray(point_flags, np.uint8); ks = _i32(kfs); al = _i32(already)
    P = _f32(pos, 3).copy(); sb = _f64(sim3_before, 8); sa = _f64(sim3_after, 8)
    assert len(cnt) == rows.shape[0] and len(P) == len(fl) and len(sb) == len(sa) == len(ks)
    cap = int(cnt[ks].sum()) if cap is None else int(cap)
    ent = np.zeros(max(cap, 1), _lib.CORRECT_DTYPE); out = np.zeros((max(cap, 1), 3), np.float32); n = C.c_int()
    tiw = np.zeros((max(len(ks), 1), 4, 4), np.float32)
    rc = _lib.lib().orbm_local_map_correct_sim3_host(ptr(rows), ptr(cnt), rows.shape[0], max(rows.shape[1], 1), ptr(fl), ptr(P), 3, len(fl),
                                                     ptr(ks), len(ks), ptr(sb), ptr(sa), ptr(al), len(al), ptr(ent), ptr(out), cap,
                                                     C.byref(n), ptr(tiw))
    _raise_needed(rc, n.value)
    return ent[:n.value].copy(), out[:n.value].copy(), tiw[:len(ks)], P


def local_map_correct_rigid_host(pos, point_flags, point_ref, slots, kf_corrected, Tcw_before, Twc_after, gba_slots=(), gba_pos=()):
    """orbm_local_map_correct_rigid_host: the map-point update after global BA (reference src/LoopClosing.cc:953-989) on plain arrays: pos
    n_points x 3 float32 (not modified), point_ref the keyframe slot of every point's reference keyframe, slots the points to visit (None:
    all), kf_corrected one byte per keyframe, Tcw_before / Twc_after n_kfs x 12 (rows 0-2 of mTcwBefGBA and of GetPoseInverse()),
    gba_slots / gba_pos the points that take mPosGBA -> (status uint8, pos_out, the new n_points x 3 positions)."""
    P = _f32(pos, 3).copy(); fl = np.ascontiguousarray(point_flags, np.uint8); rf = _i32(point_ref)
    sl = None if slots is None else _i32(slots)
    kc = np.ascontiguousarray(kf_corrected, np.uint8).reshape(-1); tb = _f32(Tcw_before, 12); ta = _f32(Twc_after, 12)
    gs = _i32(gba_slots); gp = _f32(gba_pos, 3)
    assert len(P) == len(fl) == len(rf) and len(kc) == len(tb) == len(ta) and len(gs) == len(gp)
    n = len(P) if sl is None else len(sl)
    st = np.zeros(max(n, 1), np.uint8); out = np.zeros((max(n, 1), 3), np.float32)
    check(_lib.lib().orbm_local_map_correct_rigid_host(ptr(P), 3, ptr(fl), ptr(rf), len(P), None if sl is None else ptr(sl), n, ptr(kc),
                                                       ptr(tb), ptr(ta), len(kc), ptr(gs), ptr(gp), len(gs), ptr(st), ptr(out)))
    return st[:n], out[:n], P


class ResidentMap:
    """A map resident in HBM under stable slots (orbm_map): one slot per map point (a POINT_DTYPE row + a flag byte, bit 0 = bad),
    per keyframe (mvpMapPoints as point slots) and per observation (OBS_DTYPE), and Tracking::UpdateLocalMap's data-parallel parts
    over it: vote, local_points, search."""

    def __init__(self, matcher, kf_capacity, point_capacity, obs_capacity, features_per_keyframe):
        self._m = matcher; self._h = C.c_void_p()
        self.kf_capacity, self.point_capacity, self.obs_capacity = int(kf_capacity), int(point_capacity), int(obs_capacity)
        self.features_per_keyframe = int(features_per_keyframe)
        check(_lib.lib().orbm_map_create(matcher._h, self.kf_capacity, self.point_capacity, self.obs_capacity,
                                         self.features_per_keyframe, C.byref(self._h)))

    def _write(self, name, slots, values):
        """One value per listed slot into a column (orbm_map_write_<name>)."""
        slots = _i32(slots)
        assert len(values) == len(slots)
        check(getattr(_lib.lib(), "orbm_map_write_" + name)(self._m._h, self._h, ptr(slots), len(slots), ptr(values)))

    def _last(self, name):
        out = (C.c_int * 4)()
        check(getattr(_lib.lib(), "orbm_debug_last_" + name)(self._h, out))
        return tuple(out)

    def _high_water(self, name):
        n = int(getattr(_lib.lib(), name)(self._h))
        if n < 0:
            raise _lib.OrbError(n, name + " on a closed map")
        return n

    def write_points(self, slots, rows, flags=None):
        """Rows (POINT_DTYPE) and flag bytes into the listed point slots, one call (orbm_map_write_points)."""
        slots = _i32(slots); rows = np.ascontiguousarray(rows, POINT_DTYPE)
        fl = None if flags is None else np.ascontiguousarray(flags, np.uint8)
        assert len(rows) == len(slots) and (fl is None or len(fl) == len(slots))
        check(_lib.lib().orbm_map_write_points(self._m._h, self._h, ptr(slots), len(slots), ptr(rows), None if fl is None else ptr(fl)))

    def write_observations(self, slots, records):
        """Records (OBS_DTYPE; point -1 frees the slot) into the listed record slots (orbm_map_write_observations)."""
        self._write("observations", slots, np.ascontiguousarray(records, OBS_DTYPE))

    def write_keyframe(self, kf, point_of_feature, bad=False):
        pof = _i32(point_of_feature)
        check(_lib.lib().orbm_map_write_keyframe(self._m._h, self._h, int(kf), ptr(pof), len(pof), int(bool(bad))))

    def set_keyframe_bad(self, kf, bad=True):
        check(_lib.lib().orbm_map_set_keyframe_bad(self._m._h, self._h, int(kf), int(bool(bad))))

    @property
    def keyframes(self):
        """Keyframe high-water mark (orbm_map_keyframes)."""
        return self._high_water("orbm_map_keyframes")

    def keyframe_bad(self, kf):
        r = int(_lib.lib().orbm_map_keyframe_bad(self._h, int(kf)))
        check(min(r, 0))
        return bool(r)

    def vote(self, frame_points):
        """orbm_map_vote -> votes[keyframes]."""
        fp = _i32(frame_points); votes = np.zeros(max(self.kf_capacity, 1), np.int32)
        check(_lib.lib().orbm_map_vote(self._m._h, self._h, ptr(fp), len(fp), ptr(votes)))
        return votes[:self.keyframes]

    def local_points(self, local_kfs):
        """orbm_map_local_points -> the kept point slots in order; the list stays on the device for search()."""
        lk = _i32(local_kfs); out = np.zeros(MAX_POINTS, np.int32); n = C.c_int()
        check(_lib.lib().orbm_map_local_points(self._m._h, self._h, ptr(lk), len(lk), ptr(out), C.byref(n)))
        return out[:n.value].copy()

    def search(self, frame, view, frame_points=(), seen=(), occupied=None, th_high=TH_HIGH, n_list=None, want_track=True):
        """orbm_map_search_local_points over the list of the last local_points() -> (n_to_match, nmatches, match_of_feature, track);
        match_of_feature and track index the LIST.  n_list: the length of that list (sizes `track`; default the largest a list has)."""
        fp = _i32(frame_points); sn = _i32(seen)
        occ = None if occupied is None else np.ascontiguousarray(occupied, np.uint8)
        assert occ is None or len(occ) >= frame.data.n_total
        n = MAX_POINTS if n_list is None else int(n_list)
        mo = np.zeros(max(frame.data.n_total, 1), np.int32); nm = C.c_int(); nt = C.c_int()
        track = np.zeros(max(n, 1), TRACK_DTYPE) if want_track else None
        check(_lib.lib().orbm_map_search_local_points(self._m._h, frame._h, self._h, C.byref(view.c), ptr(fp), len(fp), ptr(sn), len(sn),
                                                      None if occ is None else ptr(occ), self._m.nnratio, th_high,
                                                      None if track is None else ptr(track), ptr(mo), C.byref(nt), C.byref(nm)))
        return nt.value, nm.value, mo[:frame.data.n_total], (None if track is None else track[:n])

    def last_local_map(self):
        """(1 if the last vote / point list ran on the device, records scanned by the last vote, candidates of the last point list,
        points it kept) (orbm_debug_last_local_map)."""
        return self._last("local_map")

    def write_observation_features(self, slots, feature):
        """The feature index of each listed record in its keyframe (orbm_map_write_observation_features)."""
        self._write("observation_features", slots, _i32(feature))

    def write_keyframe_features(self, kf, feature_bytes, n_cam1):
        """One byte per feature of keyframe slot kf (bits 0-4 the level, bit 7 far) and its camera-1 feature count
        (orbm_map_write_keyframe_features)."""
        fb = np.ascontiguousarray(feature_bytes, np.uint8).reshape(-1)
        check(_lib.lib().orbm_map_write_keyframe_features(self._m._h, self._h, int(kf), ptr(fb), len(fb), int(n_cam1)))

    def write_point_nobs(self, slots, n_obs):
        """MapPoint::Observations() of each listed point slot (orbm_map_write_point_nobs)."""
        self._write("point_nobs", slots, _i32(n_obs))

    def covisibility(self, kfs, entries_cap=None):
        """orbm_map_covisibility -> one COVIS_DTYPE array per listed keyframe (all > 0, ascending keyframe slot).  entries_cap None:
        room for every keyframe of the map per listed one, up to 2^20 entries; a call that reports ORB_E_CAPACITY beyond that is
        repeated once with the room it asked for."""
        ks = _i32(kfs); first = np.zeros(len(ks) + 1, np.int32)
        cap = min(len(ks) * max(self.keyframes, 1), 1 << 20) if entries_cap is None else int(entries_cap)
        for _ in range(2):
            ent = np.zeros(max(cap, 1), COVIS_DTYPE)
            rc = _lib.lib().orbm_map_covisibility(self._m._h, self._h, ptr(ks), len(ks), ptr(first), ptr(ent), cap)
            if rc != _lib.ORB_E_CAPACITY or entries_cap is not None or int(first[len(ks)]) <= cap:
                break
            cap = int(first[len(ks)])
        check(rc)
        return _split_covisibility(first, ent)

    def culling_counts(self, kfs, mono=False):
        """orbm_map_culling_counts -> counts[len(kfs), 2]: nMPs, nRedundantObservations."""
        ks = _i32(kfs); out = np.zeros((max(len(ks), 1), 2), np.int32)
        check(_lib.lib().orbm_map_culling_counts(self._m._h, self._h, ptr(ks), len(ks), int(bool(mono)), ptr(out)))
        return out[:len(ks)]

    def last_covisibility(self):
        """(1 if the last covisibility / culling call ran on the device, 1 if it rebuilt the point -> records index, records indexed,
        keyframes processed) (orbm_debug_last_covisibility)."""
        return self._last("covisibility")

    @property
    def points(self):
        """Point high-water mark (orbm_map_points)."""
        return self._high_water("orbm_map_points")

    def write_positions(self, slots, pos):
        """The position field alone of the listed point slots (orbm_map_write_positions)."""
        self._write("positions", slots, _f32(pos, 3))

    def write_point_ref(self, slots, ref_kf):
        """The keyframe slot of each listed point's reference keyframe (orbm_map_write_point_ref)."""
        self._write("point_ref", slots, _i32(ref_kf))

    def correct_sim3(self, kfs, sim3_before, sim3_after, already=(), cap=None):
        """orbm_map_correct_sim3 -> (entries CORRECT_DTYPE, pos_out k x 3, Tiw n x 4 x 4); the rows change in place.  cap None: room for
        every point slot of the map.  Beyond cap: OrbError with .needed, and nothing has changed."""
        ks = _i32(kfs); al = _i32(already); sb = _f64(sim3_before, 8); sa = _f64(sim3_after, 8)
        assert len(sb) == len(sa) == len(ks)
        cap = self.point_capacity if cap is None else int(cap)
        ent = np.zeros(max(cap, 1), _lib.CORRECT_DTYPE); out = np.zeros((max(cap, 1), 3), np.float32); n = C.c_int()
        tiw = np.zeros((max(len(ks), 1), 4, 4), np.float32)
        rc = _lib.lib().orbm_map_correct_sim3(self._m._h, self._h, ptr(ks), len(ks), ptr(sb), ptr(sa), ptr(al), len(al), ptr(ent), ptr(out),
                                              cap, C.byref(n), ptr(tiw))
        _raise_needed(rc, n.value)
        return ent[:n.value].copy(), out[:n.value].copy(), tiw[:len(ks)]

    def correct_rigid(self, slots, kf_corrected, Tcw_before, Twc_after, gba_slots=(), gba_pos=()):
        """orbm_map_correct_rigid over the listed point slots (None: every slot below the high-water mark) -> (status uint8, pos_out);
        the rows change in place."""
        sl = None if slots is None else _i32(slots)
        kc = np.ascontiguousarray(kf_corrected, np.uint8).reshape(-1); tb = _f32(Tcw_before, 12); ta = _f32(Twc_after, 12)
        gs = _i32(gba_slots); gp = _f32(gba_pos, 3)
        assert len(kc) == len(tb) == len(ta) and len(gs) == len(gp)
        n = self.points if sl is None else len(sl)
        st = np.zeros(max(n, 1), np.uint8); out = np.zeros((max(n, 1), 3), np.float32)
        check(_lib.lib().orbm_map_correct_rigid(self._m._h, self._h, None if sl is None else ptr(sl), n, ptr(kc), ptr(tb), ptr(ta), len(kc),
                                                ptr(gs), ptr(gp), len(gs), ptr(st), ptr(out)))
        return st[:n], out[:n]

    def last_correction(self):
        """(1 if the last correct_sim3 / correct_rigid ran on the device, candidates, points kept or changed, keyframes)
        (orbm_debug_last_correction)."""
        return self._last("correction")

    def read_points(self, slots):
        """The rows of the listed point slots as HBM holds them, not the mirror (orbm_debug_map_read_points)."""
        slots = _i32(slots); rows = np.zeros(max(len(slots), 1), POINT_DTYPE)
        check(_lib.lib().orbm_debug_map_read_points(self._m._h, self._h, ptr(slots), len(slots), ptr(rows)))
        return rows[:len(slots)]

    def close(self):
        if getattr(self, "_h", None):
            try:
                _lib.lib().orbm_map_destroy(self._h)
            except Exception:
                pass
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class FrameData:
    """Flat arrays of the Frame members the matcher reads (reference src/Frame.cc:191-288): cam-major global index."""

    def __init__(self, un_x, un_y, octave, angle, uright, cam_of, local_of, descs, bounds):
        self.un_x = np.ascontiguousarray(un_x, np.float32); self.un_y = np.ascontiguousarray(un_y, np.float32)
        self.octave = np.ascontiguousarray(octave, np.int32); self.angle = np.ascontiguousarray(angle, np.float32)
        self.uright = np.ascontiguousarray(uright, np.float32)
        self.cam_of = np.ascontiguousarray(cam_of, np.int32); self.local_of = np.ascontiguousarray(local_of, np.int32)
        self.descs = [np.ascontiguousarray(d, np.uint8) for d in descs]
        self.bounds = tuple(float(b) for b in bounds)
        self.n_total = len(self.un_x); self.n_cams = len(self.descs)
        self._ptrs = (C.c_void_p * self.n_cams)(*[d.ctypes.data for d in self.descs])
        self.c = FrameDesc(self.n_total, self.n_cams, self.un_x.ctypes.data, self.un_y.ctypes.data,
                           self.octave.ctypes.data, self.angle.ctypes.data, self.uright.ctypes.data,
                           self.cam_of.ctypes.data, self.local_of.ctypes.data, C.cast(self._ptrs, C.c_void_p),
                           *self.bounds)

    @staticmethod
    def from_cameras(per_cam, width, height, uright=None):
        """Frame merge (reference src/Frame.cc:191-239): per_cam = [(keypoints, descriptors), ...] -> `_total` arrays.
        Undistortion is the identity (k1 == 0) and the image bounds are [0,W]x[0,H] (Frame.cc:743-779)."""
        xs, ys, octs, angs, cams, locs, descs = [], [], [], [], [], [], []
        for c, (k, d) in enumerate(per_cam):
            xs.append(k["x"]); ys.append(k["y"]); octs.append(k["octave"]); angs.append(k["angle"])
            cams.append(np.full(len(k), c, np.int32)); locs.append(np.arange(len(k), dtype=np.int32)); descs.append(d)
        cat = np.concatenate
        n = sum(len(x) for x in xs)
        ur = np.full(n, -1.0, np.float32) if uright is None else uright
        return FrameData(cat(xs), cat(ys), cat(octs), cat(angs), ur, cat(cams), cat(locs), descs, (0, 0, width, height))


class _Count:
    def __init__(self, n_total, n_cams):
        self.n_total, self.n_cams = n_total, n_cams


class Frame:
    def __init__(self, matcher, data=None, handle=None, n_total=0, n_cams=0, resident=None):
        """resident: None -> orbm_frame_create (host-built grid, every array sent); a list with one entry per camera -- a DEVICE
        pointer to that camera's descriptor rows, or 0 / None -- -> orbm_frame_create_resident (grid built on the device, the
        named cameras' descriptors read where they are)."""
        self._m = matcher
        if handle is not None:           # device-built frame (orbm_frame_from_device)
            self._h = handle
            self.data = _Count(n_total, n_cams)
        elif resident is not None:
            self.data = data
            self._h = C.c_void_p()
            ptrs = (C.c_void_p * data.n_cams)(*[(p or None) for p in resident])
            check(_lib.lib().orbm_frame_create_resident(matcher._h, C.byref(data.c), ptrs, C.byref(self._h)))
        else:
            self.data = data
            self._h = C.c_void_p()
            check(_lib.lib().orbm_frame_create(matcher._h, C.byref(data.c), C.byref(self._h)))
        # orbm_frame_destroy hands the buffers back to the matcher's pool: the frame must go before its matcher does, also when the
        # last reference to it dies late (a failed test's traceback keeps it alive beyond the fixture that closes the matcher)
        children = getattr(matcher, "_frames", None)
        if children is not None:
            children.add(self)

    def download(self, kps=True, desc=True, uright=True, depth=True):
        """Host copies of the merged arrays of a device-built frame (global, cam-major order)."""
        n = max(self.data.n_total, 1)
        k = np.zeros(n, KP_DTYPE) if kps else None
        d = np.zeros((n, 32), np.uint8) if desc else None
        ur = np.zeros(n, np.float32) if uright else None
        dp = np.zeros(n, np.float32) if depth else None
        check(_lib.lib().orbm_frame_download(self._m._h, self._h, None if k is None else ptr(k), None if d is None else ptr(d),
                                             None if ur is None else ptr(ur), None if dp is None else ptr(dp)))
        nt = self.data.n_total
        return tuple(None if a is None else a[:nt] for a in (k, d, ur, dp))

    def close(self):
        if getattr(self, "_h", None):
            try:
                _lib.lib().orbm_frame_destroy(self._h)
            except Exception:
                pass
            self._h = None

    __del__ = close

    def grid(self):
        cs = np.zeros(self.data.n_cams * 64 * 48 + 1, np.int32); items = np.zeros(max(self.data.n_total, 1), np.int32)
        check(_lib.lib().orbm_frame_grid(self._h, ptr(cs), ptr(items)))
        return cs, items[:cs[-1]]


class Matcher:
    """ORBmatcher(nnratio=0.6, checkOri=True) (reference include/ORBmatcher.h:41)."""

    def __init__(self, nnratio=0.6, check_orientation=True, device=0):
        self.nnratio = float(nnratio); self.check_orientation = bool(check_orientation)
        self._h = C.c_void_p()
        self._frames = weakref.WeakSet()
        check(_lib.lib().orbm_create(device, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None):
            try:
                for f in list(getattr(self, "_frames", ())):      # frames first: their destroy reads the matcher
                    f.close()
            except Exception:  # interpreter teardown
                pass
            try:
                _lib.lib().orbm_destroy(self._h)
            except Exception:  # interpreter teardown
                pass
            self._h = None

    __del__ = close

    @property
    def stream(self):
        return _lib.lib().orbm_stream(self._h)

    DescriptorDistance = staticmethod(descriptor_distance)

    def hamming_top2(self, q, r):
        q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32); r = np.ascontiguousarray(r, np.uint8).reshape(-1, 32)
        bi = np.zeros(len(q), np.int32); bd = np.zeros(len(q), np.int32); sd = np.zeros(len(q), np.int32)
        check(_lib.lib().orbm_hamming_top2(self._h, ptr(q), len(q), ptr(r), len(r), ptr(bi), ptr(bd), ptr(sd)))
        return bi, bd, sd

    def hamming_matrix(self, q, r):
        q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32); r = np.ascontiguousarray(r, np.uint8).reshape(-1, 32)
        out = np.zeros((len(q), len(r)), np.uint16)
        check(_lib.lib().orbm_hamming_matrix(self._h, ptr(q), len(q), ptr(r), len(r), ptr(out)))
        return out

    # -- device-pointer entry points (asynchronous on `stream`)
    @staticmethod
    def top2_scratch_bytes(nq, nr):
        return int(_lib.lib().orbm_top2_scratch_bytes(nq, nr))

    @staticmethod
    def hamming_top2_device(d_q, nq, d_r, nr, d_best_idx, d_best_dist, d_second, d_scratch, stream):
        check(_lib.lib().orbm_hamming_top2_device(C.c_void_p(d_q), nq, C.c_void_p(d_r), nr, C.c_void_p(d_best_idx),
                                                  C.c_void_p(d_best_dist), C.c_void_p(d_second), C.c_void_p(d_scratch),
                                                  C.c_void_p(stream)))

    @staticmethod
    def use_matrix_cores(on):
        """orbm_use_matrix_cores: 1 / 0 = matrix-core / popcount form of the all-pairs kernels, -1 = default; returns the
        previous setting."""
        return int(_lib.lib().orbm_use_matrix_cores(int(on)))

    @staticmethod
    def use_fp4_top2(on):
        """orbm_use_fp4_top2: 1 / 0 = FP4 / int8 arithmetic in the matrix-core top-2 kernels, -1 = default; returns the previous
        setting."""
        return int(_lib.lib().orbm_use_fp4_top2(int(on)))

    @staticmethod
    def hamming_matrix_device(d_q, nq, d_r, nr, d_out, stream):
        check(_lib.lib().orbm_hamming_matrix_device(C.c_void_p(d_q), nq, C.c_void_p(d_r), nr, C.c_void_p(d_out),
                                                    C.c_void_p(stream)))

    def frame(self, data, resident=None):
        return Frame(self, data, resident=resident)

    def set_stream(self, stream):
        check(_lib.lib().orbm_set_stream(self._h, C.c_void_p(stream) if stream else None))

    def frame_from_device(self, cams, mbf, bounds):
        """Frame assembly on the device (merge + depth -> uRight + grid) from HBM-resident per-camera outputs.
        cams: [(d_kps, d_desc, n, d_depth or 0, depth_stride)]; bounds = (min_x, min_y, max_x, max_y)."""
        arr = (CamFeatures * len(cams))(*[CamFeatures(c[0], c[1], c[2], c[3] or None, c[4]) for c in cams])
        h = C.c_void_p()
        check(_lib.lib().orbm_frame_from_device(self._h, arr, len(cams), mbf, bounds[0], bounds[1], bounds[2], bounds[3],
                                                C.byref(h)))
        return Frame(self, handle=h, n_total=sum(c[2] for c in cams), n_cams=len(cams))

    def frame_from_device_counts(self, cams, d_counts, counts, mbf, bounds):
        """Inspection only (orbm_debug_frame_from_device_counts): the assembly as the front end enqueues it, the per-camera counts read on
        the device.  cams as for frame_from_device, their n being CAPACITIES; d_counts: device pointer to len(cams) + 1 ints (the
        counts, then a status word of 0); counts: the same numbers on the host (the returned Frame is sized by them)."""
        arr = (CamFeatures * len(cams))(*[CamFeatures(c[0], c[1], c[2], c[3] or None, c[4]) for c in cams])
        h = C.c_void_p()
        check(_lib.lib().orbm_debug_frame_from_device_counts(self._h, arr, len(cams), C.c_void_p(d_counts), mbf, bounds[0], bounds[1],
                                                             bounds[2], bounds[3], C.byref(h)))
        return Frame(self, handle=h, n_total=int(sum(counts)), n_cams=len(cams))

    def set_calibration(self, calib):
        """orbm_set_calibration: the undistortion device-built frames apply (fx, fy, cx, cy, k1, k2, p1, p2[, k3]); None or k1 == 0: off."""
        if calib is None:
            check(_lib.lib().orbm_set_calibration(self._h, None))
        else:
            c = _lib.Calibration(*([float(v) for v in calib] + [0.0] * (9 - len(calib))))
            check(_lib.lib().orbm_set_calibration(self._h, C.byref(c)))

    def cross_top2_blocks(self, block_ptrs, counts, first_query_block, n_query_blocks):
        """Cross-camera top-2 over HBM-resident descriptor blocks (one per camera of the whole rig)."""
        nb = len(block_ptrs)
        ptrs = (C.c_void_p * nb)(*block_ptrs)
        cnt = (C.c_int * nb)(*counts)
        nq = sum(counts[first_query_block:first_query_block + n_query_blocks])
        bi = np.zeros(max(nq, 1), np.int32); bd = np.zeros(max(nq, 1), np.int32); sd = np.zeros(max(nq, 1), np.int32)
        check(_lib.lib().orbm_cross_top2_blocks(self._h, ptrs, cnt, nb, first_query_block, n_query_blocks, ptr(bi), ptr(bd),
                                                ptr(sd)))
        return bi[:nq], bd[:nq], sd[:nq]

    def wait_for_stream(self, stream_handle):
        """Order this matcher's stream behind another HIP stream's work so far (orbm_wait_for_stream); no host wait."""
        check(_lib.lib().orbm_wait_for_stream(self._h, C.c_void_p(stream_handle)))

    def last_resolve(self):
        """(status, matches, sweeps, longest candidate list) of the last device resolve (orbm_debug_last_resolve)."""
        out = (C.c_int * 4)()
        check(_lib.lib().orbm_debug_last_resolve(self._h, out))
        return tuple(out)

    def last_resolve_form(self):
        """(form, capacity retries) of the last search: which resolve delivered its result, one of FORM_* (orbm_debug_last_resolve_form)."""
        out = (C.c_int * 2)()
        check(_lib.lib().orbm_debug_last_resolve_form(self._h, out))
        return tuple(out)

    def cross_top2_gathered(self, gathered_ptr, world, block_bytes, cap_rows, cams_per_rank, rank):
        """Cross-camera top-2 of this rank's features against the whole rig from ONE all-gathered buffer
        (orbm_cross_top2_gathered).  -> (best_idx, best_dist, second_dist, counts of every camera of the rig)."""
        key = (cap_rows, world * cams_per_rank)
        buf = getattr(self, "_gathered_buf", None)
        if buf is None or buf[0] != key:      # result buffers are reused from call to call (copied out below)
            buf = self._gathered_buf = (key, np.zeros(cap_rows, np.int32), np.zeros(cap_rows, np.int32), np.zeros(cap_rows, np.int32),
                                        np.zeros(world * cams_per_rank, np.int32))
        _, bi, bd, sd, cnt = buf
        nq = C.c_int()
        check(_lib.lib().orbm_cross_top2_gathered(self._h, C.c_void_p(gathered_ptr), world, block_bytes, cap_rows, cams_per_rank, rank,
                                                  ptr(bi), ptr(bd), ptr(sd), ptr(cnt), C.byref(nq)))
        return bi[:nq.value].copy(), bd[:nq.value].copy(), sd[:nq.value].copy(), cnt.tolist()

    def cross_top2_gathered_enqueue(self, gathered_ptr, world, block_bytes, cap_rows, cams_per_rank, rank, after_stream=None):
        """Enqueue half of cross_top2_gathered (side stream, joined into the main stream).  after_stream: raw handle of the
        stream the gathered buffer is produced on (0 = the default stream); None: no ordering needed."""
        self._gathered_shape = (cap_rows, world * cams_per_rank)
        check(_lib.lib().orbm_cross_top2_gathered_enqueue(self._h, C.c_void_p(gathered_ptr), world, block_bytes, cap_rows, cams_per_rank,
                                                          rank, C.c_void_p(after_stream or 0), 0 if after_stream is None else 1))

    def cross_top2_gathered_collect_views(self):
        """Collect half without copies: (best_idx, best_dist, second_dist) as views of the native pinned arrays + counts."""
        from .frontend import _view
        cap_rows, n_cams = self._gathered_shape
        cnt = np.zeros(n_cams, np.int32); nq = C.c_int()
        check(_lib.lib().orbm_cross_top2_gathered_collect(self._h, None, None, None, ptr(cnt), C.byref(nq)))
        p = [C.c_void_p() for _ in range(3)]
        check(_lib.lib().orbm_cross_top2_gathered_views(self._h, *[C.byref(x) for x in p]))
        n = nq.value
        return tuple(_view(x.value, np.int32, n) for x in p) + (cnt.tolist(),)

    def cross_top2_gathered_collect(self):
        """Collect half: after the handle's main stream has been synchronised (orbf_step_end)."""
        cap_rows, n_cams = self._gathered_shape
        bi = np.zeros(cap_rows, np.int32); bd = np.zeros(cap_rows, np.int32); sd = np.zeros(cap_rows, np.int32)
        cnt = np.zeros(n_cams, np.int32); nq = C.c_int()
        check(_lib.lib().orbm_cross_top2_gathered_collect(self._h, ptr(bi), ptr(bd), ptr(sd), ptr(cnt), C.byref(nq)))
        return bi[:nq.value], bd[:nq.value], sd[:nq.value], cnt.tolist()

    def cross_top2(self, frame):
        n = max(frame.data.n_total, 1)
        bi = np.zeros(n, np.int32); bd = np.zeros(n, np.int32); sd = np.zeros(n, np.int32)
        check(_lib.lib().orbm_cross_top2(self._h, frame._h, ptr(bi), ptr(bd), ptr(sd)))
        nt = frame.data.n_total
        return bi[:nt], bd[:nt], sd[:nt]

    def features_in_area(self, frame, cam, x, y, r, min_level=-1, max_level=-1):
        out = np.zeros(max(frame.data.n_total, 1), np.int32); n = C.c_int()
        check(_lib.lib().orbm_features_in_area(self._h, frame._h, cam, x, y, r, min_level, max_level, ptr(out), len(out),
                                               C.byref(n)))
        return out[:n.value].copy()

    def project_best(self, frame, queries, occupied=None, gate=0, inv_level_sigma2=None):
        """Nearest candidate of every projected point on its own (orbm_project_best: the inner loop of SearchBySim3 / Fuse).
        gate 0 none, 1 right-coordinate window, 2 Fuse's chi-square gate (needs inv_level_sigma2)."""
        queries = np.ascontiguousarray(queries, QUERY_DTYPE); nq = len(queries)
        bi, bd = np.zeros(max(nq, 1), np.int32), np.zeros(max(nq, 1), np.int32)
        occ = None if occupied is None else np.ascontiguousarray(occupied, np.uint8)
        sg = None if inv_level_sigma2 is None else np.ascontiguousarray(inv_level_sigma2, np.float32)
        check(_lib.lib().orbm_project_best(self._h, frame._h, ptr(queries), nq, None if occ is None else ptr(occ), gate,
                                           None if sg is None else ptr(sg), 0 if sg is None else len(sg), ptr(bi), ptr(bd)))
        return bi[:nq], bd[:nq]

    def time_project(self, frame, queries, th_high=TH_HIGH, iters=50):
        """(average launch duration of the projection kernel in microseconds, candidates that passed the gates):
        orbm_debug_time_project -- the kernel alone, as the frame search launches it (roofline M3)."""
        queries = np.ascontiguousarray(queries, QUERY_DTYPE)
        us = C.c_float(); n = C.c_longlong()
        check(_lib.lib().orbm_debug_time_project(self._h, frame._h, ptr(queries), len(queries), th_high, iters, C.byref(us), C.byref(n)))
        return us.value, n.value

    def project_candidates(self, frame, queries, cap):
        queries = np.ascontiguousarray(queries, QUERY_DTYPE); nq = len(queries)
        idx = np.zeros((max(nq, 1), cap), np.int32); dist = np.zeros((max(nq, 1), cap), np.uint16)
        cnt = np.zeros(max(nq, 1), np.int32)
        check(_lib.lib().orbm_project_candidates(self._h, frame._h, ptr(queries), nq, cap, ptr(idx), ptr(dist), ptr(cnt)))
        return idx[:nq], dist[:nq], cnt[:nq]

    def SearchByProjection(self, frame, queries, th_high=TH_HIGH, occupied=None):
        """SearchByProjection(CurrentFrame, LastFrame, th, bMono, Calib) from the projected queries on
        (reference src/ORBmatcher.cc:3448-3641).  Returns (nmatches, match_of_feature); match_of_feature[g] is the
        query index, -1 (untouched) or -2 (cleared by the rotation-histogram filter)."""
        queries = np.ascontiguousarray(queries, QUERY_DTYPE)
        m = np.zeros(max(frame.data.n_total, 1), np.int32); n = C.c_int()
        occ = None if occupied is None else np.ascontiguousarray(occupied, np.uint8)
        check(_lib.lib().orbm_search_by_projection(self._h, frame._h, ptr(queries), len(queries),
                                                   None if occ is None else ptr(occ), th_high,
                                                   int(self.check_orientation), ptr(m), C.byref(n)))
        return n.value, m[:frame.data.n_total]

    def SearchByProjectionWindows(self, frame, queries, windows2, th_high=TH_LOW, occupied=None):
        """Two-camera loop search (reference src/ORBmatcher.cc:566-750) from the projected windows on: queries[i] carries the
        camera-1 window, windows2[i] the camera-2 window (cam < 0: none); orbm_search_by_projection_windows."""
        from ._lib import WINDOW_DTYPE
        queries = np.ascontiguousarray(queries, QUERY_DTYPE); windows2 = np.ascontiguousarray(windows2, WINDOW_DTYPE)
        assert len(queries) == len(windows2)
        m = np.zeros(max(frame.data.n_total, 1), np.int32); n = C.c_int()
        occ = None if occupied is None else np.ascontiguousarray(occupied, np.uint8)
        check(_lib.lib().orbm_search_by_projection_windows(self._h, frame._h, ptr(queries), ptr(windows2), len(queries),
                                                           None if occ is None else ptr(occ), th_high, 0, ptr(m), C.byref(n)))
        return n.value, m[:frame.data.n_total]

    def SearchByProjectionPoints(self, frame, queries, occupied=None, th_high=TH_HIGH):
        """SearchByProjection(F, vpMapPoints, th) (reference src/ORBmatcher.cc:62-149)."""
        queries = np.ascontiguousarray(queries, QUERY_DTYPE)
        m = np.zeros(max(frame.data.n_total, 1), np.int32); n = C.c_int()
        occ = None if occupied is None else np.ascontiguousarray(occupied, np.uint8)
        check(_lib.lib().orbm_search_by_projection_points(self._h, frame._h, ptr(queries), len(queries),
                                                          None if occ is None else ptr(occ), self.nnratio, th_high,
                                                          ptr(m), C.byref(n)))
        return n.value, m[:frame.data.n_total]

    def RefreshPoints(self, batch):
        """MapPoint::ComputeDistinctiveDescriptors + MapPoint::UpdateNormalAndDepth (reference src/MapPoint.cc:325-438, :480-528)
        for every point of a RefreshBatch in one device call (orbm_refresh_points) -> REFRESH_DTYPE records."""
        out = np.zeros(max(batch.n_points, 1), REFRESH_DTYPE)
        check(_lib.lib().orbm_refresh_points(self._h, C.byref(batch.c), ptr(out)))
        return out[:batch.n_points]

    def PoseOptimization(self, problems):
        """Optimizer::PoseOptimization (reference src/Optimizer.cc:352-898) for a batch of PoseProblem in one device call, one workgroup
        per problem (orbm_pose_optimize) -> [(POSE_RESULT_DTYPE record, outlier flag per edge)] per problem."""
        recs, first, feat, pos, obs, octave = _pose_pack(problems)
        flags = np.zeros(max(int(first[-1]), 1), np.uint8); res = np.zeros(len(problems), POSE_RESULT_DTYPE)
        check(_lib.lib().orbm_pose_optimize(self._h, ptr(recs), len(problems), ptr(first), ptr(feat), ptr(pos), ptr(obs), ptr(octave),
                                            ptr(flags), ptr(res)))
        return _pose_unpack(problems, first, flags, res)

    def PoseOptimizationResident(self, problem, frame, points, point_of_feature):
        """The same for one problem whose observations are the resident frame's and whose positions are rows of a LocalPoints table
        (orbm_pose_optimize_resident); the edges of `problem` itself are not read.  point_of_feature[g] = a table row or -1
        -> (POSE_RESULT_DTYPE record, outlier flag per FEATURE)."""
        pof = np.ascontiguousarray(point_of_feature, np.int32)
        assert len(pof) >= frame.data.n_total
        flags = np.zeros(max(frame.data.n_total, 1), np.uint8); res = np.zeros(1, POSE_RESULT_DTYPE)
        check(_lib.lib().orbm_pose_optimize_resident(self._h, ptr(problem.rec), frame._h, points._h, ptr(pof), ptr(flags), ptr(res)))
        return res[0].copy(), flags[:frame.data.n_total]

    def Sim3Ransac(self, problems):
        """Every RANSAC hypothesis of a batch of Sim3Solvers in one call, two kernels back to back, one synchronisation
        (orbm_sim3_ransac) -> [(SIM3_HYP_DTYPE records H, mask words H x W uint64)] per problem."""
        args, its_first, hyp, masks = _sim3_pack(problems)
        check(_lib.lib().orbm_sim3_ransac(self._h, *args, ptr(hyp), ptr(masks)))
        return _sim3_unpack(problems, its_first, hyp, masks)

    def sim3_optimize(self, problems):
        """Optimizer::OptimizeSim3_cam1 (reference src/Optimizer.cc:1984-2243) for a batch of Sim3OptProblem in one device call, one
        workgroup per problem (orbm_sim3_optimize) -> [(SIM3OPT_RESULT_DTYPE record, flag per correspondence)] per problem."""
        recs, first, arrays, flags, res = _sim3opt_pack(problems)
        check(_lib.lib().orbm_sim3_optimize(self._h, ptr(recs), len(problems), ptr(first), *[ptr(a) for a in arrays], ptr(flags), ptr(res)))
        return _sim3opt_unpack(problems, first, flags, res)

    def local_ba(self, problem, stop=None):
        """Optimizer::LocalBundleAdjustment (reference src/Optimizer.cc:921-1353) from its graph on, on the device (orbm_local_ba): the
        Levenberg loop is driven from the host, one synchronisation per trial -> LocalBAResult.  stop: see local_ba_host."""
        res = LocalBAResult(problem); P = problem.native(); R = res.native()
        cb, keep = _lba_stop(stop)
        check(_lib.lib().orbm_local_ba(self._h, C.byref(P), cb, None, C.byref(R)))
        return res.take(R)

    def local_ba_host(self, problem, order=POSE_ORDER_INDEX, stop=None):
        """The same call through the host routine (orbm_local_ba_host); no device is used."""
        return local_ba_host(problem, order, stop)

    def last_local_ba(self):
        """What the last local_ba did: (path: 0 the device, 1 the host routine because a cap LBA_MAX_* is exceeded, 2 the host routine
        because no pose is free; kernel launches; stream synchronisations; polls of stop) (orbm_debug_last_local_ba)."""
        out = (C.c_int * 4)()
        check(_lib.lib().orbm_debug_last_local_ba(self._h, out))
        return tuple(out)

    def bundle_adjust(self, problem, iterations, robust, stop=None):
        """Optimizer::BundleAdjustment (reference src/Optimizer.cc:47-330) from its graph on, on the device (orbm_bundle_adjust): the
        local BA's kernels, the reduced system over the block pairs that exist, the blocked LDL^T across workgroups; one
        synchronisation per Levenberg trial -> GlobalBAResult."""
        res = GlobalBAResult(problem); P = problem.native(); R = res.native()
        cb, keep = _lba_stop(stop)
        check(_lib.lib().orbm_bundle_adjust(self._h, C.byref(P), int(iterations), 1 if robust else 0, cb, None, C.byref(R)))
        return res.take(R)

    def last_bundle_adjust(self):
        """What the last bundle_adjust did: (path: 0 the device, 1 the host routine because a cap BA_MAX_* is exceeded, 2 the host
        routine because no free pose is active; kernel launches; stream synchronisations; polls of stop; block pairs of the reduced
        system computed; block pairs possible; panels of the blocked LDL^T; 0) (orbm_debug_last_bundle_adjust)."""
        out = (C.c_int * 8)()
        check(_lib.lib().orbm_debug_last_bundle_adjust(self._h, out))
        return tuple(out)

    def essential_graph(self, problem, iterations=20):
        """Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:1373-1677) from its graph on, on the device
        (orbm_essential_graph): the Levenberg loop is driven from the host, one synchronisation per trial -> EssentialGraphResult."""
        res = EssentialGraphResult(problem); P = problem.native(); R = res.native()
        check(_lib.lib().orbm_essential_graph(self._h, C.byref(P), int(iterations), C.byref(R)))
        return res.take(R)

    def last_essential_graph(self):
        """What the last essential_graph did: (path: 0 the device, 1 the host routine because a cap EG_MAX_* is exceeded, 2 the host
        routine because no free vertex is active; kernel launches; stream synchronisations; 0; block pairs computed; block pairs
        possible; panels of the blocked LDL^T; 0) (orbm_debug_last_essential_graph)."""
        out = (C.c_int * 8)()
        check(_lib.lib().orbm_debug_last_essential_graph(self._h, out))
        return tuple(int(v) for v in out)

    def ba_ldlt_device(self, H, b):
        """The device solver of the reduced system alone (orbm_ba_ldlt_device) -> x, or None on a zero or non-finite pivot."""
        H = np.ascontiguousarray(H, np.float64); b = np.ascontiguousarray(b, np.float64); x = np.zeros(len(b))
        rc = _lib.lib().orbm_ba_ldlt_device(self._h, len(b), ptr(H), ptr(b), ptr(x))
        if rc < 0:
            check(rc)
        return x if rc == 1 else None

    def last_sim3opt(self):
        """Problems of the last sim3_optimize by path: (device, host routine because of more than SIM3OPT_CAP correspondences)
        (orbm_debug_last_sim3opt)."""
        out = (C.c_int * 2)()
        check(_lib.lib().orbm_debug_last_sim3opt(self._h, out))
        return tuple(out)

    def pnp_ransac(self, problems):
        """Every EPnP RANSAC hypothesis of a batch of PnPProblems and Refine() on every record, one enqueue and one synchronisation
        (orbm_pnp_ransac) -> per problem (hypothesis records, mask words H x W, refined records, their mask words)."""
        args, out = _pnp_pack(problems)
        check(_lib.lib().orbm_pnp_ransac(self._h, *args))
        return _pnp_unpack(problems, out)

    def last_pnp(self):
        """Where the work of the last pnp_ransac went: (problems on the device, problems through the host routine because of more than
        PNP_CAP correspondences, records refined on the device, records beyond PNP_MAX_RECORDS refined by the host routine)
        (orbm_debug_last_pnp)."""
        out = (C.c_int * 4)()
        check(_lib.lib().orbm_debug_last_pnp(self._h, out))
        return tuple(out)

    def pnp_buffers(self):
        """Capacities in bytes of the buffers pnp_ransac keeps between calls: (staged inputs, device block, mapped results)
        (orbm_debug_pnp_buffers)."""
        out = (C.c_ulonglong * 3)()
        check(_lib.lib().orbm_debug_pnp_buffers(self._h, out))
        return tuple(int(v) for v in out)

    def last_sim3(self):
        """Problems of the last Sim3Ransac by path: (device, host routine because of more than SIM3_CAP correspondences)
        (orbm_debug_last_sim3)."""
        out = (C.c_int * 2)()
        check(_lib.lib().orbm_debug_last_sim3(self._h, out))
        return tuple(out)

    def last_pose(self):
        """Problems of the last PoseOptimization[Resident] by path: (device, host routine because of more than POSE_CAP edges)
        (orbm_debug_last_pose)."""
        out = (C.c_int * 2)()
        check(_lib.lib().orbm_debug_last_pose(self._h, out))
        return tuple(out)

    def last_refresh(self):
        """Points of the last RefreshPoints by path: (16-lane groups, one wavefront, one workgroup, host routine because of more than
        REFRESH_CAP observations, no work) (orbm_debug_last_refresh)."""
        out = (C.c_int * 5)()
        check(_lib.lib().orbm_debug_last_refresh(self._h, out))
        return tuple(out)

    def last_local_map(self, resident_map):
        """What the last vote / point list on a ResidentMap did: (device path ran, observation records scanned, candidates, points
        kept) (orbm_debug_last_local_map)."""
        return resident_map.last_local_map()

    def SearchLocalPoints(self, frame, points, view, skip=None, occupied=None, th_high=TH_HIGH, n=None, want_track=True):
        """Tracking::SearchLocalPoints from its second loop on (reference src/Tracking.cc:1730-1768) over the first n rows
        (default: all written rows) of a LocalPoints table: Frame::isInFrustum, scale prediction and
        SearchByProjection(F, vpMapPoints, th) on the device.  -> (n_to_match, nmatches, match_of_feature, track);
        match_of_feature[g] indexes the table."""
        n = points.count if n is None else int(n)
        m = np.zeros(max(frame.data.n_total, 1), np.int32); nm = C.c_int(); nt = C.c_int()
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8)
        occ = None if occupied is None else np.ascontiguousarray(occupied, np.uint8)
        assert sk is None or len(sk) >= n
        assert occ is None or len(occ) >= frame.data.n_total
        track = np.zeros(max(n, 1), TRACK_DTYPE) if want_track else None
        check(_lib.lib().orbm_search_local_points(self._h, frame._h, points._h, n, C.byref(view.c), None if sk is None else ptr(sk),
                                                  None if occ is None else ptr(occ), self.nnratio, th_high,
                                                  None if track is None else ptr(track), ptr(m), C.byref(nt), C.byref(nm)))
        return nt.value, nm.value, m[:frame.data.n_total], (None if track is None else track[:max(n, 0)])
