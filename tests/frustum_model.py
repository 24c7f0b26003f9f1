"""Model of the local-map tracking front half in NumPy, every step in the number format the reference uses:
Frame::isInFrustum (reference src/Frame.cc:443-499), MapPoint::PredictScale (src/MapPoint.cc:602-617) and the query that
SearchByProjection(F, vpMapPoints, th) builds from the scratch fields (src/ORBmatcher.cc:62-157).  Written from those lines,
not from the kernel.  float32 arrays keep NumPy's arithmetic in float32 (one IEEE operation per ufunc call, no contraction);
every widening to double is spelled out.  The level uses the C library's logf through ctypes: NumPy's log is a different
implementation.

One deliberate deviation, shared with the library: a non-finite projection (PcZ == 0) is out of view.
"""
import ctypes
import ctypes.util
import numpy as np
from multi_orb_slam_amd._lib import QUERY_DTYPE, POINT_DTYPE, TRACK_DTYPE

f32, f64 = np.float32, np.float64
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype = ctypes.c_float
_libm.logf.argtypes = [ctypes.c_float]

# verdict of a point
IN_VIEW, BEHIND, OUTSIDE, TOO_NEAR, TOO_FAR, GRAZING, SKIPPED, NONFINITE = range(8)
REJECTIONS = (BEHIND, OUTSIDE, TOO_NEAR, TOO_FAR, GRAZING)


def logf(x):
    """std::log(float) of the host's C library, element by element."""
    x = np.asarray(x, f32)
    return np.array([_libm.logf(float(v)) for v in x.ravel()], f32).reshape(x.shape)


def predict_level(ratio, log_scale_factor, n_levels):
    """MapPoint::PredictScale from the ratio on: ceil(log(ratio) / mfLogScaleFactor) in float, clamped to [0, n_levels - 1].
    (A NaN or -inf quotient, whose int conversion the reference leaves undefined, gives level 0.)"""
    with np.errstate(all="ignore"):
        s = np.ceil(logf(ratio) / f32(log_scale_factor))
    lvl = np.zeros(s.shape, np.int32)
    pos = s > 0
    lvl[pos] = np.minimum(s[pos], f32(n_levels - 1)).astype(np.int32)
    return lvl


class View:
    """The Frame members isInFrustum reads, as float32."""

    def __init__(self, Rcw, tcw, Ow, fx, fy, cx, cy, mbf, bounds, scale_factors, log_scale_factor, th, viewing_cos_limit=0.5):
        self.Rcw = np.asarray(Rcw, f32).reshape(3, 3); self.tcw = np.asarray(tcw, f32).reshape(3); self.Ow = np.asarray(Ow, f32).reshape(3)
        self.fx, self.fy, self.cx, self.cy, self.mbf = f32(fx), f32(fy), f32(cx), f32(cy), f32(mbf)
        self.min_x, self.min_y, self.max_x, self.max_y = (f32(b) for b in bounds)   # (min_x, min_y, max_x, max_y)
        self.scale_factors = np.asarray(scale_factors, f32); self.n_levels = len(self.scale_factors)
        self.log_scale_factor = f32(log_scale_factor); self.th = f32(th); self.viewing_cos_limit = f32(viewing_cos_limit)

    def native(self):
        import multi_orb_slam_amd as m
        return m.View(self.Rcw, self.tcw, self.Ow, self.fx, self.fy, self.cx, self.cy, self.mbf,
                      (self.min_x, self.min_y, self.max_x, self.max_y), self.scale_factors, self.log_scale_factor, float(self.th),
                      float(self.viewing_cos_limit))


def camera_centre(Rcw, tcw):
    """Frame::UpdatePoseMatrices: mOw = -mRcw.t()*mtcw.  The unary minus binds to the transpose: OpenCV evaluates the transposed
    matrix, carries the -1 as the weight of the product, and calls cv::gemm(Rt, t, alpha = -1) WITHOUT a transposition flag -- the
    small path: products and sums in float, left to right, then (float)(t * -1.0 + 0.0f * 0.0) in double
    (host/cv_compat.h: expr_neg, expr_matmul, gemm_small_elem)."""
    R = np.asarray(Rcw, f32).reshape(3, 3); t = np.asarray(tcw, f32).reshape(3)
    out = np.zeros(3, f32)
    for i in range(3):
        s = f32(f32(R[0, i] * t[0]) + f32(R[1, i] * t[1]))
        s = f32(s + f32(R[2, i] * t[2]))
        out[i] = f32(f64(s) * f64(-1.0) + f64(f32(0.0)) * f64(0.0))
    return out


def frustum(points, view, skip=None):
    """-> (verdict[n], track[n] (TRACK_DTYPE), queries (QUERY_DTYPE, the in-view points in table order), keep (their rows))."""
    P = np.ascontiguousarray(points["pos"], f32).reshape(-1, 3); Pn = np.ascontiguousarray(points["normal"], f32).reshape(-1, 3)
    n = len(P)
    V = view
    verdict = np.full(n, -1, np.int32)
    if skip is not None:
        verdict[np.asarray(skip[:n]) != 0] = SKIPPED

    def settle(mask, what):
        verdict[(verdict < 0) & mask] = what

    with np.errstate(all="ignore"):
        # Pc = mRcw*P + mtcw: ONE cv::gemm, small path: float products and sums left to right, then (float)(t*1.0 + c*1.0) in double
        Pc = np.zeros((n, 3), f32)
        for k in range(3):
            t = V.Rcw[k, 0] * P[:, 0] + V.Rcw[k, 1] * P[:, 1]
            t = t + V.Rcw[k, 2] * P[:, 2]
            Pc[:, k] = (t.astype(f64) * f64(1.0) + f64(V.tcw[k]) * f64(1.0)).astype(f32)
        settle(Pc[:, 2] < f32(0.0), BEHIND)
        invz = f32(1.0) / Pc[:, 2]
        u = V.fx * Pc[:, 0] * invz + V.cx
        v = V.fy * Pc[:, 1] * invz + V.cy
        settle(~(np.isfinite(u) & np.isfinite(v)), NONFINITE)
        settle((u < V.min_x) | (u > V.max_x), OUTSIDE)
        settle((v < V.min_y) | (v > V.max_y), OUTSIDE)
        max_d = f32(1.2) * np.asarray(points["max_dist"], f32)      # GetMaxDistanceInvariance
        min_d = f32(0.8) * np.asarray(points["min_dist"], f32)      # GetMinDistanceInvariance
        PO = P - V.Ow[None, :]                                      # float
        PO64 = PO.astype(f64)
        s = f64(0) + PO64[:, 0] * PO64[:, 0]
        s = s + PO64[:, 1] * PO64[:, 1]
        s = s + PO64[:, 2] * PO64[:, 2]
        dist = np.sqrt(s).astype(f32)                               # const float dist = cv::norm(PO)
        settle(dist < min_d, TOO_NEAR)
        settle(dist > max_d, TOO_FAR)
        Pn64 = Pn.astype(f64)
        d = f64(0) + PO64[:, 0] * Pn64[:, 0]
        d = d + PO64[:, 1] * Pn64[:, 1]
        d = d + PO64[:, 2] * Pn64[:, 2]
        view_cos = (d / dist.astype(f64)).astype(f32)               # PO.dot(Pn) / dist: double / float
        settle(view_cos < V.viewing_cos_limit, GRAZING)
        settle(np.ones(n, bool), IN_VIEW)
        keep = np.nonzero(verdict == IN_VIEW)[0]
        ratio = np.asarray(points["max_dist"], f32)[keep] / dist[keep]
        level = predict_level(ratio, V.log_scale_factor, V.n_levels)
        proj_xr = u - V.mbf * invz
        # SearchByProjection: r = RadiusByViewingCos (the literal 0.998 is a double), r *= th unless th == 1.0
        r = np.where(view_cos[keep].astype(f64) > 0.998, f32(2.5), f32(4.0)).astype(f32)
        if f64(V.th) != 1.0:
            r = r * V.th
        radius = r * V.scale_factors[level]

    track = np.zeros(n, TRACK_DTYPE)
    track["in_view"][keep] = 1
    track["proj_x"][keep] = u[keep]; track["proj_y"][keep] = v[keep]; track["proj_xr"][keep] = proj_xr[keep]
    track["view_cos"][keep] = view_cos[keep]; track["level"][keep] = level
    q = np.zeros(len(keep), QUERY_DTYPE)
    q["u"] = u[keep]; q["v"] = v[keep]; q["radius"] = radius; q["ur"] = proj_xr[keep]
    q["min_level"] = level - 1; q["max_level"] = level; q["cam"] = 0
    q["blocks"] = (np.asarray(points["blocks"])[keep] != 0).astype(np.int32); q["angle"] = 0
    q["desc"] = np.asarray(points["desc"])[keep]
    return verdict, track, q, keep


def expected_search(oracle_frame, points, view, skip, occupied, nnratio, th_high):
    """The whole call under the model and the oracle: (n_to_match, nmatches, match_of_feature in TABLE indices, track, verdict)."""
    import oracle
    verdict, track, q, keep = frustum(points, view, skip)
    n_total = len(oracle_frame.un_x)
    if len(q):
        cnt, mo = oracle.search_by_projection_points(oracle_frame, q, occupied, nnratio, th_high)
        mo = np.asarray(mo, np.int32).copy()
        hit = mo >= 0
        mo[hit] = keep[mo[hit]].astype(np.int32)
    else:
        cnt, mo = 0, np.full(n_total, -1, np.int32)
    return len(keep), int(cnt), mo, track, verdict


def make_points(n):
    return np.zeros(n, POINT_DTYPE)
