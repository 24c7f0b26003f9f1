"""NumPy model of the pair loop of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:398-669) and of
KeyFrame::UnprojectStereo (src/KeyFrame.cc:985-1012), written from the reference's statements and OpenCV's semantics (2.4.x / 3.2) with
scalar np.float32 / np.float64 arithmetic, one NumPy operation per machine operation.  Every helper below stands for one OpenCV call:

  mat_mul_3x1     cv::gemm, the small path a 3x3 * 3x1 takes: float products, float sums left to right, then (float)(t*alpha + c*beta)
  row_dot         cv::Mat::dot: double products, double running sum
  l2_norm         cv::norm: squares summed in double, sqrt in double
  scaled_minus    `s*M.row(2) - M.row(q)`: cv::subtract for s == 1, else cv::addWeighted with float weights a*s + b*(-1) + 0
  divided_by      `M / w`: weight 1./w in double; cv::add(M, 0) for 1, cv::subtract(0, M) for -1, else convertTo: x*(float)weight + 0
  jacobi_vt       cv::SVD::compute(MODIFY_A | FULL_UV) of a 4x4 float matrix: JacobiSVDImpl_<float>, with the C library's hypot replaced
                  by sqrt(p*p + beta*beta) in double (the project's stated replacement: no libm call may run in the kernel)

cos(2*atan2(mb/2, depth)) is an input (one value per feature), as it is for the library.  A NaN coordinate is reported with the bit
pattern 0xffc00000, the library's convention."""
import numpy as np

f32, f64 = np.float32, np.float64
NONE, ACCEPTED, CAM_OFF, LOW_PARALLAX, W_ZERO, Z1, Z2, REPROJ1, REPROJ2, ZERO_DIST, SCALE = range(11)
OUTCOME_NAMES = ("none", "accepted", "camera off", "low parallax", "w == 0", "z1 <= 0", "z2 <= 0", "reprojection 1", "reprojection 2",
                 "zero distance", "scale")
PATH_NONE, PATH_SVD, PATH_UNPROJECT1, PATH_UNPROJECT2 = range(4)
PATH_NAMES = ("none", "svd", "unproject 1", "unproject 2")
RECORD = np.dtype([("x3D", np.float32, 3), ("outcome", np.int32), ("path", np.int32)])
FLT_EPSILON = f32(2.0 ** -23)


def mat_mul_3x1(M, x, c=None):
    """M (3 rows of 3 float32) times x, plus c when given."""
    out = []
    for i in range(3):
        t = M[i][0] * x[0] + M[i][1] * x[1]
        t = t + M[i][2] * x[2]
        if c is None:
            d = f64(t) * f64(1.0) + f64(f32(0.0)) * f64(0.0)
        else:
            d = f64(t) * f64(1.0) + f64(c[i]) * f64(1.0)
        out.append(f32(d))
    return out


def row_dot(a, b):
    s = f64(0.0)
    for k in range(len(a)):
        s = s + f64(a[k]) * f64(b[k])
    return s


def l2_norm(a):
    s = f64(0.0)
    for v in a:
        s = s + f64(v) * f64(v)
    return np.sqrt(s)


def scaled_minus(s, row_a, row_b):
    if f64(s) == 1.0:
        return [a - b for a, b in zip(row_a, row_b)]
    al, be = f32(f64(s)), f32(-1.0)
    return [a * al + b * be + f32(0.0) for a, b in zip(row_a, row_b)]


def divided_by(v, w):
    weight = f64(1.0) / f64(w)
    if weight == 1.0:
        return [x + f32(0.0) for x in v]
    if weight == -1.0:
        return [f32(0.0) - x for x in v]
    sc = f32(weight)
    return [x * sc + f32(0.0) for x in v]


def hypot_replacement(a, b):
    return np.sqrt(a * a + b * b)


def jacobi_vt(A):
    """Vt (4 rows of 4 float32) of the 4x4 float32 matrix A (list of rows), rows ordered by descending singular value."""
    n = 4
    At = [[f32(A[k][i]) for k in range(n)] for i in range(n)]          # transpose(src, temp_a)
    Vt = [[f32(1.0) if i == k else f32(0.0) for k in range(n)] for i in range(n)]
    W = []
    for i in range(n):
        sd = f64(0.0)
        for k in range(n):
            sd = sd + f64(At[i][k]) * f64(At[i][k])
        W.append(sd)
    eps = f32(FLT_EPSILON * f32(2.0))
    for _ in range(30):                                                # max_iter = max(m, 30)
        changed = False
        for i in range(n - 1):
            for j in range(i + 1, n):
                a, b, p = W[i], W[j], f64(0.0)
                for k in range(n):
                    p = p + f64(At[i][k]) * f64(At[j][k])
                if abs(p) <= f64(eps) * np.sqrt(a * b):
                    continue
                p = p * f64(2.0)
                beta = a - b
                gamma = hypot_replacement(p, beta)
                if beta < 0:
                    delta = (gamma - beta) * f64(0.5)
                    s = f32(np.sqrt(delta / gamma))
                    c = f32(p / (gamma * f64(s) * f64(2.0)))
                else:
                    c = f32(np.sqrt((gamma + beta) / (gamma * f64(2.0))))
                    s = f32(p / (gamma * f64(c) * f64(2.0)))
                a = b = f64(0.0)
                for k in range(n):
                    t0 = c * At[i][k] + s * At[j][k]
                    t1 = (-s) * At[i][k] + c * At[j][k]
                    At[i][k], At[j][k] = t0, t1
                    a = a + f64(t0) * f64(t0)
                    b = b + f64(t1) * f64(t1)
                W[i], W[j] = a, b
                changed = True
                for k in range(n):
                    t0 = c * Vt[i][k] + s * Vt[j][k]
                    t1 = (-s) * Vt[i][k] + c * Vt[j][k]
                    Vt[i][k], Vt[j][k] = t0, t1
        if not changed:
            break
    for i in range(n):
        sd = f64(0.0)
        for k in range(n):
            sd = sd + f64(At[i][k]) * f64(At[i][k])
        W[i] = np.sqrt(sd)
    for i in range(n - 1):
        j = i
        for k in range(i + 1, n):
            if W[j] < W[k]:
                j = k
        if i != j:
            W[i], W[j] = W[j], W[i]
            At[i], At[j] = At[j], At[i]
            Vt[i], Vt[j] = Vt[j], Vt[i]
    return Vt


def rows_of(M34):
    """A (3, 4) float32 array as the rotation rows and the translation: ([R row 0, 1, 2], t)."""
    return [[f32(M34[r, c]) for c in range(3)] for r in range(3)], [f32(M34[r, 3]) for r in range(3)]


def unproject_stereo(kf, i):
    """KeyFrame::UnprojectStereo(i) for z > 0."""
    z = f32(kf.depth[i])
    u, v = f32(kf.xd[i]), f32(kf.yd[i])
    x = (u - kf.cx) * z * kf.invfx
    y = (v - kf.cy) * z * kf.invfy
    x3Dc = [x, y, z]
    Rwc, twc = rows_of(kf.Twc)
    if 0 <= i < kf.n_cam1:
        return mat_mul_3x1(Rwc, x3Dc, twc)
    R12 = [[f32(kf.Rcam12[r, c]) for c in range(3)] for r in range(3)]
    inner = mat_mul_3x1(R12, x3Dc, [f32(t) for t in kf.tcam12])
    return mat_mul_3x1(Rwc, inner, twc)


def system_matrix(kf1, kf2, idx1, idx2):
    """xn1, xn2 and the 4x4 A of the linear triangulation (:424-425, :472-484)."""
    cam = int(kf1.cam_of[idx1])
    xn1 = [(f32(kf1.x[idx1]) - kf1.cx) * kf1.invfx, (f32(kf1.y[idx1]) - kf1.cy) * kf1.invfy, f32(1.0)]
    xn2 = [(f32(kf2.x[idx2]) - kf2.cx) * kf2.invfx, (f32(kf2.y[idx2]) - kf2.cy) * kf2.invfy, f32(1.0)]
    T1 = [[f32(v) for v in kf1.Tcw[cam][r]] for r in range(3)]
    T2 = [[f32(v) for v in kf2.Tcw[cam][r]] for r in range(3)]
    A = [scaled_minus(xn1[0], T1[2], T1[0]), scaled_minus(xn1[1], T1[2], T1[1]),
         scaled_minus(xn2[0], T2[2], T2[0]), scaled_minus(xn2[1], T2[2], T2[1])]
    return xn1, xn2, A


def reprojection_rejects(kf, idx, R, t, x3D, z, mbf_current, rules=(), trace=None, which=1):
    exceeds = (lambda a, b: a >= b) if "reproj_ge" in rules else (lambda a, b: a > b)
    stereo_gate = f64(7.815) if "stereo_7.815" in rules else f64(7.8)
    sigma_square = f32(kf.level_sigma2[int(kf.octave[idx])])
    x = f32(row_dot(R[0], x3D) + f64(t[0]))
    y = f32(row_dot(R[1], x3D) + f64(t[1]))
    invz = f32(f64(1.0) / f64(z))
    kx, ky, ur = f32(kf.x[idx]), f32(kf.y[idx]), f32(kf.uright[idx])
    if not ur >= 0:
        u = kf.fx * x * invz + kf.cx
        v = kf.fy * y * invz + kf.cy
        ex, ey = u - kx, v - ky
        if trace is not None:
            trace["err%d" % which], trace["gate%d" % which] = f64(ex * ex + ey * ey), f64(5.991) * f64(sigma_square)
        return bool(exceeds(f64(ex * ex + ey * ey), f64(5.991) * f64(sigma_square)))
    u = kf.fx * x * invz + kf.cx
    u_r = u - mbf_current * invz
    v = kf.fy * y * invz + kf.cy
    ex, ey, er = u - kx, v - ky, u_r - ur
    if trace is not None:
        trace["err%d" % which], trace["gate%d" % which] = f64(ex * ex + ey * ey + er * er), f64(7.8) * f64(sigma_square)
    return bool(exceeds(f64(ex * ex + ey * ey + er * er), stereo_gate * f64(sigma_square)))


RULES = ("reproj_ge", "stereo_7.815", "float_0.9998", "depth_lt", "scale_le")


def one_pair(kf1, kf2, cam_enabled, idx1, idx2, ratio_factor, rules=(), trace=None):
    """-> (x3D or None, outcome, path).  `rules`: names of deliberately WRONG rules (RULES; tests/test_geometry_boundary_worlds.py shows
    that the boundary worlds catch each of them): ">=" for ">" in the reprojection gates, 7.815 for the stage's 7.8, the float
    constant 0.9998f for the double one, "<" for "<=" on the depth signs, "<=" for "<" in the first scale gate.  `trace`: a dict that
    receives the intermediates the boundary worlds are built from.  With neither, the function is what it was."""
    assert all(r in RULES for r in rules), rules
    tr = trace if trace is not None else {}
    behind = (lambda z: z < 0) if "depth_lt" in rules else (lambda z: z <= 0)
    stereo1, stereo2 = bool(kf1.uright[idx1] >= 0), bool(kf2.uright[idx2] >= 0)
    cam = int(kf1.cam_of[idx1])
    if not cam_enabled[cam]:
        return None, CAM_OFF, PATH_NONE
    xn1, xn2, A = system_matrix(kf1, kf2, idx1, idx2)
    # Rwc1 = Rcw1.t(), Rwc2 = Rcw2.t(): the FIRST camera's rotations whatever the pair's camera
    Rcw1, _ = rows_of(kf1.Tcw[0]); Rcw2, _ = rows_of(kf2.Tcw[0])
    Rwc1 = [[Rcw1[c][r] for c in range(3)] for r in range(3)]
    Rwc2 = [[Rcw2[c][r] for c in range(3)] for r in range(3)]
    ray1, ray2 = mat_mul_3x1(Rwc1, xn1), mat_mul_3x1(Rwc2, xn2)
    cos_rays = f32(row_dot(ray1, ray2) / (l2_norm(ray1) * l2_norm(ray2)))
    cos_stereo = cos_rays + f32(1.0)
    cos_stereo1 = cos_stereo2 = cos_stereo
    if stereo1:
        cos_stereo1 = f32(kf1.cos_stereo[idx1])
    elif stereo2:
        cos_stereo2 = f32(kf2.cos_stereo[idx2])
    cos_stereo = cos_stereo2 if cos_stereo2 < cos_stereo1 else cos_stereo1
    tr.update(cam=cam, stereo1=stereo1, stereo2=stereo2, cos_rays=cos_rays, cos_stereo1=cos_stereo1, cos_stereo2=cos_stereo2)
    limit = f64(f32(0.9998)) if "float_0.9998" in rules else f64(0.9998)

    if cos_rays < cos_stereo and cos_rays > 0 and (stereo1 or stereo2 or f64(cos_rays) < limit):
        vt3 = jacobi_vt(A)[3]
        path = PATH_SVD
        if vt3[3] == 0:
            return vt3[:3], W_ZERO, path
        x3D = divided_by(vt3[:3], vt3[3])
    elif stereo1 and cos_stereo1 < cos_stereo2:
        x3D, path = unproject_stereo(kf1, idx1), PATH_UNPROJECT1
    elif stereo2 and cos_stereo2 < cos_stereo1:
        x3D, path = unproject_stereo(kf2, idx2), PATH_UNPROJECT2
    else:
        return None, LOW_PARALLAX, PATH_NONE

    R1, t1 = rows_of(kf1.Tcw[cam]); R2, t2 = rows_of(kf2.Tcw[cam])
    z1 = f32(row_dot(R1[2], x3D) + f64(t1[2]))
    tr.update(x3D=list(x3D), z1=z1)
    if behind(z1):
        return x3D, Z1, path
    z2 = f32(row_dot(R2[2], x3D) + f64(t2[2]))
    tr.update(z2=z2)
    if behind(z2):
        return x3D, Z2, path
    if reprojection_rejects(kf1, idx1, R1, t1, x3D, z1, kf1.mbf, rules, tr, 1):
        return x3D, REPROJ1, path
    if reprojection_rejects(kf2, idx2, R2, t2, x3D, z2, kf1.mbf, rules, tr, 2):
        return x3D, REPROJ2, path
    normal1 = [x3D[k] - f32(kf1.centre[cam][k]) for k in range(3)]
    normal2 = [x3D[k] - f32(kf2.centre[cam][k]) for k in range(3)]
    dist1, dist2 = f32(l2_norm(normal1)), f32(l2_norm(normal2))
    if dist1 == 0 or dist2 == 0:
        return x3D, ZERO_DIST, path
    ratio_dist = dist2 / dist1
    ratio_octave = f32(kf1.scale_factors[int(kf1.octave[idx1])]) / f32(kf2.scale_factors[int(kf2.octave[idx2])])
    rf = f32(ratio_factor)
    tr.update(dist1=dist1, dist2=dist2, ratio_dist=ratio_dist, ratio_octave=ratio_octave, low=ratio_dist * rf, high=ratio_octave * rf)
    too_near = ratio_dist * rf <= ratio_octave if "scale_le" in rules else ratio_dist * rf < ratio_octave
    if too_near or ratio_dist > ratio_octave * rf:
        return x3D, SCALE, path
    return x3D, ACCEPTED, path


def triangulate(kf1, kf2, cam_enabled, pairs, ratio_factor, rules=(), traces=None):
    """Records (RECORD) of the pairs; kf1 / kf2: triangulate_worlds.KF.  rules: see one_pair; traces: a list that receives one dict of
    intermediates per pair."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    rec = np.zeros(len(pairs), RECORD)
    with np.errstate(all="ignore"):
        for p, (i1, i2) in enumerate(pairs):
            tr = {} if traces is not None else None
            x3D, outcome, path = one_pair(kf1, kf2, cam_enabled, int(i1), int(i2), ratio_factor, rules, tr)
            if traces is not None:
                traces.append(tr)
            rec["outcome"][p], rec["path"][p] = outcome, path
            if x3D is not None:
                rec["x3D"][p] = np.array(x3D, np.float32)
    bits = rec["x3D"].view(np.uint32)
    bits[np.isnan(rec["x3D"])] = 0xffc00000
    return rec
