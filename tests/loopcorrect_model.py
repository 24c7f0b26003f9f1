"""NumPy model of the two point passes of LoopClosing (reference src/LoopClosing.cc:678-722 and :953-989), written from the reference's
statements, Eigen's quaternion operations and Thirdparty/g2o/g2o/types/sim3.h -- not from the library, which it never calls.

A Sim3 is 8 doubles: the quaternion's coefficients x y z w (Eigen's order), the translation, the scale.  Every operation below is one
IEEE + - * / on float64 or float32 arrays; NumPy contracts nothing, so the bits are those of the C++ statements compiled without
contraction."""
import numpy as np

F32, F64 = np.float32, np.float64


def _cross(a, b):
    """Eigen's cross product, coefficient by coefficient; a, b (..., 3)."""
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def quat_rotate(q, v):
    """QuaternionBase::_transformVector: uv = vec.cross(v); uv += uv; v + w*uv + vec.cross(uv).  No normalisation."""
    q = np.asarray(q, F64); v = np.asarray(v, F64)
    vec, w = q[..., :3], q[..., 3:4]
    uv = _cross(vec, v)
    uv = uv + uv
    return v + w * uv + _cross(vec, uv)


def sim3_map(S, xyz):
    """Sim3::map: s*(r*xyz) + t  (sim3.h:144-146)."""
    S = np.asarray(S, F64)
    return S[..., 7:8] * quat_rotate(S[..., :4], xyz) + S[..., 4:7]


def sim3_inverse(S):
    """Sim3::inverse: Sim3(r.conjugate(), r.conjugate()*((-1./s)*t), 1./s)  (sim3.h:233-236)."""
    S = np.asarray(S, F64)
    conj = np.concatenate([-S[..., :3], S[..., 3:4]], axis=-1)
    t = quat_rotate(conj, (F64(-1.) / S[..., 7:8]) * S[..., 4:7])
    return np.concatenate([conj, t, F64(1.) / S[..., 7:8]], axis=-1)


def quat_to_matrix(q):
    """QuaternionBase::toRotationMatrix -> 3 x 3."""
    x, y, z, w = [F64(c) for c in q]
    tx, ty, tz = F64(2) * x, F64(2) * y, F64(2) * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[F64(1) - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, F64(1) - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, F64(1) - (txx + tyy)]], F64)


def corrected_pose(S):
    """:714-720: eigR = rotation().toRotationMatrix(); eigt = translation(); eigt *= (1./s); Converter::toCvSE3 -> float 4 x 4."""
    S = np.asarray(S, F64)
    T = np.zeros((4, 4), F32)
    T[:3, :3] = quat_to_matrix(S[:4]).astype(F32)
    T[:3, 3] = (S[4:7] * (F64(1.) / S[7])).astype(F32)
    T[3, 3] = F32(1)
    return T


def correct_sim3(kf_rows, kf_count, flags, pos, kfs, before, after, already=()):
    """CorrectLoop's loop over CorrectedSim3 (:678-722) with the keyframes and points as slots: kfs in the map's iteration order,
    before[j] = NonCorrectedSim3[kfs[j]], after[j] = CorrectedSim3[kfs[j]], already = the points whose mnCorrectedByKF is the current
    keyframe's id when the loop begins.  -> (entries (k, 2) int32: point slot and position j, pos_out (k, 3) float32, Tiw (n, 4, 4)
    float32, the new positions).  The claim is the reference's sequential loop; the arithmetic is applied to all kept points at once."""
    pos = np.array(pos, F32).reshape(-1, 3)
    before = np.asarray(before, F64).reshape(-1, 8); after = np.asarray(after, F64).reshape(-1, 8)
    corrected = np.zeros(len(flags), bool)             # mnCorrectedByKF == mpCurrentKF->mnId
    for a in already:
        if a >= 0:
            corrected[a] = True
    entries = []
    for j, kf in enumerate(kfs):
        for s in kf_rows[kf, :kf_count[kf]].tolist():  # vpMPsi
            if s < 0:                                  # !pMPi
                continue
            if flags[s] & 1:                           # isBad()
                continue
            if corrected[s]:
                continue
            entries.append((s, j))
            corrected[s] = True
    entries = np.array(entries, np.int32).reshape(-1, 2)
    slots, j = entries[:, 0], entries[:, 1]
    if len(entries):
        swi = sim3_inverse(after)                      # g2oCorrectedSwi = g2oCorrectedSiw.inverse()
        P = pos[slots].astype(F64)                     # Converter::toVector3d
        w = sim3_map(swi[j], sim3_map(before[j], P))   # g2oCorrectedSwi.map(g2oSiw.map(eigP3Dw))
        out = w.astype(F32)                            # Converter::toCvMat
        pos[slots] = out
    else:
        out = np.zeros((0, 3), F32)
    Tiw = np.stack([corrected_pose(S) for S in after]) if len(after) else np.zeros((0, 4, 4), F32)
    return entries, out, Tiw, pos


def gemm3(A, x, c):
    """cv::gemm(A, x, 1, c, 1) for a 3 x 3 by 3 x 1 product, the small path: products and sums in float left to right, then
    (float)(t*alpha + c*beta) in double.  A (..., 3, 3), x (..., 3), c (..., 3), all float32."""
    t = A[..., :, 0] * x[..., None, 0] + A[..., :, 1] * x[..., None, 1]
    t = t + A[..., :, 2] * x[..., None, 2]
    assert t.dtype == F32
    return (t.astype(F64) * F64(1.0) + c.astype(F64) * F64(1.0)).astype(F32)


def correct_rigid(pos, flags, ref_kf, slots, kf_corrected, Tcw_before, Twc_after, gba_slots=(), gba_pos=()):
    """Step 2 of the update after global BA (:953-989) with points and keyframes as slots: kf_corrected[r] says mnBAGlobalForKF ==
    nLoopKF of keyframe r, Tcw_before / Twc_after (n_kfs, 3, 4) are rows 0-2 of mTcwBefGBA and GetPoseInverse(), gba_slots / gba_pos the
    points with mnBAGlobalForKF == nLoopKF and their mPosGBA (a later entry replaces an earlier one).  slots None: every point.
    -> (status uint8: 0 untouched, 1 took mPosGBA, 2 moved through its reference keyframe; pos_out; the new positions)."""
    pos = np.array(pos, F32).reshape(-1, 3)
    n_kfs = len(kf_corrected)
    Tb = np.asarray(Tcw_before, F32).reshape(n_kfs, 3, 4); Ta = np.asarray(Twc_after, F32).reshape(n_kfs, 3, 4)
    gba_pos = np.asarray(gba_pos, F32).reshape(-1, 3)
    given = np.full(len(pos), -1, np.int64)
    for g, s in enumerate(gba_slots):
        if s >= 0:
            given[s] = g
    slots = np.arange(len(pos)) if slots is None else np.asarray(slots, np.int64)
    status = np.zeros(len(slots), np.uint8)
    good = (flags[slots] & 1) == 0                                    # !isBad()
    take = good & (given[slots] >= 0)                                 # mnBAGlobalForKF == nLoopKF: SetWorldPos(mPosGBA)
    r = ref_kf[slots].astype(np.int64)
    known = (r >= 0) & (r < n_kfs)
    ok = np.zeros(len(slots), bool)
    ok[known] = np.asarray(kf_corrected)[r[known]] != 0               # pRefKF->mnBAGlobalForKF == nLoopKF
    move = good & ~take & ok
    status[take] = 1; status[move] = 2
    pos[slots[take]] = gba_pos[given[slots[take]]]
    if move.any():
        rm = r[move]; P = pos[slots[move]]
        Xc = gemm3(Tb[rm][:, :, :3], P, Tb[rm][:, :, 3])               # Rcw*pMP->GetWorldPos()+tcw
        pos[slots[move]] = gemm3(Ta[rm][:, :, :3], Xc, Ta[rm][:, :, 3])   # Rwc*Xc+twc
    return status, pos[slots].copy(), pos
