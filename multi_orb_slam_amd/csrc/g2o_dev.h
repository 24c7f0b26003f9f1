// g2o_dev.h -- the Eigen / g2o boundary: the parts of Eigen and g2o that the reference's optimisers run and this library restates, ONE
// definition each, for the kernels and the host routines (pose.hip, sim3opt.hip, lba.hip, essgraph.hip).  Restated from the published sources (Eigen's
// Geometry, Cholesky and LU modules; Thirdparty/g2o/g2o/types/se3quat.h, types/sim3.h, types/types_six_dof_expmap.cpp as far as its edges
// share their Jacobian, core/robust_kernel_impl.cpp with the deltas the reference sets) and UNPINNED: Eigen is not linked and g2o was never
// compiled against this code, so each is ONE function that a later pin changes.  The library is built without
// contraction and without fast-math, and the tests compare bytes: nothing inside these bodies is to be reordered.
#pragma once
#include <cfloat>
#include <cmath>
#include <hip/hip_runtime.h>
#include "../../include/orbm.h"
#include "cv_dev.h"   // x86_nan
#include "sincos_dev.h"

struct SE3Quat { double q[4], t[3]; };   // g2o::SE3Quat: quaternion in Eigen's coefficient order x y z w, translation

// ---- Eigen ----------------------------------------------------------------------------------------------------------------------------
// Quaternion<double>(Matrix3d) (Geometry/Quaternion.h, quaternionbase_assign_impl<Other,3,3>)
__host__ __device__ inline void eigen_quat_from_matrix(const double* m, double* q) {
    double t = m[0] + m[4] + m[8];
    if (t > 0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[7] - m[5]) * t;
        q[1] = (m[2] - m[6]) * t;
        q[2] = (m[3] - m[1]) * t;
    } else if (!(m[4] > m[0]) && !(m[8] > m[0])) {        // i = 0, j = 1, k = 2
        t = sqrt(m[0] - m[4] - m[8] + 1.0);
        q[0] = 0.5 * t; t = 0.5 / t;
        q[3] = (m[7] - m[5]) * t; q[1] = (m[3] + m[1]) * t; q[2] = (m[6] + m[2]) * t;
    } else if (m[4] > m[0] && !(m[8] > m[4])) {           // i = 1, j = 2, k = 0
        t = sqrt(m[4] - m[8] - m[0] + 1.0);
        q[1] = 0.5 * t; t = 0.5 / t;
        q[3] = (m[2] - m[6]) * t; q[2] = (m[7] + m[5]) * t; q[0] = (m[1] + m[3]) * t;
    } else {                                              // i = 2, j = 0, k = 1
        t = sqrt(m[8] - m[0] - m[4] + 1.0);
        q[2] = 0.5 * t; t = 0.5 / t;
        q[3] = (m[3] - m[1]) * t; q[0] = (m[2] + m[6]) * t; q[1] = (m[5] + m[7]) * t;
    }
}
// QuaternionBase::normalize: coeffs /= sqrt(squaredNorm), the squares summed in coefficient order
__host__ __device__ inline void eigen_quat_normalize(double* q) {
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    q[0] = q[0] / n; q[1] = q[1] / n; q[2] = q[2] / n; q[3] = q[3] / n;
}
// QuaternionBase::_transformVector: uv = vec x v; uv += uv; v + w*uv + vec x uv
__host__ __device__ inline void eigen_quat_rotate(const double* q, const double* v, double* out) {
    double uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
    uv[0] = uv[0] + uv[0]; uv[1] = uv[1] + uv[1]; uv[2] = uv[2] + uv[2];
    const double c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
    out[0] = v[0] + q[3] * uv[0] + c[0];
    out[1] = v[1] + q[3] * uv[1] + c[1];
    out[2] = v[2] + q[3] * uv[2] + c[2];
}
// quat_product<Architecture::Generic>
__host__ __device__ inline void eigen_quat_mul(const double* a, const double* b, double* r) {
    const double w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    const double x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    const double y = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    const double z = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
    r[0] = x; r[1] = y; r[2] = z; r[3] = w;
}
// QuaternionBase::toRotationMatrix
__host__ __device__ inline void eigen_quat_to_matrix(const double* q, double* m) {
    const double tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
    const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    m[0] = 1 - (tyy + tzz); m[1] = txy - twz; m[2] = txz + twy;
    m[3] = txy + twz; m[4] = 1 - (txx + tzz); m[5] = tyz - twx;
    m[6] = txz - twy; m[7] = tyz + twx; m[8] = 1 - (txx + tyy);
}
// LDLT<MatrixXd>::compute (ldlt_inplace<Lower>::unblocked: the pivot is the FIRST largest |diagonal| of the remaining block) followed
// by isPositive() and solve() (P, L, D with the 1/highest() tolerance, L^T, P^T); every inner product sequential in ascending index.
// A: NxN row-major (N = 6: the pose vertex, 7: the Sim3 vertex), destroyed (only its lower triangle is read).  Returns isPositive(); x is
// written only then, as g2o does.
template <int N = 6>
__host__ __device__ inline bool eigen_ldlt_solve(double* A, const double* b, double* x, double* temp, int* transp) {
    int sign = 0;   // 0 ZeroSign, 1 PositiveSemiDef, -1 NegativeSemiDef, 2 Indefinite
    bool done = false;
    for (int k = 0; k < N && !done; ++k) {
        int idx = k;
        double big = fabs(A[(N + 1) * k]);
        for (int i = k + 1; i < N; ++i) { const double v = fabs(A[(N + 1) * i]); if (v > big) { big = v; idx = i; } }
        transp[k] = idx;
        if (k != idx) {
            for (int j = 0; j < k; ++j) { const double t = A[N * k + j]; A[N * k + j] = A[N * idx + j]; A[N * idx + j] = t; }
            for (int i = idx + 1; i < N; ++i) { const double t = A[N * i + k]; A[N * i + k] = A[N * i + idx]; A[N * i + idx] = t; }
            { const double t = A[(N + 1) * k]; A[(N + 1) * k] = A[(N + 1) * idx]; A[(N + 1) * idx] = t; }
            for (int i = k + 1; i < idx; ++i) { const double t = A[N * i + k]; A[N * i + k] = A[N * idx + i]; A[N * idx + i] = t; }
        }
        if (k > 0) {
            for (int j = 0; j < k; ++j) temp[j] = A[(N + 1) * j] * A[N * k + j];
            double s = 0;
            for (int j = 0; j < k; ++j) s += A[N * k + j] * temp[j];
            A[(N + 1) * k] -= s;
            for (int i = k + 1; i < N; ++i) {
                double r = 0;
                for (int j = 0; j < k; ++j) r += A[N * i + j] * temp[j];
                A[N * i + k] -= r;
            }
        }
        const double akk = A[(N + 1) * k];
        const bool valid = fabs(akk) > 0;
        if (k == 0 && !valid) {
            for (int j = 0; j < N; ++j) transp[j] = j;
            done = true;
        } else {
            if (valid) for (int i = k + 1; i < N; ++i) A[N * i + k] = A[N * i + k] / akk;
            if (sign == 1) { if (akk < 0) sign = 2; }
            else if (sign == -1) { if (akk > 0) sign = 2; }
            else if (sign == 0) { if (akk > 0) sign = 1; else if (akk < 0) sign = -1; }
        }
    }
    if (!(sign == 1 || sign == 0)) return false;
    for (int i = 0; i < N; ++i) x[i] = b[i];
    for (int k = 0; k < N; ++k) { const double t = x[k]; x[k] = x[transp[k]]; x[transp[k]] = t; }
    for (int i = 1; i < N; ++i) { double s = 0; for (int j = 0; j < i; ++j) s += A[N * i + j] * x[j]; x[i] -= s; }
    const double tol = 1.0 / DBL_MAX;
    for (int i = 0; i < N; ++i) x[i] = fabs(A[(N + 1) * i]) > tol ? x[i] / A[(N + 1) * i] : 0.0;
    for (int i = N - 2; i >= 0; --i) { double s = 0; for (int j = i + 1; j < N; ++j) s += A[N * j + i] * x[j]; x[i] -= s; }
    for (int k = N - 1; k >= 0; --k) { const double t = x[k]; x[k] = x[transp[k]]; x[transp[k]] = t; }
    return true;
}

// Matrix3d::inverse() (LU/InverseImpl.h, compute_inverse<Matrix3d, Matrix3d, 3>: the cofactor form).  cofactor_3x3<i, j> =
// m(i1, j1) m(i2, j2) - m(i1, j2) m(i2, j1) with i1 = (i + 1) % 3, i2 = (i + 2) % 3 and j1, j2 alike; det = the first column of cofactors
// times the first column of m, summed in order; result(i, j) = cofactor<j, i> * (1 / det).  m, inv: row-major, inv is not m.  No test of
// the determinant, as Eigen has none.
__host__ __device__ inline double eigen_cofactor3(const double* m, int i, int j) {
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return m[3 * i1 + j1] * m[3 * i2 + j2] - m[3 * i1 + j2] * m[3 * i2 + j1];
}
__host__ __device__ inline void eigen_inverse3(const double* m, double* inv) {
    const double c00 = eigen_cofactor3(m, 0, 0), c10 = eigen_cofactor3(m, 1, 0), c20 = eigen_cofactor3(m, 2, 0);
    const double det = (c00 * m[0] + c10 * m[3]) + c20 * m[6];
    const double invdet = 1.0 / det;
    inv[0] = c00 * invdet; inv[1] = c10 * invdet; inv[2] = c20 * invdet;
    inv[3] = eigen_cofactor3(m, 0, 1) * invdet; inv[4] = eigen_cofactor3(m, 1, 1) * invdet; inv[5] = eigen_cofactor3(m, 2, 1) * invdet;
    inv[6] = eigen_cofactor3(m, 0, 2) * invdet; inv[7] = eigen_cofactor3(m, 1, 2) * invdet; inv[8] = eigen_cofactor3(m, 2, 2) * invdet;
}

// ---- SE(3) (types/se3quat.h) ------------------------------------------------------------------------------------------------------------
__host__ __device__ inline void se3_normalize_rotation(SE3Quat& T) {   // SE3Quat::normalizeRotation
    if (T.q[3] < 0) { T.q[0] *= -1; T.q[1] *= -1; T.q[2] *= -1; T.q[3] *= -1; }
    eigen_quat_normalize(T.q);
}
__host__ __device__ inline void se3_map(const SE3Quat& T, const double* v, double* out) {   // SE3Quat::map: _r*xyz + _t
    double r[3];
    eigen_quat_rotate(T.q, v, r);
    out[0] = r[0] + T.t[0]; out[1] = r[1] + T.t[1]; out[2] = r[2] + T.t[2];
}
// SE3Quat(R, t): Quaterniond(R), normalizeRotation
__host__ __device__ inline void se3_from_matrix(const double* R, const double* t, SE3Quat& T) {
    eigen_quat_from_matrix(R, T.q);
    T.t[0] = t[0]; T.t[1] = t[1]; T.t[2] = t[2];
    se3_normalize_rotation(T);
}
// Converter::toSE3Quat: float 4x4 -> Matrix3d, Vector3d -> SE3Quat(R, t)
__host__ __device__ inline void se3_from_cv(const float* M, SE3Quat& T) {
    double R[9], t[3];
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) R[3 * r + c] = (double)M[4 * r + c]; t[r] = (double)M[4 * r + 3]; }
    se3_from_matrix(R, t, T);
}
// SE3Quat::operator*: t = t1 + r1*t2, r = r1*r2, normalizeRotation
__host__ __device__ inline void se3_mul(const SE3Quat& a, const SE3Quat& b, SE3Quat& out) {
    double r[3], q[4];
    eigen_quat_rotate(a.q, b.t, r);
    eigen_quat_mul(a.q, b.q, q);
    out.t[0] = a.t[0] + r[0]; out.t[1] = a.t[1] + r[1]; out.t[2] = a.t[2] + r[2];
    out.q[0] = q[0]; out.q[1] = q[1]; out.q[2] = q[2]; out.q[3] = q[3];
    se3_normalize_rotation(out);
}
// SE3Quat::exp (:223-257).  order: where sin, cos and pow(theta, 3) come from.
__host__ __device__ inline void se3_exp(const double* update, int order, SE3Quat& T) {
    const double o0 = update[0], o1 = update[1], o2 = update[2];
    const double theta = sqrt(o0 * o0 + o1 * o1 + o2 * o2);
    const double O[9] = {0.0, -o2, o1, o2, 0.0, -o0, -o1, o0, 0.0};   // skew(omega)
    double O2[9], R[9], V[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) O2[3 * i + j] = O[3 * i] * O[j] + O[3 * i + 1] * O[3 + j] + O[3 * i + 2] * O[6 + j];
    if (theta < 0.00001) {
        for (int i = 0; i < 9; ++i) { R[i] = ((i % 4 == 0 ? 1.0 : 0.0) + O[i]) + O2[i]; V[i] = R[i]; }
    } else {
        double sn, cs, th3;
#ifndef __HIP_DEVICE_COMPILE__
        if (order == ORBM_POSE_ORDER_INDEX) { sn = sin(theta); cs = cos(theta); th3 = pow(theta, 3); } else
#endif
        { pose_sincos(theta, &sn, &cs); th3 = theta * theta * theta; }
        const double a = sn / theta, c = (1 - cs) / (theta * theta), d = (theta - sn) / th3;
        for (int i = 0; i < 9; ++i) {
            const double I = i % 4 == 0 ? 1.0 : 0.0;
            R[i] = (I + a * O[i]) + c * O2[i];
            V[i] = (I + c * O[i]) + d * O2[i];
        }
    }
    double t[3];
    for (int i = 0; i < 3; ++i) t[i] = V[3 * i] * update[3] + V[3 * i + 1] * update[4] + V[3 * i + 2] * update[5];
    se3_from_matrix(R, t, T);   // SE3Quat(Quaterniond(R), V*upsilon)
}

// an SE3Quat as seven doubles, q (x y z w) then t: how a port keeps its poses outside a record
__host__ __device__ inline void se3_load7(const double* v, SE3Quat& T) {
    T.q[0] = v[0]; T.q[1] = v[1]; T.q[2] = v[2]; T.q[3] = v[3]; T.t[0] = v[4]; T.t[1] = v[5]; T.t[2] = v[6];
}
__host__ __device__ inline void se3_store7(const SE3Quat& T, double* v) {
    v[0] = T.q[0]; v[1] = T.q[1]; v[2] = T.q[2]; v[3] = T.q[3]; v[4] = T.t[0]; v[5] = T.t[1]; v[6] = T.t[2];
}
// Converter::toCvMat(SE3Quat): to_homogeneous_matrix() rounded to float, M: 4x4 row-major
__host__ __device__ inline void se3_to_cv(const SE3Quat& T, float* M) {
    double R[9];
    eigen_quat_to_matrix(T.q, R);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) M[4 * r + c] = x86_nan((float)R[3 * r + c]);
        M[4 * r + 3] = x86_nan((float)T.t[r]);
    }
    M[12] = 0.0f; M[13] = 0.0f; M[14] = 0.0f; M[15] = 1.0f;
}

// ---- the edges through Tcim (types/types_six_dof_expmap.cpp) ------------------------------------------------------------------------------
// linearizeOplus of the _multi edges and of EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ as far as they share it (:627-696, :952-1036,
// :103-218, :318-461): t2 = t1 * Rcim, t1 the projection's derivative at pc = Tcim.map(p) (its zeros are not multiplied); with `row2`
// also the stereo row, row 2 = row 0 - bf / zc^2 * (the last row of Rcim), else row 2 is not written.  r: Rcim, row-major.  (row2 is
// the caller's and not "the edge is stereo": k_pose_optimize asks for it always and reads it for a stereo edge only, because a branch
// here costs its loop over the edges 1.4 - 2.2 % from 800 edges on, profiles/r21/notes_lba_shared.md.)
__host__ __device__ __forceinline__ void g2o_cam_jacobian_rows(double fx, double fy, double bf, const double* r, const double* pc, bool row2,
                                                               double (*t2)[3]) {
    const double xc = pc[0], yc = pc[1], zc = pc[2], zc_2 = zc * zc;
    const double t00 = -fx / zc, t02 = fx * xc / zc_2, t11 = -fy / zc, t12 = fy * yc / zc_2;
    t2[0][0] = t00 * r[0] + t02 * r[6];
    t2[0][1] = t00 * r[1] + t02 * r[7];
    t2[0][2] = t00 * r[2] + t02 * r[8];
    t2[1][0] = t11 * r[3] + t12 * r[6];
    t2[1][1] = t11 * r[4] + t12 * r[7];
    t2[1][2] = t11 * r[5] + t12 * r[8];
    if (!row2) return;
    const double a1 = bf / zc_2;
    t2[2][0] = t2[0][0] - a1 * r[6];
    t2[2][1] = t2[0][1] - a1 * r[7];
    t2[2][2] = t2[0][2] - a1 * r[8];
}
// one row of the pose block: t2's row times [-skew(p) | I], p = the point in the body frame
__host__ __device__ __forceinline__ void g2o_cam_jacobian_pose(const double* t2k, const double* p, double* Jk) {
    const double x = p[0], y = p[1], z = p[2];
    Jk[0] = -t2k[1] * z + t2k[2] * y;
    Jk[1] = t2k[0] * z - t2k[2] * x;
    Jk[2] = -t2k[0] * y + t2k[1] * x;
    Jk[3] = t2k[0];
    Jk[4] = t2k[1];
    Jk[5] = t2k[2];
}

// ---- the Huber kernel (core/robust_kernel_impl.cpp) ---------------------------------------------------------------------------------------
// `const float deltaMono = sqrt(5.991)` / `thHuberMono`, `sqrt(7.815)` for a stereo edge, rk->setDelta(th): _delta = the float as a
// double, dsqr = (float)(delta * delta), a FLOAT member.  Index 0: a mono edge, 1: a stereo one.
__host__ __device__ inline void g2o_huber_constants(double* delta, double* dsqr) {
    const float th[2] = {(float)sqrt(5.991), (float)sqrt(7.815)};
    for (int s = 0; s < 2; ++s) { delta[s] = (double)th[s]; dsqr[s] = (double)(float)(delta[s] * delta[s]); }
}
// RobustKernelHuber::robustify as far as rho[0] and rho[1] go (core/robust_kernel_impl.cpp:78-91); dsqr is the kernel's float member
__host__ __device__ inline void g2o_huber(double e, double delta, double dsqr, double* rho0, double* rho1) {
    if (e <= dsqr) { *rho0 = e; *rho1 = 1.; }
    else { const double sqrte = sqrt(e); *rho0 = 2 * sqrte * delta - dsqr; *rho1 = delta / sqrte; }
}

// ---- Sim(3) (types/sim3.h) --------------------------------------------------------------------------------------------------------------
// g2o::Sim3 NEVER normalises its quaternion: with theta < 1e-5 the rotation of Sim3(update) is I + Omega + Omega^2, which is not
// orthonormal, Quaterniond(R) of it is not a unit quaternion, operator* multiplies the quaternions as they are and map() rotates with
// _transformVector, which assumes a unit one.  All of that is followed here; se3_normalize_rotation is not to be called on a Sim3Quat.
struct Sim3Quat { double q[4], t[3], s; };   // g2o::Sim3: r (x y z w), t, s
enum { SIM3_EXP_SIGMA0_THETA0 = 0, SIM3_EXP_SIGMA0 = 1, SIM3_EXP_THETA0 = 2, SIM3_EXP_GENERAL = 3 };   // the branches of Sim3(Vector7d)

__host__ __device__ inline void sim3_map(const Sim3Quat& T, const double* v, double* out) {   // Sim3::map: s*(r*xyz) + t
    double r[3];
    eigen_quat_rotate(T.q, v, r);
    out[0] = T.s * r[0] + T.t[0]; out[1] = T.s * r[1] + T.t[1]; out[2] = T.s * r[2] + T.t[2];
}
// Sim3(Matrix3d, Vector3d, double): Quaterniond(R) as it comes
__host__ __device__ inline void sim3_from_matrix(const double* R, const double* t, double s, Sim3Quat& T) {
    eigen_quat_from_matrix(R, T.q);
    T.t[0] = t[0]; T.t[1] = t[1]; T.t[2] = t[2];
    T.s = s;
}
// Sim3::inverse: Sim3(r.conjugate(), r.conjugate()*((-1./s)*t), 1./s)
__host__ __device__ inline void sim3_inverse(const Sim3Quat& T, Sim3Quat& out) {
    const double c = -1. / T.s;
    const double v[3] = {c * T.t[0], c * T.t[1], c * T.t[2]};
    out.q[0] = -T.q[0]; out.q[1] = -T.q[1]; out.q[2] = -T.q[2]; out.q[3] = T.q[3];
    eigen_quat_rotate(out.q, v, out.t);
    out.s = 1. / T.s;
}
// Sim3::operator*: r = r1*r2, t = s1*(r1*t2) + t1, s = s1*s2 (out is neither a nor b)
__host__ __device__ inline void sim3_mul(const Sim3Quat& a, const Sim3Quat& b, Sim3Quat& out) {
    double r[3];
    eigen_quat_mul(a.q, b.q, out.q);
    eigen_quat_rotate(a.q, b.t, r);
    out.t[0] = a.s * r[0] + a.t[0]; out.t[1] = a.s * r[1] + a.t[1]; out.t[2] = a.s * r[2] + a.t[2];
    out.s = a.s * b.s;
}
// Swi.map(Siw.map(P)) on a cv::Mat point: Converter::toVector3d, the two maps, Converter::toCvMat.  Step 7 of the essential graph
// (eg_dev.h eg_correct_point) and LoopClosing::CorrectLoop (src/LoopClosing.cc:701-705; mapcorrect_dev.h) are this one body.
__host__ __device__ inline void sim3_correct_point(const Sim3Quat& Siw, const Sim3Quat& Swi, const float* P, float* out) {
    const double p[3] = {(double)P[0], (double)P[1], (double)P[2]};   // Converter::toVector3d
    double a[3], b[3];
    sim3_map(Siw, p, a);
    sim3_map(Swi, a, b);
    out[0] = x86_nan((float)b[0]); out[1] = x86_nan((float)b[1]); out[2] = x86_nan((float)b[2]);   // Converter::toCvMat
}
// Sim3(const Vector7d& update) (:70-142), all four branches of fabs(sigma) < eps x theta < eps.  order: where sin, cos and exp come
// from (ORBM_POSE_ORDER_INDEX: the C library; otherwise pose_sincos and pose_exp).  Returns the branch taken.
__host__ __device__ inline int sim3_exp(const double* update, int order, Sim3Quat& T) {
    const double o0 = update[0], o1 = update[1], o2 = update[2];
    const double sigma = update[6];
    const double theta = sqrt(o0 * o0 + o1 * o1 + o2 * o2);
    const double O[9] = {0.0, -o2, o1, o2, 0.0, -o0, -o1, o0, 0.0};   // skew(omega)
    double O2[9], R[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) O2[3 * i + j] = O[3 * i] * O[j] + O[3 * i + 1] * O[3 + j] + O[3 * i + 2] * O[6 + j];
    double s, sn = 0., cs = 0.;
    const double eps = 0.00001;
#ifndef __HIP_DEVICE_COMPILE__
    if (order == ORBM_POSE_ORDER_INDEX) { s = exp(sigma); if (!(theta < eps)) { sn = sin(theta); cs = cos(theta); } } else
#endif
    { s = pose_exp(sigma); if (!(theta < eps)) pose_sincos(theta, &sn, &cs); }
    double A, B, C;
    int branch;
    if (fabs(sigma) < eps) {
        C = 1;
        if (theta < eps) {
            branch = SIM3_EXP_SIGMA0_THETA0;
            A = 1. / 2.;
            B = 1. / 6.;
            for (int i = 0; i < 9; ++i) R[i] = ((i % 4 == 0 ? 1.0 : 0.0) + O[i]) + O2[i];
        } else {
            branch = SIM3_EXP_SIGMA0;
            const double theta2 = theta * theta;
            A = (1 - cs) / theta2;
            B = (theta - sn) / (theta2 * theta);
            const double a = sn / theta, c = (1 - cs) / (theta * theta);
            for (int i = 0; i < 9; ++i) R[i] = ((i % 4 == 0 ? 1.0 : 0.0) + a * O[i]) + c * O2[i];
        }
    } else {
        C = (s - 1) / sigma;
        if (theta < eps) {
            branch = SIM3_EXP_THETA0;
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
            for (int i = 0; i < 9; ++i) R[i] = ((i % 4 == 0 ? 1.0 : 0.0) + O[i]) + O2[i];
        } else {
            branch = SIM3_EXP_GENERAL;
            const double ra = sn / theta, rc = (1 - cs) / (theta * theta);
            for (int i = 0; i < 9; ++i) R[i] = ((i % 4 == 0 ? 1.0 : 0.0) + ra * O[i]) + rc * O2[i];
            const double a = s * sn, b = s * cs;
            const double theta2 = theta * theta, sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    }
    eigen_quat_from_matrix(R, T.q);                        // r = Quaterniond(R)
    double W[9];
    for (int i = 0; i < 9; ++i) W[i] = (A * O[i] + B * O2[i]) + C * (i % 4 == 0 ? 1.0 : 0.0);
    for (int i = 0; i < 3; ++i) T.t[i] = W[3 * i] * update[3] + W[3 * i + 1] * update[4] + W[3 * i + 2] * update[5];
    T.s = s;
    return branch;
}

// Matrix3d::lu().solve(b) (LU/PartialPivLU.h: partial_lu_impl::unblocked_lu, then P b, the unit lower and the upper triangular solve).
// Per column the pivot is the FIRST largest |entry| at or below the diagonal, whole rows are swapped, the column below is divided by
// the pivot (not when it is exactly 0), the trailing block is updated entry by entry; each substitution subtracts its row's sum, taken
// in ascending index.  W: row-major, destroyed.  UNPINNED like the rest of this file.
__host__ __device__ inline void eigen_lu3_solve(double* W, const double* b, double* x) {
    double r[3] = {b[0], b[1], b[2]};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int row = k;
        double big = fabs(W[3 * k + k]);
#pragma unroll
        for (int i = k + 1; i < 3; ++i) { const double v = fabs(W[3 * i + k]); if (v > big) { big = v; row = i; } }
        if (big != 0.0) {
#pragma unroll
            for (int i = k + 1; i < 3; ++i) {
                if (i != row) continue;
#pragma unroll
                for (int c = 0; c < 3; ++c) { const double t = W[3 * k + c]; W[3 * k + c] = W[3 * i + c]; W[3 * i + c] = t; }
                const double t = r[k]; r[k] = r[i]; r[i] = t;                  // P b, transposition by transposition
            }
#pragma unroll
            for (int i = k + 1; i < 3; ++i) W[3 * i + k] = W[3 * i + k] / W[3 * k + k];
        }
#pragma unroll
        for (int i = k + 1; i < 3; ++i)
#pragma unroll
            for (int c = k + 1; c < 3; ++c) W[3 * i + c] = W[3 * i + c] - W[3 * i + k] * W[3 * k + c];
    }
    r[1] = r[1] - W[3] * r[0];
    r[2] = r[2] - (W[6] * r[0] + W[7] * r[1]);
    x[2] = r[2] / W[8];
    x[1] = (r[1] - W[5] * x[2]) / W[4];
    x[0] = (r[0] - (W[1] * x[1] + W[2] * x[2])) / W[0];
}

enum { SIM3_LOG_SIGMA0_D1 = 0, SIM3_LOG_SIGMA0 = 1, SIM3_LOG_D1 = 2, SIM3_LOG_GENERAL = 3 };   // the branches of Sim3::log()
// Sim3::log() (:148-230), all four branches of fabs(sigma) < eps x d > 1 - eps, statement by statement: deltaR, skew, W = A Omega +
// B Omega Omega + C I, W.lu().solve(t).  Nothing is normalised; near d = -1 the division by sqrt(1 - d*d) is the reference's.  order:
// where log, acos, sin and cos come from (ORBM_POSE_ORDER_INDEX: the C library; otherwise pose_log, pose_acos, pose_sincos).  Returns
// the branch taken.
__host__ __device__ inline int sim3_log(const Sim3Quat& T, int order, double* res) {
    double R[9];
    eigen_quat_to_matrix(T.q, R);
    const double s = T.s;
    double sigma;
#ifndef __HIP_DEVICE_COMPILE__
    const bool libm = order == ORBM_POSE_ORDER_INDEX;
    if (libm) sigma = log(s); else
#endif
    sigma = pose_log(s);
    const double d = 0.5 * (((R[0] + R[4]) + R[8]) - 1);
    const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};   // deltaR(R)
    const double eps = 0.00001;
    double omega[3], A, B, C;
    int branch;
    double theta = 0., sn = 0., cs = 0.;
    if (!(d > 1 - eps)) {
#ifndef __HIP_DEVICE_COMPILE__
        if (libm) { theta = acos(d); sn = sin(theta); cs = cos(theta); } else
#endif
        { theta = pose_acos(d); pose_sincos(theta, &sn, &cs); }
    }
    if (fabs(sigma) < eps) {
        C = 1;
        if (d > 1 - eps) {
            branch = SIM3_LOG_SIGMA0_D1;
            for (int i = 0; i < 3; ++i) omega[i] = 0.5 * dR[i];
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            branch = SIM3_LOG_SIGMA0;
            const double theta2 = theta * theta;
            const double f = theta / (2 * sqrt(1 - d * d));
            for (int i = 0; i < 3; ++i) omega[i] = f * dR[i];
            A = (1 - cs) / (theta2);
            B = (theta - sn) / (theta2 * theta);
        }
    } else {
        C = (s - 1) / sigma;
        if (d > 1 - eps) {
            branch = SIM3_LOG_D1;
            const double sigma2 = sigma * sigma;
            for (int i = 0; i < 3; ++i) omega[i] = 0.5 * dR[i];
            A = ((sigma - 1) * s + 1) / (sigma2);
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
        } else {
            branch = SIM3_LOG_GENERAL;
            const double f = theta / (2 * sqrt(1 - d * d));
            for (int i = 0; i < 3; ++i) omega[i] = f * dR[i];
            const double theta2 = theta * theta;
            const double a = s * sn;
            const double b = s * cs;
            const double c = theta2 + sigma * sigma;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
        }
    }
    const double O[9] = {0.0, -omega[2], omega[1], omega[2], 0.0, -omega[0], -omega[1], omega[0], 0.0};   // skew(omega)
    double O2[9], W[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) O2[3 * i + j] = O[3 * i] * O[j] + O[3 * i + 1] * O[3 + j] + O[3 * i + 2] * O[6 + j];
    for (int i = 0; i < 9; ++i) W[i] = (A * O[i] + B * O2[i]) + C * (i % 4 == 0 ? 1.0 : 0.0);
    double ups[3];
    eigen_lu3_solve(W, T.t, ups);
    res[0] = omega[0]; res[1] = omega[1]; res[2] = omega[2];
    res[3] = ups[0]; res[4] = ups[1]; res[5] = ups[2];
    res[6] = sigma;
    return branch;
}
