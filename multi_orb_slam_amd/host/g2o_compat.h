// g2o_compat.h -- a stand-in for g2o::Sim3 (reference Thirdparty/g2o/g2o/types/sim3.h) with the members Optimizer::OptimizeSim3_cam1 and
// its callers use: the three constructors, rotation(), translation(), scale(), operator*, inverse(), map().  The host library links no
// g2o and no Eigen, so the quaternion, the 3-vector and the 3x3 matrix are small types of the same names in namespace g2o, where the
// reference's `using namespace Eigen` puts Eigen's.  Like the original, nothing here normalises the quaternion.
// Inside the reference build define HAVE_G2O: the reference's own header is used and this file declares nothing (the way cv_compat.h
// yields to OpenCV under HAVE_OPENCV).
#pragma once
#ifdef HAVE_G2O
#include "Thirdparty/g2o/g2o/types/sim3.h"
#else
#include <cmath>

namespace g2o {

struct Vector3d {
    double v[3];
    Vector3d() : v{0, 0, 0} {}
    Vector3d(double x, double y, double z) : v{x, y, z} {}
    double& operator[](int i) { return v[i]; }
    const double& operator[](int i) const { return v[i]; }
    double& operator()(int i) { return v[i]; }
    const double& operator()(int i) const { return v[i]; }
};

struct Matrix3d {   // row-major storage; (r, c) as Eigen's
    double m[9];
    Matrix3d() : m{0, 0, 0, 0, 0, 0, 0, 0, 0} {}
    double& operator()(int r, int c) { return m[3 * r + c]; }
    const double& operator()(int r, int c) const { return m[3 * r + c]; }
    static Matrix3d Identity() { Matrix3d I; I.m[0] = I.m[4] = I.m[8] = 1; return I; }
};

struct Quaterniond {   // Eigen's coefficient order x y z w
    double c[4];
    Quaterniond() : c{0, 0, 0, 1} {}
    Quaterniond(double w, double x, double y, double z) : c{x, y, z, w} {}
    // Quaternion(Matrix3d): quaternionbase_assign_impl<Other,3,3>
    explicit Quaterniond(const Matrix3d& M) {
        const double* m = M.m;
        double t = m[0] + m[4] + m[8];
        if (t > 0) {
            t = std::sqrt(t + 1.0);
            c[3] = 0.5 * t;
            t = 0.5 / t;
            c[0] = (m[7] - m[5]) * t; c[1] = (m[2] - m[6]) * t; c[2] = (m[3] - m[1]) * t;
        } else {
            int i = 0;
            if (m[4] > m[0]) i = 1;
            if (m[8] > m[4 * i]) i = 2;
            const int j = (i + 1) % 3, k = (j + 1) % 3;
            t = std::sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0);
            c[i] = 0.5 * t;
            t = 0.5 / t;
            c[3] = (m[3 * k + j] - m[3 * j + k]) * t;
            c[j] = (m[3 * j + i] + m[3 * i + j]) * t;
            c[k] = (m[3 * k + i] + m[3 * i + k]) * t;
        }
    }
    double x() const { return c[0]; } double y() const { return c[1]; } double z() const { return c[2]; } double w() const { return c[3]; }
    const double* coeffs() const { return c; }
    void setIdentity() { c[0] = c[1] = c[2] = 0; c[3] = 1; }
    Quaterniond conjugate() const { return Quaterniond(c[3], -c[0], -c[1], -c[2]); }
    Quaterniond operator*(const Quaterniond& b) const {   // quat_product
        return Quaterniond(c[3] * b.c[3] - c[0] * b.c[0] - c[1] * b.c[1] - c[2] * b.c[2],
                           c[3] * b.c[0] + c[0] * b.c[3] + c[1] * b.c[2] - c[2] * b.c[1],
                           c[3] * b.c[1] + c[1] * b.c[3] + c[2] * b.c[0] - c[0] * b.c[2],
                           c[3] * b.c[2] + c[2] * b.c[3] + c[0] * b.c[1] - c[1] * b.c[0]);
    }
    Vector3d operator*(const Vector3d& v) const {          // _transformVector
        double uv[3] = {c[1] * v[2] - c[2] * v[1], c[2] * v[0] - c[0] * v[2], c[0] * v[1] - c[1] * v[0]};
        uv[0] = uv[0] + uv[0]; uv[1] = uv[1] + uv[1]; uv[2] = uv[2] + uv[2];
        return Vector3d(v[0] + c[3] * uv[0] + (c[1] * uv[2] - c[2] * uv[1]), v[1] + c[3] * uv[1] + (c[2] * uv[0] - c[0] * uv[2]),
                        v[2] + c[3] * uv[2] + (c[0] * uv[1] - c[1] * uv[0]));
    }
    Matrix3d toRotationMatrix() const {
        const double tx = 2 * c[0], ty = 2 * c[1], tz = 2 * c[2];
        const double twx = tx * c[3], twy = ty * c[3], twz = tz * c[3];
        const double txx = tx * c[0], txy = ty * c[0], txz = tz * c[0];
        const double tyy = ty * c[1], tyz = tz * c[1], tzz = tz * c[2];
        Matrix3d R;
        R.m[0] = 1 - (tyy + tzz); R.m[1] = txy - twz; R.m[2] = txz + twy;
        R.m[3] = txy + twz; R.m[4] = 1 - (txx + tzz); R.m[5] = tyz - twx;
        R.m[6] = txz - twy; R.m[7] = tyz + twx; R.m[8] = 1 - (txx + tyy);
        return R;
    }
};

struct Sim3 {
protected:
    Quaterniond r;
    Vector3d t;
    double s;

public:
    Sim3() : s(1.) {}
    Sim3(const Quaterniond& r_, const Vector3d& t_, double s_) : r(r_), t(t_), s(s_) {}
    Sim3(const Matrix3d& R, const Vector3d& t_, double s_) : r(Quaterniond(R)), t(t_), s(s_) {}
    Vector3d map(const Vector3d& xyz) const { const Vector3d p = r * xyz; return Vector3d(s * p[0] + t[0], s * p[1] + t[1], s * p[2] + t[2]); }
    Sim3 inverse() const {
        const double k = -1. / s;
        return Sim3(r.conjugate(), r.conjugate() * Vector3d(k * t[0], k * t[1], k * t[2]), 1. / s);
    }
    Sim3 operator*(const Sim3& other) const {
        const Vector3d p = r * other.t;
        return Sim3(r * other.r, Vector3d(s * p[0] + t[0], s * p[1] + t[1], s * p[2] + t[2]), s * other.s);
    }
    const Vector3d& translation() const { return t; }
    Vector3d& translation() { return t; }
    const Quaterniond& rotation() const { return r; }
    Quaterniond& rotation() { return r; }
    const double& scale() const { return s; }
    double& scale() { return s; }
};

}  // namespace g2o
#endif
