// triangulate.hip -- triangulation and gating of new map points on the device (include/orbv.h, "Triangulation and gating"): the loop over
// the matched pairs in LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:388-669) and KeyFrame::UnprojectStereo
// (src/KeyFrame.cc:985-1012), from the pair of feature indices to the verdict and the point, up to `new MapPoint`.
//   tri_*            the arithmetic, ONE statement sequence for the kernel and for the host routine (orbv_triangulate_pairs_host), statement
//                    by statement in the number formats the reference's statements have under OpenCV 2.4.x / 3.2 (the rules of
//                    host/cv_compat.h: gemm_small_f32 for 3x3 * 3x1, Mat::dot and cv::norm in double, MatExpr folding).  The OpenCV
//                    operations that other routines call as well are cv_dev.h's; the SVD and the row expression are this file's.
//   k_triangulate    one lane per pair, no LDS, no exchange between lanes: pairs are independent.  The 4x4, its working copy, Vt and the
//                    four double row norms of the Jacobi sweeps stay in registers (every index below is a compile-time constant after
//                    unrolling; the row swaps of the sort are selects).  A few hundred flops per pair on at most a few thousand lanes:
//                    latency-bound, sized at one wavefront per workgroup so that a batch spreads over the compute units.
//   k_triangulate_round   the fused form of k_triangulate (pair (i, match[i])) for one neighbour of the chained call
//                    (orbv_create_new_points_keyframe): the lane that owns feature i also keeps the feature's state byte -- bit 0 = "has
//                    no map point yet", cleared when the pair is accepted, as mpCurrentKeyFrame->AddMapPoint does between two neighbours
//                    (:682) -- and writes the flag byte the NEXT neighbour's search reads for i.  A feature is in at most one pair per
//                    round and every lane touches its own bytes only: no atomics, no LDS.  k_round_flags forms the first round's flags.
// No libm function runs in the kernel: + - * / sqrt in float and double only.  cos(2*atan2(mb/2, depth)) is a per-feature constant and
// arrives as an array (orbv_cos_stereo, host libm), as k_frustum takes its logf.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/orbv.h"
#include "orb_common.h"
#include "bow_internal.h"
#include "cv_dev.h"
#include "stage_pack.h"

using morb::MAX_LEVELS;

namespace {

struct TriKf {   // one keyframe's constants.  The kernel reads the pair of them from device memory: the camera and the octave index into
                 // them per lane, and a by-value kernel argument indexed at run time is copied to scratch memory first
    float Tcw[2][12], centre[2][3], Twc[12], Rcam12[9], tcam12[3];
    float fx, fy, cx, cy, invfx, invfy, mbf;
    int n_levels, n_cam1;
    float scale[MAX_LEVELS], sigma2[MAX_LEVELS];
};
struct TriFeat { float x, y, xd, yd, uright, depth, cos_stereo; int octave, cam, idx; };   // one feature of a pair

// ---- the OpenCV boundary: what only CreateNewMapPoints calls (the rest: cv_dev.h) ------------------------------------------------------
// cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) of a 4x4 CV_32F, as far as vt goes.  UNPINNED against OpenCV: restated from
// JacobiSVDImpl_<float> (modules/core/src/lapack.cpp, 2.4.x / 3.2) as called by _SVDcompute for m == n == 4:
//   * the working copy is the TRANSPOSE of A (row i of At = column i of A; Vt starts as the identity);
//   * W[i] = the squared norm of row i and p = the product of rows i and j are accumulated in DOUBLE, in element order;
//   * a pair is skipped when |p| <= eps*sqrt(a*b) with eps = FLT_EPSILON*2 (a float, promoted); minval = FLT_MIN enters only the
//     completion below and is therefore not used here;
//   * at most max(m, 30) = 30 sweeps over the pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), ended by a sweep that rotates nothing;
//   * c and s are computed in double from p*2, beta = a - b and gamma = hypot(p, beta) (cv_hypot_libm here) and ROUNDED TO FLOAT, the
//     second of them from the rounded first; the rotation of the rows of At and of Vt is in float, t0 = c*x + s*y, t1 = -s*x + c*y
//     (the SSE form of the Vt rotation, y*c - x*s, has the same bits); the new W[i], W[j] are double sums of the rotated elements;
//   * the singular values are sqrt of freshly summed row norms; the sort is a selection sort, descending, strict `W[j] < W[k]`, that
//     swaps W and the rows of At and Vt of i and j;
//   * the completion to a full basis (random vectors for singular values <= minval, then the scaling by 1/sd) touches At -- that is
//     U -- only: for a square matrix Vt is complete from the rotations.  The reference reads vt.row(3) alone, so U and w are not
//     produced.
// null[4] = vt.row(3).
__host__ __device__ inline void tri_svd_null(const float A[4][4], float* null4) {
    float At[4][4], Vt[4][4];
    double W[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float t = A[k][i];
            At[i][k] = t;
            sd += (double)t * t;
            Vt[i][k] = 0;
        }
        W[i] = sd;
        Vt[i][i] = 1;
    }
    const float eps = FLT_EPSILON * 2;
    for (int iter = 0; iter < 30; ++iter) {
        bool changed = false;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = i + 1; j < 4; ++j) {
                double a = W[i], p = 0, b = W[j];
#pragma unroll
                for (int k = 0; k < 4; ++k) p += (double)At[i][k] * At[j][k];
                if (fabs(p) <= eps * sqrt(a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = cv_hypot_libm(p, beta);
                float c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = (float)sqrt(delta / gamma);
                    c = (float)(p / (gamma * s * 2));
                } else {
                    c = (float)sqrt((gamma + beta) / (gamma * 2));
                    s = (float)(p / (gamma * c * 2));
                }
                a = b = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float t0 = c * At[i][k] + s * At[j][k];
                    const float t1 = -s * At[i][k] + c * At[j][k];
                    At[i][k] = t0; At[j][k] = t1;
                    a += (double)t0 * t0; b += (double)t1 * t1;
                }
                W[i] = a; W[j] = b;
                changed = true;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float t0 = c * Vt[i][k] + s * Vt[j][k];
                    const float t1 = -s * Vt[i][k] + c * Vt[j][k];
                    Vt[i][k] = t0; Vt[j][k] = t1;
                }
            }
        }
        if (!changed) break;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { const float t = At[i][k]; sd += (double)t * t; }
        W[i] = sqrt(sd);
    }
    // for i: j = i; for k > i: if (W[j] < W[k]) j = k; swap(i, j) -- with the swap as selects, so that no index is a run-time value
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        int j = i;
        double wj = W[i];
#pragma unroll
        for (int k = i + 1; k < 4; ++k) if (wj < W[k]) { j = k; wj = W[k]; }
#pragma unroll
        for (int k = i + 1; k < 4; ++k)
            if (j == k) {
                const double tw = W[i]; W[i] = W[k]; W[k] = tw;
#pragma unroll
                for (int q = 0; q < 4; ++q) { const float tv = Vt[i][q]; Vt[i][q] = Vt[k][q]; Vt[k][q] = tv; }
            }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) null4[q] = Vt[3][q];
}

// A.row(r) = s*T.row(2) - T.row(q): a scaled-matrix expression minus a matrix folds into ONE element-wise call (cv_compat.h
// expr_addsub / ADDEX): cv::subtract when s == 1, otherwise cv::addWeighted with float weights, `a*s + b*(-1.0f) + 0.0f`.
// UNPINNED against OpenCV.
__host__ __device__ inline void tri_row(float s, const float* T, int q, float* row) {
    const double alpha = (double)s;
    const float al = (float)alpha, be = -1.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) row[k] = alpha == 1 ? T[8 + k] - T[4 * q + k] : T[8 + k] * al + T[4 * q + k] * be + 0.0f;
}
// KeyFrame::UnprojectStereo(i) (src/KeyFrame.cc:985-1012) for z > 0 (validated by the callers): the DISTORTED keypoint, the camera by
// i >= N of the feature's own keyframe, camera 2 through mRcam12*x3Dc + mtcam12; every product-plus-vector is one small-path gemm with
// beta = 1.
__host__ __device__ inline void tri_unproject(const TriKf& K, const TriFeat& f, float* x3D) {
    const float z = f.depth;
    const float u = f.xd, v = f.yd;
    const float x = (u - K.cx) * z * K.invfx;
    const float y = (v - K.cy) * z * K.invfy;
    float c[3] = {x, y, z};
    if (!(f.idx < K.n_cam1)) {
        float t[3];
        for (int r = 0; r < 3; ++r) t[r] = cv_gemm3(K.Rcam12 + 3 * r, 1, c, 1.0, K.tcam12[r], 1.0);
        for (int r = 0; r < 3; ++r) c[r] = t[r];
    }
    for (int r = 0; r < 3; ++r) x3D[r] = cv_gemm3(K.Twc + 4 * r, 1, c, 1.0, K.Twc[4 * r + 3], 1.0);
}

// the reprojection test of one keyframe (:549-591 / :596-634): T = the pair camera's [R|t] of that keyframe, K its intrinsics, mbf the
// CURRENT keyframe's in both tests (:583, :626).  true = rejected.
__host__ __device__ inline bool tri_reproject_fails(const float* T, const TriKf& K, float mbf, const TriFeat& f, const float* x3D, float z) {
    const float sigmaSquare = K.sigma2[f.octave];
    const float x = (float)(cv_dot3(T, x3D) + T[3]);
    const float y = (float)(cv_dot3(T + 4, x3D) + T[7]);
    const float invz = (float)(1.0 / z);
    if (!(f.uright >= 0)) {
        const float u = K.fx * x * invz + K.cx;
        const float v = K.fy * y * invz + K.cy;
        const float errX = u - f.x;
        const float errY = v - f.y;
        return (errX * errX + errY * errY) > 5.991 * sigmaSquare;
    }
    const float u = K.fx * x * invz + K.cx;
    const float u_r = u - mbf * invz;
    const float v = K.fy * y * invz + K.cy;
    const float errX = u - f.x;
    const float errY = v - f.y;
    const float errX_r = u_r - f.uright;
    return (errX * errX + errY * errY + errX_r * errX_r) > 7.8 * sigmaSquare;
}

// One pass of the loop body (:398-669).  cam_bits: bit c = istrian[c].
__host__ __device__ inline void tri_pair(const TriKf& K1, const TriKf& K2, const TriFeat& f1, const TriFeat& f2, unsigned cam_bits,
                                         float ratioFactor, orbv_tri_out& o) {
    o.x3D[0] = o.x3D[1] = o.x3D[2] = 0.0f; o.path = ORBV_TRI_PATH_NONE;
    const bool bStereo1 = f1.uright >= 0, bStereo2 = f2.uright >= 0;
    const int camIdx1 = f1.cam;                                       // the pair's camera comes from keyframe 1's feature only (:410)
    if (camIdx1 < 0 || camIdx1 > 1 || !((cam_bits >> camIdx1) & 1u)) { o.outcome = ORBV_TRI_CAM_OFF; return; }
    const float xn1[3] = {(f1.x - K1.cx) * K1.invfx, (f1.y - K1.cy) * K1.invfy, 1.0f};
    const float xn2[3] = {(f2.x - K2.cx) * K2.invfx, (f2.y - K2.cy) * K2.invfy, 1.0f};
    // ray = Rwc*xn with Rwc = Rcw.t() evaluated: the CAMERA-1 rotations, also for a camera-2 pair (:428-429)
    float ray1[3], ray2[3];
    for (int r = 0; r < 3; ++r) {
        ray1[r] = cv_gemm3(&K1.Tcw[0][r], 4, xn1, 1.0, 0.0f, 0.0);
        ray2[r] = cv_gemm3(&K2.Tcw[0][r], 4, xn2, 1.0, 0.0f, 0.0);
    }
    const float cosParallaxRays = (float)(cv_dot3(ray1, ray2) / (cv_norm3(ray1) * cv_norm3(ray2)));
    float cosParallaxStereo = cosParallaxRays + 1;
    float cosParallaxStereo1 = cosParallaxStereo;
    float cosParallaxStereo2 = cosParallaxStereo;
    if (bStereo1) cosParallaxStereo1 = f1.cos_stereo;
    else if (bStereo2) cosParallaxStereo2 = f2.cos_stereo;
    cosParallaxStereo = cosParallaxStereo2 < cosParallaxStereo1 ? cosParallaxStereo2 : cosParallaxStereo1;   // std::min(a, b)

    const float* T1 = K1.Tcw[camIdx1];
    const float* T2 = K2.Tcw[camIdx1];
    float x3D[3];
    if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && (bStereo1 || bStereo2 || cosParallaxRays < 0.9998)) {
        float A[4][4], nv[4];
        tri_row(xn1[0], T1, 0, A[0]);
        tri_row(xn1[1], T1, 1, A[1]);
        tri_row(xn2[0], T2, 0, A[2]);
        tri_row(xn2[1], T2, 1, A[3]);
        tri_svd_null(A, nv);
        o.path = ORBV_TRI_PATH_SVD;
        if (nv[3] == 0) {
            for (int k = 0; k < 3; ++k) o.x3D[k] = x86_nan(nv[k]);
            o.outcome = ORBV_TRI_W_ZERO; return;
        }
        const double alpha = 1. / (double)nv[3];
        for (int k = 0; k < 3; ++k) x3D[k] = cv_scale(nv[k], alpha);
    } else if (bStereo1 && cosParallaxStereo1 < cosParallaxStereo2) {
        tri_unproject(K1, f1, x3D);
        o.path = ORBV_TRI_PATH_UNPROJECT1;
    } else if (bStereo2 && cosParallaxStereo2 < cosParallaxStereo1) {
        tri_unproject(K2, f2, x3D);
        o.path = ORBV_TRI_PATH_UNPROJECT2;
    } else {
        o.outcome = ORBV_TRI_LOW_PARALLAX; return;
    }
    for (int k = 0; k < 3; ++k) o.x3D[k] = x86_nan(x3D[k]);

    const float z1 = (float)(cv_dot3(T1 + 8, x3D) + T1[11]);
    if (z1 <= 0) { o.outcome = ORBV_TRI_Z1; return; }
    const float z2 = (float)(cv_dot3(T2 + 8, x3D) + T2[11]);
    if (z2 <= 0) { o.outcome = ORBV_TRI_Z2; return; }
    if (tri_reproject_fails(T1, K1, K1.mbf, f1, x3D, z1)) { o.outcome = ORBV_TRI_REPROJ1; return; }
    if (tri_reproject_fails(T2, K2, K1.mbf, f2, x3D, z2)) { o.outcome = ORBV_TRI_REPROJ2; return; }

    float normal1[3], normal2[3];
    for (int k = 0; k < 3; ++k) { normal1[k] = x3D[k] - K1.centre[camIdx1][k]; normal2[k] = x3D[k] - K2.centre[camIdx1][k]; }
    const float dist1 = (float)cv_norm3(normal1);
    const float dist2 = (float)cv_norm3(normal2);
    if (dist1 == 0 || dist2 == 0) { o.outcome = ORBV_TRI_ZERO_DIST; return; }
    const float ratioDist = dist2 / dist1;
    const float ratioOctave = K1.scale[f1.octave] / K2.scale[f2.octave];
    if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) { o.outcome = ORBV_TRI_SCALE; return; }
    o.outcome = ORBV_TRI_ACCEPTED;
}

// ---- the kernel ------------------------------------------------------------------------------------------------------------------------
struct TriArrays {   // per-feature arrays of one keyframe in device memory
    int n;
    const float* x; const float* y; const float* xd; const float* yd; const float* uright; const float* depth; const float* cos_stereo;
    const int32_t* octave; const int32_t* cam_of;
};

__device__ __forceinline__ TriFeat tri_load(const TriArrays& F, int i, int n_levels) {
    TriFeat f;
    f.idx = i;
    f.x = F.x[i]; f.y = F.y[i]; f.xd = F.xd[i]; f.yd = F.yd[i]; f.uright = F.uright[i]; f.depth = F.depth[i];
    f.cos_stereo = f.uright >= 0 ? F.cos_stereo[i] : 0.0f;
    f.octave = min(max(F.octave[i], 0), n_levels - 1);   // (validated on the host where the host has the octaves; a table is never indexed beyond its end)
    f.cam = F.cam_of[i];
    return f;
}

// pairs != NULL: pair p = (pairs[2p], pairs[2p+1]).  pairs == NULL: pair p = (p, match[p]), no pair where match[p] < 0 (the fused call).
__global__ __launch_bounds__(64) void k_triangulate(const TriKf* __restrict__ K, TriArrays F1, TriArrays F2, const int32_t* __restrict__ pairs,
                                                    const int32_t* __restrict__ match, int n, unsigned cam_bits, float ratio_factor,
                                                    orbv_tri_out* __restrict__ out) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n) return;
    const TriKf& K1 = K[0];
    const TriKf& K2 = K[1];
    const int i1 = pairs ? pairs[2 * p] : p;
    const int i2 = pairs ? pairs[2 * p + 1] : match[p];
    orbv_tri_out o;
    o.x3D[0] = o.x3D[1] = o.x3D[2] = 0.0f; o.outcome = ORBV_TRI_NONE; o.path = ORBV_TRI_PATH_NONE;
    if (i1 >= 0 && i1 < F1.n && i2 >= 0 && i2 < F2.n) {
        const TriFeat f1 = tri_load(F1, i1, K1.n_levels), f2 = tri_load(F2, i2, K2.n_levels);
        tri_pair(K1, K2, f1, f2, cam_bits, ratio_factor, o);
    }
    out[p] = o;
}

// The chained call.  state[i]: the flag byte of feature i of `a` as the call received it, with bit 0 = free[i].  The flags a round's
// search reads: the state with bit 0 further gated by the round's camera bits (the reference's vbCam inside SearchForTriangulation).
__device__ __forceinline__ uint8_t round_flag(uint8_t state, int cam, unsigned cam_bits) {
    const bool on = cam >= 0 && cam <= 1 && ((cam_bits >> cam) & 1u);
    return (uint8_t)((state & 0xFEu) | ((state & 1u) && on ? 1u : 0u));
}
// in: the flags of the call (NULL: every feature usable and not stereo, as the searches read a NULL array)
__global__ __launch_bounds__(64) void k_round_flags(const uint8_t* __restrict__ in, const int32_t* __restrict__ cam_of, int n, unsigned cam_bits,
                                                    uint8_t* __restrict__ state, uint8_t* __restrict__ flags) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const uint8_t s = in ? in[i] : (uint8_t)1;
    state[i] = s;
    flags[i] = round_flag(s, cam_of[i], cam_bits);
}
// One neighbour: the record of the pair (p, match[p]) as k_triangulate's fused form writes it, then the state of feature p and, when
// another round follows (next_flags != NULL), that round's flag byte.  match: the words k_bow_finish left in HBM.
__global__ __launch_bounds__(64) void k_triangulate_round(const TriKf* __restrict__ K, TriArrays F1, TriArrays F2, const int32_t* __restrict__ match,
                                                          int n, unsigned cam_bits, float ratio_factor, orbv_tri_out* __restrict__ out,
                                                          uint8_t* __restrict__ state, uint8_t* next_flags, unsigned next_cam_bits) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n) return;
    const TriKf& K1 = K[0];
    const TriKf& K2 = K[1];
    const int i2 = match[p];
    orbv_tri_out o;
    o.x3D[0] = o.x3D[1] = o.x3D[2] = 0.0f; o.outcome = ORBV_TRI_NONE; o.path = ORBV_TRI_PATH_NONE;
    if (p < F1.n && i2 >= 0 && i2 < F2.n) {
        const TriFeat f1 = tri_load(F1, p, K1.n_levels), f2 = tri_load(F2, i2, K2.n_levels);
        tri_pair(K1, K2, f1, f2, cam_bits, ratio_factor, o);
    }
    out[p] = o;
    uint8_t s = state[p];
    if (o.outcome == ORBV_TRI_ACCEPTED) { s &= 0xFEu; state[p] = s; }
    if (next_flags) next_flags[p] = round_flag(s, F1.cam_of[p], next_cam_bits);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
int check_constants(const orbv_tri_keyframe* k, const char* name) {
    if (!k) { morb::set_error("%s is NULL", name); return ORB_E_ARG; }
    if (!k->scale_factors || !k->level_sigma2) { morb::set_error("%s: scale_factors / level_sigma2 is NULL", name); return ORB_E_ARG; }
    if (k->n_levels < 1 || k->n_levels > MAX_LEVELS) { morb::set_error("%s: n_levels = %d is outside 1..%d", name, k->n_levels, MAX_LEVELS); return ORB_E_ARG; }
    return ORB_OK;
}
int check_arrays(const orbv_tri_keyframe* k, const char* name) {
    if (k->n < 0 || k->n_cam1 < 0) { morb::set_error("%s: n = %d, n_cam1 = %d", name, k->n, k->n_cam1); return ORB_E_ARG; }
    if (k->n > 0 && !(k->x && k->y && k->xd && k->yd && k->octave && k->uright && k->depth && k->cos_stereo)) {
        morb::set_error("%s: a per-feature array is NULL", name); return ORB_E_ARG;
    }
    return ORB_OK;
}
void fill_constants(const orbv_tri_keyframe* k, TriKf& K) {
    memset(&K, 0, sizeof(K));
    memcpy(K.Tcw, k->Tcw, sizeof(K.Tcw)); memcpy(K.centre, k->centre, sizeof(K.centre)); memcpy(K.Twc, k->Twc, sizeof(K.Twc));
    memcpy(K.Rcam12, k->Rcam12, sizeof(K.Rcam12)); memcpy(K.tcam12, k->tcam12, sizeof(K.tcam12));
    K.fx = k->fx; K.fy = k->fy; K.cx = k->cx; K.cy = k->cy; K.invfx = k->invfx; K.invfy = k->invfy; K.mbf = k->mbf;
    K.n_levels = k->n_levels; K.n_cam1 = k->n_cam1;
    memcpy(K.scale, k->scale_factors, k->n_levels * sizeof(float)); memcpy(K.sigma2, k->level_sigma2, k->n_levels * sizeof(float));
}
inline int cam_of(const orbv_tri_keyframe* k, int i) { return k->cam_of ? k->cam_of[i] : (i >= k->n_cam1 ? 1 : 0); }
TriFeat feature_of(const orbv_tri_keyframe* k, int i) {
    TriFeat f;
    f.idx = i; f.x = k->x[i]; f.y = k->y[i]; f.xd = k->xd[i]; f.yd = k->yd[i]; f.uright = k->uright[i]; f.depth = k->depth[i];
    f.cos_stereo = f.uright >= 0 ? k->cos_stereo[i] : 0.0f;
    f.octave = k->octave[i]; f.cam = cam_of(k, i);
    return f;
}
int check_feature(const orbv_tri_keyframe* k, const char* name, int p, int i) {
    if (i < 0 || i >= k->n) { morb::set_error("pair %d: index %d is outside the %d features of %s", p, i, k->n, name); return ORB_E_ARG; }
    if (k->octave[i] < 0 || k->octave[i] >= k->n_levels) { morb::set_error("pair %d: octave %d of feature %d of %s is outside the %d levels", p, k->octave[i], i, name, k->n_levels); return ORB_E_ARG; }
    if (k->uright[i] >= 0 && !(k->depth[i] > 0)) { morb::set_error("pair %d: feature %d of %s is stereo (uright >= 0) with depth %g", p, i, name, (double)k->depth[i]); return ORB_E_ARG; }
    return ORB_OK;
}
int validate(const orbv_tri_keyframe* kf1, const orbv_tri_keyframe* kf2, const uint8_t* cam_enabled, const int32_t* pairs, int n_pairs,
             const orbv_tri_out* out) {
    int rc;
    if ((rc = check_constants(kf1, "kf1")) || (rc = check_constants(kf2, "kf2")) || (rc = check_arrays(kf1, "kf1")) || (rc = check_arrays(kf2, "kf2"))) return rc;
    if (!cam_enabled) { morb::set_error("cam_enabled is NULL"); return ORB_E_ARG; }
    if (n_pairs < 0 || (n_pairs > 0 && (!pairs || !out))) { morb::set_error("n_pairs = %d with pairs / out NULL or n_pairs negative", n_pairs); return ORB_E_ARG; }
    for (int p = 0; p < n_pairs; ++p) {
        if ((rc = check_feature(kf1, "kf1", p, pairs[2 * p])) || (rc = check_feature(kf2, "kf2", p, pairs[2 * p + 1]))) return rc;
        const int c = cam_of(kf1, pairs[2 * p]);
        if (c < 0 || c > 1) { morb::set_error("pair %d: camera %d of feature %d of kf1 is outside cam_enabled[2]", p, c, pairs[2 * p]); return ORB_E_ARG; }
    }
    return ORB_OK;
}
// the two keyframes' constants, written by the host straight into the staging buffer the kernel reads (no copy call)
int stage_constants(orbv_workspace* w, const orbv_tri_keyframe* kf1, const orbv_tri_keyframe* kf2, const TriKf** d_K) {
    int rc = w->tri_const.reserve(2 * sizeof(TriKf));
    if (rc) return rc;
    TriKf K[2];
    fill_constants(kf1, K[0]); fill_constants(kf2, K[1]);
    memcpy(w->tri_const.p, K, sizeof(K));
    w->tri_const.publish();
    *d_K = (const TriKf*)w->tri_const.dp;
    return ORB_OK;
}
inline unsigned cam_bits_of(const uint8_t* cam_enabled) { return (cam_enabled[0] ? 1u : 0u) | (cam_enabled[1] ? 2u : 0u); }

// what the fused calls validate beyond the search, for one (a, b, geometry)
int check_fused(const orbv_keyframe* a, const orbv_keyframe* b, const orbv_tri_geometry* geometry) {
    if (!geometry) { morb::set_error("geometry is NULL"); return ORB_E_ARG; }
    int rc;
    if ((rc = check_constants(&geometry->kf1, "geometry->kf1")) || (rc = check_constants(&geometry->kf2, "geometry->kf2"))) return rc;
    if (!a->has_geometry || !b->has_geometry) { morb::set_error("keyframe %s has no geometry arrays (orbv_keyframe_set_geometry)", !a->has_geometry ? "a" : "b"); return ORB_E_ARG; }
    if (a->max_cam > 1) { morb::set_error("keyframe a has a feature of camera %d, outside cam_enabled[2]", a->max_cam); return ORB_E_ARG; }
    if (a->max_octave >= geometry->kf1.n_levels) { morb::set_error("keyframe a has octave %d, outside the %d levels", a->max_octave, geometry->kf1.n_levels); return ORB_E_ARG; }
    if (b->max_octave >= geometry->kf2.n_levels) { morb::set_error("keyframe b has octave %d, outside the %d levels", b->max_octave, geometry->kf2.n_levels); return ORB_E_ARG; }
    return ORB_OK;
}
TriArrays arrays_of(const orbv_keyframe* k) {
    TriArrays F;
    F.n = k->D.n; F.x = k->D.x; F.y = k->D.y; F.octave = k->D.octave; F.cam_of = k->D.cam_of;
    F.xd = k->G.xd; F.yd = k->G.yd; F.uright = k->G.uright; F.depth = k->G.depth; F.cos_stereo = k->G.cos_stereo;
    return F;
}

}  // namespace

extern "C" {

int orbv_cos_stereo(float mb, const float* depth, int n, float* cos_stereo) {
    MORB_ARG(n >= 0 && (n == 0 || (depth && cos_stereo)));
    // cosParallaxStereo1 = cos(2*atan2(mpCurrentKeyFrame->mb/2, mpCurrentKeyFrame->mvDepth_total[idx1]))   (src/LocalMapping.cc:447, :449)
    // mb and the depth are float.  Compiled against host/cv_shim with the headers the reference's translation unit sees, the call
    // atan2(float, float) resolves to the float overload, `2*` stays float and cos(float) is the float overload again (checked with
    // static_assert on decltype of the three sub-expressions): atan2f, then cosf, nothing in double.
    for (int i = 0; i < n; ++i) cos_stereo[i] = cosf(2 * atan2f(mb / 2, depth[i]));
    return ORB_OK;
}

int orbv_triangulate_pairs_host(const orbv_tri_keyframe* kf1, const orbv_tri_keyframe* kf2, const uint8_t* cam_enabled, const int32_t* pairs,
                                int n_pairs, float ratio_factor, orbv_tri_out* out) {
    int rc = validate(kf1, kf2, cam_enabled, pairs, n_pairs, out);
    if (rc) return rc;
    TriKf K1, K2;
    fill_constants(kf1, K1); fill_constants(kf2, K2);
    const unsigned bits = cam_bits_of(cam_enabled);
    for (int p = 0; p < n_pairs; ++p) tri_pair(K1, K2, feature_of(kf1, pairs[2 * p]), feature_of(kf2, pairs[2 * p + 1]), bits, ratio_factor, out[p]);
    return ORB_OK;
}

int orbv_triangulate_pairs(orbv_workspace* w, const orbv_tri_keyframe* kf1, const orbv_tri_keyframe* kf2, const uint8_t* cam_enabled,
                           const int32_t* pairs, int n_pairs, float ratio_factor, orbv_tri_out* out) {
    MORB_ARG(w != nullptr);
    int rc = validate(kf1, kf2, cam_enabled, pairs, n_pairs, out);
    if (rc) return rc;
    if (n_pairs == 0) return ORB_OK;
    MORB_HIP(hipSetDevice(w->device));
    // one packed block through the pinned stage: nine arrays per keyframe (a keyframe without features keeps its slots), then the pairs
    const orbv_tri_keyframe* kf[2] = {kf1, kf2};
    morb::StagePack pk;
    int id[2][9];
    for (int s = 0; s < 2; ++s) {
        const orbv_tri_keyframe* k = kf[s]; const size_t slot = (size_t)std::max(k->n, 1) * 4;
        const void* src[8] = {k->x, k->y, k->xd, k->yd, k->uright, k->depth, k->cos_stereo, k->octave};
        for (int a = 0; a < 8; ++a) id[s][a] = k->n > 0 ? pk.add(src[a], slot) : pk.add_in_place(slot);
        id[s][8] = pk.add_in_place(slot);   // the camera of every feature, written below
    }
    const int i_pairs = pk.add(pairs, (size_t)n_pairs * 8);
    const morb::StagePack::Block blk = pk.open(w->h_stage, w->d_stage, &rc);
    if (rc || (rc = w->h_tri.reserve((size_t)n_pairs * sizeof(orbv_tri_out)))) return rc;
    TriArrays F[2];
    for (int s = 0; s < 2; ++s) {
        const int* a = id[s];
        for (int i = 0; i < kf[s]->n; ++i) blk.host<int32_t>(a[8])[i] = cam_of(kf[s], i);
        F[s].n = kf[s]->n; F[s].x = blk.dev<float>(a[0]); F[s].y = blk.dev<float>(a[1]); F[s].xd = blk.dev<float>(a[2]); F[s].yd = blk.dev<float>(a[3]);
        F[s].uright = blk.dev<float>(a[4]); F[s].depth = blk.dev<float>(a[5]); F[s].cos_stereo = blk.dev<float>(a[6]);
        F[s].octave = blk.dev<int32_t>(a[7]); F[s].cam_of = blk.dev<int32_t>(a[8]);
    }
    const TriKf* d_K = nullptr;
    if ((rc = stage_constants(w, kf1, kf2, &d_K))) return rc;
    MORB_HIP(hipMemcpyAsync(w->d_stage.p, w->h_stage.p, pk.bytes(), hipMemcpyHostToDevice, w->stream));
    hipLaunchKernelGGL(k_triangulate, dim3((n_pairs + 63) / 64), dim3(64), 0, w->stream, d_K, F[0], F[1], blk.dev<int32_t>(i_pairs),
                       (const int32_t*)nullptr, n_pairs, cam_bits_of(cam_enabled), ratio_factor, (orbv_tri_out*)w->h_tri.dp);
    MORB_HIP(hipGetLastError());
    MORB_HIP(hipStreamSynchronize(w->stream));
    memcpy(out, w->h_tri.p, (size_t)n_pairs * sizeof(orbv_tri_out));
    return ORB_OK;
}

int orbv_keyframe_set_geometry(orbv_workspace* w, orbv_keyframe* k, const float* uright, const float* depth, const float* cos_stereo,
                               const float* xd, const float* yd) {
    MORB_ARG(w != nullptr && k != nullptr && w->device == k->device);
    if (!k->tri) { morb::set_error("the keyframe was built without the triangulation arrays (x / y / octave)"); return ORB_E_ARG; }
    const int n = k->D.n;
    if (n > 0 && !(uright && depth && cos_stereo && xd && yd)) { morb::set_error("a geometry array is NULL"); return ORB_E_ARG; }
    for (int i = 0; i < n; ++i)
        if (uright[i] >= 0 && !(depth[i] > 0)) { morb::set_error("feature %d is stereo (uright >= 0) with depth %g", i, (double)depth[i]); return ORB_E_ARG; }
    MORB_HIP(hipSetDevice(w->device));
    const size_t stride = morb::align16((size_t)std::max(n, 1) * 4);
    int rc = k->geometry.reserve(5 * stride);
    if (rc) return rc;
    std::vector<uint8_t> host(5 * stride, 0);
    const float* src[5] = {uright, depth, cos_stereo, xd, yd};
    for (int a = 0; a < 5; ++a) if (n > 0) memcpy(host.data() + a * stride, src[a], (size_t)n * 4);
    MORB_HIP(hipMemcpyAsync(k->geometry.p, host.data(), host.size(), hipMemcpyHostToDevice, w->stream));
    MORB_HIP(hipStreamSynchronize(w->stream));   // (the source is a local)
    const uint8_t* B = k->geometry.p;
    k->G.uright = (const float*)B; k->G.depth = (const float*)(B + stride); k->G.cos_stereo = (const float*)(B + 2 * stride);
    k->G.xd = (const float*)(B + 3 * stride); k->G.yd = (const float*)(B + 4 * stride);
    k->has_geometry = true;
    return ORB_OK;
}

int orbv_create_new_points_resident(orbv_workspace* w, const orbv_keyframe* a, const uint8_t* flags_a, const orbv_keyframe* b,
                                    const uint8_t* flags_b, const orbv_triangulation* t, const orbv_tri_geometry* geometry, int th_low,
                                    int check_orientation, int32_t* match, orbv_tri_out* out, int* n_accepted) {
    MORB_ARG(w != nullptr && a != nullptr && b != nullptr && n_accepted != nullptr);
    int rc = check_fused(a, b, geometry);
    if (rc) return rc;
    const int n = a->D.n;
    if (n > 0 && !out) { morb::set_error("out is NULL"); return ORB_E_ARG; }
    *n_accepted = 0;
    const TriKf* d_K = nullptr;
    if (n > 0) {
        MORB_ARG(w->device == a->device);
        MORB_HIP(hipSetDevice(w->device));
        if ((rc = w->h_tri.reserve((size_t)n * sizeof(orbv_tri_out))) || (rc = stage_constants(w, &geometry->kf1, &geometry->kf2, &d_K))) return rc;
    }
    int nmatches = 0, enqueued = 0;
    const int32_t* d_match = nullptr;
    if ((rc = morb::bow_triangulation_search_enqueue(w, a, flags_a, b, flags_b, t, th_low, check_orientation, match, &nmatches, &enqueued, &d_match))) return rc;
    if (n > 0) memset(out, 0, (size_t)n * sizeof(orbv_tri_out));
    if (!enqueued) return ORB_OK;
    const TriArrays F[2] = {arrays_of(a), arrays_of(b)};
    // behind the search on the same stream: the match words are read where k_bow_finish left them
    hipLaunchKernelGGL(k_triangulate, dim3((n + 63) / 64), dim3(64), 0, w->stream, d_K, F[0], F[1], (const int32_t*)nullptr, d_match, n,
                       cam_bits_of(geometry->cam_enabled), geometry->ratio_factor, (orbv_tri_out*)w->h_tri.dp);
    MORB_HIP(hipGetLastError());
    MORB_HIP(hipStreamSynchronize(w->stream));
    morb::bow_search_collect(w, n, match, &nmatches);
    memcpy(out, w->h_tri.p, (size_t)n * sizeof(orbv_tri_out));
    int acc = 0;
    for (int i = 0; i < n; ++i) acc += out[i].outcome == ORBV_TRI_ACCEPTED;
    *n_accepted = acc;
    return ORB_OK;
}

int orbv_create_new_points_keyframe(orbv_workspace* w, const orbv_keyframe* a, const uint8_t* flags_a, const orbv_new_points_round* rounds,
                                    int n_rounds, int th_low, int check_orientation, int32_t* match, orbv_tri_out* out, int* n_matches,
                                    int* n_accepted) {
    MORB_ARG(w != nullptr && a != nullptr);
    for (int i = 0; i < 4; ++i) w->last_kf_call[i] = 0;
    if (n_rounds < 0 || n_rounds > ORBV_MAX_ROUNDS) { morb::set_error("n_rounds = %d is outside 0..%d", n_rounds, ORBV_MAX_ROUNDS); return ORB_E_ARG; }
    MORB_ARG(n_rounds == 0 || (rounds != nullptr && n_matches != nullptr && n_accepted != nullptr));
    const int n = a->D.n;
    if (n_rounds > 0 && n > 0 && (!match || !out)) { morb::set_error("match / out is NULL"); return ORB_E_ARG; }
    // ---- validation, all or nothing: nothing has been touched when a round is refused
    bool runs[ORBV_MAX_ROUNDS];
    int n_run = 0, first = -1;
    size_t stage_bytes = flags_a ? morb::align16((size_t)n) : 0, flags_off[ORBV_MAX_ROUNDS];
    for (int k = 0; k < n_rounds; ++k) {
        const orbv_new_points_round& r = rounds[k];
        int rc = r.b ? ORB_OK : ORB_E_ARG;
        if (rc) morb::set_error("the neighbour is NULL");
        if (!rc) rc = check_fused(a, r.b, &r.geometry);
        if (!rc) rc = morb::bow_chain_check(w, a, r.b, &r.t);
        if (rc) { const std::string why = orb_last_error(); morb::set_error("round %d: %s", k, why.c_str()); return rc; }
        runs[k] = n > 0 && morb::bow_chain_runs(a, r.b);
        flags_off[k] = stage_bytes;
        if (runs[k]) {
            if (first < 0) first = k;
            ++n_run;
            if (r.flags_b) stage_bytes += morb::align16((size_t)r.b->D.n);
        }
    }
    w->last_kf_call[0] = n_rounds;
    for (int k = 0; k < n_rounds; ++k) {
        n_matches[k] = 0; n_accepted[k] = 0;
        for (int i = 0; i < n; ++i) match[(size_t)k * n + i] = -1;
        if (n > 0) memset(out + (size_t)k * n, 0, (size_t)n * sizeof(orbv_tri_out));
    }
    if (n_run == 0) return ORB_OK;
    MORB_HIP(hipSetDevice(w->device));
    // ---- every buffer of the call, before the first launch: a round's flags_b, constants, pinned match words and pinned records have
    //      slices of their own (the next round is enqueued while this one's are still to be read); the join's work area and the device
    //      match words are shared, stream order serialises the rounds
    const size_t state_bytes = morb::align16((size_t)n);
    int rc;
    if ((rc = morb::bow_chain_reserve(w, n, n_rounds, stage_bytes)) || (rc = w->h_tri.reserve((size_t)n_rounds * n * sizeof(orbv_tri_out))) ||
        (rc = w->tri_const.reserve((size_t)n_rounds * 2 * sizeof(TriKf))) || (rc = w->d_chain.reserve(2 * state_bytes))) return rc;
    if (flags_a) memcpy(w->h_stage.p, flags_a, (size_t)n);
    for (int k = 0; k < n_rounds; ++k) {
        if (!runs[k]) continue;
        if (rounds[k].flags_b) memcpy(w->h_stage.p + flags_off[k], rounds[k].flags_b, (size_t)rounds[k].b->D.n);
        TriKf K[2];
        fill_constants(&rounds[k].geometry.kf1, K[0]); fill_constants(&rounds[k].geometry.kf2, K[1]);
        memcpy(w->tri_const.p + (size_t)k * sizeof(K), K, sizeof(K));
    }
    w->tri_const.publish();
    // ---- the enqueue.  From the first launch on an error still waits for the stream: the kernels in flight hold the workspace's buffers
    int launches = 0;
    hipStream_t st = w->stream;
    auto fail = [&](int code) { (void)hipStreamSynchronize(st); return code; };
    if (stage_bytes) MORB_HIP(hipMemcpyAsync(w->d_stage.p, w->h_stage.p, stage_bytes, hipMemcpyHostToDevice, st));
    uint8_t* d_state = w->d_chain.p;
    uint8_t* d_flags = w->d_chain.p + state_bytes;
    const TriArrays F1 = arrays_of(a);
    hipLaunchKernelGGL(k_round_flags, dim3((n + 63) / 64), dim3(64), 0, st, flags_a ? (const uint8_t*)w->d_stage.p : a->D.flags, a->D.cam_of, n,
                       cam_bits_of(rounds[first].geometry.cam_enabled), d_state, d_flags);
    ++launches;
    for (int k = first; k < n_rounds; ++k) {
        if (!runs[k]) continue;
        const orbv_new_points_round& r = rounds[k];
        int next = k + 1;
        while (next < n_rounds && !runs[next]) ++next;
        const int32_t* d_match = nullptr;
        int l = 0;
        if ((rc = morb::bow_chain_enqueue(w, a, d_flags, r.b, r.flags_b ? w->d_stage.p + flags_off[k] : nullptr, &r.t, th_low, check_orientation, k,
                                          &d_match, &l))) return fail(rc);
        launches += l;
        hipLaunchKernelGGL(k_triangulate_round, dim3((n + 63) / 64), dim3(64), 0, st, (const TriKf*)w->tri_const.dp + 2 * k, F1, arrays_of(r.b), d_match, n,
                           cam_bits_of(r.geometry.cam_enabled), r.geometry.ratio_factor, (orbv_tri_out*)w->h_tri.dp + (size_t)k * n, d_state,
                           next < n_rounds ? d_flags : (uint8_t*)nullptr, next < n_rounds ? cam_bits_of(rounds[next].geometry.cam_enabled) : 0u);
        ++launches;
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    w->last_kf_call[1] = n_run; w->last_kf_call[2] = launches; w->last_kf_call[3] = 1;
    if (e != hipSuccess) { morb::set_error("the chained call failed: %s", hipGetErrorString(e)); return fail(ORB_E_HIP); }
    for (int k = 0; k < n_rounds; ++k) {
        if (!runs[k]) continue;
        morb::bow_search_collect(w, n, match + (size_t)k * n, &n_matches[k], k);
        orbv_tri_out* o = out + (size_t)k * n;
        memcpy(o, (const orbv_tri_out*)w->h_tri.p + (size_t)k * n, (size_t)n * sizeof(orbv_tri_out));
        int acc = 0;
        for (int i = 0; i < n; ++i) acc += o[i].outcome == ORBV_TRI_ACCEPTED;
        n_accepted[k] = acc;
    }
    return ORB_OK;
}

}  // extern "C"
