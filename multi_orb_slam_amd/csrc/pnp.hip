// pnp.hip -- every EPnP RANSAC hypothesis of a relocalisation's PnPsolvers in one call (include/orbm.h, "PnPsolver"): compute_pose and
// everything below it, CheckInliers and Refine (reference src/PnPsolver.cc:266-956) restated, with the OpenCV operators they call
// (cv_dev.h: cv_jacobi_svd_f64, cv_svd_backsubst_*; cvMulTransposed is the running sum of pnp_mtm_entry / the PW0 products).
//   pnp_compute_pose  ONE statement sequence for the host routine and both kernels.  It is written in phases: `par(count, f)` runs f for
//                     every output index -- each output is one running sum over the points in the reference's order, so the phases are
//                     parallel ACROSS outputs and never along a sum -- and `one(f)` runs the serial parts (the SVDs, the beta
//                     approximations, Gauss-Newton, the 3x3 of estimate_R_and_t, the final sum of the reprojection error).
//                     PnpSerial executes both as plain loops (host routine; one lane of k_pnp_hyp), PnpGroup spreads `par` over a
//                     workgroup and gives `one` to its first lane (k_pnp_refine).  The same expressions in the same order either way.
//   the work block    every matrix the routine addresses with run-time indices (the 12x12 MtM / Ut, L_6x10, the small SVDs' factors,
//                     Gauss-Newton's A and b ...) lies in one block of PNP_WS doubles behind a strided view (cv_vec): a stack array on
//                     the host, LDS on the device -- element-major, lane-minor in k_pnp_hyp, so that a lane's run-time index is an LDS
//                     address and nothing goes to scratch memory.
//   k_pnp_hyp         one lane per (problem, hypothesis), PNP_HYP_T lanes per workgroup (the block is 3 520 B per lane: 16 lanes fill
//                     55 KB of static LDS): gathers the quadruple, runs the four-point pnp_compute_pose, writes the record.
//   k_pnp_inliers     one wave per hypothesis, as k_sim3_inliers: coalesced structure-of-arrays reads, pnp_inlier through
//                     ransac_mask_sweep (ransac_dev.h) for the mask words and the count.  No atomics.
//   k_pnp_refine      one workgroup per (problem, record slot): scans the problem's counts for the strict prefix maxima, leaves when
//                     its slot is empty, else gathers the record's inlier set and runs the n-point pnp_compute_pose.
//                     The per-point arrays (alphas, pcs) live in the port's device block, which grows and is reused.
//   k_pnp_refine_inliers  one wave per (problem, record slot): CheckInliers with the refined pose, as k_pnp_inliers.  A kernel of its
//                     own so that nothing it needs stays live in scalar registers across the pose.
// The four kernels go onto the stream back to back: one enqueue, one synchronisation per call (ransac_csr_call, ransac_dev.h; the
// checks of a call: ransac_validate<4>, then the refined masks' table here).
// No libm function runs anywhere: + - * / sqrt fabs in double, CheckInliers' float steps, conversions.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/orbm.h"
#include "../../include/orb_debug.h"
#include "orb_common.h"
#include "matcher_internal.h"
#include "cv_dev.h"
#include "stage_pack.h"
#include "ransac_dev.h"

namespace {

constexpr int PNP_HYP_T = 16;    // hypotheses (lanes) of one k_pnp_hyp workgroup
constexpr int PNP_INL_T = 64;    // lanes of one k_pnp_inliers workgroup = one wave
constexpr int PNP_REF_T = 128;   // lanes of one k_pnp_refine workgroup = two waves

// the work block, in doubles
enum { WS_UT = 0,       // 144: MtM (transposed: it is symmetric), then Ut
       WS_W12 = 144,    // 12: the singular values of MtM
       WS_CWS = 156,    // 12: cws[4][3]
       WS_L = 168,      // 60: l_6x10
       WS_RHO = 228,    // 6
       WS_SA = 234,     // 30: At of a small SVD (3x3, 6x3, 6x4, 6x5)
       WS_SV = 264,     // 25: its Vt
       WS_SW = 289,     // 5: its singular values
       WS_TMP = 294,    // 48: pw0tpw0 / cc + cc_inv / dv / b3..b5 / Gauss-Newton's A b A1 A2 x / abt
       WS_CCS = 342,    // 12: ccs[4][3]
       WS_BET = 354,    // 4: the current betas
       WS_PC0 = 358, WS_PW0 = 361,
       WS_R = 364, WS_T = 373,      // R, t of the current approximation
       WS_RB = 376, WS_TB = 385,    // R, t of the best one so far
       WS_ERR = 388,                // [0] the current reprojection error, [1] the best
       PNP_WS = 392,
       // k_pnp_hyp only: the four points and their per-point arrays
       WS_PWS = 392, WS_US = 404, WS_ALPHAS = 412, WS_PCS = 428, PNP_WS4 = 440 };
enum { IW_FLAGS = 0, IW_CHOICE = 1, IW_NEG = 2, PNP_IW = 3 };

// ---- how the phases are executed ----------------------------------------------------------------------------------------------------------
struct PnpSerial {
    template <class F> __host__ __device__ __forceinline__ void par(int n, F f) const { for (int i = 0; i < n; ++i) f(i); }
    template <class F> __host__ __device__ __forceinline__ void one(F f) const { f(); }
};
struct PnpGroup {   // every lane of the workgroup calls every phase; what a phase leaves for the next lies in LDS or in the device block
    int tid;
    template <class F> __device__ __forceinline__ void par(int n, F f) const { for (int i = tid; i < n; i += PNP_REF_T) f(i); __syncthreads(); }
    template <class F> __device__ __forceinline__ void one(F f) const { if (tid == 0) f(); __syncthreads(); }
};

// ---- where the points come from -----------------------------------------------------------------------------------------------------------
// add_correspondence widens the floats of mvP3Dw / mvP2D to double: point i of the set is correspondence idx[i] of the problem
struct PnpGather {
    const float *p3, *p2;             // the problem's first correspondence: world x, image u
    int s3, c3, s2, c2;               // point stride and component stride: 3, 1 / 2, 1 for the caller's arrays; 1 and the distance between
                                      // the arrays for the structure of arrays
    const int32_t* idx;
    __host__ __device__ __forceinline__ double pw(int i, int j) const { return (double)p3[(size_t)idx[i] * s3 + (size_t)j * c3]; }
    __host__ __device__ __forceinline__ double us(int i, int j) const { return (double)p2[(size_t)idx[i] * s2 + (size_t)j * c2]; }
};
struct PnpDoubles {   // pws / us as compute_pose holds them (the test hook; the lane's copy in LDS)
    cv_vec pws, uv;
    __host__ __device__ __forceinline__ double pw(int i, int j) const { return pws[3 * i + j]; }
    __host__ __device__ __forceinline__ double us(int i, int j) const { return uv[2 * i + j]; }
};

__host__ __device__ __forceinline__ double pnp_dot3(cv_vec a, int ia, cv_vec b, int ib) { return a[ia] * b[ib] + a[ia + 1] * b[ib + 1] + a[ia + 2] * b[ib + 2]; }

// ---- qr_solve (:866-956), transcribed with its pointer walks as indices.  Returns 1 on the singular return (X untouched). ------------------
// Note the first loop: it starts at A[k][k] AGAIN and advances after the comparison, so row nr-1 is never looked at.
__host__ __device__ inline int pnp_qr_solve(cv_vec A, int nr, int nc, cv_vec b, cv_vec X, cv_vec A1, cv_vec A2) {
    int pkk = 0;
    for (int k = 0; k < nc; ++k) {
        int pik = pkk;
        double eta = fabs(A[pik]);
        for (int i = k + 1; i < nr; ++i) {
            const double elt = fabs(A[pik]);
            if (eta < elt) eta = elt;
            pik += nc;
        }
        if (eta == 0) { A1[k] = 0.0; A2[k] = 0.0; return 1; }
        pik = pkk;
        double sum = 0.0;
        const double inv_eta = 1. / eta;
        for (int i = k; i < nr; ++i) {
            const double a = A[pik] * inv_eta;
            A[pik] = a;
            sum += a * a;
            pik += nc;
        }
        double sigma = sqrt(sum);
        if (A[pkk] < 0) sigma = -sigma;
        const double akk = A[pkk] + sigma;
        A[pkk] = akk;
        A1[k] = sigma * akk;
        A2[k] = -eta * sigma;
        for (int j = k + 1; j < nc; ++j) {
            pik = pkk;
            double s = 0;
            for (int i = k; i < nr; ++i) { s += A[pik] * A[pik + j - k]; pik += nc; }
            const double tau = s / A1[k];
            pik = pkk;
            for (int i = k; i < nr; ++i) { A[pik + j - k] -= tau * A[pik]; pik += nc; }
        }
        pkk += nc + 1;
    }
    // b <- Qt b
    int pjj = 0;
    for (int j = 0; j < nc; ++j) {
        int pij = pjj;
        double tau = 0;
        for (int i = j; i < nr; ++i) { tau += A[pij] * b[i]; pij += nc; }
        tau /= A1[j];
        pij = pjj;
        for (int i = j; i < nr; ++i) { b[i] -= tau * A[pij]; pij += nc; }
        pjj += nc + 1;
    }
    // X = R-1 b
    X[nc - 1] = b[nc - 1] / A2[nc - 1];
    for (int i = nc - 2; i >= 0; --i) {
        int pij = i * nc + (i + 1);
        double sum = 0;
        for (int j = i + 1; j < nc; ++j) { sum += A[pij] * X[j]; ++pij; }
        X[i] = (b[i] - sum) / A2[i];
    }
    return 0;
}

// one element of M (fill_M, :442-457): row 2i (second == false) or 2i+1 of point i, column col
__host__ __device__ __forceinline__ double pnp_m_elem(bool second, int col, cv_vec alphas, int i, double fu, double fv, double ucu, double vcv) {
    const int q = col / 3, d = col - 3 * q;
    const double as = alphas[4 * i + q];
    if (!second) return d == 0 ? as * fu : d == 1 ? 0.0 : as * ucu;
    return d == 0 ? 0.0 : d == 1 ? as * fv : as * vcv;
}

// ---- compute_pose (:483-531) with everything it calls ------------------------------------------------------------------------------------
// ws: the work block; alphas 4n, pcs 3n; iw: PNP_IW ints (flags, choice, a sign) that every lane of the executing group can read.
// Leaves R, t in ws[WS_RB], ws[WS_TB], the reprojection error in ws[WS_ERR + 1], the choice and the flags in iw.
template <class E, class P>
__host__ __device__ __forceinline__ void pnp_compute_pose(const E& ex, const P& pts, int n, const double* K, cv_vec ws, cv_vec alphas,
                                                          cv_vec pcs, int* iw) {
    const double dn = (double)n;
    const cv_vec ut = ws.at(WS_UT), cws = ws.at(WS_CWS), L = ws.at(WS_L), rho = ws.at(WS_RHO), SA = ws.at(WS_SA), SV = ws.at(WS_SV), SW = ws.at(WS_SW),
                 tmp = ws.at(WS_TMP), ccs = ws.at(WS_CCS), betas = ws.at(WS_BET), pc0 = ws.at(WS_PC0), pw0 = ws.at(WS_PW0), R = ws.at(WS_R), T = ws.at(WS_T);
    ex.one([=] { iw[IW_FLAGS] = 0; iw[IW_CHOICE] = 0; iw[IW_NEG] = 0; });
    // choose_control_points (:381-415): the centroid ...
    ex.par(3, [=](int j) {
        double s = 0;
        for (int i = 0; i < n; ++i) s += pts.pw(i, j);
        cws[j] = s / dn;
    });
    // ... cvMulTransposed(PW0, PW0tPW0, 1): the upper triangle, each element one running sum over the rows, mirrored
    ex.par(6, [=](int e) {
        const int a = e < 3 ? 0 : e < 5 ? 1 : 2, b = e < 3 ? e : e < 5 ? e - 2 : 2;
        double s = 0;
        for (int i = 0; i < n; ++i) s += (pts.pw(i, a) - cws[a]) * (pts.pw(i, b) - cws[b]);
        tmp[3 * a + b] = s; tmp[3 * b + a] = s;
    });
    // ... cvSVD(PW0tPW0, DC, UCt, 0, MODIFY_A | U_T), the three other control points; then compute_barycentric_coordinates' cvInvert
    ex.one([=] {
        for (int i = 0; i < 3; ++i) for (int k = 0; k < 3; ++k) SA[3 * i + k] = tmp[3 * k + i];
        if (cv_jacobi_svd_f64(SA, 3, 3, SW, SV, false)) iw[IW_FLAGS] |= ORBM_PNP_FLAG_RANDOM_SVD;
        for (int i = 1; i < 4; ++i) {
            const double k = sqrt(SW[i - 1] / dn);
            for (int j = 0; j < 3; ++j) cws[3 * i + j] = cws[j] + k * SA[3 * (i - 1) + j];
        }
        for (int i = 0; i < 3; ++i) for (int j = 1; j < 4; ++j) tmp[3 * i + j - 1] = cws[3 * j + i] - cws[i];   // cc
        for (int i = 0; i < 3; ++i) for (int k = 0; k < 3; ++k) SA[3 * i + k] = tmp[3 * k + i];
        if (cv_jacobi_svd_f64(SA, 3, 3, SW, SV, true)) iw[IW_FLAGS] |= ORBM_PNP_FLAG_RANDOM_SVD;
        cv_svd_backsubst_inv(SA, 3, SW, SV, tmp.at(9));                                                        // cc_inv
    });
    ex.par(n, [=](int i) {
        const cv_vec ci = tmp.at(9);
        const double d0 = pts.pw(i, 0) - cws[0], d1 = pts.pw(i, 1) - cws[1], d2 = pts.pw(i, 2) - cws[2];
        double a[3];
        for (int j = 0; j < 3; ++j) a[j] = ci[3 * j] * d0 + ci[3 * j + 1] * d1 + ci[3 * j + 2] * d2;
        alphas[4 * i + 1] = a[0]; alphas[4 * i + 2] = a[1]; alphas[4 * i + 3] = a[2];
        alphas[4 * i] = 1.0 - a[0] - a[1] - a[2];
    });
    // cvMulTransposed(M, MtM, 1) over the 2n rows of fill_M: 78 elements, each one running sum; the mirror; the transpose cvSVD works on
    ex.par(78, [=](int e) {
        const double fu = K[0], fv = K[1], uc = K[2], vc = K[3];
        int r = 0, c = e;
        while (c >= 12 - r) { c -= 12 - r; ++r; }
        c += r;
        double s = 0;
        for (int i = 0; i < n; ++i) {
            const double ucu = uc - pts.us(i, 0), vcv = vc - pts.us(i, 1);
            s += pnp_m_elem(false, r, alphas, i, fu, fv, ucu, vcv) * pnp_m_elem(false, c, alphas, i, fu, fv, ucu, vcv);
            s += pnp_m_elem(true, r, alphas, i, fu, fv, ucu, vcv) * pnp_m_elem(true, c, alphas, i, fu, fv, ucu, vcv);
        }
        ut[12 * r + c] = s; ut[12 * c + r] = s;
    });
    ex.one([=] {
        if (cv_jacobi_svd_f64(ut, 12, 12, ws.at(WS_W12), SV, false)) iw[IW_FLAGS] |= ORBM_PNP_FLAG_RANDOM_SVD;
        // compute_L_6x10 (:766-806): dv[i][j] of the four null vectors v[i] = ut + 12*(11 - i), row by row
        int a = 0, b = 1;
        for (int j = 0; j < 6; ++j) {
            for (int i = 0; i < 4; ++i) {
                const int v = 12 * (11 - i);
                for (int d = 0; d < 3; ++d) tmp[3 * i + d] = ut[v + 3 * a + d] - ut[v + 3 * b + d];
            }
            L[10 * j + 0] = pnp_dot3(tmp, 0, tmp, 0);
            L[10 * j + 1] = 2.0 * pnp_dot3(tmp, 0, tmp, 3);
            L[10 * j + 2] = pnp_dot3(tmp, 3, tmp, 3);
            L[10 * j + 3] = 2.0 * pnp_dot3(tmp, 0, tmp, 6);
            L[10 * j + 4] = 2.0 * pnp_dot3(tmp, 3, tmp, 6);
            L[10 * j + 5] = pnp_dot3(tmp, 6, tmp, 6);
            L[10 * j + 6] = 2.0 * pnp_dot3(tmp, 0, tmp, 9);
            L[10 * j + 7] = 2.0 * pnp_dot3(tmp, 3, tmp, 9);
            L[10 * j + 8] = 2.0 * pnp_dot3(tmp, 6, tmp, 9);
            L[10 * j + 9] = pnp_dot3(tmp, 9, tmp, 9);
            // compute_rho (:808-816): dist2 of the same pair of control points
            const double e0 = cws[3 * a] - cws[3 * b], e1 = cws[3 * a + 1] - cws[3 * b + 1], e2 = cws[3 * a + 2] - cws[3 * b + 2];
            rho[j] = e0 * e0 + e1 * e1 + e2 * e2;
            ++b;
            if (b > 3) { ++a; b = a + 1; }
        }
    });
    for (int approx = 1; approx <= 3; ++approx) {
        ex.one([=] {
            // find_betas_approx_1/2/3 (:673-764): the columns {0 1 3 6}, {0 1 2}, {0 1 2 3 4} of L_6x10, cvSolve(., Rho, ., CV_SVD)
            const int nc = approx == 1 ? 4 : approx == 2 ? 3 : 5;
            for (int c = 0; c < nc; ++c) {
                const int col = approx == 1 ? (c == 0 ? 0 : c == 1 ? 1 : c == 2 ? 3 : 6) : c;
                for (int i = 0; i < 6; ++i) SA[6 * c + i] = L[10 * i + col];
            }
            if (cv_jacobi_svd_f64(SA, 6, nc, SW, SV, true)) iw[IW_FLAGS] |= ORBM_PNP_FLAG_RANDOM_SVD;
            const cv_vec bb = tmp;
            cv_svd_backsubst_vec(SA, 6, nc, SW, SV, rho, bb);
            if (approx == 1) {
                if (bb[0] < 0) {
                    betas[0] = sqrt(-bb[0]);
                    betas[1] = -bb[1] / betas[0];
                    betas[2] = -bb[2] / betas[0];
                    betas[3] = -bb[3] / betas[0];
                } else {
                    betas[0] = sqrt(bb[0]);
                    betas[1] = bb[1] / betas[0];
                    betas[2] = bb[2] / betas[0];
                    betas[3] = bb[3] / betas[0];
                }
            } else {
                if (bb[0] < 0) {
                    betas[0] = sqrt(-bb[0]);
                    betas[1] = (bb[2] < 0) ? sqrt(-bb[2]) : 0.0;
                } else {
                    betas[0] = sqrt(bb[0]);
                    betas[1] = (bb[2] > 0) ? sqrt(bb[2]) : 0.0;
                }
                if (bb[1] < 0) betas[0] = -betas[0];
                betas[2] = approx == 3 ? bb[3] / betas[0] : 0.0;
                betas[3] = 0.0;
            }
            // gauss_newton (:846-864): x starts as zeros HERE (the reference's is uninitialised) and a singular qr_solve leaves it
            const cv_vec A = tmp, b = tmp.at(24), A1 = tmp.at(30), A2 = tmp.at(34), x = tmp.at(40);
            for (int i = 0; i < 4; ++i) x[i] = 0.0;
            for (int k = 0; k < 5; ++k) {
                const double b0 = betas[0], b1 = betas[1], b2 = betas[2], b3 = betas[3];
                for (int i = 0; i < 6; ++i) {                                   // compute_A_and_b_gauss_newton (:818-844)
                    const cv_vec rowL = L.at(10 * i);
                    A[4 * i + 0] = 2 * rowL[0] * b0 + rowL[1] * b1 + rowL[3] * b2 + rowL[6] * b3;
                    A[4 * i + 1] = rowL[1] * b0 + 2 * rowL[2] * b1 + rowL[4] * b2 + rowL[7] * b3;
                    A[4 * i + 2] = rowL[3] * b0 + rowL[4] * b1 + 2 * rowL[5] * b2 + rowL[8] * b3;
                    A[4 * i + 3] = rowL[6] * b0 + rowL[7] * b1 + rowL[8] * b2 + 2 * rowL[9] * b3;
                    b[i] = rho[i] - (rowL[0] * b0 * b0 + rowL[1] * b0 * b1 + rowL[2] * b1 * b1 + rowL[3] * b0 * b2 + rowL[4] * b1 * b2 +
                                     rowL[5] * b2 * b2 + rowL[6] * b0 * b3 + rowL[7] * b1 * b3 + rowL[8] * b2 * b3 + rowL[9] * b3 * b3);
                }
                if (pnp_qr_solve(A, 6, 4, b, x, A1, A2)) iw[IW_FLAGS] |= ORBM_PNP_FLAG_SINGULAR_QR;
                for (int i = 0; i < 4; ++i) betas[i] += x[i];
            }
            // compute_ccs (:459-470)
            for (int k = 0; k < 12; ++k) ccs[k] = 0.0;
            for (int i = 0; i < 4; ++i) {
                const int v = 12 * (11 - i);
                for (int k = 0; k < 12; ++k) ccs[k] += betas[i] * ut[v + k];
            }
        });
        // compute_pcs (:472-481)
        ex.par(n, [=](int i) {
            for (int j = 0; j < 3; ++j)
                pcs[3 * i + j] = alphas[4 * i] * ccs[j] + alphas[4 * i + 1] * ccs[3 + j] + alphas[4 * i + 2] * ccs[6 + j] + alphas[4 * i + 3] * ccs[9 + j];
        });
        // solve_for_sign (:642-655) reads pcs[2] alone
        ex.one([=] {
            iw[IW_NEG] = pcs[2] < 0.0 ? 1 : 0;
            if (iw[IW_NEG]) for (int k = 0; k < 12; ++k) ccs[k] = -ccs[k];
        });
        ex.par(n, [=](int i) {
            if (iw[IW_NEG]) for (int j = 0; j < 3; ++j) pcs[3 * i + j] = -pcs[3 * i + j];
        });
        // estimate_R_and_t (:575-633): the two centroids, ABt, its SVD
        ex.par(6, [=](int j) {
            double s = 0;
            if (j < 3) { for (int i = 0; i < n; ++i) s += pcs[3 * i + j]; pc0[j] = s / dn; }
            else { for (int i = 0; i < n; ++i) s += pts.pw(i, j - 3); pw0[j - 3] = s / dn; }
        });
        ex.par(9, [=](int e) {
            const int j = e / 3, c = e - 3 * j;
            double s = 0;
            for (int i = 0; i < n; ++i) s += (pcs[3 * i + j] - pc0[j]) * (pts.pw(i, c) - pw0[c]);
            tmp[e] = s;
        });
        ex.one([=] {
            for (int i = 0; i < 3; ++i) for (int k = 0; k < 3; ++k) SA[3 * i + k] = tmp[3 * k + i];
            if (cv_jacobi_svd_f64(SA, 3, 3, SW, SV, true)) iw[IW_FLAGS] |= ORBM_PNP_FLAG_RANDOM_SVD;
            // abt_u[3i + k] = U[i][k] = SA[3k + i], abt_v[3j + k] = V[j][k] = SV[3k + j]
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) R[3 * i + j] = SA[i] * SV[j] + SA[3 + i] * SV[3 + j] + SA[6 + i] * SV[6 + j];
            const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
            if (det < 0) { R[6] = -R[6]; R[7] = -R[7]; R[8] = -R[8]; }
            for (int i = 0; i < 3; ++i) T[i] = pc0[i] - pnp_dot3(R, 3 * i, pw0, 0);
        });
        // reprojection_error (:556-573): the terms (into pcs, which nothing reads any more), then their sum in point order
        ex.par(n, [=](int i) {
            const double fu = K[0], fv = K[1], uc = K[2], vc = K[3];
            const double p0 = pts.pw(i, 0), p1 = pts.pw(i, 1), p2 = pts.pw(i, 2);
            const double Xc = (R[0] * p0 + R[1] * p1 + R[2] * p2) + T[0];
            const double Yc = (R[3] * p0 + R[4] * p1 + R[5] * p2) + T[1];
            const double inv_Zc = 1.0 / ((R[6] * p0 + R[7] * p1 + R[8] * p2) + T[2]);
            const double ue = uc + fu * Xc * inv_Zc;
            const double ve = vc + fv * Yc * inv_Zc;
            const double u = pts.us(i, 0), v = pts.us(i, 1);
            pcs[3 * i] = sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
        });
        ex.one([=] {
            double sum2 = 0.0;
            for (int i = 0; i < n; ++i) sum2 += pcs[3 * i];
            const double err = sum2 / dn;
            ws[WS_ERR] = err;
            // `N = 1; if (rep_errors[2] < rep_errors[1]) N = 2; if (rep_errors[3] < rep_errors[N]) N = 3;`
            if (approx == 1 || err < ws[WS_ERR + 1]) {
                ws[WS_ERR + 1] = err;
                iw[IW_CHOICE] = approx;
                for (int k = 0; k < 9; ++k) ws[WS_RB + k] = R[k];
                for (int k = 0; k < 3; ++k) ws[WS_TB + k] = T[k];
            }
        });
    }
}

// ---- CheckInliers (:314-345) for one correspondence: Xc, Yc, invZc double sums rounded to float, ue / ve double, the rest float ----------
__host__ __device__ __forceinline__ bool pnp_inlier(const double* R, const double* t, double fu, double fv, double uc, double vc, float X, float Y, float Z,
                                                    float u, float v, float max_err) {
    const float Xc = (float)(R[0] * (double)X + R[1] * (double)Y + R[2] * (double)Z + t[0]);
    const float Yc = (float)(R[3] * (double)X + R[4] * (double)Y + R[5] * (double)Z + t[1]);
    const float invZc = (float)(1 / (R[6] * (double)X + R[7] * (double)Y + R[8] * (double)Z + t[2]));
    const double ue = uc + fu * (double)Xc * (double)invZc;
    const double ve = vc + fv * (double)Yc * (double)invZc;
    const float distX = (float)((double)u - ue);
    const float distY = (float)((double)v - ve);
    const float error2 = distX * distX + distY * distY;
    return error2 < max_err;
}

// ---- the kernels ------------------------------------------------------------------------------------------------------------------------
struct PnpDev {
    const orbm_pnp_problem* prob;      // per problem
    const int32_t* first;              // CSR of the correspondences, per problem + 1
    const int32_t* its_first;          // CSR of the hypotheses, per problem + 1
    const int32_t* mask_first;         // first mask word of every problem
    const int32_t* rmask_first;        // first word of every problem's refined masks
    const int32_t* pp_first;           // first point of every problem's ORBM_PNP_MAX_RECORDS per-point blocks, -1: the host takes the problem
    const int32_t* hyp_prob;           // per hypothesis: its problem, or -1 when the host routine takes that problem
    const int32_t* quads;              // per hypothesis: four positions inside the problem
    const float *x, *y, *z, *u, *v, *e;   // structure of arrays
    int soa_stride;                    // floats between consecutive arrays of it (y = x + soa_stride, ...; v = u + soa_stride)
    int n_hyp;
    orbm_pnp_hyp* rec_dev;             // HBM: read by k_pnp_inliers
    int32_t* cnt_dev;                  // HBM: the counts, read by k_pnp_refine
    uint64_t* mask_dev;                // HBM: the mask words, read by k_pnp_refine
    int32_t* idx_dev;                  // HBM: the inlier sets of the records
    double* pp_dev;                    // HBM: alphas (4) and pcs (3) of every point of every record
    orbm_pnp_refined* ref_dev;         // HBM: the refined records, read by k_pnp_refine_inliers (hyp = -1: an empty slot)
    orbm_pnp_hyp* rec_out;             // mapped pinned
    uint64_t* mask_out;                // mapped pinned
    orbm_pnp_refined* ref_out;         // mapped pinned
    uint64_t* rmask_out;               // mapped pinned
};

__global__ __launch_bounds__(PNP_HYP_T) void k_pnp_hyp(PnpDev A) {
    __shared__ double lds[PNP_WS4 * PNP_HYP_T];
    const int g = blockIdx.x * PNP_HYP_T + threadIdx.x;
    if (g >= A.n_hyp) return;                          // (no barrier in this kernel)
    const int b = A.hyp_prob[g];
    if (b < 0) return;
    const cv_vec ws = {lds + threadIdx.x, PNP_HYP_T};
    const int n0 = A.first[b];
    for (int i = 0; i < 4; ++i) {
        const int c = n0 + A.quads[4 * (size_t)g + i];   // (validated on the host: inside the problem)
        ws[WS_PWS + 3 * i] = (double)A.x[c]; ws[WS_PWS + 3 * i + 1] = (double)A.y[c]; ws[WS_PWS + 3 * i + 2] = (double)A.z[c];
        ws[WS_US + 2 * i] = (double)A.u[c]; ws[WS_US + 2 * i + 1] = (double)A.v[c];
    }
    const PnpDoubles pts = {ws.at(WS_PWS), ws.at(WS_US)};
    const orbm_pnp_problem& P = A.prob[b];
    int iw[PNP_IW];
    pnp_compute_pose(PnpSerial(), pts, 4, &P.fu, ws, ws.at(WS_ALPHAS), ws.at(WS_PCS), iw);
    orbm_pnp_hyp o;
    for (int k = 0; k < 9; ++k) o.R[k] = x86_nan(ws[WS_RB + k]);
    for (int k = 0; k < 3; ++k) o.t[k] = x86_nan(ws[WS_TB + k]);
    o.rep_error = x86_nan(ws[WS_ERR + 1]);
    o.choice = iw[IW_CHOICE]; o.n_inliers = 0; o.flags = iw[IW_FLAGS]; o.reserved = 0;
    A.rec_dev[g] = o;
    A.rec_out[g] = o;
}

__global__ __launch_bounds__(PNP_INL_T) void k_pnp_inliers(PnpDev A) {
    const int g = blockIdx.x;
    const int lane = threadIdx.x;
    const int b = A.hyp_prob[g];
    if (b < 0) return;
    const orbm_pnp_problem P = A.prob[b];
    const int n0 = A.first[b];
    const int n = A.first[b + 1] - n0;
    const orbm_pnp_hyp& rec = A.rec_dev[g];
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = rec.R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = rec.t[k];
    const size_t w0 = (size_t)A.mask_first[b] + (size_t)(g - A.its_first[b]) * ransac_words(n);
    const int count = ransac_mask_sweep(n, lane,
        [&](int i) { const int k = n0 + i; return pnp_inlier(R, t, P.fu, P.fv, P.uc, P.vc, A.x[k], A.y[k], A.z[k], A.u[k], A.v[k], A.e[k]); },
        [&](int c, unsigned long long word) { A.mask_out[w0 + c] = word; A.mask_dev[w0 + c] = word; });
    if (lane == 0) { A.rec_out[g].n_inliers = count; A.cnt_dev[g] = count; }
}

__global__ __launch_bounds__(PNP_REF_T) void k_pnp_refine(PnpDev A) {
    __shared__ double lds[PNP_WS];
    __shared__ int iw[PNP_IW + 2];        // + {the record's hypothesis, its set size}
    __shared__ int woff[ORBM_PNP_CAP / 64 + 1];
    const int b = blockIdx.x / ORBM_PNP_MAX_RECORDS, slot = blockIdx.x - b * ORBM_PNP_MAX_RECORDS;
    const int tid = threadIdx.x;
    orbm_pnp_refined* const rec = A.ref_dev + (size_t)b * ORBM_PNP_MAX_RECORDS + slot;
    if (A.pp_first[b] < 0) { if (tid == 0) rec->hyp = -1; return; }   // (uniform: the host takes the problem)
    const int n0 = A.first[b], N = A.first[b + 1] - n0, h0 = A.its_first[b], H = A.its_first[b + 1] - h0;
    const int W = ransac_words(N);
    // the strict prefix maxima above best_start among the counts >= min_inliers: record number `slot` is this workgroup's
    if (tid == 0) {
        const int min_inliers = A.prob[b].min_inliers;
        int best = A.prob[b].best_start, nrec = 0, hyp = -1, nset = 0;
        for (int h = 0; h < H && hyp < 0; ++h) {
            const int c = A.cnt_dev[h0 + h];
            if (c >= min_inliers && c > best) {
                best = c;
                if (nrec == slot) { hyp = h; nset = c; }
                ++nrec;
            }
        }
        iw[PNP_IW] = hyp; iw[PNP_IW + 1] = nset;
    }
    __syncthreads();
    const int hyp = iw[PNP_IW], n = iw[PNP_IW + 1];
    if (hyp < 0) { if (tid == 0) rec->hyp = -1; return; }   // (uniform: the slot is empty)
    // the record's inlier set, in ascending position
    const uint64_t* words = A.mask_dev + (size_t)A.mask_first[b] + (size_t)hyp * W;
    if (tid == 0) {
        int o = 0;
        for (int c = 0; c < W; ++c) { woff[c] = o; o += __popcll(words[c]); }
    }
    __syncthreads();
    const size_t p0 = (size_t)A.pp_first[b] + (size_t)slot * N;
    int32_t* idx = A.idx_dev + p0;
    for (int c = tid; c < W; c += PNP_REF_T) {
        unsigned long long word = words[c];
        int o = woff[c];
        while (word) {
            const int bit = __ffsll((long long)word) - 1;
            idx[o++] = c * 64 + bit;
            word &= word - 1;
        }
    }
    __syncthreads();
    const PnpGather pts = {A.x + n0, A.u + n0, 1, A.soa_stride, 1, A.soa_stride, idx};
    const cv_vec ws = {lds, 1}, alphas = {A.pp_dev + p0 * 7, 1}, pcs = {A.pp_dev + p0 * 7 + (size_t)N * 4, 1};
    const PnpGroup ex = {tid};
    pnp_compute_pose(ex, pts, n, &A.prob[b].fu, ws, alphas, pcs, iw);
    // the record, without its count, to HBM: k_pnp_refine_inliers reads the pose there, adds the count and hands the record to the host
    if (tid == 0) {
        orbm_pnp_refined o;
        o.hyp = hyp; o.n_set = n; o.n_inliers = 0; o.flags = iw[IW_FLAGS];
        for (int k = 0; k < 9; ++k) o.R[k] = x86_nan(lds[WS_RB + k]);
        for (int k = 0; k < 3; ++k) o.t[k] = x86_nan(lds[WS_TB + k]);
        *rec = o;
    }
}

// CheckInliers with a refined pose: one wave per (problem, record slot), as k_pnp_inliers
__global__ __launch_bounds__(PNP_INL_T) void k_pnp_refine_inliers(PnpDev A) {
    const int b = blockIdx.x / ORBM_PNP_MAX_RECORDS, slot = blockIdx.x - b * ORBM_PNP_MAX_RECORDS;
    const int lane = threadIdx.x;
    const orbm_pnp_refined& rec = A.ref_dev[(size_t)b * ORBM_PNP_MAX_RECORDS + slot];
    if (rec.hyp < 0) return;
    const orbm_pnp_problem P = A.prob[b];
    const int n0 = A.first[b], N = A.first[b + 1] - n0;
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = rec.R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = rec.t[k];
    uint64_t* rwords = A.rmask_out + (size_t)A.rmask_first[b] + (size_t)slot * ransac_words(N);
    const int count = ransac_mask_sweep(N, lane,
        [&](int i) { const int k = n0 + i; return pnp_inlier(R, t, P.fu, P.fv, P.uc, P.vc, A.x[k], A.y[k], A.z[k], A.u[k], A.v[k], A.e[k]); },
        [&](int c, unsigned long long word) { rwords[c] = word; });
    if (lane == 0) {
        orbm_pnp_refined* out = A.ref_out + (size_t)b * ORBM_PNP_MAX_RECORDS + slot;
        out->hyp = rec.hyp; out->n_set = rec.n_set; out->n_inliers = count; out->flags = rec.flags;
#pragma unroll
        for (int k = 0; k < 9; ++k) out->R[k] = R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) out->t[k] = t[k];
    }
}

// ---- host routine -----------------------------------------------------------------------------------------------------------------------
struct PnpIn {
    const orbm_pnp_problem* problems; const int32_t* first; const float* p3dw; const float* p2d; const float* max_err;
    const int32_t* its_first; const int32_t* quads;
};

void pnp_check_inliers_host(const PnpIn& I, int b, const double* R, const double* t, uint64_t* words, int* count_out) {
    const orbm_pnp_problem& P = I.problems[b];
    const int n0 = I.first[b], n = I.first[b + 1] - n0;
    *count_out = ransac_mask_sweep_host(n, words, [&](int i) {
        const size_t k = (size_t)n0 + i;
        return pnp_inlier(R, t, P.fu, P.fv, P.uc, P.vc, I.p3dw[3 * k], I.p3dw[3 * k + 1], I.p3dw[3 * k + 2], I.p2d[2 * k], I.p2d[2 * k + 1], I.max_err[k]);
    });
}

// compute_pose on the points idx[0 .. n-1] of problem b
void pnp_pose_host(const PnpIn& I, int b, const int32_t* idx, int n, std::vector<double>& pp, double* R, double* t, double* err, int* choice, int* flags) {
    const orbm_pnp_problem& P = I.problems[b];
    const size_t n0 = (size_t)I.first[b];
    const PnpGather pts = {I.p3dw + 3 * n0, I.p2d + 2 * n0, 3, 1, 2, 1, idx};
    double wsd[PNP_WS];
    int iw[PNP_IW];
    if (pp.size() < (size_t)n * 7 + 1) pp.resize((size_t)n * 7 + 1);
    const cv_vec ws = {wsd, 1}, alphas = {pp.data(), 1}, pcs = {pp.data() + (size_t)n * 4, 1};
    pnp_compute_pose(PnpSerial(), pts, n, &P.fu, ws, alphas, pcs, iw);
    for (int k = 0; k < 9; ++k) R[k] = x86_nan(wsd[WS_RB + k]);
    for (int k = 0; k < 3; ++k) t[k] = x86_nan(wsd[WS_TB + k]);
    *err = x86_nan(wsd[WS_ERR + 1]);
    *choice = iw[IW_CHOICE]; *flags = iw[IW_FLAGS];
}

// the hypotheses of one problem: records hyp[0 .. H-1] and mask words[0 .. H*W-1]
void pnp_hyps_host(const PnpIn& I, int b, orbm_pnp_hyp* hyp, uint64_t* words) {
    const int n = I.first[b + 1] - I.first[b], h0 = I.its_first[b], H = I.its_first[b + 1] - h0, W = ransac_words(n);
    std::vector<double> pp;
    for (int h = 0; h < H; ++h) {
        orbm_pnp_hyp& o = hyp[h];
        pnp_pose_host(I, b, I.quads + 4 * (size_t)(h0 + h), 4, pp, o.R, o.t, &o.rep_error, &o.choice, &o.flags);
        o.reserved = 0;
        pnp_check_inliers_host(I, b, o.R, o.t, words + (size_t)h * W, &o.n_inliers);
    }
}

// the records of one problem out of its counts: the hypotheses `iterate` makes its best, in order
void pnp_records(const orbm_pnp_problem& P, const orbm_pnp_hyp* hyp, int H, std::vector<int>& rec) {
    rec.clear();
    int best = P.best_start;
    for (int h = 0; h < H; ++h)
        if (hyp[h].n_inliers >= P.min_inliers && hyp[h].n_inliers > best) { best = hyp[h].n_inliers; rec.push_back(h); }
}

// Refine() on hypothesis h of problem b (its mask in hwords)
void pnp_refine_host(const PnpIn& I, int b, int h, const uint64_t* hwords, std::vector<double>& pp, std::vector<int32_t>& idx, orbm_pnp_refined* out, uint64_t* rwords) {
    const int n = I.first[b + 1] - I.first[b], W = ransac_words(n);
    idx.clear();
    for (int c = 0; c < W; ++c)
        for (int l = 0; l < 64; ++l) if (hwords[c] >> l & 1) idx.push_back(c * 64 + l);
    double err;
    int choice;
    out->hyp = h; out->n_set = (int)idx.size();
    pnp_pose_host(I, b, idx.data(), (int)idx.size(), pp, out->R, out->t, &err, &choice, &out->flags);
    pnp_check_inliers_host(I, b, out->R, out->t, rwords, &out->n_inliers);
}

// Argument checks; mask_first[b] = the first mask word of problem b, rmask_first[b] = the first word of its refined masks.
int validate(const PnpIn& I, int B, const orbm_pnp_hyp* hyp_out, const uint64_t* mask_out, const int32_t* n_records_out, const orbm_pnp_refined* refined_out,
             const uint64_t* refined_mask_out, int extra_cap, std::vector<int32_t>& mask_first, std::vector<int32_t>& rmask_first) {
    MORB_ARG(I.problems && n_records_out && refined_out && extra_cap >= 0);
    if (const int rc = ransac_validate<4>(B, ORBM_PNP_MAX_BATCH, ORBM_PNP_MAX_ITS, I.first, I.its_first, I.quads, hyp_out, mask_out, mask_first)) return rc;
    if (I.first[B] > 0 && !(I.p3dw && I.p2d && I.max_err)) { morb::set_error("a correspondence array is NULL"); return ORB_E_ARG; }
    rmask_first.assign((size_t)B + 1, 0);
    long long rwords = 0;
    for (int b = 0; b < B; ++b) {
        rwords += (long long)ORBM_PNP_MAX_RECORDS * ransac_words(I.first[b + 1] - I.first[b]);
        if (rwords > INT_MAX) { morb::set_error("the refined masks of the call exceed 2^31 words"); return ORB_E_CAPACITY; }
        rmask_first[(size_t)b + 1] = (int32_t)rwords;
    }
    if (rwords > 0 && !refined_mask_out) { morb::set_error("refined_mask_out is NULL"); return ORB_E_ARG; }
    return ORB_OK;
}

// What follows the hypotheses, on the host: n_records_out, the zeroed slots, the records in `host_from[b] ..` refined here (0: all of a
// host problem's; ORBM_PNP_MAX_RECORDS: the tail of a device problem's), the extras appended.  Returns the records refined here in *n_host.
int pnp_finish_host(const PnpIn& I, int B, const int* host_from, const std::vector<int32_t>& mask_first, const std::vector<int32_t>& rmask_first,
                    const orbm_pnp_hyp* hyp_out, const uint64_t* mask_out, int32_t* n_records_out, orbm_pnp_refined* refined_out, uint64_t* refined_mask_out,
                    int extra_cap, int* n_host) {
    std::vector<std::vector<int>> recs((size_t)B);
    long long extras = 0;
    for (int b = 0; b < B; ++b) {
        pnp_records(I.problems[b], hyp_out + I.its_first[b], I.its_first[b + 1] - I.its_first[b], recs[b]);
        n_records_out[b] = (int32_t)recs[b].size();
        extras += std::max(0, (int)recs[b].size() - (int)ORBM_PNP_MAX_RECORDS);
    }
    if (extras > extra_cap) { morb::set_error("%lld records lie beyond ORBM_PNP_MAX_RECORDS, extra_cap = %d", extras, extra_cap); return ORB_E_CAPACITY; }
    std::vector<double> pp;
    std::vector<int32_t> idx;
    size_t xr = (size_t)B * ORBM_PNP_MAX_RECORDS, xw = (size_t)rmask_first[B];
    *n_host = 0;
    for (int b = 0; b < B; ++b) {
        const int W = ransac_words(I.first[b + 1] - I.first[b]), nr = (int)recs[b].size();
        for (int r = 0; r < std::max(nr, (int)ORBM_PNP_MAX_RECORDS); ++r) {
            const bool extra = r >= ORBM_PNP_MAX_RECORDS;
            orbm_pnp_refined* out = extra ? refined_out + xr : refined_out + (size_t)b * ORBM_PNP_MAX_RECORDS + r;
            uint64_t* rw = extra ? refined_mask_out + xw : refined_mask_out + (size_t)rmask_first[b] + (size_t)r * W;
            if (extra) { ++xr; xw += (size_t)W; }
            if (r >= nr) { memset(out, 0, sizeof(*out)); if (W) memset(rw, 0, (size_t)W * 8); continue; }
            if (r < host_from[b]) continue;            // the device refined it
            pnp_refine_host(I, b, recs[b][r], mask_out + (size_t)mask_first[b] + (size_t)recs[b][r] * W, pp, idx, out, rw);
            ++*n_host;
        }
    }
    return ORB_OK;
}

}  // namespace

extern "C" {

int orbm_pnp_ransac_host(const orbm_pnp_problem* problems, int B, const int32_t* first, const float* p3dw, const float* p2d,
                         const float* max_err, const int32_t* its_first, const int32_t* quads, orbm_pnp_hyp* hyp_out, uint64_t* mask_out,
                         int32_t* n_records_out, orbm_pnp_refined* refined_out, uint64_t* refined_mask_out, int extra_cap) {
    const PnpIn I = {problems, first, p3dw, p2d, max_err, its_first, quads};
    std::vector<int32_t> mask_first, rmask_first;
    int rc = validate(I, B, hyp_out, mask_out, n_records_out, refined_out, refined_mask_out, extra_cap, mask_first, rmask_first);
    if (rc) return rc;
    for (int b = 0; b < B; ++b) pnp_hyps_host(I, b, hyp_out + its_first[b], mask_out + mask_first[b]);
    int host_from[ORBM_PNP_MAX_BATCH] = {0}, n_host = 0;
    return pnp_finish_host(I, B, host_from, mask_first, rmask_first, hyp_out, mask_out, n_records_out, refined_out, refined_mask_out, extra_cap, &n_host);
}

int orbm_pnp_ransac(orbm_matcher* m, const orbm_pnp_problem* problems, int B, const int32_t* first, const float* p3dw, const float* p2d,
                    const float* max_err, const int32_t* its_first, const int32_t* quads, orbm_pnp_hyp* hyp_out, uint64_t* mask_out,
                    int32_t* n_records_out, orbm_pnp_refined* refined_out, uint64_t* refined_mask_out, int extra_cap) {
    MORB_ARG(m != nullptr);
    const PnpIn I = {problems, first, p3dw, p2d, max_err, its_first, quads};
    std::vector<int32_t> mask_first, rmask_first;
    int rc = validate(I, B, hyp_out, mask_out, n_records_out, refined_out, refined_mask_out, extra_cap, mask_first, rmask_first);
    if (rc) return rc;
    const int N = first[B], HT = its_first[B];
    // the device refines the records of the problems it runs hypotheses for: those with hypotheses and at most ORBM_PNP_CAP correspondences
    std::vector<int32_t> pp_first((size_t)B, -1);
    int host_from[ORBM_PNP_MAX_BATCH] = {0};
    long long pp_points = 0;
    for (int b = 0; b < B; ++b) {
        const int n = first[b + 1] - first[b];
        if (n > ORBM_PNP_CAP || its_first[b + 1] == its_first[b]) continue;   // without hypotheses pp_first stays -1 and the host zeroes the slots
        host_from[b] = ORBM_PNP_MAX_RECORDS;
        pp_first[b] = (int32_t)pp_points;
        pp_points += (long long)ORBM_PNP_MAX_RECORDS * n;
        if (pp_points > INT_MAX) { morb::set_error("the per-point blocks of the call exceed 2^31 points"); return ORB_E_CAPACITY; }
    }
    size_t o_ref = 0, o_rmask = 0;
    int split[2] = {0, 0}, n_rec_dev = 0;
    std::vector<int> rec;
    rc = ransac_csr_call(m, m->pnp, B, first, its_first, mask_first, ORBM_PNP_CAP, hyp_out, mask_out, split,
        [&](const std::vector<int32_t>& hyp_prob, size_t* o_mask) -> int {
            morb::StagePack pk;
            const int i_prob = pk.add(problems, (size_t)B * sizeof(orbm_pnp_problem)), i_first = pk.add(first, (size_t)(B + 1) * 4),
                      i_its = pk.add(its_first, (size_t)(B + 1) * 4), i_mf = pk.add(mask_first.data(), (size_t)(B + 1) * 4),
                      i_rmf = pk.add(rmask_first.data(), (size_t)(B + 1) * 4), i_ppf = pk.add(pp_first.data(), (size_t)B * 4),
                      i_hp = pk.add(hyp_prob.data(), (size_t)HT * 4), i_quads = pk.add(quads, (size_t)HT * 16);
            int i_soa[6];                                      // x y z u v e, transposed below
            for (int k = 0; k < 6; ++k) i_soa[k] = pk.add_in_place((size_t)N * 4);
            // what the kernels write for the host: records, masks, refined records, refined masks
            *o_mask = morb::align16((size_t)HT * sizeof(orbm_pnp_hyp));
            o_ref = morb::align16(*o_mask + (size_t)mask_first[B] * 8);
            o_rmask = morb::align16(o_ref + (size_t)B * ORBM_PNP_MAX_RECORDS * sizeof(orbm_pnp_refined));
            const size_t out_bytes = o_rmask + (size_t)rmask_first[B] * 8 + 16;
            // what one kernel leaves for the next: records, counts, masks, the records' inlier sets and per-point arrays
            morb::BlockLayout sl;
            const size_t s_rec = sl.take((size_t)HT * sizeof(orbm_pnp_hyp)), s_cnt = sl.take((size_t)HT * 4), s_mask = sl.take((size_t)mask_first[B] * 8),
                         s_idx = sl.take((size_t)pp_points * 4), s_pp = sl.take((size_t)pp_points * 7 * 8),
                         s_ref = sl.take((size_t)B * ORBM_PNP_MAX_RECORDS * sizeof(orbm_pnp_refined));
            int rc;
            const morb::StagePack::Block blk = pk.open(m->pnp.stage, &rc);
            if (rc || (rc = m->pnp.scratch.reserve(sl.off + 16)) || (rc = m->pnp.out.reserve(out_bytes))) return rc;
            float* soa[6];
            for (int k = 0; k < 6; ++k) soa[k] = blk.host<float>(i_soa[k]);
            for (int k = 0; k < N; ++k) {                      // array of structures -> structure of arrays, once per call
                soa[0][k] = p3dw[3 * (size_t)k]; soa[1][k] = p3dw[3 * (size_t)k + 1]; soa[2][k] = p3dw[3 * (size_t)k + 2];
                soa[3][k] = p2d[2 * (size_t)k]; soa[4][k] = p2d[2 * (size_t)k + 1]; soa[5][k] = max_err[k];
            }
            blk.publish();
            PnpDev A;
            A.prob = blk.dev<orbm_pnp_problem>(i_prob); A.first = blk.dev<int32_t>(i_first); A.its_first = blk.dev<int32_t>(i_its);
            A.mask_first = blk.dev<int32_t>(i_mf); A.rmask_first = blk.dev<int32_t>(i_rmf); A.pp_first = blk.dev<int32_t>(i_ppf);
            A.hyp_prob = blk.dev<int32_t>(i_hp); A.quads = blk.dev<int32_t>(i_quads);
            A.x = blk.dev<float>(i_soa[0]); A.y = blk.dev<float>(i_soa[1]); A.z = blk.dev<float>(i_soa[2]);
            A.u = blk.dev<float>(i_soa[3]); A.v = blk.dev<float>(i_soa[4]); A.e = blk.dev<float>(i_soa[5]);
            A.n_hyp = HT;
            A.soa_stride = (int)(A.y - A.x);
            uint8_t* S = m->pnp.scratch.p;
            A.rec_dev = (orbm_pnp_hyp*)(S + s_rec); A.cnt_dev = (int32_t*)(S + s_cnt); A.mask_dev = (uint64_t*)(S + s_mask);
            A.idx_dev = (int32_t*)(S + s_idx); A.pp_dev = (double*)(S + s_pp); A.ref_dev = (orbm_pnp_refined*)(S + s_ref);
            uint8_t* O = m->pnp.out.dp;
            A.rec_out = (orbm_pnp_hyp*)O; A.mask_out = (uint64_t*)(O + *o_mask); A.ref_out = (orbm_pnp_refined*)(O + o_ref); A.rmask_out = (uint64_t*)(O + o_rmask);
            hipLaunchKernelGGL(k_pnp_hyp, dim3((unsigned)((HT + PNP_HYP_T - 1) / PNP_HYP_T)), dim3(PNP_HYP_T), 0, m->stream, A);
            hipLaunchKernelGGL(k_pnp_inliers, dim3((unsigned)HT), dim3(PNP_INL_T), 0, m->stream, A);
            hipLaunchKernelGGL(k_pnp_refine, dim3((unsigned)(B * ORBM_PNP_MAX_RECORDS)), dim3(PNP_REF_T), 0, m->stream, A);
            hipLaunchKernelGGL(k_pnp_refine_inliers, dim3((unsigned)(B * ORBM_PNP_MAX_RECORDS)), dim3(PNP_INL_T), 0, m->stream, A);
            MORB_HIP(hipGetLastError());
            return ORB_OK;
        },
        [&](int b) { pnp_hyps_host(I, b, hyp_out + its_first[b], mask_out + mask_first[b]); },
        [&](int b) {   // the slots the device filled: the first min(records, ORBM_PNP_MAX_RECORDS)
            const orbm_pnp_refined* Rf = (const orbm_pnp_refined*)(m->pnp.out.p + o_ref);
            const uint64_t* Rw = (const uint64_t*)(m->pnp.out.p + o_rmask);
            pnp_records(problems[b], hyp_out + its_first[b], its_first[b + 1] - its_first[b], rec);
            const int nd = std::min((int)rec.size(), (int)ORBM_PNP_MAX_RECORDS), W = ransac_words(first[b + 1] - first[b]);
            if (nd) memcpy(refined_out + (size_t)b * ORBM_PNP_MAX_RECORDS, Rf + (size_t)b * ORBM_PNP_MAX_RECORDS, (size_t)nd * sizeof(orbm_pnp_refined));
            if (nd && W) memcpy(refined_mask_out + rmask_first[b], Rw + rmask_first[b], (size_t)nd * W * 8);
            n_rec_dev += nd;
        });
    if (rc) return rc;
    int n_rec_host = 0;
    rc = pnp_finish_host(I, B, host_from, mask_first, rmask_first, hyp_out, mask_out, n_records_out, refined_out, refined_mask_out, extra_cap, &n_rec_host);
    if (rc) return rc;
    // (records of host problems are not "the tail": count only those beyond ORBM_PNP_MAX_RECORDS of device problems)
    int tail = 0;
    for (int b = 0; b < B; ++b) if (host_from[b]) tail += std::max(0, n_records_out[b] - (int)ORBM_PNP_MAX_RECORDS);
    m->last_pnp[0] = split[0]; m->last_pnp[1] = split[1]; m->last_pnp[2] = n_rec_dev; m->last_pnp[3] = tail;
    return ORB_OK;
}

int orbm_pnp_walk(const int32_t* counts, int H, int block_start, const int32_t* rec_hyp, const int32_t* rec_inliers, int n_rec, int N,
                  int min_inliers, int max_its, int n_iterations, orbm_pnp_walk_state* st) {
    if (!st || (H > 0 && !counts) || (n_rec > 0 && !(rec_hyp && rec_inliers))) return -1;
    st->no_more = 0;
    if (!st->exhausted) st->current = 0;
    st->exhausted = 0;
    if (N < min_inliers) { st->no_more = 1; return ORBM_PNP_WALK_NOTHING; }          // `if(N<mRansacMinInliers)`
    while (st->iterations < max_its || st->current < n_iterations) {
        const int h = st->iterations - block_start;
        if (h < 0 || h >= H) { st->exhausted = 1; return ORBM_PNP_WALK_NOTHING; }
        st->current++;
        st->iterations++;
        const int n = counts[h];
        if (n >= min_inliers) {
            if (n > st->best_inliers) {
                st->best_inliers = n;
                st->best_hyp = block_start + h;
                st->best_record = -1;
                for (int r = 0; r < n_rec; ++r) if (rec_hyp[r] == h) { st->best_record = r; st->best_refined_inliers = rec_inliers[r]; }
                if (st->best_record < 0) return -1;                                  // the records do not belong to these counts
            }
            if (st->best_refined_inliers > min_inliers) return ORBM_PNP_WALK_REFINED;  // `if(Refine())`
        }
    }
    if (st->iterations >= max_its) {
        st->no_more = 1;
        if (st->best_inliers >= min_inliers) return ORBM_PNP_WALK_BEST;
    }
    return ORBM_PNP_WALK_NOTHING;
}

int orbm_pnp_parameters(double probability, int min_inliers, int max_its, int min_set, float epsilon, int N, int32_t* out2, float* epsilon_out) {
    if (!out2 || !epsilon_out) return -1;
    int nMinInliers = ransac_cvtt((double)((float)N * epsilon));
    if (nMinInliers < min_inliers) nMinInliers = min_inliers;
    if (nMinInliers < min_set) nMinInliers = min_set;
    if (epsilon < (float)nMinInliers / (float)N) epsilon = (float)nMinInliers / (float)N;
    out2[0] = ransac_iterations(probability, epsilon, max_its, nMinInliers == N);
    out2[1] = nMinInliers;
    *epsilon_out = epsilon;
    return 0;
}

int orbm_pnp_svd(const double* A, int m, int n, double* w, double* ut, double* vt) {
    if (!A || !w || !ut || n < 1 || m < n || m > 64) return -1;
    for (int i = 0; i < n; ++i) for (int k = 0; k < m; ++k) ut[i * m + k] = A[k * n + i];
    std::vector<double> v((size_t)n * n);
    const cv_vec At = {ut, 1}, W = {w, 1}, Vt = {vt ? vt : v.data(), 1};
    return cv_jacobi_svd_f64(At, m, n, W, Vt, true);
}

int orbm_pnp_qr_solve(double* A, int nr, int nc, double* b, double* x) {
    if (!A || !b || !x || nc < 1 || nr < nc || nc > 64) return -1;
    double A1[64], A2[64];
    const cv_vec a = {A, 1}, bb = {b, 1}, xx = {x, 1}, a1 = {A1, 1}, a2 = {A2, 1};
    return pnp_qr_solve(a, nr, nc, bb, xx, a1, a2);
}

double orbm_pnp_compute_pose(const double* pws, const double* us, int n, const double* K4, double* R9, double* t3, int32_t* out2) {
    if (!pws || !us || n < 1 || !K4 || !R9 || !t3 || !out2) return -1;
    double wsd[PNP_WS];
    int iw[PNP_IW];
    std::vector<double> pp((size_t)n * 7);
    const PnpDoubles pts = {{const_cast<double*>(pws), 1}, {const_cast<double*>(us), 1}};
    const cv_vec ws = {wsd, 1}, alphas = {pp.data(), 1}, pcs = {pp.data() + (size_t)n * 4, 1};
    pnp_compute_pose(PnpSerial(), pts, n, K4, ws, alphas, pcs, iw);
    for (int k = 0; k < 9; ++k) R9[k] = x86_nan(wsd[WS_RB + k]);
    for (int k = 0; k < 3; ++k) t3[k] = x86_nan(wsd[WS_TB + k]);
    out2[0] = iw[IW_CHOICE]; out2[1] = iw[IW_FLAGS];
    return x86_nan(wsd[WS_ERR + 1]);
}

}  // extern "C"
