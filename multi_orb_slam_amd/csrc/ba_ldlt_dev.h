// ba_ldlt_dev.h -- the reduced system of the global bundle adjustment on the device (lba.hip, include/orbm.h "global bundle
// adjustment"): a blocked LDL^T without pivoting across workgroups, n = 6 na up to 6 * ORBM_BA_MAX_FREE rows, whose every element is
// the bytes of the sequential routine (lba.hip's ba_ldlt_host, the definition).  What makes that possible is the order of the sums:
//   factor    L(i,k) = (H(k,i) - sum_{j<k, ascending} L(i,j) (d_j L(k,j))) / d_k, every sum from 0.0
//   forward   y_i = b_i - sum_{j<i, ascending} L(i,j) y_j
//   backward  x_i = y_i / d_i - sum_{j>i, DESCENDING} L(j,i) x_j
// so that a row's terms arrive panel by panel in the order the sequential routine adds them: a sum is carried from one panel to
// the next (in the place its result will take: Lt for the factor, `carry` for the substitutions) and never split or re-associated.
// Per panel of BA_PANEL columns, left-looking:
//   k_ba_panel_update  every element at or below the panel's diagonal: its sum over ALL columns left of the panel, tiles in LDS
//   k_ba_panel_diag    one workgroup: the panel's diagonal block, column by column; its pivots; the failure flag
//   k_ba_panel_rows    the rows below: the panel's columns from the carried sums
//   k_ba_fwd_diag / k_ba_fwd_rows, k_ba_back_diag / k_ba_back_rows   the substitutions the same way
// Double throughout, multiply and add separate (-ffp-contract=off; no matrix instruction: the order of their four products is not
// documented).  No atomics, no kernel waits for another, the lanes' sums live in registers or LDS.  After a zero or non-finite pivot
// every later kernel returns at once, x is not written and *ok2 = 0: the flag never leaves the device.
// Bounds: Lt and Hs are n x n; every access is row * n + column with row, column < n (guards `< n` on the ragged last panel).
#pragma once
#include <cfloat>
#include <cmath>
#include <hip/hip_runtime.h>

constexpr int BA_PANEL = 64;          // w: columns of a panel = rows of a tile = lanes of the single-workgroup kernels
constexpr int BA_UPDATE_T = 256;      // lanes of k_ba_panel_update: 64 rows x 4 groups of BA_PANEL / 4 columns
constexpr int BA_JB = 32;             // columns left of the panel staged at a time (divides BA_PANEL, so a chunk is never ragged)
static_assert(BA_PANEL == 64 && BA_PANEL % BA_JB == 0, "the tile shapes below");

namespace {

struct BaSolve {
    int n;
    const double* Hs; const double* bs;   // n x n row-major (upper triangle read), n
    double* Lt; double* d;                // Lt[k n + i] = L(i, k), i > k; D
    double* y; double* carry; double* x;  // n each; x is written only on success
    int* fail; int* ok2;
};

__device__ __forceinline__ bool ba_bad_pivot(double dk) { return !(fabs(dk) > 0) || !(fabs(dk) <= DBL_MAX); }

// blockIdx.x: a tile of 64 rows from the panel's first row on.  Lane (ii, kg) owns row i0 + ii and the 16 columns k0 + 16 kg ..:
// acc(i, k) = sum_{j < k0} L(i, j) (d_j L(k, j)), j ascending from 0.0, left where L(i, k) will stand.
__global__ __launch_bounds__(BA_UPDATE_T) void k_ba_panel_update(BaSolve A, int k0) {
    __shared__ double s_a[BA_JB][64];
    __shared__ double s_b[BA_JB][BA_PANEL];
    if (*A.fail) return;
    const int n = A.n, t = threadIdx.x, ii = t & 63, kg = t >> 6;
    const int i0 = k0 + 64 * (int)blockIdx.x;
    double acc[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[c] = 0.0;
    for (int j0 = 0; j0 < k0; j0 += BA_JB) {
        for (int q = t; q < BA_JB * 64; q += BA_UPDATE_T) {
            const int jj = q >> 6, c = q & 63;
            const size_t row = (size_t)(j0 + jj) * n;
            s_a[jj][c] = i0 + c < n ? A.Lt[row + i0 + c] : 0.0;
            s_b[jj][c] = k0 + c < n ? A.d[j0 + jj] * A.Lt[row + k0 + c] : 0.0;
        }
        __syncthreads();
        for (int jj = 0; jj < BA_JB; ++jj) {
            const double a = s_a[jj][ii];
#pragma unroll
            for (int c = 0; c < 16; ++c) acc[c] = acc[c] + a * s_b[jj][16 * kg + c];
        }
        __syncthreads();
    }
    const int i = i0 + ii;
    if (i >= n) return;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const int k = k0 + 16 * kg + c;
        if (k < n && i >= k) A.Lt[(size_t)k * n + i] = acc[c];
    }
}

// One workgroup of BA_PANEL lanes, lane ii owns row k0 + ii of the diagonal block: the statements of the sequential routine column by
// column, every sum continued from the carried one.  The first panel's kernel is the first of a solve and clears the failure flag.
__global__ __launch_bounds__(BA_PANEL) void k_ba_panel_diag(BaSolve A, int k0) {
    __shared__ double s_L[BA_PANEL][BA_PANEL + 1];     // s_L[ii][jj] = L(k0 + ii, k0 + jj)
    __shared__ double s_t[BA_PANEL], s_d[BA_PANEL];
    __shared__ double s_dk;
    __shared__ int s_fail;
    const int n = A.n, ii = threadIdx.x, i = k0 + ii, wp = min(BA_PANEL, n - k0);
    if (k0 > 0 && *A.fail) return;
    if (ii == 0) { s_fail = 0; if (k0 == 0) *A.fail = 0; }
    __syncthreads();
    for (int kk = 0; kk < wp; ++kk) {
        const size_t row = (size_t)(k0 + kk) * n;
        if (ii < kk) s_t[ii] = s_d[ii] * s_L[kk][ii];
        __syncthreads();
        double r = 0.0;
        if (ii >= kk && ii < wp) {
            double s = k0 > 0 ? A.Lt[row + i] : 0.0;
            for (int jj = 0; jj < kk; ++jj) s = s + s_L[ii][jj] * s_t[jj];
            r = A.Hs[row + i] - s;
            if (ii == kk) { s_dk = r; s_d[kk] = r; if (ba_bad_pivot(r)) s_fail = 1; }
        }
        __syncthreads();
        if (s_fail) break;
        if (ii > kk && ii < wp) s_L[ii][kk] = r / s_dk;
        __syncthreads();
    }
    if (s_fail) { if (ii == 0) *A.fail = 1; return; }
    if (ii < wp) A.d[i] = s_d[ii];
    for (int jj = 0; jj < wp; ++jj)
        if (ii > jj && ii < wp) A.Lt[(size_t)(k0 + jj) * n + i] = s_L[ii][jj];
}

// The rows below a full panel, one lane per row (blockIdx.x: 64 of them).  s_T[kk][jj] = d_j L(k, j) inside the panel; the row's own
// L(i, k0 ..) stays in the lane's column of s_L.
__global__ __launch_bounds__(BA_PANEL) void k_ba_panel_rows(BaSolve A, int k0) {
    __shared__ double s_T[BA_PANEL][BA_PANEL + 1];
    __shared__ double s_L[BA_PANEL][BA_PANEL];
    __shared__ double s_d[BA_PANEL];
    if (*A.fail) return;
    const int n = A.n, t = threadIdx.x;
    s_d[t] = A.d[k0 + t];
    for (int jj = 0; jj < BA_PANEL; ++jj) s_T[t][jj] = t > jj ? A.d[k0 + jj] * A.Lt[(size_t)(k0 + jj) * n + k0 + t] : 0.0;
    __syncthreads();
    const int i = k0 + BA_PANEL + 64 * (int)blockIdx.x + t;
    if (i >= n) return;
    for (int kk = 0; kk < BA_PANEL; ++kk) {
        const size_t at = (size_t)(k0 + kk) * n + i;
        double s = k0 > 0 ? A.Lt[at] : 0.0;
        for (int jj = 0; jj < kk; ++jj) s = s + s_L[jj][t] * s_T[kk][jj];
        const double v = (A.Hs[at] - s) / s_d[kk];
        s_L[kk][t] = v;
        A.Lt[at] = v;
    }
}

// y of the panel's rows: lane ii continues row k0 + ii's sum with the panel's own y as they appear
__global__ __launch_bounds__(BA_PANEL) void k_ba_fwd_diag(BaSolve A, int k0) {
    __shared__ double s_y[BA_PANEL];
    if (*A.fail) return;
    const int n = A.n, ii = threadIdx.x, i = k0 + ii, wp = min(BA_PANEL, n - k0);
    double s = (k0 > 0 && ii < wp) ? A.carry[i] : 0.0;
    for (int jj = 0; jj < wp; ++jj) {
        if (ii == jj) s_y[jj] = A.bs[i] - s;
        __syncthreads();
        if (ii > jj && ii < wp) s = s + A.Lt[(size_t)(k0 + jj) * n + i] * s_y[jj];
    }
    if (ii < wp) A.y[i] = s_y[ii];
}
// the rows below a full panel add the panel's terms in ascending column
__global__ __launch_bounds__(BA_UPDATE_T) void k_ba_fwd_rows(BaSolve A, int k0) {
    __shared__ double s_y[BA_PANEL];
    if (*A.fail) return;
    const int n = A.n, t = threadIdx.x;
    if (t < BA_PANEL) s_y[t] = A.y[k0 + t];
    __syncthreads();
    const int i = k0 + BA_PANEL + BA_UPDATE_T * (int)blockIdx.x + t;
    if (i >= n) return;
    double s = k0 > 0 ? A.carry[i] : 0.0;
    for (int jj = 0; jj < BA_PANEL; ++jj) s = s + A.Lt[(size_t)(k0 + jj) * n + i] * s_y[jj];
    A.carry[i] = s;
}

// x of the panel's rows, last row first.  s_B[ii][jj] = L(k0 + jj, k0 + ii) (read along Lt's rows, so the loads coalesce).  The
// kernel of panel 0 is the last of a solve and leaves ok2.
__global__ __launch_bounds__(BA_PANEL) void k_ba_back_diag(BaSolve A, int k0) {
    __shared__ double s_B[BA_PANEL][BA_PANEL + 1];
    __shared__ double s_x[BA_PANEL];
    const int n = A.n, ii = threadIdx.x, i = k0 + ii, wp = min(BA_PANEL, n - k0);
    if (*A.fail) { if (k0 == 0 && ii == 0) *A.ok2 = 0; return; }
    const bool last = k0 + BA_PANEL >= n;
    for (int r = 0; r < wp; ++r) s_B[r][ii] = ii < wp ? A.Lt[(size_t)(k0 + r) * n + i] : 0.0;
    __syncthreads();
    const double z = ii < wp ? A.y[i] / A.d[i] : 0.0;
    double s = (!last && ii < wp) ? A.carry[i] : 0.0;
    for (int jj = wp - 1; jj >= 0; --jj) {
        if (ii == jj) s_x[jj] = z - s;
        __syncthreads();
        if (ii < jj) s = s + s_B[ii][jj] * s_x[jj];
    }
    if (ii < wp) A.x[i] = s_x[ii];
    if (k0 == 0 && ii == 0) *A.ok2 = 1;
}
// the rows above add the panel's terms in descending column (blockIdx.x: 64 rows; every row above the panel exists)
__global__ __launch_bounds__(BA_PANEL) void k_ba_back_rows(BaSolve A, int k0) {
    __shared__ double s_B[BA_PANEL][BA_PANEL + 1];     // s_B[r][c] = L(k0 + c, i0 + r)
    __shared__ double s_x[BA_PANEL];
    if (*A.fail) return;
    const int n = A.n, t = threadIdx.x, wp = min(BA_PANEL, n - k0), i0 = 64 * (int)blockIdx.x;
    const bool last = k0 + BA_PANEL >= n;
    s_x[t] = t < wp ? A.x[k0 + t] : 0.0;
    for (int r = 0; r < 64; ++r) s_B[r][t] = t < wp ? A.Lt[(size_t)(i0 + r) * n + k0 + t] : 0.0;
    __syncthreads();
    const int i = i0 + t;                              // < k0 <= n - 1
    double s = last ? 0.0 : A.carry[i];
    for (int jj = wp - 1; jj >= 0; --jj) s = s + s_B[t][jj] * s_x[jj];
    A.carry[i] = s;
}
__global__ void k_ba_solved_nothing(int* ok2) { *ok2 = 1; }      // n == 0: the sequential routine succeeds

// the whole solve on `st`; returns the launches
inline int ba_ldlt_enqueue(hipStream_t st, const BaSolve& A) {
    const int n = A.n, w = BA_PANEL;
    int launches = 0;
    if (n == 0) { hipLaunchKernelGGL(k_ba_solved_nothing, dim3(1), dim3(1), 0, st, A.ok2); return 1; }
    for (int k0 = 0; k0 < n; k0 += w) {
        if (k0 > 0) { hipLaunchKernelGGL(k_ba_panel_update, dim3((unsigned)((n - k0 + 63) / 64)), dim3(BA_UPDATE_T), 0, st, A, k0); ++launches; }
        hipLaunchKernelGGL(k_ba_panel_diag, dim3(1), dim3(w), 0, st, A, k0); ++launches;
        if (n > k0 + w) { hipLaunchKernelGGL(k_ba_panel_rows, dim3((unsigned)((n - k0 - w + 63) / 64)), dim3(w), 0, st, A, k0); ++launches; }
    }
    for (int k0 = 0; k0 < n; k0 += w) {
        hipLaunchKernelGGL(k_ba_fwd_diag, dim3(1), dim3(w), 0, st, A, k0); ++launches;
        if (n > k0 + w) { hipLaunchKernelGGL(k_ba_fwd_rows, dim3((unsigned)((n - k0 - w + BA_UPDATE_T - 1) / BA_UPDATE_T)), dim3(BA_UPDATE_T), 0, st, A, k0); ++launches; }
    }
    for (int k0 = (n - 1) / w * w; k0 >= 0; k0 -= w) {
        hipLaunchKernelGGL(k_ba_back_diag, dim3(1), dim3(w), 0, st, A, k0); ++launches;
        if (k0 > 0) { hipLaunchKernelGGL(k_ba_back_rows, dim3((unsigned)(k0 / 64)), dim3(w), 0, st, A, k0); ++launches; }
    }
    return launches;
}

}  // namespace
