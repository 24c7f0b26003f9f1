// mapcorrect_dev.h -- loop correction over the resident map (localmap.hip; include/orbm.h, "loop correction over the resident map"):
// the two passes of LoopClosing that move map points, in place in HBM.
//   LoopClosing::CorrectLoop, steps 4.2 (reference src/LoopClosing.cc:678-710)
//                k_map_stamp           the points the caller names as already corrected, stamped with a NEWER epoch than the claim's: no
//                                      candidate's key can win them, and none equals theirs
//                k_map_first / k_map_count / k_map_scan   (localmap_dev.h) the ordered claim, counted
//                k_map_correct_scatter the kept {point slot, position in kfs} to their places -- nothing when they are more than fit
//                k_map_correct_sim3    one lane per kept entry: Swi.map(Siw.map(P)) in double (g2o_dev.h sim3_correct_point)
//   LoopClosing::RunGlobalBundleAdjustment, step 2 (:953-989)
//                k_map_stamp_last      the points that take mPosGBA: the LAST entry that names a slot (64-bit minimum under the call's epoch)
//                k_map_correct_rigid   one lane per slot, grid-stride: the given bytes, or Rwc*(Rcw_before*P + tcw_before) + twc
// The per-point statements are __host__ __device__: orbm_local_map_correct_*_host run the same ones.  Positions written from the host
// (orbm_map_write_positions, the host routes of both corrections) go through k_map_put_words of localmap_dev.h.
#pragma once
#include "localmap_dev.h"
#include "eg_dev.h"   // eg_load, eg_Tiw; g2o_dev.h sim3_*; cv_dev.h cv_gemm3

namespace morb {

constexpr int MAP_SIM3_TABLE = 16;    // doubles per listed keyframe: Siw (NonCorrectedSim3), then the inverse of CorrectedSim3
constexpr int MAP_RIGID_TABLE = 24;   // floats per keyframe slot: rows 0-2 of mTcwBefGBA, then rows 0-2 of GetPoseInverse()
constexpr int MAP_RIGID_MAX_BLOCKS = 2048;

// One keyframe's entry of the Sim3 table, on the host: g2oSiw as given and g2oCorrectedSiw.inverse() (:682)
__host__ __device__ inline void map_sim3_table_entry(const double* before8, const double* after8, double* out16) {
    Sim3Quat A, Ai;
    eg_load(after8, A);
    sim3_inverse(A, Ai);
    for (int k = 0; k < 8; ++k) out16[k] = before8[k];
    eg_store(Ai, out16 + 8);
}
// :701-705 for one point under the table entry of its claimant
__host__ __device__ inline void map_correct_sim3_point(const double* entry16, const float* P, float* out) {
    Sim3Quat Siw, Swi;
    eg_load(entry16, Siw); eg_load(entry16 + 8, Swi);
    sim3_correct_point(Siw, Swi, P, out);
}
// :978-987 for one point: Xc = Rcw*P + tcw, then Rwc*Xc + twc, each one cv::gemm on its small path with alpha = beta = 1
__host__ __device__ inline void map_correct_rigid_point(const float* T24, const float* P, float* out) {
    float Xc[3];
    for (int k = 0; k < 3; ++k) Xc[k] = cv_gemm3(T24 + 4 * k, 1, P, 1.0, T24[4 * k + 3], 1.0);
    for (int k = 0; k < 3; ++k) out[k] = cv_gemm3(T24 + 12 + 4 * k, 1, Xc, 1.0, T24[12 + 4 * k + 3], 1.0);
}
// the key of entry i of the list of given positions: a later entry has the smaller key
__host__ __device__ inline unsigned long long map_last_key(uint32_t epoch, int i) { return map_key(epoch, 0xffffffffu - (uint32_t)i); }

__global__ __launch_bounds__(MAP_BLOCK) void k_map_stamp(const int32_t* __restrict__ slots, int n, unsigned long long* __restrict__ first,
                                                         unsigned long long key) {
    const int i = blockIdx.x * MAP_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int s = slots[i];   // (validated on the host: negative or inside the capacity)
    if (s >= 0) first[s] = key;
}

__global__ __launch_bounds__(MAP_BLOCK) void k_map_stamp_last(const int32_t* __restrict__ slots, int n, unsigned long long* __restrict__ first,
                                                              uint32_t epoch) {
    const int i = blockIdx.x * MAP_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int s = slots[i];
    if (s >= 0) atomicMin(&first[s], map_last_key(epoch, i));
}

// k_map_scatter's twin for a list of {point slot, position in kfs}; entries and entries_out (mapped) have room for cap of them.  A
// total beyond cap writes nothing at all: the call then reports the number and leaves the map as it was.
__global__ __launch_bounds__(MAP_BLOCK) void k_map_correct_scatter(const int32_t* __restrict__ kf_rows, const int32_t* __restrict__ kf_count,
                                                                   const int32_t* __restrict__ kfs, int stride, int bpk,
                                                                   const uint8_t* __restrict__ flags,
                                                                   const unsigned long long* __restrict__ first, uint32_t epoch,
                                                                   const int32_t* __restrict__ block_off, const int32_t* __restrict__ total,
                                                                   orbm_correct_entry* __restrict__ entries,
                                                                   orbm_correct_entry* __restrict__ entries_out, int cap) {
    if (*total > cap) return;   // (uniform)
    const MapCand c = map_candidate(kf_rows, kf_count, kfs, stride, bpk, flags);
    const bool keep = c.slot >= 0 && first[c.slot] == map_key(epoch, c.pos);
    const int at = map_place(keep, block_off);
    if (at >= 0 && at < cap) {
        orbm_correct_entry e; e.point = c.slot; e.position = (int32_t)(blockIdx.x / bpk);
        entries[at] = e; entries_out[at] = e;
    }
}

// One lane per kept entry; n_launched = what the grid was sized for (at most cap).  A point is kept once, so no two lanes share a row.
__global__ __launch_bounds__(MAP_BLOCK) void k_map_correct_sim3(const orbm_correct_entry* __restrict__ entries, int n_launched,
                                                                const int32_t* __restrict__ total, int cap,
                                                                const double* __restrict__ table, orbm_point* __restrict__ rows,
                                                                float* __restrict__ pos_out) {
    const int i = blockIdx.x * MAP_BLOCK + threadIdx.x;
    if (i >= n_launched) return;
    const int n = *total;
    if (n > cap || i >= n) return;
    const orbm_correct_entry e = entries[i];
    float* pos = rows[e.point].pos;
    const float P[3] = {pos[0], pos[1], pos[2]};
    float w[3];
    map_correct_sim3_point(table + (size_t)MAP_SIM3_TABLE * (size_t)e.position, P, w);
    pos[0] = w[0]; pos[1] = w[1]; pos[2] = w[2];
    pos_out[3 * (size_t)i] = w[0]; pos_out[3 * (size_t)i + 1] = w[1]; pos_out[3 * (size_t)i + 2] = w[2];
}

// One lane per entry, grid-stride; slots == NULL: entry i is slot i.  The listed slots are distinct (checked on the host), so no two
// lanes share a row.  status_out and pos_out are mapped; pos_out[3 i ..] is written where the status is not 0.
__global__ __launch_bounds__(MAP_BLOCK) void k_map_correct_rigid(const int32_t* __restrict__ slots, int n, orbm_point* __restrict__ rows,
                                                                 const uint8_t* __restrict__ flags, const int32_t* __restrict__ ref_kf,
                                                                 const uint8_t* __restrict__ kf_corrected, const float* __restrict__ table,
                                                                 int n_kfs, const unsigned long long* __restrict__ first, uint32_t epoch,
                                                                 const float* __restrict__ gba_pos, uint8_t* __restrict__ status_out,
                                                                 float* __restrict__ pos_out) {
    for (long long i = (long long)blockIdx.x * MAP_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * MAP_BLOCK) {
        const int s = slots ? slots[i] : (int)i;
        int st = 0;
        float w[3] = {0.0f, 0.0f, 0.0f};
        if (!(flags[s] & ORBM_POINT_BAD)) {
            const unsigned long long key = first[s];
            if ((uint32_t)(key >> 32) == 0xffffffffu - epoch) {
                const size_t g = (size_t)(0xffffffffu - (uint32_t)key);
                w[0] = gba_pos[3 * g]; w[1] = gba_pos[3 * g + 1]; w[2] = gba_pos[3 * g + 2];
                st = 1;
            } else {
                const int r = ref_kf[s];
                if (r >= 0 && r < n_kfs && kf_corrected[r]) {
                    const float* pos = rows[s].pos;
                    const float P[3] = {pos[0], pos[1], pos[2]};
                    map_correct_rigid_point(table + (size_t)MAP_RIGID_TABLE * (size_t)r, P, w);
                    st = 2;
                }
            }
        }
        if (st) {
            float* pos = rows[s].pos;
            pos[0] = w[0]; pos[1] = w[1]; pos[2] = w[2];
            pos_out[3 * (size_t)i] = w[0]; pos_out[3 * (size_t)i + 1] = w[1]; pos_out[3 * (size_t)i + 2] = w[2];
        }
        status_out[i] = (uint8_t)st;
    }
}

}  // namespace morb
