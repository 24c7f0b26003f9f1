// localmap_dev.h -- the kernels of the resident map (localmap.hip; include/orbm.h, "the local map on the device").
// Every sum here is an integer: the atomics are integer adds and unsigned minima, so any arrival order leaves the same bits.
//   vote:        k_map_mult      one lane per frame feature: multiplicity of the frame per point slot (and the vote bins cleared)
//                k_map_vote      one lane per observation record, grid-stride: the histogram private to the workgroup in LDS, one
//                                merge per non-zero bin
//                k_map_vote_out  the bins into the mapped result, the multiplicities back to zero
//   point list:  k_map_first     one lane per candidate: the least position per point (64-bit minimum, the call's epoch on top)
//                k_map_count     kept candidates per block of 256
//                k_map_scan      one workgroup: exclusive prefix sum over the block counts, the total
//                k_map_scatter   the kept slots to their places
//   writes:      k_map_put_words one lane per 32-bit word: entry r of the staged block into its words of row slots[r] (every slot writer)
//                k_map_put_flags one lane per entry: the flag bytes of orbm_map_write_points
//   search:      k_map_mark      the frame's own points and the `seen` list stamped with the call's epoch (k_frustum<true> reads it)
//   counting:    k_map_chain     one lane per record: the chain from a point to its live records (an exchange on the point's head)
//                k_map_covis     one workgroup per keyframe: UpdateConnections' two counters in LDS bins, compacted in slot order
//                k_map_cull      one workgroup per keyframe: KeyFrameCulling's two counts, ballots only
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/orbm.h"

namespace morb {

constexpr int MAP_BLOCK = 256;         // lanes per workgroup of every kernel here but the scan; the compaction's block size
constexpr int MAP_SCAN_LANES = 1024;   // the one workgroup of k_map_scan
constexpr int MAP_VOTE_PER_LANE = 16;  // records per lane k_map_vote's grid is sized for (a workgroup pays kf bins to clear and merge)
constexpr int MAP_VOTE_MAX_BLOCKS = 512;

// A candidate's key: the call's epoch, inverted, above its position.  A later call's keys are all smaller than an earlier call's, so the
// minimum needs no clearing between calls: whatever an older call left loses to the first candidate of this one.
__host__ __device__ inline unsigned long long map_key(uint32_t epoch, uint32_t pos) {
    return ((unsigned long long)(0xffffffffu - epoch) << 32) | pos;
}

__global__ __launch_bounds__(MAP_BLOCK) void k_map_mult(const int32_t* __restrict__ frame_points, int n_features,
                                                        const uint8_t* __restrict__ flags, int32_t* __restrict__ mult,
                                                        int32_t* __restrict__ votes, int n_kfs) {
    const int i = blockIdx.x * MAP_BLOCK + threadIdx.x;
    if (i < n_kfs) votes[i] = 0;
    if (i >= n_features) return;
    const int p = frame_points[i];   // (validated on the host: negative or a slot inside the capacity)
    if (p >= 0 && !(flags[p] & ORBM_POINT_BAD)) atomicAdd(&mult[p], 1);
}

// Adds from every lane into a few global bins serialise at the memory side; here a lane adds into its workgroup's LDS copy of the bins
// and the workgroup merges each bin it touched with one global add.  Dynamic LDS: n_kfs ints (at most 64 KiB).
__global__ __launch_bounds__(MAP_BLOCK) void k_map_vote(const orbm_obs* __restrict__ obs, int n_obs, const int32_t* __restrict__ mult,
                                                        int32_t* __restrict__ votes, int n_kfs) {
    extern __shared__ int32_t bins[];
    for (int k = threadIdx.x; k < n_kfs; k += MAP_BLOCK) bins[k] = 0;
    __syncthreads();
    for (long long i = (long long)blockIdx.x * MAP_BLOCK + threadIdx.x; i < n_obs; i += (long long)gridDim.x * MAP_BLOCK) {
        const orbm_obs r = obs[i];
        if (r.point < 0) continue;   // a free record
        const int w = mult[r.point];
        if (w) atomicAdd(&bins[r.keyframe], w);   // (keyframe < n_kfs: the high-water mark covers every record's)
    }
    __syncthreads();
    for (int k = threadIdx.x; k < n_kfs; k += MAP_BLOCK) {
        const int v = bins[k];
        if (v) atomicAdd(&votes[k], v);
    }
}

__global__ __launch_bounds__(MAP_BLOCK) void k_map_vote_out(const int32_t* __restrict__ frame_points, int n_features,
                                                            int32_t* __restrict__ mult, const int32_t* __restrict__ votes, int n_kfs,
                                                            int32_t* __restrict__ out) {
    const int i = blockIdx.x * MAP_BLOCK + threadIdx.x;
    if (i < n_kfs) out[i] = votes[i];
    if (i >= n_features) return;
    const int p = frame_points[i];
    if (p >= 0) mult[p] = 0;
}

// The candidates of a point list: block b covers the features [256 (b % bpk), +256) of local keyframe b / bpk; a candidate's
// position is keyframe position * stride + feature, ascending in the reference's order.
struct MapCand { int slot; uint32_t pos; };

__device__ inline MapCand map_candidate(const int32_t* __restrict__ kf_rows, const int32_t* __restrict__ kf_count,
                                        const int32_t* __restrict__ local_kfs, int stride, int bpk, const uint8_t* __restrict__ flags) {
    const int j = blockIdx.x / bpk, f = (blockIdx.x % bpk) * MAP_BLOCK + threadIdx.x;
    const int kf = local_kfs[j];
    MapCand c; c.slot = -1; c.pos = (uint32_t)j * (uint32_t)stride + (uint32_t)f;
    if (f < kf_count[kf]) {
        const int s = kf_rows[(size_t)kf * stride + f];
        if (s >= 0 && !(flags[s] & ORBM_POINT_BAD)) c.slot = s;
    }
    return c;
}

__global__ __launch_bounds__(MAP_BLOCK) void k_map_first(const int32_t* __restrict__ kf_rows, const int32_t* __restrict__ kf_count,
                                                         const int32_t* __restrict__ local_kfs, int stride, int bpk,
                                                         const uint8_t* __restrict__ flags, unsigned long long* __restrict__ first,
                                                         uint32_t epoch) {
    const MapCand c = map_candidate(kf_rows, kf_count, local_kfs, stride, bpk, flags);
    if (c.slot >= 0) atomicMin(&first[c.slot], map_key(epoch, c.pos));
}

__global__ __launch_bounds__(MAP_BLOCK) void k_map_count(const int32_t* __restrict__ kf_rows, const int32_t* __restrict__ kf_count,
                                                         const int32_t* __restrict__ local_kfs, int stride, int bpk,
                                                         const uint8_t* __restrict__ flags, const unsigned long long* __restrict__ first,
                                                         uint32_t epoch, int32_t* __restrict__ block_count) {
    __shared__ int wave_n[MAP_BLOCK / 64];
    const MapCand c = map_candidate(kf_rows, kf_count, local_kfs, stride, bpk, flags);
    const bool keep = c.slot >= 0 && first[c.slot] == map_key(epoch, c.pos);
    const unsigned long long b = __ballot(keep);
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < MAP_BLOCK / 64; ++w) s += wave_n[w];
        block_count[blockIdx.x] = s;
    }
}

// One workgroup: block_count[0 .. nb) becomes its exclusive prefix sum, *total and *total_out (mapped) the sum.  A lane owns a
// contiguous run of blocks; the runs' sums are scanned through LDS.
__global__ __launch_bounds__(MAP_SCAN_LANES) void k_map_scan(int32_t* __restrict__ block_count, int nb, int32_t* __restrict__ total,
                                                             int32_t* __restrict__ total_out) {
    __shared__ int run_sum[MAP_SCAN_LANES];
    const int per = (nb + MAP_SCAN_LANES - 1) / MAP_SCAN_LANES;
    const int lo = min(nb, (int)threadIdx.x * per), hi = min(nb, lo + per);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += block_count[i];
    run_sum[threadIdx.x] = s;
    __syncthreads();
    for (int d = 1; d < MAP_SCAN_LANES; d <<= 1) {   // Hillis-Steele, inclusive
        const int v = threadIdx.x >= (unsigned)d ? run_sum[threadIdx.x - d] : 0;
        __syncthreads();
        run_sum[threadIdx.x] += v;
        __syncthreads();
    }
    int off = run_sum[threadIdx.x] - s;
    for (int i = lo; i < hi; ++i) { const int c = block_count[i]; block_count[i] = off; off += c; }
    if (threadIdx.x == MAP_SCAN_LANES - 1) { *total = run_sum[threadIdx.x]; *total_out = run_sum[threadIdx.x]; }
}

// The place of a kept candidate in the compacted list: its block's offset plus the kept candidates before it in the block; -1 for a
// candidate that is not kept.  Every lane of the workgroup calls it (a barrier inside).
__device__ inline int map_place(bool keep, const int32_t* __restrict__ block_off) {
    __shared__ int wave_n[MAP_BLOCK / 64];
    const unsigned long long b = __ballot(keep);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_n[wave] = __popcll(b);
    __syncthreads();
    if (!keep) return -1;
    int at = block_off[blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) at += wave_n[w];
    return at;
}

// list and list_out (mapped) have room for list_cap entries; a place beyond it is not written (the caller reports the overflow).
__global__ __launch_bounds__(MAP_BLOCK) void k_map_scatter(const int32_t* __restrict__ kf_rows, const int32_t* __restrict__ kf_count,
                                                           const int32_t* __restrict__ local_kfs, int stride, int bpk,
                                                           const uint8_t* __restrict__ flags, const unsigned long long* __restrict__ first,
                                                           uint32_t epoch, const int32_t* __restrict__ block_off, int32_t* __restrict__ list,
                                                           int32_t* __restrict__ list_out, int list_cap) {
    const MapCand c = map_candidate(kf_rows, kf_count, local_kfs, stride, bpk, flags);
    const bool keep = c.slot >= 0 && first[c.slot] == map_key(epoch, c.pos);
    const int at = map_place(keep, block_off);
    if (at >= 0 && at < list_cap) { list[at] = c.slot; list_out[at] = c.slot; }
}

// The scattered write of every slot writer (localmap.hip, write_slots): entry r of the staged block, `words` 32-bit words long, into
// words [offset, offset + words) of row slots[r] of a column whose rows are `pitch` words apart; one lane per word.  (A slot named
// twice was staged twice with the same bytes.)
__global__ __launch_bounds__(MAP_BLOCK) void k_map_put_words(const uint32_t* __restrict__ src, const int32_t* __restrict__ slots, int n,
                                                             int words, int pitch, int offset, uint32_t* __restrict__ dst) {
    const long long i = (long long)blockIdx.x * MAP_BLOCK + threadIdx.x;
    if (i >= (long long)n * words) return;
    const int r = (int)(i / words), w = (int)(i % words);
    dst[(size_t)slots[r] * pitch + offset + w] = src[i];
}

// the flag bytes of orbm_map_write_points, staged next to the rows
__global__ __launch_bounds__(MAP_BLOCK) void k_map_put_flags(const uint8_t* __restrict__ src, const int32_t* __restrict__ slots, int n,
                                                             uint8_t* __restrict__ dst) {
    const int r = blockIdx.x * MAP_BLOCK + threadIdx.x;
    if (r < n) dst[slots[r]] = src[r];
}

// The skip marks of a search: the frame's own points that are not bad, and the points of `seen`.  Every lane stores the same value.
__global__ __launch_bounds__(MAP_BLOCK) void k_map_mark(const int32_t* __restrict__ frame_points, int n_features,
                                                        const int32_t* __restrict__ seen, int n_seen, const uint8_t* __restrict__ flags,
                                                        uint32_t* __restrict__ mark, uint32_t epoch) {
    const int i = blockIdx.x * MAP_BLOCK + threadIdx.x;
    if (i < n_features) {
        const int p = frame_points[i];
        if (p >= 0 && !(flags[p] & ORBM_POINT_BAD)) mark[p] = epoch;
    } else if (i < n_features + n_seen) {
        const int p = seen[i - n_features];
        if (p >= 0) mark[p] = epoch;
    }
}

// ---- covisibility and culling counts (include/orbm.h, "covisibility on the device")
// The index from a point to its live records: head[point] (cleared to -1 before), next[record]; one lane per record slot below the
// high-water mark.  The exchange is the only ordering there is: a record's place in its chain is arbitrary, so the readers count
// and never report a position.
__global__ __launch_bounds__(MAP_BLOCK) void k_map_chain(const orbm_obs* __restrict__ obs, int n_obs, int32_t* __restrict__ head,
                                                         int32_t* __restrict__ next) {
    const int r = blockIdx.x * MAP_BLOCK + threadIdx.x;
    if (r >= n_obs) return;
    const int p = obs[r].point;
    next[r] = p >= 0 ? atomicExch(&head[p], r) : -1;
}

// One bin holds both counters of a keyframe: `all` in the low half, `cam1` in the high half.  Either is at most the length of a
// row (ORBM_MAP_MAX_FEATURES = 8192 < 65536: one live record per (point, keyframe), one add per row entry and record), so one walk
// of the chains fills both and no carry crosses the halves.
constexpr int COVIS_CAM1_SHIFT = 16;
static_assert(ORBM_MAP_MAX_FEATURES < (1 << COVIS_CAM1_SHIFT), "a row's count must fit half a bin");

// One workgroup per listed keyframe.  Lanes stride over the row, each lane walks its point's chain and adds into the workgroup's
// bins in LDS (k_map_vote's idiom); the non-zero bins are then compacted in slot order, 256 at a time.  The workgroup takes its span
// of the output with one add on *cursor, so no workgroup waits for another; span[j] = {start, count} lets the host lay the lists
// out in the order of kfs.  An entry beyond entries_cap is not written (the cursor still says how many there were).
// Dynamic LDS: n_kfs ints and MAP_BLOCK / 64 more.
__global__ __launch_bounds__(MAP_BLOCK) void k_map_covis(const int32_t* __restrict__ kfs, const int32_t* __restrict__ kf_rows,
                                                         const int32_t* __restrict__ kf_count, const int32_t* __restrict__ kf_ncam1,
                                                         int stride, const uint8_t* __restrict__ flags,
                                                         const orbm_obs* __restrict__ obs, const int32_t* __restrict__ obs_feat,
                                                         const int32_t* __restrict__ head, const int32_t* __restrict__ next, int n_kfs,
                                                         int32_t* __restrict__ cursor, int32_t* __restrict__ span,
                                                         orbm_covis_entry* __restrict__ entries, int entries_cap) {
    extern __shared__ int32_t bins[];
    int32_t* wave_n = bins + n_kfs;   // [MAP_BLOCK / 64], then the span's start
    const int k = kfs[blockIdx.x];
    for (int b = threadIdx.x; b < n_kfs; b += MAP_BLOCK) bins[b] = 0;
    __syncthreads();
    const int cnt = kf_count[k], ncam1 = kf_ncam1[k];
    const int32_t* row = kf_rows + (size_t)k * stride;
    for (int i = threadIdx.x; i < cnt; i += MAP_BLOCK) {
        const int p = row[i];
        if (p < 0 || (flags[p] & ORBM_POINT_BAD)) continue;
        for (int r = head[p]; r >= 0; r = next[r]) {
            const int kf = obs[r].keyframe;
            if (kf == k) continue;
            int add = 1;
            if (i < ncam1 && obs_feat[r] < kf_ncam1[kf]) add |= 1 << COVIS_CAM1_SHIFT;
            atomicAdd(&bins[kf], add);
        }
    }
    __syncthreads();
    // the workgroup's total, then its span
    int mine = 0;
    for (int b = threadIdx.x; b < n_kfs; b += MAP_BLOCK) mine += bins[b] != 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d);
    if (lane == 0) wave_n[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < MAP_BLOCK / 64; ++w) total += wave_n[w];
        const int start = atomicAdd(cursor, total);
        span[2 * blockIdx.x] = start; span[2 * blockIdx.x + 1] = total;
        wave_n[MAP_BLOCK / 64] = start;
    }
    __syncthreads();
    int at = wave_n[MAP_BLOCK / 64];
    __syncthreads();
    for (int base = 0; base < n_kfs; base += MAP_BLOCK) {   // (uniform trip count: the ballots and barriers see every lane)
        const int b = base + threadIdx.x;
        const int v = b < n_kfs ? bins[b] : 0;
        const unsigned long long bal = __ballot(v != 0);
        if (lane == 0) wave_n[wave] = __popcll(bal);
        __syncthreads();
        int mine_at = at + __popcll(bal & ((1ull << lane) - 1ull)), step = 0;
        for (int w = 0; w < MAP_BLOCK / 64; ++w) { if (w < wave) mine_at += wave_n[w]; step += wave_n[w]; }
        if (v != 0 && mine_at < entries_cap) {
            orbm_covis_entry e; e.keyframe = b; e.all = v & ((1 << COVIS_CAM1_SHIFT) - 1); e.cam1 = v >> COVIS_CAM1_SHIFT;
            entries[mine_at] = e;
        }
        at += step;
        __syncthreads();
    }
}

// One workgroup per listed keyframe; no bins: per lane two predicates, per wave a ballot and a population count.
// counts[2 j] = nMPs, counts[2 j + 1] = nRedundantObservations.
__global__ __launch_bounds__(MAP_BLOCK) void k_map_cull(const int32_t* __restrict__ kfs, const int32_t* __restrict__ kf_rows,
                                                        const int32_t* __restrict__ kf_count, const uint8_t* __restrict__ kf_feat,
                                                        int stride, const uint8_t* __restrict__ flags, const int32_t* __restrict__ nobs,
                                                        const orbm_obs* __restrict__ obs, const int32_t* __restrict__ obs_feat,
                                                        const int32_t* __restrict__ head, const int32_t* __restrict__ next, int mono,
                                                        int32_t* __restrict__ counts) {
    __shared__ int wave_mp[MAP_BLOCK / 64], wave_red[MAP_BLOCK / 64];
    const int k = kfs[blockIdx.x];
    const int cnt = kf_count[k];
    const int32_t* row = kf_rows + (size_t)k * stride;
    const uint8_t* feat = kf_feat + (size_t)k * stride;
    int n_mp = 0, n_red = 0;   // wave-uniform
    for (int base = 0; base < cnt; base += MAP_BLOCK) {
        const int i = base + threadIdx.x;
        bool counted = false, redundant = false;
        if (i < cnt) {
            const int p = row[i];
            const int fb = feat[i];
            if (p >= 0 && !(flags[p] & ORBM_POINT_BAD) && (mono || !(fb & ORBM_FEATURE_FAR))) {
                counted = true;
                if (nobs[p] > 3) {
                    const int limit = (fb & ORBM_FEATURE_LEVEL_MASK) + 1;
                    int c = 0;
                    for (int r = head[p]; r >= 0; r = next[r]) {
                        const int kf = obs[r].keyframe;
                        if (kf == k) continue;
                        c += (kf_feat[(size_t)kf * stride + obs_feat[r]] & ORBM_FEATURE_LEVEL_MASK) <= limit;
                    }
                    redundant = c >= 3;
                }
            }
        }
        n_mp += __popcll(__ballot(counted));
        n_red += __popcll(__ballot(redundant));
    }
    if ((threadIdx.x & 63) == 0) { wave_mp[threadIdx.x >> 6] = n_mp; wave_red[threadIdx.x >> 6] = n_red; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int a = 0, b = 0;
        for (int w = 0; w < MAP_BLOCK / 64; ++w) { a += wave_mp[w]; b += wave_red[w]; }
        counts[2 * blockIdx.x] = a; counts[2 * blockIdx.x + 1] = b;
    }
}

}  // namespace morb
