// hamming_dev.h -- 256-bit Hamming distance device helpers shared by the matcher's translation units.
#pragma once
#include <hip/hip_runtime.h>

// popcount(x) + acc in ONE instruction (v_bcnt_u32_b32's accumulate operand; hipcc otherwise emits bcnt + add3 trees)
static __device__ __forceinline__ unsigned bcnt_acc(unsigned x, unsigned acc) {
    unsigned r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
    return r;
}

static __device__ __forceinline__ unsigned ham256_chain(const uint4& q0, const uint4& q1, const uint4& a, const uint4& b) {
    unsigned d = __popc(q0.x ^ a.x);
    d = bcnt_acc(q0.y ^ a.y, d); d = bcnt_acc(q0.z ^ a.z, d); d = bcnt_acc(q0.w ^ a.w, d);
    d = bcnt_acc(q1.x ^ b.x, d); d = bcnt_acc(q1.y ^ b.y, d); d = bcnt_acc(q1.z ^ b.z, d); d = bcnt_acc(q1.w ^ b.w, d);
    return d;
}

static __device__ __forceinline__ int ham256(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}


// Merge of the S slice partials of a top-2 (second = 2nd smallest WITH multiplicity: min(s1, s2, max(b1, b2)); the lower slice wins a tie
// of the best): k_top2_merge's body, also run by extra workgroups of the resolve's launch (MergeJob: search.hip, isolated steps).
struct MergeJob {
    const int* p_idx; const int* p_best; const int* p_second; int S, nq;
    int* o_idx; int* o_best; int* o_second; const int* d_range;
    unsigned* done; unsigned target;   // (carried by the resolve's launch: every merging workgroup adds one to *done behind a system-scope
};                                     //  release; the resolve waits for `target` before its result words say "finished")
static __device__ __forceinline__ void top2_merge_query(const int* __restrict__ p_idx, const int* __restrict__ p_best, const int* __restrict__ p_second,
                                                        int S, int nq, int qi, int* __restrict__ best_idx, int* __restrict__ best_dist,
                                                        int* __restrict__ second_dist) {
    int B = 256, Sd = 256, I = -1;
    for (int k = 0; k < S; ++k) {
        const int b2 = p_best[(size_t)k * nq + qi], s2 = p_second[(size_t)k * nq + qi], i2 = p_idx[(size_t)k * nq + qi];
        Sd = min(min(Sd, s2), max(B, b2));
        I = b2 < B ? i2 : I;
        B = min(B, b2);
    }
    best_idx[qi] = I; best_dist[qi] = B; second_dist[qi] = Sd;
}

// A merging workgroup of a carrier launch (the resolve's: workgroups from `first_block` on; isolated steps only): the slice merge of
// the camera-pair top-2 that rode in the projection's launch.  The resolve does not need it, the step does -- one kernel and one
// kernel boundary less between projection and resolve.  Called by every thread of the workgroup, which then returns.
static __device__ __forceinline__ void merge_carrier_block(const MergeJob& MJ, int first_block) {
    const int mq = MJ.d_range ? MJ.d_range[2] : MJ.nq;
    const int qi = ((int)blockIdx.x - first_block) * blockDim.x + threadIdx.x;
    if (qi < mq) top2_merge_query(MJ.p_idx, MJ.p_best, MJ.p_second, MJ.S, mq, qi, MJ.o_idx, MJ.o_best, MJ.o_second);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");   // (system scope: the results live in mapped host memory)
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_fetch_add(MJ.done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The carrier's side of it.  Every exit of the resolve publishes tagged result words the host takes as "the launch is over": none of
// them may be written before the merging workgroups of the same launch have released their results.  Called by all threads of the
// workgroup (s_flag: one int of its LDS); false when the bounded wait gave up -- the status word then says 3 and the host synchronises
// the stream before it reads anything.
static __device__ __forceinline__ bool merge_wait(const MergeJob& MJ, int* s_flag) {
    if (!(MJ.S > 1 && MJ.done)) return true;
    if (threadIdx.x == 0) {
        int spins = 0;
        while ((int)(__hip_atomic_load(MJ.done, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) - MJ.target) < 0 && ++spins < (1 << 22)) __builtin_amdgcn_s_sleep(2);
        *s_flag = spins < (1 << 22) ? 1 : 0;
    }
    __syncthreads();
    return *s_flag != 0;
}
