// resolve_dev.h -- the steps every form of SearchByProjection's resolve shares (search.hip: k_resolve, k_resolve_mono, k_rs_*,
// k_resolve_cams, host_resolve), written once, and the LDS layout of each single-workgroup form as the host and the kernel both see it.
// The forms differ in the schedule of their rounds, in where the per-query state lives, in whether claims carry sweep tags and in
// whether the rotation histogram is summed in LDS or across workgroups -- not in the arithmetic below.  Everything is forced inline
// (mono_pass at its call sites): a helper boundary must not become a point where LDS reads that are issued together get waited for one by one.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <type_traits>
#include "../../include/orbm.h"
#include "orb_common.h"
#include "matcher_internal.h"

namespace morb {

// Rotation bin of a match (reference src/ORBmatcher.cc:3597-3606), -1 outside [0, ORBM_HISTO_LENGTH): such a match is never
// counted and never rejected.  One float subtraction, one multiplication: nothing here can be contracted into an FMA, so the
// result does not depend on -ffp-contract; the `< 0.0` compare promotes to double as the reference's does.
static __host__ __device__ __forceinline__ int rotation_bin(float query_angle, float feature_angle) {
    float rot = query_angle - feature_angle;
    if (rot < 0.0) rot += 360.0f;
    int bin = (int)roundf(rot * (1.0f / ORBM_HISTO_LENGTH));
    if (bin == ORBM_HISTO_LENGTH) bin = 0;
    return (bin >= 0 && bin < ORBM_HISTO_LENGTH) ? bin : -1;
}

// ComputeThreeMaxima (reference src/ORBmatcher.cc:3948-3989), serial: keeps the three fullest bins; an earlier bin wins a tie
// (strict '>'), 2nd/3rd dropped below 10% of the 1st.
static __host__ __device__ __forceinline__ void three_maxima(const int* histo, int L, int* ind) {
    int m1 = 0, m2 = 0, m3 = 0, i1 = -1, i2 = -1, i3 = -1;
    for (int i = 0; i < L; i++) {
        const int s = histo[i];
        if (s > m1) { m3 = m2; i3 = i2; m2 = m1; i2 = i1; m1 = s; i1 = i; }
        else if (s > m2) { m3 = m2; i3 = i2; m2 = s; i2 = i; }
        else if (s > m3) { m3 = s; i3 = i; }
    }
    if ((float)m2 < 0.1f * (float)m1) { i2 = -1; i3 = -1; }
    else if ((float)m3 < 0.1f * (float)m1) { i3 = -1; }
    ind[0] = i1; ind[1] = i2; ind[2] = i3;
}

// ComputeThreeMaxima on one whole wave, lane b holding bin b's count in `sv` (0 in the lanes past the histogram).  The reference's
// scan with strict '>' keeps the three fullest non-empty bins, the earlier bin first among equals: bin b's place is the number of
// bins that beat it (fuller, or as full and earlier) -- 30 readlanes on one wave instead of 30 dependent LDS reads on one thread.
// `keep` comes out the same in every lane.
static __device__ __forceinline__ void three_maxima_wave(int sv, int lane, int keep[3]) {
    int rank = 0;
#pragma unroll
    for (int j = 0; j < ORBM_HISTO_LENGTH; ++j) {
        const int sj = __builtin_amdgcn_readlane(sv, j);
        rank += (sj > sv || (sj == sv && j < lane)) ? 1 : 0;
    }
    const bool in = lane < ORBM_HISTO_LENGTH && sv > 0;
    const unsigned long long r1 = __ballot(in && rank == 0), r2 = __ballot(in && rank == 1), r3 = __ballot(in && rank == 2);
    int i1 = r1 ? __ffsll((long long)r1) - 1 : -1, i2 = r2 ? __ffsll((long long)r2) - 1 : -1, i3 = r3 ? __ffsll((long long)r3) - 1 : -1;
    const int m1 = i1 >= 0 ? __builtin_amdgcn_readlane(sv, i1) : 0, m2 = i2 >= 0 ? __builtin_amdgcn_readlane(sv, i2) : 0,
              m3 = i3 >= 0 ? __builtin_amdgcn_readlane(sv, i3) : 0;
    if ((float)m2 < 0.1f * (float)m1) { i2 = -1; i3 = -1; }
    else if ((float)m3 < 0.1f * (float)m1) { i3 = -1; }
    keep[0] = i1; keep[1] = i2; keep[2] = i3;
}

// One match per active lane into the rotation histogram in LDS.  Most matches of a frame share a rotation bin: up to three bins of
// the wave (those of its first lanes) are counted with one atomic each, whatever is left (scattered bins: few lanes per address)
// goes in directly.
static __device__ __forceinline__ void hist_add_wave(int* s_hist, bool in_range, int bin, int lane) {
    unsigned long long todo = __ballot(in_range);
    for (int rounds = 0; todo && rounds < 3; ++rounds) {
        const int b0 = __builtin_amdgcn_readlane(bin, __ffsll((long long)todo) - 1);
        const unsigned long long same = __ballot(in_range && bin == b0);
        if (in_range && bin == b0 && lane == __ffsll((long long)same) - 1) atomicAdd(&s_hist[b0], __popcll(same));
        todo &= ~same;
    }
    if (in_range && ((todo >> lane) & 1)) atomicAdd(&s_hist[bin], 1);
}

// Rescan of query q's full candidate list (transposed: [k * nq + q], `full` entries) by a whole wave, 64 candidates per trip, keys
// (distance << 16 | visiting position): the smallest key among the candidates that are neither occupied nor `hidden(g, q)` --
// claimed by a lower blocking query, in the caller's claim table -- is the sequential scan's first minimum, the next one (SECOND)
// its runner-up.  k1 / k2 = 0x7fffffff: none; g1 = the feature (global index) behind k1.  Wave-uniform.
struct Rescan { int k1, g1, k2; };
template <bool SECOND, typename Hidden>
static __device__ __forceinline__ Rescan rescan_wave(int q, int full, int nq, const int* __restrict__ cand_idx,
                                                     const uint16_t* __restrict__ cand_dist, const uint8_t* __restrict__ occupied,
                                                     int lane, Hidden hidden) {
    int k1 = 0x7fffffff, k2 = 0x7fffffff, g1 = -1;
    for (int k0 = 0; k0 < full; k0 += 64) {
        const int k = k0 + lane;
        int key = 0x7fffffff, g = -1;
        if (k < full) {
            g = cand_idx[k * nq + q];
            const int d = cand_dist[k * nq + q];
            bool avail = !(occupied && occupied[g]);
            if (hidden(g, q)) avail = false;
            if (avail) key = (d << 16) | k;
        }
        const int m1 = (int)wave_min_u32((unsigned)key);   // keys are non-negative: unsigned order == signed order
        int m2 = 0x7fffffff;
        if (SECOND) m2 = (int)wave_min_u32((unsigned)(key == m1 ? 0x7fffffff : key));
        // merge the round's (m1 <= m2) into the running (k1 <= k2); the winner's feature comes along by readlane
        if (m1 < k1) {
            k2 = min(k1, m2); k1 = m1;
            g1 = __builtin_amdgcn_readlane(g, __ffsll((long long)__ballot(key == m1)) - 1);   // positions are unique
        }
        else k2 = min(k2, m1);
    }
    return {k1, g1, k2};
}

// Advance of a displaced query i on its sorted shortlist e (0xffff = no entry), cursor at p, in two steps so that a caller with
// several queries per thread can put the reads of all of them in flight before it looks at any:
//   shortlist_claims      the claims on ALL later entries at once (the reads of a slot are in flight together.  Measured: asking for
//                         the next entry alone first costs a third trip more often than it saves reads); -1 where there is nothing to ask;
//   shortlist_first_free  the first of them that no LOWER blocking query holds: new cursor nk (K = ran dry) and new entry ne.
struct Advance { int nk, ne; };
template <int K>
static __device__ __forceinline__ void shortlist_claims(const int (&e)[K], int p, bool displaced, const int* claims, int (&ck)[K]) {
#pragma unroll
    for (int k = 1; k < K; ++k) {
        const bool want = displaced && k > p && e[k] != 0xffff;
        const int v = claims[want ? e[k] : 0];   // (unconditional reads: issued together, no branch)
        ck[k] = want ? v : -1;
    }
}
template <int K>
static __device__ __forceinline__ Advance shortlist_first_free(const int (&e)[K], const int (&ck)[K], int i) {
    int nk = K;
#pragma unroll
    for (int k = K - 1; k >= 1; --k) if (ck[k] >= i) nk = k;
    int ne = 0xffff;
#pragma unroll
    for (int k = 1; k < K; ++k) if (nk == k) ne = e[k];
    return {nk, ne};
}
template <int K>
static __device__ __forceinline__ Advance shortlist_advance(const int (&e)[K], int p, int i, const int* claims) {
    int ck[K];
    shortlist_claims(e, p, true, claims, ck);
    return shortlist_first_free(e, ck, i);
}

// What a rescan of the monotone forms reads: the transposed candidate lists of the whole frame and the first feature of the claim
// table (f0 = 0 when the table spans the frame, the camera's first feature when it spans one camera).
struct RescanCtx {
    int nq; const int* cand_idx; const uint16_t* cand_dist; const uint8_t* occupied; int th_high, f0;
};

// One pass of the monotone iteration over the RQ register-resident queries of every thread of a wave: is the current pick still
// free of lower blocking claims (one LDS read each, issued together)?  For a displaced query the claims on ALL later shortlist
// entries are fetched in one batch, the first free one is taken and claimed; a dry shortlist that is not the whole list is
// rescanned by the whole wave (rare).  Returns "somebody in this wave was displaced".
//   claims    lowest blocking claimant (global query index) per feature of the table;
//   qi        global query indices (0x7fffffff / any index with c < 0: no query in this slot);
//   e, c, p   shortlists and picks in the TABLE's index space (0xffff = no entry, c < 0 = no pick), cursors;
//   fl        bit0 blocks, bit1 list longer than the shortlist;
//   l_choice  u16 mirror of the picks by global query index (0xffff = none), or nullptr: none is kept;
//   list_len  q -> length of q's full candidate list;  chg (instrumented build): this round's counters, or nullptr.
// Inlining: the function itself carries no always_inline -- with it the body is inlined before it has been simplified and the same
// text costs the four-queries-per-thread kernels 21-23 VGPRs (k_resolve_mono<4> 91 -> 114, k_resolve_cams 57 -> 78).  Its call sites
// force it instead (`[[clang::always_inline]] return mono_pass<RQ>(...)`), which reproduces the parent's allocation and does not
// leave the array-reference parameters to the inliner's cost model: a call that stayed a call would put them in scratch.  Scratch
// must stay 0 in both kernels (-Rpass-analysis=kernel-resource-usage; profiles/r16/notes_resolve_refactor.md has the tables).
template <int RQ, typename Choice, typename Len>
static __device__ inline bool mono_pass(int* claims, const int (&qi)[RQ], const int (&e)[RQ][RESOLVE_K], int (&c)[RQ], int (&p)[RQ],
                                                 const int (&fl)[RQ], Choice l_choice, const RescanCtx& R, Len list_len, int lane,
                                                 unsigned long long* chg) {
    constexpr int K = RESOLVE_K;
    constexpr bool MIRROR = !std::is_same<Choice, std::nullptr_t>::value;
    bool disp[RQ], need_rescan[RQ];
    int cl[RQ];
#pragma unroll
    for (int b = 0; b < RQ; ++b) cl[b] = claims[c[b] >= 0 ? c[b] : 0];   // (unconditional reads: issued together, no branch)
#pragma unroll
    for (int b = 0; b < RQ; ++b) { disp[b] = c[b] >= 0 && cl[b] < qi[b]; need_rescan[b] = false; }  // (only blocking queries write claims; an own claim equals the index)
    bool any = false;
#pragma unroll
    for (int b = 0; b < RQ; ++b) any |= disp[b];
    if (!__ballot(any)) return false;
    // (a register slot b none of whose 64 queries is displaced is skipped by the WAVE -- after the first pass or two a handful
    //  of lanes are still moving, on one slot, and the wave whose queries depend on everybody else's walks eight passes while the other
    //  fifteen wait at the round's barrier: its pass went from ~2 us to ~0.6, profiles/r06/notes_experiments.md)
    {
        int ck[RQ][K];
#pragma unroll
        for (int b = 0; b < RQ; ++b) {
            if (!__ballot(disp[b])) continue;
            shortlist_claims(e[b], p[b], disp[b], claims, ck[b]);
        }
#pragma unroll
        for (int b = 0; b < RQ; ++b) {
            if (!__ballot(disp[b])) continue;
            if (!disp[b]) continue;
            const int i = qi[b];
#ifdef MORB_PHASE_CLOCKS
            if (chg) atomicAdd(chg, 1ull);
#endif
            const Advance a = shortlist_first_free(e[b], ck[b], i);
            if (a.nk < K) {
                c[b] = a.ne; p[b] = a.nk;
                if constexpr (MIRROR) l_choice[i] = (unsigned short)a.ne;
                if (fl[b] & 1) atomicMin(&claims[a.ne], i);
            } else {
                c[b] = -1; p[b] = K;
                if constexpr (MIRROR) l_choice[i] = 0xffff;
                // the shortlist is exact unless it ran dry while longer lists exist: rescanned right below
                need_rescan[b] = (fl[b] & 2) != 0;
            }
        }
    }
#pragma unroll
    for (int b = 0; b < RQ; ++b) {
        unsigned long long todo = __ballot(need_rescan[b]);
#ifdef MORB_PHASE_CLOCKS
        if (todo && lane == 0 && chg) atomicAdd(chg + 16, (unsigned long long)__popcll(todo));
#endif
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int q = __builtin_amdgcn_readlane(qi[b], src);
            const Rescan r = rescan_wave<false>(q, list_len(q), R.nq, R.cand_idx, R.cand_dist, R.occupied, lane,
                                                [&](int g, int q_) { return claims[g - R.f0] < q_; });
            if (lane == src && r.k1 != 0x7fffffff && (r.k1 >> 16) <= R.th_high) {   // the rescanned pick is the entry under the cursor from now on
                const int g1 = r.g1 - R.f0;
                c[b] = g1;
                if constexpr (MIRROR) l_choice[q] = (unsigned short)g1;
                if (fl[b] & 1) atomicMin(&claims[g1], q);
            }
        }
    }
    return true;
}

// The result words of a single-workgroup resolve: owner[g] (query index, -1 none, -2 rejected) for the `count` features the table
// holds, into words[0, count).  tagb != 0: every word carries the launch's sequence number in bits 20.. (a match word is stored as
// value + 2).
static __device__ __forceinline__ void write_matches(int* __restrict__ words, const int* owner, int count, int tagb, int tid, int T) {
    for (int g = tid; g < count; g += T) words[g] = tagb ? (tagb | (owner[g] + 2)) : owner[g];
}
// A tagged launch rewrites EVERY word of the frame's capacity, the ones past this frame's count NT as "no match": a word can then
// only carry the current sequence number if this launch stored it (the numbers cycle after 2047 launches; a word left alone since
// its last use -- the count dropped, stayed low for a multiple of 2047 launches and rose again -- would otherwise show the right
// tag with an old value before this launch's store has crossed PCIe).  Called by one workgroup of the launch.
static __device__ __forceinline__ void write_no_match_tail(int* __restrict__ match_of_feature, int NT, int capacity, int tagb, int tid, int T) {
    if (tagb) for (int g = NT + tid; g < capacity; g += T) match_of_feature[g] = tagb | 1;
}

// ---- LDS layouts: one per single-workgroup form, byte offsets into the kernel's dynamic LDS.  search_enqueue sizes the launch and
// decides what fits from the same struct the kernel takes its pointers from.
template <typename T>
static __device__ __forceinline__ T* lds_at(int* base, size_t byte_offset) {
    return reinterpret_cast<T*>(reinterpret_cast<unsigned char*>(base) + byte_offset);
}

// k_resolve: two claim tables (int per feature of the frame's capacity), the candidate counts (u16 per query, padded to 4 bytes);
// with the per-query sweep state (LDSQ) behind them: choice (int), shortlist (distance << 16 | feature) [K][nq], query angle, feature
// angle (float per feature), flags (u8 per query).
struct JacobiLds {
    size_t n, nq;
    __host__ __device__ JacobiLds(int n_, int nq_) : n((size_t)n_), nq((size_t)nq_) {}
    __host__ __device__ size_t claim2() const { return 4 * n; }
    __host__ __device__ size_t cnt() const { return 8 * n; }
    __host__ __device__ size_t tables_bytes() const { return cnt() + (nq + 1) / 2 * 4; }
    __host__ __device__ size_t choice() const { return tables_bytes(); }
    __host__ __device__ size_t gd() const { return choice() + 4 * nq; }
    __host__ __device__ size_t ang() const { return gd() + 4 * RESOLVE_K * nq; }
    __host__ __device__ size_t fang() const { return ang() + 4 * nq; }
    __host__ __device__ size_t fl() const { return fang() + 4 * n; }
    __host__ __device__ size_t bytes(bool ldsq) const { return ldsq ? fl() + nq + 16 : tables_bytes(); }
};

// k_resolve_mono: claims, owners (int per feature); per query (nq2 = nq rounded up to even): list length, pick, K shortlist features
// (u16: the frames this kernel takes have < 65535 features; 0xffff = none), flags (u8, padded to 4 bytes); with `ang` the query /
// feature angles for the rotation histogram (else they are read from HBM in the tail: what lets 4 x 1000 or 2 x 2000 features in at
// all); the worklist of displaced queries (u16, nq2 entries).
struct MonoLds {
    size_t n, nq, nq2;
    bool with_ang;
    __host__ __device__ MonoLds(int n_, int nq_, bool ang_) : n((size_t)n_), nq((size_t)nq_), nq2(((size_t)nq_ + 1) & ~(size_t)1), with_ang(ang_) {}
    __host__ __device__ size_t owner() const { return 4 * n; }
    __host__ __device__ size_t cnt() const { return 8 * n; }
    __host__ __device__ size_t choice() const { return cnt() + 2 * nq2; }
    __host__ __device__ size_t gd() const { return choice() + 2 * nq2; }
    __host__ __device__ size_t fl() const { return gd() + 2 * RESOLVE_K * nq2; }
    __host__ __device__ size_t ang() const { return fl() + ((nq + 3) & ~(size_t)3); }
    __host__ __device__ size_t fang() const { return ang() + 4 * nq; }
    __host__ __device__ size_t wl() const { return with_ang ? fang() + 4 * n : ang(); }
    __host__ __device__ size_t bytes() const { return wl() + 2 * nq2 + 16; }
};

// k_resolve_cams: claims and owners of one camera (int per feature of the largest camera), the camera's queries (u16 global indices,
// as many as a workgroup holds in registers).
struct CamsLds {
    size_t nf_cap, q_cap;
    __host__ __device__ CamsLds(int nf_cap_, int q_cap_) : nf_cap((size_t)nf_cap_), q_cap((size_t)q_cap_) {}
    __host__ __device__ size_t owner() const { return 4 * nf_cap; }
    __host__ __device__ size_t queries() const { return 8 * nf_cap; }
    __host__ __device__ size_t bytes() const { return queries() + 2 * q_cap; }
};

}  // namespace morb
