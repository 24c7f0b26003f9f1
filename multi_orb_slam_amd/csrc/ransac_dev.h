// ransac_dev.h -- what the RANSAC ports share (sim3.hip: minimal sets of 3, pnp.hip: of 4), ONE definition each, for the kernels and the
// host routines.  Both ports are "every hypothesis of a batch in one call": a CSR of problems (first[]) and a CSR of hypotheses
// (its_first[]), one lane per hypothesis for the minimal-set solve, one wave per hypothesis for the inlier mask.
//   ransac_words            the 64-bit words of a mask over n correspondences.
//   ransac_mask_sweep       the wave's inlier sweep: lane l takes positions l, l + 64, ...; a ballot gives the word of 64 consecutive
//                           positions, its population count the count.  ransac_mask_sweep_host: the same statement on the host, bit l
//                           of word c is position c * 64 + l -- the boundary tests hold the device to it byte for byte.
//   ransac_validate<K>      the checks of a call on top of morb::validate_csr (stage_pack.h): the hypothesis counts, mask_first[] with
//                           its 2^31-word cap, every position of every set of K inside its problem.
//   ransac_csr_call         the skeleton of a call: which problems the device takes, launch, the host routine on the others while the
//                           kernels run, one synchronisation, records and mask words copied out of mapped pinned memory.
//   ransac_cvtt, ransac_iterations   the iteration count of SetRansacParameters as the reference's x86 build computes it.
// Apart on purpose: orbm_sim3_walk / orbm_pnp_walk (two different loops of the reference, PnP's interleaves Refine()), the transposes
// to structures of arrays (the field lists differ), k_sim3_hyp / k_pnp_hyp, host/Sim3Solver.cc / host/PnPsolver.cc (ransac_draw.h is theirs).
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "orb_common.h"
#include "matcher_internal.h"
#include "stage_pack.h"

__host__ __device__ __forceinline__ int ransac_words(int n) { return (n + 63) >> 6; }

// ---- the inlier mask of one hypothesis --------------------------------------------------------------------------------------------------
// Every lane of the wave calls it.  test(i): is position i < n an inlier; store(c, word): lane 0 alone, where word c goes.  Returns the
// count (the same in every lane).  No atomics, no LDS, no floating-point value crosses lanes.
template <class Test, class Store>
__device__ __forceinline__ int ransac_mask_sweep(int n, int lane, Test test, Store store) {
    const int W = ransac_words(n);
    int count = 0;
    for (int c = 0; c < W; ++c) {
        const int i = c * 64 + lane;
        const bool in = i < n && test(i);
        const unsigned long long word = __ballot(in);
        count += __popcll(word);
        if (lane == 0) store(c, word);
    }
    return count;
}
template <class Test>
inline int ransac_mask_sweep_host(int n, uint64_t* words, Test test) {
    const int W = ransac_words(n);
    int count = 0;
    for (int c = 0; c < W; ++c) {
        uint64_t word = 0;
        for (int l = 0; l < 64 && c * 64 + l < n; ++l)
            if (test(c * 64 + l)) { word |= (uint64_t)1 << l; ++count; }
        words[c] = word;
    }
    return count;
}

// ---- the batched call -------------------------------------------------------------------------------------------------------------------
// sets: K positions per hypothesis.  mask_first[b] = the first mask word of problem b, mask_first[B] = all of them.  The port checks its
// own arrays (problems, the correspondences, further outputs) around this.
template <int K>
inline int ransac_validate(int B, int max_batch, int max_its, const int32_t* first, const int32_t* its_first, const int32_t* sets,
                           const void* hyp_out, const uint64_t* mask_out, std::vector<int32_t>& mask_first) {
    MORB_ARG(first && its_first);
    if (const int rc = morb::validate_csr(B, max_batch, first)) return rc;
    MORB_ARG(its_first[0] == 0);
    mask_first.assign((size_t)B + 1, 0);
    long long words = 0;
    for (int b = 0; b < B; ++b) {
        const int H = its_first[b + 1] - its_first[b];
        if (H < 0 || H > max_its) { morb::set_error("problem %d: %d hypotheses are outside 0..%d", b, H, max_its); return ORB_E_ARG; }
        words += (long long)H * ransac_words(first[b + 1] - first[b]);
        if (words > INT_MAX) { morb::set_error("the masks of the call exceed 2^31 words"); return ORB_E_CAPACITY; }
        mask_first[(size_t)b + 1] = (int32_t)words;
    }
    if (its_first[B] > 0 && !(sets && hyp_out)) { morb::set_error("the minimal sets or hyp_out is NULL"); return ORB_E_ARG; }
    if (words > 0 && !mask_out) { morb::set_error("mask_out is NULL"); return ORB_E_ARG; }
    for (int b = 0; b < B; ++b) {
        const int n = first[b + 1] - first[b];
        for (int g = its_first[b]; g < its_first[b + 1]; ++g)
            for (int i = 0; i < K; ++i) {
                const int t = sets[K * (size_t)g + i];
                if (t < 0 || t >= n) { morb::set_error("hypothesis %d: position %d is outside the %d correspondences of problem %d", g, t, n, b); return ORB_E_ARG; }
            }
    }
    return ORB_OK;
}

// The problems at or under `cap` correspondences are the device's (with no hypotheses too: nothing runs for them), the longer ones the
// host routine's.  launch(hyp_prob, &mask_off) stages, reserves every buffer and enqueues -- hyp_prob[g] = the problem of hypothesis g,
// or -1 when the host takes it; the kernels leave the records at the start of port.out and the mask words at mask_off, both in the
// caller's order -- and runs only when a hypothesis goes to the device.  host(b): records and mask words of problem b, while the kernels
// run.  after(b): what else the port copies out for device problem b, behind its records and words.  split[0], split[1]: how many
// problems went to the device and to the host.
template <class Rec, class Launch, class Host, class After>
int ransac_csr_call(orbm_matcher* m, PortBufs<uint8_t>& port, int B, const int32_t* first, const int32_t* its_first,
                    const std::vector<int32_t>& mask_first, int cap, Rec* hyp_out, uint64_t* mask_out, int* split, Launch launch,
                    Host host, After after) {
    std::vector<int32_t> hyp_prob((size_t)its_first[B], -1);
    int n_dev = 0, hyp_dev = 0;
    for (int b = 0; b < B; ++b) {
        if (first[b + 1] - first[b] > cap) continue;
        ++n_dev;
        for (int g = its_first[b]; g < its_first[b + 1]; ++g) hyp_prob[g] = b;
        hyp_dev += its_first[b + 1] - its_first[b];
    }
    size_t mask_off = 0;
    if (hyp_dev > 0) {
        MORB_HIP(hipSetDevice(m->device));
        const int rc = launch(hyp_prob, &mask_off);
        if (rc) return rc;
    }
    for (int b = 0; b < B; ++b)             // while the kernels run
        if (first[b + 1] - first[b] > cap) host(b);
    if (hyp_dev > 0) {
        MORB_HIP(hipStreamSynchronize(m->stream));
        const Rec* R = (const Rec*)port.out.p;
        const uint64_t* Wd = (const uint64_t*)(port.out.p + mask_off);
        for (int b = 0; b < B; ++b) {
            if (first[b + 1] - first[b] > cap) continue;
            const size_t H = (size_t)(its_first[b + 1] - its_first[b]), nw = (size_t)(mask_first[b + 1] - mask_first[b]);
            if (H) memcpy(hyp_out + its_first[b], R + its_first[b], H * sizeof(Rec));
            if (nw) memcpy(mask_out + mask_first[b], Wd + mask_first[b], nw * 8);
            after(b);
        }
    }
    split[0] = n_dev; split[1] = B - n_dev;
    return ORB_OK;
}

// ---- SetRansacParameters ----------------------------------------------------------------------------------------------------------------
inline int ransac_cvtt(double d) { return (d >= -2147483648.0 && d < 2147483648.0) ? (int)d : INT_MIN; }   // cvttsd2si / cvttss2si's answer to a NaN or an overflow

// `ceil(log(1 - p) / log(1 - pow(epsilon, 3)))` clamped to 1..max_its; all_inliers: `if(mRansacMinInliers==N) nIterations=1;`
inline int ransac_iterations(double probability, float epsilon, int max_its, bool all_inliers) {
    const int n = all_inliers ? 1 : ransac_cvtt(ceil(log(1 - probability) / log(1 - pow((double)epsilon, 3))));
    return std::max(1, std::min(n, max_its));
}
