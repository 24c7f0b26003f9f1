// bow_internal.h -- what bow.hip and triangulate.hip share: the device-side view of a frame / keyframe, the handles behind
// orbv_workspace / orbv_keyframe, the two hooks through which the fused call (orbv_create_new_points_resident) runs the resident
// triangulation search without its synchronisation, and the four through which the chained call (orbv_create_new_points_keyframe)
// runs one such search per neighbour out of buffers reserved once.
#pragma once
#include "../../include/orbv.h"
#include "orb_common.h"

namespace morb {

constexpr int MAX_LEVELS = 32;   // pyramid levels a triangulation search may name

struct SideDev {
    int n, n_nodes;
    const uint4* desc; const float* angle; const uint8_t* flags; const uint32_t* node_id; const int32_t* node_start;
    const uint32_t* items; const float* x; const float* y; const int32_t* octave; const int32_t* cam_of;
};

struct TriDev {
    float F12[ORBV_MAX_CAMS][9];
    float ex[ORBV_MAX_CAMS], ey[ORBV_MAX_CAMS];
    float scale[MAX_LEVELS], sigma2[MAX_LEVELS];
};

struct JoinWork {
    int32_t* match;    // n_out
    uint8_t* bin_of;   // n_out: histogram bin of an accepted match
    int* hist;         // HISTO bins, then [HISTO] = accepted matches
};

// per-feature arrays of the triangulation stage (orbv_keyframe_set_geometry), n floats each in one block
struct GeometryDev {
    const float* uright = nullptr; const float* depth = nullptr; const float* cos_stereo = nullptr;
    const float* xd = nullptr; const float* yd = nullptr;
};

}  // namespace morb

struct orbv_workspace {
    int device = 0;
    hipStream_t stream = nullptr;
    morb::PinnedBuf<uint8_t> h_stage;
    morb::DevBuf<uint8_t> d_stage, d_work;
    morb::PinnedBuf<int32_t> h_match;
    morb::PinnedBuf<uint8_t> h_tri;   // records of the triangulation kernel
    morb::StageBuf tri_const;         // the two keyframes' constants of a triangulation call
    int last_join[4] = {0, 0, 0, 0};  // {waves per node, largest B node, lds_cand, mode} of the last enqueued join (orbv_debug_last_join)
    morb::DevBuf<uint8_t> d_chain;    // orbv_create_new_points_keyframe: the state byte of every feature of `a`, then the round's flags
    int last_kf_call[4] = {0, 0, 0, 0};  // {rounds given, rounds enqueued, kernel launches, synchronisations} of the last such call
    int last_kf_build[5] = {0, 0, 0, 0, 0};  // {bins, chunks of 1024, FeatureVector nodes, largest node, items} of the last
                                             // orbv_keyframe_from_device (orbv_debug_last_keyframe_build)
};

// One frame / keyframe resident in HBM for any number of searches (descriptors, angles, FeatureVector, and the triangulation
// arrays when given): a keyframe is searched against ~20 covisible neighbours by LocalMapping alone (src/LocalMapping.cc).
struct orbv_keyframe {
    int device = 0;
    morb::DevBuf<uint8_t> block;
    morb::SideDev D;
    int max_node = 1, max_cam = 0, max_octave = 0;
    bool tri = false;
    const uint32_t* d_word = nullptr; const uint32_t* d_node = nullptr;   // per-feature descent results (device-built keyframes)
    morb::DevBuf<uint8_t> geometry;   // set by orbv_keyframe_set_geometry
    morb::GeometryDev G;
    bool has_geometry = false;
};

namespace morb {
// orbv_search_for_triangulation_resident up to, not including, its synchronisation.  *enqueued = 0: a side is empty and match[] is
// complete.  Otherwise *d_final is the device address of the a->n final match words (valid on the workspace's stream until its next
// search), and after the caller's synchronisation bow_search_collect copies them out of pinned memory.
int bow_triangulation_search_enqueue(orbv_workspace* w, const orbv_keyframe* a, const uint8_t* flags_a, const orbv_keyframe* b,
                                     const uint8_t* flags_b, const orbv_triangulation* t, int th_low, int check_ori, int32_t* match,
                                     int* nmatches, int* enqueued, const int32_t** d_final);
void bow_search_collect(orbv_workspace* w, int n_out, int32_t* match, int* nmatches, int round = 0);   // round: the chained call's slice

// The chained call (orbv_create_new_points_keyframe): every neighbour's search enqueued before the one synchronisation.
//   bow_chain_check    what the resident triangulation search validates, and the node limit of the join: nothing is touched.
//   bow_chain_runs     false: the search has an empty side and enqueues nothing.
//   bow_chain_reserve  EVERY buffer the searches of one call use, before its first launch (a reserve that reallocates while an enqueued
//                      kernel holds the old pointer is a use-after-free): the join's work area (shared by the rounds: stream order
//                      serialises them), n_rounds slices of n_out pinned match words, stage_bytes of the pinned stage and its mirror.
//   bow_chain_enqueue  init + join + finish of one round, no reserve and no copy: d_flags_a / d_flags_b are device addresses (NULL =
//                      the keyframe's own), the filtered words go to slice `round` of the pinned words and to *d_final as in
//                      bow_triangulation_search_enqueue.  *launches receives the kernels enqueued.
int bow_chain_check(const orbv_workspace* w, const orbv_keyframe* a, const orbv_keyframe* b, const orbv_triangulation* t);
bool bow_chain_runs(const orbv_keyframe* a, const orbv_keyframe* b);
int bow_chain_reserve(orbv_workspace* w, int n_out, int n_rounds, size_t stage_bytes);
int bow_chain_enqueue(orbv_workspace* w, const orbv_keyframe* a, const uint8_t* d_flags_a, const orbv_keyframe* b, const uint8_t* d_flags_b,
                      const orbv_triangulation* t, int th_low, int check_ori, int round, const int32_t** d_final, int* launches);
}  // namespace morb
