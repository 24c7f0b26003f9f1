/* orb_debug.h -- inspection, test and bench hooks of libmorb.so.  Nothing a SLAM caller needs: the parity tests read intermediate
 * stages through these, bench.py times single kernels with them, the multi-GPU tests probe the exchange.  Kept out of orbx.h / orbm.h /
 * orbf.h so that those three headers are the product's interface and nothing else. */
#ifndef ORB_DEBUG_H
#define ORB_DEBUG_H
#include "orbx.h"
#include "orbm.h"
#include "orbf.h"
#include "orbv.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- extractor: stage inspection for the level-by-level parity tests -------------------------------------------------- */
/* (orbx_debug_level, a pyramid level of the last run, stayed in orbx.h: ORBextractor::mvImagePyramid is filled through it) */
/* candidates handed to the quadtree (x, y relative to (16,16); response = score), cell-major order */
int orbx_debug_candidates(orbx_extractor* ex, int cam, int level, orb_keypoint* out, int cap, int* n);
/* host-only: the library's quadtree (DistributeOctTree, reference src/ORBextractor.cc:540-764) on caller-supplied
 * candidates (x, y relative to (16,16), integral; response); runs without a GPU.  *n_out may exceed cap. */
int orbx_debug_distribute_octree(const orb_keypoint* in, int n, int min_x, int max_x, int min_y, int max_y,
                                 int n_features, orb_keypoint* out, int cap, int* n_out);
/* inspection: which keypoint-distribution path produced the last finished run -- 0 device quadtree, 1 device quadtree
 * including the memory-backed pass for levels beyond 4096 candidates, 2 host quadtree (fallback / MORB_HOST_OCTREE=1) */
int orbx_debug_last_path(const orbx_extractor* ex);
/* inspection: cameras whose pyramid level 0 the most recently enqueued run reads in the caller's device buffer instead of a copy
 * (large rigs driven through orbf_*, which promises the buffers' lifetime; 0 everywhere else) */
int orbx_debug_level0_in_place(const orbx_extractor* ex);
/* inspection: how the geometry of the most recent run builds its pyramid -- 0 one tile launch for all levels (k_pyramid_tiled: small
 * rigs), 2 the generic chain (one k_resize launch per level: parameter sets outside both tile forms, MORB_PYR_CHAIN=2), 3 two tile
 * launches with four pixels per lane (k_pyramid_tiled4: large rigs, MORB_PYR_CHAIN=1); -1 before the first run */
int orbx_debug_pyramid_form(const orbx_extractor* ex);
/* tests of the large-rig plan's geometry: tile width / height and split level (defaults 128, 64, 3; 0 = unchanged) of every handle
 * created afterwards.  Process-wide; the product never calls it. */
int orbx_debug_pyramid_plan(int tile_w, int tile_h, int split);

/* ---- matcher ------------------------------------------------------------------------------------------------------------- */
/* {status, nmatches, sweeps, longest candidate list} of the last device-side resolve (inspection only) */
int orbm_debug_last_resolve(const orbm_matcher* m, int* out4);
/* {which resolve produced the result of the last search, capacity retries it took} (inspection only; host-side bookkeeping of
 * search_enqueue, no kernel knows it).  A test written for one form asserts this, so that a moved threshold fails it instead of
 * quietly running another kernel.  The form is the one that delivered the result: the host routine after a device resolve that did
 * not converge, the form of the last launch after a capacity retry. */
#define ORBM_FORM_NONE 0           /* nothing to resolve (no queries or no features) */
#define ORBM_FORM_HOST 1           /* host_resolve: MORB_HOST_RESOLVE=1, more queries than the device takes, or the fallback */
#define ORBM_FORM_MONO2_ANG 2      /* k_resolve_mono<2, true>: up to 2048 queries, rotation angles in LDS */
#define ORBM_FORM_MONO2 3          /* k_resolve_mono<2, false>: the angles stay in HBM */
#define ORBM_FORM_MONO4_WORKLIST 4 /* k_resolve_mono<4, .>, worklist rounds (more than 2048 queries) */
#define ORBM_FORM_MONO4_WAVES 5    /* k_resolve_mono<4, .>, per-wave passes (MORB_RESOLVE_MONO=1) */
#define ORBM_FORM_JACOBI_LDSQ 6    /* k_resolve<., true>: Jacobi sweeps, per-query state in LDS */
#define ORBM_FORM_JACOBI 7         /* k_resolve<., false>: per-query state in HBM */
#define ORBM_FORM_CAMS 8           /* k_resolve_cams: one workgroup per camera */
#define ORBM_FORM_SWEEPS 9         /* k_rs_sweep + k_rs_owner [+ k_rs_reject] + k_rs_write: one launch per sweep, tables in HBM */
int orbm_debug_last_resolve_form(const orbm_matcher* m, int* out2);
/* The frame assembly with the per-camera counts still on the device, as the front end enqueues it behind an extraction it has not
 * waited for -- with keypoints of the caller's choosing (inspection only; the boundary tests of the assembly reach k_frame_build_small
 * with device counts, k_frame_fill_head, k_frame_head and k_cams_from_counts through it).  d_counts: n_cams + 1 ints in HBM, the real
 * counts and then the extractor's status word (0); cams[c].n are CAPACITIES here, 0 <= count <= capacity (checked before anything is
 * enqueued).  Enqueues what orbm_frame_from_device would, synchronises the handle's stream and sets the counts on the frame as the front
 * end does after its own synchronisation: orbm_frame_grid, orbm_frame_download and the searches then work on *out. */
int orbm_debug_frame_from_device_counts(orbm_matcher* m, const orbm_cam_features* cams, int n_cams, const int* d_counts, float mbf,
                                        float min_x, float min_y, float max_x, float max_y, orbm_frame** out);
/* Where the points of the last orbm_refresh_points went: {16-lane groups, one wavefront, one workgroup, host routine because the
 * point has more than ORBM_REFRESH_CAP observations, no work (no observations or no job)} (inspection only) */
int orbm_debug_last_refresh(const orbm_matcher* m, int* out5);
/* Where the problems of the last orbm_pose_optimize[_resident] went: {one workgroup on the device, host routine because the problem
 * has more than ORBM_POSE_CAP edges} (inspection only) */
int orbm_debug_last_pose(const orbm_matcher* m, int* out2);
/* Where the problems of the last orbm_sim3_ransac went: {the device, host routine because the problem has more than ORBM_SIM3_CAP
 * correspondences} (inspection only) */
int orbm_debug_last_sim3(const orbm_matcher* m, int* out2);
/* Where the problems of the last orbm_sim3_optimize went: {one workgroup on the device, host routine because the problem has more than
 * ORBM_SIM3OPT_CAP correspondences} (inspection only) */
int orbm_debug_last_sim3opt(const orbm_matcher* m, int* out2);
/* What the last orbm_local_ba did: {path (0 the device, 1 the host routine because a cap of ORBM_LBA_MAX_* is exceeded, 2 the host
 * routine because no pose is free), kernel launches, stream synchronisations, polls of the stop function} (inspection only) */
int orbm_debug_last_local_ba(const orbm_matcher* m, int* out4);
/* What the last orbm_bundle_adjust did: {path (0 the device, 1 the host routine because a cap of ORBM_BA_MAX_* is exceeded, 2 the host
 * routine because no free pose is active), kernel launches, stream synchronisations, polls of the stop function, block pairs of the
 * reduced system computed, block pairs possible (na (na + 1) / 2), panels of the blocked LDL^T, 0} (inspection only) */
int orbm_debug_last_bundle_adjust(const orbm_matcher* m, int* out8);
/* What the last orbm_essential_graph did: {path (0 the device, 1 the host routine because a cap of ORBM_EG_MAX_* is exceeded, 2 the
 * host routine because no free vertex is active), kernel launches, stream synchronisations, 0, block pairs computed (the diagonal
 * blocks included), block pairs possible (na (na + 1) / 2), panels of the blocked LDL^T, 0} (inspection only) */
int orbm_debug_last_essential_graph(const orbm_matcher* m, int* out8);
/* What the last orbm_map_vote / orbm_map_local_points on the map did: {1 if the last call ran on the device (0: MORB_HOST_RESOLVE=1,
 * the host routines over the mirror), observation records scanned by the last vote, candidates of the last point list (the sum of the
 * listed keyframes' feature counts), points it kept} (inspection only) */
int orbm_debug_last_local_map(const orbm_map* map, int* out4);
/* What the last orbm_map_covisibility / orbm_map_culling_counts on the map did: {1 if it ran on the device (0: MORB_HOST_RESOLVE=1, the
 * host routines over the mirror), 1 if this call rebuilt the point -> records index (only after an orbm_map_write_observations),
 * records indexed (the record high-water mark), keyframes processed} (inspection only) */
int orbm_debug_last_covisibility(const orbm_map* map, int* out4);
/* What the last orbm_map_correct_sim3 / orbm_map_correct_rigid on the map did: {1 if it ran on the device (0: MORB_HOST_RESOLVE=1, the
 * host routines over the mirror), candidates (row entries of the listed keyframes / point slots looked at), points kept (Sim3) or
 * changed (rigid: status != 0), keyframes (listed / in the table)} (inspection only) */
int orbm_debug_last_correction(const orbm_map* map, int* out4);
/* Rows of the listed point slots as HBM holds them now -- NOT the mirror (inspection only: one copy of the span the slots cover). */
int orbm_debug_map_read_points(orbm_matcher* m, orbm_map* map, const int32_t* slots, int n, orbm_point* rows);
/* Where the work of the last orbm_pnp_ransac went: {problems on the device, problems through the host routine because they have more
 * than ORBM_PNP_CAP correspondences, records refined on the device, records refined by the host routine because they lie beyond
 * ORBM_PNP_MAX_RECORDS of a device problem} (inspection only) */
int orbm_debug_last_pnp(const orbm_matcher* m, int* out4);
/* The capacities in bytes of the buffers orbm_pnp_ransac keeps between calls: {the staged inputs, the device block the kernels leave
 * for one another (records, counts, masks, the inlier sets and per-point arrays of the refinements), the mapped results}: they grow
 * with the largest call and are reused by every smaller one (inspection only) */
int orbm_debug_pnp_buffers(const orbm_matcher* m, unsigned long long* out3);
/* Inspection / bench (roofline M3): `iters` launches of the projection kernel alone, as the frame search
 * launches it (window + level + right-coordinate gates, distances, shortlist), timed with HIP events on the handle's
 * stream.  *avg_us = average launch duration, *n_gated = candidates that passed the gates, summed over the queries. */
int orbm_debug_time_project(orbm_matcher* m, const orbm_frame* f, const orbm_query* q, int nq, int th_high, int iters,
                            float* avg_us, long long* n_gated);

/* ---- BoW-gated searches -------------------------------------------------------------------------------------------------- */
/* {waves per vocabulary node (1 or 4), largest node of side B, candidates of a node staged in LDS (lds_cand; candidates from there on
 * are read from HBM), mode (0 SearchByBoW(KF, F), 1 SearchByBoW(KF, KF), 2 SearchForTriangulation)} of the last join enqueued on the
 * workspace (inspection only; host-side bookkeeping of enqueue_join, no kernel knows it; all zero before the first one).  A test written
 * for one form of k_bow_join asserts this, so that a moved threshold fails it instead of quietly running another kernel. */
int orbv_debug_last_join(const orbv_workspace* w, int* out4);
/* {rounds given, rounds enqueued (a round whose search has an empty side is not), kernel launches, stream synchronisations} of the last
 * orbv_create_new_points_keyframe on the workspace (inspection only; counted on the host where the call enqueues, as last_join is; all
 * zero before the first call and after one that was refused). */
int orbv_debug_last_keyframe_call(const orbv_workspace* w, int* out4);
/* {bins (1 + vocabulary nodes at the FeatureVector's level; bin 0 is the root's), chunks of 1024 bins k_fv_offsets scanned, FeatureVector
 * nodes, largest node (what the joins size their LDS with), items (features whose word is not stopped)} of the last
 * orbv_keyframe_from_device on the workspace (inspection only; host-side bookkeeping from the sizes and the three counters the call reads
 * back anyway; all zero before the first call and after one that was refused).  A test written for one chunk count asserts this. */
int orbv_debug_last_keyframe_build(const orbv_workspace* w, int* out5);

/* ---- keyframe database --------------------------------------------------------------------------------------------------- */
/* {form of k_db_query, entries per workgroup (epb), workgroups per query, queries} of the last launch behind orbv_db_query /
 * orbv_db_score on the database (inspection only; host-side bookkeeping of the launch, no kernel knows it; all zero before the first
 * launch -- a call with no queries or no entries launches nothing and leaves the report as it was). */
#define ORBV_DB_FORM_LDS 1     /* k_db_query<true>: the longest query of the call has at most 4096 words, queries lie in LDS */
#define ORBV_DB_FORM_GLOBAL 2  /* k_db_query<false>: queries are read from global memory */
int orbv_debug_last_db_query(const orbv_database* db, int* out4);

/* ---- front end: probes of the multi-GPU exchange ------------------------------------------------------------------------- */
/* With on != 0 every step of a handle with an exchange records (HIP events) when its search and when its exchange (all-gather +
 * repack + rig-wide top-2) had finished on the device; orbf_debug_exchange_us returns the last step's two figures in microseconds
 * from the start of the step's matching (the second one is negative when the exchange -- issued with the step's extraction chain
 * -- was over before the matching began). */
int orbf_debug_exchange_timing(orbf_frontend* f, int on);
int orbf_debug_exchange_us(const orbf_frontend* f, float* out2);
/* The frame of the last finished step (NULL before the first one), owned by the front end and valid until the next step begins:
 * orbm_frame_grid / orbm_frame_count read it, nothing may destroy it.  *form says which assembly filled it: 1 the extractor's describe
 * kernel wrote the per-feature half and the cells through the frame sink (rigs of up to 4 cameras and 8192 features on the asynchronous
 * path), 2 the matcher's kernels with the counts still on the device (larger rigs), 0 orbm_frame_from_device after a synchronised
 * extraction (inspection only). */
const orbm_frame* orbf_debug_last_frame(const orbf_frontend* f, int* form);
/* steps whose blocks were shipped a second time (a block had gone out before its extraction fell back to the host quadtree) */
long orbf_debug_exchange_redos(const orbf_frontend* f);

#ifdef __cplusplus
}
#endif
#endif
