/* orbm.h -- C ABI of the MI355X ORB matcher (drop-in for the hot part of ORB_SLAM2::ORBmatcher).
 *
 * Replaces:
 *   static int ORBmatcher::DescriptorDistance(const cv::Mat&, const cv::Mat&)
 *        reference include/ORBmatcher.h:44, src/ORBmatcher.cc:3994-4010                -> orbm_descriptor_distance
 *   the exhaustive top-2 Hamming loops inside SearchByBoW / SearchForTriangulation
 *        reference src/ORBmatcher.cc:287-321, :1069-1104, :1533-1594                  -> orbm_hamming_top2[_device]
 *   (new, for cross-camera all-pairs work)                                            -> orbm_hamming_matrix[_device]
 *   int ORBmatcher::SearchByProjection(Frame&, const Frame&, float th, bool bMono, cv::Mat Calib)
 *        reference include/ORBmatcher.h:54-55, src/ORBmatcher.cc:3448-3641            -> orbm_search_by_projection
 *   int ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, float th)
 *        reference include/ORBmatcher.h:48, src/ORBmatcher.cc:62-149                  -> orbm_search_by_projection_points
 *   Frame::AssignFeaturesToGrid / GetFeaturesInArea(cam, ...)
 *        reference src/Frame.cc:348-395, :574-629                                     -> orbm_frame_create / orbm_features_in_area
 *   ORBmatcher::ComputeThreeMaxima   reference src/ORBmatcher.cc:3948-3989             -> orbm_three_maxima
 *   Tracking::SearchLocalPoints from its second loop on: Frame::isInFrustum + that SearchByProjection
 *        reference src/Tracking.cc:1730-1768, src/Frame.cc:443-499                    -> orbm_points_*, orbm_search_local_points
 *   Tracking::UpdateLocalKeyFrames' votes, Tracking::UpdateLocalPoints and that search over a map resident under stable slots
 *        reference src/Tracking.cc:1838-1855, :1794-1824                              -> orbm_map_*, orbm_local_map_*_host
 *   KeyFrame::UpdateConnections' two counters and LocalMapping::KeyFrameCulling's counts over the same map
 *        reference src/KeyFrame.cc:512-552, src/LocalMapping.cc:990-1032              -> orbm_map_covisibility, orbm_map_culling_counts
 *   MapPoint::ComputeDistinctiveDescriptors + MapPoint::UpdateNormalAndDepth, batched over the points of a keyframe
 *        reference src/MapPoint.cc:325-438, :480-528                                  -> orbm_refresh_points[_host]
 *
 * No Frame* / MapPoint* crosses the ABI: the C++ wrapper (multi_orb_slam_amd/host/ORBmatcher.h) packs flat
 * arrays.  The 3-D projection of map points stays on the host (it is cv::Mat float algebra in the reference,
 * src/ORBmatcher.cc:3513-3528); queries arrive already projected -- except for the local map, whose points can stay in HBM
 * and are projected there (orbm_search_local_points).
 *
 * A matcher handle owns one HIP stream and scratch; use one handle per thread (the reference constructs an
 * ORBmatcher on the stack per use and calls it from three threads).  No global mutable state.
 */
#ifndef ORBM_H
#define ORBM_H
#include "orb_types.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { ORBM_TH_HIGH = 100, ORBM_TH_LOW = 50, ORBM_HISTO_LENGTH = 30 }; /* reference src/ORBmatcher.cc:37-39 */
enum { ORBM_GRID_COLS = 64, ORBM_GRID_ROWS = 48 };                     /* reference include/Frame.h:37-38   */

typedef struct orbm_matcher orbm_matcher;
typedef struct orbm_frame orbm_frame;

int orbm_create(int device, orbm_matcher** out);
void orbm_destroy(orbm_matcher* m);
void* orbm_stream(const orbm_matcher* m);
/* Make the matcher issue all its work on a caller-owned hipStream_t (e.g. orbx_stream(ex), so frame building and
 * matching are ordered after the extractor's kernels without events); NULL restores the matcher's own stream. */
/* Orders this handle's stream behind everything enqueued so far on another HIP stream of the same device (e.g. the
 * stream a collective library ran an all-gather on) without blocking the host. */
int orbm_wait_for_stream(orbm_matcher* m, void* other_stream);
int orbm_set_stream(orbm_matcher* m, void* stream);

/* host helper, identical result to the reference's SWAR popcount; rows need 1-byte alignment only */
int orbm_descriptor_distance(const uint8_t* a, const uint8_t* b);
void orbm_three_maxima(const int* bin_sizes, int L, int* ind3);
/* host: how many top-2 results pass SearchByBoW's acceptance (reference src/ORBmatcher.cc:324-327): best <= th_low and
 * (float)best < ratio * (float)second.  Returns the count (>= 0) or ORB_E_ARG. */
int orbm_count_ratio_accepted(const int32_t* best_dist, const int32_t* second_dist, int n, int th_low, float ratio);

/* Exhaustive top-2 per query over all nr references, strict '<' updates in reference order:
 * best_idx = lowest index attaining the minimum, second_dist = 2nd smallest WITH multiplicity,
 * (-1, 256, 256) when nothing is closer than 256.  Host pointers. */
int orbm_hamming_top2(orbm_matcher* m, const uint8_t* q, int nq, const uint8_t* r, int nr, int32_t* best_idx,
                      int32_t* best_dist, int32_t* second_dist);
/* Same on device pointers, asynchronous on `stream` (a hipStream_t; NULL = default stream).
 * d_scratch: at least orbm_top2_scratch_bytes(nq, nr) bytes of HBM (may be NULL when that returns 0). */
size_t orbm_top2_scratch_bytes(int nq, int nr);
int orbm_hamming_top2_device(const uint8_t* d_q, int nq, const uint8_t* d_r, int nr, int32_t* d_best_idx,
                             int32_t* d_best_dist, int32_t* d_second_dist, void* d_scratch, void* stream);

/* Full nq x nr distance matrix, uint16 row-major (the HBM-write-bound mode). */
int orbm_hamming_matrix(orbm_matcher* m, const uint8_t* q, int nq, const uint8_t* r, int nr, uint16_t* out);
int orbm_hamming_matrix_device(const uint8_t* d_q, int nq, const uint8_t* d_r, int nr, uint16_t* d_out,
                               void* stream);

/* The two all-pairs entry points above compute their distances either with xor + popcount on the vector ALU or, from one
 * tile of work on (>= 64 queries, >= 64 references), as an int8 dot product of the +-1-expanded descriptors on the matrix
 * cores (256 - 2 * distance, exact): same results bit for bit, the second form about 1.4x / 2x faster at 32 000 x 32 000.
 * on = 1 / 0 selects the matrix-core / popcount kernels for the whole process, -1 restores the default (matrix cores).
 * Returns the previous setting.  orbm_top2_scratch_bytes follows it. */
int orbm_use_matrix_cores(int on);
/* The matrix-core form of the top-2 searches (orbm_hamming_top2*, the camera-pair searches of orbm_cross_top2* / orbf_step) has two
 * arithmetic forms of its own: FP4 (the default: descriptor bits as +-4 in E2M1 on gfx950's v_mfma_f32_32x32x64_f8f6f4, twice the
 * int8 rate, the f32 result is the exact integer sort key) and int8 (v_mfma_i32_32x32x32_i8).  Same results bit for bit.
 * on = 1 / 0 selects FP4 / int8 for the whole process, -1 restores the default (FP4 unless MORB_TOP2_FP4=0).  Returns the
 * previous setting. */
int orbm_use_fp4_top2(int on);

/* -- projection-gated search ---------------------------------------------------------------------------- */
typedef struct orbm_frame_desc { /* flat view of the Frame members the matcher reads (src/Frame.cc:191-288) */
    int32_t n_total, n_cams;     /* N_total; global index g: cam-major concatenation (cam 2: g = N + i)      */
    const float* un_x;           /* mvKeysUn_total[g].pt.x                                                   */
    const float* un_y;
    const int32_t* octave;       /* mvKeysUn_total[g].octave                                                 */
    const float* angle;          /* mvKeysUn_total[g].angle                                                  */
    const float* uright;         /* mvuRight_total[g]                                                        */
    const int32_t* cam_of;       /* keypoint_to_cam[g]                                                       */
    const int32_t* local_of;     /* cont_idx_to_local_cam_idx[g]                                             */
    const uint8_t* const* desc;  /* mDescriptors_total[cam], N_cam x 32                                      */
    float min_x, min_y, max_x, max_y; /* mnMinX, mnMinY, mnMaxX, mnMaxY                                      */
} orbm_frame_desc;

typedef struct orbm_query { /* one projected map point */
    float u, v;             /* projection in the current frame                                               */
    float radius;           /* th * mvScaleFactors[octave]                      (src/ORBmatcher.cc:3543)     */
    float ur;               /* u - mbf*invzc  |  mTrackProjXR                   (:3573 | :113); NaN = no right-   */
                            /* coordinate gate (relocalisation :3809-3946 and loop :753-867 overloads have none) */
    int32_t min_level, max_level; /* as handed to GetFeaturesInArea             (:3547-3552 | :89)           */
    int32_t cam;
    int32_t blocks;         /* 1 if the MapPoint has Observations()>0: its claim hides the feature (:3566)   */
    float angle;            /* LastFrame.mvKeysUn_total[i].angle                (:3604)                      */
    uint8_t desc[32];       /* pMP->GetDescriptor()                                                          */
} orbm_query;

/* Host-only convenience for synthetic streams and tests: the last frame's features become projected map points under
 * a constant image-plane motion (du, dv): u = x + du, v = y + dv, radius = th * scale_factors[octave],
 * ur = u - mbf / depth (u where depth <= 0), levels octave-1 .. octave+1, blocks = 1, angle/desc copied.  A SLAM
 * caller computes the same fields from its 3-D map points instead (reference src/ORBmatcher.cc:3502-3552). */
int orbm_queries_from_motion(const orb_keypoint* kps, const uint8_t* desc, const float* depth, const int32_t* cam_of, int n,
                             float du, float dv, float th, const float* scale_factors, float mbf, orbm_query* out,
                             const float* un_x, const float* un_y); /* undistorted positions, or NULL, NULL: kps[i].x/y */

/* Frame::UndistortKeyPoints / ComputeImageBounds (reference src/Frame.cc:673-778) = cv::undistortPoints(pts, K, dist,
 * noArray(), K) of OpenCV 2.4.x / 3.2, host side (the same operation sequence the kernels run).  calib == NULL or
 * k1 == 0: plain copy / (0, 0, cols, rows), as in the reference.  out4 = {minX, minY, maxX, maxY}. */
int orbm_undistort_points(const orb_calibration* calib, const float* x, const float* y, int n, float* ux, float* uy);
int orbm_image_bounds(const orb_calibration* calib, int cols, int rows, float* out4);
/* Calibration applied by the frames this handle assembles ON THE DEVICE from now on (orbm_frame_from_device): positions
 * are undistorted before grid assignment and uRight, the depth image is still read at the distorted pixel
 * (src/Frame.cc:968-981).  The caller passes matching bounds (orbm_image_bounds).  NULL switches it off. */
int orbm_set_calibration(orbm_matcher* m, const orb_calibration* calib);

/* Builds the 64x48 per-camera grid (round-to-cell insertion, ascending global indices) and uploads the frame. */
int orbm_frame_create(orbm_matcher* m, const orbm_frame_desc* f, orbm_frame** out);

/* orbm_frame_create for a frame whose descriptors are (partly) still in HBM: for every camera c with d_desc[c] != NULL the rows
 * N_c x 32 are read from that DEVICE pointer (16-byte aligned; e.g. orbx_device_descriptors of the extraction that produced
 * the frame -- the caller guarantees they hold what f->desc[c] holds and stay unchanged until the frame's first search has
 * returned); the other cameras' rows are taken from f->desc[c] as usual.  The 64x48 grid is built on the device (same
 * round-to-cell arithmetic), nothing but x, y, uright, angle, octave and one index word per feature crosses the bus.
 * d_desc == NULL: every camera from the host.  f->desc must be valid for every camera in any case: frames beyond 8192
 * features or 4 cameras, and MORB_RESIDENT_FRAMES=0, take orbm_frame_create. */
int orbm_frame_create_resident(orbm_matcher* m, const orbm_frame_desc* f, const uint8_t* const* d_desc, orbm_frame** out);

/* Frame assembly ON THE DEVICE from HBM-resident extractor outputs -- the merge of reference src/Frame.cc:191-239,
 * ComputeStereoFromRGBD (:959-986: depth lookup at (int)kp.pt.y,(int)kp.pt.x, uRight = x - mbf/d, -1 where d <= 0) and
 * AssignFeaturesToGrid (:348-395) -- with no host round trip.  Undistortion is the identity (k1 == 0, :676-680).
 * Everything is enqueued on the matcher's stream; the inputs must stay valid until that work has run. */
typedef struct orbm_cam_features {
    const orb_keypoint* d_kps; /* device, n keypoints (e.g. orbx_device_keypoints)                               */
    const uint8_t* d_desc;     /* device, n x 32                                                                 */
    int32_t n;
    const float* d_depth;      /* device depth image in metres (imDepth after convertTo), or NULL: uRight = -1   */
    int32_t depth_stride;      /* floats per row                                                                 */
} orbm_cam_features;
int orbm_frame_from_device(orbm_matcher* m, const orbm_cam_features* cams, int n_cams, float mbf, float min_x,
                           float min_y, float max_x, float max_y, orbm_frame** out);
/* Host copies of a frame's merged arrays (any pointer may be NULL): keypoints and descriptors in global (cam-major)
 * order, mvuRight_total, mvDepth_total.  Synchronises the matcher's stream. */
int orbm_frame_download(orbm_matcher* m, const orbm_frame* f, orb_keypoint* kps, uint8_t* desc, float* uright,
                        float* depth);
int orbm_frame_count(const orbm_frame* f);

/* Cross-camera exhaustive top-2 in one launch: every feature g of the frame against all features of the OTHER
 * cameras (reference analogue: the unrestricted inner loop of src/ORBmatcher.cc:287-321).  best_idx indexes the
 * concatenation of the other cameras' features in camera order; outputs have n_total entries (host pointers). */
int orbm_cross_top2(orbm_matcher* m, const orbm_frame* f, int32_t* best_idx, int32_t* best_dist,
                    int32_t* second_dist);
/* Same over a list of HBM-resident descriptor blocks, one per camera of the whole rig in global camera order (e.g. the
 * slices of an RCCL all-gather receive buffer): the cameras [first_query_block, +n_query_blocks) are the queries (the
 * ones this process owns), every other block is a reference.  Outputs hold sum(counts[query blocks]) entries. */
int orbm_cross_top2_blocks(orbm_matcher* m, const uint8_t* const* d_desc_blocks, const int* counts, int n_blocks,
                           int first_query_block, int n_query_blocks, int32_t* best_idx, int32_t* best_dist,
                           int32_t* second_dist);

/* Multi-GPU form of orbm_cross_top2_blocks: `d_gathered` is the result of ONE all-gather of every rank's export block
 * (orbf_export_block: cap_rows descriptor rows, the rank's cameras packed back to back, followed by a trailer of int32
 * per-camera counts), `world` blocks of `block_bytes` in rank order.  Queries = the features of rank `rank`, candidates =
 * every other camera of the rig; indices as in orbm_cross_top2 (position in the concatenation of the other cameras, global
 * camera order).  Nothing about the counts has to be known on the host beforehand: counts_out[world * cams_per_rank]
 * (may be NULL) and *nq_out are filled from the gathered trailers; the result arrays need room for cap_rows entries. */
int orbm_cross_top2_gathered(orbm_matcher* m, const uint8_t* d_gathered, int world, size_t block_bytes, int cap_rows,
                             int cams_per_rank, int rank, int32_t* best_idx, int32_t* best_dist, int32_t* second_dist,
                             int32_t* counts_out, int* nq_out);
/* The same in two halves, for a caller that overlaps the exchange with an orbf_step in flight (orbf_step_begin reported
 * the export block ready): _enqueue puts repack + top-2 on this handle's side stream -- behind `after_stream`, the stream
 * the all-gather was enqueued on, when wait_after != 0 (NULL then means the default stream) -- and joins it into the
 * handle's main stream; after that stream has been synchronised (orbf_step_end does) _collect copies the results out. */
int orbm_cross_top2_gathered_enqueue(orbm_matcher* m, const uint8_t* d_gathered, int world, size_t block_bytes, int cap_rows,
                                     int cams_per_rank, int rank, void* after_stream, int wait_after);
/* (collect: the three result pointers may all be NULL when the caller reads the results in place through _views: pinned
 * host arrays of *nq_out entries, valid until the next cross-camera search of this matcher) */
int orbm_cross_top2_gathered_views(orbm_matcher* m, const int32_t** best_idx, const int32_t** best_dist, const int32_t** second_dist);
int orbm_cross_top2_gathered_collect(orbm_matcher* m, int32_t* best_idx, int32_t* best_dist, int32_t* second_dist,
                                     int32_t* counts_out, int* nq_out);
void orbm_frame_destroy(orbm_frame* f);
/* grid as CSR: cell = (cam*64 + ix)*48 + iy; cell_start has n_cams*3072+1 entries */
int orbm_frame_grid(const orbm_frame* f, int32_t* cell_start, int32_t* items);
/* GetFeaturesInArea(cam, x, y, r, minLevel, maxLevel) on the GPU; returns count in *n (may exceed cap) */
int orbm_features_in_area(orbm_matcher* m, const orbm_frame* f, int cam, float x, float y, float r,
                          int min_level, int max_level, int32_t* out, int cap, int* n);

/* Ordered candidate lists: for query i, cand_count[i] candidates in the reference's visiting order
 * (ix, iy, ascending index) that pass the window/level/right-coordinate gates, with their distances.
 * Lists are stored at [i*cap_per_query ...]; a count above cap_per_query => ORB_E_CAPACITY. */
int orbm_project_candidates(orbm_matcher* m, const orbm_frame* f, const orbm_query* q, int nq, int cap_per_query,
                            int32_t* cand_idx, uint16_t* cand_dist, int32_t* cand_count);

/* (inspection and timing hooks -- orbm_debug_*: include/orb_debug.h) */

/* SearchByProjection(CurrentFrame, LastFrame, th, bMono, Calib) from the projected queries on.
 * occupied[g] != 0 where CurrentFrame.mvpMapPoints[g] already holds an observed point before the call (may be NULL:
 * TrackWithMotionModel clears the vector first, reference src/Tracking.cc:1254).
 * match_of_feature[g]: >= 0 = index of the query whose MapPoint ends in CurrentFrame.mvpMapPoints[g]; -1 = untouched;
 * -2 = set to NULL by the rotation-histogram filter (reference src/ORBmatcher.cc:3631).
 * *nmatches = the reference's return value. */
int orbm_search_by_projection(orbm_matcher* m, const orbm_frame* cur, const orbm_query* q, int nq,
                              const uint8_t* occupied, int th_high, int check_orientation,
                              int32_t* match_of_feature, int* nmatches);

/* The two-camera loop-closing search, SearchByProjection(KeyFrame*, Scw, vpPoints, vLoopMPCams, vpMatched, th, Calib)
 * (reference src/ORBmatcher.cc:566-750): every point is projected into BOTH cameras of the keyframe; the candidates of the
 * camera-2 window follow those of the camera-1 window (the reference's `for camidx` loop), ONE strict `<` chain runs over both,
 * and an accepted match (<= th_high = TH_LOW there) hides its feature from the later points (vpMatched[idx]).  q[i] holds
 * the first window (q[i].cam < 0: the point is not visible in that camera), second[i] the other one (cam < 0: none); the
 * descriptor, `blocks` and `angle` come from q[i].  Everything else as orbm_search_by_projection. */
typedef struct orbm_window {
    float u, v, radius;
    int32_t cam;                  /* < 0: no window */
    int32_t min_level, max_level; /* level gate of this window, as in orbm_query */
} orbm_window;
int orbm_search_by_projection_windows(orbm_matcher* m, const orbm_frame* cur, const orbm_query* q, const orbm_window* second,
                                      int nq, const uint8_t* occupied, int th_high, int check_orientation,
                                      int32_t* match_of_feature, int* nmatches);

/* The inner loop the remaining projection searches share: every projected point scans its window
 * -- same cell walk and level gate as above -- and reports the FIRST candidate in visiting order with the smallest
 * distance (`if(dist<bestDist)`), independently of every other point: no claims between queries.
 *   SearchBySim3 (reference src/ORBmatcher.cc:2814-3135, each direction): gate NONE, caller accepts <= TH_HIGH
 *   Fuse x2 (:1986-2509): gate CHI2 = the reprojection-error test of :2118-2143 (7.8 with a right coordinate, 5.99
 *     without; q.ur = projected right coordinate), levels nPredictedLevel-1 .. nPredictedLevel, caller accepts <= TH_LOW
 *     and then merges / replaces map points on the host as the reference does
 * occupied[g] != 0 hides feature g (may be NULL).  best_idx[i] = -1 / best_dist[i] = 256 when the window holds nothing. */
enum { ORBM_GATE_NONE = 0, ORBM_GATE_RIGHT = 1, ORBM_GATE_CHI2 = 2 };
int orbm_project_best(orbm_matcher* m, const orbm_frame* f, const orbm_query* q, int nq, const uint8_t* occupied, int gate,
                      const float* inv_level_sigma2, int n_levels, int32_t* best_idx, int32_t* best_dist);

/* SearchByProjection(F, vpMapPoints, th): camera-1 grid only, top-2 with level bookkeeping and nnratio.
 * occupied[g] != 0 where F.mvpMapPoints[g] already holds an observed point (may be NULL). */
int orbm_search_by_projection_points(orbm_matcher* m, const orbm_frame* cur, const orbm_query* q, int nq,
                                     const uint8_t* occupied, float nnratio, int th_high,
                                     int32_t* match_of_feature, int* nmatches);

/* -- local-map tracking: Frame::isInFrustum fused with the search ---------------------------------------------
 * Tracking::SearchLocalPoints from its second loop on (reference src/Tracking.cc:1730-1768): Frame::isInFrustum
 * (src/Frame.cc:443-499) per point, MapPoint::PredictScale (src/MapPoint.cc:602-617), the query of
 * SearchByProjection(F, vpMapPoints, th) (src/ORBmatcher.cc:62-157) and its top-2 search, over a table of map points that
 * stays in HBM between frames.  Neither the points nor the queries cross the bus per frame: the caller rewrites the rows
 * that changed (orbm_points_write) and hands in the pose. */
typedef struct orbm_points orbm_points;

typedef struct orbm_point {        /* what isInFrustum and the search read of one MapPoint */
    float pos[3];                  /* GetWorldPos()                                        */
    float normal[3];               /* GetNormal()                                          */
    float min_dist, max_dist;      /* mfMinDistance, mfMaxDistance (NOT yet * 0.8 / 1.2)   */
    int32_t blocks;                /* Observations() > 0                                   */
    uint8_t desc[32];              /* GetDescriptor()                                      */
} orbm_point;                      /* 68 bytes */

typedef struct orbm_view {         /* the Frame members isInFrustum reads */
    float Rcw[9], tcw[3], Ow[3];   /* mRcw row-major, mtcw, mOw                            */
    float fx, fy, cx, cy, mbf;
    float min_x, max_x, min_y, max_y;
    float viewing_cos_limit;       /* 0.5 in SearchLocalPoints                             */
    float th;                      /* SearchByProjection's th (1, 3 or 5)                  */
    float log_scale_factor; int32_t n_levels;   /* mfLogScaleFactor, mnScaleLevels (1 .. ORBM_MAX_LEVELS) */
    const float* scale_factors;    /* mvScaleFactors, n_levels (host)                      */
} orbm_view;

typedef struct orbm_track {        /* what isInFrustum leaves in the MapPoint */
    float proj_x, proj_y, proj_xr, view_cos;   /* mTrackProjX, mTrackProjY, mTrackProjXR, mTrackViewCos */
    int32_t level;                 /* mnTrackScaleLevel                                    */
    int32_t in_view;               /* mbTrackInView; 0 also for skipped points (the other fields are 0 then) */
} orbm_track;

enum { ORBM_MAX_LEVELS = 32, ORBM_MAX_POINTS = 65535 };

int orbm_points_create(orbm_matcher* m, int capacity, orbm_points** out);
void orbm_points_destroy(orbm_points* p);
/* rows [first, first + n) of the table; any sub-range inside the capacity.  Returns when the rows are in HBM. */
int orbm_points_write(orbm_matcher* m, orbm_points* p, int first, int n, const orbm_point* src);
int orbm_points_count(const orbm_points* p);   /* high-water mark: one past the last row ever written */
/* Frustum test, scale prediction, query construction and the top-2 search of the first n rows of the table against `cur`.
 * skip[i] != 0 (n entries, may be NULL) is the reference's `mnLastFrameSeen == mnId || isBad()`: the point is neither tested
 * nor searched.  occupied / nnratio / th_high as in orbm_search_by_projection_points.  track (n entries, may be NULL)
 * receives what isInFrustum writes; match_of_feature[g] is an index into the TABLE (0 .. n-1) or -1; *n_to_match = points
 * that passed the test (the reference's nToMatch); *nmatches = SearchByProjection's return value.  Points claim in table
 * order.  n beyond orbm_points_count or ORBM_MAX_POINTS: ORB_E_CAPACITY.
 * One deviation from the reference: a non-finite projection (PcZ == 0) is out of view; the reference lets it through its
 * bound checks into an int cast. */
int orbm_search_local_points(orbm_matcher* m, const orbm_frame* cur, const orbm_points* pts, int n, const orbm_view* view,
                             const uint8_t* skip, const uint8_t* occupied, float nnratio, int th_high, orbm_track* track,
                             int32_t* match_of_feature, int* n_to_match, int* nmatches);
/* (test / inspection hooks, like orbm_debug_*: not needed by a caller of orbm_search_local_points)
 * Host: the level thresholds the kernel uses in place of a logarithm.  out[k], k = 0 .. n_levels-2, is the largest float
 * ratio r with ceil(logf(r) / log_scale_factor) <= k under the C library's logf; the predicted level of a ratio is the number
 * of thresholds it exceeds.  Verifies that the predicate flips exactly once around every threshold; ORB_E_ARG otherwise. */
int orbm_level_thresholds(float log_scale_factor, int n_levels, float* out);
/* (test / inspection hook) Host: the same arithmetic as the kernel, operation for operation, for n points in host memory (the exact fallback of the
 * search uses it; a test can hold it against a model without a device).  track and q (n entries each, either may be NULL):
 * q[i] is the query of point i, with cam = -1 (no window) where the point is not in view. */
int orbm_frustum_host(const orbm_point* pts, int n, const orbm_view* view, const uint8_t* skip, orbm_track* track,
                      orbm_query* q, int* n_to_match);

/* -- the local map on the device: Tracking::UpdateLocalMap over a resident map ----------------------------------
 * A map that stays in HBM under stable slots -- one per map point, one per keyframe, one per observation -- and the three calls
 * of Tracking::TrackLocalMap's first half over it (reference src/Tracking.cc:1794-1949, :1730-1768):
 *   orbm_map_vote                 the keyframe votes of UpdateLocalKeyFrames (:1838-1855): one stream over the observation records
 *   orbm_map_local_points         UpdateLocalPoints (:1794-1824): a gather over the local keyframes' rows, de-duplicated in order
 *   orbm_map_search_local_points  orbm_search_local_points over the list the call before left on the device
 * What is sequential pointer logic (K1 in std::map order, the K2 walk with its marks) stays with the caller, where the graph
 * lives.  A point's row is sent when the point changes (orbm_map_write_points), never because its place in a list moved.
 * The object keeps a host mirror of everything it holds; every call runs on the handle's stream and synchronises it once. */
typedef struct orbm_map orbm_map;
typedef struct { int32_t point, keyframe; } orbm_obs;   /* one observation; point == -1: a free record */
enum { ORBM_MAP_MAX_KEYFRAMES = 16384, ORBM_MAP_MAX_FEATURES = 8192, ORBM_MAP_MAX_LOCAL = 4096 };
enum { ORBM_POINT_BAD = 1 };   /* bit 0 of a point's flag byte: MapPoint::isBad() */

/* kf_capacity 1 .. ORBM_MAP_MAX_KEYFRAMES, features_per_keyframe 1 .. ORBM_MAP_MAX_FEATURES (the stride of a keyframe's row);
 * point_capacity and obs_capacity >= 0, bounded by memory alone.  Everything starts empty: rows of zeros that are not bad, free
 * records, keyframes without points. */
int orbm_map_create(orbm_matcher* m, int kf_capacity, int point_capacity, int obs_capacity, int features_per_keyframe, orbm_map** out);
void orbm_map_destroy(orbm_map* map);
/* Point slots slots[0 .. n): row rows[i] and flag byte flags[i] (flags == NULL: 0) into slot slots[i].  A slot named twice takes
 * its last entry.  One synchronisation; returns when the rows are in HBM.  A slot outside the capacity: ORB_E_CAPACITY, nothing written. */
int orbm_map_write_points(orbm_matcher* m, orbm_map* map, const int32_t* slots, int n, const orbm_point* rows, const uint8_t* flags);
/* Record slots slots[0 .. n).  records[i].point is a point slot or -1 (free), .keyframe a keyframe slot (ignored in a free
 * record).  AT MOST ONE LIVE RECORD PER (point, keyframe), as std::map<KeyFrame*, size_t> guarantees: this is the caller's to
 * keep and is not checked -- a pair held twice votes twice.  The keyframe high-water mark covers every keyframe a record names. */
int orbm_map_write_observations(orbm_matcher* m, orbm_map* map, const int32_t* slots, int n, const orbm_obs* records);
/* Keyframe slot kf: mvpMapPoints as point slots (-1 = none), n_features <= features_per_keyframe entries, and isBad(). */
int orbm_map_write_keyframe(orbm_matcher* m, orbm_map* map, int kf, const int32_t* point_of_feature, int n_features, int bad);
int orbm_map_set_keyframe_bad(orbm_matcher* m, orbm_map* map, int kf, int bad);   /* the flag alone (host mirror: no kernel reads it) */
int orbm_map_keyframes(const orbm_map* map);   /* keyframe high-water mark: one past the last keyframe slot written or named by a record */
int orbm_map_keyframe_bad(const orbm_map* map, int kf);

/* votes[k], k < orbm_map_keyframes(map): the sum over the features f with frame_points[f] >= 0 and the point not bad of
 * [a live record (frame_points[f], k) exists] -- keyframeCounter of :1838-1855; a point that sits at two features votes twice.  Bad
 * keyframes are counted; the caller drops them (:1875).  frame_points[f] is a point slot or negative. */
int orbm_map_vote(orbm_matcher* m, orbm_map* map, const int32_t* frame_points, int n_features, int32_t* votes);
/* The candidates are the entries of the rows of local_kfs[0 .. n_local), n_local <= ORBM_MAP_MAX_LOCAL, in the order (position in
 * local_kfs, feature index).  A candidate is kept if its slot is not negative, the point is not bad and no earlier candidate
 * holds the same point.  list (room for ORBM_MAX_POINTS entries) receives the kept slots in order, *n_list their number; the list
 * also stays on the device for orbm_map_search_local_points.  More than ORBM_MAX_POINTS kept points: ORB_E_CAPACITY, and no
 * list is left.
 * One deviation from the reference: its mark mnTrackReferenceForFrame survives between calls, so a second UpdateLocalPoints for the
 * same frame id yields an empty list there.  Here every call starts unmarked. */
int orbm_map_local_points(orbm_matcher* m, orbm_map* map, const int32_t* local_kfs, int n_local, int32_t* list, int* n_list);
/* orbm_search_local_points over the list of the last orbm_map_local_points: point i of the search is the point in slot list[i];
 * track (n_list entries, may be NULL) and match_of_feature index the LIST.  The skip flag is built on the device: a point is
 * skipped if it is bad, if it is one of frame_points[0 .. n_features) whose point is not bad (the frame's own points, Tracking.cc
 * :1735-1750) or if it is one of seen[0 .. n_seen) (mnLastFrameSeen as TrackWithMotionModel sets it at :1310).  Everything else as
 * in orbm_search_local_points, the deviation included. */
int orbm_map_search_local_points(orbm_matcher* m, const orbm_frame* cur, orbm_map* map, const orbm_view* view,
                                 const int32_t* frame_points, int n_features, const int32_t* seen, int n_seen,
                                 const uint8_t* occupied, float nnratio, int th_high, orbm_track* track, int32_t* match_of_feature,
                                 int* n_to_match, int* nmatches);
/* Host, on plain arrays, no device and no handle: the fallback and the cross-check of the two calls above.
 * obs[0 .. n_obs) records (free ones included), point_flags[0 .. n_points), votes[0 .. n_kfs).  A record whose point or keyframe
 * lies outside those counts: ORB_E_ARG. */
int orbm_local_map_vote_host(const orbm_obs* obs, int n_obs, const uint8_t* point_flags, int n_points, const int32_t* frame_points,
                             int n_features, int n_kfs, int32_t* votes);
/* kf_rows[k * stride + f], f < kf_count[k], the rows of n_kfs keyframes; list has room for list_cap entries; *n_list is the number
 * kept even when it exceeds list_cap (ORB_E_CAPACITY then, the first list_cap entries written). */
int orbm_local_map_points_host(const int32_t* kf_rows, const int32_t* kf_count, int n_kfs, int stride, const uint8_t* point_flags,
                               int n_points, const int32_t* local_kfs, int n_local, int32_t* list, int list_cap, int* n_list);

/* -- covisibility on the device: KeyFrame::UpdateConnections' counters and LocalMapping::KeyFrameCulling's counts ----------
 * The two routines of the LocalMapping and LoopClosing threads that walk keyframe -> map points -> observations and count
 * (reference src/KeyFrame.cc:512-552, src/LocalMapping.cc:990-1032), over the same resident map.  The map learns four more facts,
 * all additive: what the calls above read and return is untouched by them.
 *   per record    the feature index of the observation in its keyframe (mObservations[pKF]); a record never written holds 0
 *   per keyframe  one byte per feature -- bits 0-4 mvKeysUn_total[i].octave, bit 7 (ORBM_FEATURE_FAR) the HOST's float evaluation
 *                 of `mvDepth_total[i] > mThDepth || mvDepth_total[i] < 0` -- and N, the camera-1 feature count; never written: zeros
 *   per point     n_obs, what MapPoint::Observations() returns (mirrored as a value, not recomputed); never written: 0
 *   an index      from a point to its live records: a chain head[point], next[record], built on the device by the first counting
 *                 call after any orbm_map_write_observations.  A record's place in its chain is arbitrary from build to build:
 *                 NOTHING THAT DEPENDS ON CHAIN ORDER IS EVER READ OUT OF IT -- both calls below only count.
 * Integer counting only: the device's results are exact whatever order the lanes arrive in. */
enum { ORBM_FEATURE_LEVEL_MASK = 0x1f, ORBM_FEATURE_FAR = 0x80 };
typedef struct { int32_t keyframe, all, cam1; } orbm_covis_entry;
/* feature[i], in 0 .. features_per_keyframe-1, into record slot slots[i].  Outside: ORB_E_ARG / ORB_E_CAPACITY, nothing written. */
int orbm_map_write_observation_features(orbm_matcher* m, orbm_map* map, const int32_t* slots, int n, const int32_t* feature);
/* Keyframe slot kf: feature_bytes[0 .. n_features) (the rest of the row becomes 0) and n_cam1 in 0 .. features_per_keyframe. */
int orbm_map_write_keyframe_features(orbm_matcher* m, orbm_map* map, int kf, const uint8_t* feature_bytes, int n_features, int n_cam1);
int orbm_map_write_point_nobs(orbm_matcher* m, orbm_map* map, const int32_t* slots, int n, const int32_t* n_obs);
/* For keyframe k = kfs[j], j < n <= ORBM_MAP_MAX_LOCAL (src/KeyFrame.cc:512-552):
 *   for i in 0 .. kf_count[k]-1:  p = row[k][i];  skip p < 0;  skip bad(p)
 *     for every live record r of p with r.keyframe != k:
 *       all[r.keyframe] += 1
 *       if i < n_cam1[k] and feature(r) < n_cam1[r.keyframe]:  cam1[r.keyframe] += 1
 * The entries with all > 0, in ascending keyframe slot, are entries[first_out[j] .. first_out[j+1]-1]; first_out has n + 1 entries.
 * A point at two features of k counts twice; bad keyframes are counted; a keyframe named twice gets two equal lists.  The device
 * keeps both counters of a keyframe in one 32-bit bin, which holds as long as a count stays below 65 536: it cannot exceed the
 * length of a row while the map keeps to one live record per (point, keyframe) (orbm_map_write_observations).  More entries
 * than entries_cap: ORB_E_CAPACITY, first_out[n] (and the error text) the number needed, first_out[0 .. n) zero, no list. */
int orbm_map_covisibility(orbm_matcher* m, orbm_map* map, const int32_t* kfs, int n, int32_t* first_out, orbm_covis_entry* entries,
                          int entries_cap);
/* counts_out[2 j], counts_out[2 j + 1] = nMPs, nRedundantObservations of keyframe kfs[j] (src/LocalMapping.cc:990-1032):
 *   for i in 0 .. kf_count[k]-1:  p = row[k][i];  skip p < 0;  skip bad(p);  skip far(k, i) unless mono
 *     nMPs += 1
 *     if n_obs[p] > 3:
 *       c = #{ live records r of p : r.keyframe != k  and  level(r.keyframe, feature(r)) <= level(k, i) + 1 }
 *       if c >= 3: nRedundant += 1
 * (the reference's break at the third hit is an early exit only: c >= 3 does not depend on the order of the observations.) */
int orbm_map_culling_counts(orbm_matcher* m, orbm_map* map, const int32_t* kfs, int n, int mono, int32_t* counts_out);
/* Host, on plain arrays: the fallback (MORB_HOST_RESOLVE=1, over the mirror), the route of a map without a device and the
 * cross-check of the two calls above.  obs_feature[i] belongs to obs[i]; kf_feature_bytes[k * stride + f]; a record or a row entry
 * outside the counts given: ORB_E_ARG.  The covisibility routine writes the first entries_cap entries when there are more. */
int orbm_local_map_covisibility_host(const orbm_obs* obs, const int32_t* obs_feature, int n_obs, const uint8_t* point_flags, int n_points,
                                     const int32_t* kf_rows, const int32_t* kf_count, const int32_t* kf_n_cam1, int n_kfs, int stride,
                                     const int32_t* kfs, int n, int32_t* first_out, orbm_covis_entry* entries, int entries_cap);
int orbm_local_map_culling_host(const orbm_obs* obs, const int32_t* obs_feature, int n_obs, const uint8_t* point_flags,
                                const int32_t* point_n_obs, int n_points, const int32_t* kf_rows, const int32_t* kf_count,
                                const uint8_t* kf_feature_bytes, int n_kfs, int stride, const int32_t* kfs, int n, int mono,
                                int32_t* counts_out);

/* -- loop correction over the resident map: LoopClosing::CorrectLoop's point pass and the update after global BA ----------
 * The two passes of the LoopClosing thread that move map points one cv::Mat at a time (reference src/LoopClosing.cc:678-722 and
 * :953-989), in place over the same resident map: after either only the 12 position bytes of a corrected point's row differ, so the
 * rows are changed where they lie, in HBM and in the mirror, and no row crosses the bus.  Everything here is additive: what the calls
 * above read and return is untouched.  The map learns one more fact per point: the keyframe slot of mpRefKF (never written: -1).
 * A Sim3 is 8 doubles in the layout of orbm_eg_problem::vertex: quaternion x y z w, translation, scale.
 * Every device call runs on the handle's stream and synchronises it once.  All arithmetic is + - * / in IEEE double and float without
 * contraction, the same statements on the device and in the host routines; what a NaN, infinite or subnormal INPUT gives is not
 * specified bit for bit. */
typedef struct { int32_t point, position; } orbm_correct_entry;   /* a corrected point's slot and the position in kfs of its claimant */
int orbm_map_points(const orbm_map* map);   /* point high-water mark: one past the last point slot ever written */
/* The position field alone of point slots slots[0 .. n): pos3[3 i ..] into slot slots[i], HBM and mirror.  A slot named twice takes its
 * last entry.  A slot outside the capacity: ORB_E_CAPACITY, nothing written.  For callers that already hold the new positions
 * (orbm_eg_result::point_f, SetWorldPos(mPosGBA)). */
int orbm_map_write_positions(orbm_matcher* m, orbm_map* map, const int32_t* slots, int n, const float* pos3);
/* ref_kf[i], the keyframe slot of GetReferenceKeyFrame() (any value; one outside the keyframes given to orbm_map_correct_rigid reads as
 * "not corrected"), into point slot slots[i].  Shape and errors of orbm_map_write_point_nobs. */
int orbm_map_write_point_ref(orbm_matcher* m, orbm_map* map, const int32_t* slots, int n, const int32_t* ref_kf);
/* CorrectLoop's step 4.2 (:678-710) and the poses of step 4.3 (:714-720).  kfs[0 .. n), n <= ORBM_MAP_MAX_LOCAL, are keyframe slots in
 * CorrectedSim3's iteration order, sim3_before[8 j ..] = NonCorrectedSim3 and sim3_after[8 j ..] = CorrectedSim3 of kfs[j]; already[0 ..
 * n_already) are the point slots the reference would skip at :696 (negative entries are ignored).
 * The candidates are the row entries of the listed keyframes in the order (position in kfs, feature index), as in
 * orbm_map_local_points.  A candidate is kept if its slot is not negative, the point is not bad, the point is not in `already` and no
 * earlier candidate holds the same point.  A kept candidate at position j moves its point (:701-705):
 *   P = (double)pos;  w = after[j].inverse().map(before[j].map(P));  pos = (float)w, component by component
 * (Sim3::map and Sim3::inverse of Thirdparty/g2o/g2o/types/sim3.h; the one definition the essential graph's step 7 runs.)
 * entries[i] = {point slot, j} and pos_out[3 i ..] the new position, in candidate order; *n_out the number kept; the position field of
 * every kept point's row is the new one, in HBM and in the mirror.  Tiw_out[16 j ..] is the float 4x4 SetPose receives (:714-720):
 * toRotationMatrix, t * (1./s), toCvSE3 of after[j] (computed on the host).  entries, pos_out (cap entries) and Tiw_out (n) may not be NULL
 * unless cap / n is 0.
 * More than cap kept: ORB_E_CAPACITY, *n_out (and the error text) the number needed, and NO row and no mirror entry has changed (the
 * reference has no such limit; a caller repeats the call with room).  The list is not bound by ORBM_MAX_POINTS.  Every call starts
 * unmarked, and the list orbm_map_local_points left for orbm_map_search_local_points is not disturbed. */
int orbm_map_correct_sim3(orbm_matcher* m, orbm_map* map, const int32_t* kfs, int n, const double* sim3_before, const double* sim3_after,
                          const int32_t* already, int n_already, orbm_correct_entry* entries, float* pos_out, int cap, int* n_out,
                          float* Tiw_out);
/* RunGlobalBundleAdjustment's step 2 (:953-989) over point slots slots[0 .. n), all distinct (a slot named twice: ORB_E_ARG);
 * slots == NULL: every point slot below the high-water mark, and n must be orbm_map_points(map).  kf_corrected[r] != 0 says
 * mnBAGlobalForKF == nLoopKF of keyframe slot r < n_kfs; Tcw_before[12 r ..] and Twc_after[12 r ..] are rows 0-2 of its mTcwBefGBA and of
 * its GetPoseInverse(); gba_slots[0 .. n_gba) are the points with mnBAGlobalForKF == nLoopKF and gba_pos[3 g ..] their mPosGBA (a slot
 * named twice takes its last entry; negative entries are ignored).  Per point, in this order:
 *   1. bad: untouched, status 0
 *   2. listed in gba_slots: the position becomes the given 12 bytes, status 1
 *   3. r = ref_kf[slot]; r < 0, r >= n_kfs or !kf_corrected[r]: untouched, status 0
 *   4. Xc = Rcw_before[r]*P + tcw_before[r], pos = Rwc_after[r]*Xc + twc_after[r], each one cv::gemm on its small path with
 *      alpha = beta = 1 (float products and sums left to right, one double step), status 2
 * status (n bytes) and pos_out (3 n floats: the position the row holds after the call) may be NULL.  Rows and mirror change in place. */
int orbm_map_correct_rigid(orbm_matcher* m, orbm_map* map, const int32_t* slots, int n, const uint8_t* kf_corrected,
                           const float* Tcw_before, const float* Twc_after, int n_kfs, const int32_t* gba_slots, const float* gba_pos,
                           int n_gba, uint8_t* status, float* pos_out);
/* Host, on plain arrays, no device and no handle: the fallback (MORB_HOST_RESOLVE=1, over the mirror), the route of a map without a
 * device and the cross-check of the two calls above.  pos[pos_stride * slot + k], k < 3, is the position of a point (pos_stride 3: a
 * packed array; 17: the rows of orbm_point), read and written in place; kf_rows / kf_count as in orbm_local_map_points_host.  A row
 * entry, a listed slot or a keyframe outside the counts given: ORB_E_ARG.  The Sim3 routine counts first: beyond cap it returns
 * ORB_E_CAPACITY with *n_out the number needed and nothing changed. */
int orbm_local_map_correct_sim3_host(const int32_t* kf_rows, const int32_t* kf_count, int n_kfs, int stride, const uint8_t* point_flags,
                                     float* pos, int pos_stride, int n_points, const int32_t* kfs, int n, const double* sim3_before,
                                     const double* sim3_after, const int32_t* already, int n_already, orbm_correct_entry* entries,
                                     float* pos_out, int cap, int* n_out, float* Tiw_out);
int orbm_local_map_correct_rigid_host(float* pos, int pos_stride, const uint8_t* point_flags, const int32_t* point_ref, int n_points,
                                      const int32_t* slots, int n, const uint8_t* kf_corrected, const float* Tcw_before,
                                      const float* Twc_after, int n_kfs, const int32_t* gba_slots, const float* gba_pos, int n_gba,
                                      uint8_t* status, float* pos_out);

/* -- map-point refresh: distinctive descriptor, normal, depth --------------------------------------------------
 * The producer of what an orbm_point row holds beyond the position: MapPoint::ComputeDistinctiveDescriptors (reference
 * src/MapPoint.cc:325-438) and MapPoint::UpdateNormalAndDepth (:480-528), which the reference calls for every point of every
 * new keyframe, as ONE batched call over P points whose observations arrive as a CSR list (point p owns the observations
 * first[p] .. first[p+1]-1, in the iteration order of its std::map<KeyFrame*, size_t>).  Two jobs per point, selected by what[p]:
 *   ORBM_REFRESH_DESCRIPTOR    among the observations flagged alive (the reference skips pKF->isBad() here and only here), in
 *                              list order: d[i][j] = 256-bit Hamming distance, median_i = element (int)(0.5*(N-1)) of row i sorted
 *                              ascending (the row includes d[i][i] = 0), winner = the first i with the least median.
 *   ORBM_REFRESH_NORMAL_DEPTH  over ALL observations, in list order: normal = mean of the unit vectors pos - obs_centre, in the
 *                              number formats of the reference's cv::Mat statements (float subtraction, cv::norm in double,
 *                              (float)(1/norm) weight, a sequential float sum, one (float)(1/n) scale); dist = (float)norm(pos -
 *                              ref_centre), max_dist = dist * scale_factors[ref_level], min_dist = max_dist / scale_factors[n_levels-1].
 * A NaN result (a centre equal to the position) is written as 0xffc00000, the NaN x86 produces from an invalid operation, by the
 * device and the host routine alike; what a NaN or infinite INPUT gives is not specified bit for bit. */
enum { ORBM_REFRESH_DESCRIPTOR = 1, ORBM_REFRESH_NORMAL_DEPTH = 2 };
enum { ORBM_REFRESH_CAP = 256 };   /* observations of one point the device takes; a longer point runs on the host inside the same call */

typedef struct orbm_refresh_in {
    int32_t n_points, n_obs;
    const int32_t* first;          /* n_points + 1, first[0] = 0, non-decreasing, first[n_points] = n_obs            */
    const uint8_t* obs_desc;       /* n_obs x 32: pKF->GetDescriptor(cam, local index) of the observation            */
    const float* obs_centre;       /* n_obs x 3: centre of the observing CAMERA (Owi[cam])                           */
    const uint8_t* obs_alive;      /* n_obs: != 0 where !pKF->isBad()                                                */
    const float* pos;              /* n_points x 3: mWorldPos                                                        */
    const float* ref_centre;       /* n_points x 3: mpRefKF->GetCameraCenter() (camera 1, whatever camera observed)  */
    const int32_t* ref_level;      /* n_points: mpRefKF->mvKeysUn_total[observations[mpRefKF]].octave                */
    const uint8_t* what;           /* n_points: ORBM_REFRESH_* bits                                                  */
    const float* scale_factors;    /* mvScaleFactors, n_levels (1 .. ORBM_MAX_LEVELS)                                */
    int32_t n_levels;
} orbm_refresh_in;

typedef struct orbm_refresh_out {  /* one per point; the fields of a job that was not asked for are zero */
    uint8_t desc[32];              /* mDescriptor                                                         */
    float normal[3];               /* mNormalVector                                                       */
    float min_dist, max_dist;      /* mfMinDistance, mfMaxDistance                                        */
    int32_t best_obs;              /* position of the winner in the point's observation list; -1 = the descriptor job was asked for
                                      and produced nothing (no alive observation: the reference leaves mDescriptor alone) */
    int32_t best_median;           /* its median distance                                                 */
} orbm_refresh_out;                /* 60 bytes */

/* Device path.  Points are worked on by observation count: up to 16 a 16-lane group (four points per wavefront), up to 64 one
 * wavefront, up to ORBM_REFRESH_CAP one workgroup; a point beyond the cap goes through the host routine inside the same call
 * (orbm_debug_last_refresh, include/orb_debug.h, says how many did).  A point without observations is legal: the reference returns
 * early for it, its record is zero (best_obs = -1 if the descriptor job was asked for).  The normal / depth job of a point with
 * observations needs 0 <= ref_level < n_levels.  Runs on the handle's stream with the handle's scratch; returns when `out`
 * (n_points records, host) is written. */
int orbm_refresh_points(orbm_matcher* m, const orbm_refresh_in* in, orbm_refresh_out* out);
/* The same routine entirely on the host, no device needed: the fallback above and the cross-check of the kernels. */
int orbm_refresh_points_host(const orbm_refresh_in* in, orbm_refresh_out* out);

/* -- pose optimisation: motion-only Levenberg-Marquardt ----------------------------------------------------------
 * Optimizer::PoseOptimization(Frame*) (reference src/Optimizer.cc:352-618, camera 1 only) and PoseOptimization(Frame*, bool bAllCams)
 * (:620-898, every camera through Tcim) from the edge list on: one 6-dof vertex, one unary edge per feature with a map point
 * (EdgeSE3ProjectXYZOnlyPose / EdgeStereoSE3ProjectXYZOnlyPose, mono or stereo by uright < 0; their _multi forms in the all-cameras
 * mode), four rounds of at most ten Levenberg iterations each restarting from the start pose, a re-classification of every edge
 * after each round ((float)chi2 > 5.991f / 7.815f), the Huber kernel in the first three rounds.  g2o, Eigen and the C library's sin /
 * cos / pow are restated, not linked; what that leaves UNPINNED is listed in DESIGN.md section 2.
 * Two evaluation orders of ONE host routine:
 *   ORBM_POSE_ORDER_INDEX    every sum over edges sequential in ascending edge position, sin / cos / pow(., 3) of the C library: the
 *                            restatement of the reference.
 *   ORBM_POSE_ORDER_DEVICE   the sums in the kernel's fixed tree (256 lanes: lane l owns edges l, l + 256, ... in ascending order, then an
 *                            xor butterfly 1, 2, ..., 32 inside each wave, then the four waves in wave order); sine and cosine from a fixed
 *                            sequence of + - * / in double, the cube by multiplication.  What the device computes, bit for bit. */
enum { ORBM_POSE_CAM0 = 0, ORBM_POSE_ALL_CAMS = 1 };
enum { ORBM_POSE_ORDER_INDEX = 0, ORBM_POSE_ORDER_DEVICE = 1 };
enum { ORBM_POSE_CAP = 8192,      /* edges of one problem the device takes; a longer one runs on the host inside the same call */
       ORBM_POSE_MAX_BATCH = 64, ORBM_POSE_ROUNDS = 4 };

typedef struct orbm_pose_problem {
    float Tcw[16];                 /* pFrame->mTcw, row-major 4x4: the start pose of every round                      */
    float fx, fy, cx, cy, bf;      /* pFrame->fx, fy, cx, cy, mbf                                                      */
    float Rcam12[9], tcam12[3];    /* pFrame->mRcam12 (row-major), mtcam12: read in the all-cameras mode only          */
    float inv_level_sigma2[ORBM_MAX_LEVELS];   /* pFrame->mvInvLevelSigma2                                             */
    int32_t n_levels;              /* 1 .. ORBM_MAX_LEVELS: every edge's octave lies below it                          */
    int32_t mode;                  /* ORBM_POSE_CAM0 / ORBM_POSE_ALL_CAMS                                              */
    int32_t n_cam0;                /* pFrame->N: in the all-cameras mode feature g belongs to camera 2 when g >= n_cam0 */
} orbm_pose_problem;               /* 272 bytes */

typedef struct orbm_pose_round {   /* one optimizer.optimize(10) */
    int32_t iterations, trials;    /* Levenberg iterations run, linear solves (trials) run over all of them            */
    double chi2, lambda;           /* the robust chi2 and the damping the round ended with (0 when nothing was active) */
} orbm_pose_round;

typedef struct orbm_pose_result {
    float Tcw[16];                 /* Converter::toCvMat of the final estimate: what SetPose receives (the start pose, bit for bit, when n_initial < 3) */
    double q[4], t[3];             /* the estimate it was rounded from: quaternion x y z w, translation                */
    int32_t n_initial, n_bad;      /* nInitialCorrespondences, nBad of the last round run                              */
    int32_t n_inliers;             /* the reference's return value: n_initial - n_bad, 0 when n_initial < 3            */
    int32_t rounds;                /* rounds run: 0 (n_initial < 3), 1 (n_initial < 10) or 4                           */
    orbm_pose_round round[ORBM_POSE_ROUNDS];
} orbm_pose_result;                /* 232 bytes, no padding */

/* B problems (1 .. ORBM_POSE_MAX_BATCH) in one call, one workgroup per problem, resident from the first residual to the last flag.
 * The edges arrive as host arrays, CSR per problem: problem b owns edges first[b] .. first[b+1]-1 in ascending feature index.
 *   feat[e]    feature index i of the edge (decides the camera in the all-cameras mode)
 *   pos[3e..]  pMP->GetWorldPos()
 *   obs[3e..]  mvKeysUn[_total][i].pt.x, .pt.y, mvuRight[_total][i]   (uright < 0: a monocular edge)
 *   octave[e]  mvKeysUn[_total][i].octave
 * outlier_out[e] = mvbOutlier of the edge's feature; results[b] as above.  A NaN result is written as the NaN x86 makes from an
 * invalid operation (sign bit set) by the device and the host routine alike; what a NaN or infinite INPUT gives is not specified bit
 * for bit.  A problem beyond ORBM_POSE_CAP edges runs through the host routine in the device order inside the same call
 * (orbm_debug_last_pose, include/orb_debug.h). */
int orbm_pose_optimize(orbm_matcher* m, const orbm_pose_problem* problems, int B, const int32_t* first, const int32_t* feat,
                       const float* pos, const float* obs, const int32_t* octave, uint8_t* outlier_out, orbm_pose_result* results);
/* The same routine entirely on the host, no device needed, in either order. */
int orbm_pose_optimize_host(const orbm_pose_problem* problems, int B, const int32_t* first, const int32_t* feat, const float* pos,
                            const float* obs, const int32_t* octave, int order, uint8_t* outlier_out, orbm_pose_result* results);
/* One problem whose observations and positions are already in HBM: x, y, uright and octave of feature g are read from the resident
 * frame `cur` (the arrays the searches compare against), the position from row point_of_feature[g] of the table `pts`
 * (point_of_feature: n_total entries on the host, a row or a negative value = no point; the shape orbm_search_local_points returns in
 * match_of_feature).  Edges = the features with a point in ascending g (g < n_cam0 only in ORBM_POSE_CAM0).  One 4-byte word per
 * edge goes up; outlier_out has n_total entries, 0 for a feature without an edge.  Same bytes as orbm_pose_optimize on the same data. */
int orbm_pose_optimize_resident(orbm_matcher* m, const orbm_pose_problem* problem, const orbm_frame* cur, const orbm_points* pts,
                                const int32_t* point_of_feature, uint8_t* outlier_out, orbm_pose_result* result);
/* (test hook) The sine / cosine sequence of ORBM_POSE_ORDER_DEVICE on the host. */
void orbm_pose_sincos(double x, double* s, double* c);

/* -- Sim3Solver: every RANSAC hypothesis of a loop in one call --------------------------------------------------------
 * Sim3Solver (reference src/Sim3Solver.cc) between SearchByBoW and SearchBySim3 of LoopClosing::ComputeSim3: per hypothesis the
 * three-point Horn alignment (ComputeCentroid, ComputeSim3 steps 1-8, both branches of mbFixScale) and CheckInliers (Project in both
 * directions with the second-camera branch, FromCameraToImage, the two threshold tests).  No iteration depends on another, so all
 * hypotheses of all candidates are evaluated at once and orbm_sim3_walk recovers the reference's sequential `iterate` from the counts.
 * RANSAC's randomness is an INPUT: the triples arrive drawn.  The OpenCV operators on the path (reduce, gemm, eigen, norm, Rodrigues,
 * dot, pow, the scaled forms) are restated one function each and UNPINNED.
 * Two orders of ONE routine, differing in three calls only:
 *   ORBM_SIM3_MATH_LIBM     atan2, sin, cos of the C library: the restatement of the reference.
 *   ORBM_SIM3_MATH_DEVICE   atan2 from + - * / sqrt in double (orbm_sim3_atan2), sine / cosine of orbm_pose_sincos.  What the device
 *                           computes, bit for bit.  No floating-point value crosses lanes: there is no summation order to choose. */
enum { ORBM_SIM3_MATH_LIBM = 0, ORBM_SIM3_MATH_DEVICE = 1 };
enum { ORBM_SIM3_CAP = 8192,      /* correspondences of one problem the device takes; a longer one runs on the host inside the same call */
       ORBM_SIM3_MAX_ITS = 1024,  /* hypotheses of one problem (the reference draws at most 300)                                          */
       ORBM_SIM3_MAX_BATCH = 64 };

typedef struct orbm_sim3_problem {
    float fx1, fy1, cx1, cy1;      /* mK1 = pKF1->mK                                                                   */
    float fx2, fy2, cx2, cy2;      /* mK2 = pKF2->mK                                                                   */
    float Rcam21[9], tcam21[3];    /* mRcam21 = Rcam12.t(), mtcam21 = -mRcam21 * tcam12 (row-major), as the constructor forms them */
    int32_t fix_scale;             /* mbFixScale                                                                       */
} orbm_sim3_problem;               /* 84 bytes */

typedef struct orbm_sim3_hyp {     /* one iteration of `iterate` */
    float R12[9], t12[3], s12;     /* mR12i (row-major), mt12i, ms12i                                                  */
    float T12[16], T21[16];        /* mT12i, mT21i (row-major 4x4)                                                     */
    int32_t n_inliers;             /* mnInliersi                                                                       */
} orbm_sim3_hyp;                   /* 184 bytes, no padding */

/* B problems (1 .. ORBM_SIM3_MAX_BATCH), one enqueue, one synchronisation.  Correspondences are CSR per problem: problem b owns
 * first[b] .. first[b+1]-1, in the order of the constructor's push_backs:
 *   x3dc1[3i..], x3dc2[3i..]   mvX3Dc1[i], mvX3Dc2[i] (camera-frame points of keyframe 1 and 2)
 *   cam1[i], cam2[i]           camIdx1[i], camIdx2[i] (1 = the second camera of the rig)
 *   max_err1[i], max_err2[i]   mvnMaxError1[i], mvnMaxError2[i] as the comparison reads them: 9.210 * sigma2 through the reference's
 *                              std::vector<size_t> (truncated), converted to float
 * mvP1im1 / mvP2im2 are computed inside.  Hypotheses are CSR per problem too: problem b owns its_first[b] .. its_first[b+1]-1 (at most
 * ORBM_SIM3_MAX_ITS), hypothesis g draws the correspondences triples[3g..3g+2] (positions inside the problem, 0 .. N_b-1).
 * hyp_out[g] is the record of hypothesis g.  mask_out holds one bit per correspondence (bit i & 63 of word i >> 6 = mvbInliersi[i]),
 * W_b = (N_b + 63) / 64 words per hypothesis, hypothesis-major inside a problem, the problems one after another: hypothesis h of
 * problem b starts at word sum over b' < b of H_b' * W_b', plus h * W_b.
 * A degenerate triple (coincident or collinear points) gives non-finite values: every comparison with them is false, the count is 0
 * and the mask empty.  A NaN is written as the NaN x86 makes from an invalid operation; what a non-finite INPUT gives is unspecified.
 * A problem beyond ORBM_SIM3_CAP correspondences runs through the host routine in DEVICE order inside the same call
 * (orbm_debug_last_sim3, include/orb_debug.h). */
int orbm_sim3_ransac(orbm_matcher* m, const orbm_sim3_problem* problems, int B, const int32_t* first, const float* x3dc1,
                     const float* x3dc2, const int32_t* cam1, const int32_t* cam2, const float* max_err1, const float* max_err2,
                     const int32_t* its_first, const int32_t* triples, orbm_sim3_hyp* hyp_out, uint64_t* mask_out);
/* The same routine entirely on the host, no device needed, in either order. */
int orbm_sim3_ransac_host(const orbm_sim3_problem* problems, int B, const int32_t* first, const float* x3dc1, const float* x3dc2,
                          const int32_t* cam1, const int32_t* cam2, const float* max_err1, const float* max_err2,
                          const int32_t* its_first, const int32_t* triples, int order, orbm_sim3_hyp* hyp_out, uint64_t* mask_out);

/* The reference's `iterate` loop over precomputed counts (host only; the class, the Python wrapper and the tests share it).
 * counts[0 .. H-1]: n_inliers of the solver's hypotheses in drawing order, H = mRansacMaxIts; N = correspondences. */
typedef struct orbm_sim3_walk_state {
    int32_t iterations;            /* mnIterations after the call                                                      */
    int32_t best_inliers;          /* mnBestInliers; start a solver with 0                                             */
    int32_t best_index;            /* the hypothesis mBestT12 / mBestRotation / ... were taken from; start with -1     */
    int32_t no_more;               /* bNoMore of the call                                                              */
} orbm_sim3_walk_state;
/* iterate(n_iterations, ...) starting at mnIterations = start_iteration: `mnInliersi >= mnBestInliers` (greater OR EQUAL) makes a
 * hypothesis the best, `mnInliersi > mRansacMinInliers` (strictly greater) then ends the call.  Returns the hypothesis whose T12
 * `iterate` returns, or -1 for the empty cv::Mat; N < min_inliers returns -1 at once with no_more set. */
int orbm_sim3_walk(const int32_t* counts, int H, int N, int min_inliers, int start_iteration, int n_iterations, orbm_sim3_walk_state* state);
/* SetRansacParameters' arithmetic as the reference's statement resolves it: float epsilon, pow, log and ceil of the C library, the
 * conversion to int as x86 performs it (INT_MIN for a NaN or a value out of range), max(1, min(., max_its)). */
int orbm_sim3_iterations(double probability, int min_inliers, int max_its, int N);
/* (test hook) The atan2 sequence of ORBM_SIM3_MATH_DEVICE on the host: y >= 0, x in [-1, 1]. */
double orbm_sim3_atan2(double y, double x);

/* -- Sim3 refinement: Optimizer::OptimizeSim3_cam1 ----------------------------------------------------------------------
 * Optimizer::OptimizeSim3_cam1 (reference src/Optimizer.cc:1984-2243) from its correspondence list on: one 7-dof Sim3 vertex, per
 * correspondence an EdgeSim3ProjectXYZ (the point of keyframe 2 through S12 into camera 1) and an EdgeInverseSim3ProjectXYZ (the point
 * of keyframe 1 through S12^-1 into camera 2) with fixed point vertices and Huber kernels, optimize(5), the chi-square test that
 * removes correspondences, optimize(5 or 10) on the survivors, the final test.  Neither edge has an analytic Jacobian: g2o's numeric
 * linearizeOplus (central differences at 1e-9 through oplus) is restated with them, as are g2o::Sim3 (never normalised), the Huber
 * kernel, the Levenberg loop, optimize()'s stopping rules and Eigen's LDLT; what that leaves UNPINNED is listed in DESIGN.md section 2.
 * Two orders of ONE host routine, as for the pose (ORBM_POSE_ORDER_INDEX / ORBM_POSE_ORDER_DEVICE):
 *   INDEX    sums over correspondences sequential in ascending position (e12 then e21 of each); sin, cos, exp, pow of the C library.
 *   DEVICE   the kernel's tree (256 lanes, lane l owns l, l + 256, ...; xor butterfly in each wave; the four waves in order),
 *            orbm_pose_sincos, orbm_sim3opt_exp, the cube by multiplication.  What the device computes, bit for bit. */
enum { ORBM_SIM3OPT_CAP = 8192,   /* correspondences of one problem the device takes; a longer one runs on the host inside the same call */
       ORBM_SIM3OPT_MAX_BATCH = 64 };

typedef struct orbm_sim3opt_problem {
    float K1[4], K2[4];            /* fx, fy, cx, cy of pKF1->mK, pKF2->mK                                              */
    float inv_level_sigma2_1[ORBM_MAX_LEVELS];   /* pKF1->mvInvLevelSigma2                                              */
    float inv_level_sigma2_2[ORBM_MAX_LEVELS];   /* pKF2->mvInvLevelSigma2                                              */
    int32_t n_levels1, n_levels2;  /* 1 .. ORBM_MAX_LEVELS: every octave1 / octave2 lies below it                       */
    float R[9], t[3], s;           /* the start g2oS12 as g2o::Sim3(Matrix3d, Vector3d, double) receives it (R row-major) */
    float th2;                     /* th2: the chi-square bound of both tests, deltaHuber = sqrt(th2) in float          */
    int32_t fix_scale;             /* bFixScale                                                                         */
} orbm_sim3opt_problem;            /* 356 bytes */

typedef struct orbm_sim3opt_result {
    double q[4], t[3], s;          /* the vertex's estimate when the call returns (quaternion x y z w, NOT normalised); the start when written == 0 */
    int32_t n_inliers;             /* the reference's return value: nIn, 0 on the early return                          */
    int32_t n_correspondences, n_bad, n_more_iterations;   /* nCorrespondences, nBad, nMoreIterations                   */
    int32_t written;               /* 1: `g2oS12 = vSim3_recov->estimate()` was reached; 0: the early return left g2oS12 alone */
    int32_t optimisations;         /* optimize() calls that found an active edge: 0, 1 or 2                             */
    orbm_pose_round round[2];      /* optimize(5) and optimize(nMoreIterations)                                         */
} orbm_sim3opt_result;             /* 136 bytes, no padding */

/* B problems (1 .. ORBM_SIM3OPT_MAX_BATCH), one workgroup per problem, one enqueue, one synchronisation.  Correspondences are CSR per
 * problem (problem b owns first[b] .. first[b+1]-1), in the order of the reference's loop over vpMatches1:
 *   x3dc1[3i..], x3dc2[3i..]   P3D1c = R1w*P3D1w + t1w and P3D2c = R2w*P3D2w + t2w, camera-frame float points
 *   obs1[2i..], obs2[2i..]     kpUn1.pt, kpUn2.pt
 *   octave1[i], octave2[i]     kpUn1.octave, kpUn2.octave
 * flag_out[i]: 0 = kept, 1 = removed by the test after the first optimisation, 2 = failed the final test (vpMatches1 is nulled for
 * both).  A NaN result leaves as the NaN x86 makes; what a non-finite INPUT gives is unspecified.  A problem beyond ORBM_SIM3OPT_CAP
 * runs through the host routine in DEVICE order inside the same call (orbm_debug_last_sim3opt, include/orb_debug.h). */
int orbm_sim3_optimize(orbm_matcher* m, const orbm_sim3opt_problem* problems, int B, const int32_t* first, const float* x3dc1,
                       const float* x3dc2, const float* obs1, const float* obs2, const int32_t* octave1, const int32_t* octave2,
                       uint8_t* flag_out, orbm_sim3opt_result* results);
/* The same routine entirely on the host, no device needed, in either order (ORBM_POSE_ORDER_INDEX / ORBM_POSE_ORDER_DEVICE). */
int orbm_sim3_optimize_host(const orbm_sim3opt_problem* problems, int B, const int32_t* first, const float* x3dc1, const float* x3dc2,
                            const float* obs1, const float* obs2, const int32_t* octave1, const int32_t* octave2, int order,
                            uint8_t* flag_out, orbm_sim3opt_result* results);
/* (test hook) The exponential of the DEVICE order on the host; exp(0) is exactly 1. */
double orbm_sim3opt_exp(double x);
/* (test hooks) g2o::Sim3(Vector7d) in either order -> q[4], t[3], s in out8, returns the branch of fabs(sigma) < eps x theta < eps
 * (0: both small, 1: sigma small, 2: theta small, 3: neither); the 7x7 LDLT solve of the Levenberg trial (A row-major, destroyed). */
int orbm_sim3opt_expmap(const double* update7, int order, double* out8);
int orbm_sim3opt_ldlt7(double* A49, const double* b7, double* x7);

/* -- local bundle adjustment ---------------------------------------------------------------------------------------------
 * Optimizer::LocalBundleAdjustment (reference src/Optimizer.cc:921-1353) from the graph on: free and fixed keyframe poses, marginalised
 * points, one binary edge per observation (EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ with Tcim_quat, mono by ur < 0), Huber kernels,
 * optimize(5), the chi-square / depth test that moves edges to level 1 and drops the kernels, initializeOptimization(0), optimize(10),
 * the final test.  g2o's block solver is restated: Hpp, Hll, Hpl and b summed in active-edge order, computeLambdaInit over every
 * diagonal entry of every active vertex, setLambda on both diagonals (the undamped diagonals are kept, not recovered by subtraction),
 * the Schur loop of BlockSolver::solve landmark by landmark in ascending order, computeScale over all of x, the lambda rules.
 *   poses    n_poses of them: the free ones first (the local keyframes except mnId == 0, in ascending mnId: g2o's VertexIDCompare order),
 *            then the fixed ones.  Tcw: the float 4x4 Converter::toSE3Quat reads, row-major; K: fx fy cx cy mbf per pose.
 *   points   in ascending vertex id; bad[l] != 0 reproduces `pMP->isBad()` at both tests: the point's edges are skipped there, so they
 *            keep level 0 and their kernels and are never marked.
 *   edges    a CSR per point: point l owns edges first[l] .. first[l+1]-1.  edge_pose: index into the poses; edge_cam: 0 or 1 selects
 *            Tcim; obs: u, v, ur (ur < 0: the mono form); inv_sigma2: mvInvLevelSigma2[octave].  A (pose, point) pair occurs once.  The
 *            edge position IS the active-edge order (g2o: insertion order): a caller that inserts its points in another order than
 *            ascending vertex id gets the sums of its own order by handing the points in that order -- the landmark order follows.
 *   stop     g2o polls the flag at core/sparse_optimizer.cpp:376 and optimization_algorithm_levenberg.cpp:149, the reference at
 *            Optimizer.cc:1204 and :1217; stop(ctx) is called at exactly those points in that order (not at all when stop is NULL).
 * Stated deviations from the reference: (a) the reduced system is solved by a dense LDL^T WITHOUT pivoting in the natural order of
 * the free poses, every inner product sequential in ascending index, failing on a zero or non-finite pivot -- not by Eigen's
 * SimplicialLDLT behind an AMD ordering; the same factorisation up to the order of its sums, parity with g2o / Eigen is not claimed for
 * it, nor for Matrix3d::inverse() and what csrc/g2o_dev.h marks UNPINNED.  (b) Inside std::map<KeyFrame*, size_t> a point's
 * observations are ordered by heap address; here the order is the caller's (the class orders them by mnId).  An edge that no
 * computeActiveErrors ever reached (the call was stopped before the first iteration) is tested with chi2 = 0; g2o leaves its error
 * uninitialised.  After a failed solve the update is the previous x, position by position, as g2o's vector is.
 * Two orders of ONE host routine, as for the pose: ORBM_POSE_ORDER_INDEX (the C library's sin / cos / pow, the total chi2 summed
 * sequentially over the active edges: the restatement of the reference) and ORBM_POSE_ORDER_DEVICE (orbm_pose_sincos, the cube by
 * multiplication, the total chi2 in the kernels' tree: edge positions 256 k .. 256 k + 255 through lm_dev.h's butterfly and wave sum,
 * an inactive edge counting 0.0, then the partials in ascending k): what the device computes, bit for bit. */
enum { ORBM_LBA_MAX_FREE = 64, ORBM_LBA_MAX_POSES = 4096, ORBM_LBA_MAX_POINTS = 65536, ORBM_LBA_MAX_EDGES = 262144 };
enum { ORBM_LBA_ENDED_COMPLETE = 0,        /* both optimisations and both tests                                                      */
       ORBM_LBA_ENDED_STOPPED_AT_START = 1,/* the flag was set at :1204: the reference returns, nothing is to be written              */
       ORBM_LBA_ENDED_NO_SECOND = 2 };     /* the flag was set at :1217 (bDoMore = false): the final test follows optimize(5)         */
enum { ORBM_LBA_FLAG_LEVEL1 = 1,           /* setLevel(1) at the test after optimize(5)                                              */
       ORBM_LBA_FLAG_ERASE = 2 };          /* the pair goes to vToErase at the final test                                            */
typedef int (*orbm_lba_stop_fn)(void* ctx);

typedef struct orbm_lba_problem {
    int32_t n_free, n_poses, n_points, reserved;
    const float* Tcw;              /* n_poses x 16                                                                      */
    const float* K;                /* n_poses x 5                                                                       */
    const float* points;           /* n_points x 3: pMP->GetWorldPos()                                                  */
    const uint8_t* bad;            /* n_points, or NULL: no point is bad                                                */
    const int32_t* first;          /* n_points + 1                                                                      */
    const int32_t* edge_pose;      /* per edge                                                                          */
    const uint8_t* edge_cam;
    const float* obs;              /* 3 per edge                                                                        */
    const float* inv_sigma2;
    float Tcim[2][16];             /* Tcam11 (the identity) and Tcam21 as the reference builds them (:1048-1061)        */
} orbm_lba_problem;

typedef struct orbm_lba_result {
    double* pose;                  /* n_poses x 7: the estimates, quaternion x y z w and translation                    */
    float* Tcw;                    /* n_poses x 16: Converter::toCvMat of them, what SetPose receives                   */
    double* point;                 /* n_points x 3                                                                      */
    float* point_f;                /* n_points x 3: Converter::toCvMat(Vector3d), what SetWorldPos receives             */
    uint8_t* flags;                /* per edge: ORBM_LBA_FLAG_*                                                         */
    orbm_pose_round round[2];      /* optimize(5) and optimize(10)                                                      */
    int32_t ended;                 /* ORBM_LBA_ENDED_*                                                                  */
    int32_t optimisations;         /* optimize() calls that had an active vertex                                        */
    int32_t polls;                 /* calls of stop                                                                     */
    int32_t n_level1, n_erase;     /* edges flagged at either test                                                      */
    int32_t active_poses[2], active_points[2], active_edges[2];   /* of either initializeOptimization                   */
    int32_t reserved;
} orbm_lba_result;

/* One local bundle adjustment on the device: the Levenberg loop is driven by the host, which synchronises once per trial and reads
 * one 4-byte command word; every step is a short chain of kernels, every sum has the order it has in the host routine, no atomics.  A
 * problem beyond a cap (ORBM_LBA_MAX_*), or one without a free pose, runs through the host routine in DEVICE order inside the same
 * call (orbm_debug_last_local_ba, include/orb_debug.h).  Same bytes as orbm_local_ba_host(..., ORBM_POSE_ORDER_DEVICE). */
int orbm_local_ba(orbm_matcher* m, const orbm_lba_problem* problem, orbm_lba_stop_fn stop, void* stop_ctx, orbm_lba_result* result);
/* The same statements on the host, no device needed, in either order. */
int orbm_local_ba_host(const orbm_lba_problem* problem, orbm_lba_stop_fn stop, void* stop_ctx, int order, orbm_lba_result* result);
/* (test hooks, host only) One edge at a pose (q x y z w, t) and a point: out[0..2] the error, out[3] chi2, out[4] the depth,
 * out[5..13] the 3x3 Jacobian by the point, out[14..31] the 3x6 Jacobian by the pose (row 2 is zero for a mono edge). */
int orbm_lba_edge_eval(const float* Tcim2x16, const float* K5, const double* pose7, const double* point3, int cam, const float* obs3,
                       float inv_sigma2, double* out32);
/* The dense LDL^T without pivoting of the reduced system (deviation (a)): H n x n row-major, its upper triangle is read; returns 1 and
 * writes x, or 0 on a zero or non-finite pivot (x untouched). */
int orbm_lba_ldlt(int n, const double* H, const double* b, double* x);
/* The controller of the local BA and lm_step of the dense ports on ONE stream of chi2 values (the first of an iteration is the pass at
 * the estimate, the others its trials; the stream ends the run), a 6-vector problem H = diag(hdiag6), b = b6, max_iter iterations:
 * per step both write lambda, ni and a verdict (1 a trial follows, 2 the next iteration, 3 optimize() returned) into out_lba / out_lm
 * (3 doubles per step).  Returns the steps taken. */
int orbm_lba_controller_trace(const double* chi, int n_chi, const double* hdiag6, const double* b6, int max_iter, int order, int max_steps,
                              double* out_lba, double* out_lm);

/* -- global bundle adjustment: Optimizer::BundleAdjustment from its graph on -----------------------------------------------
 * Optimizer::BundleAdjustment (reference src/Optimizer.cc:47-330; LoopClosing::RunGlobalBundleAdjustment: 10 iterations, no kernels;
 * Tracking: 20 iterations, robust) between the graph and the recovery: ONE initializeOptimization(), ONE optimize(n_iterations),
 * no chi-square test, no flags, no second optimisation.  The problem is orbm_lba_problem as it stands (the free poses -- every
 * keyframe but mnId == 0 -- first, a CSR per point, the caller's edge order is the active-edge order); `bad` is IGNORED: the
 * reference skips bad points before the graph.  robust != 0 puts the Huber kernel (sqrt(5.99) / sqrt(7.815)) on every edge, 0 on
 * none.  A vertex without an active edge is not active and its estimate is returned as it came.  stop is polled exactly where g2o
 * polls forceStopFlag (core/sparse_optimizer.cpp:376 at the head of an iteration, optimization_algorithm_levenberg.cpp:149 in the
 * trial loop) and nowhere else -- the reference polls nowhere in this function; after a stop the estimates reached so far are
 * returned, as the reference writes them.
 * Everything up to the reduced system is the local BA's, statement for statement, with its stated deviations.  The reduced system:
 * only the block pairs (i1 <= i2) of active free poses that share an active landmark, and every diagonal block, are computed; the
 * other blocks are exactly 0.0 (nothing is subtracted from 0.0 there), so the matrix has the bytes of the full loop.  It is solved by
 * orbm_ba_ldlt: deviation (a) of the local BA (dense, no pivoting, natural order, failure on a zero or non-finite pivot with x
 * untouched, parity with Eigen not claimed), factorisation and forward substitution with the statements and summation order of
 * orbm_lba_ldlt, but the BACKWARD substitution sums in DESCENDING j: s = 0; for j = n-1 .. i+1: s += L(j,i) y_j; x_i = y_i - s.
 * With these orders the blocked execution across workgroups (csrc/ba_ldlt_dev.h: panels of ORBM_BA_PANEL columns, every element's sum
 * carried from panel to panel, never split or re-associated) has the bytes of the sequential routine.  Nothing of the reference is
 * restated in the solver, so both orders of the host routine use it. */
enum { ORBM_BA_MAX_FREE = 1024, ORBM_BA_MAX_POSES = 4096, ORBM_BA_MAX_POINTS = 1 << 19, ORBM_BA_MAX_EDGES = 1 << 22 };
enum { ORBM_BA_PANEL = 64 };
typedef struct orbm_ba_result {
    double* pose;                  /* n_poses x 7: the estimates, quaternion x y z w and translation                    */
    float* Tcw;                    /* n_poses x 16: Converter::toCvMat of them, what SetPose / mTcwGBA receive          */
    double* point;                 /* n_points x 3                                                                      */
    float* point_f;                /* n_points x 3: what SetWorldPos / mPosGBA receive                                  */
    orbm_pose_round round;         /* of the one optimize()                                                             */
    int32_t optimised;             /* 1: optimize() had an active vertex                                                */
    int32_t polls;                 /* calls of stop                                                                     */
    int32_t active_poses, active_points, active_edges;   /* of initializeOptimization()                                 */
    int32_t reserved[3];
} orbm_ba_result;
/* On the device: the local BA's kernels per edge, point and pose, k_ba_schur_pairs over the pairs that exist and the blocked LDL^T;
 * one synchronisation per Levenberg trial.  A problem beyond a cap (ORBM_BA_MAX_*), or without an active free pose, runs through
 * the host routine in DEVICE order inside the same call (orbm_debug_last_bundle_adjust).  Same bytes as
 * orbm_bundle_adjust_host(..., ORBM_POSE_ORDER_DEVICE). */
int orbm_bundle_adjust(orbm_matcher* m, const orbm_lba_problem* problem, int n_iterations, int robust, orbm_lba_stop_fn stop, void* stop_ctx,
                       orbm_ba_result* result);
/* The same statements on the host, no device needed, in either order. */
int orbm_bundle_adjust_host(const orbm_lba_problem* problem, int n_iterations, int robust, orbm_lba_stop_fn stop, void* stop_ctx, int order,
                            orbm_ba_result* result);
/* The solver of the reduced system, on the host: the definition.  H n x n row-major (upper triangle read), n <= 6 ORBM_BA_MAX_FREE;
 * returns 1 and writes x, or 0 on a zero or non-finite pivot (x untouched). */
int orbm_ba_ldlt(int n, const double* H, const double* b, double* x);
/* (test hook) The device solver alone on host arrays: the same bytes, the same return values; negative on an error. */
int orbm_ba_ldlt_device(orbm_matcher* m, int n, const double* H, const double* b, double* x);

/* -- essential graph: Optimizer::OptimizeEssentialGraph from its graph on ------------------------------------------------------
 * Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:1373-1677, called by LoopClosing::CorrectLoop) between the graph and
 * the recovery: VertexSim3Expmap vertices, EdgeSim3 edges with information = I and no robust kernel, setUserLambdaInit(1e-16), ONE
 * initializeOptimization(), ONE optimize(n_iterations), then step 6 (the poses SetPose receives) and step 7 (every map point moved
 * through its reference keyframe's input and final Sim3).  Restated from g2o: Sim3::log() with its four branches (types/sim3.h:148-230),
 * EdgeSim3::computeError, the NUMERIC Jacobian of BaseBinaryEdge::linearizeOplus (delta = 1e-9, central differences, the perturbed
 * estimate is Sim3(+-delta e_d) * estimate), constructQuadraticForm without a kernel, the block (i1 <= i2) an edge's off-diagonal part
 * goes to by _hessianRowMajor, setLambda on the diagonal (the undamped diagonal is kept), computeScale over all of x, the lambda rules.
 *   vertices  the free ones first in ascending mnId (g2o's VertexIDCompare order), then the fixed ones.  A vertex without an edge is
 *             not active: its estimate is returned as it came.  Without an active free vertex optimize() returns before its loop.
 *   edges     the edge position IS the active-edge order (insertion order); a pair may occur more than once, in either direction;
 *             an edge of a vertex to itself is refused.  An edge between two fixed vertices has no Jacobian and still counts in chi2.
 *   fix_scale `_fix_scale` of EVERY vertex: oplusImpl writes update[6] = 0 into the caller's array.  In linearizeOplus that makes both
 *             steps along the scale the same estimate, so column 6 of both Jacobians is exactly 0 (for finite errors) and the seventh
 *             diagonal entry of every block is the damping alone; in the trial loop update(x) runs before computeScale(), which
 *             therefore reads the solver's x with every seventh entry zeroed.
 *   points    point_ref: the vertex of nIDr, or -1 when vScw / vCorrectedSwc hold the default-constructed Sim3 there (identity, zero,
 *             1): the position still goes through both maps in double and back to float.
 * Kept products by the identity: ALL of them -- information() * _error in chi2() and in omega_r, A^T * omega, B^T * omega -- are
 * evaluated as sums of seven products in ascending index (0 * NaN and 0 * inf are NaN, a sum of signed zeros is not its last term).
 * Stated deviations: the linear system is solved by orbm_ba_ldlt (dense, no pivoting, natural order of the active free vertices, failure
 * on a zero or non-finite pivot with x untouched) in both orders, not by Eigen's SimplicialLDLT behind an AMD ordering; Eigen's
 * operators (the small products taken in ascending index, Matrix3d::lu().solve, Quaterniond(Matrix3d), toRotationMatrix) are restated
 * and UNPINNED (csrc/g2o_dev.h).  There is no stop function: the reference passes none and g2o's forceStopFlag is null here.
 * Two orders of ONE host routine: ORBM_POSE_ORDER_INDEX (the C library's log / acos / sin / cos / exp / pow, chi2 and computeScale
 * summed sequentially: the restatement of the reference) and ORBM_POSE_ORDER_DEVICE (pose_log, pose_acos, orbm_pose_sincos,
 * orbm_sim3opt_exp, the cube by multiplication; the total chi2 over edge positions 256 k .. 256 k + 255 through lm_dev.h's butterfly and
 * wave sum, then the partials in ascending k, and computeScale's terms over positions 256 k .. of x the same way): what the device
 * computes, bit for bit. */
enum { ORBM_EG_MAX_FREE = 877,      /* 7 * 877 = 6139 <= 6 * ORBM_BA_MAX_FREE rows: what the blocked solver is sized for */
       ORBM_EG_MAX_VERTICES = 4096, ORBM_EG_MAX_EDGES = 65536, ORBM_EG_MAX_POINTS = 1 << 19 };
typedef struct orbm_eg_problem {
    int32_t n_free, n_vertices, n_edges, n_points, fix_scale, reserved[3];
    const double*  vertex;        /* n_vertices x 8: quaternion x y z w, translation, scale; the free ones first in ascending mnId
                                     (VertexIDCompare), then the fixed ones                                                     */
    const double*  measurement;   /* n_edges x 8: Sji                                                                          */
    const int32_t* edge_v0;       /* _vertices[0] (Siw) and _vertices[1] (Sjw) as vertex indices; the edge position IS the      */
    const int32_t* edge_v1;       /* active-edge order (EdgeIDCompare: insertion order); a pair may occur more than once       */
    const float*   points;        /* n_points x 3: GetWorldPos()                                                               */
    const int32_t* point_ref;     /* per point the vertex of nIDr, or -1: both Sim3 of step 7 are the default-constructed one  */
} orbm_eg_problem;
typedef struct orbm_eg_result {
    double* estimate;              /* n_vertices x 8: the estimates after optimize()                                    */
    float* Tiw;                    /* n_vertices x 16: what SetPose receives: R, t * (1./s), Converter::toCvSE3         */
    float* point_f;                /* n_points x 3: what SetWorldPos receives                                           */
    orbm_pose_round round;         /* of the one optimize()                                                             */
    int32_t optimised;             /* 1: optimize() had an active free vertex                                           */
    int32_t active_vertices, active_edges;   /* of initializeOptimization(): vertices with an edge (fixed ones included), edges */
    int32_t reserved;
} orbm_eg_result;
/* On the device: per linearisation the perturbed estimates once per vertex, one lane per (edge, evaluation), the blocks over the pairs
 * that exist; per Levenberg trial the damping, the blocked LDL^T (csrc/ba_ldlt_dev.h), the update, the errors, the controller, one
 * synchronisation and one 4-byte command word; k_eg_correct_points behind the last iteration.  A problem beyond a cap
 * (ORBM_EG_MAX_*), or without an active free vertex, runs through the host routine in DEVICE order inside the same call
 * (orbm_debug_last_essential_graph).  Same bytes as orbm_essential_graph_host(..., ORBM_POSE_ORDER_DEVICE). */
int orbm_essential_graph(orbm_matcher* m, const orbm_eg_problem* problem, int n_iterations, orbm_eg_result* result);
/* The same statements on the host, no device needed, in either order. */
int orbm_essential_graph_host(const orbm_eg_problem* problem, int n_iterations, int order, orbm_eg_result* result);
/* (test hooks, host only) One edge at two estimates (8 doubles each): out[0..6] the error, out[7] chi2, out[8..56] the Jacobian by
 * vertex 0, out[57..105] by vertex 1 (7 x 7 row-major: row the error, column the dimension).  The logarithm alone: out[0..6], returns
 * the branch (0: |sigma| < eps and d > 1 - eps, 1: |sigma| < eps, 2: d > 1 - eps, 3: neither) or a negative error. */
int orbm_eg_edge_eval(const double* measurement8, const double* v0_8, const double* v1_8, int fix_scale, int order, double* out106);
int orbm_sim3_log_eval(const double* sim3_8, int order, double* out7);
/* (test hooks, host only) The arc cosine and the natural logarithm of the DEVICE order. */
double orbm_pose_acos(double d);
double orbm_pose_log(double x);

/* -- PnPsolver: every EPnP RANSAC hypothesis of a relocalisation in one call ---------------------------------------------
 * PnPsolver (reference src/PnPsolver.cc) between SearchByBoW_cam1 and Optimizer::PoseOptimization of Tracking::Relocalization: per
 * hypothesis the four-point EPnP (compute_pose: choose_control_points, compute_barycentric_coordinates, M^T M, its 12x12 SVD, the three
 * beta approximations with five Gauss-Newton steps each, estimate_R_and_t, the reprojection error) and CheckInliers; per record --
 * a hypothesis that `iterate` makes its best -- Refine(): the n-point compute_pose on the record's inlier set and CheckInliers again.
 * No iteration depends on another, so all hypotheses of all candidates are evaluated at once and orbm_pnp_walk recovers the
 * reference's sequential `iterate` from the counts and the refined records.  RANSAC's randomness is an INPUT: the quadruples arrive drawn.
 * The OpenCV operators on the path (cvMulTransposed, cvSVD, cvInvert, cvSolve) are restated one function each and UNPINNED (DESIGN.md
 * section 2).  Everything below compute_pose is + - * / sqrt fabs in double: there is ONE order, no transcendental function, and every
 * sum runs in the reference's element order on the device as on the host.
 * The one stated deviation: qr_solve's result `x` is an uninitialised stack array in the reference's gauss_newton and qr_solve returns
 * without writing it when a column is all zero.  Here x starts as zeros at the entry of gauss_newton, a singular return leaves it as
 * it was, and the record carries ORBM_PNP_FLAG_SINGULAR_QR. */
enum { ORBM_PNP_CAP = 8192,         /* correspondences of one problem the device takes; a longer one runs on the host inside the same call */
       ORBM_PNP_MAX_ITS = 1024,     /* hypotheses of one problem (the reference draws at most 300 per block)                              */
       ORBM_PNP_MAX_BATCH = 64,
       ORBM_PNP_MAX_RECORDS = 16 }; /* refined records of one problem the device takes; later ones are refined on the host inside the same call */
enum { ORBM_PNP_FLAG_SINGULAR_QR = 1,   /* qr_solve met an all-zero column in some Gauss-Newton step                                        */
       ORBM_PNP_FLAG_RANDOM_SVD = 2 };  /* some cvSVD completed U with the random-vector branch (a singular value <= DBL_MIN)              */

typedef struct orbm_pnp_problem {
    double fu, fv, uc, vc;         /* F.fx, F.fy, F.cx, F.cy widened to the solver's double members                     */
    int32_t min_inliers;           /* mRansacMinInliers after SetRansacParameters (orbm_pnp_parameters)                 */
    int32_t best_start;            /* mnBestInliers on entry: 0 for a fresh solver                                      */
} orbm_pnp_problem;                /* 40 bytes */

typedef struct orbm_pnp_hyp {      /* one iteration of `iterate` */
    double R[9], t[3], rep_error;  /* mRi (row-major), mti, compute_pose's return value                                 */
    int32_t choice;                /* 1..3: which beta approximation won                                                */
    int32_t n_inliers;             /* mnInliersi                                                                        */
    int32_t flags;                 /* ORBM_PNP_FLAG_*                                                                   */
    int32_t reserved;              /* 0: the fourth int32 that keeps the record free of implicit padding                */
} orbm_pnp_hyp;                    /* 120 bytes, no padding */

typedef struct orbm_pnp_refined {  /* Refine() on one record */
    int32_t hyp;                   /* the record's hypothesis (position inside the problem)                             */
    int32_t n_set;                 /* points of the n-point compute_pose = the record's n_inliers                       */
    int32_t n_inliers;             /* mnRefinedInliers                                                                  */
    int32_t flags;                 /* ORBM_PNP_FLAG_*                                                                   */
    double R[9], t[3];             /* mRi, mti after the n-point compute_pose                                           */
} orbm_pnp_refined;                /* 112 bytes, no padding */

/* B problems (1 .. ORBM_PNP_MAX_BATCH), one enqueue (four kernels back to back), one synchronisation.  Correspondences are CSR per
 * problem: problem b owns first[b] .. first[b+1]-1, in the order of the constructor's push_backs:
 *   p3dw[3i..]    mvP3Dw[i] (world position, floats)
 *   p2d[2i..]     mvP2D[i] = mvKeysUn[.].pt
 *   max_err[i]    mvMaxError[i] = mvSigma2[i]*th2 in float
 * Hypotheses are CSR per problem too: problem b owns its_first[b] .. its_first[b+1]-1 (at most ORBM_PNP_MAX_ITS), hypothesis g draws
 * the correspondences quads[4g..4g+3] (positions inside the problem, 0 .. N_b-1) in drawing order -- EPnP's sums depend on it.
 * hyp_out[g] is the record of hypothesis g.  mask_out is laid out as orbm_sim3_ransac's: one bit per correspondence, W_b = (N_b + 63) / 64
 * words per hypothesis, hypothesis-major inside a problem, the problems one after another.
 * The problem's RECORDS are the strict prefix maxima of n_inliers above best_start among the hypotheses with n_inliers >= min_inliers,
 * in order: exactly the hypotheses `iterate` would copy into mvbBestInliers.  n_records_out[b] counts them (all of them).  Record r <
 * ORBM_PNP_MAX_RECORDS of problem b is refined_out[b*ORBM_PNP_MAX_RECORDS + r], its mask W_b words at refined_mask_out[16 * (sum over
 * b' < b of W_b') + r*W_b]: Refine() on the record's mask -- the n-point compute_pose, then CheckInliers.  Unused slots are zero.
 * Records beyond ORBM_PNP_MAX_RECORDS are refined by the host routine inside the same call and APPENDED by the caller's leave:
 * refined_out is sized by the caller for B*ORBM_PNP_MAX_RECORDS + extra_cap records and refined_mask_out for 16 * (sum of W_b) words +
 * the extra records' W_b words each; the extra records follow in problem order, then record order, from refined_out[B *
 * ORBM_PNP_MAX_RECORDS] and from the end of the regular mask block.  More extra records than extra_cap: ORB_E_CAPACITY, nothing of the
 * extras is written (min(H_b, N_b) - ORBM_PNP_MAX_RECORDS per problem always suffices).
 * Device memory: the handle keeps, and reuses, a block sized by its largest call -- per device problem 120 B per hypothesis, 8 B per mask
 * word and, for the inlier sets and per-point arrays of the ORBM_PNP_MAX_RECORDS refinements, 16 x 60 B per correspondence (a record's
 * set can be the whole problem, and how many records there are is known only on the device): 1 MB per 1 000 correspondences, 500 MB for
 * the largest call there is (64 problems of 8 192).
 * A NaN is written as the NaN x86 makes from an invalid operation; what a non-finite INPUT gives is unspecified.  A problem beyond
 * ORBM_PNP_CAP correspondences runs through the host routine inside the same call (orbm_debug_last_pnp, include/orb_debug.h). */
int orbm_pnp_ransac(orbm_matcher* m, const orbm_pnp_problem* problems, int B, const int32_t* first, const float* p3dw, const float* p2d,
                    const float* max_err, const int32_t* its_first, const int32_t* quads, orbm_pnp_hyp* hyp_out, uint64_t* mask_out,
                    int32_t* n_records_out, orbm_pnp_refined* refined_out, uint64_t* refined_mask_out, int extra_cap);
/* The same routine entirely on the host, no device needed, the same bytes: there is one order. */
int orbm_pnp_ransac_host(const orbm_pnp_problem* problems, int B, const int32_t* first, const float* p3dw, const float* p2d,
                         const float* max_err, const int32_t* its_first, const int32_t* quads, orbm_pnp_hyp* hyp_out, uint64_t* mask_out,
                         int32_t* n_records_out, orbm_pnp_refined* refined_out, uint64_t* refined_mask_out, int extra_cap);

/* The reference's `iterate` loop over precomputed counts and records (host only; the class, the Python wrapper and the tests share it). */
typedef struct orbm_pnp_walk_state {
    int32_t iterations;            /* mnIterations                                                                      */
    int32_t best_inliers;          /* mnBestInliers; start a solver with 0                                              */
    int32_t best_hyp;              /* the iteration (counted from the solver's first) mBestTcw was taken from; start with -1 */
    int32_t best_record;           /* the record of THIS block that holds mvbBestInliers, -1 while the best comes from an earlier block */
    int32_t best_refined_inliers;  /* mnRefinedInliers of Refine() on the current best: carried from block to block; start with 0 */
    int32_t no_more;               /* bNoMore of the call                                                               */
    int32_t current;               /* nCurrentIterations of the call in progress                                        */
    int32_t exhausted;             /* 1: the loop wants iteration `iterations` and the block ends before it: evaluate a continuation
                                      block (best_start = best_inliers) and call again with the same state               */
} orbm_pnp_walk_state;
enum { ORBM_PNP_WALK_NOTHING = 0,  /* the empty cv::Mat                                                                 */
       ORBM_PNP_WALK_REFINED = 1,  /* mRefinedTcw: Refine() on the current best succeeded                               */
       ORBM_PNP_WALK_BEST = 2 };   /* mBestTcw: the exit at mnIterations >= mRansacMaxIts                               */
/* iterate(n_iterations, ...) on a block of evaluated hypotheses: counts[0 .. H-1] are the n_inliers of the iterations block_start ..
 * block_start + H - 1, rec_hyp[r] / rec_inliers[r] (r < n_rec) the block's records (position inside the block, refined n_inliers).
 * Transcribed literally: `while(mnIterations<mRansacMaxIts || nCurrentIterations<nIterations)` with ||; a hypothesis becomes the best
 * with `>= min_inliers` and strict `> mnBestInliers`; Refine() runs on the CURRENT best at every iteration with `>= min_inliers` and
 * succeeds on strict `> min_inliers`; `mnIterations >= mRansacMaxIts` at the end sets bNoMore and answers mBestTcw when
 * `mnBestInliers >= min_inliers`.  A call whose state has exhausted == 1 continues the interrupted call (current is kept), any
 * other starts one.  N < min_inliers answers NOTHING at once with no_more set. */
int orbm_pnp_walk(const int32_t* counts, int H, int block_start, const int32_t* rec_hyp, const int32_t* rec_inliers, int n_rec, int N,
                  int min_inliers, int max_its, int n_iterations, orbm_pnp_walk_state* state);
/* SetRansacParameters' arithmetic: `int nMinInliers = N*mRansacEpsilon` (a float product, truncated as x86 does: INT_MIN for a NaN or
 * a value out of range), the two lower clamps, epsilon raised to (float)mRansacMinInliers/N, ceil(log(1-p)/log(1-pow(eps,3))) with the
 * exponent 3, max(1, min(., max_its)).  out2 = {mRansacMaxIts, mRansacMinInliers}, *epsilon_out = mRansacEpsilon. */
int orbm_pnp_parameters(double probability, int min_inliers, int max_its, int min_set, float epsilon, int N, int32_t* out2, float* epsilon_out);
/* (test hooks, host only) cvSVD of an m x n matrix, m >= n, row-major: w n values, ut n x m (U transposed), vt n x n (may be NULL);
 * returns 1 when the random completion ran.  qr_solve(A nr x nc, b nr) -> x nc (left alone on a singular return), returns 1 when
 * singular; A and b are destroyed.  compute_pose of n points: pws 3n, us 2n doubles, K = fu fv uc vc -> R 9, t 3, out2 = {choice, flags},
 * returns the reprojection error. */
int orbm_pnp_svd(const double* A, int m, int n, double* w, double* ut, double* vt);
int orbm_pnp_qr_solve(double* A, int nr, int nc, double* b, double* x);
double orbm_pnp_compute_pose(const double* pws, const double* us, int n, const double* K4, double* R9, double* t3, int32_t* out2);

#ifdef __cplusplus
}
#endif
#endif
