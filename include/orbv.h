/* orbv.h -- C ABI of the vocabulary-tree transform and the BoW-gated searches.
 *
 * Replaces:
 *   ORBVocabulary (= DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>)
 *     loadFromTextFile          reference Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1339-1425  -> orbv_load_text
 *     transform(feature, ...)   reference TemplatedVocabulary.h:1219-1260 (one descent: at every level the FIRST child
 *                               with the smallest Hamming distance, FORB.cpp:77-96)               -> orbv_transform[_device]
 *     transform(features, BowVector&, FeatureVector&, levelsup)
 *                               reference TemplatedVocabulary.h:1127-1180, BowVector.cpp:34-84,
 *                               FeatureVector.cpp:31-45 (TF_IDF weighting, L1 norm: what ORBvoc.txt declares; callers
 *                               src/Frame.cc:649-659, src/KeyFrame.cc ComputeBoW)                 -> orbv_bow_vectors
 *     score(BowVector, BowVector)  reference ScoringObject.cpp:23-68 (L1)                         -> orbv_score_l1
 *   int ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&)
 *                               reference include/ORBmatcher.h:64, src/ORBmatcher.cc:206-388      -> orbv_search_by_bow, mode 0
 *   int ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vector<MapPoint*>&)
 *                               reference include/ORBmatcher.h:65, src/ORBmatcher.cc:996-1165     -> orbv_search_by_bow, mode 1
 *   int ORBmatcher::SearchForTriangulation(KeyFrame*, KeyFrame*, cv::Mat F12, vector<pair<size_t,size_t>>&, bool, vector<bool>)
 *                               reference include/ORBmatcher.h:85-87, src/ORBmatcher.cc:1364-1786 -> orbv_search_for_triangulation
 *
 * No KeyFrame* / MapPoint* / std::map crosses the ABI: a DBoW2::FeatureVector travels as CSR arrays (node ids ascending, as
 * the std::map iterates; feature indices per node in push_back order), MapPoint validity as one flag byte per feature.
 * The vocabulary file itself is not part of the reference checkout (Vocabulary/ORBvoc.txt.tar.gz is a missing blob):
 * orbv_load_text reads the text format the reference's loader reads, orbv_create takes the same tree from arrays.
 *
 * A vocabulary handle and a search workspace each own one HIP stream and scratch buffers: the (large, read-only) tree may be
 * shared by threads only through orbv_transform_device; everything else is one handle per calling thread.
 */
#ifndef ORBV_H
#define ORBV_H
#include "orb_types.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct orbv_vocabulary orbv_vocabulary;
typedef struct orbv_workspace orbv_workspace; /* stream + scratch of the BoW-gated searches (an ORBmatcher owns one) */

/* Tree from arrays, node ids as the reference's loader assigns them (TemplatedVocabulary.h:1377-1421): node 0 is the
 * root (its parent / descriptor / weight entries are ignored), parent[i] < i is not required but parent[i] must exist;
 * children are visited in ascending node id; word ids count the nodes flagged is_leaf in id order; a descent ends at the
 * first node without children.  desc: n_nodes x 32 bytes; weight: n_nodes doubles (idf of the words). */
int orbv_create(int n_nodes, int L, const int32_t* parent, const uint8_t* is_leaf, const uint8_t* desc, const double* weight,
                int device, orbv_vocabulary** out);
/* "k L scoring weighting" header line, then one line per node: parent is_leaf 32 descriptor bytes weight.  Only
 * scoring 0 (L1_NORM) with weighting 0 (TF_IDF) -- the ORBvoc.txt configuration -- is accepted.  A trailing empty line is
 * ignored (the reference's `while(!f.eof())` turns it into a node with an uninitialised descriptor). */
int orbv_load_text(const char* path, int device, orbv_vocabulary** out);
void orbv_destroy(orbv_vocabulary* v);
int orbv_info(const orbv_vocabulary* v, int* n_nodes, int* n_words, int* k, int* L);
void* orbv_stream(orbv_vocabulary* v);

/* One descent per feature.  features: n x 32 bytes on the host; word_id / node_id: n entries each (node_id = the node
 * `levelsup` levels above the leaves, 0 when L - levelsup <= 0).  weight may be NULL. */
int orbv_transform(orbv_vocabulary* v, const uint8_t* features, int n, int levelsup, uint32_t* word_id, uint32_t* node_id,
                   double* weight);
/* Enqueue-only form for resident descriptors (e.g. the block orbf_export_block hands out): device pointers, caller's stream. */
int orbv_transform_device(const orbv_vocabulary* v, const uint8_t* d_features, int n, int levelsup, uint32_t* d_word_id,
                          uint32_t* d_node_id, void* stream);

/* BowVector + FeatureVector of one frame: descents on the device, the two std::map constructions restated on flat
 * arrays on the host (double sums in feature order, L1 normalisation in ascending word order -- bit-identical doubles).
 * Outputs hold up to n entries (fv_start: n + 1).  *n_words / *n_fv_nodes receive the entry counts. */
int orbv_bow_vectors(orbv_vocabulary* v, const uint8_t* features, int n, int levelsup, uint32_t* bow_id, double* bow_val,
                     int* n_words, uint32_t* fv_node, int32_t* fv_start, uint32_t* fv_items, int* n_fv_nodes);
double orbv_score_l1(const uint32_t* id1, const double* v1, int n1, const uint32_t* id2, const double* v2, int n2);

int orbv_workspace_create(int device, orbv_workspace** out);
void orbv_workspace_destroy(orbv_workspace* w);

/* One frame / keyframe as the BoW searches read it. */
typedef struct orbv_side {
    int n;                     /* features (N_total)                                                                  */
    const uint8_t* desc;       /* n x 32, global feature order (mDescriptors_total[cam].row(local))                  */
    const float* angle;        /* n: mvKeysUn_total[i].angle (mvKeys_total for a Frame: undistortion keeps the angle) */
    const uint8_t* flags;      /* n, or NULL = every feature usable and not stereo.  bit0 usable, bit1 stereo        */
    int n_nodes;               /* FeatureVector entries                                                               */
    const uint32_t* node_id;   /* n_nodes, strictly ascending                                                         */
    const int32_t* node_start; /* n_nodes + 1                                                                         */
    const uint32_t* items;     /* node_start[n_nodes] feature indices                                                 */
    const float* x;            /* triangulation only: mvKeysUn_total[i].pt                                            */
    const float* y;
    const int32_t* octave;     /* triangulation only                                                                  */
    const int32_t* cam_of;     /* triangulation only: keypoint_to_cam                                                 */
} orbv_side;

/* mode 0, SearchByBoW(pKF, F, vpMapPointMatches): a = pKF with flags bit0 = "has a MapPoint that is not bad", b = F;
 *         match[] has b->n entries: index of the keyframe feature whose MapPoint lands in vpMapPointMatches[i], or -1;
 *         accepted when best <= th_low and (float)best < nnratio * (float)second.
 * mode 1, SearchByBoW(pKF1, pKF2, vpMatches12): flags bit0 on both sides as above; match[] has a->n entries: feature of
 *         pKF2 whose MapPoint lands in vpMatches12[i], or -1; accepted when best < th_low (strict) and the ratio test.
 * Rotation-histogram filter when check_orientation != 0.  *nmatches = the reference's return value. */
int orbv_search_by_bow(orbv_workspace* w, const orbv_side* a, const orbv_side* b, int mode, int th_low, float nnratio,
                       int check_orientation, int32_t* match, int* nmatches);

enum { ORBV_MAX_CAMS = 8 };
typedef struct orbv_triangulation {
    int n_cams, n_levels;
    float F12[ORBV_MAX_CAMS][9];                /* F12s[cam], row-major (reference src/ORBmatcher.cc:1395-1399)        */
    float ex[ORBV_MAX_CAMS], ey[ORBV_MAX_CAMS]; /* epipole of pKF1's camera c in pKF2's camera c (:1407-1416)          */
    const float* scale_factors;                 /* pKF2->mvScaleFactors, n_levels                                      */
    const float* level_sigma2;                  /* pKF2->mvLevelSigma2, n_levels                                       */
} orbv_triangulation;

/* SearchForTriangulation from the fundamental matrices on.  flags bit0: the feature takes part (no MapPoint yet, its camera
 * enabled in vbCam, stereo when bOnlyStereo); bit1: mvuRight_total >= 0.  match[] has a->n entries (feature of pKF2 or -1):
 * vMatchedPairs is {(i, match[i]) : match[i] >= 0} in ascending i.  *nmatches = the reference's return value. */
int orbv_search_for_triangulation(orbv_workspace* w, const orbv_side* a, const orbv_side* b, const orbv_triangulation* t,
                                  int th_low, int check_orientation, int32_t* match, int* nmatches);

/* Resident form: a frame / keyframe is uploaded once (descriptors, angles, FeatureVector and -- when s->x is given -- the
 * triangulation arrays; the caller's arrays are free again on return) and searched any number of times.  The MapPoint state
 * changes between searches, so every search takes the two flag arrays of the moment (a->n / b->n bytes, meaning as above;
 * NULL = the flags uploaded with the keyframe, which may themselves be NULL = all usable). */
typedef struct orbv_keyframe orbv_keyframe;
int orbv_keyframe_create(orbv_workspace* w, const orbv_side* s, orbv_keyframe** out);
void orbv_keyframe_destroy(orbv_keyframe* k);
int orbv_keyframe_count(const orbv_keyframe* k);
/* A keyframe that never leaves HBM: descriptors, angles (and positions / octaves / right coordinates for triangulation)
 * are copied device-to-device -- e.g. from the frame orbf_export_features hands out --, the descents run on them and the
 * FeatureVector is built on the device (the nodes `levelsup` above the leaves must number <= 4096: 100 for the stock
 * k = 10, L = 6 vocabulary at levelsup = 4).  Flags start as bit0 = 1, bit1 = (uright >= 0).  after_stream: the stream the
 * source arrays are produced on (NULL: they are complete).  One synchronisation (the node count comes back to the host). */
typedef struct orbv_device_side {
    int n;
    const uint8_t* d_desc;     /* n x 32, 16-byte aligned                       */
    const float* d_angle;      /* n                                             */
    const float* d_x;          /* n, or NULL: no triangulation arrays           */
    const float* d_y;
    const int32_t* d_octave;
    const float* d_uright;     /* n, or NULL (= no feature is stereo)           */
    int n_cams;                /* cameras are contiguous index ranges:          */
    int cam_start[9];          /* camera c = [cam_start[c], cam_start[c+1])     */
} orbv_device_side;
int orbv_keyframe_from_device(orbv_workspace* w, const orbv_vocabulary* v, const orbv_device_side* s, int levelsup, void* after_stream,
                              orbv_keyframe** out);
/* Per-feature word / node ids of a device-built keyframe (for the BowVector, which stays a host std::map) and its
 * FeatureVector as CSR; any output pointer may be NULL.  fv_items needs fv_start. */
int orbv_keyframe_download(orbv_workspace* w, const orbv_keyframe* k, uint32_t* word_id, uint32_t* node_of_feature, uint32_t* fv_node,
                           int32_t* fv_start, uint32_t* fv_items, int* n_fv_nodes);

int orbv_search_by_bow_resident(orbv_workspace* w, const orbv_keyframe* a, const uint8_t* flags_a, const orbv_keyframe* b,
                                const uint8_t* flags_b, int mode, int th_low, float nnratio, int check_orientation, int32_t* match,
                                int* nmatches);
int orbv_search_for_triangulation_resident(orbv_workspace* w, const orbv_keyframe* a, const uint8_t* flags_a, const orbv_keyframe* b,
                                           const uint8_t* flags_b, const orbv_triangulation* t, int th_low, int check_orientation,
                                           int32_t* match, int* nmatches);

/* ---- Triangulation and gating of new map points: the loop over the matched pairs in LocalMapping::CreateNewMapPoints (reference
 * src/LocalMapping.cc:388-669) with KeyFrame::UnprojectStereo (src/KeyFrame.cc:985-1012), up to, not including, `new MapPoint`.
 * One statement sequence (csrc/triangulate.hip) serves the kernel and the host routine; DESIGN.md section 2 lists the operators at
 * the OpenCV boundary whose parity is unpinned (the Jacobi SVD, its hypot replacement, the weighted row difference, v / w). */
typedef struct orbv_tri_keyframe {
    float Tcw[2][12];          /* per camera [R|t], 3x4 row-major: GetRotation / GetTranslation and their _cam2 forms         */
    float centre[2][3];        /* GetCameraCenter, GetCameraCenter_cam2                                                      */
    float Twc[12];             /* Twc.rowRange(0,3), 3x4 row-major (UnprojectStereo)                                         */
    float Rcam12[9], tcam12[3];/* mRcam12, mtcam12 (UnprojectStereo, camera 2)                                               */
    float fx, fy, cx, cy, invfx, invfy, mbf;
    int n_levels;
    const float* scale_factors;/* mvScaleFactors, n_levels                                                                   */
    const float* level_sigma2; /* mvLevelSigma2, n_levels                                                                    */
    int n;                     /* features (N_total)                                                                         */
    int n_cam1;                /* the reference's N: UnprojectStereo takes camera 2 for i >= N                               */
    /* per feature, n entries each.  The resident calls ignore these nine and read the keyframe's own arrays instead.        */
    const float* x;            /* mvKeysUn_total[i].pt                                                                       */
    const float* y;
    const float* xd;           /* mvKeys_total[i].pt (distorted: what UnprojectStereo reads)                                 */
    const float* yd;
    const int32_t* octave;     /* mvKeysUn_total[i].octave                                                                   */
    const float* uright;       /* mvuRight_total                                                                             */
    const float* depth;        /* mvDepth_total                                                                              */
    const float* cos_stereo;   /* orbv_cos_stereo(mb, depth): read where uright >= 0 only                                    */
    const int32_t* cam_of;     /* keypoint_to_cam, or NULL = (i >= n_cam1)                                                   */
} orbv_tri_keyframe;

enum { ORBV_TRI_NONE = 0,         /* no pair (the fused call's record where match[i] < 0)   */
       ORBV_TRI_ACCEPTED = 1,     /* reached `new MapPoint`                                  */
       ORBV_TRI_CAM_OFF = 2,      /* istrian[camIdx1] == false                         :414  */
       ORBV_TRI_LOW_PARALLAX = 3, /* no stereo and very low parallax                   :515  */
       ORBV_TRI_W_ZERO = 4,       /* x3D.at<float>(3) == 0                             :491  */
       ORBV_TRI_Z1 = 5,           /* z1 <= 0                                           :527  */
       ORBV_TRI_Z2 = 6,           /* z2 <= 0                                           :530  */
       ORBV_TRI_REPROJ1 = 7,      /* chi-square test in the current keyframe           :577  */
       ORBV_TRI_REPROJ2 = 8,      /* chi-square test in the neighbour                  :620  */
       ORBV_TRI_ZERO_DIST = 9,    /* dist1 == 0 || dist2 == 0                          :657  */
       ORBV_TRI_SCALE = 10 };     /* scale consistency                                 :668  */
enum { ORBV_TRI_PATH_NONE = 0, ORBV_TRI_PATH_SVD = 1, ORBV_TRI_PATH_UNPROJECT1 = 2, ORBV_TRI_PATH_UNPROJECT2 = 3 };
typedef struct orbv_tri_out {
    float x3D[3];              /* the point whenever one was computed, also for a rejected pair (w == 0: the first three
                                  components of the null vector); a NaN is written as 0xffc00000                              */
    int32_t outcome;           /* ORBV_TRI_*                                                                                  */
    int32_t path;              /* ORBV_TRI_PATH_*                                                                             */
} orbv_tri_out;

/* cos(2*atan2(mb/2, depth[i])) as the reference's translation unit evaluates it (float overloads: atan2f, cosf), for every feature.
 * Host libm; the device never evaluates it. */
int orbv_cos_stereo(float mb, const float* depth, int n, float* cos_stereo);
/* pairs: n_pairs x 2 int32 (idx1 in kf1 = the current keyframe, idx2 in kf2); cam_enabled: the reference's istrian, 2 bytes;
 * ratio_factor = 1.5f * mfScaleFactor.  ORB_E_ARG (the offender named in orb_last_error()): an index out of range, an octave outside
 * n_levels, a camera id outside cam_enabled, a stereo feature (uright >= 0) whose depth is not positive (the reference's
 * UnprojectStereo returns an empty matrix there and the caller faults), a null array.  Needs no device. */
int orbv_triangulate_pairs_host(const orbv_tri_keyframe* kf1, const orbv_tri_keyframe* kf2, const uint8_t* cam_enabled, const int32_t* pairs,
                                int n_pairs, float ratio_factor, orbv_tri_out* out);
/* The same on the workspace's stream: one lane per pair, one synchronisation. */
int orbv_triangulate_pairs(orbv_workspace* w, const orbv_tri_keyframe* kf1, const orbv_tri_keyframe* kf2, const uint8_t* cam_enabled,
                           const int32_t* pairs, int n_pairs, float ratio_factor, orbv_tri_out* out);
/* Adds to a resident keyframe (built with the triangulation arrays) the per-feature arrays this stage reads beyond them:
 * orbv_keyframe_count(k) entries each, copied from the host; the searches on the keyframe are unaffected. */
int orbv_keyframe_set_geometry(orbv_workspace* w, orbv_keyframe* k, const float* uright, const float* depth, const float* cos_stereo,
                               const float* xd, const float* yd);
typedef struct orbv_tri_geometry {
    orbv_tri_keyframe kf1, kf2;   /* poses, intrinsics, level tables, n_cam1; the per-feature pointers and n are ignored */
    uint8_t cam_enabled[2];
    float ratio_factor;
} orbv_tri_geometry;
/* orbv_search_for_triangulation_resident followed by the triangulation of its pairs, the match words read where the search leaves
 * them in HBM: one synchronisation.  match[] / the return of the search as there; out[i] (a->n records) belongs to the pair
 * (i, match[i]) and is all zero where match[i] < 0; *n_accepted counts ORBV_TRI_ACCEPTED.  Both keyframes need
 * orbv_keyframe_set_geometry.  A device-built keyframe's octaves are vouched for by the caller, as in the search. */
int orbv_create_new_points_resident(orbv_workspace* w, const orbv_keyframe* a, const uint8_t* flags_a, const orbv_keyframe* b,
                                    const uint8_t* flags_b, const orbv_triangulation* t, const orbv_tri_geometry* geometry, int th_low,
                                    int check_orientation, int32_t* match, orbv_tri_out* out, int* n_accepted);

/* LocalMapping::CreateNewMapPoints for ALL neighbours of a keyframe (reference src/LocalMapping.cc:315-690) in one enqueue with one
 * synchronisation.  The call is defined by the loop it replaces.  A state free[i] starts as bit 0 of flags_a[i] (flags_a == NULL: of the
 * flags uploaded with `a`; those NULL too: every feature is free).  Round k is exactly
 *     orbv_create_new_points_resident(w, a, <flags>, rounds[k].b, rounds[k].flags_b, &rounds[k].t, &rounds[k].geometry, ...)
 * with <flags>[i] = flags_a[i] with bit 0 replaced by free[i] && rounds[k].geometry.cam_enabled[cam_of[i]] (the reference's vbCam
 * filter inside SearchForTriangulation and its istrian[camIdx1] test at :414 are the same bits, so ORBV_TRI_CAM_OFF cannot occur
 * here), and writes match + k*a->n, out + k*a->n, n_matches[k] and n_accepted[k].  After round k, free[i] = 0 wherever the round's
 * record has outcome == ORBV_TRI_ACCEPTED (mpCurrentKeyFrame->AddMapPoint(pMP, idx1), :682; the next neighbour's search skips the
 * feature, src/ORBmatcher.cc !pKF1->GetMapPoint(i)); no other outcome takes a feature out.  The update runs on the device
 * (k_triangulate_round): the state and the round's flags live in the workspace, the flags stored with `a` are never written.
 * Every output equals, byte for byte, what that loop of calls returns.  geometry.kf1 describes `a` in every round.
 * Validation is all or nothing and precedes the first launch: everything orbv_create_new_points_resident checks, for every round
 * (orb_last_error() names the round), and 0 <= n_rounds <= ORBV_MAX_ROUNDS.  A round whose search has an empty side launches
 * nothing, returns all -1 / zero records and leaves free[] alone; n_rounds == 0 or a->n == 0 launches nothing at all.
 * One deviation from the reference: it abandons the remaining neighbours when CheckNewKeyFrames() turns true between two of them
 * (:318); one enqueue cannot, so the caller checks before the call and gets all neighbours. */
enum { ORBV_MAX_ROUNDS = 32 };            /* the reference asks for 15 neighbours (20 monocular) */
typedef struct orbv_new_points_round {    /* one neighbour */
    const orbv_keyframe* b;               /* resident, with geometry */
    const uint8_t* flags_b;               /* b->n bytes, or NULL: as in orbv_create_new_points_resident */
    orbv_triangulation t;                 /* F12 / epipoles of (a, b), b's level tables */
    orbv_tri_geometry geometry;           /* kf1 = a (the same in every round), kf2 = b, cam_enabled = this round's istrian, ratio_factor */
} orbv_new_points_round;
int orbv_create_new_points_keyframe(orbv_workspace* w, const orbv_keyframe* a, const uint8_t* flags_a,
                                    const orbv_new_points_round* rounds, int n_rounds, int th_low, int check_orientation,
                                    int32_t* match /* n_rounds x a->n */, orbv_tri_out* out /* n_rounds x a->n */,
                                    int* n_matches /* n_rounds */, int* n_accepted /* n_rounds */);

/* Resident keyframe database: KeyFrameDatabase's inverted-file walk and the scores behind it (reference src/KeyFrameDatabase.cc:132-153,
 * :187, :429-446, :477; LoopClosing::DetectLoop's minScore loop, src/LoopClosing.cc:150-170) without an inverted file.  Every BowVector
 * added stays in HBM (word ids strictly ascending, values double); one pass of k_db_query over all of them gives, per entry, the number
 * of words shared with the query, the smallest shared word and L1Scoring::score(query, entry) -- bit-identical to orbv_score_l1.
 * One handle = one stream + scratch, one calling thread at a time.  Word ids >= n_words, unsorted or duplicate ids, n < 0 or
 * n > 65535: ORB_E_ARG. */
typedef struct orbv_database orbv_database;
int orbv_db_create(int n_words, int device, orbv_database** out);
void orbv_db_destroy(orbv_database* db);
/* key already present: ORB_E_ARG (the database is unchanged).  n == 0 is accepted: an empty BowVector is stored (it counts in
 * orbv_db_count and can be erased) and is never returned by a query.  The call returns after the upload has completed. */
int orbv_db_add(orbv_database* db, uint64_t key, const uint32_t* id, const double* val, int n);
/* unknown key: no-op, returns 0 (reference :63-97).  The arena is compacted once dead words exceed half of it. */
int orbv_db_erase(orbv_database* db, uint64_t key);
int orbv_db_clear(orbv_database* db);
int orbv_db_count(const orbv_database* db); /* alive entries */
/* Per query q: the entries that share at least one word with it, in the order the reference's lKFsSharingWords has them (ascending
 * smallest shared word, then add order), as rows of `capacity` in key / common / score; n_hits[q] = their number.  A query with more
 * hits than `capacity` is ORB_E_ARG, never a truncated answer (capacity = orbv_db_count() always suffices).  At most
 * ORBV_DB_MAX_QUERIES queries per call, and n_queries x orbv_db_count() <= 2^26 (16 B per pair come back): more is ORB_E_ARG. */
enum { ORBV_DB_MAX_QUERIES = 1024 };
int orbv_db_query(orbv_database* db, int n_queries, const uint32_t* const* id, const double* const* val, const int* n, int capacity,
                  uint64_t* key, int32_t* common, double* score, int* n_hits);
/* L1 score of one query against the named entries (score[k] for keys[k]); a key that is not in the database: ORB_E_ARG. */
int orbv_db_score(orbv_database* db, const uint32_t* id, const double* val, int n, const uint64_t* keys, int n_keys, double* score);

#ifdef __cplusplus
}
#endif
#endif
