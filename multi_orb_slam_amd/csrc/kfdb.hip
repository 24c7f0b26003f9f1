// kfdb.hip -- resident keyframe database: the first half of place recognition (include/orbv.h, orbv_db_*).
//
// Replaces the inverted-file walk of KeyFrameDatabase::DetectLoopCandidates[_cam1] / DetectRelocalizationCandidates (reference
// src/KeyFrameDatabase.cc:132-153, :282-302, :429-446) and the ORBVocabulary::score calls behind it (:187, :335, :477;
// Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68).  No inverted file: every BowVector of the database lies in one arena (word ids
// uint32 strictly ascending, values double) and one pass over it yields, for every alive entry, the three things the list walk yields:
// the number of shared words, the smallest shared word (which fixes the position in lKFsSharingWords) and the L1 score.
//
// k_db_query: one wave per (query, entry).  The query's ids and values lie in LDS (queries of up to DB_LDS_WORDS words) or stay in
// global memory (longer ones); 64 lanes take 64 consecutive entry words, each looks its word up in the query by binary search, a ballot
// gives the count and the shared lanes.  The score is bit-identical to the host's: every lane forms its own term
// fabs(v - w) - fabs(v) - fabs(w) (exact IEEE double operations, no multiply, so nothing to contract), and the terms are added ONE BY
// ONE in ascending word id into a double that starts at 0 -- the wave walks the ballot mask and reads each term with v_readlane.  No tree
// reduction, no reassociation.  Only this chain is serial, and there is one per wave in flight.
#include <algorithm>
#include <unordered_map>
#include <vector>
#include "../../include/orbv.h"
#include "../../include/orb_debug.h"
#include "orb_common.h"
#include "stage_pack.h"

using morb::DevBuf;
using morb::PinnedBuf;

namespace {

constexpr int DB_LDS_WORDS = 4096;   // 4096 x (8 + 4) B = 48 KB of LDS: three workgroups per CU
constexpr int DB_BLOCK = 256;        // four waves
constexpr int DB_MAX_WORDS = 65535;  // a BowVector has at most one word per feature
constexpr int DB_MAX_QUERIES = 1024; // per call (ORBV_DB_MAX_QUERIES): gridDim.y, and 1024 x 65 535 words keep the int offsets far from wrapping
constexpr size_t DB_MAX_OUT_BYTES = (size_t)1 << 30;   // 16 B per (query, entry) come back: 64 M pairs per call

__device__ __forceinline__ double readlane_f64(double v, int lane) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), lane);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// table[e] = (offset, length) of an entry in the arena.  Outputs are indexed [q * n_entries + e].
// grid = (ceil(n_entries / epb), n_queries); workgroup b takes entries [b * epb, (b + 1) * epb), one per wave at a time.
template <bool IN_LDS>
__global__ __launch_bounds__(DB_BLOCK) void k_db_query(const uint32_t* __restrict__ a_id, const double* __restrict__ a_val,
                                                       const uint2* __restrict__ table, int n_entries, int epb,
                                                       const uint32_t* __restrict__ q_id, const double* __restrict__ q_val,
                                                       const int* __restrict__ q_off, int lds_words, double* __restrict__ o_score,
                                                       int32_t* __restrict__ o_common, uint32_t* __restrict__ o_first) {
    extern __shared__ double s_mem[];
    const int q = blockIdx.y;
    const int qb = q_off[q], qn = q_off[q + 1] - qb;
    const uint32_t* ids = q_id + qb;
    const double* vals = q_val + qb;
    if (IN_LDS) {
        double* sv = s_mem;
        uint32_t* si = (uint32_t*)(s_mem + lds_words);
        for (int i = threadIdx.x; i < qn; i += DB_BLOCK) { sv[i] = vals[i]; si[i] = ids[i]; }
        __syncthreads();
        ids = si; vals = sv;
    }
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int e_end = min(n_entries, (int)(blockIdx.x + 1) * epb);
    for (int e = blockIdx.x * epb + wave; e < e_end; e += DB_BLOCK / 64) {
        const uint2 ent = table[e];
        const uint32_t* eid = a_id + ent.x;
        const double* eval = a_val + ent.x;
        const int len = (int)ent.y;
        int common = 0;
        uint32_t first = 0;
        double score = 0.0;
        for (int base = 0; base < len; base += 64) {
            const int i = base + lane;
            const bool valid = i < len;
            const uint32_t w = valid ? eid[i] : 0u;
            int lo = 0, hi = valid ? qn : 0;
            while (lo < hi) {   // lower_bound of w among the query's ids
                const int mid = (lo + hi) >> 1;
                if (ids[mid] < w) lo = mid + 1; else hi = mid;
            }
            const bool found = valid && lo < qn && ids[lo] == w;
            const unsigned long long mask = __ballot(found);
            if (mask == 0) continue;
            double term = 0.0;
            if (found) {
                const double vi = vals[lo], wi = eval[i];
                term = fabs(vi - wi) - fabs(vi) - fabs(wi);
            }
            if (common == 0) first = (uint32_t)__builtin_amdgcn_readlane((int)w, __ffsll((long long)mask) - 1);
            common += __popcll(mask);
            for (unsigned long long m = mask; m; m &= m - 1) score += readlane_f64(term, __ffsll((long long)m) - 1);
        }
        if (lane == 0) {
            const size_t o = (size_t)q * n_entries + e;
            o_score[o] = -score / 2.0;
            o_common[o] = common;
            o_first[o] = first;
        }
    }
}

// Arena compaction: entry e moves from move[e].x to move[e].y (move[e].z words), old arena -> new arena.
__global__ __launch_bounds__(DB_BLOCK) void k_db_compact(const uint32_t* __restrict__ s_id, const double* __restrict__ s_val,
                                                         uint32_t* __restrict__ d_id, double* __restrict__ d_val,
                                                         const uint4* __restrict__ move, int n_entries) {
    const int e = blockIdx.x;
    if (e >= n_entries) return;
    const uint4 mv = move[e];
    for (uint32_t i = threadIdx.x; i < mv.z; i += DB_BLOCK) { d_id[mv.y + i] = s_id[mv.x + i]; d_val[mv.y + i] = s_val[mv.x + i]; }
}

struct Entry { uint64_t key, seq; uint32_t off, len; };

}  // namespace

struct orbv_database {
    int device = 0, n_words = 0;
    hipStream_t stream = nullptr;
    uint32_t* d_id = nullptr;   // arena
    double* d_val = nullptr;
    size_t cap = 0, used = 0, dead = 0;   // words
    std::vector<Entry> entries;           // alive entries, ascending add sequence
    std::unordered_map<uint64_t, uint64_t> seq_of;   // key -> add sequence
    uint64_t next_seq = 0;
    bool table_dirty = true;
    DevBuf<uint2> d_table, d_list;
    DevBuf<uint4> d_move;
    DevBuf<uint8_t> d_q, d_out;
    PinnedBuf<uint8_t> h_q, h_out;
    int last_query[4] = {0, 0, 0, 0};   // {form, epb, workgroups per query, queries} of the last k_db_query launch (orbv_debug_last_db_query)

    int find(uint64_t seq) const {
        auto it = std::lower_bound(entries.begin(), entries.end(), seq, [](const Entry& a, uint64_t s) { return a.seq < s; });
        return (it != entries.end() && it->seq == seq) ? (int)(it - entries.begin()) : -1;
    }
};

namespace {

int check_bow(const orbv_database* db, const uint32_t* id, const double* val, int n) {
    MORB_ARG(n >= 0 && n <= DB_MAX_WORDS && (n == 0 || (id && val)));
    for (int i = 0; i < n; ++i) {
        MORB_ARG(id[i] < (uint32_t)db->n_words);
        MORB_ARG(i == 0 || id[i - 1] < id[i]);   // strictly ascending: sorted, no duplicates
    }
    return ORB_OK;
}

int grow(orbv_database* db, size_t need) {
    if (need <= db->cap) return ORB_OK;
    size_t cap = db->cap ? db->cap : (size_t)1 << 16;
    while (cap < need) cap *= 2;
    MORB_ARG(cap <= ((size_t)1 << 31));   // offsets are 32-bit
    uint32_t* nid = nullptr; double* nval = nullptr;
    MORB_HIP(hipMalloc((void**)&nid, cap * sizeof(uint32_t)));
    if (hipMalloc((void**)&nval, cap * sizeof(double)) != hipSuccess) { (void)hipFree(nid); morb::set_error("hipMalloc of the arena failed"); return ORB_E_HIP; }
    if (db->used) {
        hipError_t err = hipMemcpyAsync(nid, db->d_id, db->used * sizeof(uint32_t), hipMemcpyDeviceToDevice, db->stream);
        if (err == hipSuccess) err = hipMemcpyAsync(nval, db->d_val, db->used * sizeof(double), hipMemcpyDeviceToDevice, db->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(db->stream);
        if (err != hipSuccess) { (void)hipFree(nid); (void)hipFree(nval); morb::set_error("arena growth failed: %s", hipGetErrorString(err)); return ORB_E_HIP; }
    }
    if (db->d_id) (void)hipFree(db->d_id);
    if (db->d_val) (void)hipFree(db->d_val);
    db->d_id = nid; db->d_val = nval; db->cap = cap;
    return ORB_OK;
}

int compact(orbv_database* db) {
    const int E = (int)db->entries.size();
    if (E == 0) { db->used = db->dead = 0; db->table_dirty = true; return ORB_OK; }
    uint32_t* nid = nullptr; double* nval = nullptr;
    MORB_HIP(hipMalloc((void**)&nid, db->cap * sizeof(uint32_t)));
    if (hipMalloc((void**)&nval, db->cap * sizeof(double)) != hipSuccess) { (void)hipFree(nid); morb::set_error("hipMalloc of the arena failed"); return ORB_E_HIP; }
    int rc = db->h_q.reserve((size_t)E * sizeof(uint4));
    if (rc == ORB_OK) rc = db->d_move.reserve(E);
    if (rc != ORB_OK) { (void)hipFree(nid); (void)hipFree(nval); return rc; }
    uint4* mv = (uint4*)db->h_q.p;
    uint32_t off = 0;
    for (int e = 0; e < E; ++e) { mv[e] = make_uint4(db->entries[e].off, off, db->entries[e].len, 0); off += db->entries[e].len; }
    hipError_t err = hipMemcpyAsync(db->d_move.p, mv, (size_t)E * sizeof(uint4), hipMemcpyHostToDevice, db->stream);
    if (err == hipSuccess) {
        hipLaunchKernelGGL(k_db_compact, dim3(E), dim3(DB_BLOCK), 0, db->stream, db->d_id, db->d_val, nid, nval, db->d_move.p, E);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipStreamSynchronize(db->stream);
    if (err != hipSuccess) { (void)hipFree(nid); (void)hipFree(nval); morb::set_error("arena compaction failed: %s", hipGetErrorString(err)); return ORB_E_HIP; }
    (void)hipFree(db->d_id); (void)hipFree(db->d_val);
    db->d_id = nid; db->d_val = nval;
    for (int e = 0; e < E; ++e) db->entries[e].off = mv[e].y;
    db->used = off; db->dead = 0; db->table_dirty = true;
    return ORB_OK;
}

// Uploads the queries, runs k_db_query over `table` (n_entries rows on the device) and leaves the three output arrays in db->h_out:
// [score: Q*E doubles][common: Q*E int32][first_word: Q*E uint32].  Synchronises the stream.
int run_query(orbv_database* db, const uint2* d_table, int E, int Q, const uint32_t* const* id, const double* const* val, const int* n) {
    size_t total = 0; int nmax = 0;
    for (int q = 0; q < Q; ++q) { total += (size_t)n[q]; nmax = std::max(nmax, n[q]); }
    morb::BlockLayout L;
    const size_t o_off = L.take((size_t)(Q + 1) * sizeof(int)), o_val = L.take(total * sizeof(double)), o_id = L.take(total * sizeof(uint32_t));
    const size_t q_bytes = L.off;
    int rc = db->h_q.reserve(q_bytes); if (rc != ORB_OK) return rc;
    rc = db->d_q.reserve(q_bytes); if (rc != ORB_OK) return rc;
    int* h_off = (int*)(db->h_q.p + o_off);
    size_t acc = 0;
    for (int q = 0; q < Q; ++q) {
        h_off[q] = (int)acc;
        if (n[q]) {
            memcpy(db->h_q.p + o_val + acc * sizeof(double), val[q], (size_t)n[q] * sizeof(double));
            memcpy(db->h_q.p + o_id + acc * sizeof(uint32_t), id[q], (size_t)n[q] * sizeof(uint32_t));
        }
        acc += (size_t)n[q];
    }
    h_off[Q] = (int)acc;
    const size_t QE = (size_t)Q * E, out_bytes = QE * 16;
    rc = db->d_out.reserve(out_bytes); if (rc != ORB_OK) return rc;
    rc = db->h_out.reserve(out_bytes); if (rc != ORB_OK) return rc;
    MORB_HIP(hipMemcpyAsync(db->d_q.p, db->h_q.p, q_bytes, hipMemcpyHostToDevice, db->stream));
    double* o_score = (double*)db->d_out.p;
    int32_t* o_common = (int32_t*)(db->d_out.p + QE * 8);
    uint32_t* o_first = (uint32_t*)(db->d_out.p + QE * 12);
    // enough workgroups to cover the chip a few times over, but not one LDS fill of the query per four entries
    const int epb = (int)std::min<size_t>(64, std::max<size_t>(4, QE / 1024));
    const dim3 grid((unsigned)((E + epb - 1) / epb), (unsigned)Q);
    const uint32_t* dq_id = (const uint32_t*)(db->d_q.p + o_id);
    const double* dq_val = (const double*)(db->d_q.p + o_val);
    const int* dq_off = (const int*)(db->d_q.p + o_off);
    db->last_query[0] = nmax <= DB_LDS_WORDS ? ORBV_DB_FORM_LDS : ORBV_DB_FORM_GLOBAL; db->last_query[1] = epb;   // (host bookkeeping, no kernel reads it)
    db->last_query[2] = (int)grid.x; db->last_query[3] = Q;
    if (nmax <= DB_LDS_WORDS)
        hipLaunchKernelGGL(k_db_query<true>, grid, dim3(DB_BLOCK), (size_t)nmax * 12, db->stream, db->d_id, db->d_val, d_table, E, epb, dq_id, dq_val,
                           dq_off, nmax, o_score, o_common, o_first);
    else
        hipLaunchKernelGGL(k_db_query<false>, grid, dim3(DB_BLOCK), 0, db->stream, db->d_id, db->d_val, d_table, E, epb, dq_id, dq_val, dq_off, 0,
                           o_score, o_common, o_first);
    MORB_HIP(hipGetLastError());
    MORB_HIP(hipMemcpyAsync(db->h_out.p, db->d_out.p, out_bytes, hipMemcpyDeviceToHost, db->stream));
    MORB_HIP(hipStreamSynchronize(db->stream));
    return ORB_OK;
}

}  // namespace

extern "C" {

int orbv_db_create(int n_words, int device, orbv_database** out) {
    MORB_ARG(out != nullptr && n_words >= 1);
    int rc = morb::select_device(device);
    if (rc != ORB_OK) return rc;
    orbv_database* db = new orbv_database();
    db->device = device; db->n_words = n_words;
    hipError_t e = hipStreamCreateWithFlags(&db->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { morb::set_error("hipStreamCreate: %s", hipGetErrorString(e)); delete db; return ORB_E_HIP; }
    *out = db;
    return ORB_OK;
}

void orbv_db_destroy(orbv_database* db) {
    if (!db) return;
    (void)hipSetDevice(db->device);
    if (db->stream) { (void)hipStreamSynchronize(db->stream); (void)hipStreamDestroy(db->stream); }
    if (db->d_id) (void)hipFree(db->d_id);
    if (db->d_val) (void)hipFree(db->d_val);
    db->d_table.release(); db->d_list.release(); db->d_move.release(); db->d_q.release(); db->d_out.release();
    db->h_q.release(); db->h_out.release();
    delete db;
}

int orbv_db_add(orbv_database* db, uint64_t key, const uint32_t* id, const double* val, int n) {
    MORB_ARG(db != nullptr);
    int rc = check_bow(db, id, val, n);
    if (rc != ORB_OK) return rc;
    if (db->seq_of.count(key)) { morb::set_error("orbv_db_add: key %llu is already in the database", (unsigned long long)key); return ORB_E_ARG; }
    MORB_HIP(hipSetDevice(db->device));
    rc = grow(db, db->used + (size_t)n);
    if (rc != ORB_OK) return rc;
    if (n) {
        // through the pinned staging block: the caller's arrays are free again on return
        rc = db->h_q.reserve((size_t)n * 12 + 16); if (rc != ORB_OK) return rc;
        memcpy(db->h_q.p, val, (size_t)n * sizeof(double));
        memcpy(db->h_q.p + (size_t)n * 8, id, (size_t)n * sizeof(uint32_t));
        MORB_HIP(hipMemcpyAsync(db->d_val + db->used, db->h_q.p, (size_t)n * sizeof(double), hipMemcpyHostToDevice, db->stream));
        MORB_HIP(hipMemcpyAsync(db->d_id + db->used, db->h_q.p + (size_t)n * 8, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, db->stream));
        MORB_HIP(hipStreamSynchronize(db->stream));
    }
    db->entries.push_back(Entry{key, db->next_seq, (uint32_t)db->used, (uint32_t)n});
    db->seq_of[key] = db->next_seq++;
    db->used += (size_t)n;
    db->table_dirty = true;
    return ORB_OK;
}

int orbv_db_erase(orbv_database* db, uint64_t key) {
    MORB_ARG(db != nullptr);
    auto it = db->seq_of.find(key);
    if (it == db->seq_of.end()) return ORB_OK;   // the reference's erase of a keyframe that is in no list changes nothing
    const int e = db->find(it->second);
    db->seq_of.erase(it);
    if (e < 0) return ORB_OK;
    db->dead += db->entries[e].len;
    db->entries.erase(db->entries.begin() + e);
    db->table_dirty = true;
    if (db->dead * 2 > db->used) {
        MORB_HIP(hipSetDevice(db->device));
        return compact(db);
    }
    return ORB_OK;
}

int orbv_db_clear(orbv_database* db) {
    MORB_ARG(db != nullptr);
    db->entries.clear(); db->seq_of.clear();
    db->used = db->dead = 0;
    db->table_dirty = true;
    return ORB_OK;
}

int orbv_db_count(const orbv_database* db) { return db ? (int)db->entries.size() : 0; }

int orbv_debug_last_db_query(const orbv_database* db, int* out4) {
    MORB_ARG(db != nullptr && out4 != nullptr);
    for (int i = 0; i < 4; ++i) out4[i] = db->last_query[i];
    return ORB_OK;
}

int orbv_db_query(orbv_database* db, int n_queries, const uint32_t* const* id, const double* const* val, const int* n, int capacity,
                  uint64_t* key, int32_t* common, double* score, int* n_hits) {
    MORB_ARG(db != nullptr && n_queries >= 0 && n_queries <= DB_MAX_QUERIES && capacity >= 0 && (n_queries == 0 || (id && val && n && n_hits)));
    MORB_ARG((size_t)n_queries * db->entries.size() * 16 <= DB_MAX_OUT_BYTES);
    MORB_ARG(n_queries == 0 || capacity == 0 || (key && common && score));
    for (int q = 0; q < n_queries; ++q) { int rc = check_bow(db, id[q], val[q], n[q]); if (rc != ORB_OK) return rc; }
    const int E = (int)db->entries.size();
    for (int q = 0; q < n_queries; ++q) n_hits[q] = 0;
    if (n_queries == 0 || E == 0) return ORB_OK;
    MORB_HIP(hipSetDevice(db->device));
    int rc;
    if (db->table_dirty) {
        rc = db->d_table.reserve(E); if (rc != ORB_OK) return rc;
        rc = db->h_q.reserve((size_t)E * sizeof(uint2)); if (rc != ORB_OK) return rc;
        uint2* t = (uint2*)db->h_q.p;
        for (int e = 0; e < E; ++e) t[e] = make_uint2(db->entries[e].off, db->entries[e].len);
        MORB_HIP(hipMemcpyAsync(db->d_table.p, t, (size_t)E * sizeof(uint2), hipMemcpyHostToDevice, db->stream));
        MORB_HIP(hipStreamSynchronize(db->stream));   // the staging block is reused for the queries
        db->table_dirty = false;
    }
    rc = run_query(db, db->d_table.p, E, n_queries, id, val, n);
    if (rc != ORB_OK) return rc;
    const size_t QE = (size_t)n_queries * E;
    const double* h_score = (const double*)db->h_out.p;
    const int32_t* h_common = (const int32_t*)(db->h_out.p + QE * 8);
    const uint32_t* h_first = (const uint32_t*)(db->h_out.p + QE * 12);
    // lKFsSharingWords order: a keyframe is first met at its smallest shared word; among those first met at the same word the earlier
    // add comes first (the lists keep insertion order).  entries[] is in add order, so a stable sort by first word is the whole of it.
    std::vector<int> hits;
    for (int q = 0; q < n_queries; ++q) {
        const size_t b = (size_t)q * E;
        hits.clear();
        for (int e = 0; e < E; ++e) if (h_common[b + e] > 0) hits.push_back(e);
        if ((int)hits.size() > capacity) {
            morb::set_error("orbv_db_query: query %d shares words with %d entries, capacity is %d", q, (int)hits.size(), capacity);
            return ORB_E_ARG;
        }
        std::stable_sort(hits.begin(), hits.end(), [&](int a, int c) { return h_first[b + a] < h_first[b + c]; });
        for (size_t k = 0; k < hits.size(); ++k) {
            const size_t o = (size_t)q * capacity + k;
            key[o] = db->entries[hits[k]].key; common[o] = h_common[b + hits[k]]; score[o] = h_score[b + hits[k]];
        }
        n_hits[q] = (int)hits.size();
    }
    return ORB_OK;
}

int orbv_db_score(orbv_database* db, const uint32_t* id, const double* val, int n, const uint64_t* keys, int n_keys, double* score) {
    MORB_ARG(db != nullptr && n_keys >= 0 && (size_t)n_keys * 16 <= DB_MAX_OUT_BYTES && (n_keys == 0 || (keys && score)));
    int rc = check_bow(db, id, val, n);
    if (rc != ORB_OK) return rc;
    if (n_keys == 0) return ORB_OK;
    std::vector<uint2> list(n_keys);
    for (int k = 0; k < n_keys; ++k) {
        auto it = db->seq_of.find(keys[k]);
        const int e = it == db->seq_of.end() ? -1 : db->find(it->second);
        if (e < 0) { morb::set_error("orbv_db_score: key %llu is not in the database", (unsigned long long)keys[k]); return ORB_E_ARG; }
        list[k] = make_uint2(db->entries[e].off, db->entries[e].len);
    }
    MORB_HIP(hipSetDevice(db->device));
    rc = db->d_list.reserve(n_keys); if (rc != ORB_OK) return rc;
    MORB_HIP(hipMemcpyAsync(db->d_list.p, list.data(), (size_t)n_keys * sizeof(uint2), hipMemcpyHostToDevice, db->stream));
    MORB_HIP(hipStreamSynchronize(db->stream));
    rc = run_query(db, db->d_list.p, n_keys, 1, &id, &val, &n);
    if (rc != ORB_OK) return rc;
    memcpy(score, db->h_out.p, (size_t)n_keys * sizeof(double));
    return ORB_OK;
}

}  // extern "C"
