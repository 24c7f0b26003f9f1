// test_kfdb.cc -- driver of KeyFrameDatabase for tests/test_kfdb_model.py, tests/test_gpu_kfdb.py and tools/kfdb_bench.py.
//
//   test_kfdb run     WORLD.bin OUT.bin   the script through ORB_SLAM2::KeyFrameDatabase (the databases live on the device)
//   test_kfdb cpu     WORLD.bin OUT.bin   the same script through HostDatabase below: the reference's algorithm on the host, inverted files
//                                         as lists and ORBVocabulary::score -- a third implementation beside the class and the Python model,
//                                         and the comparison leg of the benchmark.  Needs no device.
//   test_kfdb threads WORLD.bin OUT.bin   one thread performs the script's add_cam1 operations while another asks for relocalisation
//                                         candidates in a loop (the reloc operations with minScore < 0); after the join the rest of the script runs as in `run`
//   test_kfdb time    WORLD.bin SECONDS   both databases are filled once by the script's add operations; then, five times in turn, the script's
//                                         reloc operations run for SECONDS through the host restatement and for SECONDS through the class (a fresh
//                                         frame id per call); prints one JSON line per leg: calls, microseconds per call
//
// WORLD.bin (little endian): int32 magic, n_words, n_keyframes, n_ops; per keyframe: uint64 id, int32 n, n1, ncov, ncov1, nconn, nconn1,
// uint32 id[n], double val[n], uint32 id1[n1], double val1[n1], then the four lists as int32 keyframe indices (covisibility ordered best
// first, all cameras / camera 1; connected set, all cameras / camera 1); per operation: int32 code (add, add_cam1, erase, clear, loop,
// loop_cam1, reloc), int32 keyframe index, uint64 frame id (reloc), float minScore (loop).
// OUT.bin: per detect call int32 n, uint64 id[n] (the returned keyframes in order), then per keyframe of the world
// uint64 mnLoopQuery, int32 mnLoopWords, float mLoopScore, uint64 mnRelocQuery, int32 mnRelocWords, float mRelocScore.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>
#include <memory>
#include <string>
#include <thread>
#include <vector>
#include "KeyFrameDatabase.h"

using namespace ORB_SLAM2;

namespace {

enum { OP_ADD, OP_ADD_CAM1, OP_ERASE, OP_CLEAR, OP_LOOP, OP_LOOP_CAM1, OP_RELOC };
struct Op { int32_t code, kf; uint64_t frame; float min_score; };

struct World {
    int n_words = 0;
    std::vector<std::unique_ptr<KeyFrame>> kfs;
    std::vector<Op> ops;
};

bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

bool load(const char* path, World& w) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return false; }
    int32_t hdr[4];
    if (!rd(f, hdr, sizeof hdr) || hdr[0] != 0x4B464442 || hdr[1] < 1 || hdr[2] < 0 || hdr[3] < 0) { fprintf(stderr, "bad header\n"); fclose(f); return false; }
    w.n_words = hdr[1];
    const int K = hdr[2];
    std::vector<std::vector<int32_t>> lists((size_t)K * 4);
    for (int k = 0; k < K; ++k) {
        uint64_t id; int32_t n[6];
        if (!rd(f, &id, 8) || !rd(f, n, sizeof n)) { fclose(f); return false; }
        for (int j = 0; j < 6; ++j) if (n[j] < 0 || n[j] > (1 << 20)) { fclose(f); return false; }
        std::unique_ptr<KeyFrame> kf(new KeyFrame());
        kf->mnId = id;
        for (int c = 0; c < 2; ++c) {
            std::vector<uint32_t> ids(n[c]); std::vector<double> vals(n[c]);
            if (!rd(f, ids.data(), (size_t)n[c] * 4) || !rd(f, vals.data(), (size_t)n[c] * 8)) { fclose(f); return false; }
            DBoW2::BowVector& v = c ? kf->mBowVec_cam1 : kf->mBowVec;
            for (int i = 0; i < n[c]; ++i) v.insert(v.end(), std::make_pair(ids[i], vals[i]));
        }
        for (int j = 0; j < 4; ++j) {
            lists[(size_t)k * 4 + j].resize(n[2 + j]);
            if (!rd(f, lists[(size_t)k * 4 + j].data(), (size_t)n[2 + j] * 4)) { fclose(f); return false; }
        }
        w.kfs.push_back(std::move(kf));
    }
    for (int k = 0; k < K; ++k)
        for (int j = 0; j < 4; ++j)
            for (int32_t i : lists[(size_t)k * 4 + j]) {
                if (i < 0 || i >= K) { fclose(f); return false; }
                KeyFrame* o = w.kfs[i].get(); KeyFrame* kf = w.kfs[k].get();
                if (j == 0) kf->mvpOrderedConnectedKeyFrames.push_back(o);
                else if (j == 1) kf->mvpOrderedConnectedKeyFrames_cam1.push_back(o);
                else if (j == 2) kf->mConnectedKeyFrames.insert(o);
                else kf->mConnectedKeyFrames_cam1.insert(o);
            }
    w.ops.resize(hdr[3]);
    for (Op& o : w.ops) {
        if (!rd(f, &o.code, 4) || !rd(f, &o.kf, 4) || !rd(f, &o.frame, 8) || !rd(f, &o.min_score, 4)) { fclose(f); return false; }
        if (o.code < 0 || o.code > OP_RELOC || o.kf < 0 || o.kf >= K) { fclose(f); return false; }
    }
    fclose(f);
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The reference's algorithm on the host (src/KeyFrameDatabase.cc), restated: one list of keyframes per word and file, the walk over the
// query's words that marks, counts and lists, the common-word threshold, the scores, the covisibility groups, the retained best.
// Loop detection and relocalisation differ in the scratch fields they use and in four places, named in Kind.
struct Kind {
    long unsigned int KeyFrame::*query; int KeyFrame::*words; float KeyFrame::*score;
    bool skip_connected;    // loop: keyframes connected to the query are counted but neither marked nor listed (:146)
    bool filter_min_score;  // loop: only scores >= minScore become matches (:190); relocalisation keeps all (:479)
    bool group_needs_words; // loop: a neighbour counts when marked AND above the word threshold (:216); relocalisation: marked (:505)
};
const Kind LOOP = {&KeyFrame::mnLoopQuery, &KeyFrame::mnLoopWords, &KeyFrame::mLoopScore, true, true, true};
const Kind RELOC = {&KeyFrame::mnRelocQuery, &KeyFrame::mnRelocWords, &KeyFrame::mRelocScore, false, false, false};

class HostDatabase {
public:
    HostDatabase(const ORBVocabulary& voc, int n_words) : voc_(&voc), file_(n_words), file1_(n_words) {}
    void add(KeyFrame* kf) { for (const auto& e : kf->mBowVec) file_[e.first].push_back(kf); }
    void add_cam1(KeyFrame* kf) { for (const auto& e : kf->mBowVec_cam1) file1_[e.first].push_back(kf); }
    void erase(KeyFrame* kf) {
        drop(file_, kf->mBowVec, kf);
        drop(file1_, kf->mBowVec_cam1, kf);
    }
    void clear() { const size_t n = file_.size(); file_.assign(n, {}); file1_.assign(n, {}); }
    std::vector<KeyFrame*> loop(KeyFrame* q, float min_score, bool cam1) {
        const std::set<KeyFrame*> connected = cam1 ? q->GetConnectedKeyFrames_cam1() : q->GetConnectedKeyFrames();
        return detect(LOOP, cam1, q->mnId, cam1 ? q->mBowVec_cam1 : q->mBowVec, connected, min_score, min_score);
    }
    std::vector<KeyFrame*> reloc(Frame* f) { return detect(RELOC, true, f->mnId, f->mBowVec_cam1, {}, 0.f, 0.f); }

private:
    typedef std::vector<std::list<KeyFrame*>> File;
    static void drop(File& file, const DBoW2::BowVector& v, KeyFrame* kf) {
        for (const auto& e : v) {
            std::list<KeyFrame*>& l = file[e.first];
            for (auto it = l.begin(); it != l.end(); ++it)
                if (*it == kf) { l.erase(it); break; }
        }
    }
    std::vector<KeyFrame*> detect(const Kind& kind, bool cam1, long unsigned int qid, const DBoW2::BowVector& qv, const std::set<KeyFrame*>& connected,
                                  float min_score, float best_acc_start) {
        File& file = cam1 ? file1_ : file_;
        std::list<KeyFrame*> sharing;
        for (const auto& e : qv)
            for (KeyFrame* k : file[e.first]) {
                if (k->*kind.query != qid) {
                    k->*kind.words = 0;
                    if (!kind.skip_connected || !connected.count(k)) { k->*kind.query = qid; sharing.push_back(k); }
                }
                (k->*kind.words)++;
            }
        if (sharing.empty()) return {};
        int max_common = 0;
        for (KeyFrame* k : sharing) if (k->*kind.words > max_common) max_common = k->*kind.words;
        const int min_common = max_common * 0.8f;
        std::list<std::pair<float, KeyFrame*>> matches;
        for (KeyFrame* k : sharing)
            if (k->*kind.words > min_common) {
                const float si = voc_->score(qv, cam1 ? k->mBowVec_cam1 : k->mBowVec);
                k->*kind.score = si;
                if (!kind.filter_min_score || si >= min_score) matches.push_back({si, k});
            }
        if (matches.empty()) return {};
        std::list<std::pair<float, KeyFrame*>> groups;
        float best_acc = best_acc_start;
        for (const auto& mt : matches) {
            const std::vector<KeyFrame*> neigh = cam1 ? mt.second->GetBestCovisibilityKeyFrames_cam1(10) : mt.second->GetBestCovisibilityKeyFrames(10);
            float best = mt.first, acc = mt.first;
            KeyFrame* best_kf = mt.second;
            for (KeyFrame* k2 : neigh) {
                if (k2->*kind.query != qid) continue;
                if (kind.group_needs_words && !(k2->*kind.words > min_common)) continue;
                acc += k2->*kind.score;
                if (k2->*kind.score > best) { best_kf = k2; best = k2->*kind.score; }
            }
            groups.push_back({acc, best_kf});
            if (acc > best_acc) best_acc = acc;
        }
        const float retain = 0.75f * best_acc;
        std::set<KeyFrame*> seen;
        std::vector<KeyFrame*> out;
        for (const auto& g : groups)
            if (g.first > retain && !seen.count(g.second)) { out.push_back(g.second); seen.insert(g.second); }
        return out;
    }
    const ORBVocabulary* voc_;
    File file_, file1_;
};

// ---------------------------------------------------------------------------------------------------------------------------------
void write_call(FILE* f, const World& w, const std::vector<KeyFrame*>& ret) {
    const int32_t n = (int32_t)ret.size();
    fwrite(&n, 4, 1, f);
    for (KeyFrame* k : ret) { const uint64_t id = k->mnId; fwrite(&id, 8, 1, f); }
    for (const auto& k : w.kfs) {
        const uint64_t lq = k->mnLoopQuery, rq = k->mnRelocQuery;
        const int32_t lw = k->mnLoopWords, rw = k->mnRelocWords;
        fwrite(&lq, 8, 1, f); fwrite(&lw, 4, 1, f); fwrite(&k->mLoopScore, 4, 1, f);
        fwrite(&rq, 8, 1, f); fwrite(&rw, 4, 1, f); fwrite(&k->mRelocScore, 4, 1, f);
    }
}

template <class DB, class LoopFn, class RelocFn>
void play(World& w, DB& db, LoopFn loop, RelocFn reloc, size_t first, FILE* out) {
    for (size_t i = first; i < w.ops.size(); ++i) {
        const Op& o = w.ops[i];
        KeyFrame* kf = w.kfs[o.kf].get();
        if (o.code == OP_ADD) db.add(kf);
        else if (o.code == OP_ADD_CAM1) db.add_cam1(kf);
        else if (o.code == OP_ERASE) db.erase(kf);
        else if (o.code == OP_CLEAR) db.clear();
        else {
            Frame fr;
            fr.mnId = o.frame; fr.mBowVec_cam1 = kf->mBowVec_cam1;
            const std::vector<KeyFrame*> ret = o.code == OP_RELOC ? reloc(&fr) : loop(kf, o.min_score, o.code == OP_LOOP_CAM1);
            write_call(out, w, ret);
        }
    }
}

// a vocabulary whose size() is n_words: the root and n_words leaves (the database reads nothing else of it)
bool flat_vocabulary(ORBVocabulary& voc, int n_words) {
    const int n = n_words + 1;
    std::vector<int> parent(n, 0);
    std::vector<unsigned char> leaf(n, 1), desc((size_t)n * 32, 0);
    std::vector<double> weight(n, 1.0);
    leaf[0] = 0;
    return voc.create(n, 1, parent.data(), leaf.data(), desc.data(), weight.data());
}

// the comparison legs of tools/kfdb_bench.py: same world, same process, alternated
int time_legs(World& w, double seconds) {
    ORBVocabulary voc;
    if (!flat_vocabulary(voc, w.n_words)) { fprintf(stderr, "time: the device is needed for this mode\n"); return 3; }
    HostDatabase host(voc, w.n_words);
    KeyFrameDatabase dev(voc);
    std::vector<const Op*> asks;
    for (const Op& o : w.ops) {
        KeyFrame* kf = w.kfs[o.kf].get();
        if (o.code == OP_ADD) { host.add(kf); dev.add(kf); }
        else if (o.code == OP_ADD_CAM1) { host.add_cam1(kf); dev.add_cam1(kf); }
        else if (o.code == OP_RELOC) asks.push_back(&o);
    }
    if (asks.empty()) { fprintf(stderr, "time: the script holds no reloc operation\n"); return 2; }
    uint64_t frame_id = 1;
    size_t checksum[2] = {0, 0};
    for (int round = 0; round < 5; ++round)
        for (int leg = 0; leg < 2; ++leg) {
            long calls = 0;
            const auto t0 = std::chrono::steady_clock::now();
            double us = 0;
            do {
                for (const Op* o : asks) {
                    Frame fr;
                    fr.mnId = frame_id++; fr.mBowVec_cam1 = w.kfs[o->kf]->mBowVec_cam1;
                    const auto c0 = std::chrono::steady_clock::now();
                    const std::vector<KeyFrame*> ret = leg == 0 ? host.reloc(&fr) : dev.DetectRelocalizationCandidates(&fr);
                    us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - c0).count();
                    if (round == 0 && calls < (long)asks.size()) for (KeyFrame* k : ret) checksum[leg] += k->mnId + 1;   // first pass of each leg
                    ++calls;
                }
            } while (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < seconds);
            printf("{\"leg\": \"%s\", \"round\": %d, \"calls\": %ld, \"us_per_call\": %.3f}\n", leg == 0 ? "host" : "class", round, calls, us / calls);
            fflush(stdout);
        }
    // same frames, same answers: the candidates of each leg's first pass, summed
    fprintf(stderr, "time: checksums host %zu class %zu\n", checksum[0], checksum[1]);
    if (checksum[0] != checksum[1]) { fprintf(stderr, "time: the two legs returned different candidates\n"); return 4; }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: test_kfdb run|cpu|threads WORLD.bin OUT.bin | time WORLD.bin SECONDS\n"); return 2; }
    const std::string mode = argv[1];
    World w;
    if (!load(argv[2], w)) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    if (mode == "time") return time_legs(w, atof(argv[3]));
    FILE* out = fopen(argv[3], "wb");
    if (!out) { fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
    ORBVocabulary voc;
    if (mode == "cpu") {
        HostDatabase db(voc, w.n_words);
        play(w, db, [&](KeyFrame* k, float s, bool c1) { return db.loop(k, s, c1); }, [&](Frame* f) { return db.reloc(f); }, 0, out);
    } else if (mode == "run" || mode == "threads") {
        if (!flat_vocabulary(voc, w.n_words)) { fprintf(stderr, "%s: the device is needed for this mode\n", mode.c_str()); return 3; }
        {
            KeyFrameDatabase db(voc);
            size_t first = 0;
            if (mode == "threads") {
                // the leading add_cam1 operations on one thread, relocalisation queries on another, through the class mutex
                size_t n_add = 0, n_pool = 0;
                while (n_add < w.ops.size() && w.ops[n_add].code == OP_ADD_CAM1) ++n_add;
                // the relocalisation operations with minScore < 0 that follow are the asking thread's pool (cycled, a fresh frame id each time)
                while (n_add + n_pool < w.ops.size() && w.ops[n_add + n_pool].code == OP_RELOC && w.ops[n_add + n_pool].min_score < 0) ++n_pool;
                if (!n_add || !n_pool) { fprintf(stderr, "threads: the script must start with add_cam1 operations and a pool of queries\n"); return 2; }
                std::atomic<bool> done{false};
                std::atomic<int> asked{0};
                std::thread adder([&] { for (size_t i = 0; i < n_add; ++i) db.add_cam1(w.kfs[w.ops[i].kf].get()); done = true; });
                std::thread asker([&] {
                    uint64_t id = 1;
                    while (!done || asked < 3) {
                        Frame fr;
                        fr.mnId = id++; fr.mBowVec_cam1 = w.kfs[w.ops[n_add + (size_t)asked % n_pool].kf]->mBowVec_cam1;
                        (void)db.DetectRelocalizationCandidates(&fr);
                        ++asked;
                    }
                });
                adder.join(); asker.join();
                fprintf(stderr, "threads: %zu adds, %d queries meanwhile\n", n_add, asked.load());
                n_add += n_pool;
                first = n_add;
            }
            play(w, db, [&](KeyFrame* k, float s, bool c1) { return c1 ? db.DetectLoopCandidates_cam1(k, s) : db.DetectLoopCandidates(k, s); },
                 [&](Frame* f) { return db.DetectRelocalizationCandidates(f); }, first, out);
        }
    } else {
        fprintf(stderr, "unknown mode %s\n", mode.c_str());
        return 2;
    }
    if (out) fclose(out);
    return 0;
}
