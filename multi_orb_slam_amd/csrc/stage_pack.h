// stage_pack.h -- how the batched entry points lay out and stage the arrays of one call: one block, every array 16-byte aligned, in the
// order the arrays are added.  The one definition of the round-up (align16), of the running layout (BlockLayout: bow.hip's keyframe block,
// kfdb.hip's query block), of the staging sequence (StagePack: mappoint.hip, pose.hip, sim3.hip, sim3opt.hip, pnp.hip, triangulate.hip)
// and of the checks on a call's CSR (validate_first: mappoint.hip; validate_csr: pose.hip, sim3opt.hip, ransac_dev.h).
#pragma once
#include <string.h>
#include "orb_common.h"

namespace morb {

inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

struct BlockLayout {   // offsets of consecutive 16-byte aligned arrays; `off` = the bytes of the block so far
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off = align16(off + bytes); return o; }
};

// What every CSR of a batched call must satisfy: first[0] == 0, first[] not decreasing over its B entries.  noun: what an entry is in
// the caller's words ("problem", "point").  validate_csr: a batch of problems, 1..max_batch of them.
inline int validate_first(int B, const int32_t* first, const char* noun) {
    MORB_ARG(first[0] == 0);
    for (int b = 0; b < B; ++b)
        if (first[b + 1] < first[b]) { set_error("first[] decreases at %s %d", noun, b); return ORB_E_ARG; }
    return ORB_OK;
}
inline int validate_csr(int B, int max_batch, const int32_t* first) {
    if (B < 1 || B > max_batch) { set_error("B = %d is outside 1..%d", B, max_batch); return ORB_E_ARG; }
    return validate_first(B, first, "problem");
}

// An array is named once where it is added -- with where its bytes come from -- and once more where its typed pointer is taken:
//     StagePack pk;
//     const int i_first = pk.add(first, (size_t)(B + 1) * 4);     // copied from the caller's array
//     const int i_pos = pk.add_or_zeros(in->pos, (size_t)P * 12); // an optional array: zeros when the caller has none
//     const int i_cams = pk.add_in_place((size_t)N * 4);          // written by the caller through Block::host
//     const StagePack::Block blk = pk.open(m->stage, &rc);        // reserve, then every copy and zero fill
//     if (rc) return rc;
//     int32_t* cams = blk.host<int32_t>(i_cams); ...
//     blk.publish();
//     A.first = blk.dev<int32_t>(i_first);
// Pointers come from a Block alone, and open() alone makes one, after the reserve: no pointer is taken before a reallocation.  A
// required array that is NULL with bytes to copy is an error of open(), not a block of stale bytes.  Nothing is allocated per call
// (MAX_ARRAYS entries on the stack).
class StagePack {
public:
    static constexpr int MAX_ARRAYS = 24;

    int add(const void* src, size_t bytes) { if (!src && bytes) missing = true; return push(src, bytes, false); }
    int add_or_zeros(const void* src, size_t bytes) { return push(src, bytes, src == nullptr); }
    int add_in_place(size_t bytes) { return push(nullptr, bytes, false); }
    size_t bytes() const { return layout.off; }

    class Block {   // refers to the StagePack that made it and must not outlive it; after a failed open() it holds no block: return on rc
    public:
        template <typename T> T* host(int id) const { return (T*)(h + pack->entry[id].off); }
        template <typename T> const T* dev(int id) const { return (const T*)(d + pack->entry[id].off); }
        // after the host's last write, before the launch (a StageBuf in HBM: the write-combined stores become visible)
        void publish() const { if (stage) stage->publish(); }
    private:
        friend class StagePack;
        Block() {}
        const StagePack* pack = nullptr;
        const StageBuf* stage = nullptr;
        uint8_t* h = nullptr;
        const uint8_t* d = nullptr;
    };

    // host-written, device-read in place
    Block open(StageBuf& buf, int* rc) const {
        Block b;
        if ((*rc = check()) || (*rc = buf.reserve(layout.off))) return b;
        b.stage = &buf;
        fill(buf.p, buf.dp, &b);
        return b;
    }
    // a pinned block and its device mirror: the caller copies bytes() from h.p to d.p on its stream
    Block open(PinnedBuf<uint8_t>& h, DevBuf<uint8_t>& d, int* rc) const {
        Block b;
        if ((*rc = check()) || (*rc = h.reserve(layout.off)) || (*rc = d.reserve(layout.off))) return b;
        fill(h.p, d.p, &b);
        return b;
    }

private:
    struct Entry { size_t off, bytes; const void* src; bool zeros; };
    Entry entry[MAX_ARRAYS];
    int count = 0;
    bool overflow = false, missing = false;
    BlockLayout layout;

    int push(const void* src, size_t bytes, bool zeros) {
        if (count == MAX_ARRAYS) { overflow = true; return 0; }
        entry[count] = {layout.take(bytes), bytes, src, zeros};
        return count++;
    }
    int check() const {
        if (overflow) { set_error("more than %d arrays in one staged block", (int)MAX_ARRAYS); return ORB_E_CAPACITY; }
        if (missing) { set_error("an array to stage is NULL"); return ORB_E_ARG; }
        return ORB_OK;
    }
    void fill(uint8_t* hbase, const uint8_t* dbase, Block* out) const {
        out->pack = this; out->h = hbase; out->d = dbase;
        for (int k = 0; k < count; ++k) {
            const Entry& e = entry[k];
            if (!e.bytes) continue;
            if (e.zeros) memset(hbase + e.off, 0, e.bytes);
            else if (e.src) memcpy(hbase + e.off, e.src, e.bytes);
        }
    }
};

}  // namespace morb
