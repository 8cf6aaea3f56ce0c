// lfx_merge.h — block_merge (include/lfx.h): which blocks of a plan may be joined.  merge_regions lays out the
// aligned LFX_MERGE_MAX-candidate regions of every run of a plan — pure index arithmetic, no HIP call, no context: compiles
// with a plain host compiler (tests/c/block_merge.cpp).  One workgroup of block_merge_kernel takes one region; a wrong region
// is a group across two streams.  (The decision over a region: merge_tree, lfx_merge_tree.h.)
#pragma once
#include <cstdint>
#include <vector>

#include "lfx_common.h"

namespace lfx {

constexpr uint32_t MERGE_MAX = 16;      // LFX_MERGE_MAX: candidates of one region, and so of one merged block
constexpr uint32_t MERGE_LEVELS = 4;    // log2(MERGE_MAX)

// `n` consecutive candidates (2..MERGE_MAX), the blocks first_block .. first_block + n - 1 of the plan
struct MergeRegion {
    uint32_t first_block;
    uint32_t n;
};

// The regions of a plan.  A run is a maximal sequence of consecutive BT_DYNAMIC blocks of one stream: it ends behind a block
// with BFINAL (the streams of a batch lie back to back in the merged plan, each closed by its final block) and in front of
// any block of another type (the zlib sync marker).  A run is cut into regions at every MERGE_MAX-th candidate; a region of one
// candidate has nothing to decide and is left out.
inline void merge_regions(const std::vector<BlockDesc> &blocks, std::vector<MergeRegion> &out) {
    out.clear();
    const size_t nb = blocks.size();
    for (size_t b = 0; b < nb;) {
        if (blocks[b].type != BT_DYNAMIC) { b++; continue; }
        size_t e = b;
        while (e < nb && blocks[e].type == BT_DYNAMIC) {
            e++;
            if (blocks[e - 1].final) break;
        }
        for (size_t r = b; r < e; r += MERGE_MAX) {
            const size_t n = e - r < MERGE_MAX ? e - r : MERGE_MAX;
            if (n >= 2) out.push_back(MergeRegion{(uint32_t)r, (uint32_t)n});
        }
        b = e;
    }
}

}  // namespace lfx
