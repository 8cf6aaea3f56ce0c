// lfx_merge_tree.h — block_merge (include/lfx.h): the fixed binary tree over one region of candidates.  ONE code
// path for the HIP kernel (block_merge_kernel: all lanes of the workgroup, workgroup barriers) and for the host test
// (tests/c/block_merge.cpp: lane 0 of 1, barriers are no-ops), as lfx_huff.h — whose huff_block_build gives every D: there is
// no second size estimate, the contract is exact.
#pragma once
#include "lfx_huff.h"
#include "lfx_merge.h"

namespace lfx {

// what merge_tree works on (LDS on the device)
struct MergeScratch {
    uint32_t rows[MERGE_MAX * SYM_ROW];   // in: the candidates' symbol counts; a whole node's sum lives in its first candidate's row
    uint32_t sum[SYM_ROW];                // the node under evaluation
    uint64_t D[MERGE_MAX];                // in: every candidate's exact dynamic size; D[s]: that of the whole node starting at s
    uint64_t node_D;
    uint32_t head[MERGE_MAX];             // out: the first candidate of the group candidate i ends up in
    uint32_t whole[MERGE_MAX];            // whole[s]: the largest node built so far that starts at candidate s is whole
};

// The tree over the n candidates of one region (include/lfx.h): levels bottom-up; the node at level l that starts at candidate
// s has its right child at s + 2^(l-1) — empty: the node is its left child, nothing changes — and is whole when both children
// are and one block over their summed counts (one EndOfBlock) is no longer than the two.  The sum is committed in place only
// for a whole node; a node that is not whole keeps every ancestor from being whole, so its subtree is finished.
// All lanes of the workgroup call it.  `out` takes the codes of every node evaluated (a scratch slot: the caller rebuilds the
// heads' codes afterwards); S is huff_block_build's scratch.
LFX_HD inline void merge_tree(MergeScratch &M, uint32_t n, BlockCodes *out, HuffScratch &S, int lane, int nlanes) {
    for (uint32_t i = (uint32_t)lane; i < n; i += (uint32_t)nlanes) { M.head[i] = i; M.whole[i] = 1; }
    LFX_SYNC();
    for (uint32_t l = 1; l <= MERGE_LEVELS; l++) {
        const uint32_t span = 1u << l, half = span >> 1;
        for (uint32_t s = 0; s + half < n; s += span) {          // (s + half >= n: an empty right child)
            const uint32_t mid = s + half, end = s + span < n ? s + span : n;
            bool ok = M.whole[s] != 0 && M.whole[mid] != 0;      // (uniform: read behind a barrier)
            if (ok) {
                for (uint32_t i = (uint32_t)lane; i < SYM_ROW; i += (uint32_t)nlanes)
                    M.sum[i] = i == 256 ? 1u : M.rows[s * SYM_ROW + i] + M.rows[mid * SYM_ROW + i];
                LFX_SYNC();
                huff_block_build(M.sum, BT_DYNAMIC, out, S, lane, nlanes);
                if (lane == 0) M.node_D = out->body_bits;        // (lane 0 wrote it)
                LFX_SYNC();
                ok = M.node_D <= M.D[s] + M.D[mid];
                LFX_SYNC();                                      // (every lane has read D[s] and node_D)
                if (ok) {
                    for (uint32_t i = (uint32_t)lane; i < SYM_ROW; i += (uint32_t)nlanes) M.rows[s * SYM_ROW + i] = M.sum[i];
                    for (uint32_t i = mid + (uint32_t)lane; i < end; i += (uint32_t)nlanes) M.head[i] = s;
                    if (lane == 0) M.D[s] = M.node_D;
                }
            }
            if (!ok && lane == 0) M.whole[s] = 0;
            LFX_SYNC();
        }
    }
}

}  // namespace lfx
