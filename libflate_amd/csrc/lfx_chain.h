// lfx_chain.h — ChainLz77Encoder (LFX_LZ77_CHAIN): the work list of the chain refinement kernel (lfx_chain.hip)
// and the host arithmetic that makes it.  Pure index arithmetic on a chunk list — compiles with a plain host compiler
// (tests/c/chain_opts.cpp).  Internal.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "lfx_common.h"

namespace lfx {

// Positions per workgroup.  The window instance stages [p0 - W, p0 + CHAIN_TILE + M) of the bytes and [p0 - W, p0 + CHAIN_TILE) of
// the candidates in LDS: 49 KB + 96 KB at W = 32768.  The small instance serves calls whose chunks all fit one small tile (a batch
// of records): no window in front of position 0, 8.5 KB + 16 KB, six workgroups to a CU instead of one.
constexpr uint32_t CHAIN_TILE = 16384;
constexpr uint32_t CHAIN_TILE_SMALL = 8192;

// one workgroup of the chain kernel: positions [p0, p0 + tile) of a chunk
struct ChainItem {
    uint32_t chunk;
    uint32_t p0;
};

// every chunk that is parsed fits the small tile: the small instance serves the call
inline bool chain_small(const std::vector<ChunkDesc> &chunks) {
    for (const ChunkDesc &ch : chunks)
        if (!(ch.flags & CH_LITERALS) && ch.len > CHAIN_TILE_SMALL) return false;
    return true;
}
// The work list: the visited range [0, end) of every parsed chunk (default.rs:75), `tile` positions to an item — a grid sized
// by positions, as the dictionary candidate kernel's.
inline void chain_items(const std::vector<ChunkDesc> &chunks, uint32_t tile, std::vector<ChainItem> &items) {
    items.clear();
    for (uint32_t ci = 0; ci < (uint32_t)chunks.size(); ci++) {
        const ChunkDesc &ch = chunks[ci];
        if ((ch.flags & CH_LITERALS) || ch.len <= 3) continue;
        const uint64_t end = ch.len - 3;
        for (uint64_t p0 = 0; p0 < end; p0 += tile) items.push_back(ChainItem{ci, (uint32_t)p0});
    }
}

#ifdef __HIPCC__
// behind the match stage: cd2[p] ← the distance of the longest of the first `depth` candidates on p's chain through cd (ties: the
// nearest) for every listed position p < end with cd[p] != 0, and 0 where cd[p] == 0.  cd is only read.
int launch_chain(hipStream_t st, const uint8_t *in, uint64_t in_bytes, const ChunkDesc *chunks, const ChainItem *items,
                 uint32_t nitems, bool small, uint32_t window, uint32_t max_len, uint32_t depth, const uint16_t *cd, uint16_t *cd2);
#endif

}  // namespace lfx
