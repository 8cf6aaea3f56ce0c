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

// LazyLz77Encoder's demote kernel on one work item, in positions of the CALL's arrays (in_off + p: a chunk begins
// anywhere, the per-position arrays are aligned as a whole).  The item's positions [g0, g1) are cut on the grid of 16: the
// whole groups [a, b) take 16-byte accesses, [g0, a) and [b, g1) — under 16 positions each, or all of an item that holds no
// whole group, under 31 — share their group with a neighbouring item or chunk and go one position at a time.  gend: where the
// chunk's visited range ends; a position g is demoted only with g + 1 < gend.
constexpr uint32_t DEMOTE_GROUP = 16;
struct DemoteSpan {
    uint64_t g0, a, b, g1, gend;
};
LFX_HD inline DemoteSpan demote_span(uint64_t in_off, uint64_t len, uint64_t p0, uint32_t tile) {
    const uint64_t end = (len > 3 ? len : 3) - 3;                // default.rs:75
    const uint64_t p1 = p0 + tile < end ? p0 + tile : end;
    DemoteSpan s;
    s.g0 = in_off + (p0 < p1 ? p0 : p1);
    s.g1 = in_off + p1;
    s.gend = in_off + end;
    s.a = (s.g0 + DEMOTE_GROUP - 1) / DEMOTE_GROUP * DEMOTE_GROUP;
    s.b = s.g1 / DEMOTE_GROUP * DEMOTE_GROUP;
    if (s.a >= s.b) s.a = s.b = s.g1;                            // no whole group: [g0, g1) by hand
    return s;
}

#ifdef __HIPCC__
// behind the match stage: cd2[p] ← the distance of the longest of the first `depth` candidates on p's chain through cd (ties: the
// nearest) for every listed position p < end with cd[p] != 0, and 0 where cd[p] == 0.  cd is only read.
// len (LazyLz77Encoder; nullptr: ChainLz77Encoder's one launch, unchanged): a byte per position of scratch.  The
// chain kernel's variant also leaves each listed position's length there (L - 3; 0 without a candidate), for launch_demote.
int launch_chain(hipStream_t st, const uint8_t *in, uint64_t in_bytes, const ChunkDesc *chunks, const ChainItem *items,
                 uint32_t nitems, bool small, uint32_t window, uint32_t max_len, uint32_t depth, const uint16_t *cd, uint16_t *cd2,
                 uint8_t *len = nullptr);
// LazyLz77Encoder, behind launch_chain on the same stream and over the same work list: cd2[p] ← 0 for every listed position p
// with p + 1 < end and len[p + 1] > len[p].  len is only read; nothing but the listed positions' cd2 is written.
int launch_demote(hipStream_t st, const ChunkDesc *chunks, const ChainItem *items, uint32_t nitems, bool small, const uint8_t *len,
                  uint16_t *cd2);
#endif

}  // namespace lfx
