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

// The chain kernel's LDS, in dwords: the bytes [lo, hi) — at most wcap + tile + MAX_LENGTH, + the byte phase of lo on the dword
// grid (3), + what the last compare step and its three-dword read reach past the last byte that counts (11) — and the
// candidates of [lo, p1), + their phase on the dword grid.
constexpr uint32_t chain_lds_bytes_dw(uint32_t tile, uint32_t wcap) { return (wcap + tile + MAX_LENGTH + 3 + 11 + 3) / 4 + 1; }
constexpr uint32_t chain_lds_cand_dw(uint32_t tile, uint32_t wcap) { return (wcap + tile + 1 + 1) / 2 + 1; }
// the window instance's two arrays, with or without a dictionary in front of the chunk (the hole it fills);
// the code object says 147748, with the 8 bytes that align the second array
static_assert(4 * (chain_lds_bytes_dw(CHAIN_TILE, MAX_WINDOW) + chain_lds_cand_dw(CHAIN_TILE, MAX_WINDOW)) == 147740, "one workgroup's LDS");

// A chain dictionary in front of a primed chunk.  A tile [p0, p0 + tile) of a CH_DICT chunk with
// p0 < window_size runs the dictionary instance: its positions' chains go on across position 0 into the dictionary's tail T,
// whose last n_t bytes — all a position >= p0 can reach — and their links are staged in front of the chunk's own.  The chunk
// has no window of its own in front of position 0, so T takes the room of the window bytes a tile this close to the chunk's
// start cannot have: p0 + n_t <= window_size.  dw_t / dw_c: the dwords in front of the chunk's first dword of bytes and of
// candidates (position 0 sits at LDS byte 4 * dw_t + sh, its candidate at entry 2 * dw_c + csh).
struct ChainDictFill {
    uint32_t n_t, dw_t, dw_c;
};
LFX_HD inline ChainDictFill chain_dict_fill(uint32_t usable, uint32_t window, uint32_t p0) {
    ChainDictFill f;
    f.n_t = p0 < window ? (usable < window - p0 ? usable : window - p0) : 0u;
    f.dw_t = (f.n_t + 3) >> 2;
    f.dw_c = (f.n_t + 1) >> 1;
    return f;
}
// The work list of a call with a chain dictionary: chain_items' items in two runs, [0, n_plain) for the instance that runs
// today and [n_plain, size) — the tiles of the CH_DICT chunks with p0 < window — for the dictionary instance.  Without a chain
// dictionary (dict_chain false) it is chain_items' list and n_plain its size.
inline void chain_items_dict(const std::vector<ChunkDesc> &chunks, uint32_t tile, uint32_t window, bool dict_chain,
                             std::vector<ChainItem> &items, uint32_t &n_plain) {
    chain_items(chunks, tile, items);
    n_plain = (uint32_t)items.size();
    if (!dict_chain) return;
    auto primed = [&](const ChainItem &it) { return (chunks[it.chunk].flags & CH_DICT) && it.p0 < window; };
    n_plain = (uint32_t)(std::stable_partition(items.begin(), items.end(), [&](const ChainItem &it) { return !primed(it); }) - items.begin());
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

// the tuned instances' arguments (LFX_LZ77_LEVEL): a chain walk ends behind the first candidate of
// min(lim, nice) bytes or more, and a 3-byte match farther than too_far counts as no candidate (0xFFFFFFFF: none is)
struct ChainTune {
    uint32_t nice, too_far;
};

#ifdef __HIPCC__
// the dictionary instance's arguments: lfx_dict's window (MAX_WINDOW bytes, the tail at their end), the tail's chain on the
// same grid (launch_dict_chain), its prefix table and its length
struct ChainDict {
    const uint8_t *win;
    const uint16_t *cdt;
    const unsigned long long *tab;
    uint32_t usable;
};
// behind the match stage: cd2[p] ← the distance of the longest of the first `depth` candidates on p's chain through cd (ties: the
// nearest) for every listed position p < end with cd[p] != 0, and 0 where cd[p] == 0.  cd is only read.
// len (LazyLz77Encoder; nullptr: ChainLz77Encoder's one launch, unchanged): a byte per position of scratch.  The
// chain kernel's variant also leaves each listed position's length there (L - 3; 0 without a candidate), for launch_demote.
// dict (a chain dictionary; nullptr: every item runs today's instance): the items from n_plain on are
// chain_items_dict's second run and go, in a launch of their own, to the dictionary instance.
// tune (LFX_LZ77_LEVEL; nullptr: the instances of the kinds 2 and 3, unchanged): the tuned instances, which
// always write len (it must not be nullptr); depth is not bound by the 255 of the other kinds' bit field.
int launch_chain(hipStream_t st, const uint8_t *in, uint64_t in_bytes, const ChunkDesc *chunks, const ChainItem *items,
                 uint32_t nitems, bool small, uint32_t window, uint32_t max_len, uint32_t depth, const uint16_t *cd, uint16_t *cd2,
                 uint8_t *len = nullptr, uint32_t n_plain = 0xFFFFFFFFu, const ChainDict *dict = nullptr, const ChainTune *tune = nullptr);
// LazyLz77Encoder, behind launch_chain on the same stream and over the same work list: cd2[p] ← 0 for every listed position p
// with p + 1 < end and len[p + 1] > len[p].  len is only read; nothing but the listed positions' cd2 is written.
// max_lazy (LFX_LZ77_LEVEL; 0: LazyLz77Encoder's kernel, unchanged): only positions with a length below max_lazy are demoted.
int launch_demote(hipStream_t st, const ChunkDesc *chunks, const ChainItem *items, uint32_t nitems, bool small, const uint8_t *len,
                  uint16_t *cd2, uint32_t max_lazy = 0);
#endif

}  // namespace lfx
