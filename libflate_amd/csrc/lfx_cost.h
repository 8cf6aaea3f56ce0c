// lfx_cost.h — CostLz77Encoder (LFX_LZ77_COST): the work list of the cost recurrence (lfx_cost.hip), its index
// arithmetic and the arithmetic of its cost tables.  Pure host-compilable code on a chunk list and a block's code widths —
// tests/c/cost_opts.cpp replays all of it with a plain host compiler.  Internal.
//
// The rule (include/lfx.h is its prose, tests/cost_model.py its first statement).  The candidates (L(p), D(p)) are the level's,
// a function of the position alone.  For a parsed chunk with visited range [0, end) every position chooses between "literal at
// p" and "the match (L(p), D(p)) at p" by its cost in bits under the code of the chunk's owning block:
//   lit(p) = the width of the literal buf[p]
//   mat(p) = the width of L(p)'s length symbol + its extra bits + the width of D(p)'s distance symbol + its extra bits
// The chunk is cut on a grid of COST_SEG positions from its start.  For the segment [a, b) the recurrence starts at
// top = min(b + COST_WARM, end) with cost[top] = 0 and runs backward:
//   cost[p] = min(lit(p) + cost[p + 1], mat(p) + cost[min(p + L(p), top)])        the match term only where cd2[p] != 0
// On a tie the match wins.  Decisions are kept for p in [a, b): the position loses its candidate where the literal won; the
// warm-up positions are the next segment's to decide.  Nothing at or behind top is read, so nothing is read across a chunk.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include <vector>

#include "lfx_common.h"
#include "lfx_huff.h"

namespace lfx {

// Positions per segment and the warm-up behind it.  One value each, the same in tests/cost_model.py and include/lfx.h.
// DESIGN.md §27 has the model's sweep: on text any warm-up of 128 or more gives the bits of the uncut chunk at every segment
// length from 1024 to 8192, so the two values set the lane count and the share of re-walked positions (an eighth), not the size.
constexpr uint32_t COST_SEG = 4096;
constexpr uint32_t COST_WARM = 512;
// what a symbol without a code costs when its whole alphabet has none in the block
constexpr uint32_t COST_NONE_LIT = 9, COST_NONE_DIST = 5;

// one lane of the cost kernel: the segment of chunk `chunk` that begins at position a (a multiple of COST_SEG)
struct CostItem {
    uint32_t chunk;
    uint32_t a;
};
// The work list: the visited range [0, end) of every parsed chunk (default.rs:75), COST_SEG positions to an item — the chunks
// chain_items lists, cut finer.
inline void cost_items(const std::vector<ChunkDesc> &chunks, std::vector<CostItem> &items) {
    items.clear();
    for (uint32_t ci = 0; ci < (uint32_t)chunks.size(); ci++) {
        const ChunkDesc &ch = chunks[ci];
        if ((ch.flags & CH_LITERALS) || ch.len <= 3) continue;
        const uint64_t end = ch.len - 3;
        for (uint64_t a = 0; a < end; a += COST_SEG) items.push_back(CostItem{ci, (uint32_t)a});
    }
}

// A segment in positions of its chunk: decisions for [a, b), the recurrence from top down to a.  a <= b <= top <= end; an
// item that is not listed (a >= end) is empty: a == b == top.
struct CostSpan {
    uint32_t a, b, top;
};
LFX_HD inline CostSpan cost_span(uint64_t len, uint32_t a) {
    const uint64_t end = (len > 3 ? len : 3) - 3;                // default.rs:75
    CostSpan s;
    s.a = (uint32_t)(a < end ? a : end);
    s.b = (uint32_t)((uint64_t)s.a + COST_SEG < end ? (uint64_t)s.a + COST_SEG : end);
    s.top = (uint32_t)((uint64_t)s.b + COST_WARM < end ? (uint64_t)s.b + COST_WARM : end);
    return s;
}

// The costs are kept modulo 2^16 and compared by the sign of their 16-bit difference.  That is exact: a literal costs at most
// COST_MAX_LIT bits, so cost[q] <= COST_MAX_LIT * k + cost[q + k], and every cost is at least the smallest of the
// max_length costs behind it — all costs within max_length + 1 positions lie within COST_MAX_LIT * MAX_LENGTH of each other,
// and the two sums compared differ by less than that plus one match: far below 2^15.
constexpr uint32_t COST_MAX_LIT = 16;        // a 15-bit code, or an absent symbol behind one
constexpr uint32_t COST_MAX_MATCH = 16 + 5 + 16 + 13;
static_assert(COST_MAX_LIT * MAX_LENGTH + COST_MAX_MATCH + COST_MAX_LIT < 32768, "16-bit costs compare exactly");
// the ring of a lane's last costs: cost[p + 1 .. p + max_length] are read at p, cost[p] is written — slot (top - q) mod COST_RING
constexpr uint32_t COST_RING = 262;
static_assert(COST_RING > MAX_LENGTH + 1 && COST_RING % 2 == 0 && (COST_RING / 2) % 2 == 1, "holds the reach of a match; an odd number of dwords per lane");

// The cost tables of one block, a byte per entry: [0, 256) lit(byte), [256, 512) the length part of mat by L - 3 (the byte
// of the length array), [512, 542) the distance part by distance symbol.
constexpr uint32_t COST_TAB_LEN = 256, COST_TAB_DIST = 512, COST_TAB_N = 542;
constexpr uint32_t COST_TAB_STRIDE = 548;    // bytes per lane in LDS: an odd number of dwords
static_assert(COST_TAB_STRIDE >= COST_TAB_N && COST_TAB_STRIDE % 4 == 0 && (COST_TAB_STRIDE / 4) % 2 == 1, "a lane's table");

// the fixed code's widths (FixedHuffmanCodec, symbol.rs:258-280)
LFX_HD inline uint32_t cost_fixed_lit_width(uint32_t s) { return s < 144 ? 8u : s < 256 ? 9u : s < 280 ? 7u : 8u; }
// what a symbol without a code costs in an alphabet of n entries (width << 16, BlockCodes): one bit more than the longest
// code, or `none` when the alphabet has no code at all
LFX_HD inline uint32_t cost_absent(const uint32_t *tab, uint32_t n, uint32_t none) {
    uint32_t m = 0;
    for (uint32_t i = 0; i < n; i++) m = (tab[i] >> 16) > m ? tab[i] >> 16 : m;
    return m ? m + 1 : none;
}
// entry i of a block's cost table.  lit / dist: BlockCodes::lit / dist of the first pass (unread under fixed codes);
// absent_lit / absent_dist: cost_absent of the two alphabets (286 and 30 entries).
LFX_HD inline uint32_t cost_tab_entry(uint32_t i, bool fixed, const uint32_t *lit, const uint32_t *dist, uint32_t absent_lit,
                                      uint32_t absent_dist) {
    if (i < COST_TAB_LEN) {
        if (fixed) return cost_fixed_lit_width(i);
        const uint32_t w = lit[i] >> 16;
        return w ? w : absent_lit;
    }
    if (i < COST_TAB_DIST) {
        uint32_t eb, ex;
        const uint32_t s = len_symbol(i - COST_TAB_LEN + 3, eb, ex);
        if (fixed) return cost_fixed_lit_width(s) + eb;
        const uint32_t w = lit[s] >> 16;
        return (w ? w : absent_lit) + eb;
    }
    const uint32_t s = i - COST_TAB_DIST;
    if (fixed) return 5 + dist_extra_bits_of_symbol(s);
    const uint32_t w = dist[s] >> 16;
    return (w ? w : absent_dist) + dist_extra_bits_of_symbol(s);
}

// One step of the recurrence on 16-bit costs: → the cost of p, *literal = whether the literal won.  has: cd2[p] != 0;
// c_next = cost[p + 1], c_jump = cost[min(p + L(p), top)], both modulo 2^16.
LFX_HD inline uint32_t cost_step(uint32_t lit, bool has, uint32_t mat, uint32_t c_next, uint32_t c_jump, bool *literal) {
    const uint32_t cl = (lit + c_next) & 0xFFFFu, cm = (mat + c_jump) & 0xFFFFu;
    const bool take = has && (int16_t)(uint16_t)(cm - cl) <= 0;      // a tie: the match
    *literal = !take;
    return take ? cm : cl;
}

#ifdef __HIPCC__
// behind the chain stage (cd2 and len hold the level's candidates, undemoted) and, with dynamic codes, behind a first pass'
// Huffman kernel (bc): cd[p] ← cd2[p] where the match won and 0 where the literal did, for every position p of the listed
// segments.  Out of place — a warm-up reads cd2 at positions another lane decides (lfx_cost.hip); cd is the match stage's array,
// which nothing reads behind the chain stage.  in, len, cd2, chunks, bc are only read.  fixed: the call's blocks use the fixed
// code, bc is unread.
int launch_cost_demote(hipStream_t st, const uint8_t *in, const ChunkDesc *chunks, const CostItem *items, uint32_t nitems,
                       const BlockCodes *bc, bool fixed, const uint8_t *len, const uint16_t *cd2, uint16_t *cd);
#endif

}  // namespace lfx
