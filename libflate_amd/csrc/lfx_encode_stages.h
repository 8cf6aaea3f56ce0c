// lfx_encode_stages.h — the host arithmetic of the encode's stages (encode_prepare, lfx_encode.cpp): how the chunks are cut into
// match segments, where every segment's link region lies, which workgroups the parse walk gets and in which order, how the
// emit + histogram grid is sized.  Pure index arithmetic on a Plan — no HIP call, no context: compiles with a plain host
// compiler (tests/c/encode_geom.cpp).  A wrong lnk_base or a dropped ParseWg is a wild write or a silently missing segment on
// the device.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "lfx_plan.h"

namespace lfx {

enum : int { GEOM_OK = 0, GEOM_E_CHUNK_4G = 1, GEOM_E_LINK_SCRATCH = 2 };
inline const char *geom_error(int err) {
    return err == GEOM_E_CHUNK_4G ? "an LZ77 chunk of 4 GiB or more is outside the reference's domain (u32 positions, default.rs:78)"
                                  : "input too large for the link scratch";
}

struct EncodeGeom {
    int err = GEOM_OK;            // GEOM_E_*: nothing else is meaningful then
    std::vector<SegDesc> segs;    // match segments, lnk_base filled
    uint64_t lnk_units = 0;       // link scratch, in units of 64 entries: covers every segment's region
    std::vector<ParseWg> pwgs;    // workgroups of the parse walk, in launch order ({0xFFFFFFFF, 0}: an empty slot)
    uint32_t emit_per = 0, emit_parts = 0;   // parse_emit_hist_kernel: segments per workgroup, workgroups for the chunk of most segments
    bool fused_hist = false;      // the parse counts the blocks' symbols (no histogram_kernel)
    uint32_t split = 1;           // histogram_kernel: workgroups per chunk
    bool pack_by_chunk = false;   // symbol counts per chunk, huffman_chunk_kernel, pack_chunk_kernel (no tile_bits / tile_scan / pack_kernel)
};
enum : int { PACK_BY_CHUNK_AUTO = -1, PACK_BY_CHUNK_OFF = 0, PACK_BY_CHUNK_ON = 1 };   // LFX_PACK_BY_CHUNK (Diag::pack_by_chunk)

// host_codes: the code words come from the caller (no match, no parse: no segments and no workgroups).
// pack_switch: PACK_BY_CHUNK_*.
inline EncodeGeom encode_geometry(const Plan &plan, bool host_codes, uint32_t n_cu, bool hist_separate,
                                  int pack_switch = PACK_BY_CHUNK_AUTO) {
    EncodeGeom g;
    for (const ChunkDesc &ch : plan.chunks)
        if (ch.len >= (1ull << 32) - 4) { g.err = GEOM_E_CHUNK_4G; return g; }
    const uint32_t nchunks = (uint32_t)plan.chunks.size();
    // enough workgroups to fill the GPU even when there are few chunks (schedule S1: one)
    // (more workgroups per chunk were measured slower at 1024 chunks: 8 per chunk 0.23 ms against 0.20 ms for one —
    //  every workgroup ends with a global atomic per non-zero counter)
    g.split = nchunks && nchunks < 1024 ? std::min<uint32_t>(1024, 2048 / nchunks + 1) : 1;
    if (host_codes) return g;
    // A segment is one workgroup's serial walk (plus a 32 KiB warm-up when it does not start a chunk).  Small
    // inputs are cut finer so that the GPU still fills: halve the segment length until there are >= 512 of them
    // (never below 32 Ki positions: the warm-up would dominate).
    uint64_t seg_len = SEG_POSITIONS;
    for (;;) {
        uint64_t cnt = 0;
        for (const ChunkDesc &ch : plan.chunks)
            if (!(ch.flags & CH_LITERALS) && ch.len > 3) cnt += div_up(ch.len - 3, seg_len);
        if (cnt >= 512 || seg_len <= 32768) break;
        seg_len /= 2;
    }
    for (uint32_t ci = 0; ci < nchunks; ci++) {
        const ChunkDesc &ch = plan.chunks[ci];
        if (ch.flags & CH_LITERALS) continue;
        for (uint64_t s = 0; s + 3 < ch.len; s += seg_len)
            g.segs.push_back(SegDesc{ci, (uint32_t)s, (uint32_t)std::min<uint64_t>(seg_len, ch.len - s), 0});
    }
    // lfx_match7: every segment keeps the final links of its positions — its warm-up included — in a region of its own
    for (SegDesc &sg : g.segs) {
        if (g.lnk_units > 0xFFFFFFFFull) { g.err = GEOM_E_LINK_SCRATCH; return g; }
        sg.lnk_base = (uint32_t)g.lnk_units;
        g.lnk_units += div_up((uint64_t)sg.len + std::min<uint64_t>(sg.start, MAX_WINDOW) + 4, 64);
        g.lnk_units = (g.lnk_units + 1) & ~1ull;   // (even: lfx_match7 stores two ballot words, one per unit, as 16 bytes)
    }
    // workgroups of the parse walk: PARSE_WG_SEGS consecutive segments of one chunk each
    for (uint32_t ci = 0; ci < nchunks; ci++) {
        const ChunkDesc &ch = plan.chunks[ci];
        if (ch.flags & CH_LITERALS) continue;
        for (uint32_t s = 0; s < ch.n_seg; s += PARSE_WG_SEGS) g.pwgs.push_back(ParseWg{ci, s});
    }
    // XCD-aware launch order: workgroup i runs on XCD i mod 8, and every XCD has an L2 of its own.  A workgroup stages the
    // 32 KiB window in front of its 13 KiB of positions — the positions of its two or three left neighbours — so each XCD
    // takes one contiguous eighth of the list and finds those bytes (and its own `cd` lines) in ITS L2 instead of
    // fetching them over the fabric again (slots behind the end of an eighth are marked empty).
    if (g.pwgs.size() > 8) {
        const size_t nl = g.pwgs.size(), per = (nl + 7) / 8;
        std::vector<ParseWg> phys(per * 8);
        for (size_t i = 0; i < phys.size(); i++) {
            const size_t l = (i % 8) * per + i / 8;
            phys[i] = (i / 8 < per && l < nl && l / per == i % 8) ? g.pwgs[l] : ParseWg{0xFFFFFFFFu, 0u};
        }
        g.pwgs.swap(phys);
    }
    // The blocks' symbol counts are taken by the kernel that writes the code words (parse_emit_hist_kernel): a grid of
    // nchunks x (workgroups of the longest chunk), about eight workgroups per CU in all.  A chunk list of very unequal chunks
    // (a few huge ones among thousands of small ones) would launch mostly empty workgroups: histogram_kernel counts then.
    const uint32_t target = PARSE_EMIT_WG_PER_CU * std::max<uint32_t>(n_cu, 1);
    uint32_t per = (uint32_t)div_up(std::max<uint32_t>(plan.n_segs, 1), target);
    per = (per + PARSE_EMIT_WAVES - 1) / PARSE_EMIT_WAVES * PARSE_EMIT_WAVES;
    uint32_t max_segs = 0;
    uint64_t useful = 0;
    for (uint32_t ci = 0; ci < nchunks; ci++) {
        max_segs = std::max(max_segs, plan.chunks[ci].n_seg);
        useful += div_up(plan.chunks[ci].n_seg, per);
    }
    const uint64_t parts = div_up(max_segs, per);
    g.fused_hist = !hist_separate && parts <= 65535 && (uint64_t)nchunks * parts <= 4 * useful + 4096;
    g.emit_per = per;
    g.emit_parts = (uint32_t)parts;
    // Pack by chunk needs the chunks' own symbol counts (the fused histogram keeps them) and sizes compressed blocks only.  It
    // pays where every CU gets a chunk to walk and no walk is long: a workgroup packs a chunk's tiles one after the other.
    // LFX_PACK_BY_CHUNK=1 takes it wherever it is legal, whatever the chunks; =0 never.
    bool stored = false;
    uint64_t max_tiles = 0;
    for (const BlockDesc &b : plan.blocks) stored |= b.type == BT_RAW;
    for (const ChunkDesc &ch : plan.chunks) max_tiles = std::max<uint64_t>(max_tiles, div_up(ch.len + 1, PACK_TILE));
    const bool legal = g.fused_hist && !stored && nchunks > 0;
    g.pack_by_chunk = legal && pack_switch != PACK_BY_CHUNK_OFF &&
                      (pack_switch == PACK_BY_CHUNK_ON || (nchunks >= std::max<uint32_t>(n_cu, 1) && max_tiles <= PACK_CHUNK_MAX_TILES));
    return g;
}

}  // namespace lfx
