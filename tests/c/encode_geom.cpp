// CPU: the host arithmetic of the encode's stages (libflate_amd/csrc/lfx_encode_stages.h) and Plan::append (lfx_plan.h) over
// seeded plans of the real Planner — mixed block sizes, write lists, flushes, literal-only chunks, 0 bytes to a few MiB — plus a
// handful of synthetic chunk lists of many GiB (descriptors only), for 1, 64 and 256 compute units.  The match segments tile
// their chunks, the link regions are even, ordered and disjoint (and the error fires exactly when a base leaves 32 bits), the
// parse workgroups in launch order are the logical list dealt out in contiguous eighths, the emit grid is what its formula
// says, and appended plans are shifted copies that keep the planner's own invariants.
#include <cstdio>
#include <random>

#include "../../libflate_amd/csrc/lfx_encode_stages.h"

using namespace lfx;

#define FAIL(...) do { printf("case %d: ", it); printf(__VA_ARGS__); printf("\n"); return false; } while (0)

static bool check_segs(const Plan &plan, const EncodeGeom &g, int it) {
    size_t q = 0;
    uint64_t inner = 0;      // the length of every segment that is not its chunk's last: the segment length in use
    for (uint32_t ci = 0; ci < plan.chunks.size(); ci++) {
        const ChunkDesc &ch = plan.chunks[ci];
        if ((ch.flags & CH_LITERALS) || ch.len <= 3) {
            if (q < g.segs.size() && g.segs[q].chunk == ci) FAIL("chunk %u (literals or %llu bytes) has a segment", ci, (unsigned long long)ch.len);
            continue;
        }
        uint64_t at = 0;
        while (q < g.segs.size() && g.segs[q].chunk == ci) {
            const SegDesc &s = g.segs[q];
            if (s.start != at || s.len == 0) FAIL("chunk %u: a segment starts at %u, the one before ended at %llu", ci, s.start, (unsigned long long)at);
            if ((uint64_t)s.start + 3 >= ch.len) FAIL("chunk %u: a segment starts in the last three bytes", ci);
            at += s.len;
            if (at < ch.len) {
                if (inner && s.len != inner) FAIL("two segment lengths: %llu and %u", (unsigned long long)inner, s.len);
                inner = s.len;
            }
            q++;
        }
        if (at + 3 < ch.len || at > ch.len) FAIL("chunk %u: the segments end at %llu of %llu", ci, (unsigned long long)at, (unsigned long long)ch.len);
    }
    if (q != g.segs.size()) FAIL("%zu segments belong to no chunk in order", g.segs.size() - q);
    // >= 512 segments, or the length bottomed out at 32 Ki positions; and no halving more than that needs
    auto count_at = [&](uint64_t len) {
        uint64_t cnt = 0;
        for (const ChunkDesc &ch : plan.chunks)
            if (!(ch.flags & CH_LITERALS) && ch.len > 3) cnt += div_up(ch.len - 3, len);
        return cnt;
    };
    for (const SegDesc &s : g.segs)
        if (s.len > SEG_POSITIONS) FAIL("a segment of %u positions", s.len);
    if (inner) {
        if (inner != 32768 && inner != 65536 && inner != 131072 && inner != 262144) FAIL("segment length %llu", (unsigned long long)inner);
        if (inner > 32768 && count_at(inner) < 512) FAIL("%llu segments of %llu positions: could be halved", (unsigned long long)count_at(inner), (unsigned long long)inner);
        if (inner < SEG_POSITIONS && count_at(inner * 2) >= 512) FAIL("segment length %llu: twice that still gives 512 segments", (unsigned long long)inner);
    } else if (g.segs.size() < 512) {
        for (const SegDesc &s : g.segs)
            if (s.len > 32768) FAIL("%zu segments, one of %u positions: could be halved", g.segs.size(), s.len);
    }
    return true;
}

// The link regions of segs[0, count): even, increasing bases, no region reaching into the next, and `units` the even end of the
// last one.  Independent of how the segment length was chosen: only what the device relies on.
static bool check_links(const EncodeGeom &g, size_t count, uint64_t units, int it) {
    uint64_t end = 0;
    for (size_t q = 0; q < count; q++) {
        const SegDesc &s = g.segs[q];
        if (s.lnk_base & 1) FAIL("segment %zu: odd link base %u", q, s.lnk_base);
        if (q && s.lnk_base <= g.segs[q - 1].lnk_base) FAIL("segment %zu: link base %u not behind the one before", q, s.lnk_base);
        if (s.lnk_base < end) FAIL("segment %zu: link base %u inside the region before it (ends at %llu)", q, s.lnk_base, (unsigned long long)end);
        end = (uint64_t)s.lnk_base + div_up((uint64_t)s.len + std::min<uint64_t>(s.start, MAX_WINDOW) + 4, 64);
    }
    if (units < end || units > end + 1 || (units & 1)) FAIL("lnk_units %llu, the last region ends at %llu", (unsigned long long)units, (unsigned long long)end);
    return true;
}
// A refusal: the segments in front of the first one without a base are laid out as above, and the base that one would have
// got — the even end of the regions so far — does not fit 32 bits.  (An accepted list whose bases had wrapped would fail
// check_links: they would no longer increase.)
static bool check_links_refused(const EncodeGeom &g, int it) {
    size_t based = 1;
    while (based < g.segs.size() && g.segs[based].lnk_base != 0) based++;
    if (based == g.segs.size()) FAIL("refused, but every segment has a link base");
    if (!check_links(g, based, g.lnk_units, it)) return false;
    if (g.lnk_units <= 0xFFFFFFFFull) FAIL("refused at segment %zu, whose base %llu fits 32 bits", based, (unsigned long long)g.lnk_units);
    return true;
}

static bool check_pwgs(const Plan &plan, const EncodeGeom &g, int it) {
    std::vector<ParseWg> logical;
    for (uint32_t ci = 0; ci < plan.chunks.size(); ci++) {
        const ChunkDesc &ch = plan.chunks[ci];
        if (ch.flags & CH_LITERALS) continue;
        for (uint32_t s = 0; s < ch.n_seg; s += PARSE_WG_SEGS) logical.push_back(ParseWg{ci, s});   // covers segments [s, s + PARSE_WG_SEGS) of the chunk
    }
    std::vector<ParseWg> dealt;
    if (g.pwgs.size() <= 8 || logical.size() <= 8) {
        dealt = g.pwgs;
        for (const ParseWg &w : dealt)
            if (w.chunk == 0xFFFFFFFFu) FAIL("an empty slot among %zu workgroups", g.pwgs.size());
    } else {
        if (g.pwgs.size() % 8) FAIL("%zu slots: not eight equal eighths", g.pwgs.size());
        // slot i belongs to eighth i % 8: the eighths one after the other must be the logical list, each a contiguous run of it
        for (size_t e = 0; e < 8; e++) {
            bool ended = false;
            for (size_t i = e; i < g.pwgs.size(); i += 8) {
                const ParseWg &w = g.pwgs[i];
                if (w.chunk == 0xFFFFFFFFu) {
                    if (w.seg0 != 0) FAIL("slot %zu: an empty slot with seg0 %u", i, w.seg0);
                    ended = true;
                    continue;
                }
                if (ended) FAIL("slot %zu: a workgroup behind an empty slot of its eighth", i);
                dealt.push_back(w);
            }
        }
        const size_t per = g.pwgs.size() / 8;
        if (per != (logical.size() + 7) / 8) FAIL("%zu slots for %zu workgroups", g.pwgs.size(), logical.size());
    }
    if (dealt.size() != logical.size()) FAIL("%zu workgroups in launch order, %zu in the logical list", dealt.size(), logical.size());
    for (size_t i = 0; i < logical.size(); i++)
        if (dealt[i].chunk != logical[i].chunk || dealt[i].seg0 != logical[i].seg0) FAIL("workgroup %zu: (%u, %u), the logical list has (%u, %u)", i, dealt[i].chunk, dealt[i].seg0, logical[i].chunk, logical[i].seg0);
    return true;
}

static bool check_emit(const Plan &plan, const EncodeGeom &g, uint32_t n_cu, bool hist_separate, int it) {
    if (g.emit_per == 0 || g.emit_per % PARSE_EMIT_WAVES) FAIL("emit_per %u", g.emit_per);
    uint32_t max_segs = 0;
    uint64_t useful = 0;
    for (const ChunkDesc &ch : plan.chunks) {
        max_segs = std::max(max_segs, ch.n_seg);
        useful += div_up(ch.n_seg, g.emit_per);
    }
    const uint64_t parts = div_up(max_segs, g.emit_per);
    if (g.emit_parts != parts) FAIL("emit_parts %u, %llu expected", g.emit_parts, (unsigned long long)parts);
    // (about PARSE_EMIT_WG_PER_CU workgroups per CU: a share of segments never smaller than that needs)
    if ((uint64_t)g.emit_per * PARSE_EMIT_WG_PER_CU * n_cu < plan.n_segs) FAIL("emit_per %u: more than %u workgroups per CU", g.emit_per, PARSE_EMIT_WG_PER_CU);
    const bool must_not = hist_separate || parts > 65535 || (uint64_t)plan.chunks.size() * parts > 4 * useful + 4096;
    if (g.fused_hist == must_not) FAIL("fused_hist %d (separate %d, parts %llu, grid %llu, useful %llu)", (int)g.fused_hist, (int)hist_separate,
                                       (unsigned long long)parts, (unsigned long long)(plan.chunks.size() * parts), (unsigned long long)useful);
    const uint32_t nch = (uint32_t)plan.chunks.size();
    if (g.split < 1 || g.split > 1024 || (nch >= 1024 && g.split != 1) || (nch && nch < 1024 && (uint64_t)g.split * nch < 2048 && g.split != 1024))
        FAIL("histogram split %u for %u chunks", g.split, nch);
    return true;
}

// the planner's own invariants (what the kernels rely on), for a plan and for what Plan::append makes of several
static bool check_plan(const Plan &p, int it) {
    for (size_t j = 0; j < p.chunks.size(); j++) {
        const ChunkDesc &c = p.chunks[j];
        const uint64_t code_end = c.code_off + c.len + 1, tile_end = c.tile_base + div_up(c.len + 1, PACK_TILE);
        const uint64_t vis_end = c.vis_base + (uint64_t)c.n_seg * 64, seg_end = (uint64_t)c.seg_base + c.n_seg;
        const bool last = j + 1 == p.chunks.size();
        if ((last ? p.n_codes_cap : p.chunks[j + 1].code_off) < code_end) FAIL("chunk %zu: code slots overlap the next", j);
        if ((last ? p.n_tiles : p.chunks[j + 1].tile_base) < tile_end) FAIL("chunk %zu: tiles overlap the next", j);
        if ((last ? p.n_vis : p.chunks[j + 1].vis_base) < vis_end) FAIL("chunk %zu: mask words overlap the next", j);
        if ((last ? p.n_segs : p.chunks[j + 1].seg_base) < seg_end) FAIL("chunk %zu: segments overlap the next", j);
        if (c.block >= p.blocks.size()) FAIL("chunk %zu: block %u of %zu", j, c.block, p.blocks.size());
    }
    for (size_t b = 0; b < p.blocks.size(); b++) {
        const BlockDesc &bd = p.blocks[b];
        if ((uint64_t)bd.first_chunk + bd.n_chunks > p.chunks.size()) FAIL("block %zu: chunks [%u, +%u) of %zu", b, bd.first_chunk, bd.n_chunks, p.chunks.size());
        for (uint32_t j = 0; j < bd.n_chunks; j++)
            if (p.chunks[bd.first_chunk + j].block != b) FAIL("block %zu: its chunk %u carries block %u", b, j, p.chunks[bd.first_chunk + j].block);
    }
    return true;
}
static bool check_append(const Plan &p, uint64_t len, uint32_t copies, int it) {
    Plan all;
    for (uint32_t i = 0; i < copies; i++) all.append(p, i * len);
    const size_t nc = p.chunks.size(), nb = p.blocks.size();
    if (all.chunks.size() != copies * nc || all.blocks.size() != copies * nb || all.n_codes_cap != copies * p.n_codes_cap ||
        all.n_tiles != copies * p.n_tiles || all.n_vis != copies * p.n_vis || all.n_segs != copies * p.n_segs) FAIL("append: counters of %u copies", copies);
    for (uint32_t i = 0; i < copies; i++) {
        for (size_t j = 0; j < nc; j++) {
            const ChunkDesc &a = all.chunks[i * nc + j], &c = p.chunks[j];
            if (a.in_off != c.in_off + i * len || a.len != c.len || a.code_off != c.code_off + i * p.n_codes_cap || a.block != c.block + i * nb ||
                a.flags != c.flags || a.tile_base != c.tile_base + i * p.n_tiles || a.vis_base != c.vis_base + i * p.n_vis ||
                a.seg_base != c.seg_base + i * p.n_segs || a.n_seg != c.n_seg) FAIL("append: chunk %zu of copy %u", j, i);
        }
        for (size_t b = 0; b < nb; b++) {
            const BlockDesc &a = all.blocks[i * nb + b], &c = p.blocks[b];
            if (a.in_off != c.in_off + i * len || a.in_len != c.in_len || a.first_chunk != c.first_chunk + i * nc || a.n_chunks != c.n_chunks ||
                a.type != c.type || a.final != c.final || a.align_after != c.align_after) FAIL("append: block %zu of copy %u", b, i);
        }
    }
    return check_plan(all, it);
}

// every check of one geometry; → false with a message
static bool check_geometry(const Plan &plan, bool host_codes, uint32_t n_cu, bool hist_separate, int it) {
    const EncodeGeom g = encode_geometry(plan, host_codes, n_cu, hist_separate);
    bool too_long = false;
    for (const ChunkDesc &ch : plan.chunks) too_long |= ch.len >= (1ull << 32) - 4;
    if (too_long) { if (g.err != GEOM_E_CHUNK_4G) FAIL("a chunk of 4 GiB: error %d", g.err); return true; }
    if (host_codes) {
        if (g.err || !g.segs.empty() || !g.pwgs.empty() || g.lnk_units || g.fused_hist) FAIL("host codes: segments, workgroups or a fused histogram");
        return true;
    }
    if (g.err == GEOM_E_LINK_SCRATCH) return check_links_refused(g, it);
    if (g.err) FAIL("error %d", g.err);
    return check_segs(plan, g, it) && check_links(g, g.segs.size(), g.lnk_units, it) && check_pwgs(plan, g, it) && check_emit(plan, g, n_cu, hist_separate, it);
}

// a chunk list of `count` chunks of `len` bytes, as the planner lays them out (descriptors only: there is no such input)
static Plan synthetic(uint32_t count, uint64_t len, uint64_t last_len) {
    Plan p;
    for (uint32_t i = 0; i < count; i++) {
        ChunkDesc c{};
        c.len = i + 1 == count ? last_len : len;
        c.in_off = (uint64_t)i * len; c.code_off = p.n_codes_cap; c.block = i; c.flags = CH_LAST_IN_BLOCK;
        c.tile_base = p.n_tiles; c.vis_base = p.n_vis; c.seg_base = p.n_segs; c.n_seg = (uint32_t)div_up(c.len, PARSE_SEG);
        p.n_codes_cap += c.len + 1; p.n_tiles += div_up(c.len + 1, PACK_TILE); p.n_vis += (uint64_t)c.n_seg * 64; p.n_segs += c.n_seg;
        p.chunks.push_back(c);
        BlockDesc b{};
        b.in_off = c.in_off; b.in_len = c.len; b.first_chunk = i; b.n_chunks = 1; b.type = BT_DYNAMIC; b.final = i + 1 == count;
        p.blocks.push_back(b);
    }
    return p;
}

int main() {
    std::mt19937_64 rng(20261018);
    const uint32_t cus[3] = {1, 64, 256};
    int cases = 0, permuted = 0, halved = 0, bottomed = 0, literal = 0, unfused = 0;
    for (int it = 0; it < 4000; it++) {
        PlanOpts o;
        const uint64_t bs[] = {1, 100, 4096, 65535, 65536, 300 << 10, 1 << 20, 4 << 20};
        o.block_size = bs[rng() % 8];
        o.dynamic_huffman = rng() & 1;
        o.no_compression = (rng() % 8) == 0;
        o.lz77_kind = (rng() % 5) == 0;
        const uint32_t ws[] = {256, 1024, 32768};
        o.window_size = ws[rng() % 3];
        o.zlib_sync = (rng() % 7) == 0;
        Planner pl(o);
        // a write list: a size class (0 bytes to a few MiB in all), a few writes and flushes
        const uint64_t tops[] = {0, 1, 3, 4, 5, 3328, 40000, 300000, 524288, 1 << 20, 3 << 20, 6 << 20};
        uint64_t left = tops[rng() % 12];
        if (left > 5) left = left / 2 + rng() % (left / 2 + 1);
        if (o.block_size == 1 || o.block_size == 100) left = std::min<uint64_t>(left, 40000);     // (a block per byte: keep the lists short)
        const int events = 1 + (int)(rng() % 6);
        for (int k = 0; k < events && left; k++) {
            if (rng() % 5 == 0) { pl.flush(); continue; }
            const uint64_t w = k + 1 == events ? left : rng() % (left + 1);
            if (rng() & 1) pl.write(w); else { const uint64_t piece = 1 + rng() % 8192; pl.write_repeat(piece, w / piece); pl.write(w % piece); }
            left -= w;
        }
        const uint64_t len = pl.cursor();
        const Plan plan = pl.finish();
        if (!check_plan(plan, it)) return 1;
        const uint32_t n_cu = cus[it % 3];
        const bool hist_separate = rng() % 4 == 0, host_codes = rng() % 16 == 0;
        if (!check_geometry(plan, host_codes, n_cu, hist_separate, it)) return 1;
        if (!check_append(plan, len, 1 + (uint32_t)(rng() % 4), it)) return 1;
        if (!host_codes) {
            const EncodeGeom g = encode_geometry(plan, false, n_cu, hist_separate);
            permuted += g.pwgs.size() > 8;
            unfused += !g.fused_hist && !hist_separate;
            for (const SegDesc &s : g.segs) { halved += s.len == 65536 || s.len == 131072; bottomed += s.len == 32768; }
            for (const ChunkDesc &ch : plan.chunks) literal += (ch.flags & CH_LITERALS) != 0;
        }
        cases++;
    }
    // synthetic chunk lists of many GiB: the segment length stays at its maximum, the link bases reach (and leave) 32 bits, a
    // chunk of 4 GiB is refused; a few huge chunks among thousands of small ones take the separate histogram
    int big = 0, refused_links = 0, refused_chunk = 0;
    const uint64_t g4 = (1ull << 32) - 5;          // the longest chunk inside the domain
    const struct { uint32_t count; uint64_t len, last; } lists[] = {{3, 1ull << 31, 12345}, {300, 200000, 200000}, {8, g4, g4}, {40, g4, 7}, {63, g4, g4}, {66, g4, g4},
                                                                     {70, g4, 1ull << 20}, {2, g4 + 1, 5}, {5, 1ull << 30, g4 + 100}};
    for (const auto &l : lists) {
        const int it = 100000 + big;
        const Plan plan = synthetic(l.count, l.len, l.last);
        if (!check_plan(plan, it)) return 1;
        for (uint32_t n_cu : cus)
            if (!check_geometry(plan, false, n_cu, false, it)) return 1;
        const EncodeGeom g = encode_geometry(plan, false, 256, false);
        refused_links += g.err == GEOM_E_LINK_SCRATCH;
        refused_chunk += g.err == GEOM_E_CHUNK_4G;
        for (const SegDesc &s : g.segs) halved += s.len == 65536 || s.len == 131072;
        big++;
    }
    {
        Plan mixed = synthetic(3000, 5000, 5000);
        Plan huge = synthetic(2, 1ull << 31, 1ull << 31);
        mixed.append(huge, 3000 * 5000ull);
        const int it = 200000;
        if (!check_plan(mixed, it)) return 1;
        for (uint32_t n_cu : cus)
            if (!check_geometry(mixed, false, n_cu, false, it)) return 1;
        unfused += !encode_geometry(mixed, false, 256, false).fused_hist;
        big++;
    }
    if (!permuted || !halved || !bottomed || !literal || !unfused || !refused_links || !refused_chunk) {
        printf("a kind of case never came up (%d %d %d %d %d %d %d)\n", permuted, halved, bottomed, literal, unfused, refused_links, refused_chunk);
        return 1;
    }
    printf("encode_geom ok: %d plans, %d synthetic lists\n", cases, big);
    return 0;
}
