// lazy_opts.cpp — the host-only parts of LazyLz77Encoder (LFX_LZ77_LAZY) under a plain host compiler: how
// lz77_kind is decoded and checked for kind 3 (lfx_enc_frame.h) with the kinds 0, 1 and 2 answering as before, what the
// container headers say, that the planner cuts a kind-3 schedule as it cuts a kind-0 one (lfx_plan.h), and the demote kernel's
// cut of a work item on the grid of 16 positions (lfx_chain.h), replayed on the host against the rule itself.  No HIP, no device.
//   g++ -O2 -std=c++17 -Wall [-fsanitize=address,undefined] -o lazy_opts tests/c/lazy_opts.cpp && ./lazy_opts
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../libflate_amd/csrc/lfx_chain.h"
#include "../../libflate_amd/csrc/lfx_enc_frame.h"

using namespace lfx;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "lazy_opts: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static lfx_encode_opts with_kind(int32_t kind) {
    lfx_encode_opts o;
    encode_opts_default(&o);
    o.lz77_kind = kind;
    return o;
}
// the options resolved (encode_spec): the status beside the spec
struct Resolved { int rc; EncodeSpec sp; };
static Resolved resolve(int format, const lfx_encode_opts &o) { Resolved r; r.rc = encode_spec(format, &o, &r.sp); return r; }
static bool same_plan(const Plan &a, const Plan &b) {
    if (a.chunks.size() != b.chunks.size() || a.blocks.size() != b.blocks.size() || a.n_codes_cap != b.n_codes_cap ||
        a.n_tiles != b.n_tiles || a.n_vis != b.n_vis || a.n_segs != b.n_segs) return false;
    for (size_t i = 0; i < a.chunks.size(); i++)
        if (a.chunks[i].in_off != b.chunks[i].in_off || a.chunks[i].len != b.chunks[i].len || a.chunks[i].flags != b.chunks[i].flags ||
            a.chunks[i].block != b.chunks[i].block || a.chunks[i].code_off != b.chunks[i].code_off) return false;
    for (size_t i = 0; i < a.blocks.size(); i++)
        if (a.blocks[i].in_off != b.blocks[i].in_off || a.blocks[i].in_len != b.blocks[i].in_len || a.blocks[i].type != b.blocks[i].type ||
            a.blocks[i].final != b.blocks[i].final || a.blocks[i].first_chunk != b.blocks[i].first_chunk) return false;
    return true;
}

int main() {
    // ---- kind and depth
    CHECK(LFX_LZ77_LAZY == 3 && LFX_LZ77_LAZY_DEPTH(8) == (3 | 8 << 8));
    for (int k = 1; k <= 255; k++) {
        const lfx_encode_opts o = with_kind(LFX_LZ77_LAZY_DEPTH(k));
        const Resolved r = resolve(LFX_ZLIB, o);
        CHECK(r.rc == LFX_OK && lz77_kind_of(o) == LFX_LZ77_LAZY && r.sp.chain_depth == (uint32_t)k && r.sp.lazy);
        CHECK(r.sp.plan.lz77_kind == 3);                                    // the plan sees the kind without the depth
    }
    CHECK(resolve(LFX_ZLIB, with_kind(LFX_LZ77_LAZY)).rc == LFX_E_ARG);               // depth 0: there is no default depth
    CHECK(resolve(LFX_ZLIB, with_kind(LFX_LZ77_LAZY_DEPTH(256))).rc == LFX_E_ARG);    // bit 16
    for (int bit = 16; bit < 32; bit++) CHECK(resolve(LFX_ZLIB, with_kind((int32_t)((uint32_t)LFX_LZ77_LAZY_DEPTH(8) | 1u << bit))).rc == LFX_E_ARG);
    // the kinds 0, 1 and 2 answer as before
    for (int kind = 0; kind <= 1; kind++) {
        const lfx_encode_opts o = with_kind(kind | 0x1200);
        const Resolved r = resolve(LFX_GZIP, o);
        CHECK(r.rc == LFX_OK && lz77_kind_of(o) == kind && r.sp.chain_depth == 0 && !r.sp.lazy && r.sp.plan.lz77_kind == kind);
    }
    for (int k = 1; k <= 255; k++) {
        const lfx_encode_opts o = with_kind(LFX_LZ77_CHAIN_DEPTH(k));
        const Resolved r = resolve(LFX_ZLIB, o);
        CHECK(r.rc == LFX_OK && lz77_kind_of(o) == LFX_LZ77_CHAIN && r.sp.chain_depth == (uint32_t)k && !r.sp.lazy);
        CHECK(r.sp.plan.lz77_kind == 2);
    }
    CHECK(resolve(LFX_ZLIB, with_kind(LFX_LZ77_CHAIN)).rc == LFX_E_ARG);
    for (int bit = 16; bit < 32; bit++) CHECK(resolve(LFX_ZLIB, with_kind((int32_t)((uint32_t)LFX_LZ77_CHAIN_DEPTH(8) | 1u << bit))).rc == LFX_E_ARG);
    CHECK(lz77_chained(2) && lz77_chained(3) && !lz77_chained(0) && !lz77_chained(1) && !lz77_chained(4));

    // ---- the container headers: Best unless the caller names a level; no_compression resets it
    auto flevel = [](const lfx_encode_opts &o) { std::vector<uint8_t> h; CHECK(container_header(LFX_ZLIB, o, h) == LFX_OK && h.size() == 2 && ((h[0] << 8) + h[1]) % 31 == 0); return h[1] >> 6; };
    auto xfl = [](const lfx_encode_opts &o) { std::vector<uint8_t> h; CHECK(container_header(LFX_GZIP, o, h) == LFX_OK && h.size() == 10); return (int)h[8]; };
    lfx_encode_opts o = with_kind(LFX_LZ77_LAZY_DEPTH(8));
    CHECK(flevel(o) == 3 && xfl(o) == 2);
    o.lz77_level = 1 + LFX_LEVEL_FAST;
    CHECK(flevel(o) == 1 && xfl(o) == 4);
    o.lz77_level = 1 + LFX_LEVEL_BALANCE;
    CHECK(flevel(o) == 2 && xfl(o) == 0);
    o.lz77_level = 0;
    o.no_compression = 1;
    CHECK(flevel(o) == 0 && xfl(o) == 0);
    CHECK(flevel(with_kind(0)) == 2 && xfl(with_kind(0)) == 0 && flevel(with_kind(1)) == 0 && xfl(with_kind(1)) == 0);   // as before
    CHECK(flevel(with_kind(LFX_LZ77_CHAIN_DEPTH(8))) == 3 && xfl(with_kind(LFX_LZ77_CHAIN_DEPTH(8))) == 2);

    // ---- the plan: kind 3 buffers and flushes as kind 0 does, over random schedules (write and write_repeat)
    std::mt19937_64 rng(20);
    int plans = 0;
    for (int it = 0; it < 2000; it++) {
        PlanOpts p0, p3;
        p0.window_size = p3.window_size = 1u << (8 + rng() % 8);
        p0.block_size = p3.block_size = 1 + rng() % (1u << (10 + rng() % 11));
        p0.dynamic_huffman = p3.dynamic_huffman = rng() & 1;
        p0.lz77_kind = 0;
        p3.lz77_kind = 3;
        Planner a(p0), b(p3), c(p3);
        const int events = 1 + (int)(rng() % 12);
        for (int e = 0; e < events; e++) {
            const uint64_t w = rng() % 3 == 0 ? rng() % 9 : rng() % (1u << (4 + rng() % 16)), cnt = 1 + rng() % 40;
            if (rng() % 7 == 0) { a.flush(); b.flush(); c.flush(); continue; }
            a.write_repeat(w, cnt);
            b.write_repeat(w, cnt);
            for (uint64_t q = 0; q < cnt; q++) c.write(w);
        }
        const Plan &pa = a.finish(), &pb = b.finish(), &pc = c.finish();
        CHECK(same_plan(pa, pb) && same_plan(pb, pc));
        for (const ChunkDesc &ch : pb.chunks) CHECK(!(ch.flags & CH_LITERALS));
        plans++;
    }

    // ---- the demote kernel's cut of its items, replayed: chunks at any phase of the grid, stale lengths and candidates between
    //      and behind them; the items' spans tile each chunk's visited range, the wide part is aligned and inside it, and what
    //      the spans demote is the rule — nothing else is touched, nothing outside [in_off, in_off + end] is read
    int spans = 0;
    for (int it = 0; it < 3000; it++) {
        const uint32_t tile = it % 2 ? 64 : 48;                               // (small tiles: many seams; any multiple of 16 or not)
        std::vector<ChunkDesc> chunks(1 + rng() % 5);
        uint64_t at = rng() % 40;
        for (ChunkDesc &ch : chunks) {
            ch = ChunkDesc{};
            ch.in_off = at;
            ch.len = rng() % 4 == 0 ? rng() % 8 : rng() % 300;
            ch.flags = rng() % 8 == 0 ? CH_LITERALS : 0;
            at += ch.len + (rng() % 3 ? 0 : rng() % 21);                      // back to back, or a gap (a batch)
        }
        const uint64_t total = at + 64;
        std::vector<uint8_t> len(total), touched(total, 0), readable(total, 0);
        std::vector<uint16_t> cd2(total), want(total);
        for (uint64_t g = 0; g < total; g++) { len[g] = rng() % 3 ? (uint8_t)(rng() % 4) : (uint8_t)(253 + rng() % 3); cd2[g] = (uint16_t)(1 + rng() % 5); }
        want = cd2;
        for (const ChunkDesc &ch : chunks) {
            if ((ch.flags & CH_LITERALS) || ch.len <= 3) continue;
            const uint64_t end = ch.len - 3;
            for (uint64_t p = 0; p < end; p++) {
                readable[ch.in_off + p] = 1;
                if (p + 1 < end && len[ch.in_off + p + 1] > len[ch.in_off + p]) want[ch.in_off + p] = 0;
            }
        }
        std::vector<ChainItem> items;
        chain_items(chunks, tile, items);
        auto one = [&](uint64_t g, uint64_t gend) {                           // the kernel's step at one position
            CHECK(!touched[g]++ && readable[g]);
            if (g + 1 < gend) { CHECK(readable[g + 1]); if (len[g + 1] > len[g]) cd2[g] = 0; }
        };
        for (const ChainItem &item : items) {
            const ChunkDesc &ch = chunks[item.chunk];
            const DemoteSpan s = demote_span(ch.in_off, ch.len, item.p0, tile);
            CHECK(s.g0 == ch.in_off + item.p0 && s.g0 < s.g1 && s.g1 <= s.gend && s.gend == ch.in_off + ch.len - 3);
            CHECK(s.g0 <= s.a && s.a <= s.b && s.b <= s.g1);
            CHECK(s.a - s.g0 < 32 && s.g1 - s.b < 16);                        // the lanes the kernel gives the edges
            if (s.a < s.b) CHECK(s.a - s.g0 < 16 && s.a % DEMOTE_GROUP == 0 && s.b % DEMOTE_GROUP == 0);
            else CHECK(s.a == s.g1);                                          // no whole group: everything by hand
            for (uint64_t g = s.g0; g < s.a; g++) one(g, s.gend);
            for (uint64_t g = s.a; g < s.b; g += DEMOTE_GROUP)
                for (uint64_t k = 0; k < DEMOTE_GROUP; k++) one(g + k, s.gend);
            for (uint64_t g = s.b; g < s.g1; g++) one(g, s.gend);
            spans++;
        }
        for (uint64_t g = 0; g < total; g++) CHECK(touched[g] == readable[g] && cd2[g] == want[g]);
    }
    // past the end of a chunk, and a chunk without a visited range: an empty span
    CHECK(demote_span(5, 100, 97, 16).g0 == demote_span(5, 100, 97, 16).g1);
    CHECK(demote_span(5, 2, 0, 16).g0 == demote_span(5, 2, 0, 16).g1);
    printf("lazy_opts ok: %d plans, %d spans\n", plans, spans);
    return 0;
}
