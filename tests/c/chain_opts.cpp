// chain_opts.cpp — the host-only parts of ChainLz77Encoder (LFX_LZ77_CHAIN) under a plain host compiler: how
// lz77_kind is decoded and checked (lfx_enc_frame.h), what the container headers say, that the planner buffers kind 2 as it
// buffers kind 0 (lfx_plan.h), and the chain kernel's work list (lfx_chain.h).  No HIP, no device.
//   g++ -O2 -std=c++17 -Wall [-fsanitize=address,undefined] -o chain_opts tests/c/chain_opts.cpp && ./chain_opts
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../libflate_amd/csrc/lfx_chain.h"
#include "../../libflate_amd/csrc/lfx_enc_frame.h"

using namespace lfx;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "chain_opts: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

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
    CHECK(LFX_LZ77_CHAIN == 2 && LFX_LZ77_CHAIN_DEPTH(8) == (2 | 8 << 8));
    for (int k = 1; k <= 255; k++) {
        const lfx_encode_opts o = with_kind(LFX_LZ77_CHAIN_DEPTH(k));
        const Resolved r = resolve(LFX_ZLIB, o);
        CHECK(r.rc == LFX_OK && lz77_kind_of(o) == LFX_LZ77_CHAIN && r.sp.chain_depth == (uint32_t)k);
        CHECK(r.sp.plan.lz77_kind == 2);                                    // the plan sees the kind without the depth
    }
    CHECK(resolve(LFX_ZLIB, with_kind(LFX_LZ77_CHAIN)).rc == LFX_E_ARG);              // depth 0: there is no default depth
    CHECK(resolve(LFX_ZLIB, with_kind(LFX_LZ77_CHAIN_DEPTH(256))).rc == LFX_E_ARG);   // bit 16
    for (int bit = 16; bit < 32; bit++) CHECK(resolve(LFX_ZLIB, with_kind((int32_t)((uint32_t)LFX_LZ77_CHAIN_DEPTH(8) | 1u << bit))).rc == LFX_E_ARG);
    // the kinds 0 and 1: the bits above bit 7 are not read
    for (int kind = 0; kind <= 1; kind++) {
        const lfx_encode_opts o = with_kind(kind | 0x1200);
        const Resolved r = resolve(LFX_GZIP, o);
        CHECK(r.rc == LFX_OK && lz77_kind_of(o) == kind && r.sp.chain_depth == 0 && r.sp.plan.lz77_kind == kind);
    }
    CHECK(resolve(LFX_ZLIB, with_kind(0)).rc == LFX_OK && resolve(LFX_ZLIB, with_kind(1)).rc == LFX_OK && resolve(LFX_ZLIB, with_kind(0)).sp.chain_depth == 0);

    // ---- the container headers: Best unless the caller names a level; no_compression resets it
    auto flevel = [](const lfx_encode_opts &o) { std::vector<uint8_t> h; CHECK(container_header(LFX_ZLIB, o, h) == LFX_OK && h.size() == 2 && ((h[0] << 8) + h[1]) % 31 == 0); return h[1] >> 6; };
    auto xfl = [](const lfx_encode_opts &o) { std::vector<uint8_t> h; CHECK(container_header(LFX_GZIP, o, h) == LFX_OK && h.size() == 10); return (int)h[8]; };
    lfx_encode_opts o = with_kind(LFX_LZ77_CHAIN_DEPTH(8));
    CHECK(flevel(o) == 3 && xfl(o) == 2);
    o.lz77_level = 1 + LFX_LEVEL_FAST;
    CHECK(flevel(o) == 1 && xfl(o) == 4);
    o.lz77_level = 1 + LFX_LEVEL_BALANCE;
    CHECK(flevel(o) == 2 && xfl(o) == 0);
    o.lz77_level = 0;
    o.no_compression = 1;
    CHECK(flevel(o) == 0 && xfl(o) == 0);
    CHECK(flevel(with_kind(0)) == 2 && xfl(with_kind(0)) == 0 && flevel(with_kind(1)) == 0 && xfl(with_kind(1)) == 0);   // as before

    // ---- the plan: kind 2 buffers and flushes as kind 0 does, over random schedules (write and write_repeat)
    std::mt19937_64 rng(19);
    int plans = 0;
    for (int it = 0; it < 2000; it++) {
        PlanOpts p0, p2;
        p0.window_size = p2.window_size = 1u << (8 + rng() % 8);
        p0.block_size = p2.block_size = 1 + rng() % (1u << (10 + rng() % 11));
        p0.dynamic_huffman = p2.dynamic_huffman = rng() & 1;
        p0.lz77_kind = 0;
        p2.lz77_kind = 2;
        Planner a(p0), b(p2), c(p2);
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

    // ---- the work list: the visited range of every parsed chunk, tiled once, in order
    int lists = 0;
    for (int it = 0; it < 2000; it++) {
        std::vector<ChunkDesc> chunks(1 + rng() % 9);
        bool all_small = true;
        for (ChunkDesc &ch : chunks) {
            ch = ChunkDesc{};
            ch.len = rng() % 5 == 0 ? rng() % 8 : rng() % 3 == 0 ? CHAIN_TILE_SMALL - 2 + rng() % 5 : rng() % (6 * CHAIN_TILE);
            ch.flags = rng() % 6 == 0 ? CH_LITERALS : 0;
            if (!(ch.flags & CH_LITERALS) && ch.len > CHAIN_TILE_SMALL) all_small = false;
        }
        CHECK(chain_small(chunks) == all_small);
        const uint32_t tile = all_small ? CHAIN_TILE_SMALL : CHAIN_TILE;
        std::vector<ChainItem> items;
        chain_items(chunks, tile, items);
        size_t at = 0;
        for (uint32_t ci = 0; ci < chunks.size(); ci++) {
            const ChunkDesc &ch = chunks[ci];
            const uint64_t end = (ch.len > 3 ? ch.len : 3) - 3;
            if (ch.flags & CH_LITERALS) continue;
            for (uint64_t p0 = 0; p0 < end; p0 += tile, at++) CHECK(at < items.size() && items[at].chunk == ci && items[at].p0 == p0);
            if (all_small) CHECK(end <= tile);                                // one item at most, no window in front of it
        }
        CHECK(at == items.size());
        lists++;
    }
    printf("chain_opts ok: %d plans, %d lists\n", plans, lists);
    return 0;
}
