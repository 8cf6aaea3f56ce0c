// level_opts.cpp — the host-only parts of LevelLz77Encoder (LFX_LZ77_LEVEL) under a plain host compiler: how
// lz77_kind is decoded and checked for kind 4 (lfx_enc_frame.h), the level table field by field against include/lfx.h's,
// written out here by hand, what the container headers say, that the planner cuts a kind-4 schedule as it cuts a kind-3 one
// (lfx_plan.h), every cell of encode_served for kind 4, and the demote rule with max_lazy in the bytes of the length array.
// The kinds 0..3 answer as before.  No HIP, no device.
//   g++ -O2 -std=c++17 -Wall [-fsanitize=address,undefined] -o level_opts tests/c/level_opts.cpp && ./level_opts
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../libflate_amd/csrc/lfx_chain.h"
#include "../../libflate_amd/csrc/lfx_enc_frame.h"

using namespace lfx;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "level_opts: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static lfx_encode_opts with_kind(int32_t kind) {
    lfx_encode_opts o;
    encode_opts_default(&o);
    o.lz77_kind = kind;
    return o;
}
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

// include/lfx.h's table, by hand: level → depth, lazy, nice, max_lazy, too_far (0: the rule does not apply)
static const uint32_t TABLE[10][5] = {{0, 0, 0, 0, 0},        {4, 0, 8, 0, 0},        {8, 0, 16, 0, 0},          {32, 0, 32, 0, 0},
                                      {16, 1, 16, 4, 4096},   {32, 1, 32, 16, 4096},  {128, 1, 128, 16, 4096},   {256, 1, 128, 32, 4096},
                                      {1024, 1, 258, 128, 4096}, {4096, 1, 258, 258, 4096}};

int main() {
    // ---- the constant, the level in bits 8..15, the table
    CHECK(LFX_LZ77_LEVEL == 4 && LFX_LZ77_LEVEL_N(6) == (4 | 6 << 8) && LFX_LZ77_LAZY == 3 && LFX_LZ77_CHAIN == 2);
    for (int n = 1; n <= 9; n++) {
        const lfx_encode_opts o = with_kind(LFX_LZ77_LEVEL_N(n));
        const Resolved r = resolve(LFX_ZLIB, o);
        CHECK(r.rc == LFX_OK && lz77_kind_of(o) == LFX_LZ77_LEVEL && r.sp.tuned && r.sp.plan.lz77_kind == 4);
        CHECK(r.sp.chain_depth == TABLE[n][0] && r.sp.tune.depth == TABLE[n][0]);
        CHECK(r.sp.lazy == (TABLE[n][1] != 0) && r.sp.tune.lazy == r.sp.lazy);
        CHECK(r.sp.tune.nice == TABLE[n][2]);
        if (r.sp.lazy) CHECK(r.sp.tune.max_lazy == TABLE[n][3] && r.sp.tune.too_far == TABLE[n][4]);
        else CHECK(r.sp.tune.max_lazy == LEVEL_NEVER && r.sp.tune.too_far == LEVEL_NEVER);      // no position kept for its length, no match dropped
        CHECK(r.sp.tune.nice >= 3 && r.sp.tune.nice <= MAX_LENGTH && r.sp.chain_depth >= 1);
        CHECK(!r.sp.auto_blocks);
    }
    // outside the domain
    CHECK(resolve(LFX_ZLIB, with_kind(LFX_LZ77_LEVEL)).rc == LFX_E_ARG);                   // level 0: there is no default level
    for (int n = 10; n <= 255; n++) CHECK(resolve(LFX_ZLIB, with_kind(LFX_LZ77_LEVEL_N(n))).rc == LFX_E_ARG);
    for (int bit = 16; bit < 32; bit++) CHECK(resolve(LFX_GZIP, with_kind((int32_t)((uint32_t)LFX_LZ77_LEVEL_N(6) | 1u << bit))).rc == LFX_E_ARG);
    {
        lfx_encode_opts o = with_kind(LFX_LZ77_LEVEL_N(6));
        o.block_size = 0;
        CHECK(resolve(LFX_ZLIB, o).rc == LFX_E_ARG);
        o = with_kind(LFX_LZ77_LEVEL_N(6));
        o.max_length = 2;
        CHECK(resolve(LFX_ZLIB, o).rc == LFX_E_ARG);
        o.max_length = 1000;
        o.window_size = 1u << 20;
        const Resolved r = resolve(LFX_ZLIB, o);
        CHECK(r.rc == LFX_OK && r.sp.plan.max_length == 258 && r.sp.plan.window_size == 32768);
    }
    // the kinds 0..3 answer as before: no tuning
    for (int32_t kw : {0, 1, 0 | 0x1200, LFX_LZ77_CHAIN_DEPTH(8), LFX_LZ77_LAZY_DEPTH(255)}) {
        const Resolved r = resolve(LFX_ZLIB, with_kind(kw));
        const int kind = kw & 0xFF;
        CHECK(r.rc == LFX_OK && !r.sp.tuned && r.sp.tune.depth == 0 && r.sp.tune.nice == 0 && r.sp.tune.max_lazy == 0 && r.sp.tune.too_far == 0);
        CHECK(r.sp.chain_depth == (kind >= 2 ? (uint32_t)kw >> 8 : 0u) && r.sp.lazy == (kind == 3));
    }
    CHECK(lz77_chain_stage(2) && lz77_chain_stage(3) && lz77_chain_stage(4) && !lz77_chain_stage(0) && !lz77_chain_stage(1) && !lz77_chain_stage(5));
    CHECK(level_tune(0).depth == 0 && level_tune(10).depth == 0 && level_tune(0xFFFFFFFFu).depth == 0);

    // ---- the container headers: Fast, Balance, Best by the level unless the caller names one; no_compression resets it
    auto flevel = [](const lfx_encode_opts &o) { std::vector<uint8_t> h; CHECK(container_header(LFX_ZLIB, o, h) == LFX_OK && h.size() == 2 && ((h[0] << 8) + h[1]) % 31 == 0); return h[1] >> 6; };
    auto xfl = [](const lfx_encode_opts &o) { std::vector<uint8_t> h; CHECK(container_header(LFX_GZIP, o, h) == LFX_OK && h.size() == 10); return (int)h[8]; };
    for (int n = 1; n <= 9; n++) {
        lfx_encode_opts o = with_kind(LFX_LZ77_LEVEL_N(n));
        const int want = n <= 3 ? LFX_LEVEL_FAST : n <= 6 ? LFX_LEVEL_BALANCE : LFX_LEVEL_BEST;
        CHECK(lz77_level_of(o) == 1 + want && flevel(o) == want && xfl(o) == (want == LFX_LEVEL_FAST ? 4 : want == LFX_LEVEL_BEST ? 2 : 0));
        o.lz77_level = 1 + LFX_LEVEL_BEST;
        CHECK(flevel(o) == 3 && xfl(o) == 2);
        o.lz77_level = 1 + LFX_LEVEL_FAST;
        CHECK(flevel(o) == 1 && xfl(o) == 4);
        o.lz77_level = 0;
        o.no_compression = 1;
        CHECK(lz77_level_of(o) == 0 && flevel(o) == 0 && xfl(o) == 0);
        std::vector<uint8_t> d;
        CHECK(container_header(LFX_DEFLATE, o, d) == LFX_OK && d.empty());
    }
    CHECK(flevel(with_kind(0)) == 2 && xfl(with_kind(0)) == 0 && flevel(with_kind(LFX_LZ77_LAZY_DEPTH(8))) == 3 && xfl(with_kind(LFX_LZ77_CHAIN_DEPTH(8))) == 2);

    // ---- the plan: kind 4 buffers and flushes as kind 3 does, over random schedules
    std::mt19937_64 rng(23);
    int plans = 0;
    for (int it = 0; it < 2000; it++) {
        PlanOpts p3, p4;
        p3.window_size = p4.window_size = 1u << (8 + rng() % 8);
        p3.block_size = p4.block_size = 1 + rng() % (1u << (10 + rng() % 11));
        p3.dynamic_huffman = p4.dynamic_huffman = rng() & 1;
        p3.lz77_kind = 3;
        p4.lz77_kind = 4;
        Planner a(p3), b(p4), c(p4);
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

    // ---- encode_served: every cell of kind 4 — the cells of the kinds 2 and 3, with its own name in the messages
    static const EncodeEntry ENTRIES[9] = {ENC_DEVICE, ENC_BATCH, ENC_DICT_DEVICE, ENC_DICT_BATCH, ENC_STREAM, ENC_MEMBERS, ENC_INDEX, ENC_SHARD, ENC_LZ77};
    static const DictKind DICTS[3] = {DICT_NONE, DICT_PLAIN, DICT_CHAIN};
    int cells = 0, refused = 0;
    for (int n : {1, 3, 4, 6, 9})
        for (int32_t huffman = 0; huffman <= 2; huffman++)
            for (int32_t nc = 0; nc <= 1; nc++) {
                lfx_encode_opts o = with_kind(LFX_LZ77_LEVEL_N(n)), o3 = with_kind(LFX_LZ77_LAZY_DEPTH(8));
                o.dynamic_huffman = o3.dynamic_huffman = huffman;
                o.no_compression = o3.no_compression = nc;
                const Resolved r = resolve(LFX_ZLIB, o), r3 = resolve(LFX_ZLIB, o3);
                CHECK(r.rc == LFX_OK && r3.rc == LFX_OK);
                const bool aut = huffman == 2 && !nc;
                for (EncodeEntry e : ENTRIES)
                    for (DictKind dict : DICTS) {
                        const char *want = nullptr;
                        if (e == ENC_SHARD && nc) want = "sharded encode of stored blocks is not supported (their size depends on the bit phase)";
                        else if (e == ENC_SHARD) want = "lz77_kind: the N-GPU encode does not serve LFX_LZ77_LEVEL";
                        else if (e == ENC_INDEX && aut) want = "dynamic_huffman: lfx_encode_index_device does not serve LFX_HUFFMAN_AUTO (the candidates are laid out from the host plan's block types)";
                        else if (dict == DICT_PLAIN) want = "lz77_kind: LFX_LZ77_LEVEL with a preset dictionary is not supported (a dictionary made by lfx_dict_new_chain serves it)";
                        const char *why = nullptr, *why3 = nullptr;
                        const int rc = encode_served(e, r.sp, dict, &why), rc3 = encode_served(e, r3.sp, dict, &why3);
                        if (want) { CHECK(rc == LFX_E_UNSUPPORTED && why && strcmp(why, want) == 0); refused++; }
                        else CHECK(rc == LFX_OK && why == nullptr);
                        CHECK(rc == rc3 && (why == nullptr) == (why3 == nullptr));        // the same cells as kind 3
                        if (why3) CHECK(!strstr(why3, "LFX_LZ77_LEVEL"));
                        cells++;
                    }
            }
    // of the 30 option sets: shard refuses all 30 under each dictionary (90); index 5 (AUTO) under each (15) and 25 more under a
    // plain one; each of the other seven all 30 under a plain one (210)
    CHECK(cells == 5 * 3 * 2 * 9 * 3 && refused == 90 + 15 + 25 + 210);

    // ---- the demotion with max_lazy in the bytes of the length array (lfx_chain.hip: l = L - 3, zb = Z - 3; "none" and L = 3
    //      share the 0): for every level's Z and every pair of lengths, the byte rule is the contract's
    int pairs = 0;
    for (int n = 4; n <= 9; n++) {
        const uint32_t Z = level_tune(n).max_lazy, zb = Z > 3 ? Z - 3 : 0u;
        for (uint32_t L = 0; L <= 258; L = L ? L + 1 : 3)
            for (uint32_t Ln = 0; Ln <= 258; Ln = Ln ? Ln + 1 : 3) {
                const uint32_t l = L ? L - 3 : 0, ln = Ln ? Ln - 3 : 0;
                const bool demoted = ln > l && l < zb;                        // the kernel's test
                const bool pointer = L != 0 && (L >= Z || Ln <= L);           // the contract's
                if (L != 0) CHECK(demoted == !pointer);                       // (L == 0: no candidate, cd2 is 0 whatever the kernel does)
                pairs++;
            }
    }
    printf("level_opts ok: %d plans, %d cells, %d pairs\n", plans, cells, pairs);
    return 0;
}
