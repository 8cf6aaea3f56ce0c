// block_merge.cpp — the host-only parts of block_merge (include/lfx.h) under a plain host compiler: the field in
// lfx_encode_opts and its domain (lfx_enc_frame.h), every cell of the served/refused table, the region layout (merge_regions,
// lfx_merge.h) over seeded plans against a plain loop, and the merge tree the kernel runs (merge_tree, lfx_merge_tree.h, over
// lfx_huff.h's host build) against the rule written out as a recursion.  No HIP, no device.
//   g++ -O2 -std=c++17 -Wall [-fsanitize=address,undefined] -o block_merge tests/c/block_merge.cpp && ./block_merge
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../libflate_amd/csrc/lfx_enc_frame.h"
#include "../../libflate_amd/csrc/lfx_merge_tree.h"

using namespace lfx;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "block_merge: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static lfx_encode_opts options(uint32_t merge, int32_t huffman = 1, int32_t no_compression = 0, int32_t kind = 0) {
    lfx_encode_opts o;
    encode_opts_default(&o);
    o.block_merge = merge;
    o.dynamic_huffman = huffman;
    o.no_compression = no_compression;
    o.lz77_kind = kind;
    return o;
}

// ---- the rule, as the contract words it: → (whole, D) of the node [lo, lo + span) ∩ [0, n), lo < n
static HuffScratch g_S;
static BlockCodes g_bc;
static uint64_t size_of(const std::vector<std::vector<uint32_t>> &rows, uint32_t lo, uint32_t hi) {
    uint32_t sum[SYM_ROW] = {};
    for (uint32_t q = lo; q < hi; q++)
        for (uint32_t i = 0; i < SYM_ROW; i++) sum[i] += rows[q][i];
    sum[256] = 1;
    huff_block_build(sum, BT_DYNAMIC, &g_bc, g_S, 0, 1);
    return g_bc.body_bits;
}
struct Node { bool whole; uint64_t d; };
static Node rule(const std::vector<std::vector<uint32_t>> &rows, uint32_t n, uint32_t lo, uint32_t span, std::vector<uint32_t> &head) {
    if (span == 1) return Node{true, size_of(rows, lo, lo + 1)};
    const uint32_t half = span / 2;
    const Node l = rule(rows, n, lo, half, head);
    if (lo + half >= n) return l;
    const Node r = rule(rows, n, lo + half, half, head);
    const uint32_t hi = lo + span < n ? lo + span : n;
    if (l.whole && r.whole) {
        const uint64_t d = size_of(rows, lo, hi);
        if (d <= l.d + r.d) {
            for (uint32_t i = lo; i < hi; i++) head[i] = lo;
            return Node{true, d};
        }
    }
    return Node{false, 0};
}

int main() {
    // ---- the field: in what was padding, the layout is unchanged
    CHECK(sizeof(lfx_encode_opts) == 72 && offsetof(lfx_encode_opts, block_merge) == 52 && offsetof(lfx_encode_opts, extra_len) == 48 &&
          offsetof(lfx_encode_opts, filename) == 56 && LFX_MERGE_MAX == 16 && MERGE_MAX == LFX_MERGE_MAX && (1u << MERGE_LEVELS) == MERGE_MAX);
    {
        lfx_encode_opts o;
        memset(&o, 0xFF, sizeof o);
        encode_opts_default(&o);
        CHECK(o.block_merge == 0);
        EncodeSpec sp;
        CHECK(encode_spec(LFX_ZLIB, nullptr, &sp) == LFX_OK && !sp.merge_blocks && sp.o.block_merge == 0 && !EncodeSpec().merge_blocks);
    }
    // ---- the domain: 0 and 1; no effect under no_compression or fixed codes; the plan never sees it
    for (uint32_t v : {0u, 1u, 2u, 3u, 0x80000000u, 0xFFFFFFFFu})
        for (int32_t huffman : {0, 1, 2, 3})
            for (int32_t nc : {0, 1}) {
                EncodeSpec sp, s0;
                const lfx_encode_opts o = options(v, huffman, nc), o0 = options(0, huffman, nc);
                CHECK(encode_spec(LFX_ZLIB, &o, &sp) == (v <= 1 ? LFX_OK : LFX_E_ARG));
                CHECK(sp.merge_blocks == (v == 1 && huffman != 0 && !nc));
                CHECK(encode_spec(LFX_ZLIB, &o0, &s0) == LFX_OK);
                const PlanOpts &p = sp.plan, &q = s0.plan;
                CHECK(p.block_size == q.block_size && p.dynamic_huffman == q.dynamic_huffman && p.no_compression == q.no_compression &&
                      p.lz77_kind == q.lz77_kind && p.window_size == q.window_size && p.max_length == q.max_length &&
                      p.zlib_sync == q.zlib_sync && sp.auto_blocks == s0.auto_blocks);
                std::vector<uint8_t> h1, h0;
                CHECK(container_header(LFX_GZIP, sp.o, h1) == LFX_OK && container_header(LFX_GZIP, s0.o, h0) == LFX_OK && h1 == h0);
            }
    // ---- served and refused: every entry point, merge on and off, the kinds, AUTO, the dictionaries
    int cells = 0, refused = 0;
    const EncodeEntry entries[9] = {ENC_DEVICE, ENC_BATCH, ENC_DICT_DEVICE, ENC_DICT_BATCH, ENC_STREAM, ENC_MEMBERS, ENC_INDEX, ENC_SHARD, ENC_LZ77};
    const int32_t kinds[5] = {LFX_LZ77_DEFAULT, LFX_LZ77_NOCOMPRESSION, LFX_LZ77_CHAIN_DEPTH(8), LFX_LZ77_LAZY_DEPTH(8), LFX_LZ77_LEVEL_N(6)};
    for (EncodeEntry e : entries)
        for (int32_t kind : kinds)
            for (int32_t huffman : {1, 2})
                for (DictKind dict : {DICT_NONE, DICT_PLAIN, DICT_CHAIN}) {
                    EncodeSpec on, off;
                    const lfx_encode_opts o1 = options(1, huffman, 0, kind), o0 = options(0, huffman, 0, kind);
                    CHECK(encode_spec(LFX_ZLIB, &o1, &on) == LFX_OK && encode_spec(LFX_ZLIB, &o0, &off) == LFX_OK && on.merge_blocks);
                    const char *why1 = nullptr, *why0 = nullptr;
                    const int rc1 = encode_served(e, on, dict, &why1), rc0 = encode_served(e, off, dict, &why0);
                    const bool own = e == ENC_STREAM || e == ENC_MEMBERS || e == ENC_INDEX || e == ENC_SHARD;
                    if (rc0 != LFX_OK) {
                        // refused for another reason already: that reason stands (the first row wins) unless block_merge's comes first
                        CHECK(rc1 == LFX_E_UNSUPPORTED && why1);
                    } else if (own) {
                        CHECK(rc1 == LFX_E_UNSUPPORTED && why1 && strncmp(why1, "block_merge: ", 13) == 0);
                        CHECK(strstr(why1, e == ENC_STREAM ? "stream encoder" : e == ENC_MEMBERS ? "lfx_encode_members_*"
                                               : e == ENC_INDEX ? "lfx_encode_index_device" : "N-GPU encode"));
                        refused++;
                    } else {
                        CHECK(rc1 == LFX_OK && !why1);      // device, batch, dictionary calls, the lz77 plug-in: served
                    }
                    cells++;
                }
    CHECK(cells == 9 * 5 * 2 * 3 && refused > 0);
    {
        // under no_compression or fixed codes there is nothing to refuse
        for (EncodeEntry e : {ENC_STREAM, ENC_MEMBERS, ENC_INDEX}) {
            EncodeSpec sp;
            const char *why = nullptr;
            const lfx_encode_opts of = options(1, 0, 0), on = options(1, 1, 1);
            CHECK(encode_spec(LFX_GZIP, &of, &sp) == LFX_OK && encode_served(e, sp, DICT_NONE, &why) == LFX_OK && !why);
            CHECK(encode_spec(LFX_GZIP, &on, &sp) == LFX_OK && encode_served(e, sp, DICT_NONE, &why) == LFX_OK && !why);
        }
    }

    // ---- the region layout over seeded plans (streams appended as a batch does) against a plain loop over the candidates
    std::mt19937_64 rng(24);
    int plans = 0, regions = 0;
    for (int it = 0; it < 2000; it++) {
        const int32_t huffman = rng() % 8 == 0 ? 0 : 1, nc = rng() % 16 == 0;     // (one draw per statement: the order is the source's)
        lfx_encode_opts o = options(1, huffman, nc);
        const uint32_t bits = 8 + (uint32_t)(rng() % 8);
        o.block_size = 1 + rng() % (1u << bits);
        o.zlib_flush_mode = rng() % 2 ? LFX_FLUSH_SYNC : LFX_FLUSH_NONE;
        EncodeSpec sp;
        CHECK(encode_spec(LFX_ZLIB, &o, &sp) == LFX_OK);
        Plan plan;
        std::vector<uint32_t> stream_of;
        const int streams = 1 + (int)(rng() % 4);
        uint64_t off = 0;
        for (int s = 0; s < streams; s++) {
            Planner pl(sp.plan);
            const int events = 1 + (int)(rng() % 40);
            for (int e = 0; e < events; e++) {
                if (rng() % 9 == 0) pl.flush();
                else {
                    const uint32_t wbits = 4 + (uint32_t)(rng() % 12);
                    const uint64_t w = rng() % (1u << wbits);
                    pl.write_repeat(w, 1 + rng() % 6);
                }
            }
            const uint64_t bytes = pl.cursor();
            const Plan &p = pl.finish();
            plan.append(p, off);
            stream_of.insert(stream_of.end(), p.blocks.size(), (uint32_t)s);
            off += bytes;
        }
        std::vector<MergeRegion> got, want;
        merge_regions(plan.blocks, got);
        // the plain loop: number the candidates of every run; a region starts at every candidate whose number is a multiple of 16
        uint32_t k = 0;
        for (size_t b = 0; b < plan.blocks.size(); b++) {
            const bool cand = plan.blocks[b].type == BT_DYNAMIC;
            const bool joins = cand && b > 0 && plan.blocks[b - 1].type == BT_DYNAMIC && stream_of[b - 1] == stream_of[b];
            k = joins ? k + 1 : 0;
            if (!cand) continue;
            if (k % MERGE_MAX == 0) want.push_back(MergeRegion{(uint32_t)b, 1});
            else want.back().n++;
        }
        size_t w = 0;
        for (const MergeRegion &r : want) {
            if (r.n < 2) continue;                       // (a region of one candidate is left out)
            CHECK(w < got.size() && got[w].first_block == r.first_block && got[w].n == r.n);
            w++;
        }
        CHECK(w == got.size());
        for (const MergeRegion &r : got) {
            CHECK(r.n >= 2 && r.n <= MERGE_MAX && (size_t)r.first_block + r.n <= plan.blocks.size());
            // consecutive candidates of one stream, with consecutive chunks: a merged block's chunks lie back to back
            for (uint32_t q = 0; q < r.n; q++) {
                const BlockDesc &bd = plan.blocks[r.first_block + q];
                CHECK(bd.type == BT_DYNAMIC && stream_of[r.first_block + q] == stream_of[r.first_block] && bd.n_chunks >= 1);
                if (q) CHECK(bd.first_chunk == plan.blocks[r.first_block + q - 1].first_chunk + plan.blocks[r.first_block + q - 1].n_chunks);
                if (q + 1 < r.n) CHECK(!bd.final);
            }
        }
        plans++;
        regions += (int)got.size();
    }

    // ---- the merge tree over seeded symbol counts against the rule
    static MergeScratch M;
    int trees = 0, merged = 0, cut = 0;
    for (int it = 0; it < 300; it++) {
        const uint32_t n = it < 16 ? (uint32_t)it + 1 : 1 + (uint32_t)(rng() % MERGE_MAX);
        // candidates in stretches of one "alphabet" each: neighbours of one stretch merge, stretches mostly do not
        std::vector<std::vector<uint32_t>> rows(n, std::vector<uint32_t>(SYM_ROW, 0));
        uint32_t base = 0, spread = 1, dists = 0;
        for (uint32_t q = 0; q < n; q++) {
            if (q == 0 || rng() % 3 == 0) { base = (uint32_t)(rng() % 200); spread = 1 + (uint32_t)(rng() % 56); dists = (uint32_t)(rng() % 3); }
            const bool few = rng() % 3 == 0;
            const uint32_t codes = (uint32_t)(few ? rng() % 40 : 200 + rng() % 3000);
            for (uint32_t c = 0; c < codes; c++) {
                if (dists && rng() % 4 == 0) {
                    rows[q][257 + rng() % 29]++;
                    rows[q][288 + rng() % (dists == 1 ? 4 : 30)]++;
                } else rows[q][base + rng() % spread]++;
            }
            rows[q][256] = 1;
        }
        std::vector<uint32_t> want(n);
        for (uint32_t i = 0; i < n; i++) want[i] = i;
        rule(rows, n, 0, MERGE_MAX, want);
        memset(&M, 0xEE, sizeof M);
        for (uint32_t q = 0; q < n; q++) {
            memcpy(M.rows + q * SYM_ROW, rows[q].data(), 4 * SYM_ROW);
            M.D[q] = size_of(rows, q, q + 1);
        }
        merge_tree(M, n, &g_bc, g_S, 0, 1);
        for (uint32_t i = 0; i < n; i++) {
            CHECK(M.head[i] == want[i]);
            if (want[i] != i) { merged++; continue; }
            // a head's row is its group's sum with one EndOfBlock, its D the group's exact size
            uint32_t e = i + 1;
            while (e < n && want[e] == i) e++;
            uint32_t sum[SYM_ROW] = {};
            for (uint32_t q = i; q < e; q++)
                for (uint32_t s = 0; s < SYM_ROW; s++) sum[s] += rows[q][s];
            sum[256] = 1;
            CHECK(memcmp(sum, M.rows + i * SYM_ROW, sizeof sum) == 0 && M.D[i] == size_of(rows, i, e));
            // never longer than the candidates on their own
            uint64_t apart = 0;
            for (uint32_t q = i; q < e; q++) apart += size_of(rows, q, q + 1);
            CHECK(M.D[i] <= apart);
            if (e < n) cut++;
        }
        trees++;
    }
    CHECK(merged > 100 && cut > 100);                    // (the inputs meet both answers)
    printf("block_merge ok: %d cells, %d refused, %d plans, %d regions, %d trees, %d merged, %d cuts\n", cells, refused, plans, regions, trees,
           merged, cut);
    return 0;
}
