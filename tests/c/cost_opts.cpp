// cost_opts.cpp — the host-only parts of CostLz77Encoder (LFX_LZ77_COST) under a plain host compiler: how
// lz77_kind is decoded and checked for kind 6 (lfx_enc_frame.h; 5 stays refused), what the kind resolves into, the container
// headers, every cell of encode_served for it, the work list and the segment cuts of lfx_cost.h over random chunk lists, the
// cost tables with the absent-symbol rule, and the kernel's recurrence — 16-bit costs in a ring of COST_RING slots, replayed
// here step for step — against the same recurrence in 64-bit integers.  No HIP, no device.
//   g++ -O2 -std=c++17 -Wall [-fsanitize=address,undefined] -o cost_opts tests/c/cost_opts.cpp && ./cost_opts
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../libflate_amd/csrc/lfx_cost.h"
#include "../../libflate_amd/csrc/lfx_enc_frame.h"

using namespace lfx;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "cost_opts: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static lfx_encode_opts with_kind(int32_t kind) {
    lfx_encode_opts o;
    encode_opts_default(&o);
    o.lz77_kind = kind;
    return o;
}
struct Resolved { int rc; EncodeSpec sp; };
static Resolved resolve(int format, const lfx_encode_opts &o) { Resolved r; r.rc = encode_spec(format, &o, &r.sp); return r; }

// the kernel's walk of one segment on the host: slots, clamps and cost_step as in lfx_cost.hip → the decisions of [a, b)
static void ring_walk(const std::vector<uint8_t> &buf, const std::vector<uint8_t> &len, const std::vector<uint16_t> &cd2, const uint8_t *tab,
                      CostSpan sp, std::vector<uint16_t> &out) {
    uint16_t ring[COST_RING];
    memset(ring, 0xEE, sizeof ring);                 // (a slot read before it is written shows)
    ring[0] = 0;
    uint32_t cs = 0;
    const uint32_t n = sp.top - sp.a;
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t p = sp.top - 1 - k;
        const uint32_t byte = buf[p], l = len[p], d = cd2[p];
        const uint32_t reach = k + 1;
        const uint32_t L = l + 3 < reach ? l + 3 : reach;
        uint32_t eb, ex;
        const uint32_t ds = d ? dist_symbol(d, eb, ex) : 0u;
        const uint32_t mat = (uint32_t)tab[COST_TAB_LEN + l] + tab[COST_TAB_DIST + ds];
        const uint32_t jump = cs + 1 >= L ? cs + 1 - L : cs + 1 + COST_RING - L;
        CHECK(jump < COST_RING && cs < COST_RING);
        bool literal;
        const uint32_t c = cost_step(tab[byte], d != 0, mat, ring[cs], ring[jump], &literal);
        cs = cs + 1 == COST_RING ? 0u : cs + 1;
        ring[cs] = (uint16_t)c;
        if (p < sp.b) out[p] = literal ? 0 : (uint16_t)d;
    }
}
// the contract's recurrence in 64-bit integers
static void plain_walk(const std::vector<uint8_t> &buf, const std::vector<uint8_t> &len, const std::vector<uint16_t> &cd2, const uint8_t *tab,
                       CostSpan sp, std::vector<uint16_t> &out) {
    std::vector<uint64_t> cost(sp.top - sp.a + 1, 0);
    for (uint32_t p = sp.top; p-- > sp.a;) {
        uint64_t c = tab[buf[p]] + cost[p + 1 - sp.a];
        bool literal = true;
        if (cd2[p]) {
            uint32_t eb, ex;
            const uint32_t L = len[p] + 3u, q = p + L < sp.top ? p + L : sp.top;
            const uint64_t m = (uint64_t)tab[COST_TAB_LEN + len[p]] + tab[COST_TAB_DIST + dist_symbol(cd2[p], eb, ex)] + cost[q - sp.a];
            if (m <= c) { c = m; literal = false; }
        }
        cost[p - sp.a] = c;
        if (p < sp.b) out[p] = literal ? 0 : cd2[p];
    }
}

int main() {
    // ---- the constant, the level in bits 8..15, what the kind resolves into
    CHECK(LFX_LZ77_COST == 6 && LFX_LZ77_COST_N(6) == (6 | 6 << 8) && LFX_LZ77_LEVEL == 4);
    for (int n = 1; n <= 9; n++) {
        const lfx_encode_opts o = with_kind(LFX_LZ77_COST_N(n));
        const Resolved r = resolve(LFX_ZLIB, o), r4 = resolve(LFX_ZLIB, with_kind(LFX_LZ77_LEVEL_N(n)));
        CHECK(r.rc == LFX_OK && r4.rc == LFX_OK && lz77_kind_of(o) == LFX_LZ77_COST);
        CHECK(r.sp.cost && r.sp.tuned && !r.sp.lazy && !r4.sp.cost);                 // the cost rule in place of the lazy one
        CHECK(r.sp.plan.lz77_kind == LFX_LZ77_LEVEL);                                // buffering and flushes: kind 4's plan
        CHECK(r.sp.chain_depth == r4.sp.chain_depth && r.sp.tune.depth == r4.sp.tune.depth && r.sp.tune.nice == r4.sp.tune.nice &&
              r.sp.tune.too_far == r4.sp.tune.too_far);                              // the level's candidates
        CHECK(!r.sp.auto_blocks && !r.sp.merge_blocks);
    }
    CHECK(resolve(LFX_ZLIB, with_kind(LFX_LZ77_COST)).rc == LFX_E_ARG);              // level 0
    for (int n = 10; n <= 255; n++) CHECK(resolve(LFX_ZLIB, with_kind(LFX_LZ77_COST_N(n))).rc == LFX_E_ARG);
    for (int bit = 16; bit < 32; bit++) CHECK(resolve(LFX_GZIP, with_kind((int32_t)((uint32_t)LFX_LZ77_COST_N(6) | 1u << bit))).rc == LFX_E_ARG);
    for (int32_t five : {5, 5 | 1 << 8, 5 | 6 << 8, 5 | 9 << 8}) CHECK(resolve(LFX_ZLIB, with_kind(five)).rc == LFX_E_ARG);   // 5 names no kind
    CHECK(lz77_runs_chain(2) && lz77_runs_chain(3) && lz77_runs_chain(4) && lz77_runs_chain(6) && !lz77_runs_chain(0) && !lz77_runs_chain(1) &&
          !lz77_runs_chain(5) && !lz77_runs_chain(7));
    CHECK(!lz77_chain_stage(5) && !lz77_chain_stage(6) && lz77_leveled(4) && lz77_leveled(6) && !lz77_leveled(5) && !lz77_leveled(3));
    // the kinds 0..4 answer as before
    for (int32_t kw : {0, 1, LFX_LZ77_CHAIN_DEPTH(8), LFX_LZ77_LAZY_DEPTH(255), LFX_LZ77_LEVEL_N(6)}) {
        const Resolved r = resolve(LFX_ZLIB, with_kind(kw));
        CHECK(r.rc == LFX_OK && !r.sp.cost && r.sp.plan.lz77_kind == (kw & 0xFF) && r.sp.lazy == ((kw & 0xFF) == 3 || (kw & 0xFF) == 4));
    }

    // ---- the container headers: Best unless the caller names a level; no_compression resets it
    auto flevel = [](const lfx_encode_opts &o) { std::vector<uint8_t> h; CHECK(container_header(LFX_ZLIB, o, h) == LFX_OK && h.size() == 2 && ((h[0] << 8) + h[1]) % 31 == 0); return h[1] >> 6; };
    auto xfl = [](const lfx_encode_opts &o) { std::vector<uint8_t> h; CHECK(container_header(LFX_GZIP, o, h) == LFX_OK && h.size() == 10); return (int)h[8]; };
    for (int n = 1; n <= 9; n++) {
        lfx_encode_opts o = with_kind(LFX_LZ77_COST_N(n));
        CHECK(lz77_level_of(o) == 1 + LFX_LEVEL_BEST && flevel(o) == 3 && xfl(o) == 2);
        o.lz77_level = 1 + LFX_LEVEL_FAST;
        CHECK(flevel(o) == 1 && xfl(o) == 4);
        o.lz77_level = 0;
        o.no_compression = 1;
        CHECK(lz77_level_of(o) == 0 && flevel(o) == 0 && xfl(o) == 0);
    }

    // ---- encode_served: every cell of kind 6
    static const EncodeEntry ENTRIES[10] = {ENC_DEVICE, ENC_BATCH, ENC_DICT_DEVICE, ENC_DICT_BATCH, ENC_STREAM, ENC_MEMBERS, ENC_INDEX, ENC_SHARD, ENC_LZ77, ENC_BATCH_PACKED};
    static const DictKind DICTS[3] = {DICT_NONE, DICT_PLAIN, DICT_CHAIN};
    int cells = 0, refused = 0;
    for (int n : {1, 6, 9})
        for (int32_t huffman = 0; huffman <= 2; huffman++)
            for (int32_t nc = 0; nc <= 1; nc++)
                for (int32_t bm = 0; bm <= 1; bm++) {
                    lfx_encode_opts o = with_kind(LFX_LZ77_COST_N(n)), o4 = with_kind(LFX_LZ77_LEVEL_N(n));
                    o.dynamic_huffman = o4.dynamic_huffman = huffman;
                    o.no_compression = o4.no_compression = nc;
                    o.block_merge = o4.block_merge = (uint8_t)bm;
                    const Resolved r = resolve(LFX_ZLIB, o), r4 = resolve(LFX_ZLIB, o4);
                    CHECK(r.rc == LFX_OK && r4.rc == LFX_OK && r.sp.auto_blocks == r4.sp.auto_blocks && r.sp.merge_blocks == r4.sp.merge_blocks);
                    for (EncodeEntry e : ENTRIES)
                        for (DictKind dict : DICTS) {
                            const char *why = nullptr, *why4 = nullptr;
                            const int rc = encode_served(e, r.sp, dict, &why), rc4 = encode_served(e, r4.sp, dict, &why4);
                            const char *want = nullptr;
                            bool as4 = false;                                            // the cell is kind 4's, whatever it says
                            if (e == ENC_SHARD && nc) as4 = true;                        // (the first row wins)
                            else if (e == ENC_SHARD) want = "lz77_kind: the N-GPU encode does not serve LFX_LZ77_COST";
                            else if (e == ENC_INDEX) want = "lz77_kind: lfx_encode_index_device does not serve LFX_LZ77_COST (its second parse would list the candidates twice)";
                            else if ((e == ENC_MEMBERS || e == ENC_STREAM) && r.sp.merge_blocks) as4 = true;     // block_merge's rows: combine as with kind 4
                            else if (dict == DICT_PLAIN) want = "lz77_kind: LFX_LZ77_COST with a preset dictionary is not supported (a dictionary made by lfx_dict_new_chain serves it)";
                            else as4 = true;
                            if (want) { CHECK(rc == LFX_E_UNSUPPORTED && why && strcmp(why, want) == 0); }
                            else { CHECK(as4 && rc == rc4 && (why == nullptr) == (why4 == nullptr) && (!why || strcmp(why, why4) == 0)); }
                            if (e != ENC_INDEX) CHECK(rc == rc4);                        // served where kind 4 is, but for the encode index
                            if (dict != DICT_PLAIN && e != ENC_INDEX && e != ENC_SHARD && !((e == ENC_MEMBERS || e == ENC_STREAM) && r.sp.merge_blocks))
                                CHECK(rc == LFX_OK);                                     // one-shot, batch, packed, chain dictionary, stream, members
                            refused += rc != LFX_OK;
                            cells++;
                        }
                }
    CHECK(cells == 3 * 3 * 2 * 2 * 10 * 3);

    // ---- the work list and the segment cuts: chunks that begin anywhere, of every length around the grid
    std::mt19937_64 rng(27);
    uint64_t segs = 0;
    for (int it = 0; it < 300; it++) {
        std::vector<ChunkDesc> chunks;
        uint64_t off = rng() % 7;
        const int nch = 1 + (int)(rng() % 6);
        for (int i = 0; i < nch; i++) {
            static const uint64_t EDGE[] = {0, 1, 3, 4, 5, COST_SEG + 2, COST_SEG + 3, COST_SEG + 4, COST_SEG + COST_WARM + 3, 2 * COST_SEG + COST_WARM + 2,
                                            2 * COST_SEG + COST_WARM + 3, 2 * COST_SEG + COST_WARM + 4, 262144};
            ChunkDesc ch{};
            ch.in_off = off;
            ch.len = rng() % 3 ? EDGE[rng() % (sizeof EDGE / sizeof *EDGE)] : rng() % 40000;
            ch.flags = rng() % 9 == 0 ? (uint32_t)CH_LITERALS : 0u;
            chunks.push_back(ch);
            off += ch.len + rng() % 5;
        }
        std::vector<CostItem> items;
        cost_items(chunks, items);
        size_t at = 0;
        for (uint32_t ci = 0; ci < chunks.size(); ci++) {
            const ChunkDesc &ch = chunks[ci];
            if ((ch.flags & CH_LITERALS) || ch.len <= 3) continue;
            const uint64_t end = ch.len - 3;
            uint64_t next = 0;                                                       // the segments tile [0, end) in order
            while (next < end) {
                CHECK(at < items.size() && items[at].chunk == ci && items[at].a == next && next % COST_SEG == 0);
                const CostSpan s = cost_span(ch.len, items[at].a);
                CHECK(s.a == next && s.a < s.b && s.b <= s.top && s.top <= end && s.b - s.a <= COST_SEG && s.top - s.b <= COST_WARM);
                CHECK(s.b == end || s.b - s.a == COST_SEG);
                CHECK(s.top == end || s.top - s.b == COST_WARM);                     // the warm-up is cut at `end` and nowhere else
                next = s.b;
                at++;
                segs++;
            }
            CHECK(next == end);
        }
        CHECK(at == items.size());
    }
    {   // an item that is not listed is empty, whatever its a
        const CostSpan s = cost_span(2, 0), t = cost_span(100, 4096), u = cost_span(0, 0);
        CHECK(s.a == s.b && s.b == s.top && t.a == 97 && t.b == 97 && t.top == 97 && u.top == 0);
    }

    // ---- the cost tables: the fixed code by hand, the absent-symbol rule
    uint32_t lit[288], dist[32];
    memset(lit, 0, sizeof lit);
    memset(dist, 0, sizeof dist);
    for (uint32_t i = 0; i < COST_TAB_N; i++) {
        const uint32_t v = cost_tab_entry(i, true, lit, dist, 0, 0);
        if (i < 256) CHECK(v == (i < 144 ? 8u : 9u));
        else if (i < 512) {
            const uint32_t L = i - 256 + 3;
            uint32_t eb, ex;
            const uint32_t s = len_symbol(L, eb, ex);
            CHECK(v == (s < 280 ? 7u : 8u) + eb && s >= 257 && s <= 285);
        } else CHECK(v == 5 + dist_extra_bits_of_symbol(i - 512));
    }
    CHECK(cost_absent(lit, 286, COST_NONE_LIT) == 9 && cost_absent(dist, 30, COST_NONE_DIST) == 5);    // an alphabet without any code
    lit['a'] = 3u << 16 | 5; lit[256] = 15u << 16; lit[257] = 7u << 16 | 1; dist[0] = 1u << 16; dist[29] = 4u << 16;
    const uint32_t al = cost_absent(lit, 286, COST_NONE_LIT), ad = cost_absent(dist, 30, COST_NONE_DIST);
    CHECK(al == 16 && ad == 5);                                                     // one more than the longest code
    CHECK(cost_tab_entry('a', false, lit, dist, al, ad) == 3 && cost_tab_entry('b', false, lit, dist, al, ad) == 16);
    CHECK(cost_tab_entry(COST_TAB_LEN + 0, false, lit, dist, al, ad) == 7 && cost_tab_entry(COST_TAB_LEN + 255, false, lit, dist, al, ad) == 16);   // L = 3: symbol 257; L = 258: 285, absent
    CHECK(cost_tab_entry(COST_TAB_LEN + 254, false, lit, dist, al, ad) == 16 + 5);                     // L = 257: symbol 284 (absent) + 5 extra bits
    CHECK(cost_tab_entry(COST_TAB_DIST + 0, false, lit, dist, al, ad) == 1 && cost_tab_entry(COST_TAB_DIST + 29, false, lit, dist, al, ad) == 4 + 13 &&
          cost_tab_entry(COST_TAB_DIST + 28, false, lit, dist, al, ad) == 5 + 13);
    {   // the tie goes to the match; without a candidate the literal; 16-bit wrap compares by the difference
        bool literal;
        CHECK(cost_step(8, true, 15, 100, 93, &literal) == 108 && !literal);
        CHECK(cost_step(8, true, 15, 100, 94, &literal) == 108 && literal);
        CHECK(cost_step(8, false, 0, 100, 0, &literal) == 108 && literal);
        CHECK(cost_step(9, true, 20, 65530, 65500, &literal) == ((65500u + 20u) & 0xFFFFu) && !literal);   // 65539 against 65520
        CHECK(cost_step(9, true, 20, 3, 65530, &literal) == 12 && literal);                              // 12 against 65550: the literal, through the wrap
    }

    // ---- the recurrence: the kernel's ring of 16-bit costs against plain integers, decision for decision
    uint64_t decided = 0, demoted = 0;
    for (int it = 0; it < 60; it++) {
        const uint32_t n = it < 8 ? (uint32_t[]){4, 5, 260, 262, 263, COST_SEG + 3, COST_SEG + 4, 2 * COST_SEG + COST_WARM + 4}[it] : 4 + (uint32_t)(rng() % 12000);
        const uint32_t end = n - 3;
        // widths: random codes of 1..15 bits with holes, or the fixed code
        const bool fixed = it % 5 == 4;
        for (uint32_t s = 0; s < 286; s++) lit[s] = rng() % 6 == 0 ? 0u : (uint32_t)(1 + rng() % (it % 3 == 0 ? 15 : 9)) << 16;
        for (uint32_t s = 0; s < 30; s++) dist[s] = rng() % 5 == 0 ? 0u : (uint32_t)(1 + rng() % 15) << 16;
        const uint32_t a_l = cost_absent(lit, 286, COST_NONE_LIT), a_d = cost_absent(dist, 30, COST_NONE_DIST);
        uint8_t tab[COST_TAB_N];
        for (uint32_t i = 0; i < COST_TAB_N; i++) {
            const uint32_t v = cost_tab_entry(i, fixed, lit, dist, a_l, a_d);
            CHECK(v >= 1 && v <= COST_MAX_MATCH);
            if (i < 256) CHECK(v <= COST_MAX_LIT);
            tab[i] = (uint8_t)v;
        }
        std::vector<uint8_t> buf(n), len(n);
        std::vector<uint16_t> cd2(n);
        const uint32_t dense = 1 + (uint32_t)(rng() % 4), longs = (uint32_t)(rng() % 3);
        for (uint32_t p = 0; p < n; p++) {
            buf[p] = (uint8_t)rng();
            const bool has = p < end && p > 0 && rng() % dense == 0;
            const uint32_t lim = n - p < MAX_LENGTH ? n - p : MAX_LENGTH;
            uint32_t L = longs == 0 ? 3 + (uint32_t)(rng() % 8) : longs == 1 ? 3 + (uint32_t)(rng() % 256) : (rng() % 2 ? 257 + (uint32_t)(rng() % 2) : 3 + (uint32_t)(rng() % 5));
            if (L > lim) L = lim;
            len[p] = has ? (uint8_t)(L - 3) : (uint8_t)(rng() % 2 ? 0 : 255);        // (no candidate: the byte is whatever a call left there)
            cd2[p] = has ? (uint16_t)(1 + rng() % (p < 32768 ? p : 32768)) : 0;
        }
        std::vector<uint16_t> got(n, 0xAAAA), want(n, 0xAAAA);
        for (uint32_t a = 0; a < end; a += COST_SEG) {
            const CostSpan sp = cost_span(n, a);
            ring_walk(buf, len, cd2, tab, sp, got);
            plain_walk(buf, len, cd2, tab, sp, want);
        }
        for (uint32_t p = 0; p < n; p++) {
            CHECK(got[p] == want[p]);
            if (p < end) { CHECK(got[p] == 0 || got[p] == cd2[p]); decided++; demoted += cd2[p] && !got[p]; }
            else CHECK(got[p] == 0xAAAA);                                            // nothing at or behind `end` is written
        }
    }
    CHECK(demoted > 0 && demoted < decided);
    printf("cost_opts ok: %d cells (%d refused), %llu segments, %llu decisions (%llu demoted)\n", cells, refused, (unsigned long long)segs,
           (unsigned long long)decided, (unsigned long long)demoted);
    return 0;
}
