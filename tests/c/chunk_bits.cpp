// chunk_bits.cpp — the arithmetic of pack by chunk (lfx_huff.h) under a plain host compiler: a block's symbol
// counts are kept one row per chunk; the block's histogram is the sum of the rows (sym_rows_sum), a chunk's packed size follows
// from its row and the block's code widths (chunk_bits_part), and the chunks' first bits are the running sum of the sizes
// (chunk_start_prefix).  Checked against the straight way: a code list with exactly those counts, sized word by word with
// code_bits — the function pack_chunk_kernel packs with.  Seeded random rows, all-zero chunks, a chunk that holds only
// EndOfBlock, blocks of 1, 4 and 129 chunks, dynamic and fixed codes, one lane and 64 lanes.  No HIP, no device.
//   g++ -O2 -std=c++17 -Wall [-fsanitize=address,undefined] -o chunk_bits tests/c/chunk_bits.cpp && ./chunk_bits
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

#include "../../libflate_amd/csrc/lfx_encode_stages.h"
#include "../../libflate_amd/csrc/lfx_huff.h"

using namespace lfx;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "chunk_bits: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

// the smallest length / distance of a symbol, and how many values the symbol covers: a code word for every extra-bit pattern
static uint32_t len_base(uint32_t sym) {
    for (uint32_t l = 3; l <= 258; l++) { uint32_t eb, ex; if (len_symbol(l, eb, ex) == sym) return l; }
    CHECK(false);
    return 0;
}
static uint32_t dist_base(uint32_t sym) {
    for (uint32_t d = 1; d <= 32768; d++) { uint32_t eb, ex; if (dist_symbol(d, eb, ex) == sym) return d; }
    CHECK(false);
    return 0;
}

enum Shape { RANDOM, ZERO, EOB_ONLY };

// a chunk as a code list: literals, EndOfBlock, (length, distance) pairs — the row is counted from the list, so the row and
// the list agree by construction and every length code comes with a distance code
static std::vector<uint32_t> make_codes(std::mt19937_64 &rng, Shape shape, bool last) {
    std::vector<uint32_t> codes;
    if (shape == RANDOM) {
        const uint32_t n = (uint32_t)(rng() % 3000);
        const uint32_t lit_span = rng() % 4 == 0 ? 4 : 256, match_pct = (uint32_t)(rng() % 90);
        for (uint32_t i = 0; i < n; i++) {
            if (rng() % 100 < match_pct) {
                const uint32_t ls = 257 + (uint32_t)(rng() % 29), ds = (uint32_t)(rng() % 30);
                const uint32_t lb = len_base(ls), db = dist_base(ds);
                const uint32_t le = len_extra_bits_of_symbol(ls), de = dist_extra_bits_of_symbol(ds);
                uint32_t len = lb + (uint32_t)(rng() & ((1u << le) - 1));
                if (ls == 284 && len == 258) len = 257;     // (symbol 284 ends at 257: 258 has symbol 285 to itself)
                const uint32_t dist = db + (uint32_t)(rng() & ((1u << de) - 1));
                uint32_t eb, ex;
                CHECK(len_symbol(len, eb, ex) == ls && eb == le && dist_symbol(dist, eb, ex) == ds && eb == de);
                codes.push_back(len << 16 | dist);
            } else codes.push_back((uint32_t)(rng() % lit_span) << 16);
        }
    }
    if (last) codes.push_back(CODE_EOB);
    return codes;
}
static void count_row(const std::vector<uint32_t> &codes, uint32_t *row) {
    for (uint32_t v : codes) {
        const uint32_t dist = v & 0xFFFFu, val = v >> 16;
        uint32_t eb, ex;
        if (!dist) row[val]++;
        else { row[len_symbol(val, eb, ex)]++; row[288 + dist_symbol(dist, eb, ex)]++; }
    }
}

static void check_block(std::mt19937_64 &rng, uint32_t nchunks, uint32_t type, int shape_of_all, uint64_t &words) {
    std::vector<std::vector<uint32_t>> lists(nchunks);
    std::vector<uint32_t> rows((size_t)nchunks * SYM_ROW, 0u);
    for (uint32_t c = 0; c < nchunks; c++) {
        const bool last = c + 1 == nchunks;
        Shape sh = shape_of_all >= 0 ? (Shape)shape_of_all : (rng() % 5 == 0 ? ZERO : RANDOM);
        if (last && sh == ZERO) sh = EOB_ONLY;              // (the block's last chunk always holds EndOfBlock)
        if (!last && sh == EOB_ONLY) sh = ZERO;
        lists[c] = make_codes(rng, sh, last);
        count_row(lists[c], &rows[(size_t)c * SYM_ROW]);
    }
    // the block's histogram: the sum of the rows, by one lane and by 64 — against a count of all lists
    uint32_t hist[SYM_ROW], hist64[SYM_ROW], want[SYM_ROW] = {};
    for (uint32_t i = 0; i < SYM_ROW; i++) hist[i] = hist64[i] = 0xDEADBEEFu;
    sym_rows_sum(rows.data(), nchunks, hist, 0, 1);
    for (int l = 0; l < 64; l++) sym_rows_sum(rows.data(), nchunks, hist64, l, 64);
    for (const auto &l : lists) count_row(l, want);
    for (uint32_t i = 0; i < SYM_ROW; i++) CHECK(hist[i] == want[i] && hist64[i] == want[i]);
    CHECK(hist[256] == 1 && hist[286] == 0 && hist[287] == 0 && hist[318] == 0 && hist[319] == 0);
    // the block's codes, as the kernel builds them from that histogram
    auto S = std::make_unique<HuffScratch>();
    auto bc = std::make_unique<BlockCodes>();
    huff_block_build(hist, type, bc.get(), *S, 0, 1);
    // every chunk's size: the shared function (one lane, and 64 lanes summed) against code_bits over the list
    std::vector<uint64_t> bits(nchunks), start(nchunks, ~0ull);
    uint64_t total = 0;
    for (uint32_t c = 0; c < nchunks; c++) {
        const uint32_t *row = &rows[(size_t)c * SYM_ROW];
        bits[c] = chunk_bits_part(row, bc.get(), 0, 1);
        uint64_t by64 = 0;
        for (int l = 0; l < 64; l++) by64 += chunk_bits_part(row, bc.get(), l, 64);
        uint64_t straight = 0;
        for (uint32_t v : lists[c]) {
            uint64_t b;
            const uint32_t nb = code_bits(v, bc->lit, bc->dist, b);
            CHECK(nb > 0 && nb <= 48 && (nb == 64 || (b >> nb) == 0));
            straight += nb;
        }
        words += lists[c].size();
        CHECK(bits[c] == straight && by64 == straight);
        if (lists[c].empty()) CHECK(bits[c] == 0);
        total += bits[c];
    }
    // the sizes add up to the block's body: 3 block bits + header + Σ
    CHECK(bc->body_bits == 3 + (uint64_t)bc->hdr_bits + total);
    // the first bits: a running sum
    chunk_start_prefix(bits.data(), nchunks, start.data());
    uint64_t at = 0;
    for (uint32_t c = 0; c < nchunks; c++) { CHECK(start[c] == at); at += bits[c]; }
    CHECK(at == total);
}

// which calls pack by chunk (encode_geometry, lfx_encode_stages.h): the benchmark's shape does, one chunk of the whole input
// does not, a stored block or a caller's own code words never do, and LFX_PACK_BY_CHUNK forces it only where it is legal
static Plan plan_of(uint64_t n, uint64_t write_size, bool no_compression) {
    PlanOpts o;
    o.no_compression = no_compression;
    Planner p(o);
    p.write_repeat(write_size, n / write_size);
    if (n % write_size) p.write(n % write_size);
    return p.finish();
}
static bool by_chunk(const Plan &plan, bool host_codes, uint32_t n_cu, bool hist_separate, int sw) {
    return encode_geometry(plan, host_codes, n_cu, hist_separate, sw).pack_by_chunk;
}
static void check_selection() {
    const uint64_t MIB = 1ull << 20;
    const Plan s8k = plan_of(256 * MIB, 8192, false), s1 = plan_of(256 * MIB, 256 * MIB, false), small = plan_of(MIB, 8192, false);
    CHECK(s8k.chunks.size() == 1025 && s1.chunks.size() == 2);      // (each with the empty final block: a chunk that holds only EndOfBlock)
    CHECK(by_chunk(s8k, false, 256, false, PACK_BY_CHUNK_AUTO));
    CHECK(!by_chunk(s1, false, 256, false, PACK_BY_CHUNK_AUTO));            // one chunk of 131073 tiles: fewer chunks than CUs, and over the tile bound
    CHECK(!by_chunk(plan_of(256 * MIB, 256 * MIB, false), false, 1, false, PACK_BY_CHUNK_AUTO));   // ... the tile bound alone
    CHECK(div_up(256 * MIB + 1, PACK_TILE) > PACK_CHUNK_MAX_TILES && div_up(8 * (uint64_t)MAX_WINDOW + 1, PACK_TILE) <= PACK_CHUNK_MAX_TILES);
    CHECK(!by_chunk(small, false, 256, false, PACK_BY_CHUNK_AUTO));         // 4 chunks on 256 CUs
    CHECK(by_chunk(small, false, 256, false, PACK_BY_CHUNK_ON));            // ... forced: legal whatever the chunk count
    CHECK(by_chunk(s1, false, 256, false, PACK_BY_CHUNK_ON));
    CHECK(!by_chunk(s8k, false, 256, false, PACK_BY_CHUNK_OFF));
    for (int sw : {PACK_BY_CHUNK_AUTO, PACK_BY_CHUNK_ON}) {
        CHECK(!by_chunk(s8k, true, 256, false, sw));                        // a caller's own code words
        CHECK(!by_chunk(s8k, false, 256, true, sw));                        // the histogram is not fused
        CHECK(!by_chunk(plan_of(256 * MIB, 8192, true), false, 256, false, sw));   // stored blocks
    }
    // the four-argument call of before: the geometry decides
    CHECK(encode_geometry(s8k, false, 256, false).pack_by_chunk && !encode_geometry(small, false, 256, false).pack_by_chunk);
}

int main() {
    check_selection();
    std::mt19937_64 rng(20260607);
    uint64_t blocks = 0, words = 0;
    for (uint32_t type : {(uint32_t)BT_DYNAMIC, (uint32_t)BT_FIXED})
        for (uint32_t nchunks : {1u, 4u, 129u}) {
            for (int it = 0; it < (nchunks == 129 ? 6 : 40); it++, blocks++) check_block(rng, nchunks, type, -1, words);   // seeded random rows, some all-zero
            check_block(rng, nchunks, type, ZERO, words);       // all-zero chunks, the last one only EndOfBlock
            check_block(rng, nchunks, type, RANDOM, words);
            blocks += 2;
        }
    // a block of one chunk that holds only EndOfBlock (the empty final block)
    check_block(rng, 1, BT_DYNAMIC, EOB_ONLY, words);
    check_block(rng, 1, BT_FIXED, EOB_ONLY, words);
    blocks += 2;
    printf("chunk_bits ok: %llu blocks of 1, 4 and 129 chunks, %llu code words\n", (unsigned long long)blocks, (unsigned long long)words);
    return 0;
}
