// shuffle_geom.cpp — the host arithmetic of the byte-shuffle filter (libflate_amd/csrc/lfx_shuffle.h) without a
// device: the tile list covers every element of every record exactly once, the record's trailing bytes belong to exactly one
// item, the LDS image fits, and the range check refuses what meets.  tests/test_shuffle_geom.py builds it plain and with
// AddressSanitizer + UBSan.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../libflate_amd/csrc/lfx_shuffle.h"

using namespace lfx;

#define CHECK(x)                                                         \
    do {                                                                 \
        if (!(x)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } \
    } while (0)

static void cover(uint32_t s, const std::vector<uint64_t> &lens) {
    std::vector<ShufRec> recs;
    uint64_t at = 0;
    for (uint64_t n : lens) { recs.push_back(ShufRec{at, at, n}); at += n; }
    std::vector<ShufItem> items;
    CHECK(shuf_build_items((uint32_t)recs.size(), recs.data(), s, items));
    uint64_t want = 0;
    for (uint64_t n : lens) want += shuf_items_of(n, s);
    CHECK(items.size() == want);
    std::vector<std::vector<uint8_t>> seen(lens.size());
    std::vector<uint32_t> tails(lens.size(), 0);
    for (size_t i = 0; i < lens.size(); i++) seen[i].assign((size_t)(lens[i] / s), 0);
    const uint32_t t = shuf_tile_elems(s);
    uint32_t last_rec = 0;
    for (const ShufItem &it : items) {
        CHECK(it.rec < lens.size() && it.rec >= last_rec);          // record order
        last_rec = it.rec;
        const uint64_t k = lens[it.rec] / s;
        CHECK(lens[it.rec] > 0 && it.cnt <= t && it.e0 + it.cnt <= k && it.e0 % t == 0);
        CHECK(it.cnt > 0 || k == 0);
        CHECK((uint64_t)it.cnt * shuf_lds_stride(s) <= SHUF_LDS_BYTES || shuf_register_path(s));
        for (uint64_t e = it.e0; e < it.e0 + it.cnt; e++) CHECK(seen[it.rec][(size_t)e]++ == 0);
        if (it.e0 + it.cnt == k) tails[it.rec]++;                   // the item that copies the trailing bytes
    }
    for (size_t i = 0; i < lens.size(); i++) {
        for (uint8_t v : seen[i]) CHECK(v == 1);
        CHECK(tails[i] == (lens[i] ? 1u : 0u));
    }
}

int main() {
    for (uint32_t s = 1; s <= SHUF_MAX_ELEM; s++) {
        const uint64_t t = shuf_tile_elems(s);
        CHECK(t >= 64 && t * s <= SHUF_TILE_BYTES + 64 * s);
        if (shuf_register_path(s)) CHECK(t % (SHUF_WG * shuf_lane_elems(s)) == 0 && shuf_lane_elems(s) * s % 16 == 0);
        else CHECK(t % 64 == 0 && t * shuf_lds_stride(s) <= SHUF_LDS_BYTES && (shuf_lds_stride(s) & 1));
        // k = 0, 1, tile - 1, tile, tile + 1, several tiles; with and without trailing bytes; mixed in one batch
        std::vector<uint64_t> lens;
        for (uint64_t k : {(uint64_t)0, (uint64_t)1, t - 1, t, t + 1, 3 * t, 3 * t + 7})
            for (uint64_t r : {(uint64_t)0, (uint64_t)(s - 1)}) lens.push_back(k * s + r);
        lens.push_back(0);
        cover(s, lens);
        for (uint64_t n : lens) cover(s, {n});
    }
    // too many tiles for one launch
    {
        ShufRec big{0, 0, (uint64_t)1 << 46};
        std::vector<ShufItem> items;
        CHECK(!shuf_build_items(1, &big, 4, items));
    }
    // the range check: input against output, output against output; empty records meet nothing
    {
        const uint64_t A = 0x10000, B = 0x20000;
        ShufRec apart[2] = {{0, 0, 100}, {100, 100, 100}};
        CHECK(shuf_ranges_ok(2, apart, A, B));
        CHECK(!shuf_ranges_ok(2, apart, A, A));                     // in place
        CHECK(shuf_ranges_ok(2, apart, A, A + 200) && !shuf_ranges_ok(2, apart, A, A + 199) && !shuf_ranges_ok(2, apart, A + 199, A));
        ShufRec outs[2] = {{0, 0, 100}, {100, 99, 100}};
        CHECK(!shuf_ranges_ok(2, outs, A, B));                      // two outputs meet by one byte
        ShufRec cross[2] = {{0, 500, 100}, {450, 0, 100}};
        CHECK(!shuf_ranges_ok(2, cross, A, A));                     // record 0's output over record 1's input
        ShufRec empty[2] = {{0, 0, 0}, {0, 0, 100}};
        CHECK(shuf_ranges_ok(2, empty, A, B) && !shuf_ranges_ok(2, empty, A, A + 50));
        CHECK(shuf_ranges_ok(0, nullptr, A, A));
    }
    printf("shuffle geom ok\n");
    return 0;
}
