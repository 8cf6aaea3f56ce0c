// batch_unpacked.cpp — the layout of lfx_decode_batch_packed_device (libflate_amd/csrc/lfx_batch_unpack.h) under a
// plain host compiler: the host walk of the three kernels — first scan level per 256 streams, second level in rounds of 1024
// workgroup sums, the rebase with the pairs and the total it leaves for the copy-back — against the rule itself, stream by
// stream, for decode-shaped sizes.  No HIP, no device.
//   g++ -O2 -std=c++17 -Wall [-fsanitize=address,undefined] -o batch_unpacked tests/c/batch_unpacked.cpp
//   batch_unpacked self      the scratch's places, then every count x align x shape below; prints one line per count
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../libflate_amd/csrc/lfx_batch_unpack.h"

using namespace lfx;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "batch_unpacked: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

// decoded sizes as a batch has them: empty streams, sizes that are and are not multiples of align, a few that expand 1032:1
static std::vector<uint64_t> sizes_of(uint32_t count, uint32_t align, int shape) {
    std::vector<uint64_t> v(count);
    for (uint32_t i = 0; i < count; i++) {
        const uint64_t r = rnd();
        switch (shape) {
        case 0: v[i] = 0; break;                                              // every stream empty
        case 1: v[i] = (uint64_t)align * (r % 5); break;                      // multiples of align, zero among them
        case 2: v[i] = (uint64_t)align * (r % 5) + 1 + (r >> 8) % 3; break;   // never a multiple of align > 3
        default:
            v[i] = r % 16 == 0 ? 0 : r % 97 == 1 ? 1032ull * (1 + (r >> 20) % (1u << 20)) : (r >> 12) % (3ull * align + 70);
        }
    }
    return v;
}

static void run_case(uint32_t count, uint32_t align, int shape) {
    const std::vector<uint64_t> size = sizes_of(count, align, shape);
    const uint32_t nwg = bpack_nwg(count);
    std::vector<uint64_t> local(count), wg(nwg), back(bunpack_back_words(count), ~0ull);
    bunpack_host_layout(size.data(), count, align, local.data(), wg.data(), back.data());
    // the rule, directly: out_off[0] = 0, out_off[i + 1] = round_up(out_off[i] + size[i], align), total = the last stream's end
    uint64_t at = 0;
    for (uint32_t i = 0; i < count; i++) {
        CHECK(back[2 * (size_t)i] == at);
        CHECK(back[2 * (size_t)i + 1] == size[i]);
        CHECK(at % align == 0);
        if (i + 1 == count) { CHECK(back[2 * (size_t)count] == at + size[i]); }
        else at = (at + size[i] + align - 1) / align * align;
    }
}

static int run_self() {
    // the scratch: the five regions in order, none overlapping, the copy-back block last
    for (uint32_t count : {1u, 255u, 256u, 257u, 262145u, BPACK_MAX_COUNT}) {
        const BunpackScratch w = bunpack_scratch(count);
        CHECK(w.size == 0 && w.local_off == w.size + count && w.wg_sum == w.local_off + count);
        CHECK(w.res == w.wg_sum + bpack_nwg(count) && w.pairs == w.res + BUNPACK_RES_WORDS);
        CHECK(w.words == w.pairs + 2 * (uint64_t)count + 1 && bunpack_back_words(count) == 2 * (uint64_t)count + 1);
    }
    // 262145 = 1025 workgroup sums: the first count with two rounds of the second level
    CHECK(bpack_scan_rounds(bpack_nwg(262144)) == 1 && bpack_scan_rounds(bpack_nwg(262145)) == 2);
    for (uint32_t count : {1u, 256u, 257u, 262145u}) {
        for (uint32_t align : {1u, 8u, 4096u})
            for (int shape = 0; shape < 4; shape++) run_case(count, align, shape);
        printf("count=%u nwg=%u rounds=%u ok\n", count, bpack_nwg(count), bpack_scan_rounds(bpack_nwg(count)));
    }
    // by hand: an empty stream between two others, align 8 — the gap behind a size that is no multiple, none behind one that is
    {
        const uint64_t size[4] = {5, 0, 16, 3};
        uint64_t local[4], wg[1], back[9];
        bunpack_host_layout(size, 4, 8, local, wg, back);
        const uint64_t want[9] = {0, 5, 8, 0, 8, 16, 24, 3, 27};
        CHECK(!memcmp(back, want, sizeof want));
    }
    printf("batch_unpacked self ok\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "self")) return run_self();
    fprintf(stderr, "usage: batch_unpacked self\n");
    return 2;
}
