// batch_packed.cpp — the layout arithmetic of lfx_encode_batch_packed_device (libflate_amd/csrc/lfx_batch_pack.h)
// under a plain host compiler: the walk of the three kernels' arithmetic — first scan level per 256 streams, second level in
// rounds of 1024 workgroup sums, rebase — that tests/test_batch_packed_abi.py holds against its own model.  No HIP, no device.
//   g++ -O2 -std=c++17 -Wall [-fsanitize=address,undefined] -o batch_packed tests/c/batch_packed.cpp
//   batch_packed layout <align> <lens.u64> <out.u64>   lengths (uint64 LE) → out_off[0..count), then the total; prints the geometry
//   batch_packed self                                  round_up, align domain, the fold, the bound sum and its 64-bit overflow
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../libflate_amd/csrc/lfx_batch_pack.h"

using namespace lfx;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "batch_packed: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static int run_layout(uint32_t align, const char *in_path, const char *out_path) {
    CHECK(bpack_align_ok(align));
    FILE *f = fopen(in_path, "rb");
    CHECK(f);
    std::vector<uint64_t> len;
    uint64_t v;
    while (fread(&v, 8, 1, f) == 1) len.push_back(v);
    fclose(f);
    CHECK(len.size() <= BPACK_MAX_COUNT);
    const uint32_t count = (uint32_t)len.size(), nwg = bpack_nwg(count);
    // the call's own order: the bound sum first (the lengths stand in for their bounds) — an overflow launches nothing
    uint64_t sum = 0;
    if (!bpack_bound_sum(len.data(), count, align, &sum)) { printf("overflow\n"); return 3; }
    std::vector<uint64_t> local(count), wg(nwg ? nwg : 1), off(count + 1);
    bpack_host_size(len.data(), count, align, local.data(), wg.data());
    const uint64_t total = bpack_host_scan(wg.data(), nwg);
    bpack_host_rebase(local.data(), wg.data(), count, off.data());
    off[count] = total;
    CHECK(total <= sum);
    f = fopen(out_path, "wb");
    CHECK(f);
    CHECK(fwrite(off.data(), 8, off.size(), f) == off.size());
    fclose(f);
    printf("count=%u nwg=%u rounds=%u total=%llu\n", count, nwg, bpack_scan_rounds(nwg), (unsigned long long)total);
    return 0;
}

static int run_self() {
    // the align domain
    for (uint32_t a = 0; a <= 10000; a++) {
        bool pow2 = false;
        for (uint32_t k = 0; k <= 12; k++) pow2 |= a == (1u << k);
        CHECK(bpack_align_ok(a) == pow2);
    }
    CHECK(!bpack_align_ok(8192) && !bpack_align_ok(3) && !bpack_align_ok(0x80000000u));
    // round_up and the term
    for (uint32_t a = 1; a <= 4096; a <<= 1)
        for (uint64_t x : {0ull, 1ull, 2ull, 3ull, 63ull, 64ull, 65ull, 4095ull, 4096ull, 4097ull, (1ull << 40) + 1}) {
            const uint64_t r = bpack_round_up(x, a);
            CHECK(r >= x && r - x < a && r % a == 0);
            CHECK(bpack_term(x, 3, 5, a) == r && bpack_term(x, 4, 5, a) == x);
        }
    CHECK(bpack_nwg(0) == 0 && bpack_nwg(1) == 1 && bpack_nwg(256) == 1 && bpack_nwg(257) == 2 && bpack_nwg(BPACK_MAX_COUNT) == 0xFFFFFFu);
    CHECK(bpack_scan_rounds(0) == 0 && bpack_scan_rounds(1024) == 1 && bpack_scan_rounds(1025) == 2);
    // the fold: a dynamic block, a stored one at an odd bit, an absorbed one, the closing alignment — by hand
    {
        std::vector<BlockDesc> bd(4);
        std::vector<BlockCodes> bc(4);
        memset(bd.data(), 0, sizeof(BlockDesc) * 4);
        memset(bc.data(), 0, sizeof(BlockCodes) * 4);
        bd[0].type = BT_DYNAMIC; bc[0].body_bits = 1001;
        bd[1].type = BT_RAW; bd[1].in_len = 5; bc[1].body_bits = 77777;          // (a stored block's body_bits are not read)
        bd[2].type = BT_ABSORBED; bc[2].body_bits = 99999;
        bd[3].type = BT_FIXED; bc[3].body_bits = 10; bd[3].final = 1; bd[3].align_after = 1;
        uint64_t start[4] = {~0ull, ~0ull, ~0ull, ~0ull};
        const uint64_t b0 = 16;                                   // a 2-byte header
        const uint64_t e0 = b0 + 1001, e1 = ((e0 + 3 + 7) & ~7ull) + 32 + 40, e3 = (e1 + 10 + 7) & ~7ull;
        CHECK(bpack_fold<true>(bd.data(), bc.data(), 0, 4, b0, start) == e3);
        CHECK(start[0] == b0 && start[1] == e0 && start[2] == e1 && start[3] == e1);
        CHECK(bpack_fold<false>(bd.data(), bc.data(), 0, 4, b0, nullptr) == e3);
        CHECK(bpack_stream_len(bd.data(), bc.data(), 0, 4, 2, 4) == e3 / 8 + 4);
        CHECK(bpack_stream_len(bd.data(), bc.data(), 1, 1, 0, 0) == 1 + 4 + 5);   // an empty header, one stored block
        CHECK(bpack_fold<false>(bd.data(), bc.data(), 2, 0, 123, nullptr) == 123);
    }
    // the bound sum: exact where it fits, refused where 64 bits do not hold it
    {
        const uint64_t a[3] = {1, 4096, 4097};
        uint64_t s = 0;
        CHECK(bpack_bound_sum(a, 3, 1, &s) && s == 8194);
        CHECK(bpack_bound_sum(a, 3, 4096, &s) && s == 4096 + 4096 + 8192);
        CHECK(bpack_bound_sum(a, 0, 64, &s) && s == 0);
        const uint64_t big[2] = {~0ull - 10, 10};
        CHECK(bpack_bound_sum(big, 2, 1, &s) && s == ~0ull);
        CHECK(!bpack_bound_sum(big, 2, 2, &s));                   // the first term's round-up wraps
        const uint64_t big2[2] = {~0ull - 10, 11};
        CHECK(!bpack_bound_sum(big2, 2, 1, &s));
        const uint64_t half[3] = {1ull << 63, 1ull << 62, 1ull << 62};
        CHECK(!bpack_bound_sum(half, 3, 4096, &s) && bpack_bound_sum(half, 2, 4096, &s) && s == (3ull << 62));
        std::vector<uint64_t> many(70000, 1ull << 48);            // 70000 x 2^48 > 2^64
        CHECK(!bpack_bound_sum(many.data(), 70000, 1, &s) && bpack_bound_sum(many.data(), 65535, 1, &s));
    }
    printf("batch_packed self ok\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "self")) return run_self();
    if (argc == 5 && !strcmp(argv[1], "layout")) return run_layout((uint32_t)strtoul(argv[2], nullptr, 10), argv[3], argv[4]);
    fprintf(stderr, "usage: batch_packed self | layout <align> <lens.u64> <out.u64>\n");
    return 2;
}
