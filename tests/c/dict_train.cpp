// dict_train.cpp — the host side of lfx_dict_train_device (libflate_amd/csrc/lfx_dict_train.h) under a plain host
// compiler: the argument checks and the record table they leave, the places of the call's scratch, and dtrain_host_walk — the
// kernels' steps with the kernels' own cursor and lane walk, run one lane after the other.  No HIP, no device.
//   g++ -O2 -std=c++17 -Wall [-fsanitize=address,undefined] -o dict_train tests/c/dict_train.cpp
//   dict_train self                        the checks and the layout
//   dict_train walk FILE DICT_SIZE K       FILE: u32 count, count x {u64 off, u64 len}, then the samples buffer; prints the
//                                          dictionary in hex.  The samples are copied into a block of exactly their extent,
//                                          so a read outside the records is a read outside the block.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../libflate_amd/csrc/lfx_dict_train.h"

using namespace lfx;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "dict_train: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static int check(uint32_t count, const uint64_t *off, const uint64_t *len, uint32_t size, uint32_t seg, const void *dict, uint64_t cap,
                 DtrainPlan *pl) {
    const char *why = nullptr;
    const int rc = dtrain_check(count, off, len, size, seg, dict, cap, pl, &why);
    CHECK(why && (rc == LFX_OK) == (why[0] == 0));
    return rc;
}

static int run_self() {
    DtrainPlan pl;
    uint8_t room[8];
    const uint64_t off[4] = {10, 20, 25, 40}, len[4] = {10, 0, 15, 9};
    // the domain
    CHECK(check(4, off, len, 63, 16, room, 1 << 20, &pl) == LFX_E_ARG);
    CHECK(check(4, off, len, 32769, 16, room, 1 << 20, &pl) == LFX_E_ARG);
    CHECK(check(4, off, len, 64, 15, room, 1 << 20, &pl) == LFX_E_ARG);
    CHECK(check(4, off, len, 64, 65, room, 1 << 20, &pl) == LFX_E_ARG);
    CHECK(check(4, off, len, 64, 0, room, 1 << 20, &pl) == LFX_E_ARG);        // 0 selects 128, above a dict_size of 64
    CHECK(check(4, nullptr, len, 64, 16, room, 1 << 20, &pl) == LFX_E_ARG);
    CHECK(check(4, off, nullptr, 64, 16, room, 1 << 20, &pl) == LFX_E_ARG);
    CHECK(check(4, off, len, 64, 16, room, 63, &pl) == LFX_E_NOSPACE);
    CHECK(check(4, off, len, 64, 16, nullptr, 64, &pl) == LFX_E_ARG);
    CHECK(check(0, nullptr, nullptr, 64, 16, nullptr, 64, &pl) == LFX_OK && pl.n == 0 && pl.nrec() == 0 && pl.pos.size() == 1);
    // the table: the empty record dropped, positions and offsets in step, the extent
    CHECK(check(4, off, len, 200, 0, room, 200, &pl) == LFX_OK);
    CHECK(pl.k == 128 && pl.epochs == 1 && pl.n == 34 && pl.nrec() == 3 && pl.extent_lo == 10 && pl.extent_hi == 49);
    CHECK(pl.pos == (std::vector<uint32_t>{0, 10, 25, 34}) && pl.off == (std::vector<uint64_t>{10, 25, 40}));
    CHECK(check(4, off, len, 100, 16, room, 100, &pl) == LFX_OK && pl.epochs == 6);
    // order and overlap, wrapping, too many bytes
    { const uint64_t o[2] = {10, 19}, l[2] = {10, 5}; CHECK(check(2, o, l, 64, 16, room, 64, &pl) == LFX_E_ARG); }
    { const uint64_t o[2] = {10, 5}, l[2] = {0, 1}; CHECK(check(2, o, l, 64, 16, room, 64, &pl) == LFX_E_ARG); }
    { const uint64_t o[1] = {~0ull - 3}, l[1] = {8}; CHECK(check(1, o, l, 64, 16, room, 64, &pl) == LFX_E_ARG); }
    { const uint64_t o[2] = {0, 1ull << 31}, l[2] = {1ull << 31, 1}; CHECK(check(2, o, l, 64, 16, room, 64, &pl) == LFX_E_ARG); }
    { const uint64_t o[1] = {0}, l[1] = {1ull << 31}; CHECK(check(1, o, l, 64, 16, room, 64, &pl) == LFX_OK && pl.pos[1] == 1u << 31); }
    // the scratch: the regions in order, aligned, none overlapping; the step's words cover a chunk and its k - 8 behind it
    for (uint64_t n : {1ull, 255ull, 256ull, 257ull, 1ull << 22, 1ull << 31})
        for (uint32_t k : {16u, 128u, 32768u}) {
            const uint32_t epochs = 32768 / k, nrec = (uint32_t)std::min<uint64_t>(n, 100000);
            const DtrainScratch w = dtrain_scratch(n, nrec, epochs, k);
            CHECK(w.freq == 0 && w.slots >= 4ull << DTRAIN_F && w.out_len == w.slots + 8ull * epochs && w.pos >= w.out_len + 8);
            CHECK(w.off >= w.pos + 4ull * (nrec + 1) && w.tile_rec >= w.off + 8ull * nrec && w.prefix >= w.tile_rec + 4ull * w.ntiles);
            CHECK(w.bytes == w.prefix + 8 * w.prefix_words * w.step_grid && w.prefix_words >= DTRAIN_CHUNK + k - DTRAIN_D + 1);
            for (uint64_t at : {w.slots, w.pos, w.off, w.tile_rec, w.prefix}) CHECK(at % 256 == 0);
            CHECK((uint64_t)w.ntiles * DTRAIN_TILE >= n && (uint64_t)(w.ntiles - 1) * DTRAIN_TILE < n);
            // every chunk of the longest epoch has a workgroup, or the grid is at its cap
            const uint64_t longest = n / epochs + 1;
            CHECK(w.step_grid >= 1 && w.step_grid <= DTRAIN_STEP_GRID);
            CHECK(w.step_grid == DTRAIN_STEP_GRID || (uint64_t)w.step_grid * DTRAIN_CHUNK >= longest);
        }
    // the pick's word: a higher score wins, among equal scores the lower position; the sum saturates
    CHECK(dtrain_pick_key(5, 9) > dtrain_pick_key(4, 0) && dtrain_pick_key(5, 3) > dtrain_pick_key(5, 4));
    CHECK(dtrain_pick_key(1ull << 40, 7) >> 32 == 0xFFFFFFFFull && dtrain_pick_pos(dtrain_pick_key(77, 123456)) == 123456);
    CHECK(dtrain_sort_key(dtrain_pick_key(5, 3), 2) > dtrain_sort_key(dtrain_pick_key(5, 1), 3));      // the earlier epoch later
    CHECK(dtrain_hash(0) == 0 && dtrain_hash(1) == (uint32_t)(DTRAIN_PRIME >> 44));
    printf("dict_train self ok\n");
    return 0;
}

static int run_walk(const char *path, uint32_t dict_size, uint32_t k) {
    FILE *f = fopen(path, "rb");
    CHECK(f);
    uint32_t count = 0;
    CHECK(fread(&count, 4, 1, f) == 1);
    std::vector<uint64_t> off(count), len(count);
    for (uint32_t i = 0; i < count; i++) CHECK(fread(&off[i], 8, 1, f) == 1 && fread(&len[i], 8, 1, f) == 1);
    std::vector<uint8_t> buf;
    for (int ch; (ch = fgetc(f)) != EOF;) buf.push_back((uint8_t)ch);
    fclose(f);
    DtrainPlan pl;
    std::vector<uint8_t> out(dict_size);
    const int rc = check(count, off.data(), len.data(), dict_size, k, out.data(), dict_size, &pl);
    if (rc) { printf("status %d\n", rc); return 0; }
    CHECK(pl.extent_hi <= buf.size());
    if (!pl.n) { printf("dict \n"); return 0; }
    // the records' extent alone, in a block of its own
    uint8_t *block = (uint8_t *)malloc(pl.extent_hi - pl.extent_lo);
    CHECK(block);
    memcpy(block, buf.data() + pl.extent_lo, pl.extent_hi - pl.extent_lo);
    for (uint64_t &o : pl.off) o -= pl.extent_lo;
    const uint64_t n = dtrain_host_walk(pl, block, out.data());
    free(block);
    CHECK(n <= dict_size && n % pl.k == 0);
    printf("dict ");
    for (uint64_t i = 0; i < n; i++) printf("%02x", out[i]);
    printf("\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "self")) return run_self();
    if (argc == 5 && !strcmp(argv[1], "walk")) return run_walk(argv[2], (uint32_t)atoi(argv[3]), (uint32_t)atoi(argv[4]));
    fprintf(stderr, "usage: dict_train self | walk FILE DICT_SIZE K\n");
    return 2;
}
