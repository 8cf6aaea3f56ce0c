// dict_chain_items.cpp — the host arithmetic of the chain kernel's dictionary instance (lfx_chain.h) under a plain
// host compiler: the work list in its two runs, and that what the dictionary instance stages — the dictionary's tail and its
// chain in front of the chunk's bytes and candidates — stays inside the LDS arrays for every tile, window size, dictionary
// length and phase of the chunk on the dword grids.  No HIP, no device.
//   g++ -O2 -std=c++17 -Wall [-fsanitize=address,undefined] -o dict_chain_items tests/c/dict_chain_items.cpp && ./dict_chain_items
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../libflate_amd/csrc/lfx_chain.h"

using namespace lfx;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "dict_chain_items: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

// one tile of the dictionary instance as the kernel lays it out (lfx_chain.hip): → the last LDS byte a compare may read and the
// last candidate entry, against the arrays' sizes
static void check_tile(uint32_t tile, uint32_t usable, uint32_t window, uint32_t max_len, uint32_t n, uint32_t p0, uint32_t sh, uint32_t csh) {
    const uint32_t bw = chain_lds_bytes_dw(tile, MAX_WINDOW), cw = chain_lds_cand_dw(tile, MAX_WINDOW);
    const uint32_t end = (n > 3 ? n : 3) - 3;
    CHECK(p0 < end && p0 < window && window <= MAX_WINDOW && usable <= MAX_WINDOW);
    const ChainDictFill f = chain_dict_fill(usable, window, p0);
    CHECK(f.n_t >= (usable ? 1u : 0u) && f.n_t <= usable && p0 + f.n_t <= window);      // the hole: what the chunk's own window lacks
    CHECK(4 * f.dw_t >= f.n_t && 4 * f.dw_t < f.n_t + 4 && 2 * f.dw_c >= f.n_t && 2 * f.dw_c < f.n_t + 2);
    const uint32_t p1 = p0 + tile < end ? p0 + tile : end;
    const uint32_t hi = (uint64_t)p0 + tile + max_len < n ? p0 + tile + max_len : n;
    // bytes: position q at LDS byte 4 * dw_t + sh + q; T's first staged byte at 4 * dw_t + sh - n_t >= 0
    CHECK(4 * f.dw_t + sh >= f.n_t);
    const uint32_t ndw = (hi + sh + 3) >> 2;                          // the chunk's dwords, from dw_t on
    CHECK(f.dw_t + ndw <= bw);
    // a compare step at p < p1, cur < lim <= max_len reads 8 bytes from p + cur and three dwords around them
    const uint32_t last = 4 * f.dw_t + sh + (p1 - 1) + (max_len - 1);
    CHECK(((last >> 2) + 2) < bw);
    // candidates: position q at entry 2 * dw_c + csh + q
    CHECK(2 * f.dw_c + csh >= f.n_t);
    const uint32_t ncw = (p1 + csh + 1) >> 1;
    CHECK(f.dw_c + ncw <= cw);
    if (f.n_t) CHECK(2 * f.dw_c + csh >= 1);                          // the entry of |T|-1
    // every candidate within window of a position of the tile is staged: c >= p0 - window >= -n_t or c >= -usable
    CHECK((int64_t)p0 - (int64_t)window >= -(int64_t)f.n_t || f.n_t == usable);
}

int main() {
    std::mt19937_64 rng(21);
    // ---- the LDS of the dictionary instance, both tiles: edges by hand, then random
    const uint32_t usables[] = {0, 1, 2, 3, 5, 1001, 32767, 32768}, windows[] = {1, 2, 255, 256, 1024, 16384, 16385, 32767, 32768};
    int tiles = 0;
    for (uint32_t tile : {CHAIN_TILE, CHAIN_TILE_SMALL})
        for (uint32_t usable : usables)
            for (uint32_t window : windows)
                for (uint32_t sh = 0; sh < 4; sh++)
                    for (uint32_t csh = 0; csh < 2; csh++) {
                        const uint32_t nmax = tile == CHAIN_TILE_SMALL ? CHAIN_TILE_SMALL : 6 * CHAIN_TILE;
                        for (uint32_t n : {4u, 5u, 8u, tile, tile + 3, tile + 4, 2 * tile + 3, nmax})
                            for (uint32_t p0 = 0; p0 + 3 < n && p0 < window && n <= nmax; p0 += tile) {
                                check_tile(tile, usable, window, 258, n, p0, sh, csh);
                                check_tile(tile, usable, window, 3, n, p0, sh, csh);
                                tiles += 2;
                            }
                    }
    for (int it = 0; it < 20000; it++) {
        const uint32_t tile = rng() & 1 ? CHAIN_TILE : CHAIN_TILE_SMALL;
        const uint32_t n = 4 + (uint32_t)(rng() % (tile == CHAIN_TILE_SMALL ? CHAIN_TILE_SMALL - 3 : 6 * CHAIN_TILE));
        const uint32_t window = 1 + (uint32_t)(rng() % MAX_WINDOW), usable = (uint32_t)(rng() % (MAX_WINDOW + 1));
        const uint32_t p0 = (uint32_t)(rng() % ((n - 4) / tile + 1)) * tile;
        if (p0 >= window) continue;
        check_tile(tile, usable, window, 3 + (uint32_t)(rng() % 256), n, p0, (uint32_t)(rng() & 3), (uint32_t)(rng() & 1));
        tiles++;
    }

    // ---- the work list: chain_items' items, the tiles of the primed chunks within `window` of their start last, each run in order
    int lists = 0;
    for (int it = 0; it < 2000; it++) {
        std::vector<ChunkDesc> chunks(1 + rng() % 9);
        for (ChunkDesc &ch : chunks) {
            ch = ChunkDesc{};
            ch.len = rng() % 5 == 0 ? rng() % 8 : rng() % 3 == 0 ? CHAIN_TILE_SMALL - 2 + rng() % 5 : rng() % (6 * CHAIN_TILE);
            ch.flags = rng() % 6 == 0 ? CH_LITERALS : rng() % 2 == 0 ? CH_DICT : 0;
        }
        const uint32_t tile = chain_small(chunks) ? CHAIN_TILE_SMALL : CHAIN_TILE;
        const uint32_t window = rng() % 4 == 0 ? MAX_WINDOW : 1 + (uint32_t)(rng() % MAX_WINDOW);
        std::vector<ChainItem> all, items, none;
        uint32_t n_plain = 0, n_none = 0;
        chain_items(chunks, tile, all);
        chain_items_dict(chunks, tile, window, true, items, n_plain);
        chain_items_dict(chunks, tile, window, false, none, n_none);
        CHECK(items.size() == all.size() && n_plain <= items.size() && none.size() == all.size() && n_none == all.size());
        size_t a = 0, b = n_plain;
        for (size_t k = 0; k < all.size(); k++) {
            CHECK(none[k].chunk == all[k].chunk && none[k].p0 == all[k].p0);
            const bool primed = (chunks[all[k].chunk].flags & CH_DICT) && all[k].p0 < window;
            size_t &at = primed ? b : a;
            CHECK(at < (primed ? items.size() : n_plain) && items[at].chunk == all[k].chunk && items[at].p0 == all[k].p0);
            at++;
        }
        CHECK(a == n_plain && b == items.size());
        lists++;
    }
    printf("dict_chain_items ok: %d tiles, %d lists\n", tiles, lists);
    return 0;
}
