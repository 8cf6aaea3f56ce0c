// lfx_shuffle.h — the byte-shuffle filter (lfx_shuffle_*): HDF5's H5Z_FILTER_SHUFFLE, numcodecs' Shuffle.
// For a record of n bytes and element size s: k = n / s, r = n % s;  shuffle: out[j*k + i] = in[i*s + j] (i < k, j < s), the r
// trailing bytes copied;  unshuffle: the inverse.  Host arithmetic only — the tile list one launch works through, the argument
// checks — so that a CPU program checks it (tests/c/shuffle_geom.cpp); the kernels are lfx_shuffle.hip's.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace lfx {

constexpr uint32_t SHUF_MAX_ELEM = 256;       // elem_size: 1..256
constexpr uint32_t SHUF_WG = 256;             // lanes of a workgroup
constexpr uint32_t SHUF_TILE_BYTES = 16384;   // the bytes of one item, about
// the generic path's LDS image: an element takes s | 1 bytes there (an odd stride: the transposed reads meet no bank twice), and
// a tile's elements are a multiple of 64 at s <= 256 — at most 16384 / s * (s + 1) bytes, s >= 6 where s is even
constexpr uint32_t SHUF_LDS_BYTES = 19200;

// one record of a call: where it is read, where it is written, its bytes
struct ShufRec {
    uint64_t in_off, out_off, len;
};
// one workgroup's work: `cnt` elements of record `rec` from element e0 on.  The item that holds a record's last element also
// copies its r trailing bytes; a record shorter than one element has one item with cnt = 0, an empty record none.
struct ShufItem {
    uint64_t e0;
    uint32_t rec, cnt;
};

// the register path: a lane takes E elements, 16 bytes or a multiple, and four bytes or more of every plane
inline bool shuf_register_path(uint32_t s) { return s == 2 || s == 4 || s == 8 || s == 16; }
inline uint32_t shuf_lane_elems(uint32_t s) { return s == 2 ? 8 : 4; }

// the elements of one item: about SHUF_TILE_BYTES, a multiple of what a workgroup takes in one step (register path) or of 64
inline uint32_t shuf_tile_elems(uint32_t s) {
    if (shuf_register_path(s)) return SHUF_TILE_BYTES / s;
    return std::max(64u, SHUF_TILE_BYTES / s / 64 * 64);
}
inline uint32_t shuf_lds_stride(uint32_t s) { return s | 1; }

inline uint64_t shuf_items_of(uint64_t n, uint32_t s) {
    if (!n) return 0;
    const uint64_t k = n / s, t = shuf_tile_elems(s);
    return std::max<uint64_t>(1, (k + t - 1) / t);
}

// the items of `count` records in record order → false when they are more than one launch takes (2^31 - 1)
inline bool shuf_build_items(uint32_t count, const ShufRec *recs, uint32_t s, std::vector<ShufItem> &items) {
    uint64_t total = 0;
    for (uint32_t i = 0; i < count; i++) total += shuf_items_of(recs[i].len, s);
    if (total > 0x7fffffffull) return false;
    items.clear();
    items.reserve((size_t)total);
    const uint64_t t = shuf_tile_elems(s);
    for (uint32_t i = 0; i < count; i++) {
        const uint64_t n = recs[i].len, k = n / s;
        if (!n) continue;
        if (!k) { items.push_back(ShufItem{0, i, 0}); continue; }
        for (uint64_t e = 0; e < k; e += t) items.push_back(ShufItem{e, i, (uint32_t)std::min(t, k - e)});
    }
    return true;
}

// No byte range read may meet a byte range written, and no two written ranges may meet (neighbouring records are written
// concurrently).  in_base / out_base: the buffers' addresses.  Empty records meet nothing.
inline bool shuf_ranges_ok(uint32_t count, const ShufRec *recs, uint64_t in_base, uint64_t out_base) {
    std::vector<std::pair<uint64_t, uint64_t>> w;      // [lo, hi) written, sorted
    for (uint32_t i = 0; i < count; i++)
        if (recs[i].len) w.emplace_back(out_base + recs[i].out_off, out_base + recs[i].out_off + recs[i].len);
    std::sort(w.begin(), w.end());
    for (size_t i = 1; i < w.size(); i++)
        if (w[i].first < w[i - 1].second) return false;
    for (uint32_t i = 0; i < count; i++) {
        if (!recs[i].len) continue;
        const uint64_t lo = in_base + recs[i].in_off, hi = lo + recs[i].len;
        // the first written range that ends behind lo
        auto it = std::upper_bound(w.begin(), w.end(), lo, [](uint64_t v, const std::pair<uint64_t, uint64_t> &p) { return v < p.second; });
        if (it != w.end() && it->first < hi) return false;
    }
    return true;
}

// lfx_shuffle.hip: one launch over `nitems` items; d_recs and d_items are device copies of the tables above
int launch_shuffle(void *stream, int dir, uint32_t s, const uint8_t *d_in, uint8_t *d_out, const ShufRec *d_recs, const ShufItem *d_items,
                   uint32_t nitems);

}  // namespace lfx
