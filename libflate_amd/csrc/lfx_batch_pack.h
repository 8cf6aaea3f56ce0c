// lfx_batch_pack.h — lfx_encode_batch_packed_device (include/lfx.h): the layout arithmetic of a batch whose
// streams lie back to back.  ONE statement of it for the HIP kernels (lfx_batch_pack.hip), for the entry point (lfx_api.cpp)
// and for the host test (tests/c/batch_packed.cpp, which runs the host walk below against a model), in the manner of
// lfx_encode_stages.h and lfx_merge_tree.h: nothing here needs a device.
//
//   out_off[0] = 0, out_off[i + 1] = round_up(out_off[i] + len[i], align), total = out_off[count - 1] + len[count - 1]
//
// as a two-level exclusive scan over the streams' terms — round_up(len, align), the last stream's own len:
//   level 1   one lane per stream, BPACK_WG streams per workgroup: the stream's offset inside its workgroup, the workgroup's sum
//   level 2   one workgroup over the workgroup sums, BPACK_SCAN per round with a carry: every workgroup's offset, the total
//   rebase    out_off = the workgroup's offset + the stream's offset inside it
#pragma once
#include <stdint.h>

#include "lfx_common.h"

namespace lfx {

constexpr uint32_t BPACK_WG = 256;          // streams per workgroup of the size and the rebase kernel
constexpr uint32_t BPACK_SCAN = 1024;       // workgroup sums per round of the second level (menc_scan_kernel's workgroup)
constexpr uint32_t BPACK_MAX_ALIGN = 4096;
constexpr uint32_t BPACK_MAX_COUNT = 0xFFFFFF00u;   // (a lane index of the last workgroup stays a uint32_t)

LFX_HD inline bool bpack_align_ok(uint32_t align) { return align >= 1 && align <= BPACK_MAX_ALIGN && (align & (align - 1)) == 0; }
LFX_HD inline uint64_t bpack_round_up(uint64_t x, uint32_t align) { return (x + (align - 1)) & ~(uint64_t)(align - 1); }
LFX_HD inline uint32_t bpack_nwg(uint32_t count) { return (uint32_t)(((uint64_t)count + BPACK_WG - 1) / BPACK_WG); }
LFX_HD inline uint32_t bpack_scan_rounds(uint32_t nwg) { return (uint32_t)(((uint64_t)nwg + BPACK_SCAN - 1) / BPACK_SCAN); }
// what stream s adds to the scan: the distance to the next stream's start; the last stream's length (the tail is not rounded)
LFX_HD inline uint64_t bpack_term(uint64_t len, uint32_t s, uint32_t count, uint32_t align) {
    return s + 1 == count ? len : bpack_round_up(len, align);
}

// The bits of a stream's blocks from `bit` on: the fold of offsets_batch_kernel.  WRITE: block_start[] on the way.
template <bool WRITE>
LFX_HD inline uint64_t bpack_fold(const BlockDesc *blocks, const BlockCodes *bc, uint32_t b0, uint32_t nb, uint64_t bit,
                                  uint64_t *block_start) {
    for (uint32_t b = b0; b < b0 + nb; ++b) {
        const BlockDesc bd = blocks[b];
        if (WRITE) block_start[b] = bit;
        if (bd.type == BT_RAW) { bit += 3; bit = (bit + 7) & ~7ull; bit += 32 + 8 * bd.in_len; }
        else if (bd.type != BT_ABSORBED) bit += bc[b].body_bits;
        if (bd.align_after) bit = (bit + 7) & ~7ull;
    }
    return bit;
}
// a stream's length: container header, blocks (the final one byte-aligns), trailer
LFX_HD inline uint64_t bpack_stream_len(const BlockDesc *blocks, const BlockCodes *bc, uint32_t b0, uint32_t nb, uint32_t hdr_len,
                                        uint32_t trailer_len) {
    return (bpack_fold<false>(blocks, bc, b0, nb, 8ull * hdr_len, nullptr) >> 3) + trailer_len;
}

// The host's part: no stream is longer than its bound, so sum = the sum of the terms of the bounds limits the total, the zero
// fill and every offset.  false: that sum does not fit 64 bits — the call is LFX_E_ARG before anything is launched, and the
// device's sums cannot wrap.
inline bool bpack_bound_sum(const uint64_t *bound, uint32_t count, uint32_t align, uint64_t *sum) {
    uint64_t acc = 0;
    for (uint32_t s = 0; s < count; ++s) {
        if (bound[s] > ~0ull - (align - 1)) return false;
        const uint64_t t = bpack_round_up(bound[s], align);     // (the last one rounded too: the bound of any prefix)
        if (acc > ~0ull - t) return false;
        acc += t;
    }
    *sum = acc;
    return true;
}

// The three kernels' arithmetic walked on the host, index for index (a wavefront's shuffle scan is a running sum here).
// local_off, wg_sum: the scratch the kernels use — count and bpack_nwg(count) words.
inline void bpack_host_size(const uint64_t *len, uint32_t count, uint32_t align, uint64_t *local_off, uint64_t *wg_sum) {
    for (uint32_t wg = 0; wg < bpack_nwg(count); ++wg) {
        uint64_t acc = 0;
        for (uint32_t t = 0; t < BPACK_WG; ++t) {
            const uint64_t s = (uint64_t)wg * BPACK_WG + t;
            if (s >= count) break;
            local_off[s] = acc;
            acc += bpack_term(len[s], (uint32_t)s, count, align);
        }
        wg_sum[wg] = acc;
    }
}
// → the total; wg_sum becomes its exclusive scan
inline uint64_t bpack_host_scan(uint64_t *wg_sum, uint32_t nwg) {
    uint64_t carry = 0;
    for (uint32_t r = 0; r < bpack_scan_rounds(nwg); ++r) {
        uint64_t acc = carry;
        for (uint32_t t = 0; t < BPACK_SCAN; ++t) {
            const uint64_t i = (uint64_t)r * BPACK_SCAN + t;
            if (i >= nwg) break;
            const uint64_t v = wg_sum[i];
            wg_sum[i] = acc;
            acc += v;
        }
        carry = acc;
    }
    return carry;
}
inline void bpack_host_rebase(const uint64_t *local_off, const uint64_t *wg_off, uint32_t count, uint64_t *out_off) {
    for (uint32_t s = 0; s < count; ++s) out_off[s] = wg_off[s / BPACK_WG] + local_off[s];
}

}  // namespace lfx
