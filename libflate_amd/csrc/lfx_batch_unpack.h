// lfx_batch_unpack.h — lfx_decode_batch_packed_device (include/lfx.h): a batch decoded back to back, placed by
// the decoded sizes.  The layout is §26's and its arithmetic is lfx_batch_pack.h's — the term, the two scan levels, the rebase —
// with a stream's decoded size in the place of its encoded length.  What the decode adds, stated ONCE for the HIP kernels
// (lfx_batch_unpack.hip), for the entry point (lfx_decode.cpp) and for the host test (tests/c/batch_unpacked.cpp): where the
// kernels' words lie in the call's scratch, and what the rebase kernel leaves for the host's one copy-back.  Nothing here needs
// a device.
#pragma once
#include <stdint.h>

#include "lfx_batch_pack.h"

namespace lfx {

// The call's scratch, in 64-bit words from its base: the sizes the host uploads, the two scan levels' words, the second
// level's result record, and the block that comes back in one transfer — count pairs {off, len}, then the total.
struct BunpackScratch {
    uint64_t size, local_off, wg_sum, res, pairs, words;
};
constexpr uint32_t BUNPACK_RES_WORDS = 4;       // sizeof(EncodeResult) / 8 (lfx_batch_unpack.hip asserts it)
LFX_HD inline uint64_t bunpack_back_words(uint32_t count) { return 2 * (uint64_t)count + 1; }
LFX_HD inline BunpackScratch bunpack_scratch(uint32_t count) {
    BunpackScratch s;
    s.size = 0;
    s.local_off = s.size + count;
    s.wg_sum = s.local_off + count;
    s.res = s.wg_sum + bpack_nwg(count);
    s.pairs = s.res + BUNPACK_RES_WORDS;
    s.words = s.pairs + bunpack_back_words(count);
    return s;
}

// The three kernels walked on the host, index for index: back[2 s] = out_off[s], back[2 s + 1] = size[s], back[2 count] = the
// total, which the rebase lane of the LAST stream forms from its own offset and size (no second sum).  local_off, wg_sum: the
// scratch the kernels use — count and bpack_nwg(count) words.  count >= 1.
inline void bunpack_host_layout(const uint64_t *size, uint32_t count, uint32_t align, uint64_t *local_off, uint64_t *wg_sum,
                                uint64_t *back) {
    bpack_host_size(size, count, align, local_off, wg_sum);
    (void)bpack_host_scan(wg_sum, bpack_nwg(count));
    for (uint32_t s = 0; s < count; ++s) {
        const uint64_t out_off = wg_sum[s / BPACK_WG] + local_off[s];
        back[2 * (uint64_t)s] = out_off;
        back[2 * (uint64_t)s + 1] = size[s];
        if (s + 1 == count) back[2 * (uint64_t)count] = out_off + size[s];
    }
}

}  // namespace lfx
