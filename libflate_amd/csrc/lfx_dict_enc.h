// lfx_dict_enc.h — encoding with a preset dictionary: the dictionary's prefix table, the work list of the
// dictionary candidate kernel (lfx_dict_enc.hip) and the host arithmetic that makes it.  Internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "lfx_common.h"

namespace lfx {

// the prefix table of a dictionary's tail: 64-bit entries, open addressing; at most 32766 prefixes in 65536 slots (512 KiB)
constexpr uint32_t DICT_TAB_BITS = 16;
constexpr uint32_t DICT_TAB_SLOTS = 1u << DICT_TAB_BITS;
constexpr size_t DICT_TAB_BYTES = 8ull * DICT_TAB_SLOTS;

// the hash chain of a chain dictionary's tail: 16 bits per position of the 32 KiB window d_win (64 KiB)
constexpr size_t DICT_CHAIN_BYTES = 2ull * MAX_WINDOW;

// one workgroup of the dictionary candidate kernel: positions [p0, p0 + 256) of a primed chunk
struct DictItem {
    uint32_t chunk;
    uint32_t p0;
};
constexpr uint32_t DICT_ITEM_POS = 256;

// The work list: the positions p < min(end, window_size) of every primed chunk (CH_DICT), 256 to an item — a grid sized by
// positions, so that thousands of small records fill the GPU as well as one large chunk does.
inline void dict_items(const std::vector<ChunkDesc> &chunks, uint32_t window, std::vector<DictItem> &items) {
    items.clear();
    for (uint32_t ci = 0; ci < (uint32_t)chunks.size(); ci++) {
        const ChunkDesc &ch = chunks[ci];
        if (!(ch.flags & CH_DICT) || ch.len <= 3) continue;
        const uint64_t lim = std::min<uint64_t>(ch.len - 3, window);
        for (uint64_t p0 = 0; p0 < lim; p0 += DICT_ITEM_POS) items.push_back(DictItem{ci, (uint32_t)p0});
    }
}

// the table of the tail that ends the window d_win (lfx_dict::d_win) → tab (DICT_TAB_BYTES, cleared here)
int launch_dict_table(hipStream_t st, const uint8_t *d_win, uint32_t usable, uint64_t *tab);
// the chain of the same tail → cdt (DICT_CHAIN_BYTES, cleared here): cdt[MAX_WINDOW - usable + j] = the distance from the tail's
// position j to the most recent earlier one with the same 3 bytes, 0 where there is none or j > usable - 3
int launch_dict_chain(hipStream_t st, const uint8_t *d_win, uint32_t usable, uint16_t *cdt);
// behind the match stage: cd[p] of the items' positions where it is 0 ← the distance to the most recent occurrence in the
// dictionary, if that is within `window`
int launch_dict_cand(hipStream_t st, const uint8_t *in, const ChunkDesc *chunks, const DictItem *items, uint32_t nitems,
                     uint32_t window, const uint8_t *dict_end, uint32_t usable, const uint64_t *tab, uint16_t *cd);

}  // namespace lfx
