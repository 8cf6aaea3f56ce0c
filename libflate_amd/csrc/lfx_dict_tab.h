// lfx_dict_tab.h — the lookup side of a dictionary's prefix table, shared by the dictionary candidate kernel
// (lfx_dict_enc.hip, which also builds the table) and the dictionary instance of the chain kernel (lfx_chain.hip, §21).
// Device code.  Internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfx_dict_enc.h"

namespace lfx {

// an entry: 1 << 56 | prefix << 32 | position; 0: the slot is empty
constexpr uint64_t TAB_USED = 1ull << 56;
__device__ __forceinline__ uint32_t tab_hash(uint32_t prefix) { return (prefix * 0x9E3779B1u) >> (32 - DICT_TAB_BITS); }

// → the last position j <= |T|-3 of the tail that holds `prefix`, or 0xFFFFFFFF
__device__ __forceinline__ uint32_t tab_lookup(const unsigned long long *__restrict__ tab, uint32_t prefix) {
    const uint32_t key = (uint32_t)(TAB_USED >> 32) | prefix;
    uint32_t h = tab_hash(prefix);
    for (uint32_t probe = 0; probe < DICT_TAB_SLOTS; ++probe, h = (h + 1) & (DICT_TAB_SLOTS - 1)) {
        const unsigned long long cur = tab[h];
        if (cur == 0) return 0xFFFFFFFFu;
        if ((uint32_t)(cur >> 32) == key) return (uint32_t)cur;
    }
    return 0xFFFFFFFFu;
}

}  // namespace lfx
