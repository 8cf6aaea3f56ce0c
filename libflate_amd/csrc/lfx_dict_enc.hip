// lfx_dict_enc.hip — the encode half of a preset dictionary, for gfx950: the dictionary's prefix table and the
// kernel that fills the candidates the match stage leaves open at the head of a primed chunk.
//
// The contract (include/lfx.h): the first chunk of a stream is parsed as DefaultLz77Encoder::flush (default.rs:69-109) would
// parse T ‖ buf with every position of T already in its prefix table.  flush inserts every position exactly once, in order, so
// the candidate of chunk position p is the most recent earlier occurrence of its 3-byte prefix in T ‖ buf.  The match stage has
// answered that for occurrences inside the chunk; where it found none (cd[p] == 0, p < window_size: an occurrence inside the
// chunk is never out of reach there) the most recent one in T is the candidate: the two positions whose prefix straddles the
// boundary (|T|-1, then |T|-2: they depend on the chunk's first bytes), then the last position j <= |T|-3 of the table.
//
// The table: open addressing over DICT_TAB_SLOTS 64-bit entries (1 << 56 | prefix << 32 | position), at most 32766 of them
// in 65536 slots.  An insert claims the first empty slot of its probe sequence with a compare-and-swap — a slot never changes
// its prefix afterwards — and raises the position with atomicMax; a lookup probes until it meets its prefix or an empty slot.
// Exact: a stored entry carries its whole prefix, and a prefix that was inserted is met before any empty slot.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfx_common.h"
#include "lfx_dict_enc.h"
#include "lfx_dict_tab.h"

namespace lfx {

namespace {

// one thread per position j <= usable - 3 of the tail (win + MAX_WINDOW - usable is its first byte)
__global__ __launch_bounds__(256) void dict_table_kernel(const uint8_t *__restrict__ win, uint32_t usable, unsigned long long *__restrict__ tab) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (usable < 3 || j > usable - 3) return;
    const uint8_t *t = win + (MAX_WINDOW - usable) + j;
    const uint32_t prefix = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16;
    const unsigned long long mine = TAB_USED | (unsigned long long)prefix << 32 | j;
    uint32_t h = tab_hash(prefix);
    for (uint32_t probe = 0; probe < DICT_TAB_SLOTS; ++probe, h = (h + 1) & (DICT_TAB_SLOTS - 1)) {
        unsigned long long cur = tab[h];
        if (cur == 0) cur = atomicCAS(&tab[h], 0ull, mine);       // (0: the slot is this prefix's now, with this position)
        if (cur == 0) return;
        if ((uint32_t)(cur >> 32) == (uint32_t)(mine >> 32)) { atomicMax(&tab[h], mine); return; }
    }
}

// The dictionary's own hash chain: cdt[MAX_WINDOW - usable + j] = the distance from position j <= usable - 3
// of the tail to the most recent earlier position with the same 3 bytes, 0 where there is none — on the grid of d_win, so
// that a chunk position's offset in front of the chunk indexes the bytes and the links alike.  Complete: no window cuts it.
// Built once per dictionary, so the plainest exact method serves: a workgroup keeps the prefixes of every position up to its
// own 1024 in LDS, and each thread scans back from its position to the first equal one.
constexpr uint32_t DICT_CHAIN_THREADS = 1024;
__global__ __launch_bounds__(DICT_CHAIN_THREADS) void dict_chain_kernel(const uint8_t *__restrict__ win, uint32_t usable,
                                                                        uint16_t *__restrict__ cdt) {
    __shared__ uint32_t s_key[MAX_WINDOW];
    if (usable < 3) return;
    const uint32_t npos = usable - 2;                              // positions [0, usable - 3]
    const uint32_t j0 = blockIdx.x * DICT_CHAIN_THREADS;
    const uint32_t jtop = j0 + DICT_CHAIN_THREADS < npos ? j0 + DICT_CHAIN_THREADS : npos;
    const uint8_t *t = win + (MAX_WINDOW - usable);
    for (uint32_t k = threadIdx.x; k < jtop; k += DICT_CHAIN_THREADS)
        s_key[k] = (uint32_t)t[k] | (uint32_t)t[k + 1] << 8 | (uint32_t)t[k + 2] << 16;   // (k + 2 <= usable - 1)
    __syncthreads();
    const uint32_t j = j0 + threadIdx.x;
    if (j >= npos) return;
    const uint32_t key = s_key[j];
    uint32_t d = 0;
    for (uint32_t k = j; k-- > 0;)
        if (s_key[k] == key) { d = j - k; break; }
    cdt[MAX_WINDOW - usable + j] = (uint16_t)d;                    // (d <= 32765)
}

// One workgroup per item: 256 positions of one primed chunk, from p0 on.
__global__ __launch_bounds__(256) void dict_cand_kernel(const uint8_t *__restrict__ in, const ChunkDesc *__restrict__ chunks,
                                                        const DictItem *__restrict__ items, uint32_t window,
                                                        const uint8_t *__restrict__ dict_end, uint32_t usable,
                                                        const unsigned long long *__restrict__ tab, uint16_t *__restrict__ cd) {
    const DictItem it = items[blockIdx.x];
    const ChunkDesc ch = chunks[it.chunk];
    const uint32_t n = (uint32_t)ch.len;
    const uint32_t end = (n > 3 ? n : 3) - 3;                     // default.rs:75 in the chunk's own positions
    const uint32_t lim = end < window ? end : window;             // a position from `window` on cannot reach the dictionary
    const uint32_t p = it.p0 + threadIdx.x;
    if (p >= lim) return;
    uint16_t *c = cd + ch.in_off + p;
    if (*c != 0) return;                                          // an occurrence inside the chunk is the more recent one
    const uint8_t *b = in + ch.in_off;
    const uint32_t b0 = b[p], b1 = b[p + 1], b2 = b[p + 2];       // (p + 2 < n: p < end)
    uint32_t j = 0xFFFFFFFFu;                                     // position in T
    if (usable >= 1 && b0 == dict_end[-1] && b1 == b[0] && b2 == b[1]) j = usable - 1;
    else if (usable >= 2 && b0 == dict_end[-2] && b1 == dict_end[-1] && b2 == b[0]) j = usable - 2;
    else if (usable >= 3) j = tab_lookup(tab, b0 | b1 << 8 | b2 << 16);
    if (j == 0xFFFFFFFFu) return;
    const uint32_t dist = p + usable - j;
    if (dist <= window) *c = (uint16_t)dist;                      // (32768 fits; farther: a literal, no older occurrence is tried)
}

}  // namespace

int launch_dict_table(hipStream_t st, const uint8_t *d_win, uint32_t usable, uint64_t *tab) {
    if (hipMemsetAsync(tab, 0, DICT_TAB_BYTES, st) != hipSuccess) return (int)hipGetLastError();
    if (usable < 3) return 0;
    hipLaunchKernelGGL(dict_table_kernel, dim3((usable - 2 + 255) / 256), dim3(256), 0, st, d_win, usable, (unsigned long long *)tab);
    return (int)hipGetLastError();
}

int launch_dict_chain(hipStream_t st, const uint8_t *d_win, uint32_t usable, uint16_t *cdt) {
    if (hipMemsetAsync(cdt, 0, DICT_CHAIN_BYTES, st) != hipSuccess) return (int)hipGetLastError();
    if (usable < 3) return 0;
    hipLaunchKernelGGL(dict_chain_kernel, dim3((usable - 2 + DICT_CHAIN_THREADS - 1) / DICT_CHAIN_THREADS), dim3(DICT_CHAIN_THREADS), 0, st,
                       d_win, usable, cdt);
    return (int)hipGetLastError();
}

int launch_dict_cand(hipStream_t st, const uint8_t *in, const ChunkDesc *chunks, const DictItem *items, uint32_t nitems,
                     uint32_t window, const uint8_t *dict_end, uint32_t usable, const uint64_t *tab, uint16_t *cd) {
    if (!nitems) return 0;
    hipLaunchKernelGGL(dict_cand_kernel, dim3(nitems), dim3(256), 0, st, in, chunks, items, window, dict_end, usable,
                       (const unsigned long long *)tab, cd);
    return (int)hipGetLastError();
}

}  // namespace lfx
