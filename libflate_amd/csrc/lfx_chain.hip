// lfx_chain.hip — ChainLz77Encoder's candidate refinement (LFX_LZ77_CHAIN), for gfx950.
//
// The match stage leaves cd[p] = distance to the most recent earlier occurrence of p's 3-byte prefix inside p's chunk, 0 where
// there is none within window_size — for EVERY position p < end, whatever the parse will visit (DefaultLz77Encoder::flush
// inserts every position once, in order).  That array is the hash chain: q1 = p - cd[p] holds p's prefix, so q2 = q1 - cd[q1] is
// the next older occurrence, and so on; cd[q] == 0 says that any older occurrence is farther than the window from q, hence from
// p.  This kernel walks the first `depth` links of every position's chain, measures each candidate
// (longest_common_prefix, default.rs:122-129: capped by max_length and by the end of the chunk) and writes the distance of the
// longest — among equal lengths the nearest — to a SECOND array: other positions' chains run through cd while this one is
// written.  The parse then reads the second array; all it needs of a candidate is "a match exactly when it is not 0", the
// lengths it computes itself.
//
// One workgroup per tile of positions [p0, p0 + TILE) of one chunk.  It stages the bytes [p0 - W, p0 + TILE + max_length) and
// the candidates of [p0 - W, p0 + TILE) in LDS, so that a hop (one 16-bit read) and a compare step (8 bytes at the position, 8
// at the candidate) never leave the CU: a chain is a string of dependent reads, 64 cycles apart in LDS and several hundred
// through L2.  Two instances: the window instance (W up to 32768: 145 KB, one workgroup of 16 wavefronts per CU) and the small
// one for calls whose chunks all fit one tile of 8192 (a batch of records: position 0 has no window in front).
//
// Divergence.  Chains differ in length from lane to lane, and candidates in how far they match.  A lane owns every THREADS-th
// position of the tile and runs ONE loop over a three-state machine — fetch a position / compare 8 bytes / hop — one state's step
// per trip: a lane whose position is settled fetches its next one while its neighbours still compare or hop, so a wavefront runs as
// long as its busiest lane's total over 16 positions (32 in the small instance), not as the sum of every position's longest
// chain.  Two cuts that change no result: a candidate can only win with a length above the best so far, so it is dropped at
// once when its byte at that index differs; and a walk ends when the best length is all the position can have.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfx_chain.h"
#include "lfx_common.h"

namespace lfx {

namespace {

// 8 bytes at LDS byte offset off, from aligned dword reads
__device__ __forceinline__ uint64_t lds8(const uint32_t *w, uint32_t off) {
    const uint32_t i = off >> 2, sh = off & 3;
    const uint32_t w0 = w[i], w1 = w[i + 1], w2 = w[i + 2];
    return (uint64_t)__builtin_amdgcn_alignbyte(w1, w0, sh) | (uint64_t)__builtin_amdgcn_alignbyte(w2, w1, sh) << 32;
}
__device__ __forceinline__ uint32_t lds1(const uint32_t *w, uint32_t off) { return (w[off >> 2] >> ((off & 3) * 8)) & 0xFFu; }

template <uint32_t TILE, uint32_t WCAP, uint32_t THREADS>
__global__ __launch_bounds__(THREADS) void chain_kernel(const uint8_t *__restrict__ in, const ChunkDesc *__restrict__ chunks,
                                                        const ChainItem *__restrict__ items, uint32_t window, uint32_t max_len,
                                                        uint32_t depth, const uint16_t *__restrict__ cd, uint16_t *__restrict__ cd2) {
    // bytes [lo, hi): at most WCAP + TILE + MAX_LENGTH, + the byte phase of lo on the dword grid (3), + what the last compare
    // step and its three-dword read reach past the last byte that counts (11)
    constexpr uint32_t BW = (WCAP + TILE + MAX_LENGTH + 3 + 11 + 3) / 4 + 1;
    constexpr uint32_t CW = (WCAP + TILE + 1 + 1) / 2 + 1;          // candidates [lo, p1), + their phase on the dword grid
    static_assert(4 * (BW + CW) <= 160 * 1024, "one workgroup's LDS");
    __shared__ uint32_t s_b[BW];
    __shared__ uint32_t s_c[CW];
    const ChainItem it = items[blockIdx.x];
    const ChunkDesc ch = chunks[it.chunk];
    const uint32_t n = (uint32_t)ch.len;
    const uint32_t end = (n > 3 ? n : 3) - 3;                     // default.rs:75
    const uint32_t p0 = it.p0;
    if (p0 >= end) return;                                        // (never listed)
    if (max_len > MAX_LENGTH) max_len = MAX_LENGTH;               // (the options' normal form already; the LDS is sized by it)
    const uint32_t wst = window < WCAP ? window : WCAP;
    const uint32_t lo = p0 > wst ? p0 - wst : 0u;
    const uint32_t p1 = p0 + TILE < end ? p0 + TILE : end;        // positions [p0, p1)
    const uint32_t hi = (uint64_t)p0 + TILE + max_len < n ? p0 + TILE + max_len : n;
    const uint32_t tid = threadIdx.x;
    // ---- stage the bytes and the candidates on their own dword grids: position q's byte sits at LDS byte q - lo + sh, its
    //      candidate at entry q - lo + csh.  (The dwords that hold the first and the last byte may reach up to three bytes
    //      outside [lo, hi), as the parse's reads do; a dword that holds no byte of it is not read.)
    const uint64_t a0 = (uint64_t)(in + ch.in_off) + lo;
    const uint32_t sh = (uint32_t)a0 & 3;
    const uint32_t *gw = (const uint32_t *)(a0 - sh);
    const uint32_t ndw = (hi - lo + sh + 3) >> 2;
    for (uint32_t k = tid; k < ndw && k < BW; k += THREADS) s_b[k] = gw[k];
    const uint64_t e0 = ch.in_off + lo;
    const uint32_t csh = (uint32_t)e0 & 1;
    const uint32_t *gc = (const uint32_t *)(cd + (e0 - csh));
    const uint32_t ncw = (p1 - lo + csh + 1) >> 1;
    for (uint32_t k = tid; k < ncw && k < CW; k += THREADS) s_c[k] = gc[k];
    __syncthreads();
    const uint16_t *c16 = (const uint16_t *)s_c;
    const uint32_t boff = sh - lo, coff = csh - lo;              // (unsigned wrap: q + boff = q - lo + sh)
    uint16_t *out = cd2 + ch.in_off;

    enum : uint32_t { FETCH = 0, COMPARE = 1, HOP = 2 };
    uint32_t state = FETCH;
    uint32_t p = p0 + tid;
    uint32_t c = 0, cur = 0, best = 0, bestd = 0, left = 0, lim = 0;
    for (;;) {
        if (state == FETCH) {
            if (p >= p1) break;
            const uint32_t d = c16[p + coff];
            if (d == 0 || d > p) {                                // no candidate (d > p: never, a distance stays inside the chunk)
                out[p] = 0;
                p += THREADS;
                continue;
            }
            c = p - d;
            left = depth;
            best = 0;
            bestd = d;
            cur = 3;
            lim = n - p < max_len ? n - p : max_len;              // (>= 4: p < end)
            state = c >= lo ? COMPARE : FETCH;
            if (state == FETCH) { out[p] = (uint16_t)d; p += THREADS; }   // (never: the first candidate is within the window staged)
            continue;
        }
        if (state == COMPARE) {
            const uint64_t x = lds8(s_b, p + cur + boff) ^ lds8(s_b, c + cur + boff);
            const uint32_t m = x ? (uint32_t)__builtin_ctzll(x) >> 3 : 8u;
            cur += m;
            if (m == 8 && cur < lim) continue;
            if (cur > lim) cur = lim;
            if (cur > best) { best = cur; bestd = p - c; }
            --left;
            state = HOP;
        }
        // HOP: the next older occurrence, unless the walk is over
        bool fin = best >= lim || left == 0;
        if (!fin) {
            const uint32_t dq = c16[c + coff];
            fin = dq == 0 || dq > c;
            if (!fin) {
                const uint32_t c2 = c - dq;
                fin = p - c2 > window || c2 < lo;                 // (c2 < lo: never, lo <= p0 - min(window, WCAP))
                if (!fin) {
                    c = c2;
                    // longer than `best` only if the byte at that index matches too (best < lim: p + best < n)
                    if (lds1(s_b, c + best + boff) == lds1(s_b, p + best + boff)) { cur = 3; state = COMPARE; }
                    else --left;                                  // (a candidate all the same: it counts towards the depth)
                }
            }
        }
        if (fin) {
            out[p] = (uint16_t)bestd;
            p += THREADS;
            state = FETCH;
        }
    }
}

}  // namespace

int launch_chain(hipStream_t st, const uint8_t *in, uint64_t in_bytes, const ChunkDesc *chunks, const ChainItem *items,
                 uint32_t nitems, bool small, uint32_t window, uint32_t max_len, uint32_t depth, const uint16_t *cd, uint16_t *cd2) {
    (void)in_bytes;
    if (!nitems) return 0;
    if (small)
        hipLaunchKernelGGL((chain_kernel<CHAIN_TILE_SMALL, 0, 256>), dim3(nitems), dim3(256), 0, st, in, chunks, items, window, max_len,
                           depth, cd, cd2);
    else
        hipLaunchKernelGGL((chain_kernel<CHAIN_TILE, MAX_WINDOW, 1024>), dim3(nitems), dim3(1024), 0, st, in, chunks, items, window,
                           max_len, depth, cd, cd2);
    return (int)hipGetLastError();
}

}  // namespace lfx
