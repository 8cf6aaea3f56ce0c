// lfx_members.hip — the candidate finder of the multi-member gzip decode (lfx_decode_members_device, lfx_decode.cpp).
//
// A gzip member starts with ID1 ID2 CM = 1f 8b 08 (gzip.rs:398-405) and a FLG byte; its three reserved bits are clear in
// every member a gzip writer makes.  The finder marks every offset p of the input with those four bytes (p + 3 < n) and
// compacts the offsets in input order.  Two passes over tiles of MEMBER_TILE bytes: member_cand_count_kernel counts a tile's
// candidates, the host turns the counts into output positions (and leaves out tiles denser than any real sequence of
// members), member_cand_emit_kernel writes them.  Memory-bound: one 16-byte load a lane and chunk, plus the dword behind
// it for the patterns that cross into the next chunk.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfx_common.h"
#include "lfx_decode.h"

namespace lfx {

namespace {

constexpr uint32_t MT_THREADS = 256;
constexpr uint32_t MT_CHUNKS = MEMBER_TILE / (16 * MT_THREADS);   // 16-byte chunks per lane and tile
static_assert(MT_CHUNKS * 16 * MT_THREADS == MEMBER_TILE, "tile geometry");

// bit i of the result: a candidate starts at byte 16 * chunk + i
__device__ __forceinline__ uint32_t chunk_mask(const uint8_t *__restrict__ in, uint64_t n, uint64_t chunk) {
    const uint64_t p0 = chunk * 16;
    if (p0 >= n) return 0;
    uint32_t w[5];
    if ((((uintptr_t)in) & 15) == 0 && p0 + 20 <= n) {
        const uint4 v = *(const uint4 *)(in + p0);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        w[4] = *(const uint32_t *)(in + p0 + 16);
    } else {
        // the end of the input (or an input that is not 16-byte aligned): byte loads inside [0, n) only
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            uint32_t x = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const uint64_t p = p0 + 4 * k + b;
                x |= (p < n ? (uint32_t)in[p] : 0u) << (8 * b);
            }
            w[k] = x;
        }
    }
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const uint32_t lo = w[i >> 2], hi = w[(i >> 2) + 1];
        const uint32_t x = (i & 3) ? (lo >> (8 * (i & 3))) | (hi << (32 - 8 * (i & 3))) : lo;   // bytes i .. i + 3
        m |= (uint32_t)((x & 0xE0FFFFFFu) == 0x00088B1Fu) << i;
    }
    if (p0 + 19 >= n) {    // a candidate needs its FLG byte inside the input
        const uint64_t ok = n - p0 >= 4 ? n - p0 - 3 : 0;      // positions i < ok have p0 + i + 3 < n
        m &= ok >= 16 ? 0xFFFFu : (1u << ok) - 1u;
    }
    return m;
}

__global__ __launch_bounds__(MT_THREADS) void member_cand_count_kernel(const uint8_t *__restrict__ in, uint64_t n,
                                                                       uint32_t *__restrict__ tile_count) {
    __shared__ uint32_t s_sum[MT_THREADS / 64];
    const uint32_t tid = threadIdx.x;
    const uint64_t c0 = (uint64_t)blockIdx.x * (MEMBER_TILE / 16);
    uint32_t m[MT_CHUNKS];
#pragma unroll
    for (uint32_t k = 0; k < MT_CHUNKS; ++k) m[k] = chunk_mask(in, n, c0 + k * MT_THREADS + tid);
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t k = 0; k < MT_CHUNKS; ++k) cnt += __popc(m[k]);
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((tid & 63) == 0) s_sum[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < MT_THREADS / 64; ++w) t += s_sum[w];
        tile_count[blockIdx.x] = t;
    }
}

// tile_pos[t]: where tile t's candidates go in `out` (MEMBER_SKIP: the tile is left out); out holds `cap` entries
__global__ __launch_bounds__(MT_THREADS) void member_cand_emit_kernel(const uint8_t *__restrict__ in, uint64_t n,
                                                                      const uint64_t *__restrict__ tile_pos,
                                                                      uint64_t *__restrict__ out, uint64_t cap) {
    __shared__ uint32_t s_sum[MT_THREADS / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t pos = tile_pos[blockIdx.x];
    if (pos == MEMBER_SKIP) return;
    const uint64_t c0 = (uint64_t)blockIdx.x * (MEMBER_TILE / 16);
    uint32_t m[MT_CHUNKS];
#pragma unroll
    for (uint32_t k = 0; k < MT_CHUNKS; ++k) m[k] = chunk_mask(in, n, c0 + k * MT_THREADS + tid);
    // chunk k * MT_THREADS + tid: input order is (k, tid) — one ordered compaction of the workgroup per k
#pragma unroll
    for (uint32_t k = 0; k < MT_CHUNKS; ++k) {
        const uint32_t cnt = __popc(m[k]);
        uint32_t x = cnt;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t a = __shfl_up(x, o);
            if ((int)lane >= o) x += a;
        }
        if (lane == 63) s_sum[wave] = x;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < MT_THREADS / 64; ++w) { before += w < wave ? s_sum[w] : 0u; total += s_sum[w]; }
        uint64_t at = pos + before + x - cnt;
        const uint64_t base = (c0 + (uint64_t)k * MT_THREADS + tid) * 16;
        for (uint32_t bits = m[k]; bits; bits &= bits - 1, ++at)
            if (at < cap) out[at] = base + (uint32_t)__ffs(bits) - 1;
        pos += total;
        __syncthreads();
    }
}

}  // namespace

#define LFX_LAUNCH_CHECK()                          \
    do {                                            \
        hipError_t e_ = hipGetLastError();          \
        if (e_ != hipSuccess) return (int)e_;       \
    } while (0)

int launch_member_count(hipStream_t st, const uint8_t *in, uint64_t n, uint32_t *tile_count) {
    const uint64_t ntiles = member_tiles(n);
    if (!ntiles) return 0;
    if (ntiles > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(member_cand_count_kernel, dim3((uint32_t)ntiles), dim3(MT_THREADS), 0, st, in, n, tile_count);
    LFX_LAUNCH_CHECK();
    return 0;
}

int launch_member_emit(hipStream_t st, const uint8_t *in, uint64_t n, const uint64_t *tile_pos, uint64_t *out, uint64_t cap) {
    const uint64_t ntiles = member_tiles(n);
    if (!ntiles) return 0;
    if (ntiles > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(member_cand_emit_kernel, dim3((uint32_t)ntiles), dim3(MT_THREADS), 0, st, in, n, tile_pos, out, cap);
    LFX_LAUNCH_CHECK();
    return 0;
}

}  // namespace lfx
