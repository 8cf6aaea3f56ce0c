// lfx_batch_unpack.hip — the streams of a batch decoded back to back (lfx_decode_batch_packed_device): §26's
// layout with the decoded sizes of the size half (§15) in the place of the encoded lengths.  Between the size half and the
// decode half of the call:
//   bunpack_size_kernel    one lane per stream: the first level of the scan over bpack_term(size, s, count, align) — 64-lane
//                          shuffle scan, LDS across the four wavefronts → the stream's offset inside its workgroup's 256
//                          streams, the workgroup's sum
//   menc_scan_kernel       (lfx_members_enc.hip, launch_scan_wg_sums) one workgroup: exclusive scan of the workgroup sums
//   bunpack_rebase_kernel  one lane per stream: out_off = workgroup offset + local offset; out_off and out_cap = size into the
//                          stream's DecStream record, which the checksum-ranges and the trailer kernel read in place; the
//                          {off, len} pair for the host's one copy-back, the caller's device table, and — the last stream's
//                          lane — the total
// The arithmetic is lfx_batch_pack.h's, the words' places are lfx_batch_unpack.h's.  Latency-bound kernels of a few thousand
// lanes: a lane loads three words and stores at most seven, and no lane waits for another outside its workgroup's one barrier.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfx_batch_unpack.h"
#include "lfx_decode.h"
#include "lfx_device.h"

namespace lfx {

static_assert(sizeof(EncodeResult) == 8 * BUNPACK_RES_WORDS, "the scan's result record in the scratch");

namespace {

__global__ __launch_bounds__(BPACK_WG) void bunpack_size_kernel(const uint64_t *__restrict__ size, uint32_t count, uint32_t align,
                                                                uint64_t *__restrict__ local_off, uint64_t *__restrict__ wg_sum) {
    __shared__ uint64_t s_wsum[BPACK_WG / 64];
    const uint32_t s = blockIdx.x * BPACK_WG + threadIdx.x;
    const uint64_t term = s < count ? bpack_term(size[s], s, count, align) : 0;
    // exclusive scan over the workgroup: inclusive shuffle scan per wavefront, the wavefronts' sums through LDS
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t x = term;
    for (int o = 1; o < 64; o <<= 1) { const uint64_t y = __shfl_up(x, o); if ((int)lane >= o) x += y; }
    if (lane == 63) s_wsum[wave] = x;
    __syncthreads();
    uint64_t pre = 0;
    for (uint32_t w = 0; w < wave; ++w) pre += s_wsum[w];
    if (s < count) local_off[s] = pre + x - term;
    if (threadIdx.x == BPACK_WG - 1) wg_sum[blockIdx.x] = pre + x;
}

__global__ __launch_bounds__(BPACK_WG) void bunpack_rebase_kernel(DecStream *__restrict__ streams, uint32_t count,
                                                                  const uint64_t *__restrict__ size, const uint64_t *__restrict__ local_off,
                                                                  const uint64_t *__restrict__ wg_off, uint64_t *__restrict__ back,
                                                                  uint64_t *__restrict__ table) {
    const uint32_t s = blockIdx.x * BPACK_WG + threadIdx.x;
    if (s >= count) return;
    const uint64_t out_off = wg_off[blockIdx.x] + local_off[s], len = size[s];
    streams[s].out_off = out_off;
    streams[s].out_cap = len;
    back[2 * (uint64_t)s] = out_off;
    back[2 * (uint64_t)s + 1] = len;
    if (table) { table[2 * (uint64_t)s] = out_off; table[2 * (uint64_t)s + 1] = len; }
    if (s + 1 == count) back[2 * (uint64_t)count] = out_off + len;
}

}  // namespace

#define LFX_LAUNCH_CHECK()                          \
    do {                                            \
        hipError_t e_ = hipGetLastError();          \
        if (e_ != hipSuccess) return (int)e_;       \
    } while (0)

int launch_batch_unpack_layout(hipStream_t st, DecStream *streams, uint32_t count, uint32_t align, uint64_t *scratch, uint64_t *table) {
    const uint32_t nwg = bpack_nwg(count);
    if (!nwg) return 0;
    const BunpackScratch w = bunpack_scratch(count);
    hipLaunchKernelGGL(bunpack_size_kernel, dim3(nwg), dim3(BPACK_WG), 0, st, scratch + w.size, count, align, scratch + w.local_off,
                       scratch + w.wg_sum);
    LFX_LAUNCH_CHECK();
    // (the second level's own total and capacity bit are not read: the rebase kernel states the total, the host compares it)
    if (int e = launch_scan_wg_sums(st, scratch + w.wg_sum, nwg, ~0ull, (EncodeResult *)(scratch + w.res))) return e;
    hipLaunchKernelGGL(bunpack_rebase_kernel, dim3(nwg), dim3(BPACK_WG), 0, st, streams, count, scratch + w.size, scratch + w.local_off,
                       scratch + w.wg_sum, scratch + w.pairs, table);
    LFX_LAUNCH_CHECK();
    return 0;
}

}  // namespace lfx
