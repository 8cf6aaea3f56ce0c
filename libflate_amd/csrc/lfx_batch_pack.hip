// lfx_batch_pack.hip — the streams of a batch packed back to back (lfx_encode_batch_packed_device): §14's layout
// for ragged streams.  Behind the Huffman kernel every block's size is known, so every stream's length is too; the streams are
// then packed at their final offsets, and nothing is copied.  In the place of offsets_batch_kernel:
//   bpack_size_kernel    one lane per stream: the fold of offsets_batch_kernel from bit 8 * hdr_len → the stream's length, trailer
//                        included; then the first level of the scan over round_up(length, align): 64-lane shuffle scan, LDS
//                        across the four wavefronts → the stream's offset inside its workgroup's 256 streams, the workgroup's sum
//   menc_scan_kernel     (lfx_members_enc.hip, launch_scan_wg_sums) one workgroup: exclusive scan of the workgroup sums, the
//                        total, the status bit when it exceeds cap
//   bpack_rebase_kernel  one lane per stream: out_off = workgroup offset + local offset; block_start[] of its blocks and its end
//                        bit from there; out_off and the length into the stream's BatchStream record — pack and
//                        frame_batch_kernel then run unchanged; the {off, len} pair, and the caller's device table
// The arithmetic is lfx_batch_pack.h's.  Latency-bound kernels of a few thousand lanes: a lane's loads are its stream's record
// and two words per block, and no lane waits for another outside its workgroup's one barrier.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfx_batch_pack.h"
#include "lfx_device.h"

namespace lfx {

namespace {

__global__ __launch_bounds__(BPACK_WG) void bpack_size_kernel(const BatchStream *__restrict__ streams, uint32_t count,
                                                              const BlockDesc *__restrict__ blocks, const BlockCodes *__restrict__ bc,
                                                              uint32_t hdr_len, uint32_t trailer_len, uint32_t align,
                                                              uint64_t *__restrict__ local_off, uint64_t *__restrict__ slen,
                                                              uint64_t *__restrict__ wg_sum) {
    __shared__ uint64_t s_wsum[BPACK_WG / 64];
    const uint32_t s = blockIdx.x * BPACK_WG + threadIdx.x;
    uint64_t term = 0;
    if (s < count) {
        const uint64_t len = bpack_stream_len(blocks, bc, streams[s].first_block, streams[s].n_blocks, hdr_len, trailer_len);
        slen[s] = len;
        term = bpack_term(len, s, count, align);
    }
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

__global__ __launch_bounds__(BPACK_WG) void bpack_rebase_kernel(BatchStream *__restrict__ streams, uint32_t count,
                                                                const BlockDesc *__restrict__ blocks, const BlockCodes *__restrict__ bc,
                                                                uint32_t hdr_len, const uint64_t *__restrict__ local_off,
                                                                const uint64_t *__restrict__ slen, const uint64_t *__restrict__ wg_off,
                                                                uint64_t *__restrict__ block_start, uint64_t *__restrict__ stream_end,
                                                                uint64_t *__restrict__ pairs, uint64_t *__restrict__ table) {
    const uint32_t s = blockIdx.x * BPACK_WG + threadIdx.x;
    if (s >= count) return;
    const uint64_t out_off = wg_off[blockIdx.x] + local_off[s], len = slen[s];
    stream_end[s] = bpack_fold<true>(blocks, bc, streams[s].first_block, streams[s].n_blocks, 8 * (out_off + hdr_len), block_start);
    streams[s].out_off = out_off;
    streams[s].out_cap = len;
    pairs[2 * (uint64_t)s] = out_off;
    pairs[2 * (uint64_t)s + 1] = len;
    if (table) { table[2 * (uint64_t)s] = out_off; table[2 * (uint64_t)s + 1] = len; }
}

}  // namespace

#define LFX_LAUNCH_CHECK()                          \
    do {                                            \
        hipError_t e_ = hipGetLastError();          \
        if (e_ != hipSuccess) return (int)e_;       \
    } while (0)

int launch_batch_pack_layout(hipStream_t st, BatchStream *streams, uint32_t count, const BlockDesc *blocks, const BlockCodes *bc,
                             uint32_t hdr_len, uint32_t trailer_len, uint32_t align, uint64_t cap, uint64_t *local_off, uint64_t *slen,
                             uint64_t *wg_sum, uint64_t *block_start, uint64_t *stream_end, uint64_t *pairs, uint64_t *table,
                             EncodeResult *res) {
    const uint32_t nwg = bpack_nwg(count);
    if (!nwg) return 0;
    hipLaunchKernelGGL(bpack_size_kernel, dim3(nwg), dim3(BPACK_WG), 0, st, streams, count, blocks, bc, hdr_len, trailer_len, align,
                       local_off, slen, wg_sum);
    LFX_LAUNCH_CHECK();
    if (int e = launch_scan_wg_sums(st, wg_sum, nwg, cap, res)) return e;
    hipLaunchKernelGGL(bpack_rebase_kernel, dim3(nwg), dim3(BPACK_WG), 0, st, streams, count, blocks, bc, hdr_len, local_off, slen, wg_sum,
                       block_start, stream_end, pairs, table);
    LFX_LAUNCH_CHECK();
    return 0;
}

}  // namespace lfx
