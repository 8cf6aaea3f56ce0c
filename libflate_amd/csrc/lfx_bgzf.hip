// lfx_bgzf.hip — the two kernels of the BGZF reads by virtual offset (lfx_bgzf_read_device).
//
// bgzf_hop_kernel: one wavefront per read follows the BSIZE chain from the read's coffset (lfx_bgzf.h: bgzf_walk).  The chain
// is serial — a block's start is known once the BSIZE in front of it has arrived — so a hop costs one memory latency and
// nothing else counts: lanes 0 .. 21 load one byte each of the 22-byte window around the next block start (the ISIZE of the
// block that ends there and the header of the one that begins), v_readlane hands the bytes to the whole wavefront, and the
// walk's decisions are scalar.  Lane 0 writes the segment list and the result.
//
// bgzf_gather_kernel: one workgroup per piece (at most 16 KiB) of a (read, block) segment copies the wanted bytes from the
// scratch the blocks were decoded into to the read's output range: the destination in aligned 16-byte stores, each made of
// five aligned dword loads of the source and a byte funnel shift, the bytes in front and behind one by one.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfx_bgzf.h"

namespace lfx {

namespace {

constexpr uint32_t HOP_THREADS = 256;      // four reads a workgroup
constexpr uint32_t GATHER_THREADS = 256;
constexpr uint32_t GATHER_UNROLL = 4;      // 16-byte chunks a lane loads before it stores any: one piece in one round

__global__ __launch_bounds__(HOP_THREADS) void bgzf_hop_kernel(const uint8_t *__restrict__ in, uint64_t in_base, uint64_t n,
                                                               uint32_t count, const lfx_bgzf_read *__restrict__ reads,
                                                               const uint64_t *__restrict__ seg_off, BgzfSeg *__restrict__ segs,
                                                               BgzfWalk *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t ridx = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (HOP_THREADS / 64) + (threadIdx.x >> 6)));
    if (ridx >= count) return;
    const lfx_bgzf_read r = reads[ridx];
    const uint64_t lo = in_base, hi = in_base + n;
    uint64_t slot = 0, slot_end = 0;
    if (segs) { slot = seg_off[ridx]; slot_end = seg_off[ridx + 1]; }
    auto fetch = [&](uint64_t p, uint8_t *w) {
        const uint64_t a = p + lane - 4;           // (p + lane < 4 wraps around and fails the range test)
        uint32_t b = 0;
        if (lane < BGZF_WINDOW && a >= lo && a < hi) b = in[a - lo];
#pragma unroll
        for (uint32_t k = 0; k < BGZF_WINDOW; ++k) w[k] = (uint8_t)__builtin_amdgcn_readlane((int)b, (int)k);
    };
    auto emit = [&](const BgzfSeg &s) {
        if (slot < slot_end && lane == 0) segs[slot] = s;
        ++slot;
    };
    BgzfWalk o;
    bgzf_walk(r, ridx, lo, hi, fetch, emit, o);
    if (lane == 0) out[ridx] = o;
}

__global__ __launch_bounds__(GATHER_THREADS) void bgzf_gather_kernel(const uint8_t *__restrict__ scratch, uint8_t *__restrict__ out,
                                                                     const BgzfCopy *__restrict__ tasks) {
    const BgzfCopy t = tasks[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    const uint8_t *__restrict__ s = scratch + t.src;
    uint8_t *__restrict__ d = out + t.dst;
    uint32_t len = t.len;
    const uint32_t h0 = (16 - (uint32_t)((uintptr_t)d & 15)) & 15, head = h0 < len ? h0 : len;
    if (tid < head) d[tid] = s[tid];
    s += head; d += head; len -= head;
    const uint32_t sh = (uint32_t)((uintptr_t)s & 3);
    const uint32_t *__restrict__ sw = (const uint32_t *)((uintptr_t)s & ~(uintptr_t)3);
    uint4 *__restrict__ dv = (uint4 *)d;
    // chunk k reads the source dwords [4k, 4k + 5) of sw: they lie inside the source while 16 k + 20 <= len + sh
    const uint32_t nv = len + sh >= 20 ? (len + sh - 20) / 16 + 1 : 0;
    for (uint32_t b = 0; b < nv; b += GATHER_THREADS * GATHER_UNROLL) {
        uint32_t w[GATHER_UNROLL][5];
#pragma unroll
        for (uint32_t k = 0; k < GATHER_UNROLL; ++k) {
            const uint32_t i = b + k * GATHER_THREADS + tid;
#pragma unroll
            for (uint32_t j = 0; j < 5; ++j) w[k][j] = i < nv ? sw[4 * i + j] : 0u;
        }
#pragma unroll
        for (uint32_t k = 0; k < GATHER_UNROLL; ++k) {
            const uint32_t i = b + k * GATHER_THREADS + tid;
            if (i < nv)
                dv[i] = make_uint4(__builtin_amdgcn_alignbyte(w[k][1], w[k][0], sh), __builtin_amdgcn_alignbyte(w[k][2], w[k][1], sh),
                                   __builtin_amdgcn_alignbyte(w[k][3], w[k][2], sh), __builtin_amdgcn_alignbyte(w[k][4], w[k][3], sh));
        }
    }
    const uint32_t it = nv * 16 + tid;    // (fewer than 20 bytes are left)
    if (it < len) d[it] = s[it];
}

}  // namespace

#define LFX_LAUNCH_CHECK()                          \
    do {                                            \
        hipError_t e_ = hipGetLastError();          \
        if (e_ != hipSuccess) return (int)e_;       \
    } while (0)

int launch_bgzf_hop(hipStream_t st, const uint8_t *in, uint64_t in_base, uint64_t n, uint32_t count, const lfx_bgzf_read *reads,
                    const uint64_t *seg_off, BgzfSeg *segs, BgzfWalk *out) {
    if (!count) return 0;
    const uint32_t grid = (count + HOP_THREADS / 64 - 1) / (HOP_THREADS / 64);
    hipLaunchKernelGGL(bgzf_hop_kernel, dim3(grid), dim3(HOP_THREADS), 0, st, in, in_base, n, count, reads, seg_off, segs, out);
    LFX_LAUNCH_CHECK();
    return 0;
}

int launch_bgzf_gather(hipStream_t st, const uint8_t *scratch, uint8_t *out, const BgzfCopy *tasks, uint32_t ntasks) {
    if (!ntasks) return 0;
    if (ntasks > 0x7FFFFFFFu) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(bgzf_gather_kernel, dim3(ntasks), dim3(GATHER_THREADS), 0, st, scratch, out, tasks);
    LFX_LAUNCH_CHECK();
    return 0;
}

}  // namespace lfx
