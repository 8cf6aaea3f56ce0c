// lfx_members_enc.hip — one buffer as back-to-back gzip members / BGZF (lfx_encode_members_device).
// The members' chunks and blocks form one merged plan (as in lfx_encode_batch_device); behind the Huffman kernel every
// block's size is known, so each member's byte length is too, and the members are packed at their final, gap-free offsets:
//   menc_size_kernel    one lane per member: the fold of offsets_batch_kernel relative to the member's own start → its byte
//                       length (BGZF: over 65536 → the length of the stored form, and a flag); then the first level of the scan:
//                       64-lane shuffle scan, LDS across the four wavefronts → the member's offset inside its workgroup's 256
//                       members, and the workgroup's sum
//   menc_scan_kernel    one workgroup: exclusive scan of the workgroup sums (1024 per round), the total, the capacity check
//   menc_rebase_kernel  one lane per member: out_off = workgroup offset + local offset; block_start[] of its blocks from there; the
//                       blocks of a fallen-back member become stored blocks (BlockDesc::type on the device: tile_bits, pack and
//                       block_header read it from there); the member's record
//   menc_frame_kernel   behind pack: header (shared, in LDS once per workgroup; BGZF: BSIZE patched in), trailer, the end-of-file
//                       marker.  Whole dwords where a dword holds nothing else; atomicOr where it is shared with a neighbour or
//                       with the member's own DEFLATE bits; single bytes in the one dword that reaches behind the output's end.
// Members are regular — member m is input bytes [m * member_size, ...) and owns blocks [m * bpm, ...) — so no per-member table
// is uploaded: a million members cost no host loop beyond the plan itself.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lfx.h"
#include "lfx_common.h"
#include "lfx_device.h"

namespace lfx {

namespace {

constexpr uint32_t ME_THREADS = 256;
constexpr uint32_t BGZF_MAX = 65536;      // BSIZE is 16 bits: total member length - 1
constexpr uint32_t BGZF_BSIZE_AT = 16;    // 10 fixed bytes, XLEN, 'B' 'C' 2 0, then BSIZE

__device__ __forceinline__ uint32_t menc_first_block(const MembersGeom &g, uint32_t m) { return m * g.bpm; }
__device__ __forceinline__ uint32_t menc_n_blocks(const MembersGeom &g, uint32_t m) { return m + 1 == g.count ? g.bpm_last : g.bpm; }

// bits of a member's blocks from `bit` on (the fold of offsets_batch_kernel); stored = every block taken as a stored one
template <bool WRITE>
__device__ __forceinline__ uint64_t menc_fold(const BlockDesc *__restrict__ blocks, const BlockCodes *__restrict__ bc, uint32_t b0,
                                              uint32_t nb, uint64_t bit, bool stored, uint64_t *__restrict__ block_start) {
    for (uint32_t b = b0; b < b0 + nb; ++b) {
        const BlockDesc bd = blocks[b];
        if (WRITE) block_start[b] = bit;
        if (stored || bd.type == BT_RAW) { bit += 3; bit = (bit + 7) & ~7ull; bit += 32 + 8 * bd.in_len; }
        else bit += bc[b].body_bits;
        if (bd.align_after) bit = (bit + 7) & ~7ull;
    }
    return bit;
}

__global__ __launch_bounds__(ME_THREADS) void menc_size_kernel(MembersGeom g, const BlockDesc *__restrict__ blocks,
                                                               const BlockCodes *__restrict__ bc, uint64_t *__restrict__ local_off,
                                                               uint64_t *__restrict__ mlen, uint64_t *__restrict__ wg_sum,
                                                               lfx_member *__restrict__ members) {
    __shared__ uint64_t s_wsum[ME_THREADS / 64];
    const uint32_t m = blockIdx.x * ME_THREADS + threadIdx.x;
    uint64_t len = 0;
    if (m < g.count) {
        const uint32_t b0 = menc_first_block(g, m), nb = menc_n_blocks(g, m);
        len = (menc_fold<false>(blocks, bc, b0, nb, 8ull * g.hdr_len, false, nullptr) >> 3) + 8;
        bool fb = false;
        if (g.bgzf && len > BGZF_MAX) {
            fb = true;
            len = (menc_fold<false>(blocks, bc, b0, nb, 8ull * g.hdr_len, true, nullptr) >> 3) + 8;
        }
        mlen[m] = len | (fb ? 1ull << 63 : 0ull);
        const uint64_t in_off = (uint64_t)m * g.member_size;
        members[m].in_off = in_off;                        // (the checksum kernel reads the slices from here)
        members[m].in_len = min(g.member_size, g.n - in_off);
    }
    // exclusive scan over the workgroup: inclusive shuffle scan per wavefront, the wavefronts' sums through LDS
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t x = len;
    for (int o = 1; o < 64; o <<= 1) { const uint64_t y = __shfl_up(x, o); if ((int)lane >= o) x += y; }
    if (lane == 63) s_wsum[wave] = x;
    __syncthreads();
    uint64_t pre = 0;
    for (uint32_t w = 0; w < wave; ++w) pre += s_wsum[w];
    if (m < g.count) local_off[m] = pre + x - len;
    if (threadIdx.x == ME_THREADS - 1) wg_sum[blockIdx.x] = pre + x;
}

// wg_sum[0, nwg) → its exclusive scan in place; the total length, and whether it fits
__global__ __launch_bounds__(1024) void menc_scan_kernel(uint64_t *__restrict__ wg_sum, uint32_t nwg, uint64_t tail_bytes, uint64_t cap,
                                                         EncodeResult *__restrict__ res) {
    __shared__ uint64_t s_wsum[16];
    __shared__ uint64_t s_carry;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t base = 0; base < nwg; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        const uint64_t v = i < nwg ? wg_sum[i] : 0ull;
        uint64_t x = v;
        for (int o = 1; o < 64; o <<= 1) { const uint64_t y = __shfl_up(x, o); if ((int)lane >= o) x += y; }
        if (lane == 63) s_wsum[wave] = x;
        __syncthreads();
        uint64_t pre = s_carry;
        for (uint32_t w = 0; w < wave; ++w) pre += s_wsum[w];
        if (i < nwg) wg_sum[i] = pre + x - v;
        __syncthreads();
        if (threadIdx.x == 1023) s_carry = pre + x;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const uint64_t total = s_carry + tail_bytes;
        res->out_bytes = total;
        res->end_bit = 8 * total;
        if (total > cap) res->status = 1u;     // (cleared by the prepare stage's first kernel)
    }
}

__global__ __launch_bounds__(ME_THREADS) void menc_rebase_kernel(MembersGeom g, BlockDesc *__restrict__ blocks,
                                                                 const BlockCodes *__restrict__ bc, const uint64_t *__restrict__ local_off,
                                                                 const uint64_t *__restrict__ mlen, const uint64_t *__restrict__ wg_off,
                                                                 uint64_t *__restrict__ block_start, lfx_member *__restrict__ members) {
    const uint32_t m = blockIdx.x * ME_THREADS + threadIdx.x;
    if (m >= g.count) return;
    const uint64_t out_off = wg_off[blockIdx.x] + local_off[m];
    const uint64_t ml = mlen[m];
    const bool fb = (ml >> 63) != 0;
    const uint32_t b0 = menc_first_block(g, m), nb = menc_n_blocks(g, m);
    menc_fold<true>(blocks, bc, b0, nb, 8 * (out_off + g.hdr_len), fb, block_start);
    if (fb)
        for (uint32_t b = b0; b < b0 + nb; ++b) blocks[b].type = BT_RAW;
    members[m].out_off = out_off;
    members[m].out_len = ml & ~(1ull << 63);
}

// bytes [at, at + nb) of the output, byte i = get(i).  total = the output's length: a dword that reaches behind it is written
// byte by byte (nothing behind the output is touched, not even by an OR of zeros).
template <typename F>
__device__ __forceinline__ void menc_put(uint32_t *__restrict__ out, uint64_t at, uint32_t nb, uint64_t total, F get) {
    const uint64_t end = at + nb;
    for (uint64_t w = at >> 2; w * 4 < end; ++w) {
        const uint64_t lo = max(w * 4, at), hi = min(w * 4 + 4, end);
        uint32_t v = 0;
        for (uint64_t ob = lo; ob < hi; ++ob) v |= (uint32_t)get((uint32_t)(ob - at)) << (8 * (ob & 3));
        if (w * 4 + 4 > total) {
            for (uint64_t ob = lo; ob < hi; ++ob) ((uint8_t *)out)[ob] = (uint8_t)(v >> (8 * (ob & 3)));
        } else if (hi - lo == 4) {
            out[w] = v;
        } else if (v) {
            atomicOr(&out[w], v);
        }
    }
}

__constant__ uint8_t BGZF_EOF[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43,
                                     0x02, 0,    0x1b, 0,    3, 0, 0, 0, 0, 0,    0,    0, 0,    0};

// lane m < count: member m's header and trailer; lane count (BGZF): the end-of-file marker
__global__ __launch_bounds__(ME_THREADS) void menc_frame_kernel(MembersGeom g, const uint8_t *__restrict__ hdr,
                                                                const lfx_member *__restrict__ members, const uint32_t *__restrict__ crc,
                                                                const EncodeResult *__restrict__ res, uint32_t *__restrict__ out) {
    constexpr uint32_t HDR_LDS = 512;                       // (a longer header — a long file name or comment — is read from memory)
    __shared__ uint8_t s_hdr[HDR_LDS];
    const bool in_lds = g.hdr_len <= HDR_LDS;
    if (in_lds)
        for (uint32_t i = threadIdx.x; i < g.hdr_len; i += ME_THREADS) s_hdr[i] = hdr[i];
    __syncthreads();
    if (res->status != 0) return;
    const uint64_t total = res->out_bytes;
    const uint32_t m = blockIdx.x * ME_THREADS + threadIdx.x;
    if (m < g.count) {
        const lfx_member mb = members[m];
        const uint32_t bsize = (uint32_t)(mb.out_len - 1);
        const uint8_t *h = in_lds ? s_hdr : hdr;
        const bool bgzf = g.bgzf != 0;
        menc_put(out, mb.out_off, g.hdr_len, total, [&](uint32_t i) -> uint32_t {
            if (bgzf && i == BGZF_BSIZE_AT) return bsize & 255u;
            if (bgzf && i == BGZF_BSIZE_AT + 1) return (bsize >> 8) & 255u;
            return h[i];
        });
        // gzip.rs:114-121: CRC-32 LE + ISIZE LE
        const uint32_t c = mb.in_len ? crc[m] : 0u, sz = (uint32_t)mb.in_len;
        menc_put(out, mb.out_off + mb.out_len - 8, 8, total, [&](uint32_t i) -> uint32_t { return ((i < 4 ? c : sz) >> (8 * (i & 3))) & 255u; });
    } else if (m == g.count && g.bgzf) {
        menc_put(out, total - 28, 28, total, [&](uint32_t i) -> uint32_t { return BGZF_EOF[i]; });
    }
}

}  // namespace

#define LFX_LAUNCH_CHECK()                          \
    do {                                            \
        hipError_t e_ = hipGetLastError();          \
        if (e_ != hipSuccess) return (int)e_;       \
    } while (0)

int launch_members_layout(hipStream_t st, const MembersGeom &g, BlockDesc *blocks, const BlockCodes *bc, uint64_t *local_off,
                          uint64_t *mlen, uint64_t *wg_sum, uint64_t cap, uint64_t *block_start, lfx_member *members,
                          EncodeResult *res) {
    const uint32_t nwg = (g.count + ME_THREADS - 1) / ME_THREADS;
    if (nwg) {
        hipLaunchKernelGGL(menc_size_kernel, dim3(nwg), dim3(ME_THREADS), 0, st, g, blocks, bc, local_off, mlen, wg_sum, members);
        LFX_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(menc_scan_kernel, dim3(1), dim3(1024), 0, st, wg_sum, nwg, g.bgzf ? 28ull : 0ull, cap, res);
    LFX_LAUNCH_CHECK();
    if (nwg) {
        hipLaunchKernelGGL(menc_rebase_kernel, dim3(nwg), dim3(ME_THREADS), 0, st, g, blocks, bc, local_off, mlen, wg_sum, block_start, members);
        LFX_LAUNCH_CHECK();
    }
    return 0;
}

// menc_scan_kernel alone, for lfx_batch_pack.hip: its first scan level leaves its own workgroup sums
int launch_scan_wg_sums(hipStream_t st, uint64_t *wg_sum, uint32_t nwg, uint64_t cap, EncodeResult *res) {
    hipLaunchKernelGGL(menc_scan_kernel, dim3(1), dim3(1024), 0, st, wg_sum, nwg, 0ull, cap, res);
    LFX_LAUNCH_CHECK();
    return 0;
}

int launch_members_frame(hipStream_t st, const MembersGeom &g, const uint8_t *hdr, const lfx_member *members, const uint32_t *crc,
                         const EncodeResult *res, uint32_t *out) {
    const uint32_t lanes = g.count + (g.bgzf ? 1u : 0u);
    if (!lanes) return 0;
    hipLaunchKernelGGL(menc_frame_kernel, dim3((lanes + ME_THREADS - 1) / ME_THREADS), dim3(ME_THREADS), 0, st, g, hdr, members, crc, res, out);
    LFX_LAUNCH_CHECK();
    return 0;
}

}  // namespace lfx
