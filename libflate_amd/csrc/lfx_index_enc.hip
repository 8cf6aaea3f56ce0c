// lfx_index_enc.hip — the access-point candidates of a stream the encoder has just written (lfx_encode_index_device,
// DESIGN.md §13).  Every block start of the plan is one; inside the dynamic and fixed blocks that produce more than `spacing`
// bytes, so is the first code boundary in each grain of spacing / 16 output bytes.  The encoder's own buffers hold what
// that takes: the block starts (offsets_kernel), each pack tile's start bit (tile_scan_kernel), the code words and the
// blocks' code tables.
//
// Kernels, run only over the tiles of the large blocks:
//   idx_tile_bytes_kernel   the output bytes each tile's codes cover (several tiles per workgroup, as tile_bits_kernel)
//   idx_chunk_scan_kernel   an exclusive scan of those per chunk from ChunkDesc::in_off: each tile's first output byte
//   idx_tile_points_kernel  one workgroup per tile: (bytes, bits) of every code, one workgroup-wide exclusive scan of both,
//                           and for every grain the first code start in it, into a slot array indexed by grain
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/lfx.h"
#include "lfx_abi_guard.h"
#include "lfx_common.h"
#include "lfx_ctx.h"
#include "lfx_enc_frame.h"
#include "lfx_huff.h"
#include "lfx_index.h"
#include "lfx_plan.h"

namespace lfx {

namespace {

constexpr uint32_t IE_THREADS = 256;
constexpr uint32_t IE_PER = PACK_TILE / IE_THREADS;   // codes per lane: 8
constexpr uint32_t IE_TPW = 4;                          // tiles per workgroup of idx_tile_bytes_kernel
constexpr uint32_t IE_SCAN_PER = 8;                     // tiles per lane and batch of idx_chunk_scan_kernel
constexpr uint64_t IE_EMPTY = ~0ull;                    // slot_base of a block that gets no in-block candidates; an empty slot

// output bytes a code word covers: a literal 1, EndOfBlock 0, a match its length
__device__ __forceinline__ uint32_t code_bytes(uint32_t v) {
    const uint32_t dist = v & 0xFFFFu, val = v >> 16;
    return dist ? val : (val < 256 ? 1u : 0u);
}

// tile_bytes[t - t0] for the tiles t0 <= t < t1 of the large blocks (0 for the other tiles and the empty ones)
__global__ __launch_bounds__(IE_THREADS) void idx_tile_bytes_kernel(const ChunkDesc *__restrict__ chunks, const uint32_t *__restrict__ codes,
                                                                    const uint32_t *__restrict__ ncodes, const uint32_t *__restrict__ tile_map,
                                                                    const uint64_t *__restrict__ slot_base, uint64_t t0, uint64_t t1,
                                                                    uint32_t *__restrict__ tile_bytes) {
    __shared__ uint32_t red[IE_THREADS / 64];
    const uint64_t g0 = t0 + (uint64_t)blockIdx.x * IE_TPW;
    uint32_t cm[IE_TPW];
#pragma unroll
    for (uint32_t q = 0; q < IE_TPW; ++q) cm[q] = tile_map[min(g0 + q, t1 - 1)];
    uint32_t cur_c = 0xFFFFFFFFu, n = 0;
    ChunkDesc ch{};
    bool skip = true;
    uint32_t v[IE_PER], vn[IE_PER];
    bool have_next = false;          // vn holds the codes of this tile (requested while the previous one was summed)
#pragma unroll
    for (uint32_t q = 0; q < IE_TPW; ++q) {
        const uint64_t gt = g0 + q;
        if (gt >= t1) break;
        const uint32_t c = cm[q];
        if (c != cur_c) {
            cur_c = c;
            ch = chunks[c];
            n = ncodes[c];
            skip = slot_base[ch.block] == IE_EMPTY;
            have_next = false;
        }
        const uint32_t lo = (uint32_t)(gt - ch.tile_base) * PACK_TILE;
        if (lo >= n || skip) {
            if (threadIdx.x == 0) tile_bytes[gt - t0] = 0;
            have_next = false;
            continue;
        }
        const uint32_t hi = min(n, lo + PACK_TILE);
        const uint32_t *p = codes + ch.code_off;
        if (have_next) {
#pragma unroll
            for (uint32_t k = 0; k < IE_PER; ++k) v[k] = vn[k];
        } else {
#pragma unroll
            for (uint32_t k = 0; k < IE_PER; ++k) v[k] = p[min(lo + threadIdx.x + k * IE_THREADS, hi - 1)];
        }
        // the next tile of the same chunk: its codes are requested before this one's are summed
        have_next = q + 1 < IE_TPW && gt + 1 < t1 && cm[q + 1 < IE_TPW ? q + 1 : q] == c;
        if (have_next) {
#pragma unroll
            for (uint32_t k = 0; k < IE_PER; ++k) vn[k] = p[min(lo + PACK_TILE + threadIdx.x + k * IE_THREADS, n - 1)];
        }
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t k = 0; k < IE_PER; ++k) sum += lo + threadIdx.x + k * IE_THREADS < hi ? code_bytes(v[k]) : 0u;
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o);
        __syncthreads();             // (the previous tile's total has read red[])
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
        __syncthreads();
        if (threadIdx.x == 0) tile_bytes[gt - t0] = red[0] + red[1] + red[2] + red[3];
    }
}

// one workgroup per chunk c0 + blockIdx.x of a large block: tile_out[t - t0] = in_off + the bytes of the chunk's tiles in
// front of t.  Batches of IE_SCAN_PER * blockDim.x tiles, loaded together into LDS; each lane sums IE_SCAN_PER neighbours.
__global__ __launch_bounds__(1024) void idx_chunk_scan_kernel(const ChunkDesc *__restrict__ chunks, const uint32_t *__restrict__ ncodes,
                                                              const uint64_t *__restrict__ slot_base, uint32_t c0, uint64_t t0,
                                                              const uint32_t *__restrict__ tile_bytes, uint64_t *__restrict__ tile_out) {
    __shared__ uint32_t s[IE_SCAN_PER * 1024];
    __shared__ uint64_t wsum[16];
    const ChunkDesc ch = chunks[c0 + blockIdx.x];
    if (slot_base[ch.block] == IE_EMPTY) return;
    const uint64_t nt = div_up(ncodes[c0 + blockIdx.x], PACK_TILE);   // the tiles that hold codes
    const uint32_t T = blockDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t *__restrict__ src = tile_bytes + (ch.tile_base - t0);
    uint64_t *__restrict__ dst = tile_out + (ch.tile_base - t0);
    uint64_t carry = ch.in_off;
    for (uint64_t base = 0; base < nt; base += (uint64_t)IE_SCAN_PER * T) {
        uint32_t v[IE_SCAN_PER];
#pragma unroll
        for (uint32_t k = 0; k < IE_SCAN_PER; ++k) {
            const uint64_t i = base + k * T + tid;
            v[k] = i < nt ? src[i] : 0u;
        }
        __syncthreads();             // (the previous batch has read s[] and wsum[])
#pragma unroll
        for (uint32_t k = 0; k < IE_SCAN_PER; ++k) s[k * T + tid] = v[k];
        __syncthreads();
        uint32_t mine[IE_SCAN_PER];
        uint64_t sum = 0;
#pragma unroll
        for (uint32_t k = 0; k < IE_SCAN_PER; ++k) { mine[k] = s[tid * IE_SCAN_PER + k]; sum += mine[k]; }
        uint64_t x = sum;            // inclusive wave scan of the lanes' sums
        for (int o = 1; o < 64; o <<= 1) { const uint64_t y = __shfl_up(x, o); if ((int)lane >= o) x += y; }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        uint64_t pre = carry, all = carry;
        for (uint32_t w = 0; w < T / 64; ++w) { all += wsum[w]; if (w < wave) pre += wsum[w]; }
        pre += x - sum;
#pragma unroll
        for (uint32_t k = 0; k < IE_SCAN_PER; ++k) {
            const uint64_t i = base + (uint64_t)tid * IE_SCAN_PER + k;
            if (i < nt) dst[i] = pre;
            pre += mine[k];
        }
        carry = all;
    }
}

// one workgroup per tile t0 + blockIdx.x of a large block: every code start of the tile whose grain no earlier code start of
// its block falls in — the block's first code and its EndOfBlock excepted — into slots[slot_base[block] + grain - the
// block's first grain] as (bit, output byte)
__global__ __launch_bounds__(IE_THREADS) void idx_tile_points_kernel(const ChunkDesc *__restrict__ chunks, const BlockDesc *__restrict__ blocks,
                                                                     const uint32_t *__restrict__ codes, const uint32_t *__restrict__ ncodes,
                                                                     const BlockCodes *__restrict__ bc, const uint32_t *__restrict__ tile_map,
                                                                     const uint64_t *__restrict__ tile_start, const uint64_t *__restrict__ tile_out,
                                                                     const uint64_t *__restrict__ slot_base, uint64_t grain, uint64_t t0,
                                                                     uint64_t nslots, ulonglong2 *__restrict__ slots) {
    __shared__ uint32_t lit[288], dst[32];
    // (bytes | bits << 16) per code, in code order, one pad word behind every 8: the lanes read 8 consecutive codes each, and a
    // stride of 9 words puts the 32 lanes of a ds_read_b32 half on 32 different banks (a stride of 8: on 4, 8-way conflicts)
    __shared__ uint32_t s[PACK_TILE + PACK_TILE / 8];
    __shared__ uint64_t wsum[IE_THREADS / 64];
    const uint64_t t = t0 + blockIdx.x;
    const uint32_t c = tile_map[t];
    const ChunkDesc ch = chunks[c];
    const uint64_t sb = slot_base[ch.block];
    if (sb == IE_EMPTY) return;
    const uint32_t n = ncodes[c], lo = (uint32_t)(t - ch.tile_base) * PACK_TILE;
    if (lo >= n) return;
    const uint32_t hi = min(n, lo + PACK_TILE), tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // every load of the tile is requested before the first use: codes, block, seeds, code tables
    const uint32_t *p = codes + ch.code_off;
    uint32_t v[IE_PER];
#pragma unroll
    for (uint32_t k = 0; k < IE_PER; ++k) v[k] = p[min(lo + tid + k * IE_THREADS, hi - 1)];
    const BlockDesc bd = blocks[ch.block];
    const uint64_t bit0 = tile_start[t], out0 = tile_out[t - t0];
    const BlockCodes *B = &bc[ch.block];
    lit[tid] = B->lit[tid];
    if (tid < 32) { lit[256 + tid] = B->lit[256 + tid]; dst[tid] = B->dist[tid]; }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < IE_PER; ++k) {
        uint64_t bits;
        const uint32_t nb = code_bits(v[k], lit, dst, bits);
        const uint32_t i = tid + k * IE_THREADS;
        s[i + (i >> 3)] = lo + i < hi ? code_bytes(v[k]) | nb << 16 : 0u;
    }
    __syncthreads();
    // lane l owns codes [8 l, 8 l + 8) of the tile: (bytes, bits) summed as one u64 (bytes low, bits high: a tile covers at
    // most 2048 * 258 bytes and 2048 * 48 bits)
    uint32_t w[IE_PER];
    uint64_t sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < IE_PER; ++k) { w[k] = s[tid * (IE_PER + 1) + k]; sum += (uint64_t)(w[k] & 0xFFFFu) | (uint64_t)(w[k] >> 16) << 32; }
    uint64_t x = sum;
    for (int o = 1; o < 64; o <<= 1) { const uint64_t y = __shfl_up(x, o); if ((int)lane >= o) x += y; }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    uint64_t pre = x - sum;
    for (uint32_t q = 0; q < wave; ++q) pre += wsum[q];
    uint64_t o = out0 + (pre & 0xFFFFFFFFu), bit = bit0 + (pre >> 32);
    const uint64_t blk_end = bd.in_off + bd.in_len, g_first = bd.in_off / grain;
    const bool block_head = c == bd.first_chunk && lo == 0 && tid == 0;   // this lane holds the block's first code
    // code i starts at (bit, o); the code behind it at (bit + bits_i, o + bytes_i) is the first of its grain when code i
    // lies in an earlier grain — or is the block's first code, which is no candidate itself.  `next` is the first byte of the
    // grain behind code i's: a 64-bit division only where a grain boundary is crossed, not two per code.
    uint64_t next = (o / grain + 1) * grain;
#pragma unroll
    for (uint32_t k = 0; k < IE_PER; ++k) {
        const uint64_t on = o + (w[k] & 0xFFFFu), bn = bit + (w[k] >> 16);
        const bool cross = on >= next;
        if (cross || (block_head && k == 0)) {
            const uint64_t g = on / grain;
            if (cross) next = (g + 1) * grain;
            if (lo + tid * IE_PER + k < hi && on < blk_end) {
                const uint64_t slot = sb + g - g_first;
                if (slot < nslots) slots[slot] = make_ulonglong2(bn, on);
            }
        }
        o = on;
        bit = bn;
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// host side

#define IE_HIP(expr)                                                                  \
    do {                                                                              \
        hipError_t e_ = (expr);                                                       \
        if (e_ != hipSuccess) {                                                       \
            c->set_error(std::string(#expr) + ": " + hipGetErrorString(e_));          \
            return LFX_E_DEVICE;                                                      \
        }                                                                             \
    } while (0)

namespace {
int grain_slots(Ctx *c, const Plan &plan, const std::vector<uint64_t> &slot_base, uint64_t nslots, uint64_t grain, uint32_t b_lo,
                uint32_t b_hi, std::vector<uint64_t> &h);
}  // namespace

int idx_encode_cand(Ctx *c, const Plan &plan) {
    IdxCollect &col = *c->idx_enc;
    hipStream_t st = c->stream;
    const uint32_t nblocks = (uint32_t)plan.blocks.size();
    std::vector<uint64_t> bstart(nblocks);
    IE_HIP(hipMemcpyAsync(bstart.data(), c->d_block_start.p, 8ull * nblocks, hipMemcpyDeviceToHost, st));
    IE_HIP(hipStreamSynchronize(st));
    // a slot per grain of each block larger than the spacing
    const uint64_t grain = std::max<uint64_t>(col.spacing / 16, 1);
    std::vector<uint64_t> slot_base(nblocks, IE_EMPTY);
    uint64_t nslots = 0;
    uint32_t b_lo = nblocks, b_hi = 0;
    for (uint32_t b = 0; b < nblocks; b++) {
        const BlockDesc &bd = plan.blocks[b];
        if (bd.type == BT_RAW || bd.in_len <= col.spacing || bd.n_chunks == 0) continue;
        slot_base[b] = nslots;
        nslots += (bd.in_off + bd.in_len - 1) / grain - bd.in_off / grain + 1;
        b_lo = std::min(b_lo, b);
        b_hi = b + 1;
    }
    int rc;
    std::vector<uint64_t> h;   // the slots read back: (bit, output byte) per grain of the large blocks
    if (nslots && (rc = grain_slots(c, plan, slot_base, nslots, grain, b_lo, b_hi, h))) return rc;
    // in stream order: each block's start, then its grains' first code starts
    for (uint32_t b = 0; b < nblocks; b++) {
        const BlockDesc &bd = plan.blocks[b];
        col.cand.push_back(IdxCand{bstart[b], bstart[b], bd.in_off, bd.type});
        if (slot_base[b] == IE_EMPTY) continue;
        const uint64_t ns = (bd.in_off + bd.in_len - 1) / grain - bd.in_off / grain + 1;
        for (uint64_t k = slot_base[b]; k < slot_base[b] + ns; k++)   // (an empty slot: a grain one long match covers)
            if (h[2 * k] != IE_EMPTY) col.cand.push_back(IdxCand{h[2 * k], bstart[b], h[2 * k + 1], bd.type});
    }
    // idx_finish skips its sort for candidates sorted by in_bit without repeats — checked here, not assumed
    col.in_order = std::adjacent_find(col.cand.begin(), col.cand.end(),
                                      [](const IdxCand &x, const IdxCand &y) { return x.in_bit >= y.in_bit; }) == col.cand.end();
    return LFX_OK;
}

namespace {
// the three kernels over the tiles of the large blocks [b_lo, b_hi) → h (2 u64 per slot)
int grain_slots(Ctx *c, const Plan &plan, const std::vector<uint64_t> &slot_base, uint64_t nslots, uint64_t grain, uint32_t b_lo,
                uint32_t b_hi, std::vector<uint64_t> &h) {
    hipStream_t st = c->stream;
    const uint32_t nblocks = (uint32_t)plan.blocks.size();
    // the tiles and chunks of the large blocks (and of the small blocks between them: their workgroups return at once)
    const BlockDesc &first = plan.blocks[b_lo], &last = plan.blocks[b_hi - 1];
    const uint32_t c0 = first.first_chunk, c1 = last.first_chunk + last.n_chunks;
    const uint64_t t0 = plan.chunks[c0].tile_base, t1 = plan.chunks[c1 - 1].tile_base + div_up(plan.chunks[c1 - 1].len + 1, PACK_TILE);
    uint64_t max_tiles = 0;
    for (uint32_t ci = c0; ci < c1; ci++) max_tiles = std::max<uint64_t>(max_tiles, div_up(plan.chunks[ci].len + 1, PACK_TILE));
    const uint64_t nt = t1 - t0;
    // scratch: slot_base, slots, tile bytes, tile output offsets
    const uint64_t o_slots = (8ull * nblocks + 15) & ~15ull, o_bytes = o_slots + 16 * nslots, o_out = (o_bytes + 4 * nt + 15) & ~15ull;
    int rc;
    if ((rc = c->d_idx_enc.reserve(o_out + 8 * nt))) return rc;
    uint8_t *scratch = (uint8_t *)c->d_idx_enc.p;
    uint64_t *d_sb = (uint64_t *)scratch;
    ulonglong2 *d_slots = (ulonglong2 *)(scratch + o_slots);
    uint32_t *d_tb = (uint32_t *)(scratch + o_bytes);
    uint64_t *d_to = (uint64_t *)(scratch + o_out);
    IE_HIP(hipMemcpyAsync(d_sb, slot_base.data(), 8ull * nblocks, hipMemcpyHostToDevice, st));
    IE_HIP(hipMemsetAsync(d_slots, 0xFF, 16 * nslots, st));
    const ChunkDesc *d_chunks = (const ChunkDesc *)c->d_chunks.p;
    const uint32_t *d_codes = (const uint32_t *)c->d_codes.p, *d_ncodes = (const uint32_t *)c->d_ncodes.p;
    hipLaunchKernelGGL(idx_tile_bytes_kernel, dim3((uint32_t)div_up(nt, IE_TPW)), dim3(IE_THREADS), 0, st, d_chunks, d_codes, d_ncodes,
                       c->cur_tile_map, d_sb, t0, t1, d_tb);
    IE_HIP(hipGetLastError());
    hipLaunchKernelGGL(idx_chunk_scan_kernel, dim3(c1 - c0), dim3(max_tiles > IE_SCAN_PER * 256 ? 1024 : 256), 0, st, d_chunks, d_ncodes,
                       d_sb, c0, t0, d_tb, d_to);
    IE_HIP(hipGetLastError());
    hipLaunchKernelGGL(idx_tile_points_kernel, dim3((uint32_t)nt), dim3(IE_THREADS), 0, st, d_chunks, (const BlockDesc *)c->d_blocks.p,
                       d_codes, d_ncodes, (const BlockCodes *)c->d_bc.p, c->cur_tile_map, (const uint64_t *)c->d_tile_start.p, d_to,
                       d_sb, grain, t0, nslots, d_slots);
    IE_HIP(hipGetLastError());
    h.resize(2 * nslots);
    IE_HIP(hipMemcpyAsync(h.data(), d_slots, 16 * nslots, hipMemcpyDeviceToHost, st));
    IE_HIP(hipStreamSynchronize(st));
    return LFX_OK;
}
}  // namespace

}  // namespace lfx

// ------------------------------------------------------------------------------------------------
// C ABI: lfx_encode_device, unchanged, with Ctx::idx_enc set — its last emit leaves the candidates there — then the index
// from them through idx_finish, with the encoded stream as the input and the encoder's input as the output
namespace {
struct EncIdxScope {   // Ctx::idx_enc for the length of the encode, whatever way it is left
    lfx::Ctx *c;
    EncIdxScope(lfx::Ctx *c_, lfx::IdxCollect *col) : c(c_) { c->idx_enc = col; }
    ~EncIdxScope() { c->idx_enc = nullptr; }
};
}  // namespace

extern "C" int lfx_encode_index_device(lfx_ctx *cc, int format, const lfx_encode_opts *o, const lfx_schedule *s, const void *d_in,
                                       uint64_t n, void *d_out, uint64_t cap, uint64_t *out_len, uint64_t spacing, lfx_index **idx) try {
    using namespace lfx;
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    if (idx) *idx = nullptr;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    if (!idx) { c->set_error("lfx_encode_index_device: idx is NULL"); return LFX_E_ARG; }
    if (spacing < 4096) { c->set_error("lfx_encode_index_device: spacing " + std::to_string(spacing) + " is below 4096"); return LFX_E_ARG; }
    EncodeSpec sp;
    (void)encode_spec(format, o, &sp);      // (the table answers before the domain does: lfx_encode_device checks that)
    const char *why;
    int rc = encode_served(ENC_INDEX, sp, DICT_NONE, &why);
    if (rc) { c->set_error(why); return rc; }
    IdxCollect col;
    col.spacing = spacing;
    uint64_t ol = 0;
    {
        EncIdxScope scope(c, &col);
        rc = lfx_encode_device(cc, format, o, s, d_in, n, d_out, cap, &ol);
    }
    if (rc) return rc;
    if (out_len) *out_len = ol;
    c->phase("index_cand");
    const std::vector<lfx_member> members{lfx_member{0, ol, 0, n}};
    if ((rc = idx_finish(c, col, format, 0, (const uint8_t *)d_out, ol, (const uint8_t *)d_in, n, members, idx))) return rc;
    c->phase("done");
    return LFX_OK;
} LFX_ABI_CATCH
