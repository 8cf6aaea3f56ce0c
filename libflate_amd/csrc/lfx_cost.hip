// lfx_cost.hip — CostLz77Encoder's demotion (LFX_LZ77_COST), for gfx950: the minimum-cost choice between "literal
// at p" and "the match (L(p), D(p)) at p" under the owning block's code, as a kernel that leaves 0 for the candidate of every
// position where the literal won — the shape of LazyLz77Encoder's demote_kernel (lfx_chain.hip), with a rule that looks
// max_length positions ahead instead of one.  The rule, the cut into segments and the 16-bit costs: lfx_cost.h.
//
// Out of place.  demote_kernel works in place because it reads lengths only.  This rule reads "has a candidate" and D(p), that
// is cd2, and a segment's warm-up reads them at positions the NEXT segment decides: in place, whether the warm-up sees a
// candidate or the 0 its owner left there would depend on which lane ran first.  So cd2 is only read, and the result goes to
// the match stage's array cd, which nothing reads behind the chain stage: cd[p] = cd2[p] where the match won, 0 where the
// literal did, for every position of the listed segments.  The second parse reads cd.
//
// The recurrence is serial in p and needs the last max_length + 1 costs, so lanes cannot share a segment: ONE LANE PER SEGMENT
// of COST_SEG positions, 64 segments of the work list per workgroup (one wavefront).  Left at that, neighbouring lanes would
// load and store COST_SEG positions apart, every step a round trip to L2 per lane and array.  Instead the wavefront walks in
// slabs of COST_SLAB positions:
//   * store and load, all lanes for every lane: lanes 0..31 and 32..63 take two segments at a time, write the decisions of
//     the slab just walked and fetch the next COST_SLAB positions — the byte, its length byte and its candidate, neighbouring
//     lanes at neighbouring positions — packed into one dword per position of the segment's slab in LDS;
//   * walk, every lane its own slab: one LDS read per position, three table reads (a byte each), two ring reads, a ring write
//     and the decision back into the slab.
// A lane's state is all in LDS: its block's cost table (COST_TAB_N bytes — the workgroup's segments may belong to 64 blocks,
// a batch of records: every lane gets its own copy, built by all lanes), its ring of COST_RING 16-bit costs, its slab.  Lane
// strides are odd numbers of dwords: lanes at the same offset hit different banks.  78 KB per workgroup: two per CU.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfx_common.h"
#include "lfx_cost.h"
#include "lfx_huff.h"

namespace lfx {

namespace {

constexpr uint32_t COST_LANES = 64;          // segments per workgroup: one wavefront
constexpr uint32_t COST_SLAB = 32;           // positions a lane walks between two loads
constexpr uint32_t SLAB_STRIDE = COST_SLAB + 1;              // dwords per lane: odd
constexpr uint32_t COST_LDS = COST_LANES * (COST_TAB_STRIDE + 2 * COST_RING + 4 * SLAB_STRIDE + 8 + 4 + 4 + 4 + 4);
static_assert(2 * COST_LDS <= 160 * 1024, "two workgroups per CU");
static_assert(COST_SLAB * 2 == COST_LANES, "a load step serves two segments, 32 lanes each");

__global__ __launch_bounds__(COST_LANES) void cost_demote_kernel(const uint8_t *__restrict__ in, const ChunkDesc *__restrict__ chunks,
                                                                 const CostItem *__restrict__ items, uint32_t nitems,
                                                                 const BlockCodes *__restrict__ bc, uint32_t fixed,
                                                                 const uint8_t *__restrict__ len, const uint16_t *__restrict__ cd2,
                                                                 uint16_t *__restrict__ cdo) {
    __shared__ uint32_t s_tab[COST_LANES * COST_TAB_STRIDE / 4];
    __shared__ uint32_t s_ring[COST_LANES * COST_RING / 2];
    __shared__ uint32_t s_slab[COST_LANES * SLAB_STRIDE];
    __shared__ uint64_t s_base[COST_LANES];  // the chunk's first entry in the call's arrays
    __shared__ uint32_t s_top[COST_LANES], s_n[COST_LANES], s_keep[COST_LANES], s_blk[COST_LANES];
    const uint32_t lane = threadIdx.x;
    const uint32_t idx = blockIdx.x * COST_LANES + lane;
    // ---- this lane's segment
    CostSpan sp{0u, 0u, 0u};
    uint64_t base = 0;
    uint32_t blk = 0xFFFFFFFFu;
    if (idx < nitems) {
        const CostItem it = items[idx];
        const ChunkDesc ch = chunks[it.chunk];
        sp = cost_span(ch.len, it.a);
        base = ch.in_off;
        blk = ch.block;
    }
    const uint32_t n = sp.top - sp.a;        // steps of the recurrence: step k is position top - 1 - k, down to a
    s_base[lane] = base;
    s_top[lane] = sp.top;
    s_n[lane] = n;
    s_keep[lane] = sp.top - sp.b;            // the steps of the warm-up: their decisions are the next segment's
    s_blk[lane] = n ? blk : 0xFFFFFFFFu;
    __syncthreads();
    // ---- every segment's cost table, by all lanes (under fixed codes one table's arithmetic, 64 times: no load)
    uint8_t *tab8 = (uint8_t *)s_tab;
    for (uint32_t j = 0; j < COST_LANES; j++) {
        const uint32_t b = s_blk[j];
        if (b == 0xFFFFFFFFu) continue;      // (uniform: an empty lane)
        const uint32_t *lit = bc[fixed ? 0 : b].lit, *dst = bc[fixed ? 0 : b].dist;
        uint32_t absent_lit = COST_NONE_LIT, absent_dist = COST_NONE_DIST;
        if (!fixed) {
            uint32_t ml = 0, md = lane < 30 ? dst[lane] >> 16 : 0u;
            for (uint32_t i = lane; i < 286; i += COST_LANES) ml = max(ml, lit[i] >> 16);
            for (uint32_t off = 32; off; off >>= 1) {
                ml = max(ml, (uint32_t)__shfl_xor((int)ml, (int)off));
                md = max(md, (uint32_t)__shfl_xor((int)md, (int)off));
            }
            absent_lit = ml ? ml + 1 : COST_NONE_LIT;
            absent_dist = md ? md + 1 : COST_NONE_DIST;
        }
        for (uint32_t i = lane; i < COST_TAB_N; i += COST_LANES)
            tab8[j * COST_TAB_STRIDE + i] = (uint8_t)cost_tab_entry(i, fixed != 0, lit, dst, absent_lit, absent_dist);
    }
    // the longest walk of the workgroup
    uint32_t nmax = n;
    for (uint32_t off = 32; off; off >>= 1) nmax = max(nmax, (uint32_t)__shfl_xor((int)nmax, (int)off));
    uint16_t *ring = (uint16_t *)s_ring + lane * COST_RING;
    const uint8_t *tab = tab8 + lane * COST_TAB_STRIDE;
    ring[0] = 0;                             // cost[top]
    uint32_t cs = 0;                         // the slot of the position decided last: (top - q) mod COST_RING
    const uint32_t half = lane >> 5, sl = lane & 31;
    // one trip more than there are slabs: the last one only stores
    for (uint32_t k0 = 0; k0 < nmax + COST_SLAB; k0 += COST_SLAB) {
        __syncthreads();                     // (the slab's walk is over; the first trip: the tables are whole)
#pragma unroll 4
        for (uint32_t jj = 0; jj < COST_LANES; jj += 2) {
            const uint32_t j = jj + half, nj = s_n[j];
            // ---- store the slab walked last: step kp of segment j, unless it is a step of the warm-up
            const uint32_t kp = k0 - COST_SLAB + sl;
            if (k0 && kp < nj && kp >= s_keep[j]) cdo[s_base[j] + (s_top[j] - 1 - kp)] = (uint16_t)s_slab[j * SLAB_STRIDE + sl];
            // ---- load the next one
            const uint32_t k = k0 + sl;
            if (k < nj) {
                const uint64_t g = s_base[j] + (s_top[j] - 1 - k);
                s_slab[j * SLAB_STRIDE + sl] = (uint32_t)in[g] | (uint32_t)len[g] << 8 | (uint32_t)cd2[g] << 16;
            }
        }
        __syncthreads();
        // ---- walk
        const uint32_t kend = min(k0 + COST_SLAB, n);
        for (uint32_t k = k0; k < kend; k++) {
            const uint32_t v = s_slab[lane * SLAB_STRIDE + (k - k0)];
            const uint32_t byte = v & 0xFFu, l = (v >> 8) & 0xFFu, d = v >> 16;
            const uint32_t reach = k + 1;    // top - p
            const uint32_t L = l + 3 < reach ? l + 3 : reach;          // min(p + L(p), top) - p
            uint32_t eb, ex;
            const uint32_t ds = d ? dist_symbol(d, eb, ex) : 0u;
            const uint32_t mat = (uint32_t)tab[COST_TAB_LEN + l] + tab[COST_TAB_DIST + ds];
            const uint32_t jump = cs + 1 >= L ? cs + 1 - L : cs + 1 + COST_RING - L;      // the slot of p + L (cs + 1: p's, unwrapped)
            bool literal;
            const uint32_t c = cost_step(tab[byte], d != 0, mat, ring[cs], ring[jump], &literal);
            cs = cs + 1 == COST_RING ? 0u : cs + 1;
            ring[cs] = (uint16_t)c;
            s_slab[lane * SLAB_STRIDE + (k - k0)] = literal ? 0u : d;
        }
    }
}

}  // namespace

int launch_cost_demote(hipStream_t st, const uint8_t *in, const ChunkDesc *chunks, const CostItem *items, uint32_t nitems,
                       const BlockCodes *bc, bool fixed, const uint8_t *len, const uint16_t *cd2, uint16_t *cd) {
    if (!nitems) return 0;
    hipLaunchKernelGGL(cost_demote_kernel, dim3((nitems + COST_LANES - 1) / COST_LANES), dim3(COST_LANES), 0, st, in, chunks, items, nitems,
                       bc, fixed ? 1u : 0u, len, cd2, cd);
    return (int)hipGetLastError();
}

}  // namespace lfx
