// lfx_chain.hip — ChainLz77Encoder's candidate refinement (LFX_LZ77_CHAIN) and LazyLz77Encoder's demotion on top
// of it (LFX_LZ77_LAZY, §20: demote_kernel below), for gfx950; LevelLz77Encoder's tuned instances of both (LFX_LZ77_LEVEL, §23).
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
#include "lfx_dict_tab.h"

namespace lfx {

namespace {

// 8 bytes at LDS byte offset off, from aligned dword reads
__device__ __forceinline__ uint64_t lds8(const uint32_t *w, uint32_t off) {
    const uint32_t i = off >> 2, sh = off & 3;
    const uint32_t w0 = w[i], w1 = w[i + 1], w2 = w[i + 2];
    return (uint64_t)__builtin_amdgcn_alignbyte(w1, w0, sh) | (uint64_t)__builtin_amdgcn_alignbyte(w2, w1, sh) << 32;
}
__device__ __forceinline__ uint32_t lds1(const uint32_t *w, uint32_t off) { return (w[off >> 2] >> ((off & 3) * 8)) & 0xFFu; }

// LEN (LazyLz77Encoder): the length of the candidate written, which this kernel holds anyway, goes to a byte per
// position as well — L - 3, and 0 where there is no candidate ("none" and L = 3 share the 0: only a strictly longer successor
// demotes a position, and a position without a candidate is no match anyway; 257 and 258 stay apart).  Without LEN the
// kernel is ChainLz77Encoder's, instruction for instruction, with its arguments: the length array is a parameter pack of
// none (chain_kernel<TILE, WCAP, THREADS>) or of one uint8_t * (chain_kernel<TILE, WCAP, THREADS, uint8_t *>).
//
// DICT (a chain dictionary): the same pack begins with a ChainDict (chain_kernel<..., ChainDict> and
// chain_kernel<..., ChainDict, uint8_t *>).  The tile belongs to a primed chunk and begins within window_size of its start: the
// dictionary's tail T and its chain lie in front of position 0 in LDS — position -1 is T's last byte, through the unsigned
// wrap the parse's dictionary instance uses — and a chain that reaches position 0 goes on into T.  Without the ChainDict
// every `DICT ? :` below folds to what stood there before.
//
// TUNE (LFX_LZ77_LEVEL): the pack ends with a ChainTune behind the length array (chain_kernel<..., uint8_t *,
// ChainTune> and chain_kernel<..., ChainDict, uint8_t *, ChainTune>).  Two rules, both functions of the position alone: the
// walk ends behind the first candidate of min(lim, nice) bytes or more instead of lim, and a 3-byte match farther than too_far
// is stored as "no candidate" (its length byte is the 0 it was).  Without the ChainTune both fold away.
template <typename... Extra> constexpr bool chain_has_dict = false;
template <typename... Rest> constexpr bool chain_has_dict<ChainDict, Rest...> = true;
__device__ __forceinline__ uint8_t *len_of() { return nullptr; }
__device__ __forceinline__ uint8_t *len_of(uint8_t *len) { return len; }
__device__ __forceinline__ uint8_t *len_of(const ChainDict &) { return nullptr; }
__device__ __forceinline__ uint8_t *len_of(const ChainDict &, uint8_t *len) { return len; }
__device__ __forceinline__ ChainDict dict_of() { return ChainDict{nullptr, nullptr, nullptr, 0u}; }
__device__ __forceinline__ ChainDict dict_of(uint8_t *) { return ChainDict{nullptr, nullptr, nullptr, 0u}; }
__device__ __forceinline__ ChainDict dict_of(const ChainDict &d) { return d; }
__device__ __forceinline__ ChainDict dict_of(const ChainDict &d, uint8_t *) { return d; }
__device__ __forceinline__ uint8_t *len_of(uint8_t *len, const ChainTune &) { return len; }
__device__ __forceinline__ uint8_t *len_of(const ChainDict &, uint8_t *len, const ChainTune &) { return len; }
__device__ __forceinline__ ChainDict dict_of(uint8_t *, const ChainTune &) { return ChainDict{nullptr, nullptr, nullptr, 0u}; }
__device__ __forceinline__ ChainDict dict_of(const ChainDict &d, uint8_t *, const ChainTune &) { return d; }
template <typename... Extra> __device__ __forceinline__ ChainTune tune_of(Extra...) { return ChainTune{0xFFFFFFFFu, 0xFFFFFFFFu}; }
__device__ __forceinline__ ChainTune tune_of(uint8_t *, const ChainTune &t) { return t; }
__device__ __forceinline__ ChainTune tune_of(const ChainDict &, uint8_t *, const ChainTune &t) { return t; }

// 4 bytes from byte 4 * wi + ph (ph 0..3) of an array of ndw aligned dwords; what lies outside the array reads as 0
__device__ __forceinline__ uint32_t dword_at(const uint32_t *__restrict__ w, int32_t wi, uint32_t ph, int32_t ndw) {
    const uint32_t a = wi >= 0 && wi < ndw ? w[wi] : 0u;
    const uint32_t b = ph != 0 && wi + 1 >= 0 && wi + 1 < ndw ? w[wi + 1] : 0u;
    return __builtin_amdgcn_alignbyte(b, a, ph);
}

template <uint32_t TILE, uint32_t WCAP, uint32_t THREADS, typename... Extra>
__global__ __launch_bounds__(THREADS) void chain_kernel(const uint8_t *__restrict__ in, const ChunkDesc *__restrict__ chunks,
                                                        const ChainItem *__restrict__ items, uint32_t window, uint32_t max_len,
                                                        uint32_t depth, const uint16_t *__restrict__ cd, uint16_t *__restrict__ cd2,
                                                        Extra... extra) {
    constexpr bool DICT = chain_has_dict<Extra...>;
    constexpr bool LEN = sizeof...(Extra) != (DICT ? 1 : 0);
    constexpr bool TUNE = sizeof...(Extra) == (DICT ? 3 : 2);
    static_assert(sizeof...(Extra) <= (DICT ? 3 : 2), "a chain dictionary or none, then no length array or one, then no tuning or one");
    static_assert(!DICT || WCAP == MAX_WINDOW, "the dictionary's tail takes the room of the window in front of position 0");
    constexpr uint32_t BW = chain_lds_bytes_dw(TILE, WCAP);
    constexpr uint32_t CW = chain_lds_cand_dw(TILE, WCAP);
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
    // DICT: T's last n_t bytes in front of the chunk (lo == 0: p0 < window <= WCAP); a tile that is not listed for this
    // instance (never) has n_t == 0 and runs as the instance without a dictionary does
    const ChainDict dict = dict_of(extra...);
    const ChainTune tune = tune_of(extra...);
    const ChainDictFill df = DICT && (ch.flags & CH_DICT) && lo == 0 ? chain_dict_fill(dict.usable, window, p0) : ChainDictFill{0u, 0u, 0u};
    // ---- stage the bytes and the candidates on their own dword grids: position q's byte sits at LDS byte q - lo + sh, its
    //      candidate at entry q - lo + csh.  (The dwords that hold the first and the last byte may reach up to three bytes
    //      outside [lo, hi), as the parse's reads do; a dword that holds no byte of it is not read.)
    const uint64_t a0 = (uint64_t)(in + ch.in_off) + lo;
    const uint32_t sh = (uint32_t)a0 & 3;
    const uint32_t *gw = (const uint32_t *)(a0 - sh);
    const uint32_t ndw = (hi - lo + sh + 3) >> 2;
    if (DICT) { for (uint32_t k = tid; k < ndw && df.dw_t + k < BW; k += THREADS) s_b[df.dw_t + k] = gw[k]; }
    else for (uint32_t k = tid; k < ndw && k < BW; k += THREADS) s_b[k] = gw[k];
    const uint64_t e0 = ch.in_off + lo;
    const uint32_t csh = (uint32_t)e0 & 1;
    const uint32_t *gc = (const uint32_t *)(cd + (e0 - csh));
    const uint32_t ncw = (p1 - lo + csh + 1) >> 1;
    if (DICT) { for (uint32_t k = tid; k < ncw && df.dw_c + k < CW; k += THREADS) s_c[df.dw_c + k] = gc[k]; }
    else for (uint32_t k = tid; k < ncw && k < CW; k += THREADS) s_c[k] = gc[k];
    if (DICT && df.n_t) {
        // T and its chain, whole dwords in front of the chunk's first one: LDS dword m of the bytes holds the window's bytes
        // from MAX_WINDOW + 4 * (m - dw_t) - sh on, LDS dword m of the candidates the window's entries from
        // MAX_WINDOW + 2 * (m - dw_c) - csh on — off the source's dword grid by the chunk's own phase.  The chunk's first dword
        // keeps T's last sh bytes, and the two positions whose prefix runs into the chunk have no entry in cdt: all of that is
        // patched behind the barrier.
        const uint32_t *tw = (const uint32_t *)dict.win;
        const uint32_t *tc = (const uint32_t *)dict.cdt;
        const int32_t wb = (int32_t)(MAX_WINDOW / 4) - (int32_t)df.dw_t - (sh ? 1 : 0);
        const int32_t wc = (int32_t)(MAX_WINDOW / 2) - (int32_t)df.dw_c - (int32_t)csh;
        for (uint32_t m = tid; m < df.dw_t; m += THREADS) s_b[m] = dword_at(tw, wb + (int32_t)m, (4 - sh) & 3, MAX_WINDOW / 4);
        for (uint32_t m = tid; m < df.dw_c; m += THREADS) s_c[m] = dword_at(tc, wc + (int32_t)m, csh ? 2u : 0u, MAX_WINDOW / 2);
        __syncthreads();
        if (tid < sh) ((uint8_t *)s_b)[4 * df.dw_t + tid] = dict.win[MAX_WINDOW - sh + tid];
        if (tid == 64) {
            // The links of |T|-1 and |T|-2 (n >= 4 here: both are inserted, and their prefixes are whole).  |T|-1 links to |T|-2
            // if their prefixes agree, otherwise to the table's last position of its prefix; |T|-2 to the table's.
            const uint32_t t = dict.usable;
            const uint8_t *b = in + ch.in_off, *te = dict.win + MAX_WINDOW;
            const uint32_t pre1 = (uint32_t)te[-1] | (uint32_t)b[0] << 8 | (uint32_t)b[1] << 16;
            const uint32_t pre2 = t >= 2 ? (uint32_t)te[-2] | (uint32_t)te[-1] << 8 | (uint32_t)b[0] << 16 : 0xFFFFFFFFu;
            uint32_t l1 = 0, l2 = 0;
            if (t >= 3) {
                const uint32_t j2 = tab_lookup(dict.tab, pre2);
                if (j2 != 0xFFFFFFFFu) l2 = t - 2 - j2;
            }
            if (pre1 == pre2) l1 = 1;
            else if (t >= 3) {
                const uint32_t j1 = tab_lookup(dict.tab, pre1);
                if (j1 != 0xFFFFFFFFu) l1 = t - 1 - j1;
            }
            uint16_t *cw = (uint16_t *)s_c;
            const uint32_t z = 2 * df.dw_c + csh;                 // position 0's entry (>= 1: n_t >= 1)
            cw[z - 1] = (uint16_t)l1;
            if (z >= 2) cw[z - 2] = (uint16_t)l2;                 // (z == 1: n_t == 1, there is no |T|-2 in reach)
        }
    }
    __syncthreads();
    const uint16_t *c16 = (const uint16_t *)s_c;
    // (unsigned wrap: q + boff = q - lo + sh; DICT: + the dwords in front, and q may be a wrapped position in front of 0)
    const uint32_t boff = DICT ? sh - lo + 4 * df.dw_t : sh - lo, coff = DICT ? csh - lo + 2 * df.dw_c : csh - lo;
    const uint32_t lo_t = lo - df.n_t;                            // DICT: the first position staged, wrapped
    uint16_t *out = cd2 + ch.in_off;
    uint8_t *lout = LEN ? len_of(extra...) + ch.in_off : nullptr;

    enum : uint32_t { FETCH = 0, COMPARE = 1, HOP = 2 };
    uint32_t state = FETCH;
    uint32_t p = p0 + tid;
    uint32_t c = 0, cur = 0, best = 0, bestd = 0, left = 0, lim = 0;
    for (;;) {
        if (state == FETCH) {
            if (p >= p1) break;
            const uint32_t d = c16[p + coff];
            if (d == 0 || (!DICT && d > p)) {                     // no candidate (d > p: never, a distance stays inside the chunk — or, DICT, reaches into T)
                out[p] = 0;
                if (LEN) lout[p] = 0;
                p += THREADS;
                continue;
            }
            c = p - d;
            left = depth;
            best = 0;
            bestd = d;
            cur = 3;
            lim = n - p < max_len ? n - p : max_len;              // (>= 4: p < end)
            state = (DICT ? (int32_t)(c - lo_t) >= 0 : c >= lo) ? COMPARE : FETCH;
            if (state == FETCH) {                                 // (never: the first candidate is within the window staged)
                out[p] = (uint16_t)d;
                if (LEN) lout[p] = 0;
                p += THREADS;
            }
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
        bool fin = best >= (TUNE && tune.nice < lim ? tune.nice : lim) || left == 0;
        if (!fin) {
            const uint32_t dq = c16[c + coff];
            fin = dq == 0 || (!DICT && dq > c);
            if (!fin) {
                const uint32_t c2 = c - dq;
                // (c2 in front of what is staged: never, lo <= p0 - min(window, WCAP) — DICT: T's last window - p0 bytes)
                fin = p - c2 > window || (DICT ? (int32_t)(c2 - lo_t) < 0 : c2 < lo);
                if (!fin) {
                    c = c2;
                    // longer than `best` only if the byte at that index matches too (best < lim: p + best < n)
                    if (lds1(s_b, c + best + boff) == lds1(s_b, p + best + boff)) { cur = 3; state = COMPARE; }
                    else --left;                                  // (a candidate all the same: it counts towards the depth)
                }
            }
        }
        if (fin) {
            if (TUNE && best == 3 && bestd > tune.too_far) bestd = 0;   // too far: no candidate (its length byte is 0 as it is)
            out[p] = (uint16_t)bestd;
            if (LEN) lout[p] = (uint8_t)(best - 3);               // (3 <= best <= 258: every walk that ends here compared once)
            p += THREADS;
            state = FETCH;
        }
    }
}

// LazyLz77Encoder's demotion, a launch of its own behind the chain kernel: len[p + 1] at a tile's last position
// is another workgroup's.  For every listed position p < end: cd2[p] = 0 when p + 1 < end and len[p + 1] > len[p] — zlib's
// deflate_slow rule as a function of the position alone; L(end) = 0 by contract, so nothing is read across a chunk.  Reads len,
// writes only cd2[p] of its own positions: in place, no race (a neighbour's cd2 is never read for "has a candidate").
//
// Bandwidth-bound: 1 byte of len and 2 + 2 bytes of cd2 per position.  A chunk begins anywhere, so the tile's positions
// [g0, g1) of the call's arrays are cut on the grid of 16: a lane takes 16 positions of the aligned middle with one 16-byte
// load of len, one byte of the next group, and two 16-byte loads and stores of cd2 (adjacent lanes, adjacent groups); the up
// to 15 positions in front and behind, which share their group with another tile or chunk, go one 2-byte store each
// (demote_span, lfx_chain.h).
constexpr uint32_t DEMOTE_THREADS = 256;
static_assert(DEMOTE_GROUP == 16, "a lane's uint4 of lengths");
__device__ __forceinline__ uint32_t demote_keep(uint32_t l, uint32_t nx, uint32_t k) {   // 0xFFFF: position k of the dword stays
    return ((nx >> (8 * k)) & 0xFFu) > ((l >> (8 * k)) & 0xFFu) ? 0u : 0xFFFFu;
}
__global__ __launch_bounds__(DEMOTE_THREADS) void demote_kernel(const ChunkDesc *__restrict__ chunks, const ChainItem *__restrict__ items,
                                                                uint32_t tile, const uint8_t *__restrict__ len, uint16_t *cd2) {
    const ChainItem it = items[blockIdx.x];
    const ChunkDesc ch = chunks[it.chunk];
    const DemoteSpan s = demote_span(ch.in_off, ch.len, it.p0, tile);
    const uint64_t g0 = s.g0, a = s.a, b = s.b, g1 = s.g1, gend = s.gend;
    if (g0 >= g1) return;                                         // (never listed)
    const uint32_t tid = threadIdx.x;
    // the edges: [g0, a) and [b, g1), under 16 positions each — or the whole of an item under 31
    if (tid < 32) {
        const uint64_t g = g0 + tid;
        if (g < a && g + 1 < gend && len[g + 1] > len[g]) cd2[g] = 0;
    } else if (tid < 48) {
        const uint64_t g = b + (tid - 32);
        if (g < g1 && g + 1 < gend && len[g + 1] > len[g]) cd2[g] = 0;
    }
    for (uint64_t g = a + 16 * (uint64_t)tid; g < b; g += 16 * DEMOTE_THREADS) {
        const uint4 l = *(const uint4 *)(len + g);
        const uint32_t nb = g + 16 < gend ? len[g + 16] : 0u;    // (g + 16 == gend: position end - 1 stays, L(end) = 0)
        uint4 *c = (uint4 *)(cd2 + g);
        uint4 c0 = c[0], c1 = c[1];
        const uint32_t lw[5] = {l.x, l.y, l.z, l.w, nb};
        uint32_t keep[8];
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            const uint32_t nx = __builtin_amdgcn_alignbyte(lw[j + 1], lw[j], 1);   // the lengths one position on
            keep[2 * j] = demote_keep(lw[j], nx, 0) | demote_keep(lw[j], nx, 1) << 16;
            keep[2 * j + 1] = demote_keep(lw[j], nx, 2) | demote_keep(lw[j], nx, 3) << 16;
        }
        c0.x &= keep[0]; c0.y &= keep[1]; c0.z &= keep[2]; c0.w &= keep[3];
        c1.x &= keep[4]; c1.y &= keep[5]; c1.z &= keep[6]; c1.w &= keep[7];
        c[0] = c0;
        c[1] = c1;
    }
}

// LFX_LZ77_LEVEL's demotion: demote_kernel with max_lazy.  A position whose length is Z or more keeps its
// candidate whatever follows — in the bytes of len, l >= zb = Z - 3 — so cd2[p] = 0 when p + 1 < end, len[p + 1] > len[p] and
// len[p] < zb.  (A position without a candidate shares the byte 0 with L = 3 and may be "demoted": its cd2 is 0 already.)  The
// same cut of the item, the same accesses.  A kernel of its own, and a template, for one reason: LazyLz77Encoder's kernel above
// and the chain kernel's instances of the kinds 2 and 3 keep the code object text they had, label for label — the compiler
// emits a template's instance where it is first used (launch_demote, at the end of this file), behind all of them.
__device__ __forceinline__ uint32_t demote_keep_level(uint32_t l, uint32_t nx, uint32_t k, uint32_t zb) {
    const uint32_t lk = (l >> (8 * k)) & 0xFFu;
    return ((nx >> (8 * k)) & 0xFFu) > lk && lk < zb ? 0u : 0xFFFFu;
}
template <uint32_t THREADS>
__global__ __launch_bounds__(THREADS) void demote_level_kernel(const ChunkDesc *__restrict__ chunks, const ChainItem *__restrict__ items,
                                                               uint32_t tile, const uint8_t *__restrict__ len, uint16_t *cd2, uint32_t zb) {
    const ChainItem it = items[blockIdx.x];
    const ChunkDesc ch = chunks[it.chunk];
    const DemoteSpan s = demote_span(ch.in_off, ch.len, it.p0, tile);
    const uint64_t g0 = s.g0, a = s.a, b = s.b, g1 = s.g1, gend = s.gend;
    if (g0 >= g1) return;                                         // (never listed)
    const uint32_t tid = threadIdx.x;
    if (tid < 32) {
        const uint64_t g = g0 + tid;
        if (g < a && g + 1 < gend && len[g + 1] > len[g] && len[g] < zb) cd2[g] = 0;
    } else if (tid < 48) {
        const uint64_t g = b + (tid - 32);
        if (g < g1 && g + 1 < gend && len[g + 1] > len[g] && len[g] < zb) cd2[g] = 0;
    }
    for (uint64_t g = a + 16 * (uint64_t)tid; g < b; g += 16 * THREADS) {
        const uint4 l = *(const uint4 *)(len + g);
        const uint32_t nb = g + 16 < gend ? len[g + 16] : 0u;    // (g + 16 == gend: position end - 1 stays, L(end) = 0)
        uint4 *c = (uint4 *)(cd2 + g);
        uint4 c0 = c[0], c1 = c[1];
        const uint32_t lw[5] = {l.x, l.y, l.z, l.w, nb};
        uint32_t keep[8];
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            const uint32_t nx = __builtin_amdgcn_alignbyte(lw[j + 1], lw[j], 1);
            keep[2 * j] = demote_keep_level(lw[j], nx, 0, zb) | demote_keep_level(lw[j], nx, 1, zb) << 16;
            keep[2 * j + 1] = demote_keep_level(lw[j], nx, 2, zb) | demote_keep_level(lw[j], nx, 3, zb) << 16;
        }
        c0.x &= keep[0]; c0.y &= keep[1]; c0.z &= keep[2]; c0.w &= keep[3];
        c1.x &= keep[4]; c1.y &= keep[5]; c1.z &= keep[6]; c1.w &= keep[7];
        c[0] = c0;
        c[1] = c1;
    }
}

int launch_chain_level(hipStream_t st, const uint8_t *in, const ChunkDesc *chunks, const ChainItem *items, uint32_t nitems, bool small,
                       uint32_t window, uint32_t max_len, uint32_t depth, const uint16_t *cd, uint16_t *cd2, uint8_t *len, uint32_t n_plain,
                       const ChainDict *dict, const ChainTune &tune);

}  // namespace

int launch_chain(hipStream_t st, const uint8_t *in, uint64_t in_bytes, const ChunkDesc *chunks, const ChainItem *items,
                 uint32_t nitems, bool small, uint32_t window, uint32_t max_len, uint32_t depth, const uint16_t *cd, uint16_t *cd2,
                 uint8_t *len, uint32_t n_plain, const ChainDict *dict, const ChainTune *tune) {
    (void)in_bytes;
    if (!nitems) return 0;
    if (!dict || n_plain > nitems) n_plain = nitems;
    if (tune) return launch_chain_level(st, in, chunks, items, nitems, small, window, max_len, depth, cd, cd2, len, n_plain, dict, *tune);
    if (n_plain) {
        if (len) {
            if (small)
                hipLaunchKernelGGL((chain_kernel<CHAIN_TILE_SMALL, 0, 256, uint8_t *>), dim3(n_plain), dim3(256), 0, st, in, chunks, items, window,
                                   max_len, depth, cd, cd2, len);
            else
                hipLaunchKernelGGL((chain_kernel<CHAIN_TILE, MAX_WINDOW, 1024, uint8_t *>), dim3(n_plain), dim3(1024), 0, st, in, chunks, items,
                                   window, max_len, depth, cd, cd2, len);
        } else if (small)
            hipLaunchKernelGGL((chain_kernel<CHAIN_TILE_SMALL, 0, 256>), dim3(n_plain), dim3(256), 0, st, in, chunks, items, window, max_len,
                               depth, cd, cd2);
        else
            hipLaunchKernelGGL((chain_kernel<CHAIN_TILE, MAX_WINDOW, 1024>), dim3(n_plain), dim3(1024), 0, st, in, chunks, items, window,
                               max_len, depth, cd, cd2);
        if (const int rc = (int)hipGetLastError()) return rc;
    }
    // the tiles that reach a chain dictionary: the dictionary instance, with the tail's 32 KiB and its chain's
    // 64 KiB in front of the chunk — one workgroup of 16 wavefronts per CU, for a batch of small records as well
    const uint32_t nd = nitems - n_plain;
    if (nd) {
        const ChainItem *di = items + n_plain;
        if (len) {
            if (small)
                hipLaunchKernelGGL((chain_kernel<CHAIN_TILE_SMALL, MAX_WINDOW, 1024, ChainDict, uint8_t *>), dim3(nd), dim3(1024), 0, st, in, chunks,
                                   di, window, max_len, depth, cd, cd2, *dict, len);
            else
                hipLaunchKernelGGL((chain_kernel<CHAIN_TILE, MAX_WINDOW, 1024, ChainDict, uint8_t *>), dim3(nd), dim3(1024), 0, st, in, chunks, di,
                                   window, max_len, depth, cd, cd2, *dict, len);
        } else if (small)
            hipLaunchKernelGGL((chain_kernel<CHAIN_TILE_SMALL, MAX_WINDOW, 1024, ChainDict>), dim3(nd), dim3(1024), 0, st, in, chunks, di, window,
                               max_len, depth, cd, cd2, *dict);
        else
            hipLaunchKernelGGL((chain_kernel<CHAIN_TILE, MAX_WINDOW, 1024, ChainDict>), dim3(nd), dim3(1024), 0, st, in, chunks, di, window,
                               max_len, depth, cd, cd2, *dict);
    }
    return (int)hipGetLastError();
}

int launch_demote(hipStream_t st, const ChunkDesc *chunks, const ChainItem *items, uint32_t nitems, bool small, const uint8_t *len,
                  uint16_t *cd2, uint32_t max_lazy) {
    if (!nitems) return 0;
    if (max_lazy)                                                 // LFX_LZ77_LEVEL: a length of max_lazy or more is not deferred
        hipLaunchKernelGGL(demote_level_kernel<DEMOTE_THREADS>, dim3(nitems), dim3(DEMOTE_THREADS), 0, st, chunks, items,
                           small ? CHAIN_TILE_SMALL : CHAIN_TILE, len, cd2, max_lazy > 3 ? max_lazy - 3 : 0u);
    else
        hipLaunchKernelGGL(demote_kernel, dim3(nitems), dim3(DEMOTE_THREADS), 0, st, chunks, items, small ? CHAIN_TILE_SMALL : CHAIN_TILE,
                           len, cd2);
    return (int)hipGetLastError();
}

namespace {
int launch_chain_level(hipStream_t st, const uint8_t *in, const ChunkDesc *chunks, const ChainItem *items, uint32_t nitems, bool small,
                       uint32_t window, uint32_t max_len, uint32_t depth, const uint16_t *cd, uint16_t *cd2, uint8_t *len, uint32_t n_plain,
                       const ChainDict *dict, const ChainTune &tune) {
    // LFX_LZ77_LEVEL: three tuned instances, each with the length array — the greedy levels leave it unread.
    // One dictionary instance serves both work lists: a call of the small list has one item per chunk, at p0 = 0 and of at
    // most CHAIN_TILE_SMALL positions, which the window tile covers as it is (p1 and hi are cut at the chunk's end).
    if (!len) return (int)hipErrorInvalidValue;
    if (n_plain) {
        if (small)
            hipLaunchKernelGGL((chain_kernel<CHAIN_TILE_SMALL, 0, 256, uint8_t *, ChainTune>), dim3(n_plain), dim3(256), 0, st, in, chunks, items,
                               window, max_len, depth, cd, cd2, len, tune);
        else
            hipLaunchKernelGGL((chain_kernel<CHAIN_TILE, MAX_WINDOW, 1024, uint8_t *, ChainTune>), dim3(n_plain), dim3(1024), 0, st, in, chunks,
                               items, window, max_len, depth, cd, cd2, len, tune);
        if (const int rc = (int)hipGetLastError()) return rc;
    }
    if (nitems - n_plain)
        hipLaunchKernelGGL((chain_kernel<CHAIN_TILE, MAX_WINDOW, 1024, ChainDict, uint8_t *, ChainTune>), dim3(nitems - n_plain), dim3(1024), 0, st,
                           in, chunks, items + n_plain, window, max_len, depth, cd, cd2, *dict, len, tune);
    return (int)hipGetLastError();
}
}  // namespace

}  // namespace lfx
