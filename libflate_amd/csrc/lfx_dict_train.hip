// lfx_dict_train.hip — the dictionary trainer's kernels (lfx_dict_train_device).  The constants, the hash, the
// cursor, the lane walk and the pick's key are lfx_dict_train.h's; here:
//   dtrain_index_kernel   one lane per DTRAIN_TILE positions: the record that holds the tile's first position (one search per
//                         TILE, none per position: every later lookup starts there and walks forward)
//   dtrain_count_kernel   freq[h(p)]++ for every defined position.  A lane takes DTRAIN_PPL consecutive positions with two
//                         8-byte loads; the adds are device-scope atomics into the 4 MiB table, which is what the kernel waits for
//   dtrain_step_kernel    one launch per epoch.  A workgroup takes DTRAIN_CHUNK candidates at a time: it writes the exclusive
//                         prefix sums of freq[h(q)] over the chunk and the k - 8 positions behind it (workgroup scan, 64-bit) to
//                         its own words of the scratch, then every candidate's score is the difference of two of them, and
//                         the best of the workgroup goes into the epoch's slot by one 64-bit atomic maximum
//   dtrain_zero_kernel    one workgroup, behind the step: reads the slot and clears the counters of the picked segment
//   dtrain_gather_kernel  one workgroup: the picks (2048 at most) ranked in LDS by dtrain_sort_key, the segments copied out
// The launches follow each other on one stream; the epochs depend on each other through the counters alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfx_dict_train.h"

namespace lfx {

namespace {

__global__ __launch_bounds__(DTRAIN_WG) void dtrain_index_kernel(const uint32_t *__restrict__ pos, uint32_t nrec, uint32_t ntiles,
                                                                  uint32_t *__restrict__ tile_rec) {
    const uint32_t t = blockIdx.x * DTRAIN_WG + threadIdx.x;
    if (t < ntiles) tile_rec[t] = dtrain_owner_search(pos, nrec, t * DTRAIN_TILE);
}

__global__ __launch_bounds__(DTRAIN_WG) void dtrain_count_kernel(DtrainRecs R, uint32_t *__restrict__ freq) {
    const uint64_t stride = (uint64_t)gridDim.x * DTRAIN_WG * DTRAIN_PPL;
    for (uint64_t p = ((uint64_t)blockIdx.x * DTRAIN_WG + threadIdx.x) * DTRAIN_PPL; p < R.n; p += stride) {
        const uint64_t pe = p + DTRAIN_PPL < R.n ? p + DTRAIN_PPL : R.n;
        dtrain_lane<true>(R, (uint32_t)p, (uint32_t)pe, [&](uint32_t, uint32_t, bool def, uint64_t v) {
            if (def) atomicAdd(&freq[dtrain_hash(v)], 1u);
        });
    }
}

// exclusive scan of one 64-bit value per lane over the workgroup → the lane's prefix; *total: the workgroup's sum.
// s_w: one word per wavefront.  Two barriers: the second one frees s_w for the next call.
__device__ __forceinline__ uint64_t wg_scan64(uint64_t x, uint64_t *s_w, uint64_t *total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t inc = x;
    for (int o = 1; o < 64; o <<= 1) { const uint64_t y = __shfl_up(inc, o); if ((int)lane >= o) inc += y; }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    uint64_t pre = 0, all = 0;
    for (uint32_t w = 0; w < DTRAIN_WG / 64; ++w) { const uint64_t s = s_w[w]; if (w < wave) pre += s; all += s; }
    __syncthreads();
    *total = all;
    return pre + inc - x;
}

__global__ __launch_bounds__(DTRAIN_WG) void dtrain_step_kernel(DtrainRecs R, const uint32_t *__restrict__ freq, uint64_t *__restrict__ slot,
                                                                 uint32_t lo, uint32_t hi, uint32_t k, uint64_t *__restrict__ prefix,
                                                                 uint64_t prefix_words) {
    __shared__ uint64_t s_w[DTRAIN_WG / 64];
    uint64_t *x = prefix + (uint64_t)blockIdx.x * prefix_words;       // this workgroup's CHUNK + k words
    const uint32_t span_k = k - DTRAIN_D + 1;
    uint64_t best = 0;
    for (uint64_t c = (uint64_t)lo + (uint64_t)blockIdx.x * DTRAIN_CHUNK; c < hi; c += (uint64_t)gridDim.x * DTRAIN_CHUNK) {
        const uint32_t c0 = (uint32_t)c, c1 = hi - c0 < DTRAIN_CHUNK ? hi : c0 + DTRAIN_CHUNK;
        const uint32_t s1 = (uint64_t)c1 + k - DTRAIN_D < R.n ? c1 + k - DTRAIN_D : R.n;      // the d-mers the chunk's candidates read: [c0, s1)
        // ---- x[i] = the sum of freq[h(q)] over the defined q in [c0, c0 + i), i = 0 .. s1 - c0   (s1 - c0 < CHUNK + k)
        uint64_t run = 0;
        for (uint32_t t0 = c0; t0 < s1; t0 += DTRAIN_WG * DTRAIN_SPL) {      // (t0 is the same in every lane: the barriers are uniform)
            const uint64_t q0 = (uint64_t)t0 + threadIdx.x * DTRAIN_SPL;
            const uint32_t qe = q0 + DTRAIN_SPL < s1 ? (uint32_t)q0 + DTRAIN_SPL : s1;
            uint32_t f[DTRAIN_SPL] = {0, 0, 0, 0};
            if (q0 < s1)
                dtrain_lane<true>(R, (uint32_t)q0, qe, [&](uint32_t q, uint32_t, bool def, uint64_t v) {
                    f[q - (uint32_t)q0] = def ? freq[dtrain_hash(v)] : 0u;
                });
            uint64_t total;
            uint64_t at = run + wg_scan64((uint64_t)f[0] + f[1] + f[2] + f[3], s_w, &total);
            for (uint32_t i = 0; i < DTRAIN_SPL; i++) {
                if (q0 + i < s1) x[q0 + i - c0] = at;
                at += f[i];
            }
            run += total;
        }
        if (threadIdx.x == 0) x[s1 - c0] = run;
        __syncthreads();       // the workgroup's own words, written and read through the CU's one L1
        // ---- the candidates of [c0, c1)
        for (uint64_t p0 = (uint64_t)c0 + threadIdx.x * DTRAIN_SPL; p0 < c1; p0 += DTRAIN_WG * DTRAIN_SPL) {
            const uint32_t pe = p0 + DTRAIN_SPL < c1 ? (uint32_t)p0 + DTRAIN_SPL : c1;
            dtrain_lane<false>(R, (uint32_t)p0, pe, [&](uint32_t q, uint32_t avail, bool, uint64_t) {
                if (avail < k) return;
                const uint64_t sum = x[q - c0 + span_k] - x[q - c0];
                if (sum) { const uint64_t key = dtrain_pick_key(sum, q - lo); best = key > best ? key : best; }
            });
        }
        __syncthreads();       // x is rewritten by the next chunk
    }
    // the workgroup's best: wavefront maximum by shuffles, one atomic per wavefront that has a candidate
    for (int o = 32; o > 0; o >>= 1) { const uint64_t y = __shfl_xor(best, o); best = y > best ? y : best; }
    if ((threadIdx.x & 63) == 0 && best) atomicMax((unsigned long long *)slot, (unsigned long long)best);
}

__global__ __launch_bounds__(DTRAIN_WG) void dtrain_zero_kernel(DtrainRecs R, uint32_t *__restrict__ freq, const uint64_t *__restrict__ slot,
                                                                 uint32_t lo, uint32_t k) {
    const uint64_t pick = *slot;
    if (!(pick >> 32)) return;
    const uint32_t p = lo + dtrain_pick_pos(pick);
    DtrainCursor c;
    c.seek(R, p);
    const uint8_t *a = c.at(R, p);                       // p + k stays inside the record: it was a candidate
    for (uint32_t j = threadIdx.x; j + DTRAIN_D <= k; j += DTRAIN_WG) freq[dtrain_hash(dtrain_load8(a + j))] = 0;
}

__global__ __launch_bounds__(DTRAIN_WG) void dtrain_gather_kernel(DtrainRecs R, const uint64_t *__restrict__ slots, uint32_t epochs, uint32_t k,
                                                                   uint8_t *__restrict__ out, uint64_t *__restrict__ out_len) {
    __shared__ uint64_t s_key[DTRAIN_MAX_PICKS];
    __shared__ uint32_t s_at[DTRAIN_MAX_PICKS], s_rank[DTRAIN_MAX_PICKS];
    __shared__ uint32_t s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < epochs; e += DTRAIN_WG) {
        const uint64_t pick = slots[e];
        if (!(pick >> 32)) continue;
        const uint32_t i = atomicAdd(&s_n, 1u);          // (any order: the keys are distinct, the ranks do not depend on it)
        s_key[i] = dtrain_sort_key(pick, e);
        s_at[i] = dtrain_epoch_lo(e, epochs, R.n) + dtrain_pick_pos(pick);
    }
    __syncthreads();
    const uint32_t n = s_n;
    for (uint32_t i = threadIdx.x; i < n; i += DTRAIN_WG) {
        const uint64_t key = s_key[i];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < n; j++) rank += s_key[j] < key;
        s_rank[i] = rank;
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    for (uint32_t i = threadIdx.x >> 6; i < n; i += DTRAIN_WG / 64) {     // a wavefront per segment; rank < n and n * k <= dict_size
        DtrainCursor c;
        c.seek(R, s_at[i]);
        const uint8_t *a = c.at(R, s_at[i]);
        uint8_t *o = out + (uint64_t)s_rank[i] * k;
        for (uint32_t b = lane; b < k; b += 64) o[b] = a[b];
    }
    if (threadIdx.x == 0) *out_len = (uint64_t)n * k;
}

}  // namespace

#define LFX_LAUNCH_CHECK()                          \
    do {                                            \
        hipError_t e_ = hipGetLastError();          \
        if (e_ != hipSuccess) return (int)e_;       \
    } while (0)

int launch_dict_train(void *st_, const DtrainPlan &pl, const DtrainScratch &w, uint8_t *d, const uint8_t *d_samples, uint8_t *d_dict) {
    hipStream_t st = (hipStream_t)st_;
    const uint32_t n = (uint32_t)pl.n, E = pl.epochs, k = pl.k;
    uint32_t *freq = (uint32_t *)(d + w.freq);
    uint64_t *slots = (uint64_t *)(d + w.slots);
    const DtrainRecs R{(const uint32_t *)(d + w.pos), (const uint64_t *)(d + w.off), (const uint32_t *)(d + w.tile_rec), d_samples, pl.nrec(), n};
    hipLaunchKernelGGL(dtrain_index_kernel, dim3((w.ntiles + DTRAIN_WG - 1) / DTRAIN_WG), dim3(DTRAIN_WG), 0, st, R.pos, R.nrec, w.ntiles,
                       (uint32_t *)(d + w.tile_rec));
    LFX_LAUNCH_CHECK();
    const uint64_t count_wgs = ((uint64_t)n + DTRAIN_WG * DTRAIN_PPL - 1) / (DTRAIN_WG * DTRAIN_PPL);
    hipLaunchKernelGGL(dtrain_count_kernel, dim3((uint32_t)std::min<uint64_t>(count_wgs, DTRAIN_COUNT_GRID)), dim3(DTRAIN_WG), 0, st, R, freq);
    LFX_LAUNCH_CHECK();
    for (uint32_t e = 0; e < E; e++) {
        const uint32_t lo = dtrain_epoch_lo(e, E, n), hi = dtrain_epoch_lo(e + 1, E, n);
        if (hi <= lo) continue;                          // (N < E: an epoch without a position picks nothing)
        const uint32_t chunks = (hi - lo + DTRAIN_CHUNK - 1) / DTRAIN_CHUNK;
        hipLaunchKernelGGL(dtrain_step_kernel, dim3(std::min(chunks, w.step_grid)), dim3(DTRAIN_WG), 0, st, R, freq, slots + e, lo, hi, k,
                           (uint64_t *)(d + w.prefix), w.prefix_words);
        LFX_LAUNCH_CHECK();
        hipLaunchKernelGGL(dtrain_zero_kernel, dim3(1), dim3(DTRAIN_WG), 0, st, R, freq, slots + e, lo, k);
        LFX_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(dtrain_gather_kernel, dim3(1), dim3(DTRAIN_WG), 0, st, R, slots, E, k, d_dict, (uint64_t *)(d + w.out_len));
    LFX_LAUNCH_CHECK();
    return 0;
}

}  // namespace lfx
