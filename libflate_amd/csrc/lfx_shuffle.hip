// lfx_shuffle.hip — the byte-shuffle filter's kernels (lfx_shuffle_*).  One launch serves a whole batch: a
// workgroup takes one item of lfx_shuffle.h's tile list — (record, first element, element count) — and the item that holds a
// record's last element also copies the record's trailing bytes.
//   shuf_reg_kernel<S, DIR>   s in {2, 4, 8, 16}.  A lane takes E elements (16 bytes at s = 2 and 4, 32 at 8, 64 at 16) with
//                             16-byte loads, splits them per byte plane with v_perm_b32 and stores one dword (s = 2: two) per
//                             plane: a wavefront writes 256 (512) contiguous bytes of every plane.  No LDS.  Unshuffle mirrors
//                             it: s plane loads, the permutes, 16-byte stores.
//   shuf_lds_kernel<DIR>      every other s.  The item's elements go through LDS, an element at a stride of s | 1 bytes: the
//                             interleaved side is read (written) as consecutive dwords, the plane side as dwords of four
//                             consecutive elements of one plane, whose LDS bytes lie s | 1 dwords apart from lane to lane — an
//                             odd number, so the 32 lanes of a group meet 32 banks.
// The edge rule.  A record's place, k and so every plane's start j * k are arbitrary and neighbouring records are written
// concurrently, so no store may touch a byte outside its plane's range: a dword (or wider) store is issued only where all its
// bytes are elements of this item in one plane, or bytes of this item's interleaved range; everything else is a byte store.
// The wide accesses are not aligned in general — global memory takes them at any address — and there is no read-modify-write.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfx_shuffle.h"

namespace lfx {

namespace {

template <class T> __device__ __forceinline__ T ld(const uint8_t *p) { T v; __builtin_memcpy(&v, p, sizeof v); return v; }
template <class T> __device__ __forceinline__ void st(uint8_t *p, T v) { __builtin_memcpy(p, &v, sizeof v); }

// v_perm_b32: byte n of the result is byte sel[n] of {hi, lo} (0..3: lo, 4..7: hi, 0x0c: zero)
__device__ __forceinline__ uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel) { return __builtin_amdgcn_perm(hi, lo, sel); }

template <int S> struct Reg {
    static constexpr int E = S == 2 ? 8 : 4;      // elements of a lane
    static constexpr int W = E * S / 4;           // its dwords on the interleaved side
    static constexpr int G = E / 4;               // its dwords of one plane
};

// w: E elements of S bytes → p[j][g]: the bytes j of the elements 4g .. 4g + 3
template <int S> __device__ __forceinline__ void split(const uint32_t (&w)[Reg<S>::W], uint32_t (&p)[S][Reg<S>::G]) {
#pragma unroll
    for (int j = 0; j < S; j++)
#pragma unroll
        for (int g = 0; g < Reg<S>::G; g++) {
            if constexpr (S == 2) {
                p[j][g] = perm(w[2 * g + 1], w[2 * g], (uint32_t)j | (2 + j) << 8 | (4 + j) << 16 | (6 + j) << 24);
            } else {
                const uint32_t b = j & 3, sel = b | (4 + b) << 8 | 0x0c0c0000u;
                const int at = j / 4, es = S / 4;         // the word of byte j inside an element, an element's words
                const uint32_t lo = perm(w[(4 * g + 1) * es + at], w[(4 * g) * es + at], sel);
                const uint32_t hi = perm(w[(4 * g + 3) * es + at], w[(4 * g + 2) * es + at], sel);
                p[j][g] = perm(hi, lo, 0x05040100u);
            }
        }
}

// the inverse
template <int S> __device__ __forceinline__ void join(const uint32_t (&p)[S][Reg<S>::G], uint32_t (&w)[Reg<S>::W]) {
#pragma unroll
    for (int q = 0; q < Reg<S>::W; q++) {
        if constexpr (S == 2) {
            const uint32_t x = 2 * (q & 1);
            w[q] = perm(p[1][q / 2], p[0][q / 2], x | (4 + x) << 8 | (x + 1) << 16 | (5 + x) << 24);
        } else {
            const int e = 4 * q / S, j0 = 4 * q % S, g = e / 4;
            const uint32_t x = e & 3, sel = x | (4 + x) << 8 | 0x0c0c0000u;
            const uint32_t lo = perm(p[j0 + 1][g], p[j0][g], sel);
            const uint32_t hi = perm(p[j0 + 3][g], p[j0 + 2][g], sel);
            w[q] = perm(hi, lo, 0x05040100u);
        }
    }
}

// the r trailing bytes of a record, by the item that holds its last element (r < s <= 256 = SHUF_WG)
__device__ __forceinline__ void copy_tail(const ShufItem &it, const ShufRec &r, uint64_t k, uint32_t s, const uint8_t *src, uint8_t *dst) {
    if (it.e0 + it.cnt != k) return;
    const uint64_t body = k * s;
    if (threadIdx.x < r.len - body) dst[body + threadIdx.x] = src[body + threadIdx.x];
}

template <int S, int DIR>
__global__ __launch_bounds__(SHUF_WG) void shuf_reg_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out,
                                                           const ShufRec *__restrict__ recs, const ShufItem *__restrict__ items) {
    constexpr int E = Reg<S>::E, W = Reg<S>::W, G = Reg<S>::G;
    const ShufItem it = items[blockIdx.x];
    const ShufRec r = recs[it.rec];
    const uint64_t k = r.len / S;
    const uint8_t *src = in + r.in_off;
    uint8_t *dst = out + r.out_off;
    for (uint32_t i = threadIdx.x * E; i < it.cnt; i += SHUF_WG * E) {
        const uint64_t e = it.e0 + i;
        if (i + E <= it.cnt) {
            uint32_t w[W], p[S][G];
            if (DIR == 0) {
#pragma unroll
                for (int q = 0; q < W / 4; q++) {
                    const uint4 v = ld<uint4>(src + e * S + 16 * q);
                    w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
                }
                split<S>(w, p);
#pragma unroll
                for (int j = 0; j < S; j++) {
                    if constexpr (G == 1) st<uint32_t>(dst + j * k + e, p[j][0]);
                    else st<uint2>(dst + j * k + e, uint2{p[j][0], p[j][1]});
                }
            } else {
#pragma unroll
                for (int j = 0; j < S; j++) {
                    if constexpr (G == 1) p[j][0] = ld<uint32_t>(src + j * k + e);
                    else { const uint2 v = ld<uint2>(src + j * k + e); p[j][0] = v.x; p[j][1] = v.y; }
                }
                join<S>(p, w);
#pragma unroll
                for (int q = 0; q < W / 4; q++) st<uint4>(dst + e * S + 16 * q, uint4{w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]});
            }
        } else {
            // the item's ragged end: fewer than E elements, byte by byte
            for (uint32_t m = 0; i + m < it.cnt; m++)
                for (uint32_t j = 0; j < S; j++) {
                    if (DIR == 0) dst[j * k + e + m] = src[(e + m) * S + j];
                    else dst[(e + m) * S + j] = src[j * k + e + m];
                }
        }
    }
    copy_tail(it, r, k, S, src, dst);
}

template <int DIR>
__global__ __launch_bounds__(SHUF_WG) void shuf_lds_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out,
                                                           const ShufRec *__restrict__ recs, const ShufItem *__restrict__ items, uint32_t s) {
    __shared__ uint8_t lds[SHUF_LDS_BYTES];
    const ShufItem it = items[blockIdx.x];
    const ShufRec r = recs[it.rec];
    const uint64_t k = r.len / s;
    const uint8_t *src = in + r.in_off;
    uint8_t *dst = out + r.out_off;
    const uint32_t ps = s | 1, cnt = it.cnt, nb = cnt * s;         // (cnt * ps <= SHUF_LDS_BYTES: lfx_shuffle.h)
    const uint32_t gpp = (cnt + 3) / 4, ngroups = gpp * s;         // groups of four elements: per plane, in all
    // the interleaved side walks dwords b = 4 * lane, + 4 * SHUF_WG, ...; (q, x) = (b / s, b % s) is stepped, not divided
    const uint32_t dq = 4 * SHUF_WG / s, dx = 4 * SHUF_WG % s;
    uint32_t q = 4 * threadIdx.x / s, x = 4 * threadIdx.x % s;
    if (DIR == 0) {
        const uint8_t *g = src + it.e0 * s;
        for (uint32_t b = 4 * threadIdx.x; b < nb; b += 4 * SHUF_WG) {
            const uint32_t n = nb - b < 4 ? nb - b : 4;
            uint32_t w = 0;
            if (n == 4) w = ld<uint32_t>(g + b);
            else for (uint32_t m = 0; m < n; m++) w |= (uint32_t)g[b + m] << (8 * m);
            uint32_t qq = q, xx = x;
            for (uint32_t m = 0; m < n; m++) {
                lds[qq * ps + xx] = (uint8_t)(w >> (8 * m));
                if (++xx == s) { xx = 0; qq++; }
            }
            q += dq; x += dx;
            if (x >= s) { x -= s; q++; }
        }
        __syncthreads();
        for (uint32_t t = threadIdx.x; t < ngroups; t += SHUF_WG) {
            const uint32_t j = t / gpp, i = (t - j * gpp) * 4;
            const uint32_t n = cnt - i < 4 ? cnt - i : 4;
            uint8_t *o = dst + j * k + it.e0 + i;
            uint32_t w = 0;
            for (uint32_t m = 0; m < n; m++) w |= (uint32_t)lds[(i + m) * ps + j] << (8 * m);
            if (n == 4) st<uint32_t>(o, w);
            else for (uint32_t m = 0; m < n; m++) o[m] = (uint8_t)(w >> (8 * m));
        }
    } else {
        for (uint32_t t = threadIdx.x; t < ngroups; t += SHUF_WG) {
            const uint32_t j = t / gpp, i = (t - j * gpp) * 4;
            const uint32_t n = cnt - i < 4 ? cnt - i : 4;
            const uint8_t *g = src + j * k + it.e0 + i;
            uint32_t w = 0;
            if (n == 4) w = ld<uint32_t>(g);
            else for (uint32_t m = 0; m < n; m++) w |= (uint32_t)g[m] << (8 * m);
            for (uint32_t m = 0; m < n; m++) lds[(i + m) * ps + j] = (uint8_t)(w >> (8 * m));
        }
        __syncthreads();
        uint8_t *o = dst + it.e0 * s;
        for (uint32_t b = 4 * threadIdx.x; b < nb; b += 4 * SHUF_WG) {
            const uint32_t n = nb - b < 4 ? nb - b : 4;
            uint32_t w = 0, qq = q, xx = x;
            for (uint32_t m = 0; m < n; m++) {
                w |= (uint32_t)lds[qq * ps + xx] << (8 * m);
                if (++xx == s) { xx = 0; qq++; }
            }
            if (n == 4) st<uint32_t>(o + b, w);
            else for (uint32_t m = 0; m < n; m++) o[b + m] = (uint8_t)(w >> (8 * m));
            q += dq; x += dx;
            if (x >= s) { x -= s; q++; }
        }
    }
    copy_tail(it, r, k, s, src, dst);
}

template <int S>
void launch_reg(hipStream_t st, int dir, uint32_t n, const uint8_t *in, uint8_t *out, const ShufRec *recs, const ShufItem *items) {
    if (dir == 0) hipLaunchKernelGGL((shuf_reg_kernel<S, 0>), dim3(n), dim3(SHUF_WG), 0, st, in, out, recs, items);
    else hipLaunchKernelGGL((shuf_reg_kernel<S, 1>), dim3(n), dim3(SHUF_WG), 0, st, in, out, recs, items);
}

}  // namespace

int launch_shuffle(void *stream, int dir, uint32_t s, const uint8_t *d_in, uint8_t *d_out, const ShufRec *d_recs, const ShufItem *d_items,
                   uint32_t nitems) {
    hipStream_t st = (hipStream_t)stream;
    if (!nitems) return 0;
    switch (s) {
    case 2: launch_reg<2>(st, dir, nitems, d_in, d_out, d_recs, d_items); break;
    case 4: launch_reg<4>(st, dir, nitems, d_in, d_out, d_recs, d_items); break;
    case 8: launch_reg<8>(st, dir, nitems, d_in, d_out, d_recs, d_items); break;
    case 16: launch_reg<16>(st, dir, nitems, d_in, d_out, d_recs, d_items); break;
    default:
        if (dir == 0) hipLaunchKernelGGL(shuf_lds_kernel<0>, dim3(nitems), dim3(SHUF_WG), 0, st, d_in, d_out, d_recs, d_items, s);
        else hipLaunchKernelGGL(shuf_lds_kernel<1>, dim3(nitems), dim3(SHUF_WG), 0, st, d_in, d_out, d_recs, d_items, s);
    }
    return (int)hipGetLastError();
}

}  // namespace lfx
