// lfx_index.hip — the seek index of a decoded stream (lfx_decode_index_device / lfx_index_read_device).
//
// Kernels: the lanes of the decode's proved blocks gathered for the host (the access-point candidates inside large blocks), the
// probe of an access point in the input (CRC-32 of 64 bytes, BTYPE of a block header), and a batched byte copy (a point's window
// out of the decode's output, a window in front of a segment's staging area, a read's bytes into the caller's buffer).
// Host side: the index (selection over the candidates the decode recorded, export / import / check) and the read path, whose
// segments all decode together, block by block, through the scan / emit / materialise kernels of lfx_inflate_fast.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/lfx.h"
#include "lfx_decode_int.h"
#include "lfx_index.h"
#include "lfx_abi_guard.h"

namespace lfx {

namespace {

constexpr uint32_t IX_THREADS = 256;
constexpr uint32_t IX_UNROLL = 4;     // 16-byte chunks a lane loads before it stores any

// one workgroup per task; a task is at most IDX_COPY_CHUNK bytes (the host splits longer copies)
__global__ __launch_bounds__(IX_THREADS) void idx_copy_kernel(const IdxCopy *__restrict__ tasks) {
    const IdxCopy t = tasks[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    const uint8_t *__restrict__ s = t.src;
    uint8_t *__restrict__ d = t.dst;
    uint64_t len = t.len;
    if ((((uintptr_t)s ^ (uintptr_t)d) & 15) == 0) {
        // same phase: bytes up to the first 16-byte boundary, 16-byte loads and stores, the tail bytes
        const uint64_t h0 = (16 - ((uintptr_t)d & 15)) & 15, head = h0 < len ? h0 : len;
        if (tid < head) d[tid] = s[tid];
        s += head; d += head; len -= head;
        const uint64_t nv = len / 16;
        const uint4 *__restrict__ sv = (const uint4 *)s;
        uint4 *__restrict__ dv = (uint4 *)d;
        for (uint64_t b = 0; b < nv; b += (uint64_t)IX_THREADS * IX_UNROLL) {
            uint4 v[IX_UNROLL];
#pragma unroll
            for (uint32_t k = 0; k < IX_UNROLL; ++k) {
                const uint64_t i = b + k * IX_THREADS + tid;
                if (i < nv) v[k] = sv[i];
            }
#pragma unroll
            for (uint32_t k = 0; k < IX_UNROLL; ++k) {
                const uint64_t i = b + k * IX_THREADS + tid;
                if (i < nv) dv[i] = v[k];
            }
        }
        const uint64_t tail = len - nv * 16;
        if (tid < tail) d[nv * 16 + tid] = s[nv * 16 + tid];
        return;
    }
    // different phases: the destination from its first 16-byte boundary on in aligned 16-byte stores, each made of five aligned
    // dword loads of the source and a byte funnel shift (v_alignbyte); bytes in front and behind one by one
    const uint64_t h0 = (16 - ((uintptr_t)d & 15)) & 15, head = h0 < len ? h0 : len;
    if (tid < head) d[tid] = s[tid];
    s += head; d += head; len -= head;
    const uint32_t sh = (uint32_t)((uintptr_t)s & 3);
    const uint32_t *__restrict__ sw = (const uint32_t *)((uintptr_t)s & ~(uintptr_t)3);
    uint4 *__restrict__ dv = (uint4 *)d;
    // chunk k reads source dwords [4k, 4k + 5) from sw: inside the source while 16 k + 20 <= len + sh
    const uint64_t nv = len + sh >= 20 ? (len + sh - 20) / 16 + 1 : 0;
    for (uint64_t b = 0; b < nv; b += (uint64_t)IX_THREADS * IX_UNROLL) {
        uint32_t w[IX_UNROLL][5];
#pragma unroll
        for (uint32_t k = 0; k < IX_UNROLL; ++k) {
            const uint64_t i = b + k * IX_THREADS + tid;
#pragma unroll
            for (uint32_t j = 0; j < 5; ++j) w[k][j] = i < nv ? sw[4 * i + j] : 0u;
        }
#pragma unroll
        for (uint32_t k = 0; k < IX_UNROLL; ++k) {
            const uint64_t i = b + k * IX_THREADS + tid;
            if (i < nv)
                dv[i] = make_uint4(__builtin_amdgcn_alignbyte(w[k][1], w[k][0], sh), __builtin_amdgcn_alignbyte(w[k][2], w[k][1], sh),
                                   __builtin_amdgcn_alignbyte(w[k][3], w[k][2], sh), __builtin_amdgcn_alignbyte(w[k][4], w[k][3], sh));
        }
    }
    const uint64_t it = nv * 16 + tid;    // (fewer than 20 bytes are left)
    if (it < len) d[it] = s[it];
}

// out[g * 2048 + l] = lanes[slot[g]].start[l], out[g * 2048 + 1024 + l] = lanes[slot[g]].out_off[l]
__global__ __launch_bounds__(IX_THREADS) void idx_lanes_kernel(const BlkLanes *__restrict__ lanes, const uint32_t *__restrict__ slots,
                                                               uint64_t *__restrict__ out) {
    const BlkLanes *L = &lanes[slots[blockIdx.x]];
    uint64_t *o = out + (uint64_t)blockIdx.x * 2048;
    uint64_t a[4], b[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) { a[k] = L->start[threadIdx.x + k * IX_THREADS]; b[k] = L->out_off[threadIdx.x + k * IX_THREADS]; }
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) { o[threadIdx.x + k * IX_THREADS] = a[k]; o[1024 + threadIdx.x + k * IX_THREADS] = b[k]; }
}

// per point: CRC-32 of in[bit / 8, bit / 8 + 64) clipped to [0, n), and the BTYPE of a block header at `bit` (0xFF: past the input)
__global__ __launch_bounds__(IX_THREADS) void idx_probe_kernel(const uint8_t *__restrict__ in, uint64_t n, const uint64_t *__restrict__ bits,
                                                               uint32_t np, uint32_t *__restrict__ crc, uint32_t *__restrict__ btype) {
    const uint32_t i = blockIdx.x * IX_THREADS + threadIdx.x;
    if (i >= np) return;
    const uint64_t bit = bits[i], p = bit >> 3;
    uint8_t v[IDX_CRC_BYTES + 1];
#pragma unroll
    for (uint32_t k = 0; k <= IDX_CRC_BYTES; ++k) v[k] = p + k < n ? in[p + k] : 0;
    uint32_t c = 0xFFFFFFFFu;
#pragma unroll
    for (uint32_t k = 0; k < IDX_CRC_BYTES; ++k) {
        if (p + k < n) {
            c ^= v[k];
#pragma unroll
            for (int j = 0; j < 8; ++j) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
        }
    }
    crc[i] = ~c;
    // the header's three bits: BFINAL, then BTYPE (LSB first), possibly across a byte boundary
    const uint32_t sh = (uint32_t)(bit & 7);
    const uint32_t w = (uint32_t)v[0] | (uint32_t)v[1] << 8;
    btype[i] = p < n ? (w >> (sh + 1)) & 3u : 0xFFu;
}

}  // namespace

int launch_idx_copy(hipStream_t st, const IdxCopy *d_tasks, uint32_t n) {
    if (!n) return 0;
    hipLaunchKernelGGL(idx_copy_kernel, dim3(n), dim3(IX_THREADS), 0, st, d_tasks);
    return (int)hipGetLastError();
}
int launch_idx_lanes(hipStream_t st, const BlkLanes *lanes, const uint32_t *slots, uint32_t n, uint64_t *out) {
    if (!n) return 0;
    hipLaunchKernelGGL(idx_lanes_kernel, dim3(n), dim3(IX_THREADS), 0, st, lanes, slots, out);
    return (int)hipGetLastError();
}
int launch_idx_probe(hipStream_t st, const uint8_t *in, uint64_t n, const uint64_t *bits, uint32_t np, uint32_t *crc, uint32_t *btype) {
    if (!np) return 0;
    hipLaunchKernelGGL(idx_probe_kernel, dim3((np + IX_THREADS - 1) / IX_THREADS), dim3(IX_THREADS), 0, st, in, n, bits, np, crc, btype);
    return (int)hipGetLastError();
}

}  // namespace lfx

// ------------------------------------------------------------------------------------------------
// host side
using namespace lfx;

namespace lfx {

uint32_t idx_crc32(const void *p, uint64_t n, uint32_t crc) {
    static uint32_t tab[256];
    static std::once_flag once;
    std::call_once(once, [] {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int j = 0; j < 8; j++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
            tab[i] = c;
        }
    });
    const uint8_t *b = (const uint8_t *)p;
    uint32_t c = ~crc;
    for (uint64_t i = 0; i < n; i++) c = tab[(c ^ b[i]) & 0xFF] ^ (c >> 8);
    return ~c;
}

namespace {
// tasks of at most IDX_COPY_CHUNK bytes
void split_copies(const std::vector<IdxCopy> &copies, std::vector<IdxCopy> &tasks) {
    tasks.clear();
    for (const IdxCopy &t : copies)
        for (uint64_t o = 0; o < t.len; o += IDX_COPY_CHUNK)
            tasks.push_back(IdxCopy{t.src + o, t.dst + o, std::min<uint64_t>(IDX_COPY_CHUNK, t.len - o)});
}
}  // namespace

// the copies through ONE launch; `tasks` must live until the stream has passed the upload
int idx_copy(Ctx *c, const std::vector<IdxCopy> &copies, std::vector<IdxCopy> &tasks) {
    split_copies(copies, tasks);
    if (tasks.empty()) return LFX_OK;
    int rc;
    if ((rc = c->d_idx_tasks.reserve(sizeof(IdxCopy) * tasks.size()))) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_idx_tasks.p, tasks.data(), sizeof(IdxCopy) * tasks.size(), hipMemcpyHostToDevice, c->stream));
    for (size_t t0 = 0; t0 < tasks.size(); t0 += 1u << 30)
        LAUNCH_TRY(launch_idx_copy(c->stream, (const IdxCopy *)c->d_idx_tasks.p + t0, (uint32_t)std::min<size_t>(tasks.size() - t0, 1u << 30)));
    return LFX_OK;
}

int idx_record_chain(Ctx *c, const BlkEmit *emit, uint32_t ne, const BlkLanes *d_lanes, uint64_t bit_base, uint64_t out_base,
                     bool pieces) {
    IdxCollect &col = *c->idx;
    if (!ne) return LFX_OK;
    // block k spans entries [first, last]; its output is the sum of its pieces'
    IdxCollect::Grab g;
    for (uint32_t i = 0; i < ne;) {
        uint32_t j = i;
        if (pieces) while (j + 1 < ne && emit[j].end_limit != 0) j++;
        uint64_t blk_out = 0;
        for (uint32_t k = i; k <= j; k++) blk_out += emit[k].n_out;
        const BlkEmit &h = emit[i];
        col.cand.push_back(IdxCand{bit_base + h.start_bit, bit_base + h.start_bit, out_base + h.out_off, h.btype});
        if (h.btype != 0 && blk_out > col.spacing)
            for (uint32_t k = i; k <= j; k++) {
                g.slots.push_back(emit[k].cand);
                g.meta.push_back(IdxCollect::Grab::Meta{bit_base + h.start_bit, bit_base, out_base + emit[k].out_off, h.btype,
                                                        std::min<uint32_t>(emit[k].nlanes, 1024), k == i});
            }
        i = j + 1;
    }
    if (g.slots.empty()) return LFX_OK;
    const uint32_t n = (uint32_t)g.slots.size();
    HIP_TRY(hipMalloc(&g.dev, 8ull * 2048 * n + 4ull * n));
    uint32_t *d_slots = (uint32_t *)((uint8_t *)g.dev + 8ull * 2048 * n);
    col.grabs.push_back(std::move(g));
    IdxCollect::Grab &G = col.grabs.back();
    HIP_TRY(hipMemcpyAsync(d_slots, G.slots.data(), 4ull * n, hipMemcpyHostToDevice, c->stream));
    LAUNCH_TRY(launch_idx_lanes(c->stream, d_lanes, d_slots, n, (uint64_t *)G.dev));
    return LFX_OK;
}

namespace {
// the output bytes behind segment p (the next point of its member, or the member's end)
inline uint64_t seg_out_end(const lfx_index *x, uint32_t p) {
    const lfx_index_point &a = x->pts[p];
    if (p + 1 < x->pts.size() && x->pts[p + 1].member == a.member) return x->pts[p + 1].out_off;
    return x->member_end[a.member];
}
// the bit where segment p's decode must stop at the latest: the next point (the next member's first block for a member's
// last segment; the end of the input behind the last member)
inline uint64_t seg_bit_end(const lfx_index *x, uint32_t p) {
    return p + 1 < x->pts.size() ? x->pts[p + 1].in_bit : x->info.in_len * 8;
}
// the segment that holds output byte `o` (< out_len)
inline uint32_t seg_of(const lfx_index *x, uint64_t o) {
    const auto it = std::upper_bound(x->pts.begin(), x->pts.end(), o,
                                     [](uint64_t v, const lfx_index_point &q) { return v < q.out_off; });
    return (uint32_t)(it - x->pts.begin()) - 1;
}
inline uint64_t seg_in_hi(const lfx_index *x, uint32_t p) {
    const uint64_t in_len = x->info.in_len;
    const uint64_t a = (seg_bit_end(x, p) + 7) / 8, b = x->pts[p].in_bit / 8 + IDX_CRC_BYTES;
    return std::min(in_len, std::max(a, b));
}
// device layout of the windows: each at the 16-byte phase of its source in the decode's output
void layout_windows(lfx_index *x) {
    x->win_at.resize(x->pts.size());
    uint64_t at = 0;
    for (size_t i = 0; i < x->pts.size(); i++) {
        const lfx_index_point &p = x->pts[i];
        at = ((at + 15) & ~15ull) + ((p.out_off - p.win_len) & 15);
        x->win_at[i] = at;
        at += p.win_len;
    }
    x->win_bytes = at;
}
uint64_t export_size(const lfx_index *x) {
    uint64_t w = 0;
    for (const lfx_index_point &p : x->pts) w += p.win_len;
    return 64 + 40ull * x->pts.size() + w + 4;
}
template <class T> inline T rd(const uint8_t *p) { T v; memcpy(&v, p, sizeof v); return v; }
template <class T> inline void wr(uint8_t *p, T v) { memcpy(p, &v, sizeof v); }
}  // namespace

int idx_finish(Ctx *c, IdxCollect &col, int format, uint32_t flags, const uint8_t *d_in, uint64_t consumed, const uint8_t *d_out,
               uint64_t out_len, const std::vector<lfx_member> &members, lfx_index **out) {
    hipStream_t st = c->stream;
    // ---- the lanes of the large blocks: of the lanes that start in one grain of spacing / 16 output bytes only the first is
    // kept (a one-block stream has a lane every few KiB: half a million candidates at 128 MiB, whose sort cost ten times the
    // decode; the grains keep every gap between candidates within spacing / 16 plus one lane)
    const uint64_t grain = std::max<uint64_t>(col.spacing / 16, 1);
    uint64_t last_grain = ~0ull;
    for (IdxCollect::Grab &g : col.grabs) {
        const uint32_t n = (uint32_t)g.slots.size();
        std::vector<uint64_t> h(2048ull * n);
        HIP_TRY(hipMemcpyAsync(h.data(), g.dev, 8ull * 2048 * n, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (uint32_t s = 0; s < n; s++) {
            const IdxCollect::Grab::Meta &m = g.meta[s];
            for (uint32_t l = m.skip0 ? 1 : 0; l < m.nlanes; l++) {
                const uint64_t b = h[2048ull * s + l];
                if (b == ~0ull) continue;
                const uint64_t o = m.out_base + h[2048ull * s + 1024 + l];
                if (o / grain == last_grain) continue;
                last_grain = o / grain;
                col.cand.push_back(IdxCand{m.bit_base + b, m.hdr_bit, o, m.btype});
            }
        }
    }
    // (candidates that arrive in stream order — the encode-built ones — skip the sort: 1.6 ms of host time for 65536 of them)
    if (!col.in_order)
        std::sort(col.cand.begin(), col.cand.end(), [](const IdxCand &a, const IdxCand &b) { return a.in_bit < b.in_bit; });
    col.cand.erase(std::unique(col.cand.begin(), col.cand.end(), [](const IdxCand &a, const IdxCand &b) { return a.in_bit == b.in_bit; }),
                   col.cand.end());
    // ---- greedy selection per member
    lfx_index *x = new lfx_index();
    std::unique_ptr<lfx_index> own(x);
    x->c = c;
    const uint64_t sp = col.spacing;
    uint64_t max_gap = 0;
    std::vector<uint8_t> read_btype;
    for (uint32_t mi = 0; mi < (uint32_t)members.size(); mi++) {
        const lfx_member &m = members[mi];
        const uint64_t b0 = m.in_off * 8, b1 = (m.in_off + m.in_len) * 8, o0 = m.out_off, o1 = m.out_off + m.out_len;
        auto lo = std::lower_bound(col.cand.begin(), col.cand.end(), b0, [](const IdxCand &a, uint64_t v) { return a.in_bit < v; });
        auto hi = std::lower_bound(lo, col.cand.end(), b1, [](const IdxCand &a, uint64_t v) { return a.in_bit < v; });
        std::vector<IdxCand> v;
        for (auto it = lo; it != hi; ++it) if (it->out_off >= o0 && it->out_off <= o1) v.push_back(*it);
        if (v.empty() || v[0].out_off != o0 || v[0].in_bit != v[0].hdr_bit) {
            c->set_error("index: the decode recorded no start for member " + std::to_string(mi));
            return LFX_E_DEVICE;
        }
        size_t cur = 0;
        auto push = [&](size_t k) {
            const IdxCand &q = v[k];
            lfx_index_point p{};
            p.in_bit = q.in_bit; p.hdr_bit = q.hdr_bit; p.out_off = q.out_off; p.member = mi;
            p.win_len = (uint32_t)std::min<uint64_t>(IDX_WINDOW, q.out_off - o0);
            p.btype = (uint8_t)(q.btype == IDX_BTYPE_READ ? 0 : q.btype);
            read_btype.push_back(q.btype == IDX_BTYPE_READ);
            x->pts.push_back(p);
        };
        push(0);
        for (;;) {
            if (cur + 1 >= v.size()) break;
            // the last candidate in reach, or the first one after `cur` when none is
            size_t k = cur + 1;
            while (k + 1 < v.size() && v[k + 1].out_off <= v[cur].out_off + sp) k++;
            max_gap = std::max(max_gap, v[k].out_off - v[cur].out_off);
            push(k);
            cur = k;
        }
        max_gap = std::max(max_gap, o1 - v[cur].out_off);
        x->member_end.push_back(o1);
    }
    if (x->pts.empty()) { c->set_error("index: no member"); return LFX_E_DEVICE; }
    c->phase("index_points");
    const uint32_t np = (uint32_t)x->pts.size();
    // ---- windows out of the output, and each point's probe of the input (CRC-32, BTYPE of a block header)
    layout_windows(x);
    HIP_TRY(hipMalloc((void **)&x->d_win, std::max<uint64_t>(x->win_bytes, 16)));
    std::vector<IdxCopy> copies, tasks;
    for (uint32_t i = 0; i < np; i++) {
        const lfx_index_point &p = x->pts[i];
        if (p.win_len) copies.push_back(IdxCopy{d_out + p.out_off - p.win_len, x->d_win + x->win_at[i], p.win_len});
    }
    int rc;
    if ((rc = idx_copy(c, copies, tasks))) return rc;
    std::vector<uint64_t> bits(np);
    for (uint32_t i = 0; i < np; i++) bits[i] = x->pts[i].in_bit;
    if ((rc = c->d_idx_probe.reserve(16ull * np))) return rc;
    uint64_t *d_bits = (uint64_t *)c->d_idx_probe.p;
    uint32_t *d_crc = (uint32_t *)(d_bits + np), *d_bt = d_crc + np;
    HIP_TRY(hipMemcpyAsync(d_bits, bits.data(), 8ull * np, hipMemcpyHostToDevice, st));
    LAUNCH_TRY(launch_idx_probe(st, d_in, consumed, d_bits, np, d_crc, d_bt));
    std::vector<uint32_t> crc(np), bt(np);
    HIP_TRY(hipMemcpyAsync(crc.data(), d_crc, 4ull * np, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(bt.data(), d_bt, 4ull * np, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    c->phase("index_windows");
    for (uint32_t i = 0; i < np; i++) {
        x->pts[i].in_crc = crc[i];
        if (read_btype[i]) {
            if (bt[i] > 2) { c->set_error("index: no block header at bit " + std::to_string(bits[i])); return LFX_E_DEVICE; }
            x->pts[i].btype = (uint8_t)bt[i];
        }
    }
    x->info.in_len = consumed;
    x->info.out_len = out_len;
    x->info.spacing = sp;
    x->info.max_gap = max_gap;
    x->info.format = (uint32_t)format;
    x->info.flags = flags;
    x->info.n_points = np;
    x->info.n_members = (uint32_t)members.size();
    x->info.export_bytes = export_size(x);
    *out = own.release();
    return LFX_OK;
}

}  // namespace lfx

// ------------------------------------------------------------------------------------------------
// C ABI

extern "C" int lfx_index_get_info(const lfx_index *idx, lfx_index_info *info) try {
    if (!idx || !info) return LFX_E_ARG;
    *info = idx->info;
    return LFX_OK;
} LFX_ABI_CATCH

extern "C" int lfx_index_get_point(const lfx_index *idx, uint32_t i, lfx_index_point *p) try {
    if (!idx || !p || i >= idx->pts.size()) return LFX_E_ARG;
    *p = idx->pts[i];
    return LFX_OK;
} LFX_ABI_CATCH

extern "C" int lfx_index_span(const lfx_index *idx, uint64_t off, uint64_t len, uint64_t *in_lo, uint64_t *in_hi) try {
    if (!idx || !in_lo || !in_hi) return LFX_E_ARG;
    const uint64_t ol = idx->info.out_len;
    if (off > ol) return LFX_E_ARG;
    const uint64_t e = len > ol - off ? ol : off + len;
    if (e == off) { *in_lo = *in_hi = 0; return LFX_OK; }
    const uint32_t p0 = seg_of(idx, off), p1 = seg_of(idx, e - 1);
    uint64_t hi = 0;
    uint64_t lo = ~0ull;
    for (uint32_t p = p0; p <= p1; p++) {
        hi = std::max(hi, seg_in_hi(idx, p));
        lo = std::min(lo, idx->pts[p].hdr_bit / 8);   // (a segment that starts inside a block parses that block's header)
    }
    *in_lo = lo;
    *in_hi = hi;
    return LFX_OK;
} LFX_ABI_CATCH

lfx_index::~lfx_index() {
    if (d_win) {
        (void)hipSetDevice(c->device);
        (void)hipFree(d_win);
    }
}

extern "C" void lfx_index_free(lfx_index *idx) { delete idx; }

extern "C" int lfx_index_check(const void *buf, uint64_t len, lfx_index_info *info) try {
    const uint8_t *b = (const uint8_t *)buf;
    if (!b || len < 64 + 4) return LFX_E_INVALID_DATA;
    if (memcmp(b, "LFXINDEX", 8) != 0 || rd<uint32_t>(b + 8) != 1) return LFX_E_INVALID_DATA;
    const uint32_t format = rd<uint32_t>(b + 12), flags = rd<uint32_t>(b + 16), n = rd<uint32_t>(b + 20);
    const uint64_t in_len = rd<uint64_t>(b + 24), out_len = rd<uint64_t>(b + 32), spacing = rd<uint64_t>(b + 40), max_gap = rd<uint64_t>(b + 48);
    const uint32_t n_members = rd<uint32_t>(b + 56);
    if (format > 2 || (flags & ~LFX_DEC_MULTI) || ((flags & LFX_DEC_MULTI) && format != LFX_GZIP)) return LFX_E_INVALID_DATA;
    if (rd<uint32_t>(b + 60) != 0 || n == 0) return LFX_E_INVALID_DATA;
    if (len < 64 + 40ull * n + 4) return LFX_E_INVALID_DATA;
    uint64_t wsum = 0;
    uint64_t m_first_out = 0;
    for (uint32_t i = 0; i < n; i++) {
        lfx_index_point p;
        memcpy(&p, b + 64 + 40ull * i, 40);
        if (p._pad[0] || p._pad[1] || p._pad[2]) return LFX_E_INVALID_DATA;
        if (i == 0) {
            if (p.out_off != 0 || p.member != 0) return LFX_E_INVALID_DATA;
        } else {
            lfx_index_point q;
            memcpy(&q, b + 64 + 40ull * (i - 1), 40);
            if (p.in_bit <= q.in_bit || p.out_off < q.out_off) return LFX_E_INVALID_DATA;
            if (p.member != q.member && p.member != q.member + 1) return LFX_E_INVALID_DATA;
        }
        const bool first = i == 0 || rd<uint32_t>(b + 64 + 40ull * (i - 1) + 24) != p.member;
        if (p.hdr_bit > p.in_bit || p.btype > 2 || (p.btype == 0 && p.hdr_bit != p.in_bit)) return LFX_E_INVALID_DATA;
        if (first) {
            if (p.in_bit != p.hdr_bit || p.win_len != 0) return LFX_E_INVALID_DATA;
            m_first_out = p.out_off;
        }
        if (p.win_len > IDX_WINDOW || p.win_len != std::min<uint64_t>(IDX_WINDOW, p.out_off - m_first_out)) return LFX_E_INVALID_DATA;
        if (p.out_off > out_len || p.in_bit >= 8 * in_len) return LFX_E_INVALID_DATA;
        if (i + 1 == n && n_members != p.member + 1) return LFX_E_INVALID_DATA;
        wsum += p.win_len;
    }
    if (len != 64 + 40ull * n + wsum + 4) return LFX_E_INVALID_DATA;
    if (idx_crc32(b, len - 4) != rd<uint32_t>(b + len - 4)) return LFX_E_INVALID_DATA;
    if (info) {
        info->in_len = in_len; info->out_len = out_len; info->spacing = spacing; info->max_gap = max_gap; info->export_bytes = len;
        info->format = format; info->flags = flags; info->n_points = n; info->n_members = n_members;
    }
    return LFX_OK;
} LFX_ABI_CATCH

extern "C" int lfx_index_export(lfx_ctx *cc, const lfx_index *idx, void *buf, uint64_t cap, uint64_t *len) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    if (!idx || idx->c != c || !len) return LFX_E_ARG;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    const uint64_t sz = export_size(idx);
    *len = sz;
    if (!buf || cap < sz) return LFX_E_NOSPACE;
    (void)hipSetDevice(c->device);
    std::vector<uint8_t> w(idx->win_bytes);
    if (idx->win_bytes) HIP_TRY(hipMemcpy(w.data(), idx->d_win, idx->win_bytes, hipMemcpyDeviceToHost));
    uint8_t *o = (uint8_t *)buf;
    memset(o, 0, 64);
    memcpy(o, "LFXINDEX", 8);
    const lfx_index_info &f = idx->info;
    wr<uint32_t>(o + 8, 1); wr<uint32_t>(o + 12, f.format); wr<uint32_t>(o + 16, f.flags); wr<uint32_t>(o + 20, f.n_points);
    wr<uint64_t>(o + 24, f.in_len); wr<uint64_t>(o + 32, f.out_len); wr<uint64_t>(o + 40, f.spacing); wr<uint64_t>(o + 48, f.max_gap);
    wr<uint32_t>(o + 56, f.n_members); wr<uint32_t>(o + 60, 0);
    uint8_t *q = o + 64;
    for (const lfx_index_point &p : idx->pts) { memcpy(q, &p, 40); q += 40; }
    for (size_t i = 0; i < idx->pts.size(); i++) {
        memcpy(q, w.data() + idx->win_at[i], idx->pts[i].win_len);
        q += idx->pts[i].win_len;
    }
    wr<uint32_t>(q, idx_crc32(o, (uint64_t)(q - o)));
    return LFX_OK;
} LFX_ABI_CATCH

extern "C" lfx_index *lfx_index_import(lfx_ctx *cc, const void *buf, uint64_t len, int *status) try {
    if (!cc) { if (status) *status = LFX_E_DEVICE; return nullptr; }
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    lfx_index_info info;
    int rc = lfx_index_check(buf, len, &info);
    if (rc) { if (status) *status = rc; return nullptr; }
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    (void)hipSetDevice(c->device);
    std::unique_ptr<lfx_index> x(new lfx_index());
    x->c = c;
    x->info = info;
    const uint8_t *b = (const uint8_t *)buf;
    x->pts.resize(info.n_points);
    memcpy(x->pts.data(), b + 64, 40ull * info.n_points);
    x->member_end.assign(info.n_members, 0);
    for (uint32_t i = 0; i < info.n_points; i++) {
        const uint32_t m = x->pts[i].member;
        if (m > 0 && (i == 0 || x->pts[i - 1].member != m)) x->member_end[m - 1] = x->pts[i].out_off;
    }
    x->member_end[info.n_members - 1] = info.out_len;
    layout_windows(x.get());
    std::vector<uint8_t> w(std::max<uint64_t>(x->win_bytes, 16), 0);
    const uint8_t *src = b + 64 + 40ull * info.n_points;
    for (uint32_t i = 0; i < info.n_points; i++) { memcpy(w.data() + x->win_at[i], src, x->pts[i].win_len); src += x->pts[i].win_len; }
    if (hipMalloc((void **)&x->d_win, w.size()) != hipSuccess) { if (status) *status = LFX_E_OOM; return nullptr; }
    if (hipMemcpy(x->d_win, w.data(), w.size(), hipMemcpyHostToDevice) != hipSuccess) {
        if (status) *status = LFX_E_DEVICE;
        return nullptr;
    }
    if (status) *status = LFX_OK;
    return x.release();
} LFX_ABI_CATCH_NEW

// ------------------------------------------------------------------------------------------------
// reads: the segments [point p, next point) that the reads touch, decoded together block by block
namespace {

constexpr uint64_t IDX_STAGE_BUDGET = 1ull << 30;   // staging bytes of one group of segments
constexpr uint64_t IDX_SLACK = 96u << 10;           // room behind a segment's need: the last step's overshoot (a stored block: < 64 KiB)

struct Seg {
    uint32_t p;
    uint64_t need;          // output bytes of the segment the reads want (from its point on)
    uint64_t seg_len;       // output bytes of the whole segment
    bool full;              // need == seg_len: the decode must end exactly at the next point (or at the member's end)
    bool member_end;        // the segment is its member's last: it ends at the BFINAL block's EndOfBlock
    uint64_t s_end;         // bit the decode must not pass
    uint64_t stage;         // its staging area in d_idx_stage: 32 KiB of window, then the output
    uint64_t cap;           // output room
    uint64_t bit, hdr, produced;
    bool in_block;          // the next step continues the block at `hdr` from `bit` (else a block starts at `bit`)
    uint64_t range_cap;     // != 0: the next step's bit range is at most this (a step that did not fit or converge)
    bool live;
    int status;
    std::string msg;
};

std::string point_msg(uint32_t p, const char *what) {
    return "index point " + std::to_string(p) + ": " + what;
}

// the rounds of one group of segments; on return every segment is settled (status) and, when LFX_OK, its output lies at
// d_stage + stage + IDX_WINDOW
int decode_group(Ctx *c, const lfx_index *x, const uint8_t *d_in, uint64_t in_base, uint64_t n, std::vector<Seg> &segs) {
    hipStream_t st = c->stream;
    uint8_t *d_stage = (uint8_t *)c->d_idx_stage.p;
    const uint64_t base_bit = in_base * 8;
    int rc;
    // ---- each point's bytes checked against the input held, the windows in front of the staging areas
    const uint32_t ns = (uint32_t)segs.size();
    {
        std::vector<uint64_t> bits(ns);
        for (uint32_t k = 0; k < ns; k++) bits[k] = x->pts[segs[k].p].in_bit - base_bit;
        if ((rc = c->d_idx_probe.reserve(16ull * ns))) return rc;
        uint64_t *d_bits = (uint64_t *)c->d_idx_probe.p;
        uint32_t *d_crc = (uint32_t *)(d_bits + ns), *d_bt = d_crc + ns;
        const uint64_t held = std::min<uint64_t>(n, x->info.in_len > in_base ? x->info.in_len - in_base : 0);
        HIP_TRY(hipMemcpyAsync(d_bits, bits.data(), 8ull * ns, hipMemcpyHostToDevice, st));
        LAUNCH_TRY(launch_idx_probe(st, d_in, held, d_bits, ns, d_crc, d_bt));
        std::vector<IdxCopy> copies, tasks;
        for (const Seg &s : segs) {
            const lfx_index_point &p = x->pts[s.p];
            if (p.win_len) copies.push_back(IdxCopy{x->d_win + x->win_at[s.p], d_stage + s.stage + IDX_WINDOW - p.win_len, p.win_len});
        }
        if ((rc = idx_copy(c, copies, tasks))) return rc;
        std::vector<uint32_t> crc(ns);
        HIP_TRY(hipMemcpyAsync(crc.data(), d_crc, 4ull * ns, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (uint32_t k = 0; k < ns; k++)
            if (crc[k] != x->pts[segs[k].p].in_crc) {
                segs[k].live = false;
                segs[k].status = LFX_E_INVALID_DATA;
                segs[k].msg = point_msg(segs[k].p, "the input bytes at the point do not match the index");
            }
    }
    // ---- rounds: every live segment takes one step (a block from its header, or the rest of a block from a known symbol
    // boundary), bounded by the bits its remaining need is estimated to take; the steps that fit are materialised at once
    for (;;) {
        std::vector<uint32_t> live;
        for (uint32_t k = 0; k < ns; k++) if (segs[k].live) live.push_back(k);
        if (live.empty()) break;
        const uint32_t nj = (uint32_t)live.size();
        std::vector<BlkJob> bj(nj);
        for (uint32_t q = 0; q < nj; q++) {
            const Seg &s = segs[live[q]];
            const lfx_index_point &p = x->pts[s.p];
            // bits per output byte of this segment (its whole span when known)
            const uint64_t sb = seg_bit_end(x, s.p) - p.in_bit;
            const uint64_t left = (s.full ? s.seg_len : s.need) - std::min(s.produced, s.full ? s.seg_len : s.need);
            uint64_t est = s.seg_len ? (uint64_t)((double)left * ((double)sb / (double)s.seg_len) * 1.25) : sb;
            est = std::max<uint64_t>(est + 1024, 4096);
            if (s.range_cap) est = std::min(est, s.range_cap);
            const uint64_t e = std::min(s.bit + est, s.s_end);
            BlkJob j{};
            j.start_bit = s.hdr - base_bit;
            j.end_bit = e - base_bit;
            j.lo_bit = s.in_block ? s.bit - base_bit : 0;
            j.warm_bit = 0;
            j.piece = s.in_block ? BLK_PIECE_KNOWN : 1u;
            bj[q] = j;
        }
        std::vector<BlkInfo> bi;
        bool small = false;
        if ((rc = scan_round(c, d_in, n, bj, true, bi, small))) return rc;
        std::vector<BlkEmit> emit;
        std::vector<uint32_t> owner;
        uint64_t total_codes = 0;
        for (uint32_t q = 0; q < nj; q++) {
            Seg &s = segs[live[q]];
            const BlkInfo &r = bi[q];
            auto fail = [&](const char *what) { s.live = false; s.status = LFX_E_INVALID_DATA; s.msg = point_msg(s.p, what); };
            const uint64_t range = bj[q].end_bit - (s.bit - base_bit);
            if (r.status == BLK_BAD) {
                // a speculative scan that did not converge is retried over a shorter range; anything else is damage
                if (r.rounds >= 64 && range > 128) { s.range_cap = std::max<uint64_t>(range / 2, 128); continue; }
                fail("the segment does not decode");
                continue;
            }
            const uint64_t end = r.end_bit + base_bit;
            if (r.end_bit > n * 8 || end > s.s_end || end <= s.bit) { fail("the segment does not end at the next point"); continue; }
            if (s.in_block && r.btype == 0) { fail("the segment does not decode"); continue; }
            // the first step parses the header the point names: its BTYPE must be the one the index recorded
            if (s.bit == x->pts[s.p].in_bit && r.btype != x->pts[s.p].btype) {
                fail("the block header at the point does not match the index");
                continue;
            }
            if (s.produced + r.n_out > s.cap) {
                if (range > 128 && r.btype != 0) { s.range_cap = std::max<uint64_t>(range / 2, 128); continue; }
                fail("the segment produces more output than the index says");
                continue;
            }
            BlkEmit e = blk_emit_of(r, s.hdr - base_bit, q, s.stage + IDX_WINDOW + s.produced, total_codes,
                                    x->pts[s.p].win_len + s.produced);
            e.preload = e.hist != 0;
            emit.push_back(e);
            owner.push_back(live[q]);
            total_codes += r.n_codes;
            s.range_cap = 0;
            s.produced += r.n_out;
            const bool closed = r.status == BLK_OK;
            s.bit = end;
            if (closed) { s.hdr = end; s.in_block = false; } else s.in_block = true;
            // ---- where the segment stands
            const lfx_index_point *qn = s.p + 1 < x->pts.size() ? &x->pts[s.p + 1] : nullptr;
            if (closed && r.bfinal) {
                if (!s.member_end) fail("the member ends before the next point");
                else if (s.full && s.produced != s.seg_len) fail("the member's end does not lie where the index says");
                else s.live = false;
                continue;
            }
            if (s.full) {
                if (s.produced > s.seg_len) { fail("the segment produces more output than the index says"); continue; }
                if (!s.member_end && s.bit == s.s_end) {
                    const bool at_block = qn->in_bit == qn->hdr_bit;
                    if (s.produced != s.seg_len || at_block == s.in_block || (s.in_block && s.hdr != qn->hdr_bit))
                        fail("the segment does not end at the next point");
                    else s.live = false;
                }
            } else if (s.produced >= s.need) s.live = false;
        }
        const uint32_t ne = (uint32_t)emit.size();
        if (!ne) continue;
        std::vector<uint32_t> jf;
        if ((rc = emit_round(c, d_in, n, emit, total_codes, small, d_stage, jf))) return rc;
        for (uint32_t q = 0; q < ne; q++)
            if (jf[q] && segs[owner[q]].status == LFX_OK) {     // a back-reference in front of the point's window
                Seg &s = segs[owner[q]];
                s.live = false;
                s.status = LFX_E_INVALID_DATA;
                s.msg = point_msg(s.p, "a back-reference reaches in front of the window");
            }
    }
    return LFX_OK;
}

}  // namespace

extern "C" int lfx_index_read_device(lfx_ctx *cc, const lfx_index *idx, const void *d_in_, uint64_t in_base, uint64_t n,
                                     uint32_t count, const uint64_t *off, const uint64_t *len, void *d_out_,
                                     const uint64_t *out_off, uint64_t *out_len_r, int32_t *status) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    if (!idx || idx->c != c) return LFX_E_ARG;
    if (count && (!off || !len || !out_off)) return LFX_E_ARG;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    (void)hipSetDevice(c->device);
    c->n_ev = 0;
    c->phase("start");
    const uint8_t *d_in = (const uint8_t *)d_in_;
    uint8_t *d_out = (uint8_t *)d_out_;
    const lfx_index *x = idx;
    const uint64_t OL = x->info.out_len;
    const uint32_t np = (uint32_t)x->pts.size();
    std::vector<int> rs(count, LFX_OK);
    std::vector<std::string> rmsg(count);
    std::vector<uint64_t> re(count, 0);      // end of read i (clipped); == off[i]: nothing to write
    std::vector<uint64_t> need(np, 0);
    for (uint32_t i = 0; i < count; i++) {
        if (off[i] > OL) { rs[i] = LFX_E_ARG; continue; }
        const uint64_t e = len[i] > OL - off[i] ? OL : off[i] + len[i];
        re[i] = e;
        if (e == off[i]) continue;
        uint64_t lo = 0, hi = 0;
        lfx_index_span(x, off[i], e - off[i], &lo, &hi);
        if (lo < in_base || hi > in_base + n) { rs[i] = LFX_E_ARG; re[i] = off[i]; continue; }
        for (uint32_t p = seg_of(x, off[i]), p1 = seg_of(x, e - 1); p <= p1; p++)
            need[p] = std::max(need[p], std::min(e, seg_out_end(x, p)) - x->pts[p].out_off);
    }
    // ---- segments, in groups whose staging areas fit the budget
    std::vector<uint32_t> seg_ids;
    for (uint32_t p = 0; p < np; p++) if (need[p]) seg_ids.push_back(p);
    std::vector<int> pst(np, LFX_OK);
    std::vector<std::string> pmsg(np);
    std::vector<IdxCopy> copies, tasks;
    int rc;
    for (size_t g0 = 0; g0 < seg_ids.size();) {
        std::vector<Seg> segs;
        uint64_t at = 0;
        size_t g1 = g0;
        for (; g1 < seg_ids.size(); g1++) {
            const uint32_t p = seg_ids[g1];
            const uint64_t room = ((need[p] + IDX_SLACK + 255) & ~255ull);
            const uint64_t sz = 256 + IDX_WINDOW + room;
            if (!segs.empty() && at + sz > IDX_STAGE_BUDGET) break;
            Seg s{};
            s.p = p;
            s.need = need[p];
            s.seg_len = seg_out_end(x, p) - x->pts[p].out_off;
            s.full = s.need == s.seg_len;
            s.member_end = !(p + 1 < np && x->pts[p + 1].member == x->pts[p].member);
            s.s_end = seg_bit_end(x, p);
            s.stage = at + (x->pts[p].out_off & 15);
            s.cap = room;
            s.bit = x->pts[p].in_bit;
            s.hdr = x->pts[p].hdr_bit;
            s.in_block = s.bit != s.hdr;
            s.live = true;
            s.status = LFX_OK;
            segs.push_back(s);
            at += sz;
        }
        if ((rc = c->d_idx_stage.reserve(at))) return rc;
        if ((rc = decode_group(c, x, d_in, in_base, n, segs))) return rc;
        if (c->n_ev < 12) c->phase("seg_rounds");
        for (const Seg &s : segs) { pst[s.p] = s.status; pmsg[s.p] = s.msg; }
        // ---- the reads' bytes out of this group's segments
        copies.clear();
        const uint8_t *d_stage = (const uint8_t *)c->d_idx_stage.p;
        for (uint32_t i = 0; i < count; i++) {
            if (rs[i] != LFX_OK || re[i] == off[i]) continue;
            const uint32_t p0 = seg_of(x, off[i]), p1 = seg_of(x, re[i] - 1);
            for (const Seg &s : segs) {
                if (s.p < p0 || s.p > p1 || s.status != LFX_OK) continue;
                const uint64_t so = x->pts[s.p].out_off;
                const uint64_t a = std::max(off[i], so), b = std::min(re[i], so + s.need);
                if (b > a) copies.push_back(IdxCopy{d_stage + s.stage + IDX_WINDOW + (a - so), d_out + out_off[i] + (a - off[i]), b - a});
            }
        }
        if ((rc = idx_copy(c, copies, tasks))) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
        g0 = g1;
    }
    if (c->n_ev < 16) c->phase("seg_copy");
    int first = LFX_OK;
    for (uint32_t i = 0; i < count; i++) {
        if (rs[i] == LFX_OK && re[i] > off[i])
            for (uint32_t p = seg_of(x, off[i]), p1 = seg_of(x, re[i] - 1); p <= p1; p++)
                if (pst[p] != LFX_OK) { rs[i] = pst[p]; rmsg[i] = pmsg[p]; break; }
        if (status) status[i] = rs[i];
        if (out_len_r) out_len_r[i] = rs[i] == LFX_OK ? re[i] - off[i] : 0;
        if (rs[i] != LFX_OK && first == LFX_OK) {
            first = rs[i];
            c->set_error(rmsg[i].empty() ? "read " + std::to_string(i) + ": out of range" : rmsg[i]);
        }
    }
    return first;
} LFX_ABI_CATCH
