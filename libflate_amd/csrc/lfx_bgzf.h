// lfx_bgzf.h — BGZF reads by virtual offset (lfx_bgzf_read_*): what the device walk (lfx_bgzf.hip) and the
// host walk (lfx_decode.cpp) share — the parse of a block's fixed header and trailer, the walk itself, and the records the
// walk leaves for the decode and the gather.
//
// A BGZF block in htslib's form: 1f 8b 08 04 | mtime[4] xfl os | 06 00 | 42 43 02 00 | BSIZE[2] | deflate ... | CRC32[4] ISIZE[4],
// BSIZE + 1 bytes in all.  A walk hops from block to block by BSIZE alone; ONE window of 22 bytes around a block start — the
// ISIZE of the block in front and the 18 header bytes of the block that starts there — is all it reads per hop, so a hop
// costs one dependent load.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lfx.h"
#include "lfx_common.h"

namespace lfx {

constexpr uint32_t BGZF_HEAD = 18;           // the fixed header
constexpr uint32_t BGZF_MIN_BLOCK = 26;      // header + 8-byte trailer: the least BSIZE + 1 the form admits
constexpr uint32_t BGZF_MAX_ISIZE = 65536;
constexpr uint32_t BGZF_WINDOW = 4 + BGZF_HEAD;   // bytes [p - 4, p + 18) around a block start p
constexpr uint32_t BGZF_GATHER_PIECE = 16384;     // bytes one workgroup of the gather copies

// why a walk stopped with an error (BgzfWalk::err; the message names err_coff)
enum : uint32_t { BGZF_ERR_NONE = 0, BGZF_ERR_RANGE, BGZF_ERR_HEADER, BGZF_ERR_ISIZE, BGZF_ERR_CUT, BGZF_ERR_UOFFSET };

// one (read, block) pair: bytes [first, last) of the block's output go to byte out_pos of the read's output
struct BgzfSeg {
    uint64_t coffset;   // the block's first byte in the file
    uint64_t out_pos;
    uint32_t read;
    uint32_t blen;      // BSIZE + 1
    uint32_t isize;
    uint32_t first, last;
    uint32_t ord;       // the segment's number inside its read = blocks that contributed in front of it
};                      // 40 bytes
struct BgzfWalk {
    uint64_t out_len, next_voff;
    uint64_t err_coff;  // the block a failed walk stood at
    int32_t status;     // LFX_*
    uint32_t n_blocks;
    uint32_t err;       // BGZF_ERR_*
    uint32_t _pad;
};                      // 40 bytes
struct BgzfCopy {       // one piece of a segment: scratch[src, src + len) -> out[dst, dst + len)
    uint64_t src, dst;
    uint32_t len, _pad;
};                      // 24 bytes

// The parse of a window w = file bytes [p - 4, p + 18): isize_before = the ISIZE of the block that ends at p, block_len = the
// length of the block that starts at p, 0 when those 18 bytes are not a BGZF header.
LFX_HD inline void bgzf_parse_window(const uint8_t *w, uint32_t &isize_before, uint32_t &block_len) {
    isize_before = (uint32_t)w[0] | (uint32_t)w[1] << 8 | (uint32_t)w[2] << 16 | (uint32_t)w[3] << 24;
    const uint8_t *h = w + 4;
    const bool ok = h[0] == 0x1f && h[1] == 0x8b && h[2] == 8 && h[3] == 4 && h[10] == 6 && h[11] == 0 && h[12] == 0x42 &&
                    h[13] == 0x43 && h[14] == 2 && h[15] == 0;
    const uint32_t len = ((uint32_t)h[16] | (uint32_t)h[17] << 8) + 1;
    block_len = ok && len >= BGZF_MIN_BLOCK ? len : 0;
}

// The walk of ONE read over the held file bytes [lo, hi) (include/lfx.h, rules 1-4 and 6).
//   fetch(p, w): w[0, 22) = file bytes [p - 4, p + 18), zero where they lie outside [lo, hi)
//   emit(seg):   a block that contributes at least one byte, in walk order
// Every decision is taken from values that are the same in all lanes of a wavefront, so on the device the walk runs
// uniformly and fetch / emit decide which lanes load and store.
template <class Fetch, class Emit>
LFX_HD inline void bgzf_walk(const lfx_bgzf_read &r, uint32_t read_idx, uint64_t lo, uint64_t hi, Fetch &&fetch, Emit &&emit,
                             BgzfWalk &o) {
    const uint64_t co = r.voff >> 16, e_co = r.end_voff >> 16;
    const uint32_t uo = (uint32_t)(r.voff & 0xffff), e_uo = (uint32_t)(r.end_voff & 0xffff);
    o.out_len = 0;
    o.next_voff = r.voff;
    o.err_coff = co;
    o.status = LFX_OK;
    o.n_blocks = 0;
    o.err = BGZF_ERR_NONE;
    o._pad = 0;
    if (co < lo || co > hi) { o.status = LFX_E_ARG; o.err = BGZF_ERR_RANGE; return; }
    if (r.end_voff <= r.voff || co == hi) return;
    uint8_t w[BGZF_WINDOW];
    uint64_t pos = co, delivered = 0;
    uint32_t start = uo, nb = 0, isize = 0, blen = 0, next_len = 0;
    bool first = true;
    fetch(pos, w);
    bgzf_parse_window(w, isize, blen);
    for (;;) {
        // (o.next_voff is the position behind the last byte delivered)
        if (pos == hi || pos > e_co || (pos == e_co && e_uo <= start)) return;   // a short read; end_voff at or in front of this block
        int fail = LFX_OK;
        uint32_t why = BGZF_ERR_NONE;
        if (hi - pos < BGZF_HEAD) { fail = LFX_E_UNEXPECTED_EOF; why = BGZF_ERR_CUT; }
        else if (!blen) { fail = LFX_E_INVALID_DATA; why = BGZF_ERR_HEADER; }
        else if (blen > hi - pos) { fail = LFX_E_UNEXPECTED_EOF; why = BGZF_ERR_CUT; }
        if (!fail) {
            fetch(pos + blen, w);                            // this block's ISIZE and the next block's header: one load
            bgzf_parse_window(w, isize, next_len);
            if (isize > BGZF_MAX_ISIZE) { fail = LFX_E_INVALID_DATA; why = BGZF_ERR_ISIZE; }
            else if (first && uo > isize) { fail = LFX_E_ARG; why = BGZF_ERR_UOFFSET; }
        }
        if (fail) {
            o.status = fail;
            o.err = why;
            o.err_coff = pos;
            o.next_voff = pos << 16 | start;
            return;
        }
        const uint32_t lim = pos == e_co && e_uo < isize ? e_uo : isize;
        const uint64_t avail = lim > start ? lim - start : 0, room = r.len - delivered;
        const uint32_t take = (uint32_t)(avail < room ? avail : room);
        if (take) {
            BgzfSeg s;
            s.coffset = pos; s.out_pos = delivered; s.read = read_idx; s.blen = blen; s.isize = isize;
            s.first = start; s.last = start + take; s.ord = nb;
            emit(s);
            nb++;
        }
        delivered += take;
        const uint32_t at = start + take;
        o.out_len = delivered;
        o.n_blocks = nb;
        o.next_voff = at == isize ? (pos + blen) << 16 : pos << 16 | at;
        if (at < isize || delivered == r.len || pos >= e_co) return;
        pos += blen;
        start = 0;
        first = false;
        blen = next_len;
    }
}

// reads / seg_off / segs / out: device arrays.  Read i's segments go to segs[seg_off[i], seg_off[i + 1]) — those that fit; its
// n_blocks counts all of them.  segs == nullptr: no list (size mode, a counting pass).
int launch_bgzf_hop(hipStream_t st, const uint8_t *in, uint64_t in_base, uint64_t n, uint32_t count, const lfx_bgzf_read *reads,
                    const uint64_t *seg_off, BgzfSeg *segs, BgzfWalk *out);
int launch_bgzf_gather(hipStream_t st, const uint8_t *scratch, uint8_t *out, const BgzfCopy *tasks, uint32_t ntasks);

}  // namespace lfx
