// lfx_device.h — device-side descriptors and the kernel launchers (lfx_*_kernels.hip) used by
// lfx_api.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lfx.h"
#include "lfx_common.h"

namespace lfx {

struct EncodeResult {
    uint64_t end_bit;    // bit after the last DEFLATE bit (absolute, container header included)
    uint64_t out_bytes;  // bytes of output relative to the output base
    uint32_t status;     // 0 ok, 1 capacity exceeded
    uint32_t crc32;
    uint32_t adler32;
    uint32_t match_flags;  // bit 0: the second-generation match kernel saw an LDS lane-order violation (results void);
                           // bit 1: one of its segments held runs of equal bytes (its sample) — the parse walk takes its instance for such data
};

// one stream of a batch encode: where its bytes lie, where its output goes, which blocks of the merged plan are its own
struct BatchStream {
    uint64_t in_off, in_len;
    uint64_t out_off, out_cap;
    uint32_t first_block, n_blocks;
};

int launch_match(hipStream_t st, const uint8_t *in, uint64_t in_bytes, const ChunkDesc *chunks,
                 const SegDesc *segs, uint32_t nsegs, uint32_t window, uint32_t max_len, uint32_t *md,
                 uint64_t *dbg = nullptr);
// candidate stage: per position the distance to the most recent earlier occurrence of its 3-byte prefix (0 = none) → cd.
// flags[0] |= 1 on a lane-order violation.
// lfx_match7.hip (round 5, the default): two-level bucket LRU with exact tags + the resolver kernel for the few positions
// it leaves open.  glnk: scratch for the duplicate-collapsed link of every position of every segment (warm-up included),
// regions by SegDesc::lnk_base
int launch_match7(hipStream_t st, const uint8_t *in, uint64_t in_bytes, const ChunkDesc *chunks, const SegDesc *segs,
                  uint32_t nsegs, uint32_t window, uint16_t *cd, uint32_t *glnk /* link | tag << 16 per link entry */,
                  uint64_t *umask /* 8 bytes per 64 link entries */, uint32_t *flags, uint64_t *dbg = nullptr);
// ... and the positions it leaves open (ballot words → a list per segment → chain walks through glnk): behind the
// candidate kernel of the same segments.  ucount: zeroed by the caller.
int launch_resolve7(hipStream_t st, const ChunkDesc *chunks, const SegDesc *segs, uint32_t nsegs, uint32_t window, uint16_t *cd,
                    const uint32_t *glnk, const uint64_t *umask, uint32_t *ulist /* 4 bytes per input byte */,
                    uint32_t *ucount /* 4 bytes per segment */);
// the first-generation kernel's answers (length << 16 | distance) → cd
int launch_md_to_cd(hipStream_t st, const uint32_t *md, uint64_t n, uint16_t *cd);
// the greedy walk with lazy match lengths (lfx_parse2.hip) → code words per chunk, in two launchers: the persistent walk kernel
// (n_cu: the device's compute units, one workgroup each) ...
int launch_parse_walk(hipStream_t st, const uint8_t *in, uint64_t in_bytes, const ChunkDesc *chunks, uint32_t nsegs, const ParseWg *wgs,
                      uint32_t nwgs, uint32_t n_cu, const uint16_t *cd, uint32_t max_len, uint64_t *vis, uint32_t *seg_tmp,
                      uint32_t *stage /* 4 bytes per input byte */,
                      const uint32_t *mflags /* EncodeResult::match_flags of this call (bit 1 picks the walk's instance) */,
                      uint64_t *dbg /* LFX_DEBUG: cycle stamps of one walk workgroup */,
                      const uint8_t *dict_win /* a preset dictionary's 32 KiB device window, its usable tail at the end: the
                                                 dictionary instances of the walking kernels serve the CH_DICT chunks */,
                      uint32_t dict_usable);
// ... and the chaining kernels behind it: fixseg, fix, emit.  The caller may fork a side stream between the two (stage_parse).
int launch_parse_chain(hipStream_t st, const uint8_t *in, uint64_t in_bytes, const ChunkDesc *chunks, uint32_t nchunks, uint32_t nsegs,
                       const uint16_t *cd, uint32_t max_len, uint64_t *vis, uint32_t *seg_tmp, uint32_t *codes, uint32_t *ncodes,
                       uint32_t *stage, const uint32_t *seg_map,
                       uint32_t *hist /* 320 zeroed counters per block: the code words are counted as they are emitted
                                         (launch_histogram is then not needed); nullptr: not counted */,
                       uint32_t emit_per /* with hist: segments per emit workgroup ... */,
                       uint32_t emit_parts /* ... and workgroups for the chunk of most segments (grid = nchunks x emit_parts) */,
                       const uint8_t *dict_win, bool fixseg_only = false /* diagnostics (LFX_DUMP_SEG): stop behind fixseg */,
                       bool hist_by_chunk = false /* hist holds 320 zeroed counters per CHUNK (pack by chunk) */);
struct ZeroSpan { uint32_t *p; uint32_t n; };      // n words at p to be cleared (by the kernel that runs first anyway)
int launch_chunk_maps(hipStream_t st, const ChunkDesc *chunks, uint32_t nchunks, uint64_t ntiles, uint32_t nsegs,
                      uint32_t *tile_map, uint32_t *seg_map, ZeroSpan z0 = ZeroSpan{nullptr, 0}, ZeroSpan z1 = ZeroSpan{nullptr, 0},
                      ZeroSpan z2 = ZeroSpan{nullptr, 0});
int launch_histogram(hipStream_t st, const ChunkDesc *chunks, uint32_t nchunks, uint32_t split,
                     const uint32_t *codes, const uint32_t *ncodes, uint32_t *hist);
int launch_huffman(hipStream_t st, const BlockDesc *blocks, uint32_t nblocks, const uint32_t *hist,
                   BlockCodes *bc, uint64_t *dbg = nullptr);
// LFX_HUFFMAN_AUTO: every BT_DYNAMIC block of the device table becomes the smallest of its dynamic, fixed and —
// stored_ok — stored form; choice[b] = the type block b leaves with
int launch_block_choose(hipStream_t st, BlockDesc *blocks, uint32_t nblocks, const uint32_t *hist, BlockCodes *bc, bool stored_ok,
                        uint8_t *choice);
// block_merge, behind launch_huffman: one workgroup per region (merge_regions, lfx_merge.h) joins neighbouring
// dynamic blocks where one code is no longer than two and rewrites the device's block, chunk, code-count and counter tables;
// merge_head[b] = the block candidate b ends up in (the caller presets the identity).  launch_huffman runs again behind it.
struct MergeRegion;
int launch_block_merge(hipStream_t st, const MergeRegion *regions, uint32_t nregions, BlockDesc *blocks, ChunkDesc *chunks,
                       uint32_t *ncodes, uint32_t *hist, BlockCodes *bc, uint32_t *merge_head);
int launch_offsets(hipStream_t st, const BlockDesc *blocks, uint32_t nblocks, const BlockCodes *bc,
                   uint64_t start_bit, uint64_t cap_bits, uint64_t *block_start, EncodeResult *res);
int launch_offsets_batch(hipStream_t st, const BatchStream *streams, uint32_t count, const BlockDesc *blocks, const BlockCodes *bc,
                         uint32_t hdr_len, uint32_t trailer_len, uint64_t *block_start, uint64_t *stream_end, int32_t *status,
                         EncodeResult *res);
int launch_frame_batch(hipStream_t st, int format, const BatchStream *streams, uint32_t count, const uint8_t *hdr, uint32_t hdr_len,
                       const uint64_t *stream_end, const uint32_t *crc, const uint32_t *adler, const EncodeResult *res, uint32_t *out,
                       uint64_t *out_len);
// lfx_encode_members_device (lfx_members_enc.hip): the members are regular, so this is all the kernels need to know of them —
// member m is input bytes [m * member_size, min(n, (m + 1) * member_size)) and blocks [m * bpm, + bpm) (the last: bpm_last)
struct MembersGeom {
    uint64_t n, member_size;
    uint32_t count;
    uint32_t bpm, bpm_last;     // blocks per member of the merged plan
    uint32_t hdr_len;           // the shared gzip header
    uint32_t bgzf;              // LFX_MEMBERS_BGZF: BSIZE in every header, the stored fallback, the end-of-file marker
};
// behind the Huffman kernel: every member's length (BGZF: its stored form where the compressed one exceeds 65536 bytes), the
// device-wide exclusive scan of the lengths, block_start[] at the final offsets, blocks[].type of fallen-back members = BT_RAW,
// members[] complete; res->out_bytes = the total (BGZF: marker included), res->status = 1 when it exceeds cap.
// local_off, mlen: 8 bytes per member; wg_sum: 8 bytes per 256 members (at least 8)
int launch_members_layout(hipStream_t st, const MembersGeom &g, BlockDesc *blocks, const BlockCodes *bc, uint64_t *local_off,
                          uint64_t *mlen, uint64_t *wg_sum, uint64_t cap, uint64_t *block_start, lfx_member *members,
                          EncodeResult *res);
// behind pack: headers, trailers, the end-of-file marker (nothing when res->status != 0)
int launch_members_frame(hipStream_t st, const MembersGeom &g, const uint8_t *hdr, const lfx_member *members, const uint32_t *crc,
                         const EncodeResult *res, uint32_t *out);
// the second level of that scan alone: wg_sum[0, nwg) → its exclusive scan in place, res->out_bytes = the sum (and res->end_bit
// = 8 x), res->status = 1 when it exceeds cap
int launch_scan_wg_sums(hipStream_t st, uint64_t *wg_sum, uint32_t nwg, uint64_t cap, EncodeResult *res);
// lfx_encode_batch_packed_device (lfx_batch_pack.hip) in the place of launch_offsets_batch: every stream's length
// (header and trailer included), the device-wide scan of round_up(length, align) — the last stream's unrounded —, then per stream
// streams[].out_off / out_cap = its offset and length, block_start[] and stream_end[] from there, pairs[] = {off, len} (and the
// same into table, the caller's, where given); res->out_bytes = the total, res->status = 1 when it exceeds cap.
// local_off, slen, stream_end: 8 bytes per stream; pairs: 16; wg_sum: 8 bytes per 256 streams
int launch_batch_pack_layout(hipStream_t st, BatchStream *streams, uint32_t count, const BlockDesc *blocks, const BlockCodes *bc,
                             uint32_t hdr_len, uint32_t trailer_len, uint32_t align, uint64_t cap, uint64_t *local_off, uint64_t *slen,
                             uint64_t *wg_sum, uint64_t *block_start, uint64_t *stream_end, uint64_t *pairs, uint64_t *table,
                             EncodeResult *res);
int launch_pack(hipStream_t st, const uint8_t *in, uint64_t in_bytes, const ChunkDesc *chunks,
                uint32_t nchunks, const BlockDesc *blocks, uint32_t nblocks, uint64_t ntiles,
                const uint32_t *codes, const uint32_t *ncodes, const BlockCodes *bc,
                const uint64_t *block_start, uint32_t *tile_bits, uint64_t *tile_start,
                const EncodeResult *res, uint64_t out_base_bit, uint32_t *out, const uint32_t *tile_map);
// pack by chunk.  hist_chunk: 320 counters per chunk, as launch_parse_chain(hist_by_chunk) left them; chunk_bits:
// 2 * nchunks words — every chunk's packed size, then its first bit behind its block's header.  launch_pack_chunks takes the
// place of launch_pack; check: a chunk whose walk does not end at its counted size raises res->status (2).
int launch_huffman_chunks(hipStream_t st, const BlockDesc *blocks, uint32_t nblocks, uint32_t nchunks, const uint32_t *hist_chunk,
                          BlockCodes *bc, uint64_t *chunk_bits, uint64_t *dbg = nullptr);
int launch_pack_chunks(hipStream_t st, const uint8_t *in, uint64_t in_bytes, const ChunkDesc *chunks, uint32_t nchunks,
                       const BlockDesc *blocks, uint32_t nblocks, const uint32_t *codes, const uint32_t *ncodes, const BlockCodes *bc,
                       const uint64_t *block_start, const uint64_t *chunk_bits, bool check, EncodeResult *res, uint64_t out_base_bit,
                       uint32_t *out, uint32_t n_cu);
// span of the checksum kernels = the bytes one wavefront folds serially: 64 KiB; 8 KiB up to 64 MiB (a 1 MiB buffer is
// sixteen 64 KiB spans — sixteen wavefronts on the whole GPU, each walking sixteen dependent pieces: 0.12 ms; 16 MiB are 256)
inline uint32_t ck_span(uint64_t n) { return n <= (64ull << 20) ? 8192u : 65536u; }
inline uint64_t ck_nspans(uint64_t n) { return div_up(n ? n : 1, ck_span(n)); }   // partials needed: 3 x 4 bytes each
int launch_checksum(hipStream_t st, const uint8_t *in, uint64_t n, uint32_t *crc_part,
                    uint32_t *a_part, uint32_t *b_part, EncodeResult *res,
                    int mode = 3)   /* bit 0: CRC-32, bit 1: Adler-32 (the other result is then 0) */;
// the same sweep in `nparts` launches (the caller orders them; the last one folds all spans)
int launch_checksum_part(hipStream_t st, const uint8_t *in, uint64_t n, uint32_t *crc_part, uint32_t *a_part, uint32_t *b_part,
                         EncodeResult *res, int mode, uint32_t part, uint32_t nparts);
// CRC-32 / Adler-32 of count byte ranges data[off[i*off_stride] .. +len[i*len_stride]) (strides in 8-byte units)
int launch_checksum_ranges(hipStream_t st, const uint8_t *data, uint32_t count, const uint64_t *off,
                           uint32_t off_stride, const uint64_t *len, uint32_t len_stride, uint32_t *crc, uint32_t *adler);
int launch_or_byte(hipStream_t st, uint8_t *dst, const uint8_t *src);
int launch_put_bytes(hipStream_t st, const uint8_t *d_bytes, uint32_t n, uint64_t at_byte, uint32_t *out);
int launch_trailer(hipStream_t st, int format, uint32_t isize, uint64_t out_base_bit,
                   EncodeResult *res, uint32_t *out);

}  // namespace lfx
