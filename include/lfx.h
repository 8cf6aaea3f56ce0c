/*
 * lfx.h — C ABI of the MI355X-native DEFLATE hot path (drop-in boundary for sile/libflate).
 *
 * Every entry point names the reference interface it replaces (file:line in libflate v2.3.0).
 * Plain pointers and sizes only; no torch / HIP types in the signatures (a HIP stream is
 * passed as an opaque void*).  All compression / decompression work runs in hand-written HIP
 * kernels for gfx950; there is NO CPU fallback: without a usable device every compute call
 * returns LFX_E_DEVICE.
 *
 * Bit-exactness contract: compressed bytes are a function of (input bytes, sequence of write()
 * sizes, options) exactly as in the reference (SURVEY.md "fact 2").  One lfx_encoder_write()
 * call == one `Write::write` call; the one-shot calls take an explicit lfx_schedule.
 */
#ifndef LFX_H
#define LFX_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LFX_VERSION 0x000100

/* container formats: libflate::{deflate,zlib,gzip} */
enum { LFX_DEFLATE = 0, LFX_ZLIB = 1, LFX_GZIP = 2 };

/* status codes ~ io::ErrorKind used by the reference (src/lib.rs:10-29, src/bit.rs:132-141) */
enum {
    LFX_OK = 0,
    LFX_E_INVALID_DATA = 1,   /* io::ErrorKind::InvalidData  */
    LFX_E_UNEXPECTED_EOF = 2, /* io::ErrorKind::UnexpectedEof */
    LFX_E_IO = 3,             /* error returned by a user callback */
    LFX_E_OOM = 4,
    LFX_E_DEVICE = 5,         /* no device / HIP failure (never a silent CPU fallback) */
    LFX_E_ARG = 6,            /* out-of-domain option */
    LFX_E_NOSPACE = 7,        /* output capacity too small */
    LFX_E_UNSUPPORTED = 8,
    LFX_E_WOULD_BLOCK = 9     /* io::ErrorKind::WouldBlock: a read callback of a non-blocking decoder has nothing yet */
};

/* libflate_lz77::CompressionLevel (libflate_lz77/src/lib.rs:44-58) */
enum { LFX_LEVEL_NONE = 0, LFX_LEVEL_FAST = 1, LFX_LEVEL_BALANCE = 2, LFX_LEVEL_BEST = 3 };
/* which Lz77Encode implementation (lib.rs:83-145, default.rs:14-51) */
enum { LFX_LZ77_DEFAULT = 0, LFX_LZ77_NOCOMPRESSION = 1, LFX_LZ77_CHAIN = 2, LFX_LZ77_LAZY = 3 };
/* LFX_LZ77_CHAIN — ChainLz77Encoder(depth K, window_size W, max_length M), an Lz77Encode of this library's own (the reference
 * takes any through EncodeOptions::with_lz77, encode.rs:59-65): DefaultLz77Encoder with the longest of K chained candidates
 * instead of the one most recent.  Opt-in; the default stays bit-exact with the reference.
 *  - Buffering is DefaultLz77Encoder's: encode appends and flushes at W * 8 bytes (default.rs:60-68).
 *  - flush is default.rs:69-109 with one change at a visited position i < end.  Let c1 > c2 > ... be the earlier occurrences of
 *    buf[i..i+3] in this buffer, most recent first (every position < end is inserted once, in order, as in the reference).  The
 *    candidates are c1 .. cK, cut off at the first ck with i - ck > W; none: a literal, as in the reference.
 *    L(c) = 3 + longest_common_prefix(buf, i + 3, c + 3), capped by M and by the end of the buffer (default.rs:122-129).
 *    Emitted: Pointer{L(c*), i - c*}, c* the candidate of the greatest L, among equal lengths the nearest (the first one met);
 *    then i += L.  (A walk may stop once L == min(M, n - i): nothing can be longer.)
 *  - compression_level() is Best: with lz77_level == 0 zlib's FLEVEL is 3 and gzip's XFL is 2 (no_compression resets both, as
 *    for any Lz77Encode); a caller's lz77_level wins.
 *  - At K = 1 the code words are the reference's.
 * lz77_kind & 0xFF is the kind; for LFX_LZ77_CHAIN bits 8..15 hold the depth K, 1..255 — there is no default depth.  Depth 0 or
 * any bit above 15 set: LFX_E_ARG.  For the kinds 0 and 1 the bits above bit 7 are not read.
 * Served by lfx_encode_device / _host, lfx_encode_batch_device, lfx_encoder_* (bytes mode), lfx_encode_members_* (BGZF too) and
 * lfx_encode_index_device; by the dictionary encode calls with a chain dictionary (lfx_dict_new_chain, below).
 * LFX_E_UNSUPPORTED from the dictionary encode calls with a plain dictionary (a dictionary candidate has no chain behind
 * it) and from the N-GPU encode (lfx_encode_shard_prepare, lfx_sharded_encode_begin); the lfx_lz77 plug-in handle takes no
 * options and stays DefaultLz77Encoder. */
#define LFX_LZ77_CHAIN_DEPTH(k) (LFX_LZ77_CHAIN | (k) << 8)
/* LFX_LZ77_LAZY — LazyLz77Encoder(depth K, window_size W, max_length M): ChainLz77Encoder with zlib's lazy rule (deflate_slow)
 * on top.  Opt-in, a kind of its own.
 *  - Buffering and candidates are ChainLz77Encoder's.  For a position p < end with candidates, L(p) and D(p) are the length
 *    and the distance of the candidate ChainLz77Encoder emits there (the longest of the first K, among equal lengths the
 *    nearest); L(p) = 0 where there is no candidate, and for every p >= end.  Both are functions of the position alone: every
 *    position < end is inserted once, in order, whatever the walk visits.
 *  - The walk at a visited i < end: L(i) != 0 and L(i + 1) <= L(i): Pointer{L(i), D(i)}, i += L(i).  Otherwise
 *    Literal(buf[i]), i += 1.  The tail is the reference's (default.rs:105-107).  There is no max_lazy, no good_length and no
 *    TOO_FAR: a run of deferrals is as long as the lengths keep rising.
 *  - compression_level() is Best, with the FLEVEL / XFL rules of LFX_LZ77_CHAIN.
 * Bits 8..15 hold the depth K, 1..255; depth 0 or any bit above 15 set: LFX_E_ARG.  Served and refused (LFX_E_UNSUPPORTED)
 * by the same entry points as LFX_LZ77_CHAIN. */
#define LFX_LZ77_LAZY_DEPTH(k) (LFX_LZ77_LAZY | (k) << 8)
/* LFX_LZ77_LEVEL — LevelLz77Encoder(level 1..9, window_size W, max_length M): the chained parse tuned the way zlib's deflate
 * tunes its own, by one number.  Opt-in, a kind of its own; the output is NOT bit-exact with zlib's and does
 * not claim to be.  The level resolves into five values, zlib's configuration_table without good_length:
 *
 *      level  walk     depth K   nice N   max_lazy Z   too_far F
 *        1    greedy       4        8         -            -
 *        2    greedy       8       16         -            -
 *        3    greedy      32       32         -            -
 *        4    lazy        16       16         4          4096
 *        5    lazy        32       32        16          4096
 *        6    lazy       128      128        16          4096
 *        7    lazy       256      128        32          4096
 *        8    lazy      1024      258       128          4096
 *        9    lazy      4096      258       258          4096
 *
 *  - Buffering is ChainLz77Encoder's; window_size and max_length hold as for it.  lim = min(M, n - i) at a position i.
 *  - Candidates: c1 .. cK as for LFX_LZ77_CHAIN (most recent first, cut off at the first one farther than W).  The walk along
 *    them ends behind the first candidate whose length is >= min(N, lim); that candidate is included.  L(p), D(p): the greatest
 *    length among the candidates walked and its distance, among equal lengths the nearest; L(p) = 0 without a candidate and for
 *    every p >= end.
 *  - Too far (the lazy levels only): L(p) == 3 and D(p) > F: the position has no candidate, L(p) = 0.
 *  - The greedy walk (levels 1..3) is LFX_LZ77_CHAIN's over these L and D.
 *  - The lazy walk (levels 4..9) at a visited i < end: Pointer{L(i), D(i)}, i += L(i) when L(i) != 0 and (L(i) >= Z or
 *    L(i + 1) <= L(i)); otherwise Literal(buf[i]), i += 1.  A position is deferred exactly when L(i + 1) > L(i) and L(i) < Z.
 *    The tail is the reference's (default.rs:105-107).
 *  - L and D are functions of the position alone, as for the kinds 2 and 3.  zlib's good_length is NOT modelled: it shortens
 *    the search at p + 1 to a quarter of the chain when the match at p has good_length bytes or more, which makes L(p + 1)
 *    depend on what the walk did at p — there would be no per-position L to compute ahead of the walk.
 *  - compression_level(), with lz77_level == 0: Fast for the levels 1..3 (zlib's FLEVEL 1, gzip's XFL 4), Balance for 4..6
 *    (FLEVEL 2, XFL 0), Best for 7..9 (FLEVEL 3, XFL 2).  A caller's lz77_level wins; no_compression resets it, as for any kind.
 * lz77_kind & 0xFF is the kind; bits 8..15 hold the level.  Level 0, a level above 9 or any bit above 15 set: LFX_E_ARG.
 * Served and refused (LFX_E_UNSUPPORTED) by the same entry points as LFX_LZ77_CHAIN and LFX_LZ77_LAZY, LFX_HUFFMAN_AUTO and a
 * chain dictionary included; through a chain dictionary the candidates run on into the dictionary's tail as theirs do, under
 * the same rules. */
enum { LFX_LZ77_LEVEL = 4 };
#define LFX_LZ77_LEVEL_N(n) (LFX_LZ77_LEVEL | (n) << 8)
/* LFX_LZ77_COST — CostLz77Encoder(level 1..9, window_size W, max_length M): LevelLz77Encoder(level) with the lazy rule replaced by
 * a choice by cost in bits.  Opt-in; a valid stream, deterministic, not zlib's bytes.  (The value is 6: 5 names no
 * kind and stays LFX_E_ARG.)
 *  - Candidates: L(p), D(p) of LFX_LZ77_LEVEL at the same level — depth K, nice N and too_far F of its row (the levels 1..3 have no
 *    too-far rule).  max_lazy is not used.  Buffering, window_size, max_length and the tail are LFX_LZ77_LEVEL's.
 *  - For a flushed buffer with visited range [0, end): lit(p) = the width of the literal buf[p]; mat(p) = the width of L(p)'s
 *    length symbol + its extra bits + the width of D(p)'s distance symbol + its extra bits.  All widths are those of the block
 *    that owns the buffer's code words.
 *  - The widths.  dynamic_huffman = 0: the fixed code's.  Otherwise: the code the same call builds in a first pass — the greedy
 *    walk over L and D (no position demoted), the block's symbol counts, the plain dynamic code, without LFX_HUFFMAN_AUTO and
 *    without block_merge.  A symbol without a code in that pass costs one bit more than the longest code of its alphabet
 *    (literal/length, distance) in that block; an alphabet without any code costs 9 (literal/length) or 5 (distance).
 *  - The recurrence.  The buffer is cut on a grid of COST_SEG = 4096 positions from its start.  For a segment [a, b) it starts
 *    at top = min(b + COST_WARM, end), COST_WARM = 512, with cost[top] = 0 and runs backward:
 *        cost[p] = min(lit(p) + cost[p + 1], mat(p) + cost[min(p + L(p), top)])       the match term only where L(p) != 0
 *    On a tie the match wins.  For p in [a, b): where the literal won the position loses its candidate, L(p) = 0; the positions
 *    of the warm-up are the next segment's to decide.  Nothing is read across a buffer.
 *  - The walk is LFX_LZ77_CHAIN's greedy one over what is left of L and D.
 *  - compression_level() is Best (FLEVEL 3, XFL 2), with the rules of LFX_LZ77_CHAIN.
 * lz77_kind & 0xFF is the kind; bits 8..15 hold the level.  Level 0, a level above 9 or any bit above 15 set: LFX_E_ARG.
 * Served as LFX_LZ77_LEVEL is — one-shot, batch, packed batch, a chain dictionary, lfx_encoder_* (bytes mode), members and BGZF,
 * with LFX_HUFFMAN_AUTO and block_merge on top (both decide on the final pass' code words) — with two exceptions:
 * lfx_encode_index_device is LFX_E_UNSUPPORTED (a second parse would list its candidates twice), and so is the N-GPU encode. */
enum { LFX_LZ77_COST = 6 };
#define LFX_LZ77_COST_N(n) (LFX_LZ77_COST | (n) << 8)
/* lfx_encode_opts::dynamic_huffman.  0: fixed codes for every block (fixed_huffman_codes(), encode.rs:107-110).  1, and every
 * value other than 0 and 2: dynamic codes for every block (the reference's default).
 * LFX_HUFFMAN_AUTO (2) — opt-in, not a reference option: per block the smallest of the dynamic, the fixed and
 * the stored form.  (Until this value was defined, 2 was read as "non-zero, so dynamic": it no longer is.)
 *  - The plan, the LZ77 code words, the block boundaries and the container header (FLEVEL, XFL) are those of
 *    dynamic_huffman = 1, for every lz77_kind.
 *  - Every block that plan makes a dynamic block is a candidate; its stored blocks (no_compression, the zlib sync marker) are
 *    not touched.  For a candidate, D = the bits of its dynamic form (3 + header + symbols); F = 3 + the sum over its own symbol
 *    counts, EndOfBlock included, of count * (fixed code width + extra bits); S = 8 * in_len + 42, the stored form at its worst
 *    alignment, so that the choice does not depend on the bit phase.  S is eligible only when the block has input bytes behind
 *    it — bytes mode, not lfx_encoder_write_codes — and 1 <= in_len <= 65535.
 *  - Stored, when S is eligible and S < min(D, F); otherwise fixed, when F <= D; otherwise dynamic.
 *  - A block chosen dynamic carries exactly the bits it has in the dynamic_huffman = 1 encode of the same call, a block chosen
 *    fixed those of the = 0 encode, each shifted to where it lands.  The output is never longer than either of those encodes:
 *    lfx_encode_bound and its siblings hold as they are.  With a preset dictionary a stored block holds the record's bytes alone.
 * Served by lfx_encode_device / _host, lfx_encode_batch_device, the dictionary encode calls (plain and chain dictionaries),
 * lfx_encoder_* (codes mode: fixed or dynamic only) and lfx_encode_members_* (BGZF: the 64 KiB fallback is evaluated on the
 * chosen sizes), with the lz77 kinds 0, 2 and 3.  LFX_E_UNSUPPORTED from lfx_encode_index_device and from the N-GPU encode
 * (lfx_encode_shard_prepare, lfx_sharded_encode_begin): a stored block's size depends on the bit phase there.  LFX_LZ77_LEVEL
 * (kind 4) is served and refused with LFX_HUFFMAN_AUTO exactly as the kinds 2 and 3 are. */
enum { LFX_HUFFMAN_FIXED = 0, LFX_HUFFMAN_DYNAMIC = 1, LFX_HUFFMAN_AUTO = 2 };
/* lfx_encode_opts::block_merge.  0: off (the default: the blocks are the plan's, as in the reference).  1 — opt-in, not a
 * reference option: neighbouring dynamic blocks are joined wherever one Huffman code for both is no longer
 * than two, so that block_size becomes the SMALLEST block.  Any other value: LFX_E_ARG.  No effect under no_compression or
 * dynamic_huffman = 0 (there is no dynamic block to join).
 *  - The plan, the LZ77 code words and the container header are those of the same call with block_merge = 0.
 *  - Candidates are the plan's dynamic blocks.  A run is a maximal sequence of consecutive candidates of one stream (a stream:
 *    one batch record, one dictionary record, the one buffer of a one-shot call); a stored block of the plan (the zlib sync
 *    marker) ends a run.  The candidates of a run are numbered from 0, n of them.
 *  - The decision is a fixed binary tree over a run, so it is parallel and deterministic.  The node at level l = 1..4 with
 *    index k covers the candidates [k * 2^l, min((k + 1) * 2^l, n)); its children are the two level l - 1 nodes inside it; a
 *    level 0 node is one candidate.  A leaf is whole.  A node whose right child is empty IS its left child.  Any other node is
 *    whole exactly when both children are whole and D(node) <= D(left) + D(right).
 *  - D(X) = the exact bits (3 + dynamic header + symbols) of the dynamic block over the sum of the symbol counts of X's
 *    candidates with ONE EndOfBlock.
 *  - Every maximal whole node becomes one block: at most LFX_MERGE_MAX candidates form one block, and a block never crosses a
 *    LFX_MERGE_MAX-candidate boundary of its run.  A merged block holds its candidates' code words in order without the interior
 *    EndOfBlocks, takes BFINAL and the byte alignment behind it from its last candidate, and covers the input bytes of all.
 *  - With dynamic_huffman = 1 the output is never longer than the block_merge = 0 output of the same call (by induction over the
 *    tree: a whole node is no longer than its children together): lfx_encode_bound and its siblings hold as they are.  With
 *    LFX_HUFFMAN_AUTO the form is chosen per MERGED block, behind the merge, so that output is never longer than the
 *    block_merge = 1, dynamic_huffman = 1 output (per block the smallest of three forms, the dynamic one among them).
 * Served by lfx_encode_device / _host, lfx_encode_batch_device and the dictionary encode calls (plain and chain dictionaries),
 * with every lz77_kind.  LFX_E_UNSUPPORTED from lfx_encoder_* (a merge across a flush would break what a flush promises), from
 * lfx_encode_members_*, from lfx_encode_index_device and from the N-GPU encode. */
#define LFX_MERGE_MAX 16
/* zlib::FlushMode (src/zlib.rs:184-195) */
enum { LFX_FLUSH_NONE = 0, LFX_FLUSH_SYNC = 2 };

/* Options: deflate::EncodeOptions (src/deflate/encode.rs:17-128) + DefaultLz77EncoderBuilder
 * (libflate_lz77/src/default.rs:202-249) + gzip::HeaderBuilder (src/gzip.rs:126-288) +
 * zlib::EncodeOptions.flush_mode (src/zlib.rs:414-518). */
typedef struct lfx_encode_opts {
    uint64_t block_size;       /* encode.rs:11   default 1 MiB (hint; a block holds whole writes) */
    int32_t dynamic_huffman;   /* encode.rs:107  default 1; 0 = fixed_huffman_codes(); LFX_HUFFMAN_AUTO (2) = the smallest form per block */
    int32_t no_compression;    /* encode.rs:77   stored blocks */
    int32_t lz77_kind;         /* LFX_LZ77_*     with_lz77(...) */
    uint32_t window_size;      /* default.rs:226 default 32768 (clamped) */
    uint32_t max_length;       /* default.rs:238 default 258 (clamped; must be >= 3) */
    int32_t zlib_flush_mode;   /* zlib.rs:504    LFX_FLUSH_* */
    uint32_t mtime;            /* gzip.rs:167    (reference default = now; callers set it) */
    uint8_t os;                /* gzip.rs:173    default 3 (Unix) */
    uint8_t is_text;           /* gzip.rs:179 */
    uint8_t hcrc;              /* gzip.rs:185    verify() */
    uint8_t lz77_level;        /* 0: the level of lz77_kind's encoder; 1 + LFX_LEVEL_*: E::compression_level() of a caller-supplied
                                  Lz77Encode (lfx_encoder_write_codes) — it decides zlib's FLEVEL (zlib.rs:59-68,212-220) and gzip's XFL
                                  (gzip.rs:84-92,684) */
    const uint8_t *extra;      /* gzip.rs:191    serialized subfields (id[2] len[2] data)* */
    uint32_t extra_len;
    uint32_t block_merge;      /* 0 (default): the plan's blocks; 1: neighbouring dynamic blocks joined where one code is no longer
                                  (opt-in, above; in what was padding: the size and every other offset are unchanged) */
    const char *filename;      /* gzip.rs:197    NUL-terminated */
    const char *comment;       /* gzip.rs:203 */
} lfx_encode_opts;
void lfx_encode_opts_default(lfx_encode_opts *o);

/* How the caller slices its writes (what decides LZ77 chunk and DEFLATE block boundaries:
 * default.rs:60-68, encode.rs:277-286). */
enum { LFX_SCHED_SINGLE = 0, /* one write_all(buf)            — every in-tree reference test */
       LFX_SCHED_FIXED = 1,  /* writes of `fixed_write` bytes — examples/flate.rs:52 uses 8192 */
       LFX_SCHED_LIST = 2 }; /* explicit sizes; a size of UINT64_MAX means Write::flush() */
#define LFX_SCHED_FLUSH UINT64_MAX
typedef struct lfx_schedule {
    int32_t kind;
    uint64_t fixed_write;
    const uint64_t *writes;
    size_t n_writes;
} lfx_schedule;

/* ---- device context (one per GPU; owns a HIP stream + cached scratch in HBM) ------------- */
typedef struct lfx_ctx lfx_ctx;
lfx_ctx *lfx_ctx_new(int device, int *status);
/* Every handle made from a context (lfx_encoder, lfx_decoder, lfx_lz77, a sharded encode in flight) uses it until that handle is
 * freed — free the handles first.  (The Rust crate's handles hold an Arc<Context>; the Python wrappers count themselves in and out
 * of their Context, because a garbage collector runs the finalizers of one unreachable group in an undefined order.) */
void lfx_ctx_free(lfx_ctx *c);
const char *lfx_ctx_last_error(const lfx_ctx *c);
/* use the caller's HIP stream (hipStream_t as void*) instead of the context's own */
void lfx_ctx_set_stream(lfx_ctx *c, void *hip_stream);
int lfx_device_count(void);

/* ---- one-shot, device-resident buffers (what io::copy over in-memory buffers amounts to) --
 * Replaces {deflate,zlib,gzip}::Encoder::{with_options, write*, finish}
 * (encode.rs:182-249, zlib.rs:577-681, gzip.rs:804-908) for a whole buffer. */
uint64_t lfx_encode_bound(uint64_t n, const lfx_encode_opts *o, const lfx_schedule *s);
int lfx_encode_device(lfx_ctx *c, int format, const lfx_encode_opts *o, const lfx_schedule *s,
                      const void *d_in, uint64_t n, void *d_out, uint64_t cap, uint64_t *out_len);
/* `count` independent streams in one call (BASELINE.json configs[2] needs thousands of 64 KiB streams): stream i is what
 * lfx_encode_device makes of d_in[in_off[i] .. +in_len[i]) with the same options and the schedule applied to it alone, and
 * lies at d_out[out_off[i] .. +out_len[i]) (out_off 4-byte aligned, out_cap[i] >= lfx_encode_bound(in_len[i])).  Offsets and
 * lengths are HOST arrays.  The output ranges [out_off[i], out_off[i] + out_cap[i]) must not overlap (LFX_E_ARG); the whole
 * span from the lowest out_off to the highest out_off + out_cap is zero-filled first — gaps between the ranges included, and
 * also when the call then fails.  A stream that does not fit its capacity voids the call: LFX_E_NOSPACE, status[i] =
 * LFX_E_NOSPACE for exactly the streams that were too small (0 for those that would have fit), every out_len[i] = 0. */
int lfx_encode_batch_device(lfx_ctx *c, int format, const lfx_encode_opts *o, const lfx_schedule *s, uint32_t count,
                            const void *d_in, const uint64_t *in_off, const uint64_t *in_len, void *d_out,
                            const uint64_t *out_off, const uint64_t *out_cap, uint64_t *out_len, int32_t *status);
/* same, host buffers (H2D + device path + D2H; PCIe-inclusive).  Round 6: page-locked buffers — lfx_host_alloc below, or the
 * caller's own hipHostMalloc / hipHostRegister — are handed to the DMA engine as they are; pageable ones are staged through
 * page-locked slabs by four copy threads (one thread's memcpy is slower than the link).  lfx_decode_host likewise. */
void *lfx_host_alloc(size_t bytes);   /* page-locked host memory (NULL: none to be had); for buffers that cross PCIe often */
void lfx_host_free(void *p);
int lfx_encode_host(lfx_ctx *c, int format, const lfx_encode_opts *o, const lfx_schedule *s,
                    const void *in, uint64_t n, void *out, uint64_t cap, uint64_t *out_len);

/* Replaces {deflate,zlib,gzip}::Decoder::{new, read_to_end} (decode.rs:40-164,
 * zlib.rs:312-409, gzip.rs:941-1047) and gzip::MultiDecoder (gzip.rs:1100-1166, flag below).
 * *out_len = bytes produced (also on failure: read_to_end + unread_decoded_data,
 * decode.rs:68-73); *consumed = input bytes consumed including the trailer. */
#define LFX_DEC_MULTI 1u
int lfx_decode_device(lfx_ctx *c, int format, uint32_t flags, const void *d_in, uint64_t n,
                      void *d_out, uint64_t cap, uint64_t *out_len, uint64_t *consumed);
int lfx_decode_host(lfx_ctx *c, int format, uint32_t flags, const void *in, uint64_t n, void *out,
                    uint64_t cap, uint64_t *out_len, uint64_t *consumed);
/* `count` independent streams, one wavefront each (BASELINE.json configs[2]).
 * offsets/lengths are HOST arrays; status[i] gets LFX_* per stream.  lfx_decode_batch_size_device below reports the
 * out_cap[] a batch needs. */
int lfx_decode_batch_device(lfx_ctx *c, int format, uint32_t count, const void *d_in,
                            const uint64_t *in_off, const uint64_t *in_len, void *d_out,
                            const uint64_t *out_off, const uint64_t *out_cap, uint64_t *out_len,
                            int32_t *status);
/* gzip::MultiDecoder (gzip.rs:1052-1167) over a whole buffer, with the members decoded as ONE batch: the members are found
 * on the device (candidate offsets, header parse, a walk of their blocks that produces no output), chained on the host
 * from byte 0, and the chained members go through the batch decoder; whatever that pass does not settle (a damaged
 * member, a start that is no candidate, a member longer than the walk, output that does not fit, the end of the input)
 * is decoded by the sequential member loop of lfx_decode_device from that member on.  Status, *out_len, *consumed,
 * lfx_ctx_last_error and d_out[0 .. *out_len) are exactly those of
 * lfx_decode_device(c, LFX_GZIP, LFX_DEC_MULTI, d_in, n, d_out, cap, ...).
 * members: the members whose trailer was verified, in input order; *n_members = their count (also when that exceeds
 * max_members: only the first max_members entries are written).  members may be NULL.  lfx_decode_members_size_device
 * below reports the cap an input needs. */
typedef struct lfx_member {
    uint64_t in_off, in_len;   /* the member's bytes in the input: header .. 8-byte trailer */
    uint64_t out_off, out_len; /* its output in d_out */
} lfx_member;                  /* 32 bytes */
int lfx_decode_members_device(lfx_ctx *c, const void *d_in, uint64_t n, void *d_out, uint64_t cap,
                              uint64_t *out_len, uint64_t *consumed,
                              lfx_member *members, uint32_t max_members, uint32_t *n_members);
/* same, host buffers (staged like lfx_decode_host) */
int lfx_decode_members_host(lfx_ctx *c, const void *in, uint64_t n, void *out, uint64_t cap,
                            uint64_t *out_len, uint64_t *consumed,
                            lfx_member *members, uint32_t max_members, uint32_t *n_members);

/* ---- decoded size without decoding: `gzip -l` for this library --------------------------------------------
 * Let D = (status, *out_len, *consumed) of the matching decode call with a cap that is large enough: lfx_decode_device /
 * lfx_decode_host for lfx_decode_size_*, stream i of lfx_decode_batch_device for the batch call, lfx_decode_members_* for
 * lfx_decode_members_size_*.  A size call takes no output buffer and produces no bytes:
 *  1. The checksums (CRC-32 / Adler-32) are NOT computed.  Everything else a decode checks is checked: container header and
 *     its CRC where present, block headers and code tables, every symbol, stored LEN / NLEN, "Too long backword reference" (a
 *     distance that reaches in front of the member's first byte), the end of the input inside a block, and the PRESENCE of the
 *     4- or 8-byte trailer (a missing one is LFX_E_UNEXPECTED_EOF as in the decode).
 *  2. Where D's status is anything but a checksum mismatch, the size call returns exactly D, on damaged input too: *out_len
 *     is then the partial output the decode leaves in d_out.  lfx_ctx_last_error is the decode's message.  (One verdict
 *     differs in *consumed: behind "Invalid huffman coded stream" the decode calls count the 16 bits the reference's decoder
 *     skips without reading them, up to two bytes; the size calls report the bytes the reference's reader has pulled.)
 *  3. Where D's status is a checksum mismatch, the size call goes on as if the checksum had matched (LFX_DEC_MULTI: with the
 *     next member).  So always *out_len >= D's, and a decode with cap = *out_len never returns LFX_E_NOSPACE.
 *  4. Batch: status[i], out_len[i], consumed[i] (the bytes of stream i consumed, trailer included) by the same rules; the
 *     return value is LFX_OK as in lfx_decode_batch_device.  Members: members[], *n_members and the truncation at max_members
 *     as lfx_decode_members_device documents them; by rule 3 a member with a bad CRC is listed and the walk goes on behind it.
 *  5. A NULL context: LFX_E_DEVICE, nothing written.  n == 0, count == 0, NULL out_len / consumed / status / members: as the
 *     matching decode call.
 *  6. The calls write no device memory of the caller's, reserve no output-sized scratch, and leave the context usable. */
int lfx_decode_size_device(lfx_ctx *c, int format, uint32_t flags, const void *d_in, uint64_t n,
                           uint64_t *out_len, uint64_t *consumed);
int lfx_decode_size_host(lfx_ctx *c, int format, uint32_t flags, const void *in, uint64_t n,
                         uint64_t *out_len, uint64_t *consumed);
int lfx_decode_batch_size_device(lfx_ctx *c, int format, uint32_t count, const void *d_in,
                                 const uint64_t *in_off, const uint64_t *in_len,
                                 uint64_t *out_len, uint64_t *consumed, int32_t *status);
int lfx_decode_members_size_device(lfx_ctx *c, const void *d_in, uint64_t n, uint64_t *out_len, uint64_t *consumed,
                                   lfx_member *members, uint32_t max_members, uint32_t *n_members);
int lfx_decode_members_size_host(lfx_ctx *c, const void *in, uint64_t n, uint64_t *out_len, uint64_t *consumed,
                                 lfx_member *members, uint32_t max_members, uint32_t *n_members);

/* The other direction: d_in[0, n) as gzip members that lie back to back in d_out[0, *out_len) — what lfx_decode_members_device
 * decodes as one batch, and what zcat, Python's gzip and (with LFX_MEMBERS_BGZF) bgzip / htslib read.  The
 * input is cut into ceil(n / member_size) slices of member_size bytes (the last may be shorter; n == 0: one slice of no bytes);
 * member i is byte for byte what lfx_encode_device(c, LFX_GZIP, o, s, slice i, ...) writes, the schedule applied to each slice
 * alone.  All members are encoded in one launch set and packed at their final offsets: no padding, any byte offset.
 * LFX_MEMBERS_BGZF: 1 <= member_size <= 65505; o must hold no extra, filename or comment and hcrc = 0, s must be
 * LFX_SCHED_SINGLE (LFX_E_ARG, the message names the field; also block_size <= member_size with member_size > 65500, where the
 * stored form below would not fit).  Every member is encoded with extra = 42 43 02 00 lo hi, (lo, hi) = its total length - 1; a
 * member whose total length would exceed 65536 bytes is written as the same call writes it with no_compression = 1 (decided on
 * the device before anything of it is written); behind the last member lie the 28 bytes of BGZF's end-of-file marker.  n == 0:
 * the marker alone, no member.
 * members[i] = {in_off, in_len: slice i in d_in; out_off, out_len: member i in d_out} (the marker is no member); *n_members =
 * their count, also when that exceeds max_members (only the first max_members records are written); members may be NULL.
 * d_out must be 4-byte aligned.  d_out[0, min(cap, lfx_encode_members_bound(...))) is zero-filled first; nothing behind
 * *out_len is written after that, and nothing behind cap at all.  cap below the bound is no error in itself: LFX_E_NOSPACE only
 * when the members do not fit, with *out_len = 0 and no member written.  member_size == 0: LFX_E_ARG.  A NULL context:
 * LFX_E_DEVICE, nothing written.
 * lfx_encode_members_bound: the sum of lfx_encode_bound over the slices; BGZF: every term capped at 65536, plus 28.  0 for
 * arguments the encode call would refuse. */
enum { LFX_MEMBERS_BGZF = 1u };
uint64_t lfx_encode_members_bound(uint64_t n, uint64_t member_size, uint32_t flags, const lfx_encode_opts *o, const lfx_schedule *s);
int lfx_encode_members_device(lfx_ctx *c, const lfx_encode_opts *o, const lfx_schedule *s, uint64_t member_size, uint32_t flags,
                              const void *d_in, uint64_t n, void *d_out, uint64_t cap, uint64_t *out_len,
                              lfx_member *members, uint32_t max_members, uint32_t *n_members);
/* same, host buffers (staged like lfx_encode_host) */
int lfx_encode_members_host(lfx_ctx *c, const lfx_encode_opts *o, const lfx_schedule *s, uint64_t member_size, uint32_t flags,
                            const void *in, uint64_t n, void *out, uint64_t cap, uint64_t *out_len,
                            lfx_member *members, uint32_t max_members, uint32_t *n_members);
/* host only: bgzip's .gzi index from the member table of lfx_encode_members_* (out_off = compressed, in_off = uncompressed):
 * u64 LE count = n_members - 1 (0 for no member), then for members 1 .. count a pair of u64 LE (compressed offset, uncompressed
 * offset); member 0 is implicit.  *len = its size (also when cap is too small: LFX_E_NOSPACE; buf may then be NULL). */
int lfx_members_gzi(const lfx_member *members, uint32_t n_members, void *buf, uint64_t cap, uint64_t *len);

/* ---- BGZF reads by virtual offset: what htslib's bgzf_seek + bgzf_read serve, batched, with no index ------
 * .bai / .tbi / .csi / .gzi address a BGZF file by virtual offset, coffset << 16 | uoffset: the byte at which a block starts
 * in the file, and a byte inside that block's output.  Every block is a gzip member of at most 64 KiB that names its own length
 * (BSIZE), so a read hops from block to block and decodes only the blocks it covers.  `count` reads in one call; reads and res
 * are HOST arrays; d_in holds file bytes [in_base, in_base + n) (as in lfx_index_read_device).
 *  1. Block form.  A block is accepted in htslib's form only: the 18 bytes 1f 8b 08 04, six bytes (mtime, xfl, os), 06 00 42 43
 *     02 00, BSIZE; BSIZE + 1 >= 26 bytes in all, the last four of them ISIZE <= 65536.  Anything else at a position the walk
 *     reaches (a voff that points into the middle of a block) is LFX_E_INVALID_DATA for that read; the message names the coffset.
 *  2. Walk.  A read starts in the block at voff >> 16, at byte voff & 0xffff of its output, and continues through the blocks
 *     that follow.  Empty blocks contribute nothing and are passed (the 28-byte end-of-file marker, also in the middle of
 *     `cat a b`).  It ends, with LFX_OK, at the first of: len bytes; end_voff (compared as coffset, then uoffset: the block at
 *     end_voff's coffset is not even looked at when nothing of it is wanted); the bytes held ending exactly at a block boundary
 *     (a short read).  end_voff <= voff: 0 bytes, LFX_OK, nothing is looked at.
 *  3. Start.  coffset outside [in_base, in_base + n]: LFX_E_ARG.  coffset == in_base + n: 0 bytes, LFX_OK, next_voff = voff.
 *     uoffset == ISIZE is a valid start (the read continues in the next block); uoffset > ISIZE: LFX_E_ARG.  The start block is
 *     checked (rules 1, 4) also when len == 0.
 *  4. Cut-off block.  A block that starts inside the bytes held but does not end inside them (or whose 18 header bytes do not):
 *     LFX_E_UNEXPECTED_EOF, out_len = the bytes in front of it, next_voff = that block's start (in the start block: voff) — the
 *     caller fetches more of the file and goes on from there.
 *  5. Verification.  Every block that contributes a byte is decoded whole: its CRC-32 is verified, its decoded length must be
 *     ISIZE and its DEFLATE stream must end 8 bytes in front of BSIZE + 1.  A block that fails makes every read that touches
 *     it LFX_E_INVALID_DATA with out_len = the bytes in front of that block, n_blocks = the blocks in front of it and next_voff
 *     = the first byte wanted of it; reads that do not touch it are unaffected.
 *  6. next_voff = coffset << 16 | uoffset of the first byte not delivered; where that is the end of a block, the start of the next
 *     block with uoffset 0 (bgzf_tell).
 *  7. Exactly d_out[out_off, out_off + out_len) is written for each read and nothing else.  Output ranges [out_off, out_off +
 *     len) that overlap: LFX_E_ARG for the call, res is not written.
 *  8. The return value is LFX_OK when every read is, otherwise the first failing read's status, lfx_ctx_last_error its message.
 *     res is written all at once, by a call that settled every read.  A call refused as a whole — rule 7, rule 11, bytes held
 *     that end behind coffset 2^48 (LFX_E_ARG), a device error, no memory — leaves every byte of res as the caller set it,
 *     which is how a caller tells such a refusal from a read's own LFX_E_ARG.
 *  9. A block covered by several reads is decoded once; *blocks_decoded (may be NULL) = the distinct blocks decoded.
 * 10. Size mode: d_out == NULL (out == NULL) walks and decodes nothing — out_len, next_voff, n_blocks and status come from the
 *     headers and ISIZEs alone; rule 5 is the only rule skipped, len still bounds out_len; *blocks_decoded = 0.
 * 11. A NULL context: LFX_E_DEVICE, nothing written.  count == 0: LFX_OK.  NULL reads or res with count > 0: LFX_E_ARG.
 * lfx_bgzf_read_host does not upload the file: the walk runs on the CPU over `in`, only the distinct covered blocks cross the
 * link; its results equal the device call's field for field. */
typedef struct lfx_bgzf_read {
    uint64_t voff;      /* first byte of the read: coffset << 16 | uoffset (coffset relative to byte 0 of the file) */
    uint64_t end_voff;  /* the read stops in front of this position; UINT64_MAX: no such bound */
    uint64_t len;       /* bytes delivered at most = the size of its output range */
    uint64_t out_off;   /* the bytes go to d_out + out_off */
} lfx_bgzf_read;        /* 32 bytes */
typedef struct lfx_bgzf_result {
    uint64_t out_len;   /* bytes delivered (size mode: bytes a read would deliver) */
    uint64_t next_voff; /* position behind the last byte delivered (bgzf_tell) */
    int32_t  status;    /* LFX_* of this read */
    uint32_t n_blocks;  /* blocks that contributed at least one byte */
} lfx_bgzf_result;      /* 24 bytes */
int lfx_bgzf_read_device(lfx_ctx *c, const void *d_in, uint64_t in_base, uint64_t n, uint32_t count,
                         const lfx_bgzf_read *reads, void *d_out, lfx_bgzf_result *res, uint64_t *blocks_decoded);
int lfx_bgzf_read_host(lfx_ctx *c, const void *in, uint64_t in_base, uint64_t n, uint32_t count,
                       const lfx_bgzf_read *reads, void *out, lfx_bgzf_result *res, uint64_t *blocks_decoded);
/* host only: uncompressed offset -> virtual offset through a member table (lfx_encode_members_*: out_off = compressed,
 * in_off = uncompressed; `swapped` != 0 for the table of lfx_decode_members_* / _size_*, where the roles are exchanged).  A
 * binary search over a table in file order: uoff at a member boundary is the later member with uoffset 0, uoff equal to the
 * total the position behind the last member (an empty table: 0), uoff behind that LFX_E_ARG — as is a position more than 65535
 * bytes into its member, which no virtual offset names. */
int lfx_members_voffset(const lfx_member *members, uint32_t n_members, int swapped, uint64_t uoff, uint64_t *voff);

/* ---- seek index: random-access reads of a DEFLATE / zlib / gzip stream ---------------------------------
 * One decode builds the index: a list of access points (a bit of the input where decoding can start, the output byte it
 * produces first, the 32 KiB of output in front of it).  A read of output bytes [off, off + len) decodes only from the access
 * point in front of off.  An index belongs to the context it was made on (like lfx_encoder / lfx_decoder); its windows live
 * in that context's device memory.
 * Candidates for access points: every block start, and the proved lane starts of the decode's block scan inside dynamic
 * and fixed blocks that produce more than `spacing` bytes — of those, the first in each spacing / 16 bytes of output (stored
 * blocks: block starts only).  Every member starts with a
 * point at its first block header (win_len 0); inside a member the next point is the last candidate whose out_off is at
 * most the previous point's out_off + spacing, or the first candidate after that when there is none.  max_gap = the
 * largest distance from a point to the next point or to its member's end.  A member decoded by the serial kernel (streams
 * under 4 KiB, anomalies) keeps only its start point.
 * Integrity: the checksums (CRC-32 / Adler-32) are verified when the index is built, NOT when it is read.  A read checks
 * each point's in_crc against the input bytes it holds, and a segment decoded up to the next point must end exactly at
 * that point's in_bit and out_off (a member's last segment: at its BFINAL block's EndOfBlock); anything else is
 * LFX_E_INVALID_DATA for that read, and the message names the point.
 * Serialised form (little-endian): a 64-byte header — "LFXINDEX", u32 version = 1, u32 format, u32 flags, u32 n_points,
 * u64 in_len (the decode's consumed), u64 out_len, u64 spacing, u64 max_gap, u32 n_members, u32 0 — then n_points
 * 40-byte lfx_index_point records, then the windows concatenated in point order (win_len bytes each), then a u32 CRC-32
 * of every byte in front of it.  Export is deterministic. */
typedef struct lfx_index lfx_index;
typedef struct lfx_index_point {
    uint64_t in_bit;   /* first bit decoded from this point, relative to input byte 0: a block header, or a symbol boundary
                          inside the block whose header is at hdr_bit */
    uint64_t hdr_bit;  /* header bit of the block holding in_bit (== in_bit at a block start) */
    uint64_t out_off;  /* output byte that in_bit produces first, relative to the decode's whole output */
    uint32_t member;   /* gzip member index (0 without LFX_DEC_MULTI) */
    uint32_t win_len;  /* history kept: min(32768, out_off - out_off of the member's first point) */
    uint32_t in_crc;   /* CRC-32 of input bytes [in_bit/8, in_bit/8 + 64), clipped to the input */
    uint8_t btype;     /* of the block at hdr_bit; 0 (stored) only at a block start */
    uint8_t _pad[3];
} lfx_index_point;     /* 40 bytes */
typedef struct lfx_index_info {
    uint64_t in_len, out_len, spacing, max_gap, export_bytes;
    uint32_t format, flags, n_points, n_members;
} lfx_index_info;      /* 56 bytes */
/* lfx_decode_device plus an index.  Status, *out_len, *consumed, lfx_ctx_last_error and d_out[0 .. *out_len) are EXACTLY
 * those of lfx_decode_device(c, format, flags, ...) (LFX_DEC_MULTI: of lfx_decode_members_device).  On LFX_OK, *idx is a new
 * index; on any other status, *idx = NULL.  spacing < 4096 -> LFX_E_ARG. */
int lfx_decode_index_device(lfx_ctx *c, int format, uint32_t flags, const void *d_in, uint64_t n, void *d_out,
                            uint64_t cap, uint64_t *out_len, uint64_t *consumed, uint64_t spacing, lfx_index **idx);
/* lfx_encode_device plus a seek index of the stream it writes.  Status, *out_len, lfx_ctx_last_error and
 * d_out[0 .. *out_len) are EXACTLY those of lfx_encode_device(c, format, o, s, d_in, n, d_out, cap, out_len).  On LFX_OK, *idx is
 * a new index (format = format, flags = 0, n_members = 1, in_len = *out_len, out_len = n); on any other status *idx = NULL.
 * Candidates: every block start, and inside dynamic and fixed blocks that produce more than `spacing` bytes the first code
 * boundary in each spacing / 16 bytes of output; the selection is lfx_decode_index_device's.  Where no compressed block
 * produces more than `spacing` bytes, the index equals the one lfx_decode_index_device builds from the encoded stream.
 * spacing < 4096 -> LFX_E_ARG.  A NULL context -> LFX_E_DEVICE, nothing written. */
int lfx_encode_index_device(lfx_ctx *c, int format, const lfx_encode_opts *o, const lfx_schedule *s,
                            const void *d_in, uint64_t n, void *d_out, uint64_t cap, uint64_t *out_len,
                            uint64_t spacing, lfx_index **idx);
/* `count` reads (off, len, out_off, out_len_r, status: HOST arrays).  d_in holds input bytes [in_base, in_base + n).
 * Read i writes output bytes [off[i], off[i] + len[i]) clipped to out_len at d_out + out_off[i], and writes nothing else.
 * out_len_r[i] = bytes written, status[i] = LFX_* per read: LFX_E_ARG if off[i] > out_len or the input the read needs
 * (lfx_index_span) is not inside [in_base, in_base + n); a read with len 0, or one that starts at out_len, is LFX_OK and
 * writes nothing.  The return value is LFX_OK when every read is OK, otherwise the first failing read's status. */
int lfx_index_read_device(lfx_ctx *c, const lfx_index *idx, const void *d_in, uint64_t in_base, uint64_t n,
                          uint32_t count, const uint64_t *off, const uint64_t *len, void *d_out,
                          const uint64_t *out_off, uint64_t *out_len_r, int32_t *status);
/* host only: the input bytes [*in_lo, *in_hi) that a read of [off, off + len) needs held in d_in — from the header of the block
 * that holds the first access point it decodes from (that header is parsed again) */
int lfx_index_span(const lfx_index *idx, uint64_t off, uint64_t len, uint64_t *in_lo, uint64_t *in_hi);
int lfx_index_get_info(const lfx_index *idx, lfx_index_info *info);
int lfx_index_get_point(const lfx_index *idx, uint32_t i, lfx_index_point *p);
/* the serialised index into buf[0, cap); *len = its size (also when cap is too small: LFX_E_NOSPACE; buf may be NULL) */
int lfx_index_export(lfx_ctx *c, const lfx_index *idx, void *buf, uint64_t cap, uint64_t *len);
/* a serialised index (lfx_index_check first) → a new index on c; NULL with *status on failure */
lfx_index *lfx_index_import(lfx_ctx *c, const void *buf, uint64_t len, int *status);
/* host only: validates a serialised index (LFX_E_INVALID_DATA when it breaks the format); info may be NULL */
int lfx_index_check(const void *buf, uint64_t len, lfx_index_info *info);
void lfx_index_free(lfx_index *idx);

/* ---- sharded encode: independent block ranges per rank, one gzip/zlib/deflate member
 * (SURVEY §8e).  prepare() runs match finding → Huffman build and the checksums and reports the
 * shard's bit length; after the ranks exchanged lfx_shard_info (RCCL all-gather), emit() packs the
 * shard at its global bit offset.  The byte at each shard boundary is shared (OR the halves).
 * no_compression: LFX_E_UNSUPPORTED (a stored block's size depends on the bit phase). */
typedef struct lfx_shard_info {
    uint64_t total_bits; /* DEFLATE bits of this shard (incl. final byte alignment on the last) */
    uint64_t n_bytes;    /* uncompressed bytes */
    uint32_t crc32;      /* of the shard's input */
    uint32_t adler32;    /* of the shard's input, as if it started a stream (A0 = 1) */
} lfx_shard_info;
int lfx_encode_shard_prepare(lfx_ctx *c, int format, const lfx_encode_opts *o,
                             const lfx_schedule *s, const void *d_in, uint64_t n, int is_first,
                             int is_last, lfx_shard_info *info);
/* start_bit = bit offset of this shard's first DEFLATE bit inside the member (container header
 * included).  Writes bytes [start_bit/8, ceil((start_bit+total_bits)/8)) of the member to d_out
 * (d_out[0] is byte start_bit/8); the first shard also writes the container header, the last
 * shard the trailer built from the combined checksum / size given here. */
int lfx_encode_shard_emit(lfx_ctx *c, uint64_t start_bit, uint32_t combined_check,
                          uint64_t total_n, void *d_out, uint64_t cap, uint64_t *out_len);
/* Optional, in front of lfx_encode_shard_prepare: names the buffer lfx_encode_shard_emit will write, which is then zero-filled on
 * the context's side stream beside the prepare call's kernels instead of in front of the pack kernels (what lfx_encode_device
 * does with its own output).  (NULL, 0) waits for a fill in flight and forgets it (no emit call will follow). */
int lfx_encode_shard_prezero(lfx_ctx *c, void *d_out, uint64_t cap);
/* inverse of the sharded encode: decodes the blocks of ONE shard of a member.  d_in[0] is the byte
 * that holds bit `start_bit` (0..7) of the shard; a non-last shard ends when a block ends exactly
 * `total_bits` later (it holds no BFINAL block).  Reference-made blocks never reference earlier
 * blocks (fresh PrefixTable per flush, default.rs:73), which is what makes shards decodable alone. */
int lfx_decode_shard_device(lfx_ctx *c, const void *d_in, uint64_t n, uint64_t start_bit,
                            uint64_t total_bits, int is_last, void *d_out, uint64_t cap,
                            uint64_t *out_len);
/* ---- N-GPU decode of ONE member WITHOUT the encoder's layout (north_star: "independent DEFLATE blocks
 * partition across the GPUs").  The member is cut by compressed bytes; rank r holds the bytes [lo_byte, lo_byte + n_part)
 * of it in d_part — its own range [lo_byte, hi_byte) plus a tail of a few MiB from its right neighbour, so that a block
 * that starts inside the range can be scanned to its end.
 *   1. lfx_decode_range_scan: block finder + speculative scan of every candidate that STARTS inside the range →
 *      one tuple per candidate (bit offsets relative to the member).  first_bit: the known start of the member's first
 *      block, on the rank whose range holds it (right behind the container header), ~0 elsewhere.  final_from_bit:
 *      headers with BFINAL set are reported only from this bit of the member on (0: everywhere) — a member's last block
 *      is the only one that carries the flag, so looking for it near the end halves the finder's and the scan's work;
 *      when the chain of step 3 then breaks at the last block, scan again with 0;
 *   2. the ranks all-gather their tuples (the only collective: 56 bytes per candidate, a few hundred per rank);
 *   3. lfx_decode_chain (host only, deterministic): the true block list from the known first block; candidates that
 *      are not block starts are never reached.  LFX_E_UNSUPPORTED when the chain breaks (a stored / fixed block the
 *      finder cannot see, damage): decode on one GPU then;
 *   4. lfx_decode_range_emit: materialises the chain blocks owned by `rank` (those that start in its range) into
 *      d_out — the rank's slice of the output, which starts *out_base bytes into the member's output.  Must follow the
 *      same rank's range_scan on the same context (the scan's tables live in its scratch).  *state = 0: the slice holds
 *      its bytes.  Reference-made blocks never read earlier blocks (default.rs:73), so their slices always do.
 *      *state = 1: the slice's blocks read output in front of them (another encoder's member — the reference decodes any
 *      valid stream, src/deflate/decode.rs:112-164, libflate_lz77/src/lib.rs:164-194), possibly bytes another rank
 *      produces: the slice is held as 16-bit symbols and waits for the 32 KiB window in front of it;
 *   5. window hand-over, only when some rank reported state 1: every rank writes its slice's action on the 32 KiB in
 *      front of it as ONE index map (lfx_decode_range_map: 32768 uint16 on the device — a byte value, or 256 + j = "byte
 *      j of the window in front of my slice"), the ranks all-gather the maps (64 KiB each, rank order);
 *   6. lfx_decode_range_finish: composes the window in front of the slice from the maps of the ranks before it (d_maps:
 *      world x 32768 uint16 on the device, 16-byte aligned; NULL when no rank needed a window), replaces the slice's markers, and returns
 *      the slice's CRC-32 / Adler-32 (fold them with lfx_crc32_combine / lfx_adler32_combine and compare with the
 *      trailer). */
typedef struct lfx_blk_tuple {
    uint64_t start_bit, end_bit;  /* header bit, bit behind EndOfBlock (relative to the member's first byte) */
    uint64_t n_out;               /* bytes the block produces */
    uint64_t data_bit;            /* first symbol bit */
    uint32_t n_codes, nlanes;
    uint8_t btype, bfinal, status /* 0 = scanned to its EndOfBlock */, _pad;
    uint16_t rank;                /* owner: the rank whose range holds start_bit */
    uint16_t _pad2;
    uint32_t slot;                /* the owner's scan slot */
    uint32_t _pad3;
} lfx_blk_tuple;                  /* 56 bytes */
int lfx_decode_range_scan(lfx_ctx *c, const void *d_part, uint64_t n_part, uint64_t lo_byte, uint64_t hi_byte,
                          uint64_t first_bit, uint64_t final_from_bit, uint32_t rank, lfx_blk_tuple *tuples, uint32_t cap,
                          uint32_t *count);
int lfx_decode_chain(const lfx_blk_tuple *all, uint32_t n_all, uint64_t first_bit, uint32_t *chain, uint32_t cap,
                     uint32_t *n_chain, uint64_t *total_out);
int lfx_decode_range_emit(lfx_ctx *c, const void *d_part, uint64_t n_part, uint64_t lo_byte, const lfx_blk_tuple *all,
                          const uint32_t *chain, uint32_t n_chain, uint32_t rank, void *d_out, uint64_t cap,
                          uint64_t *out_len, uint64_t *out_base, uint32_t *state);
int lfx_decode_range_map(lfx_ctx *c, void *d_map);
int lfx_decode_range_finish(lfx_ctx *c, const void *d_maps, uint32_t rank, uint32_t *crc32, uint32_t *adler32);
/* stream concatenation on the writer rank: places one shard's bytes (as written by emit(), already
 * on this device — e.g. received over RCCL / xGMI) at byte start_bit/8 of the member buffer; when the shard starts
 * inside a byte (start_bit % 8 != 0) that byte is shared with the shard in front and is OR-ed.  Place the shards in
 * rank order. */
int lfx_shard_place_device(lfx_ctx *c, void *d_member, uint64_t cap, const void *d_part, uint64_t part_len,
                           uint64_t start_bit, int is_first);
/* ---- the N-GPU drivers (round 5): the sequencing of the steps above, with the caller's collectives -----------------------
 * One rank per GPU, one lfx_ctx per rank.  The reference has ONE encoder with ONE running checksum (gzip::Encoder::finish,
 * src/gzip.rs:858-868; src/checksum.rs:22-33); here the ranks' block ranges, bit offsets and partial checksums are exchanged
 * through an lfx_comm — five callbacks the caller implements over whatever moves bytes between its ranks (torch.distributed
 * in libflate_amd/sharded.py, MPI, ...), or lfx_comm_rccl() for RCCL over xGMI.  Every callback returns 0 on success.
 *   allgather: every rank contributes `bytes` HOST bytes; recv (world * bytes, rank order) is complete on return.
 *   isend / irecv: post a transfer of a DEVICE buffer (a binding may only collect them: RCCL groups them, torch batches them);
 *   start (round 6; may be NULL when isend / irecv start their transfers themselves): everything posted so far begins to
 *     move NOW and the call returns without waiting for it — lfx_sharded_encode_begin calls it last, so the shards travel
 *     while the caller works between begin and finish;
 *   wait: everything this rank posted is complete (transfers that were never started are started first).
 * A failure on one rank travels with the next collective and comes back from the same call on EVERY rank. */
typedef struct lfx_comm {
    void *user;
    uint32_t rank, world;
    int (*allgather)(void *user, const void *send, void *recv, uint64_t bytes);
    int (*isend)(void *user, const void *d_buf, uint64_t bytes, uint32_t to_rank);
    int (*irecv)(void *user, void *d_buf, uint64_t bytes, uint32_t from_rank);
    int (*wait)(void *user);
    int (*start)(void *user);
} lfx_comm;
/* RCCL binding: `nccl_comm` is an ncclComm_t, `hip_stream` the hipStream_t its collectives run on.  librccl is loaded at run
 * time (LFX_E_UNSUPPORTED when it is not there): liblfx.so does not link it.  isend / irecv open ONE ncclGroup, start closes
 * it (all transfers of the group begin together, one per xGMI link), wait synchronises the stream; an all-gather that finds a
 * group open closes it first (a collective issued inside an open group would only be queued, and its result read too early).
 * RCCL serialises the operations of one communicator: a caller that wants its small all-gathers (lfx_sharded_decode) not to
 * queue behind shards in flight gives the two drivers two communicators. */
int lfx_comm_rccl(void *nccl_comm, void *hip_stream, uint32_t rank, uint32_t world, lfx_comm *out);
void lfx_comm_rccl_free(lfx_comm *cm);

/* Sharded encode of ONE member: rank r holds the r-th slice of the input (whole blocks: n a multiple of the block size on
 * every rank but the last).  begin(): prepare → all-gather of the 32-byte shard infos → emit at the rank's bit offset →
 * the shards start travelling to rank 0 (all transfers posted at once; d_staging on rank 0 holds the shards of ranks 1.. side
 * by side, 256-byte aligned).  Between begin and finish the caller may use its own shard (d_part).  finish(): waits, places the
 * shards in d_member (rank 0; the byte two shards share is OR-ed) and frees the state.  → the member equals what ONE
 * encoder emits for the concatenated input. */
typedef struct lfx_sharded_enc lfx_sharded_enc;
typedef struct lfx_sharded_part {
    uint64_t start_bit;   /* of this rank's first DEFLATE bit inside the member */
    uint64_t end_bit;     /* the bit behind this rank's last one = the next rank's start_bit */
    uint64_t part_len;    /* bytes emitted into d_part (d_part[0] is byte start_bit / 8 of the member) */
    uint64_t member_len;  /* bytes of the whole member */
    uint64_t total_n;     /* uncompressed bytes of the whole member */
    uint32_t check;       /* combined CRC-32 (gzip) / Adler-32 (zlib) of the whole input */
    uint32_t _pad;
} lfx_sharded_part;
int lfx_sharded_encode_begin(lfx_ctx *c, const lfx_comm *cm, int format, const lfx_encode_opts *o, const lfx_schedule *s,
                             const void *d_in, uint64_t n, void *d_part, uint64_t part_cap, void *d_member /* rank 0 */,
                             uint64_t member_cap, void *d_staging /* rank 0 */, uint64_t staging_cap, lfx_sharded_enc **state,
                             lfx_sharded_part *out);
int lfx_sharded_encode_finish(lfx_ctx *c, const lfx_comm *cm, lfx_sharded_enc *state, uint64_t *member_len /* rank 0 */);

/* N-GPU decode of ONE member cut by compressed bytes (steps 1-6 above): rank r holds d_part = member bytes [lo_byte, hold_hi)
 * (lfx_sharded_byte_range: an equal share plus a tail of one maximal block) and gets its slice of the output in d_out.
 * first_bit: the member's first DEFLATE bit (behind the container header); member_len: 0 if unknown.  Collectives: the
 * candidate tuples, the slices' (status, length, checksums), and — only for members whose blocks read earlier blocks — the
 * ranks' 64 KiB index maps. */
typedef struct lfx_sharded_slice {
    uint64_t out_len, out_base;   /* this rank's slice: bytes, and where it lies in the member's output */
    uint64_t total_out;           /* bytes of the whole member's output */
    uint32_t crc32, adler32;      /* of the whole member's output (compare with the trailer) */
} lfx_sharded_slice;
void lfx_sharded_byte_range(uint64_t first_byte, uint64_t member_len, uint32_t rank, uint32_t world, uint64_t *lo_byte,
                            uint64_t *hi_byte, uint64_t *hold_hi);
int lfx_sharded_decode(lfx_ctx *c, const lfx_comm *cm, const void *d_part, uint64_t n_part, uint64_t lo_byte, uint64_t hi_byte,
                       uint64_t first_bit, uint64_t member_len, void *d_out, uint64_t cap, lfx_sharded_slice *out);
/* the exchange steps of the two drivers on their own (host memory + the comm; no device): the layout of the ranks' bit ranges
 * and the combined trailer checksum; the all-gather of candidate tuples (*all: lfx_sharded_free); the fold of the slices'
 * checksums.  `status`: this rank's error so far — a non-zero status of ANY rank is returned on EVERY rank. */
int lfx_sharded_layout(const lfx_comm *cm, const lfx_shard_info *mine, uint64_t header_len, int format,
                       uint64_t *start_bits /* world + 1 entries */, uint32_t *check, uint64_t *total_n);
int lfx_sharded_gather_tuples(const lfx_comm *cm, const lfx_blk_tuple *mine, uint32_t count, int status, lfx_blk_tuple **all,
                              uint32_t *n_all, uint32_t *failed_rank);
int lfx_sharded_fold(const lfx_comm *cm, int status, uint32_t state, uint64_t len, uint32_t crc32, uint32_t adler32,
                     uint32_t *any_state, uint32_t *crc_all, uint32_t *adler_all, uint64_t *total, uint32_t *failed_rank);
void lfx_sharded_free(void *p);
uint32_t lfx_crc32_combine(uint32_t crc1, uint32_t crc2, uint64_t len2);
uint32_t lfx_adler32_combine(uint32_t ad1, uint32_t ad2, uint64_t len2);
uint64_t lfx_container_header_len(int format, const lfx_encode_opts *o);

/* ---- stream API: io::Write / io::Read shaped (host buffers, callbacks) --------------------
 * write_cb must consume all n bytes and return n, or a negative errno. */
typedef int64_t (*lfx_write_cb)(void *user, const uint8_t *p, size_t n);
typedef int (*lfx_flush_cb)(void *user);
/* read_cb fills up to cap bytes, returns bytes read (0 = EOF) or a negative errno */
typedef int64_t (*lfx_read_cb)(void *user, uint8_t *p, size_t cap);

typedef struct lfx_encoder lfx_encoder;
/* {deflate,zlib,gzip}::Encoder::with_options — gzip/zlib write their header immediately and
 * can fail (gzip.rs:804-812, zlib.rs:577-585). */
lfx_encoder *lfx_encoder_new(lfx_ctx *c, int format, const lfx_encode_opts *o, lfx_write_cb w,
                             lfx_flush_cb f, void *user, int *status);
/* io::Write::write — always consumes everything (encode.rs:241-244); one call = one write() */
int64_t lfx_encoder_write(lfx_encoder *e, const uint8_t *p, size_t n);
/* EncodeOptions::with_lz77(E) for a caller-supplied `E: Lz77Encode` (src/deflate/encode.rs:59-65; call sites
 * CompressBuf::{append, flush}, encode.rs:405-425: the reference Huffman-codes whatever E emits).  E runs on the caller's
 * side; this call hands over what it produced and the GPU does the rest (histogram, Huffman build, bit packing,
 * container checksum) exactly as for the built-in encoders:
 *   write(buf):  E::encode(buf, sink)  → lfx_encoder_write_codes(e, sink's codes, n, buf, len, 0)      (CompressBuf::append)
 *                then, while the bytes since the last close reach block_size (Block::write, encode.rs:282):
 *                E::flush(sink)        → lfx_encoder_write_codes(e, codes, n, NULL, 0, 1)              (CompressBuf::flush)
 *   flush():     E::flush(sink)        → lfx_encoder_write_codes(e, codes, n, NULL, 0, 1); lfx_encoder_flush(e)
 *   finish():    E::flush(sink)        → lfx_encoder_write_codes(e, codes, n, NULL, 0, 2); lfx_encoder_finish(e)
 * codes: (val << 16) | dist as in lfx_sink_cb below; end_block: 0 = the block stays open, 1 = EndOfBlock follows the
 * codes and the block closes, 2 = the same for the stream's final block.  raw: the bytes the codes stand for — only the
 * container checksum (and gzip's ISIZE) looks at them.  An encoder takes bytes (lfx_encoder_write) or codes, never
 * both; code words outside Code's domain (lib.rs:27-42) are LFX_E_ARG. */
int lfx_encoder_write_codes(lfx_encoder *e, const uint32_t *codes, size_t n_codes, const uint8_t *raw, size_t n_raw,
                            int end_block);
/* io::Write::flush — closes the current block (encode.rs:245-248); zlib Sync adds 00 00 FF FF */
int lfx_encoder_flush(lfx_encoder *e);
/* Encoder::finish (encode.rs:203-208, gzip.rs:858-868, zlib.rs:630-639). Everything already
 * handed to write_cb stays with the sink even on error (finish.rs:46-68). */
int lfx_encoder_finish(lfx_encoder *e);
const char *lfx_encoder_last_error(const lfx_encoder *e);
void lfx_encoder_free(lfx_encoder *e);

typedef struct lfx_decoder lfx_decoder;
/* {deflate,zlib,gzip}::Decoder::new / gzip::MultiDecoder::new (flag LFX_DEC_MULTI).  gzip / zlib read the container
 * header — and nothing that is not needed for it beyond the chunk the reader hands over — and can fail
 * (gzip.rs:941-944, zlib.rs:312-320); the body is decoded by the first read().
 * LFX_DEC_NONBLOCKING = src/non_blocking/{deflate,zlib,gzip}::Decoder: the read callback may return
 * -LFX_E_WOULD_BLOCK at any point; read() / header() then return LFX_E_WOULD_BLOCK and can be called again
 * (the header is read lazily, non_blocking/gzip.rs:64-113).
 *
 * The body is decoded a WINDOW at a time, as the reference decodes a block at a time (src/deflate/decode.rs:136-164,
 * 32 KiB of history: libflate_lz77/src/lib.rs:219-231): up to 16 MiB of input are pulled, the blocks that are complete
 * in them (and fit 96 MiB of output) are decoded and served, their input is dropped, the last 32 KiB of output stay as
 * history — what the decoder buffers (lfx_decoder_buffered) is bounded by one window of input plus one of output,
 * whatever the member's size, and the first byte is served as soon as the first window is decoded.  Only a block
 * larger than a window (members written by ONE huge write) makes the window grow.  A window is attempted when it is
 * full, the reader ends, hands over a short read, or would block.  Bytes pulled beyond the member's trailer are not
 * decoded: lfx_decoder_surplus() hands them back (what into_inner() means for a reader that cannot be rewound,
 * gzip.rs:987,1216-1226); a MultiDecoder continues with them. */
#define LFX_DEC_NONBLOCKING 2u
lfx_decoder *lfx_decoder_new(lfx_ctx *c, int format, uint32_t flags, lfx_read_cb r, void *user,
                             int *status);
/* io::Read::read: >0 bytes, 0 = end of stream, <0 = -(LFX_E_*) (reported once, after the bytes decoded in front of
 * the error).  A zero-capacity read returns 0 without latching end-of-stream (gzip.rs:1025-1027, zlib.rs:383-385). */
int64_t lfx_decoder_read(lfx_decoder *d, uint8_t *out, size_t cap);
/* Decoder::unread_decoded_data (decode.rs:68-73) */
int lfx_decoder_unread(lfx_decoder *d, const uint8_t **p, size_t *n);
/* bytes of the inner reader that belong to the members decoded so far (Decoder::into_inner position;
 * gzip.rs:1216-1226) */
uint64_t lfx_decoder_consumed(const lfx_decoder *d);
/* bytes the decoder holds right now: pulled input not yet decoded + decoded output not yet read + 32 KiB of history */
uint64_t lfx_decoder_buffered(const lfx_decoder *d);
/* bytes pulled from the reader behind the last finished member (valid until the next read()) */
int lfx_decoder_surplus(lfx_decoder *d, const uint8_t **p, size_t *n);
/* gzip::Header (gzip.rs:292-341: modification_time, compression_level (XFL), os, is_text, is_verified, extra_field,
 * filename, comment) / zlib::Header (zlib.rs:197-220: window_size, compression_level) of the current member.
 * Pointers stay valid until the next member starts or the decoder is freed. */
typedef struct lfx_header {
    int32_t format;
    uint32_t mtime;
    uint8_t xfl, os, is_text, is_verified, has_extra;
    uint8_t _pad[3];
    const uint8_t *extra;     /* serialized subfields (id[2] len[2] data)*; NULL when absent */
    uint32_t extra_len;
    const char *filename;     /* NUL-terminated; NULL when absent */
    const char *comment;
    uint32_t zlib_window_size; /* 256 << CINFO */
    uint32_t zlib_level;       /* FLEVEL 0..3 */
} lfx_header;
int lfx_decoder_header(lfx_decoder *d, lfx_header *h);
const char *lfx_decoder_last_error(const lfx_decoder *d);
void lfx_decoder_free(lfx_decoder *d);

/* ---- preset dictionaries: zlib streams with FDICT, raw DEFLATE that starts with history ------------------
 * What zlib's inflateSetDictionary / Python's zlib.decompressobj(zdict=...) read.  The reference refuses FDICT, and the
 * dictionary-less calls above keep doing so; these calls are ours.  Decoding only.
 *
 *  1. Dictionary.  The usable history is the LAST min(len, 32768) bytes; lfx_dict_id is the Adler-32 of ALL len bytes (RFC
 *     1950's DICTID).  len == 0 is allowed (id 1, no history).  lfx_dict_new copies what it needs to the device once and
 *     computes the id there; later calls do no per-call dictionary work.  bytes[0, len): host memory, or device memory when
 *     on_device != 0.  A dictionary belongs to its context: use it with that context's calls and decoders only (another
 *     context's: LFX_E_ARG), free it before the context.  A NULL context gives NULL with *status = LFX_E_DEVICE.
 *  2. Formats: LFX_ZLIB and LFX_DEFLATE.  LFX_GZIP is LFX_E_ARG (gzip has no preset dictionary), whatever `dict` is.  There
 *     is no `flags` argument.
 *  3. dict == NULL: every call behaves exactly as its dictionary-less twin (lfx_decode_device, lfx_decode_host,
 *     lfx_decode_batch_device with flags 0) — today's FDICT rejection and its message included.
 *  4. zlib, FDICT set: the header is six bytes; CMF / FLG are checked as ever, DICTID is big-endian.  DICTID != lfx_dict_id(dict)
 *     is LFX_E_INVALID_DATA with *out_len = 0, *consumed what the FDICT rejection reports for the same bytes, and the message
 *     "Dictionary mismatch: dictionary_id=0x%X, supplied=0x%X".  Fewer than six bytes: LFX_E_UNEXPECTED_EOF.  On a match the
 *     body is decoded with the dictionary as history; the Adler-32 trailer covers the output only, never the dictionary.
 *  5. zlib, FDICT clear: the dictionary is not used (as in zlib's inflate): status, lengths, message and bytes are
 *     lfx_decode_device's.
 *  6. Raw DEFLATE: the dictionary is always the history in front of byte 0.  A distance may reach min(len, 32768) + bytes
 *     produced so far; a longer one is "Too long backword reference: buffer.len=%d, distance=%d" with buffer.len =
 *     min(len, 32768) + bytes produced.
 *  7. Everything else — error kinds, partial output on damaged input, LFX_E_NOSPACE, trailing bytes, per-stream status in the
 *     batch with no effect on neighbours — is what the dictionary-less call does.  Nothing outside d_out[out_off, out_off +
 *     out_cap) is written for a stream, and for a stream that decodes, is cut short or does not fit, exactly d_out[out_off,
 *     out_off + out_len).  As in lfx_decode_batch_device, a DAMAGED stream of a batch may leave bytes of a discarded
 *     block-parallel attempt behind out_len, inside its own out_cap; status, out_len and d_out[out_off, out_off + out_len)
 *     are the exact decode's.
 *  8. Stream decoder: lfx_decoder_set_dict makes a zlib / deflate lfx_decoder follow rules 4-6, non-blocking mode included;
 *     on a gzip decoder it is LFX_E_ARG.  It must come before the container header is read: before the first header() /
 *     read() of a non-blocking decoder or of one made with LFX_DEC_LAZY_HEADER (a blocking decoder that, like a non-blocking
 *     one, leaves the header to the first header() / read() instead of reading it in lfx_decoder_new), any time before the
 *     first read() of a raw DEFLATE decoder; later, or a second time: LFX_E_ARG.  The dictionary must outlive the decoder. */
typedef struct lfx_dict lfx_dict;
lfx_dict *lfx_dict_new(lfx_ctx *c, const void *bytes, uint64_t len, int on_device, int *status);
uint32_t lfx_dict_id(const lfx_dict *d);
void lfx_dict_free(lfx_dict *d);
int lfx_decode_dict_device(lfx_ctx *c, int format, const lfx_dict *dict, const void *d_in, uint64_t n,
                           void *d_out, uint64_t cap, uint64_t *out_len, uint64_t *consumed);
/* same, host buffers (staged like lfx_decode_host) */
int lfx_decode_dict_host(lfx_ctx *c, int format, const lfx_dict *dict, const void *in, uint64_t n,
                         void *out, uint64_t cap, uint64_t *out_len, uint64_t *consumed);
/* lfx_decode_batch_device with one dictionary for every stream of the batch (it is never copied in front of an output) */
int lfx_decode_batch_dict_device(lfx_ctx *c, int format, const lfx_dict *dict, uint32_t count, const void *d_in,
                                 const uint64_t *in_off, const uint64_t *in_len, void *d_out, const uint64_t *out_off,
                                 const uint64_t *out_cap, uint64_t *out_len, int32_t *status);
#define LFX_DEC_LAZY_HEADER 4u
int lfx_decoder_set_dict(lfx_decoder *d, const lfx_dict *dict);

/* ---- encoding with a preset dictionary: what zlib.decompressobj(zdict=...) and the decode calls above read ----
 * The reference has no dictionary-primed parse; this is the definition the encoder is exact with.
 *
 *  Let T be the usable tail of the dictionary, its last min(len, 32768) bytes, and buf the FIRST LZ77 flush unit ("chunk") of a
 *  stream as the plan cuts it (options and schedule as in the dictionary-less call).  The code words of that chunk are what
 *  DefaultLz77Encoder::flush (default.rs:69-109) writes for the buffer T ‖ buf when its prefix table already holds every
 *  position < |T|, each inserted once, in order, and its walk starts at i = |T|.  Everything else is the reference's:
 *    - end = max(3, |T| + |buf|) - 3, and the positions from end on are literals;
 *    - a candidate is the most recent earlier occurrence of the 3-byte prefix — the two prefixes that straddle the boundary, at
 *      |T|-2 and |T|-1, are positions of T, are in the table and depend on the chunk's first two bytes;
 *    - a candidate farther than window_size makes a literal, no older occurrence is tried;
 *    - lengths are capped by max_length; a match may start in T and run on into buf.
 *  The reference clears its buffer at every flush: later chunks are exactly what the dictionary-less call makes of them.
 *  (Whenever the reference's own flush of T ‖ buf has a code-word boundary at |T|, the chunk's code words are the suffix of that
 *  flush's output behind the boundary.)
 *
 *  Container.  LFX_ZLIB: CMF and FLEVEL as lfx_encode_device writes them, FDICT set, FCHECK recomputed, then DICTID =
 *  lfx_dict_id(dict) in four bytes, big-endian, the body, and the Adler-32 of the input only.  LFX_DEFLATE: the body alone.
 *  LFX_GZIP: LFX_E_ARG, whatever `dict` is.  dict == NULL: byte for byte the dictionary-less twin.  A dictionary of another
 *  context: LFX_E_ARG.  Options that do no matching (no_compression, LFX_LZ77_NOCOMPRESSION) still write FDICT and DICTID; their
 *  code words are unchanged.  Huffman coding, block cutting, packing and the checksum run unchanged on the new code words.
 *  In the batch call every stream's first chunk is primed by the one dictionary, read in place; status, LFX_E_NOSPACE and the
 *  zero fill are lfx_encode_batch_device's.  lfx_encode_dict_bound = lfx_encode_bound + 4 (0 where that is 0).
 *  The first encode call that uses a dictionary builds its prefix table on the device and keeps it in the lfx_dict.
 *  The stream encoder takes a dictionary through lfx_encoder_new_dict (below).
 *  Not covered: the members encode, the encode-time index, the N-GPU encode, lfx_lz77. */
uint64_t lfx_encode_dict_bound(uint64_t n, const lfx_encode_opts *o, const lfx_schedule *s);
int lfx_encode_dict_device(lfx_ctx *c, int format, const lfx_encode_opts *o, const lfx_schedule *s, const lfx_dict *dict,
                           const void *d_in, uint64_t n, void *d_out, uint64_t cap, uint64_t *out_len);
/* same, host buffers (staged like lfx_encode_host) */
int lfx_encode_dict_host(lfx_ctx *c, int format, const lfx_encode_opts *o, const lfx_schedule *s, const lfx_dict *dict,
                         const void *in, uint64_t n, void *out, uint64_t cap, uint64_t *out_len);
/* lfx_encode_batch_device with one dictionary for every stream (out_cap[i] >= lfx_encode_dict_bound(in_len[i])) */
int lfx_encode_batch_dict_device(lfx_ctx *c, int format, const lfx_encode_opts *o, const lfx_schedule *s, const lfx_dict *dict,
                                 uint32_t count, const void *d_in, const uint64_t *in_off, const uint64_t *in_len, void *d_out,
                                 const uint64_t *out_off, const uint64_t *out_cap, uint64_t *out_len, int32_t *status);
/* The batch packed back to back: the caller names no place for any stream.  Stream i is byte for byte the stream
 * lfx_encode_batch_device writes for record i with the same format, options and schedule — with `dict`, the stream
 * lfx_encode_batch_dict_device writes — container header, trailer and empty records (in_len == 0) included.  The streams' sizes
 * are known on the device behind the Huffman stage; a device scan places them, and they are packed where they stay:
 *   out_off[0] = 0, out_off[i + 1] = round_up(out_off[i] + out_len[i], align), *total = out_off[count - 1] + out_len[count - 1]
 * (the tail is not rounded); gap bytes are zero.  count == 0: LFX_OK, *total = 0.
 * align: a power of two in 1..4096, else LFX_E_ARG.  d_out must be 4-byte aligned (LFX_E_ARG).  dict (NULL: none): only with
 * LFX_ZLIB or LFX_DEFLATE, and a dictionary of this context, else LFX_E_ARG.  Options are served and refused exactly as by the
 * batch call of the same dictionary kind.  in_off, in_len, out_off, out_len and total are HOST memory; out_off, out_len and total
 * may each be NULL.  d_table (NULL: none; device memory, 8-byte aligned): count pairs {off, len} of uint64_t, the same layout —
 * for a kernel or an lfx_decode_batch_device call that follows without a host round trip of the caller's.
 * Capacity.  *total > cap: LFX_E_NOSPACE; *total, out_off[], out_len[] and d_table hold the layout the call would have produced,
 * no stream is written, [0, cap) may have been zero-filled, and the context is usable for the next call, as after a voided batch
 * call.  d_out == NULL with cap == 0 is therefore the size query (d_out == NULL with any other cap: LFX_E_ARG).  There is no
 * bound to meet: any cap >= *total serves, and the sum of lfx_encode_bound (lfx_encode_dict_bound) over the records, every term
 * rounded up to align, always does.
 * Reach.  d_out[0, min(cap, that sum)) is zero-filled first.  No byte at or behind cap changes its value; read-modify-writes of
 * whole dwords stay inside [d_out, d_out + ((cap + 3) & ~3)).  A NULL context: LFX_E_DEVICE, nothing written. */
int lfx_encode_batch_packed_device(lfx_ctx *c, int format, const lfx_encode_opts *o, const lfx_schedule *s,
                                   const lfx_dict *dict /* NULL: none */, uint32_t count,
                                   const void *d_in, const uint64_t *in_off, const uint64_t *in_len,
                                   uint32_t align, void *d_out, uint64_t cap,
                                   uint64_t *out_off, uint64_t *out_len, uint64_t *total,
                                   void *d_table /* optional, device: count x {off, len} as uint64 pairs */);
/* The inverse: a batch decoded back to back, placed by the decoded sizes.  The caller names no place and no
 * capacity for any stream.  Let size[i], sstat[i], scons[i] be what lfx_decode_batch_size_device reports for stream i — with
 * `dict`, what the same size walk reports with the dictionary's bytes as history in front of the streams that read it.
 * Sizes and layout.  §26's, by a device scan over the sizes:
 *   out_off[0] = 0, out_off[i + 1] = round_up(out_off[i] + size[i], align), *total = out_off[count - 1] + size[count - 1]
 * (the tail is not rounded).  align: a power of two in 1..4096, else LFX_E_ARG.  count == 0: LFX_OK, *total = 0.
 * Decode.  Stream i is decoded exactly as lfx_decode_batch_device — with `dict`, lfx_decode_batch_dict_device — decodes it with
 * out_off[i] as above and out_cap[i] = size[i]: d_out[out_off[i], +out_len[i]), out_len[i] and status[i] are that call's, on
 * damaged streams too (a stream that fails keeps the bytes it produced before the fault; a checksum mismatch is reported with
 * all of its bytes in place).  consumed[i] = scons[i].  The return value is LFX_OK with the per-stream verdicts in status[];
 * lfx_ctx_last_error is the first failed stream's message.  No byte of d_out outside the slots [out_off[i], out_off[i] + size[i])
 * is written — gap bytes keep their values — and nothing at or behind cap.
 * Capacity.  *total > cap: LFX_E_NOSPACE; out_off[], *total and d_table hold the layout, out_len[i] = size[i], status[i] =
 * sstat[i], consumed[i] = scons[i], d_out is untouched and the context is usable for the next call.  d_out == NULL with
 * cap == 0 is therefore the size query (d_out == NULL with any other cap: LFX_E_ARG); where nothing is to be written
 * (*total == 0) it answers LFX_OK with the same fields.
 * Inputs.  The streams are d_in[off, +len): EITHER in_off and in_len (host arrays) with d_in_table NULL, OR d_in_table (device
 * memory, 8-byte aligned: count pairs {off, len} of uint64_t, what lfx_encode_batch_packed_device writes to its d_table) with
 * in_off and in_len NULL — the call copies the table itself; both, or neither, or one host array alone: LFX_E_ARG.
 * dict (NULL: none): only with LFX_ZLIB or LFX_DEFLATE, and a dictionary of this context, else LFX_E_ARG; a zlib stream without
 * FDICT in the batch is decoded without it, one with another DICTID fails alone ("Dictionary mismatch").  out_off, out_len,
 * consumed, status and total are HOST memory and may each be NULL; d_table (NULL: none; device memory, 8-byte aligned): count
 * pairs {out_off, size}.  A NULL context: LFX_E_DEVICE, nothing written.
 * The container headers are parsed once for both halves, and no scratch grows with the output (rule 6 of the size calls).
 * Not covered: multi-member gzip, the seek index, the N-GPU calls.  There is no host form: Context.decode_batch_packed_host
 * (Python) stages the records as encode_batch_packed_host does. */
int lfx_decode_batch_packed_device(lfx_ctx *c, int format, const lfx_dict *dict /* NULL: none */, uint32_t count,
                                   const void *d_in,
                                   const uint64_t *in_off, const uint64_t *in_len,   /* host, or both NULL ...        */
                                   const void *d_in_table,                            /* ... then device: count x {off, len} */
                                   uint32_t align, void *d_out, uint64_t cap,
                                   uint64_t *out_off, uint64_t *out_len, uint64_t *consumed, int32_t *status,
                                   uint64_t *total, void *d_table /* optional, device */);

/* ---- a chain dictionary: LFX_LZ77_CHAIN and LFX_LZ77_LAZY through a preset dictionary ----
 * lfx_dict_new_chain makes a dictionary that also carries the hash chain of its own tail.  With it lfx_encode_dict_device,
 * lfx_encode_dict_host and lfx_encode_batch_dict_device serve LFX_LZ77_CHAIN_DEPTH(K), LFX_LZ77_LAZY_DEPTH(K) and
 * LFX_LZ77_LEVEL_N(n) (its candidates, its nice cut and its too-far rule over the same chain); a dictionary
 * made by lfx_dict_new keeps LFX_E_UNSUPPORTED for them.  For the kinds 0 and 1 and for every decode call a chain dictionary
 * is a plain one.  Arguments, status and lifetime are lfx_dict_new's.
 *
 *  Let T be the usable tail (at most 32768 bytes), buf the stream's first chunk as above, b = T ‖ buf, n = |b| and
 *  end = max(3, n) - 3.
 *    - Every position < end counts as inserted once, in order: every position of T, and with them |T|-2 and |T|-1, whose
 *      3-byte prefix runs into buf.
 *    - The candidates of a chunk position i >= |T|, i < end, are the first K earlier occurrences of b[i..i+3] in b, most
 *      recent first, cut off at the first one farther than window_size from i: the chunk's own occurrences, then |T|-1 and
 *      |T|-2 where their prefix matches, then the dictionary's, youngest first.
 *    - L(c) = 3 + the common prefix behind the three bytes, capped by max_length and by the end of b.  The longest wins,
 *      among equal lengths the nearest (LFX_LZ77_CHAIN's rule).
 *    - LFX_LZ77_CHAIN walks greedily from |T|.  LFX_LZ77_LAZY applies its rule there: position i is a literal when
 *      L(i + 1) > L(i), with L = 0 for positions >= end.  Positions < |T| are never visited; the positions from
 *      max(end, |T|) on are literals.
 *  Later chunks are not primed: they are what LFX_LZ77_CHAIN / LFX_LZ77_LAZY make of them without a dictionary.  The container
 *  is the one above (FDICT, DICTID, Adler-32 of the input only) with FLEVEL as the kinds 2 and 3 set it; LFX_GZIP stays
 *  LFX_E_ARG; an empty dictionary primes nothing; no_compression is as above.
 *  The chain is complete — it covers the whole tail, whatever window_size a call uses; the cut-off is applied from the chunk
 *  position — takes 64 KiB of device memory, and is built by the first chained encode that takes the dictionary, on the
 *  context's stream, and freed with the lfx_dict.  Nothing of a call stays in the context. */
lfx_dict *lfx_dict_new_chain(lfx_ctx *c, const void *bytes, uint64_t len, int on_device, int *status);

/* ---- the stream encoder with a preset dictionary: zlib's deflateSetDictionary on a z_stream, Python's
 * zlib.compressobj(zdict=...) — the streams lfx_decoder_set_dict reads, written without knowing their length in advance.
 * lfx_encoder_new with a dictionary.  It comes with the constructor, not with a set_dict call as for the decoder: a zlib
 * encoder writes its header inside the constructor, and FDICT and DICTID are part of that header.  Every other lfx_encoder_*
 * call takes the encoder as it takes one made by lfx_encoder_new.
 *
 *  1. dict == NULL: byte for byte lfx_encoder_new — status, messages and every byte the sink receives.
 *  2. Formats: LFX_ZLIB and LFX_DEFLATE.  LFX_GZIP is LFX_E_ARG (gzip has no preset dictionary), whatever `dict` is.
 *  3. A dictionary of another context is LFX_E_ARG.  A NULL context gives NULL with *status = LFX_E_DEVICE.
 *  4. The dictionary must outlive the encoder.
 *  5. Output.  The writes, flushes and the finish made on the encoder are its write schedule.  The bytes handed to the sink are
 *     exactly what lfx_encode_dict_host writes for the concatenated input with that schedule, the same options and the same
 *     dictionary: the stream's first LZ77 chunk is primed as defined above (§18; with a chain dictionary and the kinds 2, 3 and
 *     4: §21), every later chunk is what the dictionary-less stream encoder makes of it.  "First chunk" is a property of the
 *     stream, not of a batch of the encoder's: exactly one chunk is primed, whichever call closes its block and however the
 *     encoder groups blocks into GPU passes.  As in the one-shot call, the first chunk is the first flush of the LZ77 stage: a
 *     flush() before the first byte closes an empty block whose empty chunk is that first chunk — nothing behind it is primed —
 *     while writes of no bytes cut nothing.  An empty dictionary primes nothing.
 *  6. LFX_ZLIB: the header is CMF and FLEVEL as lfx_encoder_new writes them, FDICT set, FCHECK recomputed, then DICTID =
 *     lfx_dict_id(dict) big-endian — six bytes, handed to the sink inside this call.  The trailer's Adler-32 covers the input only.
 *  7. LFX_DEFLATE: the body alone.
 *  8. no_compression and LFX_LZ77_NOCOMPRESSION: the zlib header still carries FDICT and DICTID, the code words are unchanged.
 *  9. Served and refused (DESIGN.md §3.0, row `stream`): a dictionary made by lfx_dict_new with LFX_LZ77_CHAIN, LFX_LZ77_LAZY or
 *     LFX_LZ77_LEVEL is LFX_E_UNSUPPORTED, one made by lfx_dict_new_chain is served; block_merge stays LFX_E_UNSUPPORTED for the
 *     stream encoder, and its reason comes first; LFX_HUFFMAN_AUTO is served as without a dictionary.  The reason is
 *     lfx_ctx_last_error's.
 * 10. Codes mode (lfx_encoder_write_codes) is served: the header carries FDICT and DICTID, and the code words are
 *     Huffman-coded as they come — the caller's Lz77Encode did its own priming, and a Pointer of the first block may reach in
 *     front of byte 0 (the codes mode checks no distance against the position).  No match stage and no dictionary stage run.
 *  Nothing of an encoder's dictionary stays in the context: a dictionary-less encoder on the same context, before or after,
 *  launches what it launches without this call. */
lfx_encoder *lfx_encoder_new_dict(lfx_ctx *c, int format, const lfx_encode_opts *o, const lfx_dict *dict,
                                  lfx_write_cb w, lfx_flush_cb f, void *user, int *status);

/* ---- training a preset dictionary from sample records ----
 * zlib has no trainer; this one is a simplified FASTCOVER, defined here and in tests/dict_train_model.py (numpy), which the
 * device result equals byte for byte.  The result is what lfx_dict_new / lfx_dict_new_chain take.
 *
 *  Inputs.  `count` records in one buffer, record i at [off[i], off[i] + len[i]); off and len are HOST arrays.  The records must
 *  not overlap and must come in ascending order of off (off[i] >= off[i - 1] + len[i - 1]), else LFX_E_ARG; gaps between them
 *  are never read.  dict_size: the target size, 64..32768.  segment: the segment length k, 16..dict_size; 0 selects 128.  Fixed:
 *  d = 8 (the d-mer), f = 20 (2^20 counters).  The records' positions in record order, concatenated, are the position space
 *  [0, N); N > 2^31 is LFX_E_ARG.  Any other out-of-domain argument: LFX_E_ARG.  cap < dict_size: LFX_E_NOSPACE.  count == 0 or
 *  N == 0: LFX_OK and *dict_len = 0.  A NULL context: LFX_E_DEVICE, nothing written.
 *  Hash.  h(p) = (le64(bytes at p) * 0x9E3779B185EBCA87 mod 2^64) >> (64 - f), defined only where p + d does not pass the end of
 *  p's record.  Nothing is read across a record's end or outside the records.
 *  Counts.  freq[x] = the number of defined positions with h(p) == x, in 32 bits.
 *  Epochs.  E = dict_size / k, rounded down; epoch e owns the positions [e * N / E, (e + 1) * N / E) (integer division).  A
 *  position is a candidate when p + k stays inside its record.
 *  Score.  The score of a candidate is the sum of freq[h(q)] over q in [p, p + k - d], read from the counters as they stand when
 *  its epoch is decided, held in 32 bits: a sum above 2^32 - 1 counts as 2^32 - 1.  A non-candidate scores 0.  A d-mer that
 *  occurs twice in one segment counts twice.
 *  Selection.  Epochs are decided in order.  The pick of an epoch is the highest score, among equal scores the lowest position;
 *  an epoch whose best score is 0 picks nothing.  After a pick freq[h(q)] = 0 for every q of the picked segment — what keeps the
 *  same content from being picked twice.
 *  Assembly.  The picks sorted by score ascending — the best segment last, at the shortest distances — among equal scores the
 *  earlier epoch later.  The dictionary is the picked segments in that order, k bytes each: *dict_len is a multiple of k and may
 *  be less than dict_size.  Only d_dict[0, *dict_len) is written.
 *  The kernels run on the context's stream with no host wait between the epochs; the call returns when the dictionary is there.
 *  The scratch (4 MiB of counters, 12 bytes per record, 4 bytes per 256 positions, the epoch step's prefix words: at most
 *  512 x (4096 + k) x 8 bytes) is the context's and grows only. */
int lfx_dict_train_device(lfx_ctx *c, const void *d_samples, uint32_t count, const uint64_t *off, const uint64_t *len,
                          uint32_t dict_size, uint32_t segment, void *d_dict, uint64_t cap, uint64_t *dict_len);
/* same, host buffers: the bytes from the first record's start to the last record's end are staged like lfx_encode_host's input */
int lfx_dict_train_host(lfx_ctx *c, const void *samples, uint32_t count, const uint64_t *off, const uint64_t *len,
                        uint32_t dict_size, uint32_t segment, void *dict, uint64_t cap, uint64_t *dict_len);

/* ---- the byte-shuffle filter for numeric records ----
 * HDF5's H5Z_FILTER_SHUFFLE, which is numcodecs' Shuffle: the pre-filter in front of DEFLATE that HDF5 (shuffle=True,
 * compression="gzip"), Zarr (Shuffle + Zlib / GZip), Blosc and TIFF ship.  Defined here and in tests/shuffle_model.py (numpy),
 * which the device result equals byte for byte.
 *
 *  Definition.  For a record of n bytes and an element size s >= 1 let k = n / s (integer division) and r = n % s.
 *    LFX_SHUFFLE:    out[j * k + i] = in[i * s + j] for 0 <= i < k, 0 <= j < s; the r trailing bytes are copied,
 *                    out[k * s + t] = in[k * s + t].
 *    LFX_UNSHUFFLE:  the inverse permutation.
 *  s == 1, k <= 1 and n == 0 follow from the formula: the identity, or nothing to do.  Records are independent: nothing is read
 *  or written outside a record, and no byte outside [out_off[i], out_off[i] + len[i]) changes — records may lie back to back at
 *  any byte offset.
 *  Arguments.  elem_size: 1..256, dir: LFX_SHUFFLE or LFX_UNSHUFFLE, else LFX_E_ARG.  count == 0 and n == 0: LFX_OK, nothing
 *  written.  A NULL context: LFX_E_DEVICE, nothing written.
 *  Records (the batch call).  Record i is d_in[off, +len) and is written to d_out[out_off[i], +len).  EITHER in_off and len (host
 *  arrays) with d_table NULL, OR d_table (device memory, 8-byte aligned: count pairs {off, len} of uint64_t — what
 *  lfx_encode_batch_packed_device and lfx_decode_batch_packed_device write to their d_table) with in_off and len NULL; the call
 *  copies the table itself.  Both, neither, or one host array alone: LFX_E_ARG.  out_off (host) NULL: the output takes the input
 *  offsets, in d_out.  With d_table out_off must be NULL (LFX_E_ARG).
 *  Overlap.  There is no in-place form: a record's input bytes [d_in + off, +len) that meet any record's output bytes, or two
 *  output ranges that meet, are LFX_E_ARG, and nothing is written.  An offset plus its length beyond 64 bits: LFX_E_ARG.
 *  The device calls run one launch on the context's stream and return when the bytes are there; lfx_shuffle_host stages its
 *  buffers as lfx_encode_host does.  The scratch (24 bytes per record, 16 bytes per tile of about 16 KiB) is the context's and
 *  grows only.
 *  Not covered: bitshuffle, delta and predictor filters, the stream encoders and decoders, members / BGZF, the seek index, the
 *  N-GPU calls. */
enum { LFX_SHUFFLE = 0, LFX_UNSHUFFLE = 1 };
int lfx_shuffle_device(lfx_ctx *c, int dir, uint32_t elem_size, const void *d_in, uint64_t n, void *d_out);
int lfx_shuffle_batch_device(lfx_ctx *c, int dir, uint32_t elem_size, uint32_t count,
                             const void *d_in, const uint64_t *in_off, const uint64_t *len,   /* host, or both NULL ...        */
                             const void *d_table,                                             /* ... then device: count x {off, len} */
                             void *d_out, const uint64_t *out_off /* host; NULL: the input offsets */);
int lfx_shuffle_host(lfx_ctx *c, int dir, uint32_t elem_size, const void *in, uint64_t n, void *out);

/* ---- plug-in: libflate_lz77::Lz77Encode (libflate_lz77/src/lib.rs:83-107) -----------------
 * Codes are delivered in batches: word = (val << 16) | dist; dist == 0 → Code::Literal(val),
 * else Code::Pointer{length: val, backward_distance: dist} (lib.rs:27-42). */
typedef void (*lfx_sink_cb)(void *user, const uint32_t *codes, size_t n);
typedef struct lfx_lz77 lfx_lz77;
lfx_lz77 *lfx_lz77_new(lfx_ctx *c, uint32_t window_size, uint32_t max_length, int *status);
/* Lz77Encode::encode — buffers; flushes when >= window*8 bytes are held (default.rs:60-68) */
int lfx_lz77_encode(lfx_lz77 *z, const uint8_t *buf, size_t len, lfx_sink_cb sink, void *user);
/* Lz77Encode::flush (default.rs:69-109) */
int lfx_lz77_flush(lfx_lz77 *z, lfx_sink_cb sink, void *user);
uint32_t lfx_lz77_window_size(const lfx_lz77 *z); /* lib.rs:103-106 */
int lfx_lz77_compression_level(const lfx_lz77 *z); /* lib.rs:96-99 → LFX_LEVEL_BALANCE */
void lfx_lz77_free(lfx_lz77 *z);

/* ---- introspection used by tests / bench -------------------------------------------------- */
/* per-phase GPU milliseconds of the last encode/decode on this context (hipEvent-timed) */
typedef struct lfx_timing {
    float total_ms;
    float phase_ms[16];
    char phase_name[16][24];
    int n_phases;
} lfx_timing;
/* encode passes this context ran on the fallback match kernel because the ordered-LDS-exchange assumption of the default one
 *  was seen violated — 0 on every part measured so far; a non-zero value explains a 3x slower match stage */
uint64_t lfx_ctx_match_fallbacks(const lfx_ctx *c);
int lfx_ctx_last_timing(lfx_ctx *c, lfx_timing *t);
void lfx_ctx_enable_timing(lfx_ctx *c, int on);   /* 0: off; 1: a HIP event behind every phase of a call (lfx_ctx_last_timing);
                                                      2..5: only the two events around ONE kernel's phase — an event record between
                                                      two kernels costs ~6 us of idle GPU — 2: lz77_walk (parse_walk_kernel),
                                                      3: blk_scan, 4: lz77_cand (lz77_match7_kernel), 5: lz77_copy;
                                                      6: as 1, with the encode's match and parse phases split by kernel
                                                      (lz77_cand + lz77_resolve, lz77_walk + lz77_chain) */
uint32_t lfx_version(void);

#ifdef __cplusplus
}
#endif
#endif
