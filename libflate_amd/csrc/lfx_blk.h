// lfx_blk.h — descriptors of the lane-parallel inflate path (lfx_inflate_fast.hip): scan jobs and results, emit jobs, units;
// the decode's error codes and the container header's verdict.
// Plain data, no HIP: the host-only stage logic (lfx_stages.h, lfx_stream_dec.h) and its CPU tests need no more than this.
#pragma once
#include <stdint.h>

namespace lfx {

// error codes → reference message texts (formatted on the host, format_error in lfx_verdict.h)
enum : uint32_t {
    ERR_NONE = 0,
    ERR_EOF,           // UnexpectedEof: "failed to fill whole buffer"
    ERR_HUFF,          // "Invalid huffman coded stream"                      huffman.rs:171-174
    ERR_CONFLICT,      // "Bit region conflict"                               huffman.rs:107-119
    ERR_HDIST,         // "The value of HDIST is too big: max=30, actual=N"   symbol.rs:395-403
    ERR_NO_PREV,       // "No preceding value"                                symbol.rs:470
    ERR_DIST_LIST,     // "The length of `distance_code_bitwidthes` is too large"  symbol.rs:433-443
    ERR_286,           // "The value N must not occur in compressed data"     symbol.rs:216-223
    ERR_BACKREF,       // "Too long backword reference: buffer.len=, distance="   lz77 lib.rs:173-185
    ERR_BTYPE3,        // "btype 0x11 of DEFLATE is reserved(error) value"    decode.rs:158-160
    ERR_LEN_NLEN,      // "LEN=.. is not the one's complement of NLEN=.."     decode.rs:88-93
    ERR_STORED_SHORT,  // "The reader has incorrect length: expected, read"   decode.rs:98-105
    ERR_NOSPACE,       // output capacity exhausted (ours)
    ERR_ZLIB_CHECK, ERR_METHOD, ERR_CINFO, ERR_FDICT,   // zlib.rs:229-259
    ERR_GZIP_ID, ERR_HCRC,                              // gzip.rs:398-441
    ERR_CRC32, ERR_ADLER32,                             // gzip.rs:1035-1040, zlib.rs:396-401
    ERR_DICT_MISMATCH, // "Dictionary mismatch: dictionary_id=, supplied=" (ours: the dictionary calls)
};

// what the container header parse (lfx_container.h: one source for the device kernel and the host stream decoder) reports
struct DecHeader {
    uint64_t deflate_off;  // first DEFLATE byte relative to the stream start
    uint32_t status;       // 0 ok, 1 InvalidData, 2 UnexpectedEof
    uint32_t err, a0, a1;
    uint32_t flags;        // gzip: FLG; zlib: HDR_DICT when FDICT was set and the caller's dictionary matched its DICTID
    uint32_t _pad;
};
constexpr uint32_t HDR_DICT = 0x100;

// ---- lane-parallel single-stream path (lfx_inflate_fast.hip)
enum : uint32_t { BLK_OK = 0, BLK_BAD = 1, BLK_NO_EOB = 2 };
constexpr uint32_t BLK_PIECE_KNOWN = 2;   // BlkJob::piece: a piece that starts at a known symbol boundary
struct BlkJob {
    uint64_t start_bit;  // block header bit
    uint64_t end_bit;    // range end guess: the next candidate's start (or the end of the input)
    // PIECE of a huge block (piece != 0): the job scans [first symbol boundary >= lo_bit, end_bit) with the tables
    // of the block whose header is at start_bit.  That boundary is found by a warm-up decode from warm_bit
    // (a few Kbit earlier, a speculative start that is in step long before lo_bit); the host accepts the piece
    // only if the boundary equals the exit of the piece before it.  A piece without EndOfBlock is "open":
    // status BLK_NO_EOB, but lanes / counts / end_bit (exit of its last lane) are valid.
    // Piece 0 starts behind the header like any job (warm_bit = 0).
    // piece == BLK_PIECE_KNOWN: lo_bit is a KNOWN symbol boundary of the block (a seek index's access point, or where the
    // piece in front of it ended): the job scans from exactly there, without a warm-up.
    uint64_t lo_bit, warm_bit;
    uint32_t piece, _pad;
    // the storing scan (round 6, launch_blk_scan_store): this job's lanes write their code words to temp + temp_off +
    // lane * cap (dwords); 0 = none
    uint64_t temp_off;
    uint32_t cap, _pad2;
};
struct BlkInfo {
    uint64_t end_bit;    // bit after EndOfBlock (stored: after the data)
    uint64_t n_out;      // bytes the block produces
    uint64_t data_bit;   // first symbol bit (stored: first data bit)
    uint32_t n_codes;
    uint32_t status, btype, bfinal, nlanes, rounds;
    uint32_t _pad;
    uint32_t cyc_hdr, cyc_total;   // shader-clock stamps (diagnostics)
};
struct BlkLanes {
    uint64_t start[1024];     // validated first bit of every lane's slice
    uint64_t out_off[1024];   // bytes of the block produced before the slice
    uint32_t code_off[1024];  // codes of the block before the slice
};
// what a storing scan leaves per lane for blk_place_kernel (indexed like BlkLanes)
struct BlkLanesX {
    uint32_t n_head[1024];    // the slice's codes: n_head of them from 0 of the lane's region ...
    uint32_t n_rest[1024];    // ... and n_rest from rest_at on
    uint32_t rest_at[1024];
    int32_t reach[1024];      // smallest (bytes of the slice produced before a match - its distance); INT32_MAX: no match
    uint32_t cut_code[1024];  // earliest cut of the slice no later code of the slice reads across: code index and byte offset,
    uint32_t cut_out[1024];   //   relative to the slice (cut_code 0xFFFFFFFF: none)
};
struct BlkEmit {
    uint64_t start_bit, data_bit;
    uint64_t code_off;   // first code slot of the block
    uint64_t out_off;    // first output byte of the block
    uint64_t n_out;
    uint32_t n_codes, nlanes, btype, cand;
    uint64_t hist;       // output bytes of the same member in front of the block (bounds its back-references)
    uint64_t end_limit;  // 0: the last lane decodes up to EndOfBlock; else (an open piece) up to this bit
    uint32_t preload;    // materialise: those bytes are already final in `out` — load up to 32 KiB of them as history
    uint32_t placed;     // round 6: 1 = the scan stored this block's codes (blk_place_kernel moves them; blk_emit_kernel skips the block)
    uint64_t temp_off;   // ... at temp + temp_off + lane * cap
    uint32_t cap;
    uint32_t dict_len;   // the dictionary instances only: of `hist`, so many bytes are the preset dictionary's tail (not in `out`)
};
constexpr uint32_t MAX_FREE_UNITS = 64;  // marker units per block (a schedule-S1 stream is ONE block)
struct BlkUnits {
    uint32_t n;          // independent units of the block (no back-reference crosses a cut)
    uint32_t code0[9];   // unit u covers codes [code0[u], code0[u+1]) of the block
    uint64_t out0[9];    // ... and bytes [out0[u], out0[u+1]) of the block's output
    uint32_t cyc[4];     // diagnostics: header, decode, cut search, unit selection (clock64 ticks)
    // the same block cut at slice boundaries WITHOUT regard to back-references (marker-based materialisation)
    uint32_t fn;
    uint32_t fcode0[MAX_FREE_UNITS + 1];
    uint64_t fout0[MAX_FREE_UNITS + 1];
};
// one unit of the marker-based path, in stream order
struct SymUnit {
    uint64_t start;      // first output byte
    uint64_t len;        // output bytes
};
}  // namespace lfx
