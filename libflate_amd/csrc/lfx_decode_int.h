// lfx_decode_int.h — what the decode's host sources share: the member decode and its stages (lfx_member.cpp) and the entry
// points around them (lfx_decode.cpp).  Internal: nothing here is part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/lfx.h"
#include "lfx_container.h"
#include "lfx_verdict.h"
#include "lfx_ctx.h"
#include "lfx_decode.h"
#include "lfx_stages.h"
#include "lfx_try.h"

namespace lfx {

struct MemberResult {
    int status = LFX_OK;
    uint64_t out_len = 0;        // bytes produced (also on failure)
    uint64_t blk_out_start = 0;  // bytes of completed blocks
    uint64_t end_byte = 0;       // input byte after the last DEFLATE byte (relative to member base)
    std::string msg;
    // windowed (partial) decode: where the decoded part ends and whether the member's last block is behind it
    uint64_t end_bit = 0;
    bool final_seen = false;
    bool need_cap = false;       // nothing decoded because the first block does not fit the output capacity
    // in: the container checksum the caller will need (launch_checksum mode: 1 CRC-32, 2 Adler-32, 0 none) and how many
    // trailer bytes follow the member; out (ck_done): checksum of the output and the trailer bytes, fetched in the SAME
    // host round trip as the materialisation's verdict (the checksum kernels are queued behind it before that verdict is
    // known: on the clean path one synchronisation less; a failed path simply ignores them)
    int ck_mode = 0;
    uint32_t trailer_len = 0;
    bool ck_done = false;
    uint32_t crc32 = 0, adler32 = 1;
    uint8_t trailer[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

struct DecodeOutcome {
    int status = LFX_OK;
    uint64_t out_len = 0, delivered_len = 0, consumed = 0;
    bool header_failed = false;  // the FIRST member's container header was rejected
    bool more = false;           // one_member: the member was verified and the loop stopped in front of the next one (at consumed)
    std::string msg;
};

// run `njobs` inflate jobs (the exact serial kernel) and fetch their results
// (dict_end: the dictionary instance — the jobs' dict_len bytes of history end there, lfx_decode.h)
int run_jobs(Ctx *c, const uint8_t *d_in, uint8_t *d_out, const std::vector<InflateJob> &jobs, std::vector<InflateResult> &res,
             const uint8_t *dict_end = nullptr);

// `consumed` behind an "Invalid huffman coded stream" verdict of the exact kernel (lfx_decode.cpp): the decode, the size call and
// the batch decode all report what the reference's reader has pulled from its input at that point
struct HuffProbe { uint64_t in_off, in_len; InflateResult r; uint64_t hist = 0; /* bytes of history in front of the stream (a preset dictionary) */ };
inline bool huff_verdict(const InflateResult &r) { return r.status == 1 && r.err == ERR_HUFF; }
int huff_consumed(Ctx *c, const uint8_t *d_in, const std::vector<HuffProbe> &probes, std::vector<uint64_t> &used);

// Decode the DEFLATE stream that starts at byte `off0` of d_in[0..n) into d_out[0..cap).
// hist0 = 0 (a member starts with an empty Lz77Decoder buffer, gzip.rs:1000-1005).
// stop_bit != ~0: the walk ends cleanly when a block ends exactly at stop_bit (a shard of a member that
// does not hold the BFINAL block); start_bit0 may be any bit of the first byte.
// partial: a WINDOW of a member (the stream decoders): decode the blocks that are complete in d_in[0..n) and fit into
// `cap`, stop cleanly in front of the first one that is not (mr.end_bit = its header bit, mr.final_seen = false); `hist`
// = bytes of the member produced by earlier windows — the last 32 KiB of them lie right in front of d_out.
// hist_win (not with partial): the history is DETACHED — a preset dictionary's tail, DESIGN §17: the last 32 KiB of the
// `hist` bytes are hist_win[0, 32768) (fewer: right-aligned), nothing in front of d_out is read.  Blocks that reach into it
// take the marker path with hist_win as the window in front of the first unit; the exact walk is the dictionary instance
// of the serial kernel.
int inflate_member(Ctx *c, const uint8_t *d_in, uint64_t n, uint64_t off0, uint8_t *d_out, uint64_t cap, MemberResult &mr,
                   uint64_t start_bit0 = ~0ull, uint64_t stop_bit = ~0ull, bool partial = false, uint64_t hist = 0,
                   const uint8_t *hist_win = nullptr);

// ---- stages that the N-GPU range calls and the size path run too

// The block finder over d_in[off0, n): find_launch queues stage 1, find_collect queues stage 2 behind it and brings the
// verdict back (a caller's phase stamp goes between the two).  The raw list: what a caller makes of it — a known first
// block, duplicates, an overflow — is the caller's business.
struct FindBufs {
    uint32_t shard_cap = 0, final_cap = 0;
    uint32_t *d_count = nullptr;      // the header (lfx_decode.h) ...
    uint64_t *d_final = nullptr;      // ... the results right behind it (both come back in ONE transfer) ...
    uint64_t *d_cand = nullptr;       // ... and stage 1's survivor lists
};
struct Found {
    std::vector<uint64_t> cand;       // header bits that passed stage 2, in no order (empty on overflow)
    bool overflow = false;            // a survivor list was full: the candidates are incomplete
    uint32_t n1 = 0;                  // survivors of stage 1
};
// BFINAL headers are reported from bit final_from of d_in on.
int find_launch(Ctx *c, const uint8_t *d_in, uint64_t n, uint64_t off0, uint64_t final_from, FindBufs &fb);
int find_collect(Ctx *c, const uint8_t *d_in, uint64_t n, const FindBufs &fb, Found &out);
// the finder's tail rule: the member's last block is looked for in the final eighth of the input, at least 8 MiB of it (one
// that starts earlier — a last block of more than that — is scanned, or walked, on demand by the chain walk)
inline uint64_t find_final_from(uint64_t n, uint64_t comp) {
    const uint64_t tail_bytes = std::max<uint64_t>(comp / 8, 8ull << 20);
    return comp > tail_bytes ? (n - tail_bytes) * 8 : 0;
}

// The storing scan's regions for bj[0, nj) (lfx_stages.h) and the two buffers they need.  false: no storing scan (the
// regions would not fit 16 GiB, or memory is short) — the jobs carry no region then.
bool plan_store(Ctx *c, BlkJob *bj, uint32_t nj);

// Candidates whose scan found no end-of-block — a false candidate inside the block cut its range guess short — are
// scanned again with wider and wider ranges (one round trip per widening step).  bi[slot[i]] is candidate i's result so
// far; a rescanned block's lanes land in its own slot i, which loses its `stored` mark.
int rescan_widen(Ctx *c, const uint8_t *d_in, uint64_t n, const std::vector<uint64_t> &starts, uint32_t nc,
                 std::vector<BlkInfo> &bi, std::vector<uint32_t> &slot, std::vector<uint8_t> &stored, bool scan_small);

// K2: the code words of emit[] into d_codes (blocks whose codes the scan stored are moved into place; the others are decoded
// a second time), flags and units beside them.  Leaves d_flags / d_emit in d_dec_tmp, the units in d_hist.
struct EmitBufs {
    uint32_t *d_flags = nullptr;
    BlkEmit *d_emit = nullptr;
};
int emit_codes(Ctx *c, const uint8_t *d_in, uint64_t n, const std::vector<BlkEmit> &emit, uint64_t total_codes, uint32_t n_placed,
               uint32_t free_shift, bool scan_small, EmitBufs &eb);

// ---- the two steps of a block round: one block of every live stream (the batch's fast path, the members walk, the reads
// of a seek index).  What a caller makes of a BlkInfo or a job flag — accept, drop, retry — is the caller's business.
// The scan of bj[]: bi[q] = job q's verdict, its lanes in d_dec_cand (want_tabs: its tables in d_dec_tabs, for emit_round).
// small = the 256-lane instances were picked (ranges of a few tens of KB); stamp: phase "blk_scan" behind the launch.
int scan_round(Ctx *c, const uint8_t *d_in, uint64_t n, const std::vector<BlkJob> &bj, bool want_tabs, std::vector<BlkInfo> &bi,
               bool &small, bool stamp = false);
// emit[] (jobs of the scan_round before it, want_tabs) decoded to code words and materialised into d_out; jf[q] != 0: job q
// reads in front of its history.  stamp: phases "blk_emit" and "lz77_copy".
// dict_end: the dictionary instance of the materialise kernel (the jobs' dict_len bytes of history end there).
int emit_round(Ctx *c, const uint8_t *d_in, uint64_t n, const std::vector<BlkEmit> &emit, uint64_t total_codes, bool small,
               uint8_t *d_out, std::vector<uint32_t> &jf, bool stamp = false, const uint8_t *dict_end = nullptr);

}  // namespace lfx
