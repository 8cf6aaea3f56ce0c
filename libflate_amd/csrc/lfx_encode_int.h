// lfx_encode_int.h — the encode core (lfx_encode.cpp) as the entry points of lfx_api.cpp see it.  Internal: nothing here is
// part of the C ABI.
#pragma once
#include <vector>

#include "lfx_ctx.h"
#include "lfx_device.h"
#include "lfx_dict.h"
#include "lfx_enc_frame.h"
#include "lfx_plan.h"
#include "lfx_try.h"
#include "lfx_verdict.h"

namespace lfx {

// code words made on the host by a caller-supplied Lz77Encode (lfx_encoder_write_codes): contiguous, chunk after chunk
struct HostCodes {
    const uint32_t *codes;        // n_codes words, (val << 16) | dist, every block's EndOfBlock included
    uint64_t n_codes;
    const uint32_t *chunk_codes;  // codes per chunk of the plan
};

// an entry point asks the table (encode_served, lfx_enc_frame.h) about its call; the reason becomes the context's error
inline int served(Ctx *c, EncodeEntry e, const EncodeSpec &sp, const lfx_dict *dict = nullptr) {
    const char *why;
    const int rc = encode_served(e, sp, !dict ? DICT_NONE : dict->chain ? DICT_CHAIN : DICT_PLAIN, &why);
    if (rc) c->set_error(why);
    return rc;
}

// Stage A: plan upload → match → parse → histogram → Huffman (+ checksum: ck_mode 1 CRC-32, 2 Adler-32, 3 both — a shard, whose
// caller folds either).  Leaves everything the emit stage needs in the context.
// dict: a preset dictionary — the plan's CH_DICT chunks take their open candidates from it and the parse reads
// its window; nullptr: the kernels and launches of a dictionary-less call, unchanged.
// sp: the call's resolved options (encode_spec), which its entry point has asked encode_served about.  With a chain depth the
// chain stage runs between the match and the parse, for LFX_LZ77_LAZY with its demotion (§20); without: no
// stage, no second candidate buffer.
int encode_prepare(Ctx *c, const Plan &plan, const EncodeSpec &sp, const uint8_t *d_in, uint64_t n, int ck_mode,
                   const HostCodes *hc = nullptr, const lfx_dict *dict = nullptr);
// Stage B: offsets → pack → framing.  `prefix` bytes are placed at the start of d_out; the DEFLATE bits start at bit
// `start_bit` of d_out (prefix may end with a partial byte).
// async_slot (page-locked, the caller's own): the result is copied there and the call returns WITHOUT waiting — the stream
// encoder's batch in flight; the caller synchronises and reads the slot itself.  host_res is not touched then.
int encode_emit(Ctx *c, int format, bool with_trailer, uint32_t trailer_check, bool use_device_check, uint64_t total_n,
                const uint8_t *prefix, uint32_t prefix_len, uint64_t start_bit, uint8_t *d_out, uint64_t cap,
                EncodeResult *host_res, EncodeResult *async_slot = nullptr);
// the pack kernels over the prepared encode: every block's bits OR-ed into d_out at d_block_start[]
int pack_blocks(Ctx *c, void *d_out);

// The second-generation match kernel proves its one hardware assumption at run time; a violation voids the results
// and makes the context fall back to the first-generation kernel for good.
inline bool match_violation(Ctx *c, const EncodeResult &res) {
    if (!(res.match_flags & 1) || c->force_match_v1) return false;
    c->force_match_v1 = true;
    return true;
}
// body(): one encode pass that leaves its result record in `res`.  Run once more — on the fallback kernel — when that record
// reports a violation (never observed); force_match_v1 is sticky, so a second violation cannot occur.
template <class Body>
int with_match_fallback(Ctx *c, const EncodeResult &res, Body body) {
    int rc = body();
    if (match_violation(c, res)) rc = body();
    return rc;
}

// lfx_encode_batch_device behind its argument checks: the streams of the merged plan, encoded, packed and framed at out_off[]
struct BatchCall {
    int format;
    const std::vector<BatchStream> &streams;
    const std::vector<uint8_t> &hdr;
    const uint8_t *d_in;
    uint64_t in_extent;
    uint8_t *d_out;
    uint64_t out_lo, out_hi;      // the span of d_out the streams' ranges lie in
    const lfx_dict *dict = nullptr;   // lfx_encode_batch_dict_device: primes every stream's first chunk
};
int encode_batch(Ctx *c, const Plan &plan, const EncodeSpec &sp, const BatchCall &b, std::vector<uint64_t> &h_len,
                 std::vector<int32_t> &h_status, EncodeResult &res);
// lfx_encode_batch_packed_device behind its argument checks: the same merged plan, the streams laid out on the
// device behind the Huffman kernel and packed back to back.  streams[].out_off / out_cap are the device's to fill.
struct BatchPackedCall {
    int format;
    const std::vector<BatchStream> &streams;
    const std::vector<uint8_t> &hdr;
    const uint8_t *d_in;
    uint64_t in_extent;
    uint8_t *d_out;
    uint64_t cap, fill;           // fill: bytes of d_out to zero, min(cap, the sum of the streams' rounded bounds)
    uint32_t align;
    const lfx_dict *dict;
    uint64_t *d_table;            // the caller's device table of {off, len}, or nullptr
};
// h_pairs: {off, len} per stream; res.out_bytes = the total, res.status != 0: it exceeds cap and no stream was written
int encode_batch_packed(Ctx *c, const Plan &plan, const EncodeSpec &sp, const BatchPackedCall &b, std::vector<uint64_t> &h_pairs,
                        EncodeResult &res);
// lfx_encode_members_device behind its argument checks and the merged plan
struct MembersCall {
    MembersGeom g;
    const std::vector<uint8_t> &hdr;
    const uint8_t *d_in;
    uint8_t *d_out;
    uint64_t cap, fill;           // fill: bytes of d_out to zero, min(cap, bound)
    lfx_member *members;
    uint32_t n_rec;               // records the caller has room for
};
int encode_members(Ctx *c, const Plan &plan, const EncodeSpec &sp, const MembersCall &m, EncodeResult &res);

}  // namespace lfx
