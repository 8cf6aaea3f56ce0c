// lfx_stream_enc.h — the stream encoder's state machine: io::Write shaped ({deflate,zlib,gzip}::Encoder).  Everything that is
// not GPU work: the options, the write-schedule planner, when the closed blocks become a batch, the one-batch-in-flight protocol
// and the two input buffers it alternates between, the partial byte and the checksum carried between batches, the container
// header and trailer, the modes' rules, the sticky failure and the order of bytes and errors.  No HIP, no context: a plain host
// compiler builds it (tests/c/stream_enc.cpp runs it with kilobyte batches over a stand-in backend, also under the
// sanitizers).  The GPU enters at ONE place, the batch backend (lfx_stream_enc.cpp).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "lfx_enc_frame.h"
#include "lfx_plan.h"

namespace lfx {

// Closed blocks are encoded — and handed to the sink — once this much is waiting; the open block's bytes — all the reference
// itself would be holding (encode.rs:386-426) — stay in `pending`.  8 MiB keeps what the encoder buffers within eight default
// blocks (the reference emits per block, encode.rs:277-286) at a third of the one-shot call's throughput: a batch is one GPU
// pass with ~0.4 ms of fixed latency.  The product runs the defaults (LFX_ENC_BATCH_MB sets batch_bytes), and nothing else; the
// host test runs kilobytes.
struct BatchPolicy {
    uint64_t batch_bytes = 8ull << 20;    // raw bytes of closed blocks (either mode)
    // codes mode: code words of closed blocks (about 8 MiB of text).  (The byte threshold holds there too: a well-compressing
    // Lz77Encode — 258-byte matches — closes 2 M code words only after half a gigabyte of raw bytes.)
    uint64_t batch_codes = 2ull << 20;
    // no_compression: stored blocks (a batch is 64 MiB of them, copied, not compressed); they leave as they are closed
    uint64_t raw_blocks = 1024;
};

// a closed block of the codes mode: n_codes includes the EndOfBlock; BT_RAW = zlib sync marker
struct CodeBlock { uint64_t n_codes; uint32_t type, final; };

// The plan of a codes-mode batch (CompressBuf::flush from the histogram on, encode.rs:416-425): a chunk per compressed block,
// its code words where the block before's end.  chunk_codes: code words per chunk.
inline Plan codes_plan(const std::vector<CodeBlock> &cblocks, bool final_closed, std::vector<uint32_t> &chunk_codes) {
    Plan plan;
    chunk_codes.clear();
    uint64_t code_cursor = 0, tile_cursor = 0;
    for (const CodeBlock &cb : cblocks) {
        BlockDesc b{};
        b.type = cb.type;
        b.final = cb.final;
        b.first_chunk = (uint32_t)plan.chunks.size();
        if (cb.type != BT_RAW) {
            ChunkDesc ch{};
            ch.len = cb.n_codes - 1;            // (slots = len + 1, as for a chunk of len bytes that is all literals + EndOfBlock)
            ch.code_off = code_cursor;
            ch.block = (uint32_t)plan.blocks.size();
            ch.flags = CH_LAST_IN_BLOCK;
            ch.tile_base = tile_cursor;
            code_cursor += cb.n_codes;
            tile_cursor += div_up(cb.n_codes, PACK_TILE);
            plan.chunks.push_back(ch);
            chunk_codes.push_back((uint32_t)cb.n_codes);
            b.n_chunks = 1;
        }
        plan.blocks.push_back(b);
    }
    if (final_closed && !plan.blocks.empty()) plan.blocks.back().align_after = 1;     // Block::finish → BitWriter::flush encode.rs:301
    plan.n_codes_cap = code_cursor;
    plan.n_tiles = tile_cursor;
    return plan;
}
// room for a batch's output.  Bytes mode: a dynamic block never costs more than ~9 bits per literal + its header; stored: 5
// bytes per block.  Codes mode: a code costs at most 15 + 5 + 15 + 13 bits.
inline uint64_t bytes_bound(uint64_t n, uint64_t blocks) { return n + n / 4 + 1024 * blocks + 128; }
inline uint64_t codes_bound(uint64_t codes, uint64_t blocks) { return 6 * codes + 1024 * blocks + 128; }
// bytes of a batch's output that are whole — all of them when the batch ends the stream; the byte behind them, [whole], is the
// one the next batch's first bits share
inline uint64_t whole_bytes(uint64_t end_bit, bool final) { return final ? (end_bit + 7) / 8 : end_bit / 8; }

// One batch for the backend: the blocks of `plan` over in[0, n), their bits behind the carry_bits low bits of `carry` (the
// partial byte the batch before left), at most `bound` bytes of output; codes mode: the caller's code words instead of a match
// search (in[0, n) is then only checksummed).
// THE CONTRACT: launch() starts the work and waits for nothing.  From launch() until collect() has returned (or settle()),
// the backend may read in[0, n) and the code words at any time — the product's H2D copy is a DMA transfer straight out of them —
// and the state machine neither writes, moves nor frees them.  At most one batch is in flight.
struct EncBatch {
    Plan plan;                    // (the backend may move it out: it keeps it to run the batch again)
    const uint8_t *in = nullptr;
    uint64_t n = 0;
    uint8_t carry = 0;
    uint32_t carry_bits = 0;
    bool final = false;           // the batch ends the stream: its last block is byte-aligned, nothing is carried
    uint64_t bound = 0;
    bool coded = false;                       // codes mode: no match search, but the caller's code words —
    const uint32_t *codes = nullptr;          // n_codes words, every block's EndOfBlock included ...
    uint64_t n_codes = 0;
    const uint32_t *chunk_codes = nullptr;    // ... and how many of them each chunk of the plan holds
    // an encoder made with a preset dictionary: plan.chunks[0] is the stream's first chunk and carries CH_DICT —
    // the backend gives the encoder's dictionary to this batch, every time it runs it, and to no other
    bool primed = false;
};
// what collect() reports of the batch
struct EncDone {
    uint32_t status = 0;          // not 0: the output did not fit `bound`
    uint64_t end_bit = 0;         // bits of output, the carried ones in front included
    uint32_t crc32 = 0, adler32 = 1;   // of in[0, n), from fresh start values (the one the format's trailer holds)
    uint8_t shared = 0;           // output byte [whole_bytes(end_bit, final)]: the partial byte the next batch continues
};

// Buf: the byte buffers that cross to the backend (the product: page-locked vectors, lfx_hostio.h).
// Backend:  int launch(EncBatch &, std::string &err)          start the batch
//           int collect(EncDone &, std::string &err)          wait for it; its result, the way back of its bytes queued
//           int bytes(uint64_t whole, const uint8_t **p)      the collected batch's first `whole` output bytes, once they are here;
//                                                             valid until the next collect()
//           void settle()                                     wait for whatever is in flight (an encoder that is freed)
//           Buf take_out()                                    ... and its output buffer, for the pool the input buffers go to
//    (each → LFX_OK or a failure of the attempt itself; err: its text, where there is one)
template <class Buf, class Backend>
struct StreamEnc {
    Backend backend;
    BatchPolicy pol;
    int format;
    EncodeSpec spec;                    // resolved (encode_spec); its options' filename / comment / extra point into the copies below
    std::string filename, comment;
    std::vector<uint8_t> extra;
    Planner pl;                        // incremental write-schedule state (chunks / blocks of `pending`)
    lfx_write_cb w = nullptr;
    lfx_flush_cb f = nullptr;
    void *user = nullptr;
    Buf pending;                        // input bytes not yet in a batch: the planner's byte 0 is pending[0]
    Buf inflight_buf;                   // the input of the batch in flight (its first inflight_n bytes): the backend's until collected
    bool inflight = false, inflight_final = false;
    uint64_t inflight_n = 0;
    uint64_t total_in = 0, encoded_in = 0;
    uint32_t crc = 0, adler = 1;        // running container checksum (combined per batch)
    uint8_t carry = 0;                  // partial last byte of the bitstream so far
    uint32_t carry_bits = 0;
    bool finished = false, failed = false;
    std::string err;
    // ---- codes mode (write_codes): the caller runs its own Lz77Encode, the backend Huffman-codes what it emitted.
    // `pending` then holds the raw bytes whose checksum is still due (they are never matched).
    int mode = 0;                        // 0 undecided, 1 bytes (write), 2 codes
    std::vector<uint32_t> codes;         // code words of the closed blocks, then of the open one
    std::vector<CodeBlock> cblocks;      // closed blocks not yet encoded
    std::vector<uint32_t> chunk_codes;   // of the batch in flight
    uint64_t closed_codes = 0, open_codes = 0;
    bool final_closed = false;
    // ---- a preset dictionary (set_dict, before enc_open).  Opaque here: the backend knows what it points to.
    const void *dict = nullptr;
    uint32_t dict_id = 1;                // RFC 1950's DICTID, for the zlib header
    bool dict_usable = false;            // it has bytes to offer: the stream's first chunk is primed
    bool first_chunk_handed = false;     // the stream's first chunk has been handed to a batch (a property of the stream, not of a batch)
    void set_dict(const void *d, uint32_t id, bool usable) { dict = d; dict_id = id; dict_usable = usable; }

    // sp: what encode_spec(format_, ...) resolved
    StreamEnc(int format_, const EncodeSpec &sp) : format(format_), spec(sp), pl(spec.plan) {
        lfx_encode_opts &o = spec.o;
        if (o.filename) { filename = o.filename; o.filename = filename.c_str(); }
        if (o.comment) { comment = o.comment; o.comment = comment.c_str(); }
        if (o.extra) { extra.assign(o.extra, o.extra + o.extra_len); o.extra = extra.data(); }
    }
    StreamEnc(const StreamEnc &) = delete;
    StreamEnc &operator=(const StreamEnc &) = delete;
};

template <class E>
int enc_sink(E *e, const uint8_t *p, size_t n) {
    if (!n) return LFX_OK;
    int64_t r = e->w(e->user, p, n);
    if (r != (int64_t)n) { e->err = "write callback failed"; e->failed = true; return LFX_E_IO; }
    return LFX_OK;
}
template <class E>
int enc_flush_cb(E *e) {
    if (e->f && e->f(e->user) != 0) { e->err = "flush callback failed"; return LFX_E_IO; }
    return LFX_OK;
}

// A batch of n input bytes is encoded: its checksum folded into the running one, its bits counted → the bytes of output that
// are whole (all of them when `final`); the rest stays as `carry_bits` of the byte the backend fetched (EncDone::shared).
template <class E>
uint64_t enc_account(E *e, const EncDone &res, uint64_t n, bool final) {
    if (n) {
        if (e->format == LFX_GZIP) e->crc = e->encoded_in == 0 ? res.crc32 : crc32_combine(e->crc, res.crc32, n);
        if (e->format == LFX_ZLIB) e->adler = e->encoded_in == 0 ? res.adler32 : adler32_combine(e->adler, res.adler32, n);
        e->encoded_in += n;
    }
    e->carry_bits = final ? 0 : (uint32_t)(res.end_bit & 7);
    e->carry = e->carry_bits ? res.shared : 0;
    return whole_bytes(res.end_bit, final);
}

// start the batch; nothing is waited for.  The batch's bytes move to `inflight_buf`, the open block's bytes stay pending —
// ping-pong: appends of later writes must not move (or free) memory the backend is still reading.
template <class E>
int enc_launch(E *e, EncBatch &b) {
    e->inflight_buf.assign(e->pending.begin() + (std::ptrdiff_t)b.n, e->pending.end());
    e->inflight_buf.swap(e->pending);              // pending = the open block's bytes, inflight_buf = the batch (its first n bytes)
    b.in = e->inflight_buf.data();
    b.carry = e->carry;
    b.carry_bits = e->carry_bits;
    const uint64_t n = b.n;
    const bool final = b.final;
    if (int rc = e->backend.launch(b, e->err)) return rc;
    e->inflight = true;
    e->inflight_final = final;
    e->inflight_n = n;
    return LFX_OK;
}

// wait for the batch in flight and settle its account.  → *whole: its whole bytes of output, on their way (backend.bytes());
// *have: there was one.  A batch's failure surfaces here: at the call that collects it — like an io::BufWriter's.
template <class E>
int enc_collect(E *e, uint64_t *whole, bool *have) {
    *have = false;
    if (!e->inflight) return LFX_OK;
    e->inflight = false;
    EncDone res;
    if (int rc = e->backend.collect(res, e->err)) return rc;
    if (res.status != 0) { e->err = "output capacity too small"; return LFX_E_NOSPACE; }
    *whole = enc_account(e, res, e->inflight_n, e->inflight_final);
    if (e->mode == 2) {                            // (the code words of the batch are done with)
        e->codes.erase(e->codes.begin(), e->codes.begin() + (std::ptrdiff_t)e->closed_codes);
        e->closed_codes = 0;
        e->cblocks.clear();
    }
    *have = true;
    return LFX_OK;
}
// the collected batch's bytes to the sink
template <class E>
int enc_deliver(E *e, uint64_t whole) {
    const uint8_t *p = nullptr;
    if (int rc = e->backend.bytes(whole, &p)) return rc;
    return enc_sink(e, p, (size_t)whole);
}

// what is closed, as the next batch: bytes mode — the closed blocks of `pending` (all of it when `final`, which first closes
// the stream); codes mode — every closed block, with all the raw bytes that wait for their checksum
template <class E>
EncBatch enc_next_batch(E *e, bool final) {
    EncBatch b;
    if (e->mode == 2) {
        b.plan = codes_plan(e->cblocks, e->final_closed, e->chunk_codes);
        b.n = e->pending.size();
        b.final = e->final_closed;
        b.bound = codes_bound(b.plan.n_codes_cap, b.plan.blocks.size());
        b.coded = true;
        b.codes = e->codes.data();
        b.n_codes = b.plan.n_codes_cap;
        b.chunk_codes = e->chunk_codes.data();
        return b;
    }
    if (final) e->pl.finish();
    b.n = final ? e->pending.size() : e->pl.closed_bytes();
    b.plan = final ? std::move(e->pl.plan()) : e->pl.take_closed();
    b.final = final;
    b.bound = bytes_bound(b.n, b.plan.blocks.size());
    // the stream's first chunk, whichever batch it lands in (stored blocks have none; an empty chunk — a flush before the first
    // byte — is the first chunk, as it is the first flush of the Lz77Encode): that one is primed, and no later one
    if (e->dict && !e->first_chunk_handed && !b.plan.chunks.empty()) {
        e->first_chunk_handed = true;
        b.primed = e->dict_usable && dict_prime_first(b.plan);
    }
    return b;
}

// ONE BATCH IN FLIGHT (round 6).  The write() that closes a batch starts it and returns; the backend works while the caller
// copies the next batch's bytes in (io::copy: 8192 at a time).  The NEXT batch's start (or flush / finish) collects it.  In
// this order: collect the batch before → start the next → the earlier batch's bytes to the sink, while the backend works on the
// one just started → with `drain`, collect that one too and hand its bytes over.  The bytes and their order are those of a
// synchronous encoder.  Codes mode always drains.
template <class E>
int enc_run(E *e, bool final, bool drain = true) {
    EncBatch b = enc_next_batch(e, final);
    int rc;
    uint64_t prev = 0, cur = 0;
    bool have_prev = false, have_cur = false;
    if ((rc = enc_collect(e, &prev, &have_prev))) return rc;
    const bool launched = !b.plan.blocks.empty();
    if (launched && (rc = enc_launch(e, b))) return rc;
    if (have_prev && (rc = enc_deliver(e, prev))) return rc;
    if (drain && launched) {
        if ((rc = enc_collect(e, &cur, &have_cur))) return rc;
        if (have_cur && (rc = enc_deliver(e, cur))) return rc;
    }
    return LFX_OK;
}

// ---- the entry points' bodies (the C ABI around them: lfx_stream_enc.cpp)
// gzip/zlib write their header immediately (gzip.rs:805, zlib.rs:578)
template <class E>
int enc_open(E *e) {
    std::vector<uint8_t> hdr;
    if (int rc = container_header(e->format, e->spec.o, hdr)) return rc;
    if (e->dict) dict_header(e->format, e->dict_id, hdr);      // (the codes mode and stored blocks included: what the one-shot calls do)
    return enc_sink(e, hdr.data(), hdr.size());
}

// io::Write::write
template <class E>
int64_t enc_write(E *e, const uint8_t *p, size_t n) {
    if (e->finished) return -(int64_t)LFX_E_ARG;
    if (e->failed) return -(int64_t)LFX_E_IO;
    if (e->mode == 2) { e->err = "lfx_encoder_write on an encoder that takes code words"; return -(int64_t)LFX_E_ARG; }
    e->mode = 1;
    e->pending.insert(e->pending.end(), p, p + n);
    e->pl.write(n);
    e->total_in += n;
    if (e->pl.closed_bytes() >= e->pol.batch_bytes || (e->spec.plan.no_compression && e->pl.closed_blocks() >= e->pol.raw_blocks)) {
        // the batch is started; the next one — or flush / finish — collects it.  Stored blocks leave as they are closed.
        int rc = enc_run(e, false, /*drain=*/e->spec.plan.no_compression);
        if (rc) { e->failed = true; return -(int64_t)rc; }
    }
    return (int64_t)n;  // encode.rs:243: always consumes everything
}

template <class E>
int enc_write_codes(E *e, const uint32_t *codes, size_t n_codes, const uint8_t *raw, size_t n_raw, int end_block) {
    if (e->finished || e->final_closed || end_block < 0 || end_block > 2 || (n_codes && !codes) || (n_raw && !raw)) return LFX_E_ARG;
    if (e->failed) return LFX_E_IO;
    // stored blocks never run an Lz77Encode (RawBuf, encode.rs:348-383); bytes and codes cannot be mixed on one encoder
    if (e->mode == 1 || e->spec.plan.no_compression) { e->err = "lfx_encoder_write_codes on an encoder that takes bytes"; return LFX_E_ARG; }
    for (size_t i = 0; i < n_codes; i++) {       // Code::Literal(u8) / Code::Pointer{3..=258, 1..=32768} (lib.rs:27-42)
        const uint32_t dist = codes[i] & 0xFFFFu, val = codes[i] >> 16;
        if (dist == 0 ? val > 255 : (val < 3 || val > MAX_LENGTH || dist > MAX_WINDOW)) { e->err = "code word outside Code's domain"; return LFX_E_ARG; }
    }
    e->mode = 2;
    e->codes.insert(e->codes.end(), codes, codes + n_codes);
    e->open_codes += n_codes;
    e->pending.insert(e->pending.end(), raw, raw + n_raw);
    e->total_in += n_raw;
    if (!end_block) return LFX_OK;
    e->codes.push_back(CODE_EOB);            // encode.rs:417
    e->cblocks.push_back(CodeBlock{e->open_codes + 1, e->spec.plan.dynamic_huffman ? (uint32_t)BT_DYNAMIC : (uint32_t)BT_FIXED, end_block == 2 ? 1u : 0u});
    e->closed_codes += e->open_codes + 1;
    e->open_codes = 0;
    if (end_block == 2) e->final_closed = true;
    else if (e->closed_codes >= e->pol.batch_codes || e->pending.size() >= e->pol.batch_bytes) {
        // (the reference emits every block as it closes)
        int rc = enc_run(e, false);
        if (rc) { e->failed = true; return rc; }
    }
    return LFX_OK;
}

// io::Write::flush pushes everything to the inner writer
template <class E>
int enc_flush(E *e) {
    if (e->finished) return LFX_E_ARG;
    if (e->failed) return LFX_E_IO;
    if (e->mode == 2) {
        // the caller closed the block with E::flush()'s codes (end_block = 1) — Encoder::flush is Block::flush (encode.rs:245-248)
        if (e->open_codes) { e->err = "close the open block first (end_block = 1)"; return LFX_E_ARG; }
        if (e->spec.plan.zlib_sync) e->cblocks.push_back(CodeBlock{0, (uint32_t)BT_RAW, 0u});   // zlib_sync_flush encode.rs:225-234
    } else {
        e->pl.flush();
    }
    int rc = enc_run(e, false);
    if (!rc) rc = enc_flush_cb(e);
    if (rc) e->failed = true;
    return rc;
}

// Encoder::finish: the rest of the stream, the trailer, the flush callback.  A failure leaves the encoder finished.
template <class E>
int enc_finish(E *e) {
    if (e->finished) return LFX_E_ARG;
    if (e->failed) return LFX_E_IO;
    if (e->mode == 2 && !e->final_closed) { e->err = "close the final block first (end_block = 2)"; return LFX_E_ARG; }
    e->finished = true;
    int rc = enc_run(e, true);
    if (rc) return rc;
    uint8_t t[8];
    size_t nt = 0;
    if (e->format == LFX_GZIP) {  // Trailer::write_to gzip.rs:114-121; ISIZE wraps (gzip.rs:893)
        uint32_t c = e->total_in ? e->crc : 0, sz = (uint32_t)e->total_in;
        t[0] = c; t[1] = c >> 8; t[2] = c >> 16; t[3] = c >> 24;
        t[4] = sz; t[5] = sz >> 8; t[6] = sz >> 16; t[7] = sz >> 24;
        nt = 8;
    } else if (e->format == LFX_ZLIB) {  // zlib.rs:630-639
        uint32_t a = e->total_in ? e->adler : 1;
        t[0] = a >> 24; t[1] = a >> 16; t[2] = a >> 8; t[3] = a;
        nt = 4;
    }
    if ((rc = enc_sink(e, t, nt))) return rc;
    return enc_flush_cb(e);
}

// the end of an encoder, finished or not: the backend lets go of the batch in flight first (the DMA engine may still read its
// input), then `give` takes the three buffers that crossed to the backend (the product pools its page-locked ones)
template <class E, class Give>
void enc_close(E *e, Give give) {
    e->backend.settle();
    give(std::move(e->pending));
    give(e->backend.take_out());
    give(std::move(e->inflight_buf));
    delete e;
}

}  // namespace lfx
