// lfx_stream_dec.h — the stream decoder's state machine: io::Read shaped ({deflate,zlib,gzip}::Decoder, gzip::MultiDecoder,
// src/non_blocking/*).  Everything that is not GPU work: the reader, the container header, when a window is attempted and
// how it grows, the history and the checksum carried between windows, the trailer, the surplus, the order of bytes and errors,
// and the worker thread that decodes a window ahead.  No HIP, no context: a plain host compiler builds it
// (tests/c/stream_dec.cpp runs it with kilobyte windows over a stand-in backend, also under the sanitizers).  The GPU enters
// at ONE place, the window backend (lfx_stream_dec.cpp).
//
// Header first: the constructor pulls only what the container header needs (plus the rest of the chunk the reader
// handed over) and reports header errors (gzip.rs:941-944, zlib.rs:312-320); the body is decoded by the first
// read().  The GPU inflates whole members, so input is pulled in growing batches and a decode is ATTEMPTED whenever
// a batch is complete, the reader ends, hands over a short read, or (non-blocking mode) would block; an attempt
// that runs out of input (UnexpectedEof while the reader has not ended) simply waits for more.  Bytes pulled
// beyond the member's trailer are never decoded: they stay in the decoder (lfx_decoder_surplus) for the caller to
// hand to whatever reads next — what `into_inner()` amounts to for a reader that cannot be rewound
// (gzip.rs:987,1216-1226) — and MultiDecoder continues with them.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "lfx_container.h"
#include "lfx_verdict.h"

namespace lfx {

// The body is decoded a WINDOW at a time (the reference decodes one block per read, src/deflate/decode.rs:136-164, and keeps
// 32 KiB of history, libflate_lz77/src/lib.rs:219-231): pull up to window_in compressed bytes, decode the blocks that are
// complete in them and fit window_out (the backend, partial), serve those bytes, drop the input they used, keep the
// last 32 KiB of output as history — what is buffered never exceeds one window of input plus one window of output,
// whatever the member's size, and the first byte is served as soon as the first window is decoded.  The container
// checksum is folded window by window (CRC-32 / Adler-32 combine).  A window without one complete block (a block larger
// than the window: schedule-S1 members) doubles the window.
// window_in_max bounds the doubling (a damaged stream whose block never reaches an EndOfBlock, on a reader that
// never ends, must not pull the rest of the input into memory): at the limit the window is decoded WITHOUT `partial` — the
// exact walk gives a verdict for a damaged stream; a valid block larger than the limit is refused.
// Round 6: a window's kernels are bound by per-block latency, not by its size — 33 one-MiB blocks (16 MiB of text stream) take
// 2.0 ms of kernels where the whole 256-block stream takes 2.6 (LFX_DEBUG window lines) — so after a first window of window_in
// bytes (first bytes early) the later ones take window_in_later: half as many windows for 16 MiB more of page-locked memory.
// The product runs the defaults, and nothing else; the host test runs kilobytes.
struct WindowPolicy {
    uint64_t window_in = 16ull << 20, window_in_later = 32ull << 20, window_out = 96ull << 20, window_in_max = 4ull << 30;
    // small members: do not wait for a whole window.  1 MiB since round 6 — a reader that has less hands over a short read or
    // its end, either of which triggers an attempt; at 64 KiB a member of 1 MiB blocks made three attempts of 0.45 ms each
    // before its first block was complete
    uint64_t first_target = 1ull << 20;
    uint64_t retry_min = 1ull << 16;         // the least target after an attempt that found no complete block
    uint64_t pull = 4ull << 20;              // the most one read() asks the reader for
    uint64_t header_pull = 1ull << 16;       // ... while the container header is incomplete
    uint64_t ahead_min = 4ull << 20;         // a window of fewer bytes is not worth a thread decoding its successor ahead
    uint64_t history = MAX_WINDOW;           // bytes of output the next window's blocks may reach back into
};

// what the policy reads of a window's decode (the fields of the member decode's result, lfx_decode_int.h)
struct WindowResult {
    int status = LFX_OK;
    uint64_t out_len = 0;        // bytes produced (also on failure)
    uint64_t blk_out_start = 0;  // bytes of completed blocks
    uint64_t end_byte = 0;       // input byte after the last DEFLATE byte
    uint64_t end_bit = 0;        // where the decoded part ends ...
    bool final_seen = false;     // ... and whether the member's last block is behind it
    bool need_cap = false;       // nothing decoded because the first block does not fit the output capacity
    std::string msg;
};

// One window for the backend: the blocks of in[0, n) from bit bit_off of in[0] on, member_out bytes of the member in front of
// them, the last hist_len of those at hist.  in_base = the reader offset of in[0].  The backend answers as inflate_member
// (lfx_decode_int.h) does — with partial(): the blocks that are complete in in[0, n) and fit out_cap, end_bit in front of the
// first one that is not; without: the rest of the member, or its verdict — puts the bytes into W.out and their container
// checksum, from fresh start values, into W.crc / W.adler; W.rc = a failure of the attempt itself.  A decode without partial()
// that ends in LFX_E_NOSPACE is called again with twice the room: there is nothing to fetch for it.
struct WindowIn {
    const uint8_t *in;
    uint64_t n;
    uint32_t bit_off;
    const uint8_t *hist;
    uint64_t hist_len;
    uint64_t member_out;
    bool reader_eof;
    uint64_t out_cap;
    uint64_t in_base;
    int format;
    uint64_t in_max;             // WindowPolicy::window_in_max
    uint64_t dict_len = 0;       // a member that reads a preset dictionary: so many bytes of history lie in front of the member's
                                 //   first byte (the backend's reach bound is dict_len + member_out; `hist` holds them like output)
    // (once the reader has ended nothing more can arrive: the exact walk gives the member's verdict)
    bool at_limit() const { return !reader_eof && n >= in_max; }
    bool partial() const { return !reader_eof && !at_limit(); }
};

// a window's decode: what the backend fills
template <class Buf>
struct DecWindow {
    Buf out;
    WindowResult mr;
    uint32_t crc = 0, adler = 1;
    uint64_t n = 0;             // bytes of `in` the window was given
    int rc = LFX_OK;            // a failure of the attempt itself (the product: the device)
};

// Buf: the byte buffers that cross to the backend (the product: page-locked vectors, lfx_hostio.h — a window's H2D / D2H copies
// are DMA transfers straight out of / into them, and resize() does not zero-fill what a copy overwrites).
// Backend: callable as backend(const WindowIn &, DecWindow<Buf> &).
template <class Buf, class Backend>
struct StreamDec {
    Backend backend;
    WindowPolicy pol;
    bool debug = false;             // LFX_DEBUG: a line per window on stderr
    int format = 0;
    uint32_t flags = 0;
    lfx_read_cb r = nullptr;
    void *user = nullptr;
    Buf in;                         // pulled from the reader and not yet consumed by a decoded window
    bool reader_eof = false;
    enum State { ST_HEADER, ST_BODY, ST_SERVE, ST_DONE, ST_FAILED } state = ST_HEADER;
    bool first_member = true;
    // current member
    ContainerFields hf{};
    std::vector<uint8_t> hdr_bytes;
    bool have_header = false;
    Buf out;
    uint64_t cursor = 0, serve_limit = 0;
    int pending_status = LFX_OK;    // reported once the bytes in front of it have been served
    uint64_t consumed_total = 0;    // reader bytes that belong to finished members
    uint64_t target = 0;            // input size at which the next attempt is due
    uint64_t tried_at = 0;          // input size of the last attempt that ran out of input
    std::string err;
    // windowed body decode: the member is decoded a window of complete blocks at a time
    bool body_started = false;      // the header bytes have been dropped from `in`; in[0] holds the next block's first bit
    uint32_t bit_off = 0;           // ... at this bit of in[0]
    uint64_t member_out = 0;        // bytes of the member decoded by earlier windows
    std::vector<uint8_t> hist;      // the last (at most 32 KiB) of them: the LZ77 window the next blocks may reach into
    uint32_t run_crc = 0, run_adler = 1;   // container checksum over member_out bytes
    bool member_final = false;      // the BFINAL block has been decoded: the trailer is next
    bool more_windows = false;      // ST_SERVE: another window follows the bytes being served
    uint64_t out_cap = 0;           // output capacity of one window
    // ---- the next window decoded AHEAD (round 6): while the caller copies window k out of `out` (io::copy: 8192 bytes a
    // read), a worker thread runs window k + 1 through the backend into `next.out`.  The input was pulled by the CALLER's thread
    // before the worker started (the read callback never runs on another thread); the worker touches `in` (read only), `hist`
    // (read only), `next`, `out_cap` and the backend — nothing the serving path reads.
    typedef DecWindow<Buf> Window;
    Window next;
    std::thread worker;
    bool ahead = false;             // `worker` is running (or has finished) window k + 1
    // ---- a preset dictionary (lfx_decoder_set_dict): its usable tail (the caller's object owns the bytes) and its
    // id.  zlib: judged against the header's DICTID, used when FDICT is set; raw DEFLATE: always the history of byte 0
    bool has_dict = false;
    const uint8_t *dict = nullptr;
    uint64_t dict_len = 0;
    uint32_t dict_id = 1;
    bool header_fdict = false;      // the current member's header carried FDICT (and the dictionary matched)
    bool started = false;           // a header was parsed or a read was served: too late for a dictionary
    uint64_t member_dict() const { return has_dict && (format == LFX_DEFLATE || header_fdict) ? dict_len : 0; }
    ~StreamDec() { if (worker.joinable()) worker.join(); }     // (however the decoder goes: never from under its worker)
};

enum { PULL_OK = 0, PULL_EOF = 1, PULL_BLOCK = 2, PULL_ERR = 3 };
// one read() of up to `want` bytes from the inner reader
template <class D>
int dec_pull(D *d, size_t want, size_t *got) {
    *got = 0;
    if (d->reader_eof) return PULL_EOF;
    // (straight into the spare room behind `in` — page-locked, no zero fill, no second copy; the vector grows geometrically,
    //  so a reader that hands over a few bytes at a time does not pay for `want` bytes each time)
    const size_t old = d->in.size();
    d->in.resize(old + want);
    const int64_t k = d->r(d->user, d->in.data() + old, want);
    d->in.resize(old + (k > 0 ? (size_t)std::min<int64_t>(k, (int64_t)want) : 0));
    if (k == -(int64_t)LFX_E_WOULD_BLOCK) return PULL_BLOCK;
    if (k < 0) return PULL_ERR;
    if (k == 0) { d->reader_eof = true; return PULL_EOF; }
    *got = (size_t)k;
    return PULL_OK;
}
// PULL_ERR as the decoder's verdict
template <class D>
int dec_reader_failed(D *d) {
    d->err = "read callback failed";
    return LFX_E_IO;
}
// a member settles with nothing to serve: only a verdict, or the next member, follows
template <class D>
void dec_serve_nothing(D *d) {
    d->out.clear(); d->cursor = 0; d->serve_limit = 0; d->more_windows = false;
}

// parse the container header at the front of d->in, pulling what is missing.
// → LFX_OK (have_header set), LFX_E_WOULD_BLOCK, LFX_E_IO, or the header's own failure (err set)
template <class D>
int dec_header(D *d) {
    if (d->format == LFX_DEFLATE) { d->have_header = true; d->hf = ContainerFields{}; d->hdr_bytes.clear(); return LFX_OK; }
    d->started = true;
    for (;;) {
        ContainerFields cf;
        DecHeader h = parse_container(d->format, d->in.data(), d->in.size(), &cf);
        if (d->has_dict && d->format == LFX_ZLIB) h = resolve_fdict(h, d->dict_id);
        if (h.status == 0) {
            d->header_fdict = d->format == LFX_ZLIB && (h.flags & HDR_DICT);
            d->hf = cf;                    // (a header that fails to parse leaves the previous member's in place)
            d->hdr_bytes.assign(d->in.begin(), d->in.begin() + (size_t)h.deflate_off);
            d->have_header = true;
            return LFX_OK;
        }
        if (h.status == 2 && !d->reader_eof) {          // the header may simply not be complete yet
            size_t got;
            const int pr = dec_pull(d, (size_t)d->pol.header_pull, &got);
            if (pr == PULL_BLOCK) return LFX_E_WOULD_BLOCK;
            if (pr == PULL_ERR) return dec_reader_failed(d);
            continue;
        }
        d->err = format_error(h.err, h.a0, h.a1);
        d->consumed_total += h.deflate_off;
        return map_status(h.status);
    }
}

// ---- one window of the member's body in three steps: input (caller's thread) → backend (caller's thread, or a worker thread
//      that decodes AHEAD while the caller drains the window before) → state update (dec_apply)
// input up to the window size; a short read or the end of the reader also triggers an attempt.  → LFX_OK: attempt now
template <class D>
int dec_fill(D *d) {
    bool attempt = d->reader_eof;
    while (!attempt) {
        if (d->in.size() >= d->target) { attempt = true; break; }
        size_t got;
        const size_t want = std::min<uint64_t>(d->target - d->in.size(), d->pol.pull);
        const int pr = dec_pull(d, want, &got);
        if (pr == PULL_ERR) return dec_reader_failed(d);
        if (pr == PULL_EOF) { attempt = true; break; }
        if (pr == PULL_BLOCK) {
            // everything the peer has sent is here: decode it if enough new bytes arrived since an attempt that found
            // no complete block (an eighth more: the retries of one long block stay linear in its size), else WouldBlock
            if (d->in.size() > d->tried_at + d->tried_at / 8) { attempt = true; break; }
            return LFX_E_WOULD_BLOCK;
        }
        // a short read hints that the reader has no more right now (pipes, sockets): worth an attempt once the
        // input has grown by a quarter since the last one (keeps the total work linear)
        if (got < want && d->in.size() >= d->tried_at + d->tried_at / 4 + 1) { attempt = true; break; }
    }
    return LFX_OK;
}

// one window through the backend (the product: on the GPU, one decode at a time per context): in[0, n) from bit bit_off with
// the history → W.  Reads d->in, d->hist, d->bit_off, d->member_out, d->reader_eof, d->consumed_total, d->out_cap (grows it
// when the tail of the member does not fit); writes only W and d->out_cap.
template <class D>
void dec_window(D *d, typename D::Window &W) {
    for (;;) {
        const WindowIn wi{d->in.data(), d->in.size(), d->bit_off, d->hist.data(), d->hist.size(), d->member_out, d->reader_eof,
                          d->out_cap, d->consumed_total, d->format, d->pol.window_in_max, d->member_dict()};
        W.n = wi.n;
        W.crc = 0;
        W.adler = 1;
        W.rc = LFX_OK;
        W.mr = WindowResult();
        d->backend(wi, W);
        if (W.rc) return;
        if (wi.at_limit() && W.mr.status == LFX_E_UNEXPECTED_EOF) {
            W.mr.status = LFX_E_UNSUPPORTED;
            W.mr.msg = "a DEFLATE block exceeds the stream decoder's window limit (4 GiB of compressed bytes)";
        }
        if (W.mr.status == LFX_E_NOSPACE && !wi.partial()) {     // (the tail of the member does not fit one window: grow and retry)
            d->out_cap *= 2;
            continue;
        }
        return;
    }
}

// ST_SERVE, first read of a window that is worth the thread (a few MiB to copy out) and has a successor: pull the successor's
// input NOW, on the caller's thread, and let a worker decode it while the caller drains this window.  Not for non-blocking
// readers (a WouldBlock in the middle of a drain has no call to come back from).
template <class D>
void dec_start_ahead(D *d) {
    if (d->ahead || !d->more_windows || d->member_final || d->pending_status != LFX_OK || (d->flags & LFX_DEC_NONBLOCKING) ||
        !d->body_started || d->serve_limit < d->pol.ahead_min) return;
    if (dec_fill(d) != LFX_OK) return;                 // (an I/O error is found again, and reported, by the window's own turn)
    if (d->in.empty()) return;
    try {
        d->worker = std::thread([d] {
            try { dec_window(d, d->next); }
            catch (const std::bad_alloc &) { d->next.rc = LFX_E_OOM; }
            catch (...) { d->next.rc = LFX_E_DEVICE; }
        });
        d->ahead = true;
    } catch (...) {
        d->ahead = false;                              // (no thread to be had: the window is decoded when its turn comes)
    }
}
// accessors and the destructor look at state the worker may be writing: let it finish first
template <class D>
void dec_settle(D *d) {
    if (d->ahead && d->worker.joinable()) d->worker.join();
}

// ---- the body's three steps (dec_body runs them in turn)
// The member's blocks are done: the trailer (gzip.rs:1030-1042, zlib.rs:387-401).  → LFX_OK: settled, state ST_SERVE
template <class D>
int dec_trailer(D *d) {
    const uint64_t trailer = trailer_len(d->format);
    const uint64_t tpos = d->bit_off ? 1 : 0;       // (the last block ends inside in[0]: the trailer is byte aligned)
    while (d->in.size() < tpos + trailer && !d->reader_eof) {
        size_t got;
        const int pr = dec_pull(d, (size_t)(tpos + trailer - d->in.size()), &got);
        if (pr == PULL_ERR) return dec_reader_failed(d);
        if (pr == PULL_BLOCK) return LFX_E_WOULD_BLOCK;
    }
    dec_serve_nothing(d);
    d->pending_status = LFX_OK; d->err.clear();
    if (d->in.size() < tpos + trailer) {
        d->pending_status = LFX_E_UNEXPECTED_EOF;
        d->err = "failed to fill whole buffer";
        d->consumed_total += d->in.size();
        d->in.clear();
    } else {
        d->pending_status = check_trailer(d->format, d->in.data() + tpos, d->run_crc, d->run_adler, d->err);
        d->consumed_total += tpos + trailer;
        d->in.erase(d->in.begin(), d->in.begin() + (std::ptrdiff_t)(tpos + trailer));   // what is left is the surplus
    }
    d->body_started = false;
    d->state = D::ST_SERVE;
    return LFX_OK;
}

// Input (dec_fill) and one window through the backend (dec_window) — or the window the worker thread decoded ahead while the
// caller was copying the one before out (dec_start_ahead).  → LFX_OK: d->next holds the window; LFX_E_WOULD_BLOCK / LFX_E_IO
// from the reader, or the attempt's own failure
template <class D>
int dec_take_window(D *d) {
    if (d->ahead) {
        if (d->worker.joinable()) d->worker.join();      // (an accessor may have waited for it already)
        d->ahead = false;
    } else {
        const int fr = dec_fill(d);
        if (fr != LFX_OK) return fr;
        dec_window(d, d->next);
    }
    return d->next.rc;
}

// history: the last 32 KiB of (history ++ the window's output, d->out)
template <class D>
void dec_keep_history(D *d) {
    const uint64_t H = d->pol.history;
    if (d->out.size() >= H) d->hist.assign(d->out.end() - (std::ptrdiff_t)H, d->out.end());
    else {
        d->hist.insert(d->hist.end(), d->out.begin(), d->out.end());
        if (d->hist.size() > H) d->hist.erase(d->hist.begin(), d->hist.end() - (std::ptrdiff_t)H);
    }
}

// The window's verdict becomes decoder state.  → true: bytes or a verdict are ready (state ST_SERVE); false: no complete
// block in this window — more input or more room, and another attempt
template <class D>
bool dec_apply(D *d) {
    typename D::Window &W = d->next;
    const uint64_t n = W.n;
    const WindowResult &mr = W.mr;
    d->out.swap(W.out);                          // (the window's bytes; W.out keeps the old buffer's room for the next one)
    if (d->debug)
        fprintf(stderr, "[lfx] window: n=%llu bit_off=%u eof=%d hist=%llu → status=%d out=%llu blk_out=%llu end_bit=%llu final=%d need_cap=%d target=%llu\n",
                (unsigned long long)n, d->bit_off, (int)d->reader_eof, (unsigned long long)d->member_out, mr.status,
                (unsigned long long)mr.out_len, (unsigned long long)mr.blk_out_start, (unsigned long long)mr.end_bit,
                (int)mr.final_seen, (int)mr.need_cap, (unsigned long long)d->target);
    if (mr.status == LFX_OK && mr.out_len == 0 && !mr.final_seen) {
        // no complete block in this window: more input (or, for a block that does not fit, more room)
        if (mr.need_cap) { d->out_cap *= 2; return false; }
        if (d->reader_eof || n >= d->pol.window_in_max) {
            // (cannot happen with !partial; kept as the way out of a reader that never ends on a broken stream)
            d->pending_status = LFX_E_UNEXPECTED_EOF; d->err = "failed to fill whole buffer";
            dec_serve_nothing(d);
            d->state = D::ST_SERVE;
            return true;
        }
        d->tried_at = n;
        d->target = std::max<uint64_t>(d->target, std::max<uint64_t>(2 * n, d->pol.retry_min));   // the next try: twice what did not suffice
        return false;
    }
    // ---- bytes (and maybe a verdict) to serve
    d->cursor = 0;
    d->pending_status = LFX_OK;
    d->err.clear();
    d->state = D::ST_SERVE;
    if (mr.status != LFX_OK) {
        // the reference hands out what completed blocks produced, then the error (decode.rs:136-164); everything
        // produced stays available through unread_decoded_data (decode.rs:68-73)
        d->serve_limit = mr.blk_out_start;
        d->pending_status = mr.status;
        d->err = mr.msg;
        d->more_windows = false;
        const uint64_t used = std::min<uint64_t>(mr.end_byte, n);
        d->consumed_total += used;
        d->in.erase(d->in.begin(), d->in.begin() + (std::ptrdiff_t)used);
        d->body_started = false;
        return true;
    }
    d->serve_limit = mr.out_len;
    if (trailer_len(d->format) && mr.out_len) {
        d->run_crc = lfx_crc32_combine(d->run_crc, W.crc, mr.out_len);
        d->run_adler = lfx_adler32_combine(d->run_adler, W.adler, mr.out_len);
    }
    d->member_out += mr.out_len;
    dec_keep_history(d);
    // input: everything in front of the byte that holds the next unread bit is done with
    const uint64_t used = std::min<uint64_t>(mr.end_bit / 8, n);
    d->consumed_total += used;
    d->in.erase(d->in.begin(), d->in.begin() + (std::ptrdiff_t)used);
    d->bit_off = (uint32_t)(mr.end_bit & 7);
    d->member_final = mr.final_seen;
    d->more_windows = true;                        // (the trailer check, at least, follows)
    d->target = std::max<uint64_t>(d->member_out > mr.out_len ? d->pol.window_in_later : d->pol.window_in,
                                   d->target > d->pol.first_target ? d->target : 0);
    d->tried_at = 0;
    return true;
}

// → LFX_OK when bytes or a verdict are ready (state ST_SERVE), LFX_E_WOULD_BLOCK / LFX_E_IO from the reader, or the backend's
// failure
template <class D>
int dec_body(D *d) {
    if (!d->body_started) {
        // the header has been parsed on the host (dec_header): drop its bytes, the first block starts at bit 0
        const size_t hl = d->hdr_bytes.size();
        d->in.erase(d->in.begin(), d->in.begin() + (std::ptrdiff_t)std::min(hl, d->in.size()));
        d->consumed_total += hl;
        d->body_started = true;
        d->bit_off = 0; d->member_out = 0; d->hist.clear(); d->run_crc = 0; d->run_adler = 1; d->member_final = false;
        // (a preset dictionary is history like any other: the first window finds its tail where later ones find earlier output;
        //  the container checksum never covers it)
        if (const uint64_t dl = d->member_dict()) d->hist.assign(d->dict, d->dict + dl);
        d->target = 0; d->tried_at = 0;
        d->out_cap = d->pol.window_out;
    }
    if (d->target == 0) d->target = d->pol.first_target;
    for (;;) {
        if (d->member_final) return dec_trailer(d);
        if (const int rc = dec_take_window(d)) return rc;
        if (dec_apply(d)) return LFX_OK;
    }
}

// ---- the entry points' bodies (the C ABI around them: lfx_stream_dec.cpp)
// gzip / zlib constructors read the header and can fail (gzip.rs:941-944, zlib.rs:312-320); the non-blocking decoders read
// it lazily (src/non_blocking/gzip.rs:64-88).  → LFX_OK, or the header's failure (err set)
template <class D>
int dec_open(D *d) {
    if (d->flags & (LFX_DEC_NONBLOCKING | LFX_DEC_LAZY_HEADER)) return LFX_OK;
    const int rc = dec_header(d);
    if (rc == LFX_OK) d->state = D::ST_BODY;
    return rc;
}

// io::Read::read.  A failure of the backend itself (next.rc) leaves err as it was: the caller knows where its text is.
template <class D>
int64_t dec_read(D *d, uint8_t *out, size_t cap) {
    if (cap == 0) return 0;  // never latches end-of-stream (gzip.rs:1025-1027, zlib.rs:383-385)
    d->started = true;
    for (;;) {
        switch (d->state) {
            case D::ST_DONE: return 0;
            case D::ST_FAILED: return 0;   // (the error was reported once, like a latched io::Error)
            case D::ST_SERVE: {
                if (d->cursor < d->serve_limit) {
                    if (d->cursor == 0) dec_start_ahead(d);       // (the next window on the GPU while this one is copied out)
                    const uint64_t k = std::min<uint64_t>(cap, d->serve_limit - d->cursor);
                    memcpy(out, d->out.data() + d->cursor, k);
                    d->cursor += k;
                    return (int64_t)k;
                }
                if (d->pending_status != LFX_OK) { d->state = D::ST_FAILED; return -(int64_t)d->pending_status; }
                if (d->more_windows) { d->state = D::ST_BODY; continue; }      // the next window (or the trailer)
                if (d->format == LFX_GZIP && (d->flags & LFX_DEC_MULTI)) {   // MultiDecoder::read gzip.rs:1142-1166
                    d->first_member = false;
                    d->state = D::ST_HEADER;
                    continue;
                }
                d->state = D::ST_DONE;
                return 0;
            }
            case D::ST_HEADER: {
                const uint64_t before = d->consumed_total;
                const int rc = dec_header(d);
                if (rc == LFX_E_WOULD_BLOCK) return -(int64_t)LFX_E_WOULD_BLOCK;
                if (rc == LFX_E_UNEXPECTED_EOF && !d->first_member) {
                    // a following member's header that ends early = clean end of the stream (gzip.rs:1150-1156);
                    // the partial header bytes were read
                    d->consumed_total = before + d->in.size();
                    d->in.clear();
                    d->err.clear();
                    d->state = D::ST_DONE;
                    return 0;
                }
                if (rc) { d->state = D::ST_FAILED; return -(int64_t)rc; }
                d->state = D::ST_BODY;
                continue;
            }
            case D::ST_BODY: {
                const int rc = dec_body(d);
                if (rc == LFX_E_WOULD_BLOCK) return -(int64_t)LFX_E_WOULD_BLOCK;
                if (rc) { d->state = D::ST_FAILED; return -(int64_t)rc; }
                continue;
            }
        }
    }
}
// data decoded but not handed out: the rest of completed blocks + the partial block (decode.rs:68-73)
template <class D>
void dec_unread(D *d, const uint8_t **p, size_t *n) {
    const uint64_t start = std::min<uint64_t>(d->cursor, d->out.size());
    *p = d->out.data() + start;
    *n = d->out.size() - start;
}
// input pulled from the reader that lies behind the last finished member (only meaningful between members /
// at the end: while a member is being collected `in` holds that member's bytes)
template <class D>
void dec_surplus(D *d, const uint8_t **p, size_t *n) {
    const bool settled = (d->state == D::ST_SERVE && !d->more_windows && !d->body_started) || d->state == D::ST_DONE ||
                         d->state == D::ST_FAILED;
    *p = d->in.data();
    *n = settled ? d->in.size() : 0;
}
template <class D>
int dec_header_get(D *d, lfx_header *h) {
    memset(h, 0, sizeof *h);
    if (!d->have_header) {
        if (!(d->flags & (LFX_DEC_NONBLOCKING | LFX_DEC_LAZY_HEADER)) || d->state != D::ST_HEADER) return LFX_E_ARG;
        const int rc = dec_header(d);          // non-blocking decoders read the header on demand (non_blocking/gzip.rs:98-113)
        if (rc) { if (rc != LFX_E_WOULD_BLOCK) d->state = D::ST_FAILED; return rc; }
        d->state = D::ST_BODY;
    }
    const ContainerFields &f = d->hf;
    const uint8_t *b = d->hdr_bytes.data();
    h->format = d->format;
    if (d->format == LFX_GZIP) {
        h->mtime = f.mtime;
        h->xfl = f.xfl;
        h->os = f.os;
        h->is_text = (f.flg & 1) != 0;
        h->is_verified = (f.flg & 2) != 0;
        if (f.flg & 4) { h->extra = b + f.extra_off; h->extra_len = (uint32_t)f.extra_len; h->has_extra = 1; }
        if (f.name_len) h->filename = (const char *)(b + f.name_off);
        if (f.comment_len) h->comment = (const char *)(b + f.comment_off);
    } else if (d->format == LFX_ZLIB) {
        h->zlib_window_size = 1u << (((uint32_t)f.cmf >> 4) + 8);   // Lz77WindowSize (zlib.rs:99-173)
        h->zlib_level = (uint32_t)f.flg >> 6;                        // CompressionLevel (zlib.rs:28-58)
    }
    return LFX_OK;
}
// the end of a decoder: the worker first, then `give` takes the three buffers that crossed to the backend (the product
// pools its page-locked ones), then the decoder goes
template <class D, class Give>
void dec_close(D *d, Give give) {
    dec_settle(d);
    give(std::move(d->in));
    give(std::move(d->out));
    give(std::move(d->next.out));
    delete d;
}
// a preset dictionary for the decoder: only before anything was parsed or served, never for gzip
template <class D>
int dec_set_dict(D *d, const uint8_t *tail, uint64_t tail_len, uint32_t id) {
    if (d->format == LFX_GZIP || d->started || d->has_dict) return LFX_E_ARG;
    d->has_dict = true; d->dict = tail; d->dict_len = tail_len; d->dict_id = id;
    return LFX_OK;
}
template <class D>
uint64_t dec_buffered(D *d) {
    dec_settle(d);      // (a window decoded ahead counts, and its buffer is not read while it grows)
    // (of the history only the member's own bytes: a preset dictionary's tail in front of them is the caller's, not buffered input)
    const uint64_t own_hist = std::min<uint64_t>(d->hist.size(), d->member_out);
    return (uint64_t)(d->in.size() + d->out.size() + own_hist + d->next.out.size());
}

}  // namespace lfx
