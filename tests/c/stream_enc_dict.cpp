// CPU: the stream encoder's state machine (libflate_amd/csrc/lfx_stream_enc.h: no HIP, no context) with a preset dictionary
// (DESIGN.md §25), over a stand-in batch backend and kilobyte-sized batches, as tests/c/stream_enc.cpp runs it without one.
// The stand-in encodes nothing: it answers every batch with 16 bits per block and RECORDS what it was handed — the `primed`
// flag, which chunks carry CH_DICT, the blocks — at launch and once more at collect, where the product's backend may run the
// batch it kept a second time (with_match_fallback).  What is checked: the header bytes (FDICT, FCHECK, DICTID) for every
// FLEVEL; that exactly one batch of a stream carries the primed chunk, and that it is the stream's first chunk, whatever the
// schedule; that a batch run again still carries it; that an encoder without a dictionary makes the call sequence and the
// records it made before the dictionary existed; that the codes mode writes the FDICT header and primes nothing.
// Built two ways: plain, and -fsanitize=address,undefined.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>

#include "../../libflate_amd/csrc/lfx_stream_enc.h"

using namespace lfx;
typedef std::vector<uint8_t> Bytes;

static int g_checks = 0, g_cases = 0;
static std::string g_case;
[[noreturn]] static void fail(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    printf("FAIL [%s]: ", g_case.c_str());
    vprintf(fmt, ap);
    printf("\n");
    va_end(ap);
    exit(1);
}
#define CHECK(cond, ...) do { g_checks++; if (!(cond)) fail(__VA_ARGS__); } while (0)

// one run of a batch as the backend saw it
struct Run {
    bool primed;
    size_t n_chunks, n_blocks, flagged;       // flagged: chunks with CH_DICT
    bool first_flagged;                       // ... and whether chunk 0 is one of them
    uint64_t first_len, first_off, n;
    bool coded;
    bool operator==(const Run &o) const {
        return primed == o.primed && n_chunks == o.n_chunks && n_blocks == o.n_blocks && flagged == o.flagged &&
               first_flagged == o.first_flagged && first_len == o.first_len && first_off == o.first_off && n == o.n && coded == o.coded;
    }
};
static Run observe(const EncBatch &b) {
    Run r{b.primed, b.plan.chunks.size(), b.plan.blocks.size(), 0, false, 0, 0, b.n, b.coded};
    for (const ChunkDesc &c : b.plan.chunks) r.flagged += (c.flags & CH_DICT) ? 1 : 0;
    if (!b.plan.chunks.empty()) {
        r.first_flagged = (b.plan.chunks[0].flags & CH_DICT) != 0;
        r.first_len = b.plan.chunks[0].len;
        r.first_off = b.plan.chunks[0].in_off;
    }
    return r;
}

// L launch, C collect, B bytes, S sink, F flush callback, X settle
struct Shared {
    std::string log;
    Bytes got;
    std::vector<Run> launched, rerun;
};
struct Fake {
    Shared *sh = nullptr;
    bool in_flight = false;
    EncBatch cur;                                 // (kept, as the product's backend keeps it)
    Bytes out;
    uint64_t whole = 0;
    int launch(EncBatch &b, std::string &) {
        sh->log += 'L';
        CHECK(!in_flight, "a batch is launched while another is in flight");
        CHECK(!b.plan.blocks.empty(), "a batch without a block");
        cur = std::move(b);
        in_flight = true;
        sh->launched.push_back(observe(cur));
        return LFX_OK;
    }
    int collect(EncDone &done, std::string &) {
        sh->log += 'C';
        CHECK(in_flight, "collect without a batch in flight");
        in_flight = false;
        sh->rerun.push_back(observe(cur));        // the batch run again from what was kept
        done.end_bit = cur.carry_bits + 16 * (uint64_t)cur.plan.blocks.size();
        done.adler32 = 1;
        whole = whole_bytes(done.end_bit, cur.final);
        out.assign(whole + 1, (uint8_t)(0xB0 + sh->launched.size()));
        done.shared = 0;
        return LFX_OK;
    }
    int bytes(uint64_t want, const uint8_t **p) {
        sh->log += 'B';
        CHECK(want == whole, "bytes(%llu) of a batch with %llu whole bytes", (unsigned long long)want, (unsigned long long)whole);
        *p = out.data();
        return LFX_OK;
    }
    void settle() { sh->log += 'X'; in_flight = false; }
    Bytes take_out() { return std::move(out); }
};
typedef StreamEnc<Bytes, Fake> Enc;

static int64_t sink_cb(void *user, const uint8_t *p, size_t n) {
    Shared *sh = (Shared *)user;
    sh->log += 'S';
    sh->got.insert(sh->got.end(), p, p + n);
    return (int64_t)n;
}
static int flush_cb(void *user) { ((Shared *)user)->log += 'F'; return 0; }

// the dictionary of a case: 0 none (set_dict never called), 1 a NULL dictionary set, 2 one with bytes to offer, 3 an empty one
enum { D_NONE, D_NULL, D_USABLE, D_EMPTY };
static const int THE_DICT = 0;                       // (opaque to the state machine: only its address matters)
static const uint32_t THE_ID = 0x12345678u;

static lfx_encode_opts small_opts() {
    lfx_encode_opts o;
    encode_opts_default(&o);
    o.block_size = 1000;
    return o;
}
static Enc *make_enc(int format, const lfx_encode_opts &o, int dict, Shared &sh) {
    EncodeSpec sp;
    CHECK(encode_spec(format, &o, &sp) == LFX_OK, "options");
    Enc *e = new Enc(format, sp);
    e->backend.sh = &sh;
    e->pol.batch_bytes = 3000; e->pol.batch_codes = 2500; e->pol.raw_blocks = 3;
    e->w = sink_cb; e->f = flush_cb; e->user = &sh;
    if (dict == D_NULL) e->set_dict(nullptr, 1, false);
    if (dict == D_USABLE) e->set_dict(&THE_DICT, THE_ID, true);
    if (dict == D_EMPTY) e->set_dict(&THE_DICT, 1, false);
    sh.log += '|';
    CHECK(enc_open(e) == LFX_OK, "enc_open");
    sh.log += '|';
    return e;
}
static void free_enc(Enc *e) { enc_close(e, [](Bytes &&v) { Bytes gone(std::move(v)); }); }

enum OpKind { OP_WRITE, OP_FLUSH, OP_FINISH };
struct Op { OpKind kind; size_t n; };
static Shared run_ops(int format, const lfx_encode_opts &o, int dict, const std::vector<Op> &ops, uint64_t batch_bytes = 3000) {
    Shared sh;
    Enc *e = make_enc(format, o, dict, sh);
    e->pol.batch_bytes = batch_bytes;
    size_t most = 0;
    for (const Op &op : ops) most = std::max(most, op.n);
    const Bytes zeros(most + 1, 'z');
    for (const Op &op : ops) {
        if (op.kind == OP_WRITE) CHECK(enc_write(e, zeros.data(), op.n) == (int64_t)op.n, "write: %s", e->err.c_str());
        else if (op.kind == OP_FLUSH) CHECK(enc_flush(e) == LFX_OK, "flush: %s", e->err.c_str());
        else CHECK(enc_finish(e) == LFX_OK, "finish: %s", e->err.c_str());
        sh.log += '|';
    }
    free_enc(e);
    CHECK(sh.launched.size() == sh.rerun.size(), "every launched batch was collected");
    return sh;
}

// ---- the header: FDICT, FCHECK, DICTID for every FLEVEL the options can produce
static void test_header() {
    g_case = "header";
    struct { const char *what; int kind; int no_compression; int level; uint8_t cmf, flg; } rows[] = {
        {"default parse: Balance", LFX_LZ77_DEFAULT, 0, 0, 0x78, 0xBB},
        {"stored blocks: None", LFX_LZ77_DEFAULT, 1, 0, 0x78, 0x20},
        {"literals only: None", LFX_LZ77_NOCOMPRESSION, 0, 0, 0x78, 0x20},
        {"a caller's Fast", LFX_LZ77_DEFAULT, 0, 1 + LFX_LEVEL_FAST, 0x78, 0x7D},
        {"a caller's Best", LFX_LZ77_DEFAULT, 0, 1 + LFX_LEVEL_BEST, 0x78, 0xF9},
        {"chain 8: Best", LFX_LZ77_CHAIN_DEPTH(8), 0, 0, 0x78, 0xF9},
        {"lazy 8: Best", LFX_LZ77_LAZY_DEPTH(8), 0, 0, 0x78, 0xF9},
        {"level 1: Fast", LFX_LZ77_LEVEL_N(1), 0, 0, 0x78, 0x7D},
        {"level 3: Fast", LFX_LZ77_LEVEL_N(3), 0, 0, 0x78, 0x7D},
        {"level 4: Balance", LFX_LZ77_LEVEL_N(4), 0, 0, 0x78, 0xBB},
        {"level 6: Balance", LFX_LZ77_LEVEL_N(6), 0, 0, 0x78, 0xBB},
        {"level 7: Best", LFX_LZ77_LEVEL_N(7), 0, 0, 0x78, 0xF9},
        {"level 9: Best", LFX_LZ77_LEVEL_N(9), 0, 0, 0x78, 0xF9},
    };
    for (const auto &r : rows) {
        g_cases++;
        lfx_encode_opts o = small_opts();
        o.lz77_kind = r.kind;
        o.no_compression = r.no_compression;
        o.lz77_level = (uint8_t)r.level;
        Shared plain, with;
        free_enc(make_enc(LFX_ZLIB, o, D_NONE, plain));
        free_enc(make_enc(LFX_ZLIB, o, D_USABLE, with));
        const uint8_t want[6] = {r.cmf, r.flg, 0x12, 0x34, 0x56, 0x78};
        CHECK(with.got.size() == 6 && memcmp(with.got.data(), want, 6) == 0, "%s: header %02x %02x ... (%zu bytes)", r.what,
              with.got.empty() ? 0 : with.got[0], with.got.size() < 2 ? 0 : with.got[1], with.got.size());
        CHECK(plain.got.size() == 2 && plain.got[0] == with.got[0] && (plain.got[1] & 0xC0) == (with.got[1] & 0xC0) && !(plain.got[1] & 0x20),
              "%s: CMF and FLEVEL are the dictionary-less header's", r.what);
        CHECK(with.log == "|S|X" && plain.log == "|S|X", "%s: the header goes out in one sink call at construction: %s", r.what, with.log.c_str());
    }
    // other windows: FCHECK recomputed over the dictionary-less CMF / FLEVEL; an empty dictionary: its id is 1
    for (uint32_t window : {256u, 300u, 4096u, 32768u}) {
        g_cases++;
        lfx_encode_opts o = small_opts();
        o.window_size = window;
        Shared plain, with;
        free_enc(make_enc(LFX_ZLIB, o, D_NONE, plain));
        free_enc(make_enc(LFX_ZLIB, o, D_EMPTY, with));
        CHECK(with.got.size() == 6 && plain.got.size() == 2, "window %u: sizes", window);
        CHECK(with.got[0] == plain.got[0] && (with.got[1] & 0xE0) == ((plain.got[1] & 0xC0) | 0x20) && (((unsigned)with.got[0] << 8) + with.got[1]) % 31 == 0,
              "window %u: %02x %02x", window, with.got[0], with.got[1]);
        CHECK(with.got[2] == 0 && with.got[3] == 0 && with.got[4] == 0 && with.got[5] == 1, "window %u: DICTID of the empty dictionary", window);
    }
    // raw DEFLATE: nothing
    Shared raw;
    free_enc(make_enc(LFX_DEFLATE, small_opts(), D_USABLE, raw));
    CHECK(raw.got.empty() && raw.log == "||X", "raw DEFLATE writes no header: %s", raw.log.c_str());
}

// exactly one batch carries the primed chunk: batch `at`, its chunk 0 alone, which is the stream's first chunk (offset 0,
// `first_len` bytes) — at launch and when the batch is run again
static void expect_one_primed(const char *name, const Shared &sh, size_t at, uint64_t first_len, size_t min_batches) {
    g_case = name;
    g_cases++;
    CHECK(sh.launched.size() >= min_batches && at < sh.launched.size(), "%zu batches", sh.launched.size());
    for (size_t i = 0; i < sh.launched.size(); i++) {
        const Run &r = sh.launched[i];
        CHECK(r == sh.rerun[i], "batch %zu: run again, it is not the batch that was launched (primed %d then %d, CH_DICT chunks %zu then %zu)", i,
              r.primed, sh.rerun[i].primed, r.flagged, sh.rerun[i].flagged);
        if (i == at) {
            CHECK(r.primed && r.flagged == 1 && r.first_flagged, "batch %zu carries the primed chunk: primed %d, CH_DICT chunks %zu", i, r.primed, r.flagged);
            CHECK(r.first_off == 0 && r.first_len == first_len, "the primed chunk: offset %llu, %llu bytes", (unsigned long long)r.first_off,
                  (unsigned long long)r.first_len);
        } else {
            CHECK(!r.primed && r.flagged == 0, "batch %zu carries no primed chunk: primed %d, CH_DICT chunks %zu", i, r.primed, r.flagged);
        }
    }
}
static void expect_none_primed(const char *name, const Shared &sh, size_t min_batches) {
    g_case = name;
    g_cases++;
    CHECK(sh.launched.size() >= min_batches, "%zu batches", sh.launched.size());
    for (size_t i = 0; i < sh.launched.size(); i++)
        CHECK(!sh.launched[i].primed && sh.launched[i].flagged == 0 && sh.launched[i] == sh.rerun[i], "batch %zu: primed %d, CH_DICT chunks %zu", i,
              sh.launched[i].primed, sh.launched[i].flagged);
}
static size_t count(const std::string &s, char c) { return (size_t)std::count(s.begin(), s.end(), c); }

static void test_schedules() {
    const lfx_encode_opts o = small_opts();
    for (int format : {(int)LFX_ZLIB, (int)LFX_DEFLATE}) {
        // the first write larger than a batch: it closes as one block of one chunk and leaves as batch 0; more batches follow
        std::vector<Op> big = {Op{OP_WRITE, 10000}};
        for (int i = 0; i < 12; i++) big.push_back(Op{OP_WRITE, 700});
        big.push_back(Op{OP_FINISH, 0});
        expect_one_primed("first write larger than a batch", run_ops(format, o, D_USABLE, big), 0, 10000, 3);
        // a flush before the first byte: the empty block's empty chunk is the stream's first chunk (the first flush of the
        // Lz77Encode, as in the one-shot call and the model) — batch 0 carries it, and nothing behind it is primed
        std::vector<Op> fl = {Op{OP_FLUSH, 0}};
        for (int i = 0; i < 12; i++) fl.push_back(Op{OP_WRITE, 700});
        fl.push_back(Op{OP_FINISH, 0});
        expect_one_primed("flush before the first byte", run_ops(format, o, D_USABLE, fl), 0, 0, 3);
        // three empty writes cut nothing and launch nothing: the data behind them starts the stream's first chunk
        std::vector<Op> ew = {Op{OP_WRITE, 0}, Op{OP_WRITE, 0}, Op{OP_WRITE, 0}};
        for (int i = 0; i < 12; i++) ew.push_back(Op{OP_WRITE, 700});
        ew.push_back(Op{OP_FINISH, 0});
        const Shared sw = run_ops(format, o, D_USABLE, ew);
        expect_one_primed("three empty writes, then data", sw, 0, 1400, 3);
        CHECK(sw.log.find('L') > sw.log.find("||||"), "the empty writes launch nothing: %s", sw.log.substr(0, 24).c_str());
        // finish with nothing written: one batch, the final empty block; its empty chunk is the first chunk
        const Shared fin = run_ops(format, o, D_USABLE, {Op{OP_FINISH, 0}});
        expect_one_primed("finish with nothing written", fin, 0, 0, 1);
        CHECK(fin.launched.size() == 1, "one batch");
        // a flush after one byte, and in mid-stream
        std::vector<Op> f1 = {Op{OP_WRITE, 1}, Op{OP_FLUSH, 0}, Op{OP_WRITE, 2500}, Op{OP_FLUSH, 0}, Op{OP_WRITE, 2500}, Op{OP_FINISH, 0}};
        expect_one_primed("flush after one byte", run_ops(format, o, D_USABLE, f1), 0, 1, 3);
    }
    // 8 KiB writes over 600 KiB with the default block size: one batch at finish, three chunks, the first alone primed
    {
        lfx_encode_opts d;
        encode_opts_default(&d);
        std::vector<Op> ops(75, Op{OP_WRITE, 8192});
        ops.push_back(Op{OP_FINISH, 0});
        const Shared sh = run_ops(LFX_ZLIB, d, D_USABLE, ops, 8ull << 20);
        expect_one_primed("600 KiB in 8 KiB writes", sh, 0, 262144, 1);
        CHECK(sh.launched.size() == 1 && sh.launched[0].n_chunks == 3 && sh.launched[0].n_blocks == 1, "three chunks in one block");
    }
    // zlib sync: the marker blocks have no chunk, the first chunk is still batch 0's
    {
        lfx_encode_opts z = small_opts();
        z.zlib_flush_mode = LFX_FLUSH_SYNC;
        expect_one_primed("zlib sync flush before the first byte",
                          run_ops(LFX_ZLIB, z, D_USABLE, {Op{OP_FLUSH, 0}, Op{OP_WRITE, 5000}, Op{OP_FLUSH, 0}, Op{OP_WRITE, 100}, Op{OP_FINISH, 0}}), 0, 0, 3);
    }
    // nothing to prime: stored blocks (no chunk at all), literal-only chunks, an empty dictionary
    std::vector<Op> plain_ops = {Op{OP_WRITE, 10000}, Op{OP_FLUSH, 0}, Op{OP_WRITE, 4000}, Op{OP_FINISH, 0}};
    lfx_encode_opts raw = small_opts();
    raw.no_compression = 1;
    expect_none_primed("stored blocks", run_ops(LFX_ZLIB, raw, D_USABLE, plain_ops), 3);
    lfx_encode_opts lit = small_opts();
    lit.lz77_kind = LFX_LZ77_NOCOMPRESSION;
    expect_none_primed("literal-only chunks", run_ops(LFX_ZLIB, lit, D_USABLE, plain_ops), 3);
    expect_none_primed("an empty dictionary", run_ops(LFX_ZLIB, o, D_EMPTY, plain_ops), 3);
}

// dict == NULL: the call sequence, the records and the bytes of an encoder that was never given one; and a dictionary changes
// nothing but the header, the flag and the mark
static void test_null_dictionary() {
    const lfx_encode_opts o = small_opts();
    std::vector<Op> ops = {Op{OP_FLUSH, 0}, Op{OP_WRITE, 0}, Op{OP_WRITE, 10000}};
    for (int i = 0; i < 9; i++) ops.push_back(Op{OP_WRITE, 777});
    ops.insert(ops.begin() + 6, Op{OP_FLUSH, 0});
    ops.push_back(Op{OP_FINISH, 0});
    for (int format : {(int)LFX_ZLIB, (int)LFX_DEFLATE}) {
        g_case = "dict == NULL";
        g_cases++;
        const Shared none = run_ops(format, o, D_NONE, ops), null = run_ops(format, o, D_NULL, ops), with = run_ops(format, o, D_USABLE, ops);
        CHECK(none.log == null.log, "the call sequence:\n%s\n%s", none.log.c_str(), null.log.c_str());
        CHECK(none.got == null.got, "the bytes the sink received");
        CHECK(none.launched == null.launched && none.rerun == null.rerun, "the batches");
        expect_none_primed("dict == NULL: nothing primed", null, 4);
        g_case = "a dictionary changes the header and the mark alone";
        CHECK(count(with.log, 'L') == count(none.log, 'L') && count(with.log, 'C') == count(none.log, 'C') && count(with.log, 'B') == count(none.log, 'B') &&
              count(with.log, 'F') == count(none.log, 'F'), "backend calls:\n%s\n%s", none.log.c_str(), with.log.c_str());
        const size_t hdr = format == LFX_ZLIB ? 2 : 0;
        CHECK(with.got.size() == none.got.size() + (format == LFX_ZLIB ? 4 : 0) &&
              std::equal(none.got.begin() + (std::ptrdiff_t)hdr, none.got.end(), with.got.begin() + (std::ptrdiff_t)(hdr ? 6 : 0)), "the bytes behind the header");
        CHECK(with.launched.size() == none.launched.size(), "batches");
        for (size_t i = 0; i < with.launched.size(); i++) {
            Run a = with.launched[i];
            a.primed = false; a.flagged = 0; a.first_flagged = false;
            CHECK(a == none.launched[i], "batch %zu differs in more than the mark", i);
        }
    }
}

// codes mode on an encoder made with a dictionary: the FDICT header, and nothing is primed — the caller's Lz77Encode did its own
static void test_codes_mode() {
    g_case = "codes mode";
    g_cases++;
    lfx_encode_opts o = small_opts();
    Shared sh;
    Enc *e = make_enc(LFX_ZLIB, o, D_USABLE, sh);
    CHECK(sh.got.size() == 6 && (sh.got[1] & 0x20) && sh.got[2] == 0x12 && sh.got[5] == 0x78, "the header carries FDICT and DICTID");
    // (a Pointer of the first block that reaches in front of byte 0: the codes mode checks no distance against the position)
    const uint32_t words[3] = {20u << 16 | 300u, (uint32_t)'a' << 16, 3u << 16 | 1u};
    const Bytes raw(24, 'a');
    for (int blk = 0; blk < 6; blk++) {
        std::vector<uint32_t> many(600, (uint32_t)'b' << 16);
        CHECK(enc_write_codes(e, blk ? many.data() : words, blk ? many.size() : 3, raw.data(), raw.size(), 0) == LFX_OK, "write_codes: %s", e->err.c_str());
        CHECK(enc_write_codes(e, nullptr, 0, nullptr, 0, blk == 5 ? 2 : 1) == LFX_OK, "close: %s", e->err.c_str());
        if (blk == 2) CHECK(enc_flush(e) == LFX_OK, "flush");
    }
    CHECK(enc_finish(e) == LFX_OK, "finish: %s", e->err.c_str());
    CHECK(!e->first_chunk_handed, "the codes mode hands no chunk of the planner's to a batch");
    free_enc(e);
    CHECK(sh.launched.size() >= 2, "%zu batches", sh.launched.size());
    for (size_t i = 0; i < sh.launched.size(); i++)
        CHECK(sh.launched[i].coded && !sh.launched[i].primed && sh.launched[i].flagged == 0 && sh.launched[i] == sh.rerun[i], "batch %zu of the codes mode", i);
    CHECK(sh.got.size() > 10, "body and trailer");
}

int main() {
    test_header();
    test_schedules();
    test_null_dictionary();
    test_codes_mode();
    printf("stream_enc_dict ok: %d cases, %d checks\n", g_cases, g_checks);
    return 0;
}
