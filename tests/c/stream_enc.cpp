// CPU: the stream encoder's state machine (libflate_amd/csrc/lfx_stream_enc.h: no HIP, no context) over a stand-in batch
// backend and kilobyte-sized batches.  The stand-in needs no DEFLATE encoder: the oracle's encoder is driven with the same call
// sequence, lfo_scan_blocks gives every block's bit range, and a launched batch of k blocks is answered with the oracle's bits of
// the next k blocks behind the carried bits.  It checks what it is handed — the input bytes (read at COLLECT time: a buffer
// touched while the batch is in flight is caught), the carry byte, the plan's block types and final flags — and returns the
// checksums of its own n bytes.  What is checked around it: the bytes the sink receives against the oracle's output, the order
// of collect / launch / bytes / sink / flush per call, the bound on what is buffered, failures and their order, the codes mode.
// Built two ways: plain (the pytest run) and -fsanitize=address,undefined.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <regex>

#include "../../libflate_amd/csrc/lfx_container.h"
#include "../../libflate_amd/csrc/lfx_stream_enc.h"
#include "../../oracle/lfo.h"

using namespace lfx;
typedef std::vector<uint8_t> Bytes;

static int g_checks = 0, g_cases = 0, g_batches = 0;
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

static Bytes make_plain(size_t n, int kind, uint32_t seed) {
    std::mt19937 rng(seed);
    Bytes v(n);
    if (kind == 0) {                      // text-like
        static const char *words[] = {"batch ", "block ", "the ", "encoder ", "of ", "carry ", "trailer\n", "a ", "stream ", "writes "};
        size_t at = 0;
        while (at < n) {
            const char *w = rng() % 7 ? words[rng() % 10] : "x";
            for (; *w && at < n; w++) v[at++] = (uint8_t)(rng() % 29 ? *w : 'a' + rng() % 26);
        }
    } else if (kind == 1) {               // incompressible
        for (auto &b : v) b = (uint8_t)rng();
    } else {                              // long runs: few code words for many bytes
        for (size_t i = 0; i < n; i++) v[i] = (uint8_t)('a' + (i / 700) % 3);
    }
    return v;
}

// ---- a caller's own Lz77Encode for the codes mode: buffers, and on flush emits literals and (distance 1) runs
struct RunLz {
    Bytes buf;
    std::vector<uint32_t> out;
    size_t encode(const uint8_t *p, size_t n) { buf.insert(buf.end(), p, p + n); out.clear(); return 0; }
    size_t flush() {
        out.clear();
        for (size_t i = 0; i < buf.size();) {
            size_t run = 0;
            if (i) while (i + run < buf.size() && run < 258 && buf[i + run] == buf[i - 1]) run++;
            if (run >= 3) { out.push_back((uint32_t)run << 16 | 1u); i += run; }
            else out.push_back((uint32_t)buf[i++] << 16);
        }
        buf.clear();
        return out.size();
    }
    static size_t cb(void *user, const uint8_t *p, size_t n, const uint32_t **codes) {
        RunLz *z = (RunLz *)user;
        const size_t k = p ? z->encode(p, n) : z->flush();
        *codes = z->out.data();
        return k;
    }
};

// ---- a case: options, a policy, and the calls
enum OpKind { OP_WRITE, OP_FLUSH, OP_FINISH };
struct Op { OpKind kind; size_t n; };
struct Case {
    int format = LFX_GZIP;
    Bytes plain;
    size_t block_size = 1000;
    bool dynamic = true, no_compression = false, zsync = false, codes = false;
    BatchPolicy pol;
    std::vector<Op> ops;
    Case() { pol.batch_bytes = 3000; pol.batch_codes = 2500; pol.raw_blocks = 3; }
};
static std::vector<Op> writes_of(size_t total, size_t w, bool finish = true) {
    std::vector<Op> ops;
    if (w == 0) ops.push_back(Op{OP_WRITE, total});
    else for (size_t at = 0; at < total; at += w) ops.push_back(Op{OP_WRITE, std::min(w, total - at)});
    if (finish) ops.push_back(Op{OP_FINISH, 0});
    return ops;
}

// what the oracle made of the case
struct Truth {
    Bytes z;                                   // the whole output
    uint64_t defl = 0;                         // first DEFLATE byte
    std::vector<lfo_blockinfo> blk;            // bit ranges relative to z[defl]
    std::vector<uint64_t> out_at;              // plain bytes in front of block j (one more entry: the total)
};
static Truth oracle_run(const Case &cs) {
    lfo_opts o;
    lfo_opts_default(&o);
    o.block_size = cs.block_size;
    o.dynamic_huffman = cs.dynamic;
    o.no_compression = cs.no_compression;
    o.zlib_sync_flush = cs.zsync;
    RunLz lz;
    if (cs.codes) { o.lz77_kind = LFO_LZ77_CUSTOM; o.custom_cb = RunLz::cb; o.custom_user = &lz; o.custom_level = LFO_LEVEL_BALANCE; }
    lfo_encoder *e = lfo_encoder_new(cs.format, &o);
    size_t at = 0;
    for (const Op &op : cs.ops) {
        if (op.kind == OP_WRITE) { lfo_encoder_write(e, cs.plain.data() + at, op.n); at += op.n; }
        else if (op.kind == OP_FLUSH) lfo_encoder_flush(e);
    }
    size_t len = 0;
    const uint8_t *p = lfo_encoder_finish(e, &len);
    Truth t;
    t.z.assign(p, p + len);
    lfo_encoder_free(e);
    const DecHeader h = parse_container(cs.format, t.z.data(), t.z.size(), nullptr);
    if (h.status) fail("the oracle's header does not parse");
    t.defl = h.deflate_off;
    t.blk.resize(8192);
    const long nb = lfo_scan_blocks(t.z.data() + t.defl, t.z.size() - t.defl, t.blk.data(), t.blk.size());
    if (nb <= 0 || nb > 8192) fail("lfo_scan_blocks: %ld", nb);
    t.blk.resize((size_t)nb);
    uint64_t out = 0;
    for (size_t j = 0; j < t.blk.size(); j++) {
        if (j && t.blk[j].start_bit != t.blk[j - 1].end_bit) fail("blocks do not tile the stream");
        t.out_at.push_back(out);
        out += t.blk[j].out_len;
    }
    t.out_at.push_back(out);
    if (out != at) fail("the oracle's blocks hold %llu bytes, the case wrote %zu", (unsigned long long)out, at);
    return t;
}

// ---- the stand-in backend, the sink and the flush callback; all of a run's events in one log:
// L launch, C collect, B bytes, S sink, F flush callback, X settle
struct Shared {
    const Truth *t = nullptr;
    const Bytes *plain = nullptr;
    std::string log;
    Bytes got;
    size_t next_block = 0;
    int sink_calls = 0, launches = 0, collects = 0;
    int sink_fail_at = -1, launch_fail_at = -1, collect_fail_at = -1, nospace_at = -1;
    bool flush_fails = false;
    bool given_after_settle = true;
};
struct Fake {
    Shared *sh = nullptr;
    bool in_flight = false, have_bytes = false;
    EncBatch cur;
    size_t first = 0;
    Bytes out;
    uint64_t whole = 0;
    int launch(EncBatch &b, std::string &err) {
        sh->log += 'L';
        CHECK(!in_flight, "a batch is launched while another is in flight");
        if (sh->launches++ == sh->launch_fail_at) { err = "stand-in: launch failed"; return LFX_E_DEVICE; }
        cur = std::move(b);
        in_flight = true;
        g_batches++;
        const Truth &t = *sh->t;
        first = sh->next_block;
        const size_t k = cur.plan.blocks.size();
        CHECK(k > 0 && first + k <= t.blk.size(), "batch of %zu blocks at block %zu of %zu", k, first, t.blk.size());
        for (size_t j = 0; j < k; j++) {
            CHECK(cur.plan.blocks[j].type == t.blk[first + j].btype, "block %zu: type %u, the oracle's %u", first + j, cur.plan.blocks[j].type, t.blk[first + j].btype);
            CHECK(cur.plan.blocks[j].final == t.blk[first + j].bfinal, "block %zu: final flag", first + j);
        }
        CHECK(cur.final == (t.blk[first + k - 1].bfinal != 0), "batch final flag");
        const uint64_t s = t.blk[first].start_bit;
        CHECK(cur.carry_bits == (s & 7), "carry_bits %u, the oracle's stream stands at bit %llu", cur.carry_bits, (unsigned long long)s);
        const uint8_t partial = (s & 7) ? (uint8_t)(t.z[t.defl + s / 8] & ((1u << (s & 7)) - 1)) : 0;
        CHECK(cur.carry == partial, "carry byte %02x, the oracle's partial byte %02x", cur.carry, partial);
        CHECK(cur.n == t.out_at[first + k] - t.out_at[first], "batch of %llu bytes, its blocks hold %llu", (unsigned long long)cur.n,
              (unsigned long long)(t.out_at[first + k] - t.out_at[first]));
        if (cur.coded) {
            uint64_t sum = 0;
            for (size_t j = 0; j < cur.plan.chunks.size(); j++) {
                sum += cur.chunk_codes[j];
                CHECK(cur.codes[sum - 1] == CODE_EOB, "chunk %zu does not end with EndOfBlock", j);
            }
            CHECK(sum == cur.n_codes && sum == cur.plan.n_codes_cap, "code words of the chunks");
        }
        const uint64_t cap = cur.coded ? codes_bound(cur.n_codes, k) : bytes_bound(cur.n, k);
        CHECK(cur.bound == cap, "output bound");
        sh->next_block = first + k;
        return LFX_OK;
    }
    int collect(EncDone &done, std::string &err) {
        sh->log += 'C';
        CHECK(in_flight, "collect without a batch in flight");
        in_flight = false;
        const int idx = sh->collects++;
        if (idx == sh->collect_fail_at) { err = "stand-in: collect failed"; return LFX_E_DEVICE; }
        if (idx == sh->nospace_at) { done.status = 1; return LFX_OK; }
        const Truth &t = *sh->t;
        const size_t k = cur.plan.blocks.size();
        // the input, read NOW: it must still be the plain text of exactly these blocks
        CHECK(cur.n == 0 || memcmp(cur.in, sh->plain->data() + t.out_at[first], cur.n) == 0, "the batch's input changed while it was in flight");
        done.crc32 = lfo_crc32(0, cur.in, cur.n);
        done.adler32 = lfo_adler32(1, cur.in, cur.n);
        const uint64_t s = t.blk[first].start_bit - cur.carry_bits, e = t.blk[first + k - 1].end_bit;
        done.end_bit = e - s;
        out.assign(t.z.begin() + (std::ptrdiff_t)(t.defl + s / 8), t.z.begin() + (std::ptrdiff_t)(t.defl + (e + 7) / 8));
        if (e & 7) out.back() &= (uint8_t)((1u << (e & 7)) - 1);     // (the bits behind are the next batch's)
        whole = whole_bytes(done.end_bit, cur.final);
        done.shared = whole < out.size() ? out[whole] : 0;
        out.resize(whole + 1);
        have_bytes = true;
        return LFX_OK;
    }
    int bytes(uint64_t want, const uint8_t **p) {
        sh->log += 'B';
        CHECK(have_bytes, "bytes() without a collected batch");
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
    if (sh->sink_calls++ == sh->sink_fail_at) return -1;
    CHECK(sh->sink_fail_at < 0 || sh->sink_calls - 1 < sh->sink_fail_at, "a sink call after the one that failed");
    sh->got.insert(sh->got.end(), p, p + n);
    return (int64_t)n;
}
static int flush_cb(void *user) {
    Shared *sh = (Shared *)user;
    sh->log += 'F';
    return sh->flush_fails ? 1 : 0;
}

static Enc *make_enc(const Case &cs, Shared &sh, int *status) {
    lfx_encode_opts o;
    encode_opts_default(&o);
    o.block_size = cs.block_size;
    o.dynamic_huffman = cs.dynamic;
    o.no_compression = cs.no_compression;
    o.zlib_flush_mode = cs.zsync ? LFX_FLUSH_SYNC : 0;
    EncodeSpec sp;
    if ((*status = encode_spec(cs.format, &o, &sp))) return nullptr;
    Enc *e = new Enc(cs.format, sp);
    e->backend.sh = &sh;
    e->pol = cs.pol;
    e->w = sink_cb; e->f = flush_cb; e->user = &sh;
    sh.log += '|';
    if ((*status = enc_open(e))) { enc_close(e, [](Bytes &&) {}); return nullptr; }
    sh.log += '|';
    return e;
}
static void free_enc(Enc *e, Shared &sh) {
    sh.log += '|';
    enc_close(e, [&sh](Bytes &&v) { if (sh.log.back() != 'X') sh.given_after_settle = false; Bytes gone(std::move(v)); });
    CHECK(sh.given_after_settle, "an input buffer was given back before the backend settled");
}

// the bound on what is buffered, from enc_write / enc_run: a write returns with the closed blocks below a batch (at or above,
// it launched ALL of them), and the open block holds less than block_size bytes (Planner: a block closes at block_size)
static void check_buffered(const Enc *e, const Case &cs) {
    const uint64_t bs = cs.no_compression ? std::min<uint64_t>(cs.block_size, 0xFFFF) : cs.block_size;
    CHECK(e->pl.closed_bytes() < cs.pol.batch_bytes, "closed bytes %llu waiting", (unsigned long long)e->pl.closed_bytes());
    if (cs.no_compression) CHECK(e->pl.closed_blocks() < cs.pol.raw_blocks, "closed stored blocks %zu waiting", e->pl.closed_blocks());
    uint64_t closed_max = cs.pol.batch_bytes - 1;
    if (cs.no_compression) closed_max = std::min<uint64_t>(closed_max, (cs.pol.raw_blocks - 1) * bs);
    CHECK(e->pending.size() <= closed_max + bs - 1, "pending holds %zu bytes", e->pending.size());
    CHECK(e->pending.size() == e->pl.cursor(), "pending and the planner disagree");
}

// one call of the codes-mode driver: what a caller with its own Lz77Encode does around write_codes (the reference's
// Block::write / CompressBuf, encode.rs:277-286,405-425)
struct CodesDriver {
    RunLz lz;
    uint64_t original = 0;
    int close(Enc *e, int end_block) {
        const size_t k = lz.flush();
        original = 0;
        return enc_write_codes(e, lz.out.data(), k, nullptr, 0, end_block);
    }
    int write(Enc *e, const uint8_t *p, size_t n, size_t block_size) {
        const size_t k = lz.encode(p, n);
        if (int rc = enc_write_codes(e, lz.out.data(), k, p, n, 0)) return rc;
        original += n;
        while (original >= block_size)
            if (int rc = close(e, 1)) return rc;
        return LFX_OK;
    }
};

// the backend calls one API call may make: only stored-block writes, flush and finish drain; a batch is collected before the
// next is launched, and its bytes reach the sink after that launch
static const std::regex &call_pattern(const Case &cs, OpKind kind) {
    static const std::regex codes_write("(LCBS?)*"), codes_flush("(LCBS?)*F"), codes_finish("(LCBS?)?S?F"), raw_write("|LCBS?"),
        write("|L|CLBS?"), flush("(LCBS?|CLBS?CBS?)F"), finish("(LCBS?|CLBS?CBS?)S?F");
    if (cs.codes) return kind == OP_WRITE ? codes_write : kind == OP_FLUSH ? codes_flush : codes_finish;
    if (kind == OP_WRITE) return cs.no_compression ? raw_write : write;
    return kind == OP_FLUSH ? flush : finish;
}

// the whole case against the oracle: bytes, call order, what is buffered.  → the log of the run
static std::string run_case(const char *name, const Case &cs) {
    g_case = name;
    g_cases++;
    const Truth t = oracle_run(cs);
    Shared sh;
    sh.t = &t; sh.plain = &cs.plain;
    int st = 0;
    Enc *e = make_enc(cs, sh, &st);
    CHECK(e && st == LFX_OK, "encoder: status %d", st);
    CHECK(sh.got.size() == t.defl && std::equal(sh.got.begin(), sh.got.end(), t.z.begin()), "the header goes out at construction");
    CodesDriver drv;
    size_t at = 0;
    for (const Op &op : cs.ops) {
        const size_t mark = sh.log.size();
        if (op.kind == OP_WRITE) {
            if (cs.codes) CHECK(drv.write(e, cs.plain.data() + at, op.n, cs.block_size) == LFX_OK, "write_codes: %s", e->err.c_str());
            else {
                CHECK(enc_write(e, cs.plain.data() + at, op.n) == (int64_t)op.n, "write: %s", e->err.c_str());
                check_buffered(e, cs);
            }
            at += op.n;
        } else if (op.kind == OP_FLUSH) {
            if (cs.codes) CHECK(drv.close(e, 1) == LFX_OK, "close for flush: %s", e->err.c_str());
            CHECK(enc_flush(e) == LFX_OK, "flush: %s", e->err.c_str());
            CHECK(!e->inflight && e->pl.closed_blocks() == 0 && e->cblocks.empty(), "flush leaves nothing closed behind");
        } else {
            if (cs.codes) CHECK(drv.close(e, 2) == LFX_OK, "close for finish: %s", e->err.c_str());
            CHECK(enc_finish(e) == LFX_OK, "finish: %s", e->err.c_str());
        }
        const std::string ev = sh.log.substr(mark);
        CHECK(std::regex_match(ev, call_pattern(cs, op.kind)), "call %d made the backend calls '%s'", (int)op.kind, ev.c_str());
        sh.log += '|';
    }
    CHECK(sh.got == t.z, "the sink received %zu bytes, the oracle wrote %zu (first difference at %zu)", sh.got.size(), t.z.size(),
          (size_t)(std::mismatch(sh.got.begin(), sh.got.begin() + (std::ptrdiff_t)std::min(sh.got.size(), t.z.size()), t.z.begin()).first - sh.got.begin()));
    CHECK(sh.next_block == t.blk.size(), "blocks launched");
    CHECK(enc_write(e, cs.plain.data(), 1) == -(int64_t)LFX_E_ARG && enc_flush(e) == LFX_E_ARG && enc_finish(e) == LFX_E_ARG &&
          enc_write_codes(e, nullptr, 0, nullptr, 0, 0) == LFX_E_ARG, "calls after finish");
    const std::string log = sh.log;
    free_enc(e, sh);
    return log;
}

static void test_formats_sizes_schedules() {
    const size_t bs = 1000;
    const size_t sizes[] = {0, 1, bs - 1, bs, 70001};
    const size_t wsizes[] = {1, 7, 8192, 65537, 0};
    for (int format = 0; format < 3; format++)
        for (size_t n : sizes)
            for (size_t w : wsizes) {
                for (int variant = 0; variant < 3; variant++) {            // dynamic, fixed, stored
                    Case cs;
                    cs.format = format;
                    cs.plain = make_plain(n, variant == 2 ? 1 : 0, (uint32_t)(n + w));
                    cs.block_size = variant == 1 ? 4096 : bs;
                    cs.dynamic = variant == 0;
                    cs.no_compression = variant == 2;
                    cs.ops = writes_of(n, w);
                    char name[96];
                    snprintf(name, sizeof name, "format %d n %zu write %zu variant %d", format, n, w, variant);
                    run_case(name, cs);
                }
            }
}

static void test_flush() {
    for (int format = 0; format < 3; format++)
        for (int zs = 0; zs < 2; zs++)
            for (int raw = 0; raw < 2; raw++) {
                if (zs && format != LFX_ZLIB) continue;
                Case cs;
                cs.format = format;
                cs.zsync = zs != 0;
                cs.no_compression = raw != 0;
                cs.plain = make_plain(20000, 0, 5);
                // on an empty encoder, twice in a row, in the middle of a block, right before finish (a final batch of n == 0)
                cs.ops = {Op{OP_FLUSH, 0}, Op{OP_FLUSH, 0}, Op{OP_WRITE, 300}, Op{OP_FLUSH, 0}};
                for (size_t at = 300; at < 20000; at += 1700) {
                    cs.ops.push_back(Op{OP_WRITE, std::min<size_t>(1700, 20000 - at)});
                    if (at % 3 == 0) cs.ops.push_back(Op{OP_FLUSH, 0});
                }
                cs.ops.push_back(Op{OP_FLUSH, 0});
                cs.ops.push_back(Op{OP_FINISH, 0});
                char name[64];
                snprintf(name, sizeof name, "flush format %d sync %d stored %d", format, zs, raw);
                const std::string log = run_case(name, cs);
                CHECK(std::regex_search(log, std::regex("\\|LCBS?F\\|LCBS?F\\|")), "two flushes in a row: %s", log.substr(0, 40).c_str());
            }
    // finish straight after flush: the final batch holds the empty final block alone
    Case cs;
    cs.plain = make_plain(5000, 0, 6);
    cs.ops = {Op{OP_WRITE, 5000}, Op{OP_FLUSH, 0}, Op{OP_FINISH, 0}};
    const Truth t = oracle_run(cs);
    CHECK(t.blk.back().out_len == 0 && t.blk.back().bfinal, "the oracle's last block is the empty final one");
    run_case("finish after flush", cs);
}

// both input buffers are reused: batches follow each other with writes arriving while one is in flight
static void test_ping_pong() {
    Case cs;
    cs.format = LFX_ZLIB;
    cs.plain = make_plain(40000, 0, 9);
    cs.ops = writes_of(40000, 7);
    const std::string log = run_case("ping-pong", cs);
    // (a write that starts a batch collects the one before: "CLB"; between two of them only writes that touch no backend)
    CHECK(std::regex_search(log, std::regex("\\|L\\|(\\|)*CLBS?\\|(\\|)+CLBS?\\|(\\|)+CLBS?\\|(\\|)+CLBS?\\|")), "four consecutive batches, writes in between");
    size_t in_between = 0, pos = log.find("|CLB");
    for (size_t i = pos; i < log.size() && log[i] != 'F'; i++) in_between += log[i] == '|';
    CHECK(in_between > 100, "writes between launch and collect");
}

// ---- failures
struct Outcome { int rc; std::string err; int sink_calls; bool failed, finished; std::string log; };
// runs the case until a call fails; → that call's status.  Then: the failure is sticky
static Outcome run_until_failure(const Case &cs, Shared &sh) {
    const Truth t = oracle_run(cs);
    sh.t = &t; sh.plain = &cs.plain;
    Outcome oc{LFX_OK, "", 0, false, false, ""};
    int st = 0;
    Enc *e = make_enc(cs, sh, &st);
    if (!e) { oc.rc = st; oc.sink_calls = sh.sink_calls; oc.log = sh.log; return oc; }
    size_t at = 0;
    for (const Op &op : cs.ops) {
        int rc;
        sh.log += '|';
        if (op.kind == OP_WRITE) { const int64_t k = enc_write(e, cs.plain.data() + at, op.n); rc = k < 0 ? (int)-k : LFX_OK; at += op.n; }
        else rc = op.kind == OP_FLUSH ? enc_flush(e) : enc_finish(e);
        if (rc) { oc.rc = rc; break; }
    }
    oc.err = e->err; oc.failed = e->failed; oc.finished = e->finished;
    if (oc.rc) {
        const int calls = sh.sink_calls;
        const int after = e->finished ? LFX_E_ARG : LFX_E_IO;      // (a failure inside finish leaves the encoder finished)
        CHECK(e->finished || e->failed, "a failed call sets `failed`");
        CHECK(enc_write(e, cs.plain.data(), 1) == -(int64_t)after && enc_flush(e) == after && enc_finish(e) == after, "the failure is sticky");
        CHECK(sh.sink_calls == calls, "no sink call after a failure");
    }
    oc.sink_calls = sh.sink_calls; oc.log = sh.log;
    free_enc(e, sh);
    return oc;
}
static void test_failures() {
    Case cs;
    cs.plain = make_plain(9000, 0, 11);
    cs.ops = writes_of(9000, 1500, false);
    cs.ops.insert(cs.ops.begin() + 3, Op{OP_FLUSH, 0});
    cs.ops.push_back(Op{OP_FINISH, 0});
    g_case = "failures";
    int total_sinks = 0;
    { Shared sh; const Outcome oc = run_until_failure(cs, sh); CHECK(oc.rc == LFX_OK, "the case itself"); total_sinks = oc.sink_calls; }
    CHECK(total_sinks >= 5, "sink calls of the short stream: %d", total_sinks);
    for (int i = 0; i < total_sinks; i++) {              // the sink fails at its i-th call, for every i
        Shared sh;
        sh.sink_fail_at = i;
        const Outcome oc = run_until_failure(cs, sh);
        CHECK(oc.rc == LFX_E_IO && (i == 0 || oc.err == "write callback failed"), "sink failure %d: status %d '%s'", i, oc.rc, oc.err.c_str());
        CHECK(oc.sink_calls == i + 1, "sink failure %d: %d calls", i, oc.sink_calls);
    }
    for (int in_finish = 0; in_finish < 2; in_finish++) {  // the flush callback fails: in flush, in finish
        Case c2 = cs;
        if (in_finish) c2.ops.erase(c2.ops.begin() + 3);
        Shared sh;
        sh.flush_fails = true;
        const Outcome oc = run_until_failure(c2, sh);
        CHECK(oc.rc == LFX_E_IO && oc.err == "flush callback failed" && oc.finished == (in_finish != 0) && oc.failed == !in_finish, "flush callback failure");
    }
    for (int k = 0; k < 3; k++) {                         // the backend fails at launch k
        Shared sh;
        sh.launch_fail_at = k;
        const Outcome oc = run_until_failure(cs, sh);
        CHECK(oc.rc == LFX_E_DEVICE && oc.err == "stand-in: launch failed", "launch failure %d: %d '%s'", k, oc.rc, oc.err.c_str());
    }
    for (int k = 0; k < 3; k++) {                         // ... at collect k: it surfaces at the call that collects
        Shared sh;
        sh.collect_fail_at = k;
        const Outcome oc = run_until_failure(cs, sh);
        CHECK(oc.rc == LFX_E_DEVICE && oc.err == "stand-in: collect failed", "collect failure %d: %d '%s'", k, oc.rc, oc.err.c_str());
        const std::string last = oc.log.substr(oc.log.rfind('|') + 1);
        CHECK(last == "C" || last == "CLBSC", "the failure surfaces at the call that collects: '%s'", last.c_str());
        if (k == 0) CHECK(oc.log.find("|L|") != std::string::npos, "the write that launched the batch had returned");
    }
    for (int k = 0; k < 3; k++) {                         // a collected status that means no space
        Shared sh;
        sh.nospace_at = k;
        const Outcome oc = run_until_failure(cs, sh);
        CHECK(oc.rc == LFX_E_NOSPACE && oc.err == "output capacity too small", "no space at %d: %d '%s'", k, oc.rc, oc.err.c_str());
    }
    {                                                     // an option outside the domain, a header that cannot be written
        lfx_encode_opts o;
        encode_opts_default(&o);
        o.block_size = 0;
        EncodeSpec sp;
        CHECK(encode_spec(LFX_GZIP, &o, &sp) == LFX_E_ARG, "block_size 0");
        Bytes big(70000, 1);
        encode_opts_default(&o);
        o.extra = big.data(); o.extra_len = 70000;
        Shared sh;
        CHECK(encode_spec(LFX_GZIP, &o, &sp) == LFX_OK, "default options");
        Enc *e = new Enc(LFX_GZIP, sp);
        e->backend.sh = &sh; e->w = sink_cb; e->user = &sh;
        CHECK(enc_open(e) == LFX_E_INVALID_DATA && sh.sink_calls == 0, "an extra field beyond 65535 bytes");
        free_enc(e, sh);
    }
}

// an encoder freed with a batch in flight: the backend settles before the buffers go
static void test_free_in_flight() {
    g_case = "free in flight";
    Case cs;
    cs.plain = make_plain(8000, 0, 13);
    cs.ops = writes_of(8000, 500, false);
    const Truth t = [&] { Case full = cs; full.ops.push_back(Op{OP_FINISH, 0}); return oracle_run(full); }();
    Shared sh;
    sh.t = &t; sh.plain = &cs.plain;
    int st = 0;
    Enc *e = make_enc(cs, sh, &st);
    size_t at = 0;
    for (const Op &op : cs.ops) { CHECK(enc_write(e, cs.plain.data() + at, op.n) == (int64_t)op.n, "write"); at += op.n; }
    CHECK(e->inflight && e->backend.in_flight, "a batch is in flight");
    free_enc(e, sh);
    CHECK(sh.log.back() == 'X', "settle at the end: %s", sh.log.c_str());
}

// ---- codes mode
static void test_codes() {
    for (int format = 0; format < 3; format++)
        for (int kind = 0; kind < 3; kind += 2)           // text (the codes threshold), runs (the raw bytes threshold)
            for (int zs = 0; zs < 2; zs++) {
                if (zs && format != LFX_ZLIB) continue;
                Case cs;
                cs.format = format;
                cs.codes = true;
                cs.zsync = zs != 0;
                cs.dynamic = kind == 0;
                cs.plain = make_plain(30000, kind, 17);
                cs.ops = writes_of(30000, 777, false);
                cs.ops.insert(cs.ops.begin() + 9, Op{OP_FLUSH, 0});
                cs.ops.insert(cs.ops.begin() + 10, Op{OP_FLUSH, 0});
                cs.ops.push_back(Op{OP_FINISH, 0});
                char name[64];
                snprintf(name, sizeof name, "codes format %d kind %d sync %d", format, kind, zs);
                const int before = g_batches;
                run_case(name, cs);
                CHECK(g_batches - before >= 5, "batches of the codes mode: %d", g_batches - before);
            }
    // each threshold alone: the other one far above the input.  Text through RunLz is about a code word per byte, blocks of 1000
    // bytes: batch_codes 2500 cuts a batch at every third block close; the run input (258-byte matches: ~10 code words per block)
    // never reaches a codes threshold, batch_bytes 3000 cuts at every third block close.  With the threshold in question
    // ignored, the whole stream would be ONE batch, at finish.
    for (int by_bytes = 0; by_bytes < 2; by_bytes++) {
        Case cs;
        cs.format = LFX_ZLIB;
        cs.codes = true;
        cs.plain = make_plain(30000, by_bytes ? 2 : 0, 19);
        cs.pol.batch_bytes = by_bytes ? 3000 : 1ull << 40;
        cs.pol.batch_codes = by_bytes ? 1ull << 40 : 2500;
        cs.ops = writes_of(30000, 777);
        const int before = g_batches;
        const std::string log = run_case(by_bytes ? "codes: the bytes threshold alone" : "codes: the codes threshold alone", cs);
        const int batches = g_batches - before;
        // 30 blocks; a batch at every third close (text: 1000 bytes give 1001 code words or fewer, so at the third; runs: 3000 bytes)
        CHECK(batches >= 9 && batches <= 11, "%d batches", batches);
        CHECK(std::regex_search(log, std::regex("\\|LCBS?\\|(\\|)+LCBS?\\|(\\|)+LCBS?\\|")), "batches cut by write_codes calls: %s", log.substr(0, 60).c_str());
    }
    g_case = "codes rules";
    Case cs;
    cs.codes = true;
    cs.plain = make_plain(100, 0, 1);
    cs.ops = {Op{OP_WRITE, 100}, Op{OP_FINISH, 0}};
    const Truth t = oracle_run(cs);
    auto fresh = [&](Shared &sh, bool raw = false) {
        Case c2 = cs;
        c2.no_compression = raw;
        sh.t = &t; sh.plain = &cs.plain;
        int st = 0;
        return make_enc(c2, sh, &st);
    };
    const uint32_t lit = 'a' << 16, bad[] = {256u << 16, 2u << 16 | 1, 259u << 16 | 1, 3u << 16 | 32769u};
    for (uint32_t b : bad) {                               // literal > 255, length < 3 or > 258, distance > 32768
        Shared sh;
        Enc *e = fresh(sh);
        const uint32_t cw[2] = {lit, b};
        CHECK(enc_write_codes(e, cw, 2, nullptr, 0, 0) == LFX_E_ARG && e->err == "code word outside Code's domain" && e->codes.empty(), "domain: %08x", b);
        free_enc(e, sh);
    }
    const uint32_t ok[3] = {lit, 258u << 16 | 32768u, 3u << 16 | 1};
    {
        Shared sh;
        Enc *e = fresh(sh);
        CHECK(enc_write_codes(e, ok, 3, nullptr, 0, 3) == LFX_E_ARG && enc_write_codes(e, ok, 3, nullptr, 0, -1) == LFX_E_ARG, "end_block");
        CHECK(enc_write_codes(e, nullptr, 3, nullptr, 0, 0) == LFX_E_ARG && enc_write_codes(e, ok, 3, nullptr, 5, 0) == LFX_E_ARG, "null with a count");
        CHECK(enc_write_codes(e, ok, 3, cs.plain.data(), 10, 0) == LFX_OK, "codes");
        CHECK(enc_write(e, cs.plain.data(), 1) == -(int64_t)LFX_E_ARG && e->err == "lfx_encoder_write on an encoder that takes code words", "bytes after codes");
        CHECK(enc_flush(e) == LFX_E_ARG && e->err == "close the open block first (end_block = 1)" && !e->failed, "flush with an open block");
        CHECK(enc_finish(e) == LFX_E_ARG && e->err == "close the final block first (end_block = 2)" && !e->finished, "finish without a final block");
        free_enc(e, sh);
    }
    {
        Shared sh;
        Enc *e = fresh(sh);
        CHECK(enc_write(e, cs.plain.data(), 10) == 10, "bytes");
        CHECK(enc_write_codes(e, ok, 3, nullptr, 0, 0) == LFX_E_ARG && e->err == "lfx_encoder_write_codes on an encoder that takes bytes", "codes after bytes");
        free_enc(e, sh);
        Shared sh2;
        e = fresh(sh2, true);
        CHECK(enc_write_codes(e, ok, 3, nullptr, 0, 0) == LFX_E_ARG && e->err == "lfx_encoder_write_codes on an encoder that takes bytes", "codes on stored blocks");
        free_enc(e, sh2);
    }
    // codes_plan directly: chunk, tile and code offsets over random block lists, BT_RAW markers among them
    g_case = "codes_plan";
    std::mt19937 rng(23);
    for (int round = 0; round < 400; round++) {
        std::vector<CodeBlock> cb(rng() % 12);
        for (auto &b : cb) b = rng() % 4 == 0 ? CodeBlock{0, BT_RAW, 0} : CodeBlock{1 + rng() % 9000, rng() % 2 ? (uint32_t)BT_DYNAMIC : (uint32_t)BT_FIXED, 0};
        const bool fin = !cb.empty() && cb.back().type != BT_RAW && rng() % 2;
        if (fin) cb.back().final = 1;
        std::vector<uint32_t> cc;
        const Plan p = codes_plan(cb, fin, cc);
        CHECK(p.blocks.size() == cb.size() && p.chunks.size() == cc.size(), "sizes");
        uint64_t code = 0, tile = 0;
        size_t ch = 0;
        for (size_t j = 0; j < cb.size(); j++) {
            const BlockDesc &b = p.blocks[j];
            CHECK(b.type == cb[j].type && b.final == cb[j].final && b.first_chunk == ch && b.align_after == (fin && j + 1 == cb.size() ? 1u : 0u), "block %zu", j);
            if (cb[j].type == BT_RAW) { CHECK(b.n_chunks == 0, "a marker has no chunk"); continue; }
            const ChunkDesc &c = p.chunks[ch];
            CHECK(b.n_chunks == 1 && c.block == j && c.len + 1 == cb[j].n_codes && c.code_off == code && c.tile_base == tile &&
                  c.flags == CH_LAST_IN_BLOCK && cc[ch] == cb[j].n_codes, "chunk of block %zu", j);
            code += cb[j].n_codes;
            tile += (cb[j].n_codes + PACK_TILE - 1) / PACK_TILE;
            ch++;
        }
        CHECK(p.n_codes_cap == code && p.n_tiles == tile && p.n_segs == 0 && p.n_vis == 0, "totals");
    }
}

// the trailer of an empty stream, ISIZE that wraps, the checksum fold against the checksums of the whole
static void test_trailer_and_fold() {
    g_case = "fold";
    const Bytes a = make_plain(70001, 0, 3);
    for (size_t cut : {(size_t)0, (size_t)1, (size_t)5552, (size_t)65521, (size_t)70001}) {
        CHECK(crc32_combine(lfo_crc32(0, a.data(), cut), lfo_crc32(0, a.data() + cut, a.size() - cut), a.size() - cut) == lfo_crc32(0, a.data(), a.size()), "crc fold at %zu", cut);
        CHECK(adler32_combine(lfo_adler32(1, a.data(), cut), lfo_adler32(1, a.data() + cut, a.size() - cut), a.size() - cut) == lfo_adler32(1, a.data(), a.size()), "adler fold at %zu", cut);
    }
    CHECK(bytes_bound(4096, 3) == 4096 + 1024 + 3072 + 128 && codes_bound(100, 2) == 600 + 2048 + 128, "the output bounds");
    const BatchPolicy def;
    CHECK(def.batch_bytes == (8ull << 20) && def.batch_codes == (2ull << 20) && def.raw_blocks == 1024, "the product's policy");
    // ISIZE wraps: the counter alone (4 GiB of writes are not made here)
    Case cs;
    cs.plain = make_plain(10, 0, 1);
    cs.ops = {Op{OP_WRITE, 10}, Op{OP_FINISH, 0}};
    const Truth t = oracle_run(cs);
    Shared sh;
    sh.t = &t; sh.plain = &cs.plain;
    int st = 0;
    Enc *e = make_enc(cs, sh, &st);
    CHECK(enc_write(e, cs.plain.data(), 10) == 10, "write");
    e->total_in += 1ull << 32;
    CHECK(enc_finish(e) == LFX_OK && sh.got == t.z, "ISIZE is total_in mod 2^32");
    free_enc(e, sh);
}

int main() {
    test_trailer_and_fold();
    test_formats_sizes_schedules();
    test_flush();
    test_ping_pong();
    test_failures();
    test_free_in_flight();
    test_codes();
    printf("stream_enc ok: %d cases, %d batches, %d checks\n", g_cases, g_batches, g_checks);
    return 0;
}
