// CPU: the stream decoder's state machine (libflate_amd/csrc/lfx_stream_dec.h: no HIP, no context) over a stand-in window
// backend and kilobyte-sized windows.  The stand-in knows every member of the input from the oracle — lfo_scan_blocks (the bit
// range, BFINAL and output length of each block) and the plain text it encoded — finds where a window starts from
// in_base * 8 + bit_off and answers as inflate_member (lfx_decode_int.h) is documented to.  What is checked is everything
// around it: readers, reads, window growth, history and checksum carried between windows, trailer, surplus, consumed, the
// order of bytes and errors, the worker thread.  Built three ways: plain (the pytest run), -fsanitize=address,undefined and
// -fsanitize=thread.
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <random>

#include "../../libflate_amd/csrc/lfx_stream_dec.h"
#include "../../oracle/lfo.h"

using namespace lfx;
typedef std::vector<uint8_t> Bytes;

static int g_checks = 0;
static const char *g_case = "";
[[noreturn]] static void fail(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    printf("FAIL [%s]: ", g_case);
    vprintf(fmt, ap);
    printf("\n");
    va_end(ap);
    exit(1);
}
#define CHECK(cond, ...) do { g_checks++; if (!(cond)) fail(__VA_ARGS__); } while (0)

// ---- the folds the state machine links against, from their definitions: CRC(A ++ B) = CRC(A ++ 0^|B|) ^ CRC(0^|B|) ^ CRC(B)
extern "C" uint32_t lfx_crc32_combine(uint32_t crc1, uint32_t crc2, uint64_t len2) {
    static const Bytes zeros(1 << 16, 0);
    uint32_t a = crc1, z = 0;
    for (uint64_t left = len2; left;) {
        const size_t k = (size_t)std::min<uint64_t>(left, zeros.size());
        a = lfo_crc32(a, zeros.data(), k);
        z = lfo_crc32(z, zeros.data(), k);
        left -= k;
    }
    return a ^ z ^ crc2;
}
extern "C" uint32_t lfx_adler32_combine(uint32_t ad1, uint32_t ad2, uint64_t len2) {
    // a = 1 + sum, b = n + sum of prefix sums (mod 65521): the second part's b starts from a1 instead of 1
    const uint64_t M = 65521, a1 = ad1 & 0xFFFF, b1 = ad1 >> 16, a2 = ad2 & 0xFFFF, b2 = ad2 >> 16;
    const uint64_t a = (a1 + a2 + M - 1) % M;
    const uint64_t b = (b1 + b2 + (len2 % M) * ((a1 + M - 1) % M)) % M;
    return (uint32_t)(b << 16 | a);
}

// ---- inputs
static Bytes make_plain(size_t n, int kind, uint32_t seed) {
    std::mt19937 rng(seed);
    Bytes v(n);
    if (kind == 0) {                      // text-like: words of a small vocabulary
        static const char *words[] = {"window ", "block ", "the ", "decoder ", "of ", "history ", "trailer\n", "a ", "stream ", "reads "};
        size_t at = 0;
        while (at < n) {
            const char *w = rng() % 7 ? words[rng() % 10] : "x";
            for (; *w && at < n; w++) v[at++] = (uint8_t)(rng() % 29 ? *w : 'a' + rng() % 26);
        }
    } else if (kind == 1) {               // incompressible
        for (auto &b : v) b = (uint8_t)rng();
    } else {                              // one short period: compresses to almost nothing
        for (size_t i = 0; i < n; i++) v[i] = (uint8_t)("abcdefg"[i % 7]);
    }
    return v;
}

struct Member {
    uint64_t base = 0, defl = 0, end = 0;      // reader offsets: first header byte, first DEFLATE byte, behind the trailer
    std::vector<lfo_blockinfo> blk;
    std::vector<uint64_t> out_at;              // output bytes in front of block j (one more entry: the total)
    Bytes plain;
};
struct Stream {
    int format = 0;
    Bytes z;
    std::vector<Member> members;
    Bytes plain() const { Bytes p; for (auto &m : members) p.insert(p.end(), m.plain.begin(), m.plain.end()); return p; }
};
static void add_member(Stream &s, const Bytes &plain, size_t block_size, size_t write_size) {
    lfo_opts o;
    lfo_opts_default(&o);
    o.block_size = block_size;
    lfo_buf b = {0, 0, 0};
    lfo_encode_buffer(s.format, &o, plain.data(), plain.size(), write_size, &b);
    Member m;
    m.base = s.z.size();
    const DecHeader h = parse_container(s.format, b.p, b.n, nullptr);
    if (h.status) fail("the oracle's header does not parse");
    m.defl = m.base + h.deflate_off;
    m.end = m.base + b.n;
    m.blk.resize(4096);
    const long nb = lfo_scan_blocks(b.p + h.deflate_off, b.n - h.deflate_off, m.blk.data(), m.blk.size());
    if (nb <= 0 || nb > 4096) fail("lfo_scan_blocks: %ld", nb);
    m.blk.resize((size_t)nb);
    uint64_t at = 0;
    for (size_t j = 0; j < m.blk.size(); j++) {
        if (j && m.blk[j].start_bit != m.blk[j - 1].end_bit) fail("blocks do not tile the member");
        m.out_at.push_back(at);
        at += m.blk[j].out_len;
    }
    m.out_at.push_back(at);
    if (at != plain.size() || (m.blk.back().end_bit + 7) / 8 + h.deflate_off + trailer_len(s.format) != b.n) fail("member layout");
    m.plain = plain;
    s.z.insert(s.z.end(), b.p, b.p + b.n);
    lfo_buf_free(&b);
    s.members.push_back(m);
}
static Stream one_member(int format, const Bytes &plain, size_t block_size, size_t write_size) {
    Stream s;
    s.format = format;
    add_member(s, plain, block_size, write_size);
    return s;
}

// ---- the stand-in backend
static const char *DAMAGE_MSG = "stand-in: damaged block";
struct Call { uint64_t n, out_cap, out_len; bool partial, off_thread; int status; };
struct Shared {                                  // what a run's backend calls leave behind (the decoder holds a copy of Fake)
    std::mutex mu;
    std::vector<Call> calls;
    std::thread::id caller;
    std::atomic<bool> hold_until_freed{false}, freeing{false};
};
struct Fake {
    const Stream *s = nullptr;
    Shared *sh = nullptr;
    long bad_member = -1, bad_block = -1;
    void operator()(const WindowIn &wi, DecWindow<Bytes> &W) const {
        const bool off_thread = std::this_thread::get_id() != sh->caller;
        if (off_thread && sh->hold_until_freed)             // (the window is in flight for as long as the caller has not begun to free)
            { while (!sh->freeing) std::this_thread::yield(); for (int i = 0; i < 2000; i++) std::this_thread::yield(); }
        const uint64_t abs_bit = wi.in_base * 8 + wi.bit_off;
        const Member *m = nullptr;
        size_t k = 0;
        for (auto &c : s->members)
            for (size_t j = 0; j < c.blk.size(); j++)
                if (c.defl * 8 + c.blk[j].start_bit == abs_bit) { m = &c; k = j; }
        if (!m) fail("a window starts at bit %llu of the reader: no block starts there", (unsigned long long)abs_bit);
        if (wi.member_out != m->out_at[k]) fail("member_out %llu in front of block %zu", (unsigned long long)wi.member_out, k);
        const uint64_t H = std::min<uint64_t>(wi.member_out, MAX_WINDOW);
        if (wi.hist_len != H || (H && memcmp(wi.hist, m->plain.data() + wi.member_out - H, H))) fail("history in front of block %zu", k);
        if (wi.format != s->format) fail("format");
        WindowResult &r = W.mr;
        const uint64_t rel0 = m->defl * 8 - wi.in_base * 8;     // the member's bit 0 relative to in[0] (mod 2^64: in_base may lie behind it)
        uint64_t got = 0;
        r.end_bit = wi.bit_off;
        for (size_t j = k; j < m->blk.size(); j++) {
            const lfo_blockinfo &b = m->blk[j];
            const bool inside = rel0 + b.end_bit <= wi.n * 8;
            if (m == &s->members[bad_member < 0 ? 0 : bad_member] && (long)j == bad_block && (inside || !wi.partial())) {
                r.status = LFX_E_INVALID_DATA;
                r.msg = DAMAGE_MSG;
                r.blk_out_start = got;
                got += b.out_len / 2;                            // (what the damaged block gave before its damage)
                r.end_byte = std::min<uint64_t>((rel0 + b.start_bit) / 8 + 1, wi.n);
                break;
            }
            if (!inside) {
                if (!wi.partial()) { r.status = LFX_E_UNEXPECTED_EOF; r.msg = "failed to fill whole buffer"; r.blk_out_start = got; r.end_byte = wi.n; }
                break;
            }
            if (got + b.out_len > wi.out_cap) {
                if (!wi.partial()) { r.status = LFX_E_NOSPACE; r.msg = "output capacity too small"; r.blk_out_start = got; }
                else if (got == 0) r.need_cap = true;
                break;
            }
            got += b.out_len;
            r.end_bit = rel0 + b.end_bit;
            r.end_byte = (r.end_bit + 7) / 8;
            if (b.bfinal) { r.final_seen = true; break; }
        }
        r.out_len = got;
        if (r.status == LFX_OK) r.blk_out_start = got;
        W.out.assign(m->plain.begin() + (std::ptrdiff_t)wi.member_out, m->plain.begin() + (std::ptrdiff_t)(wi.member_out + got));
        W.crc = lfo_crc32(0, W.out.data(), W.out.size());
        W.adler = lfo_adler32(1, W.out.data(), W.out.size());
        std::lock_guard<std::mutex> lock(sh->mu);
        sh->calls.push_back(Call{wi.n, wi.out_cap, got, wi.partial(), off_thread, r.status});
    }
};
typedef StreamDec<Bytes, Fake> Dec;

// ---- readers
enum { R_ALL, R_FIXED, R_RANDOM, R_BLOCKY };
struct Reader {
    const Bytes *z = nullptr;
    size_t pos = 0, step = 0;
    int mode = R_ALL;
    std::mt19937 rng{7};
    std::thread::id caller;
    bool other_thread = false;
    static int64_t cb(void *u, uint8_t *p, size_t cap) {
        Reader *r = (Reader *)u;
        if (std::this_thread::get_id() != r->caller) r->other_thread = true;
        size_t k = std::min(cap, r->z->size() - r->pos);
        if (r->mode == R_FIXED) k = std::min(k, r->step);
        if (r->mode == R_RANDOM || r->mode == R_BLOCKY) k = std::min<size_t>(k, 1 + r->rng() % 3000);
        if (r->mode == R_BLOCKY && r->rng() % 3 == 0) return -(int64_t)LFX_E_WOULD_BLOCK;
        memcpy(p, r->z->data() + r->pos, k);
        r->pos += k;
        return (int64_t)k;
    }
};

static WindowPolicy small_policy() {
    WindowPolicy p;
    p.first_target = 4 << 10; p.window_in = 16 << 10; p.window_in_later = 32 << 10; p.window_out = 64 << 10;
    p.window_in_max = 1 << 20; p.ahead_min = 8 << 10; p.retry_min = 1 << 10; p.pull = 8 << 10; p.header_pull = 64;
    return p;
}

struct Result {
    int ctor = LFX_OK, status = LFX_OK;
    std::string msg;
    Bytes out, surplus, unread;
    uint64_t consumed = 0, max_buffered = 0;
    std::vector<Call> calls;
    size_t reader_pos = 0;
};
struct Spec {
    uint32_t flags = 0;
    int mode = R_ALL;
    size_t step = 0, read_size = 8192;
    WindowPolicy pol = small_policy();
    long bad_member = -1, bad_block = -1;
    bool watch_buffered = true;              // dec_buffered after every call (it waits for the worker)
    const Bytes *surplus_quiet_until = nullptr;   // surplus must report 0 bytes while fewer bytes than these have come out
};
static Result run(const Stream &s, const Bytes &z, const Spec &sp) {
    Result res;
    Shared sh;
    sh.caller = std::this_thread::get_id();
    Reader rd;
    rd.z = &z; rd.mode = sp.mode; rd.step = sp.step; rd.caller = sh.caller;
    Dec *d = new Dec();
    d->backend.s = &s; d->backend.sh = &sh; d->backend.bad_member = sp.bad_member; d->backend.bad_block = sp.bad_block;
    d->pol = sp.pol;
    d->format = s.format; d->flags = sp.flags; d->r = Reader::cb; d->user = &rd;
    res.ctor = dec_open(d);
    if (res.ctor) { res.msg = d->err; delete d; return res; }
    Bytes buf(std::max<size_t>(sp.read_size, 1));
    const uint8_t *p;
    size_t n;
    for (int spins = 0;; spins++) {
        CHECK(spins < 4000000, "the decoder does not come to an end");
        CHECK(dec_read(d, buf.data(), 0) == 0, "a read of capacity 0 returns 0");
        const int64_t k = dec_read(d, buf.data(), sp.read_size);
        if (sp.watch_buffered) res.max_buffered = std::max(res.max_buffered, dec_buffered(d));
        if (k == -(int64_t)LFX_E_WOULD_BLOCK) { CHECK(sp.flags & LFX_DEC_NONBLOCKING, "WouldBlock from a blocking decoder"); continue; }
        if (k < 0) { res.status = (int)-k; res.msg = d->err; break; }
        if (k == 0) break;
        CHECK((size_t)k <= sp.read_size, "a read returns more than its capacity");
        res.out.insert(res.out.end(), buf.begin(), buf.begin() + k);
        if (sp.surplus_quiet_until && res.out.size() < sp.surplus_quiet_until->size()) {
            dec_surplus(d, &p, &n);
            CHECK(n == 0, "surplus reports %zu bytes while a member is being collected", n);
        }
    }
    for (int i = 0; i < 3; i++) {
        CHECK(dec_read(d, buf.data(), sp.read_size) == 0, "after the end (or the error, reported once) every read returns 0");
        CHECK(dec_read(d, buf.data(), 0) == 0, "a read of capacity 0 returns 0");
    }
    dec_surplus(d, &p, &n);
    res.surplus.assign(p, p + n);
    dec_unread(d, &p, &n);
    res.unread.assign(p, p + n);
    res.consumed = d->consumed_total;
    dec_close(d, [](Bytes &&v) { Bytes taken(std::move(v)); });
    CHECK(!rd.other_thread, "the read callback ran on a thread other than the caller's");
    res.calls = sh.calls;
    res.reader_pos = rd.pos;
    return res;
}
static size_t off_thread_calls(const Result &r) {
    size_t k = 0;
    for (auto &c : r.calls) k += c.off_thread;
    return k;
}

// ---- the cases
static void readers_and_reads() {
    const WindowPolicy pol = small_policy();
    const uint64_t bound = pol.window_in_later + 2 * pol.window_out + pol.history;
    for (int format = 0; format < 3; format++) {
        std::vector<Stream> streams;
        streams.push_back(one_member(format, Bytes(), 8192, 4096));
        streams.push_back(one_member(format, Bytes(1, 'q'), 8192, 4096));
        streams.push_back(one_member(format, make_plain(150000, 0, 1 + format), 8192, 4096));        // blocks far below a window
        streams.push_back(one_member(format, make_plain(120000, 1, 4 + format), 20000, 0));          // stored blocks, several a window
        for (size_t si = 0; si < streams.size(); si++) {
            const Stream &s = streams[si];
            const Bytes plain = s.plain();
            struct { int mode; size_t step; uint32_t flags; } readers[] = {
                {R_ALL, 0, 0}, {R_FIXED, 1, 0}, {R_FIXED, 7, 0}, {R_RANDOM, 0, 0}, {R_BLOCKY, 0, LFX_DEC_NONBLOCKING}};
            for (auto &rdr : readers)
                for (size_t read_size : {(size_t)1, (size_t)8192, plain.size() + 1000}) {
                    g_case = "readers and reads";
                    Spec sp;
                    sp.mode = rdr.mode; sp.step = rdr.step; sp.flags = rdr.flags; sp.read_size = read_size;
                    sp.surplus_quiet_until = &plain;
                    const Result r = run(s, s.z, sp);
                    CHECK(r.ctor == LFX_OK && r.status == LFX_OK, "format %d stream %zu: status %d / %d (%s)", format, si, r.ctor, r.status, r.msg.c_str());
                    CHECK(r.out == plain, "format %d stream %zu mode %d read %zu: %zu bytes, not the plain text", format, si, rdr.mode, read_size, r.out.size());
                    CHECK(r.consumed == s.z.size(), "consumed %llu of %zu", (unsigned long long)r.consumed, s.z.size());
                    CHECK(r.max_buffered <= bound, "buffered %llu above the bound %llu", (unsigned long long)r.max_buffered, (unsigned long long)bound);
                    CHECK(r.surplus.empty() && r.unread.empty(), "surplus / unread of a clean stream");
                    if (sp.flags & LFX_DEC_NONBLOCKING) CHECK(off_thread_calls(r) == 0, "a backend call of a non-blocking decoder left the caller's thread");
                }
        }
    }
}

static void default_policy() {
    g_case = "default policy";
    const Stream s = one_member(LFX_GZIP, make_plain(300000, 0, 21), 65536, 4096);
    Spec sp;
    sp.pol = WindowPolicy();
    sp.mode = R_RANDOM;
    const Result r = run(s, s.z, sp);
    CHECK(r.status == LFX_OK && r.out == s.plain() && r.consumed == s.z.size(), "status %d, %zu bytes", r.status, r.out.size());
    const WindowPolicy p;
    CHECK(p.window_in == 16ull << 20 && p.window_in_later == 32ull << 20 && p.window_out == 96ull << 20 && p.window_in_max == 4ull << 30 &&
          p.first_target == 1 << 20 && p.pull == 4 << 20 && p.header_pull == 1 << 16 && p.ahead_min == 4 << 20 && p.history == 32768 &&
          p.retry_min == 1 << 16, "the default policy's numbers");
}

static void surplus_and_multi() {
    g_case = "surplus";
    for (int format = 0; format < 3; format++) {
        const Stream s = one_member(format, make_plain(90000, 0, 30 + format), 8192, 4096);
        Bytes z = s.z;
        const Bytes junk = make_plain(5000, 1, 33);
        z.insert(z.end(), junk.begin(), junk.end());
        const Bytes plain = s.plain();
        Spec sp;
        sp.surplus_quiet_until = &plain;
        const Result r = run(s, z, sp);                     // (everything at once: `in` holds the junk from the first pull on)
        CHECK(r.status == LFX_OK && r.out == plain && r.consumed == s.z.size(), "status %d", r.status);
        CHECK(r.surplus.size() + r.consumed == r.reader_pos && std::equal(r.surplus.begin(), r.surplus.end(), junk.begin()),
              "surplus: %zu bytes behind %llu consumed, %zu pulled", r.surplus.size(), (unsigned long long)r.consumed, r.reader_pos);
        CHECK(!r.surplus.empty(), "the junk behind the trailer is not in the surplus");
    }
    g_case = "MultiDecoder";
    Stream s;
    s.format = LFX_GZIP;
    add_member(s, make_plain(70000, 0, 40), 8192, 4096);
    add_member(s, Bytes(), 8192, 4096);
    add_member(s, make_plain(50000, 1, 41), 16384, 0);
    for (int mode : {R_ALL, R_RANDOM, R_BLOCKY}) {
        Bytes z = s.z;
        z.insert(z.end(), s.z.begin(), s.z.begin() + 7);   // a fourth header, cut short
        Spec sp;
        sp.flags = LFX_DEC_MULTI | (mode == R_BLOCKY ? LFX_DEC_NONBLOCKING : 0);
        sp.mode = mode;
        const Result r = run(s, z, sp);
        CHECK(r.status == LFX_OK && r.out == s.plain(), "three members and a cut header: status %d (%s), %zu bytes", r.status, r.msg.c_str(), r.out.size());
        CHECK(r.consumed == z.size(), "consumed %llu of %zu", (unsigned long long)r.consumed, z.size());
    }
    // a FIRST header cut short: the constructor's failure; a non-blocking decoder's first read or header call
    const Bytes cut(s.z.begin(), s.z.begin() + 6);
    Spec sp;
    sp.flags = LFX_DEC_MULTI;
    Result r = run(s, cut, sp);
    CHECK(r.ctor == LFX_E_UNEXPECTED_EOF && r.msg == "failed to fill whole buffer", "constructor: %d (%s)", r.ctor, r.msg.c_str());
    sp.flags = LFX_DEC_MULTI | LFX_DEC_NONBLOCKING;
    r = run(s, cut, sp);
    CHECK(r.ctor == LFX_OK && r.status == LFX_E_UNEXPECTED_EOF && r.out.empty(), "non-blocking, first read: %d / %d", r.ctor, r.status);
    {
        Shared sh;
        Reader rd;
        rd.z = &cut; rd.caller = sh.caller = std::this_thread::get_id();
        Dec d;
        d.backend.s = &s; d.backend.sh = &sh;
        d.pol = small_policy(); d.format = LFX_GZIP; d.flags = sp.flags; d.r = Reader::cb; d.user = &rd;
        lfx_header h;
        CHECK(dec_open(&d) == LFX_OK && dec_header_get(&d, &h) == LFX_E_UNEXPECTED_EOF, "non-blocking, header call");
        uint8_t b[16];
        CHECK(dec_read(&d, b, 16) == 0, "a decoder that failed in header() reads 0");
    }
}

static void truncation_and_trailers() {
    for (int format = 0; format < 3; format++) {
        const Stream s = one_member(format, make_plain(130000, 0, 50 + format), 8192, 4096);
        const Member &m = s.members[0];
        const Bytes plain = s.plain();
        g_case = "cut in the body";
        for (int mode : {R_ALL, R_RANDOM, R_BLOCKY}) {
            const uint64_t cut = m.defl + (m.blk.back().end_bit / 8) * 6 / 10;
            size_t j = 0;
            while (m.defl * 8 + m.blk[j].end_bit <= cut * 8) j++;        // the first block that is not complete
            Spec sp;
            sp.mode = mode;
            sp.flags = mode == R_BLOCKY ? LFX_DEC_NONBLOCKING : 0;
            const Result r = run(s, Bytes(s.z.begin(), s.z.begin() + (std::ptrdiff_t)cut), sp);
            CHECK(r.status == LFX_E_UNEXPECTED_EOF, "status %d", r.status);
            CHECK(r.consumed == cut, "consumed %llu of the %llu bytes the reader had", (unsigned long long)r.consumed, (unsigned long long)cut);
            CHECK(r.out.size() == m.out_at[j] && std::equal(r.out.begin(), r.out.end(), plain.begin()), "%zu bytes, the complete blocks hold %llu",
                  r.out.size(), (unsigned long long)m.out_at[j]);
        }
        if (format == LFX_DEFLATE) continue;
        g_case = "cut in the trailer";
        for (size_t keep : {(size_t)0, (size_t)3}) {
            const Bytes z(s.z.begin(), s.z.end() - (std::ptrdiff_t)(trailer_len(format) - keep));
            const Result r = run(s, z, Spec());
            CHECK(r.status == LFX_E_UNEXPECTED_EOF && r.msg == "failed to fill whole buffer", "status %d (%s)", r.status, r.msg.c_str());
            CHECK(r.out == plain && r.consumed == z.size(), "%zu bytes, consumed %llu", r.out.size(), (unsigned long long)r.consumed);
        }
        g_case = "bad trailer";
        Bytes z = s.z;
        uint8_t *t = z.data() + z.size() - trailer_len(format);
        t[1] ^= 0x40;
        const uint32_t stored = format == LFX_GZIP ? (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24
                                                   : (uint32_t)t[0] << 24 | (uint32_t)t[1] << 16 | (uint32_t)t[2] << 8 | t[3];
        const std::string want = format == LFX_GZIP ? format_error(ERR_CRC32, lfo_crc32(0, plain.data(), plain.size()), stored)
                                                    : format_error(ERR_ADLER32, lfo_adler32(1, plain.data(), plain.size()), stored);
        for (int mode : {R_ALL, R_RANDOM}) {
            Spec sp;
            sp.mode = mode;
            const Result r = run(s, z, sp);
            CHECK(r.status == LFX_E_INVALID_DATA && r.msg == want, "status %d, \"%s\", expected \"%s\"", r.status, r.msg.c_str(), want.c_str());
            CHECK(r.out == plain && r.consumed == z.size(), "%zu bytes in front of the verdict", r.out.size());
        }
    }
}

static void damaged_block() {
    g_case = "a damaged block in a later window";
    const Stream s = one_member(LFX_ZLIB, make_plain(200000, 0, 60), 8192, 4096);
    const Member &m = s.members[0];
    const long bad = (long)m.blk.size() * 2 / 3;
    for (int mode : {R_ALL, R_RANDOM, R_BLOCKY})
        for (size_t read_size : {(size_t)1000, (size_t)8192, (size_t)1 << 20}) {
            Spec sp;
            sp.mode = mode;
            sp.flags = mode == R_BLOCKY ? LFX_DEC_NONBLOCKING : 0;
            sp.read_size = read_size;
            sp.bad_member = 0; sp.bad_block = bad;
            const Result r = run(s, s.z, sp);
            CHECK(r.status == LFX_E_INVALID_DATA && r.msg == DAMAGE_MSG, "status %d (%s)", r.status, r.msg.c_str());
            CHECK(r.out.size() == m.out_at[bad] && std::equal(r.out.begin(), r.out.end(), m.plain.begin()), "%zu bytes in front of the verdict, blk_out_start is %llu",
                  r.out.size(), (unsigned long long)m.out_at[bad]);
            CHECK(r.calls.size() > 3, "the damage lies in the first windows");
            const uint64_t end_byte = (m.defl * 8 + m.blk[bad].start_bit) / 8 + 1;      // (what the stand-in reports, as a reader offset)
            CHECK(r.consumed == end_byte, "consumed %llu, the verdict's end_byte is at %llu", (unsigned long long)r.consumed, (unsigned long long)end_byte);
            const uint64_t part = m.blk[bad].out_len / 2;
            CHECK(r.unread.size() == part && std::equal(r.unread.begin(), r.unread.end(), m.plain.begin() + (std::ptrdiff_t)m.out_at[bad]), "unread: %zu bytes, the damaged block gave %llu",
                  r.unread.size(), (unsigned long long)part);
        }
}

static void growth_and_limits() {
    g_case = "a block larger than the window";
    {
        const Stream s = one_member(LFX_GZIP, make_plain(150000, 1, 70), 1 << 20, 0);       // stored blocks of 65535 bytes: four windows' worth each
        Spec sp;
        sp.watch_buffered = false;
        sp.pol.window_out = 1 << 20;
        const Result r = run(s, s.z, sp);
        CHECK(r.status == LFX_OK && r.out == s.plain(), "status %d", r.status);
        std::vector<uint64_t> tries;
        for (auto &c : r.calls) { if (c.out_len) break; tries.push_back(c.n); }
        CHECK(tries.size() >= 4, "%zu attempts in front of the first block", tries.size());
        for (size_t i = 1; i < tries.size(); i++) CHECK(tries[i] == 2 * tries[i - 1], "attempt %zu had %llu bytes after %llu", i, (unsigned long long)tries[i], (unsigned long long)tries[i - 1]);
    }
    g_case = "a block larger than the output room";
    for (int path = 0; path < 2; path++) {
        const Stream s = one_member(LFX_ZLIB, make_plain(300000, 2, 71), 1 << 20, 0);       // one block, far below the first target
        Bytes z = s.z;
        if (path == 0) z.resize(z.size() + 8192, 0);         // junk behind it: the first target is reached before the reader ends → partial
        Spec sp;
        sp.watch_buffered = false;
        const Result r = run(s, z, sp);
        CHECK(r.status == LFX_OK && r.out == s.plain() && r.consumed == s.z.size(), "path %d: status %d, %zu bytes", path, r.status, r.out.size());
        CHECK(r.calls.size() == 4, "path %d: %zu backend calls", path, r.calls.size());
        // (path 1: the reader's short first read triggers a partial attempt; the next pull finds its end, and the exact walk follows)
        for (size_t i = 0; i < r.calls.size(); i++) {
            const bool partial = path == 0 || i == 0;
            CHECK(r.calls[i].out_cap == sp.pol.window_out << i && r.calls[i].partial == partial, "path %d call %zu: room %llu, partial %d", path, i,
                  (unsigned long long)r.calls[i].out_cap, (int)r.calls[i].partial);
            CHECK(r.calls[i].status == (i < 3 && !partial ? LFX_E_NOSPACE : LFX_OK), "path %d call %zu: status %d", path, i, r.calls[i].status);
        }
    }
    g_case = "no complete block at the input limit";
    {
        const Stream s = one_member(LFX_DEFLATE, make_plain(150000, 1, 72), 1 << 20, 0);    // stored blocks of 65535 bytes
        Spec sp;
        sp.watch_buffered = false;
        sp.pol.window_in_max = 32 << 10;
        sp.mode = R_RANDOM;
        const Result r = run(s, s.z, sp);
        CHECK(r.status == LFX_E_UNSUPPORTED && r.out.empty() && r.reader_pos < s.z.size(), "status %d, %zu bytes, reader at %zu", r.status, r.out.size(), r.reader_pos);
        CHECK(r.msg == "a DEFLATE block exceeds the stream decoder's window limit (4 GiB of compressed bytes)", "\"%s\"", r.msg.c_str());
        CHECK(!r.calls.back().partial && r.calls.back().n >= sp.pol.window_in_max, "the last attempt: %llu bytes", (unsigned long long)r.calls.back().n);
    }
}

static void decode_ahead() {
    g_case = "decode ahead";
    const Stream s = one_member(LFX_GZIP, make_plain(400000, 0, 80), 8192, 4096);
    Spec sp;
    sp.watch_buffered = false;                    // (the worker runs beside the serving reads)
    const Result r = run(s, s.z, sp);
    CHECK(r.status == LFX_OK && r.out == s.plain(), "status %d", r.status);
    CHECK(r.calls.size() > 3 && r.calls[0].n == sp.pol.first_target && r.calls[1].n == sp.pol.window_in && r.calls[2].n == sp.pol.window_in_later &&
          r.calls[3].n == sp.pol.window_in_later, "the windows' input: %llu, %llu, %llu bytes", (unsigned long long)r.calls[0].n,
          (unsigned long long)r.calls[1].n, (unsigned long long)r.calls[2].n);
    CHECK(off_thread_calls(r) >= 1 && off_thread_calls(r) < r.calls.size(), "%zu of %zu backend calls ran on a worker", off_thread_calls(r), r.calls.size());
    sp.flags = LFX_DEC_NONBLOCKING;
    const Result nb = run(s, s.z, sp);
    CHECK(nb.status == LFX_OK && nb.out == s.plain() && off_thread_calls(nb) == 0, "non-blocking: %zu calls on a worker", off_thread_calls(nb));
    // freed with a window in flight: the worker is held inside the backend until the free has begun
    Shared sh;
    sh.hold_until_freed = true;
    Reader rd;
    rd.z = &s.z; rd.caller = sh.caller = std::this_thread::get_id();
    Dec *d = new Dec();
    d->backend.s = &s; d->backend.sh = &sh;
    d->pol = small_policy(); d->format = LFX_GZIP; d->r = Reader::cb; d->user = &rd;
    CHECK(dec_open(d) == LFX_OK, "open");
    Bytes buf(100);
    size_t got = 0;
    while (!d->ahead && got < 300000) {
        const int64_t k = dec_read(d, buf.data(), buf.size());
        CHECK(k > 0, "read %lld", (long long)k);
        got += (size_t)k;
    }
    CHECK(d->ahead, "no window was started ahead");
    sh.freeing = true;
    size_t given = 0;
    bool early = false;
    dec_close(d, [&](Bytes &&v) {                 // (as lfx_decoder_free: the worker first, then the buffers leave, then the decoder)
        Bytes taken(std::move(v));
        std::lock_guard<std::mutex> lock(sh.mu);
        early |= !sh.calls.back().off_thread;
        given++;
    });
    CHECK(given == 3 && !early, "%zu buffers handed back, %s the worker had finished", given, early ? "BEFORE" : "after");
    CHECK(sh.calls.back().off_thread && !rd.other_thread, "the window in flight was finished by its worker");
}

int main() {
    readers_and_reads();
    default_policy();
    surplus_and_multi();
    truncation_and_trailers();
    damaged_block();
    growth_and_limits();
    decode_ahead();
    printf("stream_dec ok: %d checks\n", g_checks);
    return 0;
}
