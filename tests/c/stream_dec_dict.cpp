// The stream decoder's state machine (libflate_amd/csrc/lfx_stream_dec.h) with a preset dictionary, on the host: a plain
// compiler, no HIP.  The window backend is zlib's raw inflate primed with the history the policy hands over
// (inflateSetDictionary): it decodes a member once the reader has ended and answers "no complete block yet" before — so what is
// checked is the policy's side of DESIGN §17: the FDICT verdicts of the header (resolve_fdict), the seeding of the first
// window's history, the reach bound passed on (dict_len), the trailer over the output only, when lfx_decoder_set_dict is
// still allowed, LFX_DEC_LAZY_HEADER, and the non-blocking mode.  Streams come from zlib's deflate with deflateSetDictionary.
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../libflate_amd/csrc/lfx_stream_dec.h"

using namespace lfx;
typedef std::vector<uint8_t> Bytes;

extern "C" uint32_t lfx_crc32_combine(uint32_t a, uint32_t b, uint64_t n) { return (uint32_t)crc32_combine(a, b, (z_off_t)n); }
extern "C" uint32_t lfx_adler32_combine(uint32_t a, uint32_t b, uint64_t n) { return (uint32_t)adler32_combine(a, b, (z_off_t)n); }

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { fails++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static Bytes text(size_t n, unsigned seed) {
    static const char *w[] = {"record", "field", "value", "status", "error", "the", "of", "and", "request", "response", "user"};
    Bytes b;
    unsigned s = seed * 2654435761u + 1;
    while (b.size() < n) {
        s = s * 1664525u + 1013904223u;
        const char *p = w[(s >> 16) % 11];
        while (*p && b.size() < n) b.push_back((uint8_t)*p++);
        if (b.size() < n) b.push_back(' ');
    }
    return b;
}
static Bytes deflate_with(const Bytes &data, const Bytes *dict, int wbits) {
    z_stream z{};
    deflateInit2(&z, 9, Z_DEFLATED, wbits, 8, Z_DEFAULT_STRATEGY);
    if (dict) deflateSetDictionary(&z, dict->data(), (uInt)dict->size());
    Bytes out(deflateBound(&z, (uLong)data.size()) + 16);
    z.next_in = (Bytef *)data.data(); z.avail_in = (uInt)data.size();
    z.next_out = out.data(); z.avail_out = (uInt)out.size();
    deflate(&z, Z_FINISH);
    out.resize(z.total_out);
    deflateEnd(&z);
    return out;
}

struct Seen { uint64_t dict_len = ~0ull, hist_len = ~0ull, calls = 0; };
struct ZBackend {
    Seen *seen = nullptr;
    void operator()(const WindowIn &wi, DecWindow<Bytes> &W) const {
        seen->calls++;
        W.mr = WindowResult();
        W.mr.end_bit = wi.bit_off;
        if (wi.partial()) return;                       // (no complete block yet: the policy comes back with more input)
        seen->dict_len = wi.dict_len; seen->hist_len = wi.hist_len;
        z_stream z{};
        inflateInit2(&z, -15);
        if (wi.hist_len) inflateSetDictionary(&z, wi.hist, (uInt)wi.hist_len);
        W.out.resize(wi.out_cap);
        z.next_in = (Bytef *)wi.in; z.avail_in = (uInt)wi.n;
        z.next_out = W.out.data(); z.avail_out = (uInt)W.out.size();
        const int rc = inflate(&z, Z_FINISH);
        W.out.resize(z.total_out);
        W.mr.out_len = z.total_out; W.mr.end_byte = z.total_in; W.mr.end_bit = z.total_in * 8;
        if (rc == Z_STREAM_END) { W.mr.blk_out_start = z.total_out; W.mr.final_seen = true; W.adler = (uint32_t)adler32(1, W.out.data(), (uInt)W.out.size()); }
        else if (rc == Z_BUF_ERROR && z.avail_out == 0) W.mr.status = LFX_E_NOSPACE;
        else { W.mr.status = z.avail_in == 0 && rc == Z_BUF_ERROR ? LFX_E_UNEXPECTED_EOF : LFX_E_INVALID_DATA; W.mr.msg = z.msg ? z.msg : "damaged"; W.mr.out_len = 0; W.out.clear(); }
        inflateEnd(&z);
    }
};
typedef StreamDec<Bytes, ZBackend> Dec;

struct Reader {
    const Bytes *z; size_t pos = 0, step; bool blocky; bool armed = true;
    static int64_t cb(void *u, uint8_t *p, size_t cap) {
        Reader *r = (Reader *)u;
        if (r->blocky && r->armed && r->pos < r->z->size()) { r->armed = false; return -(int64_t)LFX_E_WOULD_BLOCK; }
        r->armed = true;
        const size_t k = std::min(std::min(cap, r->step), r->z->size() - r->pos);
        memcpy(p, r->z->data() + r->pos, k);
        r->pos += k;
        return (int64_t)k;
    }
};
struct Run { int ctor = 0, set = 0, status = 0; Bytes out; std::string msg; Seen seen; uint64_t consumed = 0; };

// new → (set_dict) → header for a lazy blocking decoder → read to the end
static Run run(int format, uint32_t flags, const Bytes &z, const Bytes *dict, size_t step, size_t read_cap) {
    Run r;
    Reader rd{&z, 0, step, (flags & LFX_DEC_NONBLOCKING) != 0};
    Dec *d = new Dec();
    d->backend.seen = &r.seen;
    d->format = format; d->flags = flags; d->r = Reader::cb; d->user = &rd;
    r.ctor = dec_open(d);
    if (r.ctor) { r.msg = d->err; dec_close(d, [](Bytes &&) {}); return r; }
    if (dict) r.set = dec_set_dict(d, dict->data() + (dict->size() > 32768 ? dict->size() - 32768 : 0), std::min<size_t>(dict->size(), 32768),
                                   (uint32_t)adler32(1, dict->data(), (uInt)dict->size()));
    if ((flags & LFX_DEC_LAZY_HEADER) && !(flags & LFX_DEC_NONBLOCKING)) {
        lfx_header h;
        r.ctor = dec_header_get(d, &h);
        if (r.ctor) { r.msg = d->err; r.consumed = d->consumed_total; dec_close(d, [](Bytes &&) {}); return r; }
    }
    Bytes buf(read_cap);
    for (;;) {
        const int64_t k = dec_read(d, buf.data(), buf.size());
        if (k == -(int64_t)LFX_E_WOULD_BLOCK) continue;
        if (k < 0) { r.status = (int)-k; r.msg = d->err; break; }
        if (k == 0) break;
        r.out.insert(r.out.end(), buf.begin(), buf.begin() + k);
    }
    r.consumed = d->consumed_total;
    dec_close(d, [](Bytes &&) {});
    return r;
}

int main() {
    const Bytes dict = text(32768, 1), big = text(40000, 2), other = text(300, 3), rec = text(1100, 4), none;
    Bytes rec40(big.begin() + 8000, big.begin() + 8600);
    rec40.insert(rec40.end(), rec.begin(), rec.begin() + 500);
    const Bytes zl = deflate_with(rec, &dict, 15), raw = deflate_with(rec, &dict, -15), plain = deflate_with(rec, nullptr, 15),
                zl40 = deflate_with(rec40, &big, 15);
    CHECK((zl[1] & 0x20) && !(plain[1] & 0x20) && zl.size() < plain.size(), "fixtures");
    const uint32_t LAZY = LFX_DEC_LAZY_HEADER, NB = LFX_DEC_NONBLOCKING;
    int n = 0;
    for (size_t step : {(size_t)1, (size_t)7, (size_t)1 << 20})
        for (size_t cap : {(size_t)1, (size_t)7, (size_t)8192})
            for (uint32_t flags : {LAZY, NB}) {
                Run r = run(LFX_ZLIB, flags, zl, &dict, step, cap);
                CHECK(!r.ctor && !r.set && !r.status && r.out == rec && r.consumed == zl.size() && r.seen.dict_len == 32768 && r.seen.hist_len == 32768,
                      "zlib step %zu cap %zu flags %u: %d %d %d (%s) out %zu dict_len %llu", step, cap, flags, r.ctor, r.set, r.status, r.msg.c_str(),
                      r.out.size(), (unsigned long long)r.seen.dict_len);
                r = run(LFX_DEFLATE, flags & NB, raw, &dict, step, cap);         // (raw DEFLATE needs no lazy header)
                CHECK(!r.ctor && !r.set && !r.status && r.out == rec && r.seen.dict_len == 32768, "raw step %zu cap %zu flags %u: %d %d %d (%s)", step, cap,
                      flags, r.ctor, r.set, r.status, r.msg.c_str());
                n += 2;
            }
    // a dictionary longer than the window: the id covers all of it, the history is its tail
    Run r = run(LFX_ZLIB, LAZY, zl40, &big, 7, 8192);
    CHECK(!r.ctor && !r.status && r.out == rec40 && r.seen.hist_len == 32768, "40000-byte dictionary: %d %d (%s)", r.ctor, r.status, r.msg.c_str());
    // FDICT clear: the dictionary is not used
    r = run(LFX_ZLIB, LAZY, plain, &dict, 7, 8192);
    CHECK(!r.ctor && !r.status && r.out == rec && r.seen.dict_len == 0 && r.seen.hist_len == 0, "FDICT clear: %d %d dict_len %llu", r.ctor, r.status,
          (unsigned long long)r.seen.dict_len);
    // an empty dictionary: id 1, no history
    const Bytes zl0 = deflate_with(rec, nullptr, -15);
    r = run(LFX_DEFLATE, 0, zl0, &none, 7, 8192);
    CHECK(!r.set && !r.status && r.out == rec && r.seen.dict_len == 0, "empty dictionary: %d %d", r.set, r.status);
    // the wrong dictionary: the header's verdict, consumed as the FDICT rejection; no dictionary: today's rejection, from the constructor
    char want[128];
    snprintf(want, sizeof want, "Dictionary mismatch: dictionary_id=0x%X, supplied=0x%X", (unsigned)adler32(1, dict.data(), (uInt)dict.size()),
             (unsigned)adler32(1, other.data(), (uInt)other.size()));
    r = run(LFX_ZLIB, LAZY, zl, &other, 1 << 20, 8192);
    CHECK(r.ctor == LFX_E_INVALID_DATA && r.msg == want && r.consumed == 6 && r.seen.calls == 0, "mismatch: %d (%s) consumed %llu", r.ctor, r.msg.c_str(),
          (unsigned long long)r.consumed);
    r = run(LFX_ZLIB, NB, zl, &other, 3, 8192);
    CHECK(!r.ctor && r.status == LFX_E_INVALID_DATA && r.msg == want && r.out.empty(), "mismatch, non-blocking: %d (%s)", r.status, r.msg.c_str());
    r = run(LFX_ZLIB, 0, zl, nullptr, 1 << 20, 8192);
    CHECK(r.ctor == LFX_E_INVALID_DATA && r.msg.rfind("Preset dictionaries are not supported: dictionary_id=0x", 0) == 0, "no dictionary: %d (%s)", r.ctor, r.msg.c_str());
    r = run(LFX_ZLIB, LAZY, zl, nullptr, 1 << 20, 8192);
    CHECK(r.ctor == LFX_E_INVALID_DATA && r.msg.rfind("Preset dictionaries are not supported", 0) == 0, "lazy, no dictionary: %d (%s)", r.ctor, r.msg.c_str());
    // fewer than six header bytes
    r = run(LFX_ZLIB, LAZY, Bytes(zl.begin(), zl.begin() + 5), &dict, 1 << 20, 8192);
    CHECK(r.ctor == LFX_E_UNEXPECTED_EOF, "five header bytes: %d", r.ctor);
    // the trailer covers the output only: the stream's own Adler-32 passed above; a damaged one is the existing verdict
    Bytes bad = zl;
    bad.back() ^= 1;
    r = run(LFX_ZLIB, LAZY, bad, &dict, 1 << 20, 8192);
    CHECK(r.status == LFX_E_INVALID_DATA && r.msg.rfind("Adler32 checksum mismatched", 0) == 0, "bad trailer: %d (%s)", r.status, r.msg.c_str());
    // too late, twice, gzip
    r = run(LFX_ZLIB, 0, plain, &dict, 1 << 20, 8192);            // a blocking constructor has read the header
    CHECK(!r.ctor && r.set == LFX_E_ARG && !r.status && r.out == rec, "set_dict behind a blocking constructor: %d %d", r.set, r.status);
    {
        Seen seen;
        Reader rd{&raw, 0, 1 << 20, false};
        Dec *d = new Dec();
        d->backend.seen = &seen; d->format = LFX_DEFLATE; d->r = Reader::cb; d->user = &rd;
        CHECK(dec_open(d) == LFX_OK && dec_set_dict(d, dict.data(), dict.size(), 5) == LFX_OK && dec_set_dict(d, dict.data(), dict.size(), 5) == LFX_E_ARG, "twice");
        uint8_t b[16];
        CHECK(dec_read(d, b, 16) == 16 && memcmp(b, rec.data(), 16) == 0, "first read");
        dec_close(d, [](Bytes &&) {});
        d = new Dec();
        d->backend.seen = &seen; d->format = LFX_DEFLATE; d->r = Reader::cb; d->user = &rd;
        rd.pos = 0;
        CHECK(dec_open(d) == LFX_OK, "open");
        (void)dec_read(d, b, 16);                              // (fails: no dictionary) — and now it is too late for one
        CHECK(dec_set_dict(d, dict.data(), dict.size(), 5) == LFX_E_ARG, "after the first read");
        dec_close(d, [](Bytes &&) {});
        d = new Dec();
        d->backend.seen = &seen; d->format = LFX_GZIP; d->flags = NB; d->r = Reader::cb; d->user = &rd;
        CHECK(dec_open(d) == LFX_OK && dec_set_dict(d, dict.data(), dict.size(), 5) == LFX_E_ARG, "gzip");
        dec_close(d, [](Bytes &&) {});
    }
    if (fails) { printf("stream_dec_dict: %d failure(s)\n", fails); return 1; }
    printf("stream_dec_dict ok: %d round trips\n", n);
    return 0;
}
