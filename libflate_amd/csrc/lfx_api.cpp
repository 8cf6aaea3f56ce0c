// lfx_api.cpp — C ABI (include/lfx.h) over the HIP kernels: the context, the one-shot / batch / members / sharded encode entry
// points, the Lz77Encode plug-in and the test hooks.  (The stream encoder: lfx_stream_enc.cpp; the decoders: lfx_decode.cpp,
// lfx_stream_dec.cpp.)  Every byte of compression work runs on the GPU.
#include "../../include/lfx.h"
#include "../../include/lfx_testhooks.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "lfx_batch_pack.h"
#include "lfx_ctx.h"
#include "lfx_device.h"
#include "lfx_dict_train.h"
#include "lfx_enc_frame.h"
#include "lfx_encode_int.h"
#include "lfx_huff.h"
#include "lfx_index.h"
#include "lfx_plan.h"
#include "lfx_shuffle.h"
#include "lfx_abi_guard.h"

using namespace lfx;

// ------------------------------------------------------------------------------------------------
// the framing helpers' C ABI (the helpers themselves: lfx_enc_frame.h)
extern "C" uint32_t lfx_crc32_combine(uint32_t crc1, uint32_t crc2, uint64_t len2) { return crc32_combine(crc1, crc2, len2); }
extern "C" uint32_t lfx_adler32_combine(uint32_t ad1, uint32_t ad2, uint64_t len2) { return adler32_combine(ad1, ad2, len2); }
extern "C" void lfx_encode_opts_default(lfx_encode_opts *o) { encode_opts_default(o); }
extern "C" uint32_t lfx_version(void) { return LFX_VERSION; }

extern "C" uint64_t lfx_container_header_len(int format, const lfx_encode_opts *o) {
    std::vector<uint8_t> b;
    EncodeSpec sp;
    (void)encode_spec(format, o, &sp);      // (the header of the normalised options, whatever their domain)
    container_header(format, sp.o, b);
    return b.size();
}

static void apply_schedule(Planner &pl, const lfx_schedule *s, uint64_t n) {
    if (!s || s->kind == LFX_SCHED_SINGLE) {
        pl.write(n);  // write_all of one slice == one write() (encode.rs:243 consumes everything)
    } else if (s->kind == LFX_SCHED_FIXED) {
        uint64_t w = s->fixed_write ? s->fixed_write : n;
        if (w) {
            pl.write_repeat(w, n / w);
            if (n % w) pl.write(n % w);
        }
    } else {
        uint64_t used = 0;
        for (size_t i = 0; i < s->n_writes; i++) {
            if (s->writes[i] == LFX_SCHED_FLUSH) { pl.flush(); continue; }
            uint64_t w = std::min(s->writes[i], n - used);
            pl.write(w);
            used += w;
        }
        if (used < n) pl.write(n - used);
    }
}

// the bound of n bytes planned into nblocks blocks (lfx_encode_batch_packed_device plans every stream anyway)
static uint64_t encode_bound_of(const lfx_encode_opts &d, uint64_t n, size_t nblocks) {
    // a dynamic block never costs more than ~9 bits per literal + its header; stored: 5 bytes per block
    uint64_t hdr = 64 + (d.extra ? d.extra_len + 2 : 0) + (d.filename ? strlen(d.filename) + 1 : 0) +
                   (d.comment ? strlen(d.comment) + 1 : 0);
    return n + n / 4 + 1024 * (uint64_t)nblocks + hdr + 64;
}
extern "C" uint64_t lfx_encode_bound(uint64_t n, const lfx_encode_opts *o, const lfx_schedule *s) {
    EncodeSpec sp;
    if (encode_spec(LFX_ZLIB, o, &sp)) return 0;
    Planner pl(sp.plan);
    apply_schedule(pl, s, n);
    return encode_bound_of(sp.o, n, pl.finish().blocks.size());
}

// ------------------------------------------------------------------------------------------------
// context
namespace lfx {

int DevBuf::reserve(size_t bytes) {
    if (bytes <= cap) return 0;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    gen++;
    size_t want = bytes + bytes / 8 + 4096;
    if (hipMalloc(&p, want) != hipSuccess) {
        if (hipMalloc(&p, bytes) != hipSuccess) { p = nullptr; return LFX_E_OOM; }
        want = bytes;
    }
    cap = want;
    return 0;
}
void DevBuf::release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
}

void Diag::read() {
    auto on = [](const char *k) { return getenv(k) != nullptr; };
    debug = on("LFX_DEBUG");
    match_v1 = on("LFX_MATCH_V1");
    no_serial = on("LFX_NO_SERIAL");
    batch_serial = on("LFX_BATCH_SERIAL");
    no_pieces = on("LFX_NO_PIECES");
    no_final_cand = on("LFX_NO_FINAL_CAND");
    if (const char *eb = getenv("LFX_ENC_BATCH_MB")) enc_batch_mb = atoi(eb);
    two_pass = on("LFX_TWO_PASS");
    hist_separate = on("LFX_HIST_SEPARATE");
    if (const char *pc = getenv("LFX_PACK_BY_CHUNK")) pack_by_chunk = atoi(pc) ? 1 : 0;
    no_pin_slots = on("LFX_NO_PIN_SLOTS");
    no_small_scan = on("LFX_NO_SMALL_SCAN");
    store_tight = on("LFX_STORE_TIGHT");
    if (const char *ds = getenv("LFX_DUMP_SEG")) dump_seg = atoi(ds);
}

void Ctx::phase(const char *name) {
    if (!timing_on) return;
    if (timing_on >= 2 && timing_on <= 5) {
        // only the event in front of ONE kernel's phase and the one behind it
        static const char *const pair[4][2] = {{"lz77_resolve", "lz77_walk"}, {"find2", "blk_scan"}, {"upload", "lz77_cand"}, {"blk_emit", "lz77_copy"}};
        const char *const *pr = pair[timing_on - 2];
        if (strcmp(name, pr[0]) != 0 && strcmp(name, pr[1]) != 0) return;
    }
    if (n_ev >= MAX_EV) return;
    if (!ev[n_ev]) (void)hipEventCreate(&ev[n_ev]);
    (void)hipEventRecord(ev[n_ev], stream);
    snprintf(ev_name[n_ev], sizeof ev_name[n_ev], "%s", name);
    n_ev++;
}

}  // namespace lfx

extern "C" int lfx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" lfx_ctx *lfx_ctx_new(int device, int *status) try {
    int st = LFX_OK;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) {
        if (status) *status = LFX_E_DEVICE;  // fail loudly: there is no CPU path
        return nullptr;
    }
    Ctx *c = new Ctx();
    c->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&c->own_stream) != hipSuccess) {
        delete c;
        if (status) *status = LFX_E_DEVICE;
        return nullptr;
    }
    c->stream = c->own_stream;
    c->diag.read();     // diagnostic environment switches are read once, here
    (void)hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, device);
    if (hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_zero, hipEventDisableTiming) != hipSuccess) {
        (void)hipStreamDestroy(c->own_stream);
        delete c;
        if (status) *status = LFX_E_DEVICE;
        return nullptr;
    }
    if (hipHostMalloc((void **)&c->h_res, 4096 + Ctx::PIN_ARENA, hipHostMallocDefault) != hipSuccess) {
        (void)hipStreamDestroy(c->own_stream);
        delete c;
        if (status) *status = LFX_E_OOM;
        return nullptr;
    }
    if (status) *status = st;
    return reinterpret_cast<lfx_ctx *>(c);
} LFX_ABI_CATCH_NEW
extern "C" void lfx_ctx_free(lfx_ctx *cc) {
    if (!cc) return;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (DevBuf *b : c->all_bufs()) b->release();
    for (DevBuf &b : c->dev_pool) b.release();
    c->dev_pool.clear();
    c->pin_pool.clear();
    for (auto &e : c->ev) if (e) (void)hipEventDestroy(e);
    if (c->h_res) (void)hipHostFree(c->h_res);
    c->hostio.release();
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->ev_zero) (void)hipEventDestroy(c->ev_zero);
    if (c->side_stream) (void)hipStreamDestroy(c->side_stream);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}
extern "C" const char *lfx_ctx_last_error(const lfx_ctx *cc) {
    return cc ? reinterpret_cast<const Ctx *>(cc)->err.c_str() : "no context";
}
extern "C" void lfx_ctx_set_stream(lfx_ctx *cc, void *s) {
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    c->stream = s ? (hipStream_t)s : c->own_stream;
}
extern "C" uint64_t lfx_ctx_match_fallbacks(const lfx_ctx *cc) {
    return cc ? reinterpret_cast<const Ctx *>(cc)->match_fallbacks : 0;
}
extern "C" void lfx_ctx_enable_timing(lfx_ctx *cc, int on) { reinterpret_cast<Ctx *>(cc)->timing_on = on >= 2 && on <= 6 ? on : on != 0; }
extern "C" int lfx_ctx_last_timing(lfx_ctx *cc, lfx_timing *t) try {
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    memset(t, 0, sizeof *t);
    if (c->n_ev < 2) return LFX_E_ARG;
    (void)hipEventSynchronize(c->ev[c->n_ev - 1]);
    (void)hipEventElapsedTime(&t->total_ms, c->ev[0], c->ev[c->n_ev - 1]);
    t->n_phases = c->n_ev - 1;
    for (int i = 0; i + 1 < c->n_ev && i < 16; i++) {
        (void)hipEventElapsedTime(&t->phase_ms[i], c->ev[i], c->ev[i + 1]);
        snprintf(t->phase_name[i], sizeof t->phase_name[i], "%s", c->ev_name[i + 1]);
    }
    return LFX_OK;
} LFX_ABI_CATCH

// ------------------------------------------------------------------------------------------------
// encode entry points: argument checks, the plan, then the encode core (lfx_encode.cpp)
// A preset dictionary in the container and in the plan: dict_header and dict_prime_first (lfx_enc_frame.h),
// which the stream encoder writes and marks with as well.
static void dict_header(int format, const lfx_dict *dict, std::vector<uint8_t> &hdr) { lfx::dict_header(format, dict->id, hdr); }
// the stream's first LZ77 flush unit is the one the dictionary primes — where the options match at all and the dictionary
// has bytes to offer
static void dict_prime(const lfx_dict *dict, Plan &p) {
    if (dict->usable) (void)dict_prime_first(p);
}

static int encode_device_impl(lfx_ctx *cc, int format, const lfx_encode_opts *o, const lfx_schedule *s, const lfx_dict *dict,
                              const void *d_in, uint64_t n, void *d_out, uint64_t cap, uint64_t *out_len) {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    EncodeSpec sp;
    int rc = encode_spec(format, o, &sp);
    if (rc) { c->set_error("option outside the reference's domain"); return rc; }
    if ((rc = served(c, dict ? ENC_DICT_DEVICE : ENC_DEVICE, sp, dict))) return rc;
    std::vector<uint8_t> hdr;
    if ((rc = container_header(format, sp.o, hdr))) { c->set_error("bad container options"); return rc; }
    Planner pl(sp.plan);
    apply_schedule(pl, s, n);
    Plan &plan = pl.finish();
    if (dict) { dict_header(format, dict, hdr); dict_prime(dict, plan); }
    EncodeResult res{};
    const bool fill_ok = ((uintptr_t)d_out & 3) == 0 && cap >= 16;
    if (fill_ok) (void)hipSetDevice(c->device);
    c->prezero.start(d_out, fill_ok ? cap / 4 * 4 : 0);
    rc = with_match_fallback(c, res, [&]() -> int {
        if (int rc2 = encode_prepare(c, plan, sp, (const uint8_t *)d_in, n, ck_mode_of(format), nullptr, dict)) return rc2;
        return encode_emit(c, format, true, 0, true, n, hdr.data(), (uint32_t)hdr.size(), 8 * (uint64_t)hdr.size(),
                           (uint8_t *)d_out, cap, &res);
    });
    c->prezero.settle();     // (prepare or emit failed before the stream waited for the fill: it is on the caller's buffer)
    if (rc) return rc;
    if (out_len) *out_len = res.out_bytes;
    // (an index build, lfx_encode_index_device: the candidates of the stream the last emit wrote, while its buffers hold it)
    if (c->idx_enc) return idx_encode_cand(c, plan);
    return LFX_OK;
}
extern "C" int lfx_encode_device(lfx_ctx *cc, int format, const lfx_encode_opts *o, const lfx_schedule *s,
                                 const void *d_in, uint64_t n, void *d_out, uint64_t cap, uint64_t *out_len) try {
    return encode_device_impl(cc, format, o, s, nullptr, d_in, n, d_out, cap, out_len);
} LFX_ABI_CATCH
// ---- the dictionary calls: the same encode with the first chunk of the stream primed; without a dictionary,
// the dictionary-less twin itself
extern "C" uint64_t lfx_encode_dict_bound(uint64_t n, const lfx_encode_opts *o, const lfx_schedule *s) {
    const uint64_t b = lfx_encode_bound(n, o, s);
    return b ? b + 4 : 0;
}
extern "C" int lfx_encode_dict_device(lfx_ctx *cc, int format, const lfx_encode_opts *o, const lfx_schedule *s, const lfx_dict *dict,
                                      const void *d_in, uint64_t n, void *d_out, uint64_t cap, uint64_t *out_len) try {
    if (!cc) return LFX_E_DEVICE;
    if (format != LFX_ZLIB && format != LFX_DEFLATE) return LFX_E_ARG;      // (gzip has no preset dictionary)
    if (dict && dict->c != reinterpret_cast<Ctx *>(cc)) return LFX_E_ARG;
    return encode_device_impl(cc, format, o, s, dict, d_in, n, d_out, cap, out_len);
} LFX_ABI_CATCH

// ---- batch encode: `count` independent streams in ONE launch set (thousands of small streams).
// Every stream is what lfx_encode_device would make of its bytes alone (same options, the schedule applied to each
// stream); the streams' chunks and blocks form one merged plan, so that the match / parse / Huffman / pack kernels see
// thousands of chunks at once instead of one launch set per 64 KiB.
static int encode_batch_impl(lfx_ctx *cc, int format, const lfx_encode_opts *o, const lfx_schedule *s, const lfx_dict *dict,
                             uint32_t count, const void *d_in, const uint64_t *in_off, const uint64_t *in_len, void *d_out,
                             const uint64_t *out_off, const uint64_t *out_cap, uint64_t *out_len, int32_t *status) {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    if (format < 0 || format > 2 || (count && (!in_off || !in_len || !out_off || !out_cap))) return LFX_E_ARG;
    EncodeSpec sp;
    int rc = encode_spec(format, o, &sp);
    if (rc) { c->set_error("option outside the reference's domain"); return rc; }
    if ((rc = served(c, dict ? ENC_DICT_BATCH : ENC_BATCH, sp, dict))) return rc;
    std::vector<uint8_t> hdr;
    if ((rc = container_header(format, sp.o, hdr))) { c->set_error("bad container options"); return rc; }
    if (dict) dict_header(format, dict, hdr);
    if (!count) return LFX_OK;
    // ---- the merged plan: every stream planned alone, its descriptors shifted into the shared index spaces
    Plan plan;
    std::vector<BatchStream> streams(count);
    uint64_t in_extent = 0, out_lo = ~0ull, out_hi = 0;
    for (uint32_t i = 0; i < count; i++) {
        if (out_off[i] & 3) { c->set_error("output offsets must be 4-byte aligned"); return LFX_E_ARG; }
        Planner pl(sp.plan);
        apply_schedule(pl, s, in_len[i]);
        Plan &p = pl.finish();
        if (dict) dict_prime(dict, p);
        streams[i] = BatchStream{in_off[i], in_len[i], out_off[i], out_cap[i], (uint32_t)plan.blocks.size(), (uint32_t)p.blocks.size()};
        plan.append(p, in_off[i]);
        in_extent = std::max(in_extent, in_off[i] + in_len[i]);
        out_lo = std::min(out_lo, out_off[i]);
        out_hi = std::max(out_hi, out_off[i] + out_cap[i]);
    }
    {
        // the streams are OR-ed into their ranges (pack kernel): two streams in one range would garble each other silently
        std::vector<uint32_t> order(count);
        for (uint32_t i = 0; i < count; i++) order[i] = i;
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return out_off[a] < out_off[b]; });
        for (uint32_t k = 0; k + 1 < count; k++)
            if (out_off[order[k]] + out_cap[order[k]] > out_off[order[k + 1]]) {
                c->set_error("the output ranges of two streams overlap");
                return LFX_E_ARG;
            }
    }
    std::vector<uint64_t> h_len;
    std::vector<int32_t> h_status;
    EncodeResult res{};
    const BatchCall call{format, streams, hdr, (const uint8_t *)d_in, in_extent, (uint8_t *)d_out, out_lo, out_hi, dict};
    if ((rc = encode_batch(c, plan, sp, call, h_len, h_status, res))) return rc;
    for (uint32_t i = 0; i < count; i++) {
        if (status) status[i] = res.status ? h_status[i] : LFX_OK;     // (a voided call: non-zero for exactly the streams that were too small)
        if (out_len) out_len[i] = res.status ? 0 : h_len[i];
    }
    if (res.status) {
        c->set_error("output capacity of a stream too small (status[] says which): the call is void, the output span holds no stream");
        return LFX_E_NOSPACE;
    }
    return LFX_OK;
}
extern "C" int lfx_encode_batch_device(lfx_ctx *cc, int format, const lfx_encode_opts *o, const lfx_schedule *s, uint32_t count,
                                       const void *d_in, const uint64_t *in_off, const uint64_t *in_len, void *d_out,
                                       const uint64_t *out_off, const uint64_t *out_cap, uint64_t *out_len, int32_t *status) try {
    return encode_batch_impl(cc, format, o, s, nullptr, count, d_in, in_off, in_len, d_out, out_off, out_cap, out_len, status);
} LFX_ABI_CATCH
extern "C" int lfx_encode_batch_dict_device(lfx_ctx *cc, int format, const lfx_encode_opts *o, const lfx_schedule *s,
                                            const lfx_dict *dict, uint32_t count, const void *d_in, const uint64_t *in_off,
                                            const uint64_t *in_len, void *d_out, const uint64_t *out_off, const uint64_t *out_cap,
                                            uint64_t *out_len, int32_t *status) try {
    if (!cc) return LFX_E_DEVICE;
    if (format != LFX_ZLIB && format != LFX_DEFLATE) return LFX_E_ARG;
    if (dict && dict->c != reinterpret_cast<Ctx *>(cc)) return LFX_E_ARG;
    return encode_batch_impl(cc, format, o, s, dict, count, d_in, in_off, in_len, d_out, out_off, out_cap, out_len, status);
} LFX_ABI_CATCH

// ---- the batch packed back to back: the batch call's merged plan and kernels; the streams' places come from
// a device scan of their sizes behind the Huffman kernel (lfx_batch_pack.hip) instead of from the caller
extern "C" int lfx_encode_batch_packed_device(lfx_ctx *cc, int format, const lfx_encode_opts *o, const lfx_schedule *s,
                                              const lfx_dict *dict, uint32_t count, const void *d_in, const uint64_t *in_off,
                                              const uint64_t *in_len, uint32_t align, void *d_out, uint64_t cap, uint64_t *out_off,
                                              uint64_t *out_len, uint64_t *total, void *d_table) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    if (format < 0 || format > 2 || (count && (!in_off || !in_len))) return LFX_E_ARG;
    if (dict && ((format != LFX_ZLIB && format != LFX_DEFLATE) || dict->c != c)) return LFX_E_ARG;
    if (!bpack_align_ok(align)) { c->set_error("align: a power of two in 1..4096"); return LFX_E_ARG; }
    if (((uintptr_t)d_out & 3) != 0) { c->set_error("output buffer must be 4-byte aligned"); return LFX_E_ARG; }
    if (!d_out && cap) { c->set_error("d_out: NULL with a capacity (the size query is d_out = NULL, cap = 0)"); return LFX_E_ARG; }
    if (((uintptr_t)d_table & 7) != 0) { c->set_error("d_table must be 8-byte aligned"); return LFX_E_ARG; }
    if (count > BPACK_MAX_COUNT) { c->set_error("count: too many streams for one call"); return LFX_E_ARG; }
    EncodeSpec sp;
    int rc = encode_spec(format, o, &sp);
    if (rc) { c->set_error("option outside the reference's domain"); return rc; }
    if ((rc = served(c, ENC_BATCH_PACKED, sp, dict))) return rc;
    std::vector<uint8_t> hdr;
    if ((rc = container_header(format, sp.o, hdr))) { c->set_error("bad container options"); return rc; }
    if (dict) dict_header(format, dict, hdr);
    if (total) *total = 0;
    if (!count) return LFX_OK;
    // ---- the merged plan, as in the batch call; every stream's bound on the way
    Plan plan;
    std::vector<BatchStream> streams(count);
    std::vector<uint64_t> bound(count);
    uint64_t in_extent = 0;
    for (uint32_t i = 0; i < count; i++) {
        Planner pl(sp.plan);
        apply_schedule(pl, s, in_len[i]);
        Plan &p = pl.finish();
        if (dict) dict_prime(dict, p);
        bound[i] = encode_bound_of(sp.o, in_len[i], p.blocks.size()) + (dict ? 4 : 0);
        streams[i] = BatchStream{in_off[i], in_len[i], 0, 0, (uint32_t)plan.blocks.size(), (uint32_t)p.blocks.size()};
        plan.append(p, in_off[i]);
        in_extent = std::max(in_extent, in_off[i] + in_len[i]);
    }
    uint64_t bound_sum = 0;
    if (!bpack_bound_sum(bound.data(), count, align, &bound_sum)) { c->set_error("in_len: the streams' bounds exceed 64 bits"); return LFX_E_ARG; }
    std::vector<uint64_t> pairs;
    EncodeResult res{};
    const BatchPackedCall call{format, streams, hdr, (const uint8_t *)d_in, in_extent, (uint8_t *)d_out, cap, std::min(cap, bound_sum),
                               align, dict, (uint64_t *)d_table};
    if ((rc = encode_batch_packed(c, plan, sp, call, pairs, res))) return rc;
    for (uint32_t i = 0; i < count; i++) {
        if (out_off) out_off[i] = pairs[2 * (size_t)i];
        if (out_len) out_len[i] = pairs[2 * (size_t)i + 1];
    }
    if (total) *total = res.out_bytes;
    if (res.status) {
        c->set_error("output capacity too small (*total says what the streams need): the call is void, no stream was written");
        return LFX_E_NOSPACE;
    }
    return LFX_OK;
} LFX_ABI_CATCH

// A host variant: `in` staged into d_io_in, run(len) — the device entry point on d_io_in / d_io_out — and len bytes back.
template <class Run>
static int encode_staged(Ctx *c, const void *in, uint64_t n, uint64_t out_bytes, void *out, uint64_t cap, uint64_t *out_len, Run run) {
    int rc;
    if ((rc = c->d_io_out.reserve(out_bytes))) return rc;
    // H2D / D2H at link rate (lfx_hostio.h): page-locked buffers (lfx_host_alloc) go to the DMA engine as they are, pageable
    // ones through page-locked slabs filled by a few threads
    if ((rc = stage_in(c, in, n))) return rc;
    uint64_t len = 0;
    rc = run(len);
    // (a page-locked `in` was only queued for DMA: no return before the stream has passed the copy, on any path)
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
    if (len > cap) { c->set_error("output capacity too small"); return LFX_E_NOSPACE; }
    if ((rc = device_to_host(c, out, c->d_io_out.p, len, c->stream))) { c->set_error("device to host copy failed"); return rc; }
    if (out_len) *out_len = len;
    return LFX_OK;
}

extern "C" int lfx_encode_host(lfx_ctx *cc, int format, const lfx_encode_opts *o, const lfx_schedule *s,
                               const void *in, uint64_t n, void *out, uint64_t cap, uint64_t *out_len) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    (void)hipSetDevice(c->device);
    uint64_t bound = lfx_encode_bound(n, o, s);
    if (bound == 0) { c->set_error("option outside the reference's domain"); return LFX_E_ARG; }
    return encode_staged(c, in, n, bound, out, cap, out_len, [&](uint64_t &len) {
        return lfx_encode_device(cc, format, o, s, c->d_io_in.p, n, c->d_io_out.p, bound & ~3ull, &len);
    });
} LFX_ABI_CATCH

extern "C" int lfx_encode_dict_host(lfx_ctx *cc, int format, const lfx_encode_opts *o, const lfx_schedule *s, const lfx_dict *dict,
                                    const void *in, uint64_t n, void *out, uint64_t cap, uint64_t *out_len) try {
    if (!cc) return LFX_E_DEVICE;
    if (format != LFX_ZLIB && format != LFX_DEFLATE) return LFX_E_ARG;
    if (!dict) return lfx_encode_host(cc, format, o, s, in, n, out, cap, out_len);
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    if (dict->c != c) return LFX_E_ARG;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    (void)hipSetDevice(c->device);
    const uint64_t bound = lfx_encode_dict_bound(n, o, s);
    if (bound == 0) { c->set_error("option outside the reference's domain"); return LFX_E_ARG; }
    return encode_staged(c, in, n, bound, out, cap, out_len, [&](uint64_t &len) {
        return lfx_encode_dict_device(cc, format, o, s, dict, c->d_io_in.p, n, c->d_io_out.p, bound & ~3ull, &len);
    });
} LFX_ABI_CATCH

// ---- training a preset dictionary from sample records: the checks and the record table are
// lfx_dict_train.h's, the kernels lfx_dict_train.hip's; one host wait, for the dictionary's length
static int dict_train_impl(Ctx *c, const DtrainPlan &pl, const uint8_t *d_samples, uint8_t *d_dict, uint64_t *dict_len) {
    (void)hipSetDevice(c->device);
    c->n_ev = 0;
    c->phase("start");
    const DtrainScratch w = dtrain_scratch(pl.n, pl.nrec(), pl.epochs, pl.k);
    if (int rc = c->d_dict_train.reserve(w.bytes)) { c->set_error("out of device memory for the trainer's scratch"); return rc; }
    uint8_t *d = (uint8_t *)c->d_dict_train.p;
    // the counters, the slots and the length word in one fill each; the record table (pl outlives the copies: the call
    // synchronises before it returns)
    if (hipMemsetAsync(d + w.freq, 0, 4ull << DTRAIN_F, c->stream) != hipSuccess ||
        hipMemsetAsync(d + w.slots, 0, 8ull * pl.epochs + 8, c->stream) != hipSuccess ||
        hipMemcpyAsync(d + w.pos, pl.pos.data(), 4ull * pl.pos.size(), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(d + w.off, pl.off.data(), 8ull * pl.off.size(), hipMemcpyHostToDevice, c->stream) != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        c->set_error("the trainer's uploads failed");
        return LFX_E_DEVICE;
    }
    int rc = launch_dict_train(c->stream, pl, w, d, d_samples, d_dict);
    c->phase("dict_train");
    uint64_t len = 0;
    if (!rc && hipMemcpyAsync(&len, d + w.out_len, 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = 1;
    if (hipStreamSynchronize(c->stream) != hipSuccess || rc) { c->set_error("the trainer's kernels failed"); return LFX_E_DEVICE; }
    *dict_len = len;
    return LFX_OK;
}

extern "C" int lfx_dict_train_device(lfx_ctx *cc, const void *d_samples, uint32_t count, const uint64_t *off, const uint64_t *len,
                                     uint32_t dict_size, uint32_t segment, void *d_dict, uint64_t cap, uint64_t *dict_len) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    DtrainPlan pl;
    const char *why;
    if (int rc = dtrain_check(count, off, len, dict_size, segment, d_dict, cap, &pl, &why)) { c->set_error(why); return rc; }
    if (pl.n && !d_samples) { c->set_error("the samples buffer is NULL"); return LFX_E_ARG; }
    uint64_t got = 0;
    if (pl.n)
        if (int rc = dict_train_impl(c, pl, (const uint8_t *)d_samples, (uint8_t *)d_dict, &got)) return rc;
    if (dict_len) *dict_len = got;
    return LFX_OK;
} LFX_ABI_CATCH

extern "C" int lfx_dict_train_host(lfx_ctx *cc, const void *samples, uint32_t count, const uint64_t *off, const uint64_t *len,
                                   uint32_t dict_size, uint32_t segment, void *dict, uint64_t cap, uint64_t *dict_len) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    DtrainPlan pl;
    const char *why;
    if (int rc = dtrain_check(count, off, len, dict_size, segment, dict, cap, &pl, &why)) { c->set_error(why); return rc; }
    if (pl.n && !samples) { c->set_error("the samples buffer is NULL"); return LFX_E_ARG; }
    uint64_t got = 0;
    if (pl.n) {
        (void)hipSetDevice(c->device);
        // the bytes from the first record's start to the last one's end go up (gaps between records with them); the table's
        // offsets move with them
        int rc;
        if ((rc = c->d_io_out.reserve(dict_size))) return rc;
        if ((rc = stage_in(c, (const uint8_t *)samples + pl.extent_lo, pl.extent_hi - pl.extent_lo))) return rc;
        for (uint64_t &o : pl.off) o -= pl.extent_lo;
        // (a page-locked `samples` was only queued for DMA: no return before the stream has passed the copy, on any path)
        if ((rc = dict_train_impl(c, pl, (const uint8_t *)c->d_io_in.p, (uint8_t *)c->d_io_out.p, &got))) { (void)hipStreamSynchronize(c->stream); return rc; }
        if ((rc = device_to_host(c, dict, c->d_io_out.p, got, c->stream))) { c->set_error("device to host copy failed"); return rc; }
    }
    if (dict_len) *dict_len = got;
    return LFX_OK;
} LFX_ABI_CATCH

// ---- the byte-shuffle filter: the tile list and the range check are lfx_shuffle.h's, the kernels
// lfx_shuffle.hip's; the record table and the tile list go up, one launch, one host wait
static int shuffle_impl(Ctx *c, int dir, uint32_t s, const std::vector<ShufRec> &recs, const void *d_in, void *d_out) {
    bool any = false;
    for (const ShufRec &r : recs) {
        if (r.in_off + r.len < r.len || r.out_off + r.len < r.len) { c->set_error("a record's offset plus its length exceeds 64 bits"); return LFX_E_ARG; }
        any = any || r.len;
    }
    if (!any) return LFX_OK;
    if (!d_in || !d_out) { c->set_error("a buffer is NULL"); return LFX_E_ARG; }
    if (!shuf_ranges_ok((uint32_t)recs.size(), recs.data(), (uint64_t)(uintptr_t)d_in, (uint64_t)(uintptr_t)d_out)) {
        c->set_error("a record's input meets an output range, or two output ranges meet: there is no in-place form");
        return LFX_E_ARG;
    }
    std::vector<ShufItem> items;
    if (!shuf_build_items((uint32_t)recs.size(), recs.data(), s, items)) { c->set_error("too many tiles for one call"); return LFX_E_ARG; }
    (void)hipSetDevice(c->device);
    c->n_ev = 0;
    c->phase("start");
    const size_t rec_bytes = sizeof(ShufRec) * recs.size(), item_bytes = sizeof(ShufItem) * items.size();
    if (int rc = c->d_shuffle.reserve(rec_bytes + item_bytes)) { c->set_error("out of device memory for the tile list"); return rc; }
    uint8_t *d = (uint8_t *)c->d_shuffle.p;
    // (recs and items outlive the copies: the call synchronises before it returns)
    if (hipMemcpyAsync(d, recs.data(), rec_bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(d + rec_bytes, items.data(), item_bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        c->set_error("the tile list's upload failed");
        return LFX_E_DEVICE;
    }
    const int rc = launch_shuffle(c->stream, dir, s, (const uint8_t *)d_in, (uint8_t *)d_out, (const ShufRec *)d, (const ShufItem *)(d + rec_bytes),
                                  (uint32_t)items.size());
    c->phase("shuffle");
    if (hipStreamSynchronize(c->stream) != hipSuccess || rc) { c->set_error("the shuffle kernel failed"); return LFX_E_DEVICE; }
    return LFX_OK;
}

static int shuffle_args(Ctx *c, int dir, uint32_t elem_size) {
    if (dir != LFX_SHUFFLE && dir != LFX_UNSHUFFLE) { c->set_error("dir: LFX_SHUFFLE or LFX_UNSHUFFLE"); return LFX_E_ARG; }
    if (elem_size < 1 || elem_size > SHUF_MAX_ELEM) { c->set_error("elem_size: 1..256"); return LFX_E_ARG; }
    return LFX_OK;
}

extern "C" int lfx_shuffle_device(lfx_ctx *cc, int dir, uint32_t elem_size, const void *d_in, uint64_t n, void *d_out) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    if (int rc = shuffle_args(c, dir, elem_size)) return rc;
    return shuffle_impl(c, dir, elem_size, {ShufRec{0, 0, n}}, d_in, d_out);
} LFX_ABI_CATCH

extern "C" int lfx_shuffle_batch_device(lfx_ctx *cc, int dir, uint32_t elem_size, uint32_t count, const void *d_in, const uint64_t *in_off,
                                        const uint64_t *len, const void *d_table, void *d_out, const uint64_t *out_off) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    if (int rc = shuffle_args(c, dir, elem_size)) return rc;
    if ((in_off == nullptr) != (len == nullptr) || (in_off && d_table) || (count && !in_off && !d_table)) {
        c->set_error("the records' places: either in_off and len (host) or d_table (device), not both");
        return LFX_E_ARG;
    }
    if (d_table && out_off) { c->set_error("out_off: NULL with d_table (the output takes the input offsets)"); return LFX_E_ARG; }
    if (((uintptr_t)d_table & 7) != 0) { c->set_error("d_table must be 8-byte aligned"); return LFX_E_ARG; }
    if (!count) return LFX_OK;
    std::vector<ShufRec> recs(count);
    if (d_table) {
        (void)hipSetDevice(c->device);
        std::vector<uint64_t> tab(2 * (size_t)count);
        if (hipMemcpyAsync(tab.data(), d_table, 16ull * count, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess) { c->set_error("the table's download failed"); return LFX_E_DEVICE; }
        for (uint32_t i = 0; i < count; i++) recs[i] = ShufRec{tab[2 * (size_t)i], tab[2 * (size_t)i], tab[2 * (size_t)i + 1]};
    } else {
        for (uint32_t i = 0; i < count; i++) recs[i] = ShufRec{in_off[i], out_off ? out_off[i] : in_off[i], len[i]};
    }
    return shuffle_impl(c, dir, elem_size, recs, d_in, d_out);
} LFX_ABI_CATCH

extern "C" int lfx_shuffle_host(lfx_ctx *cc, int dir, uint32_t elem_size, const void *in, uint64_t n, void *out) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    if (int rc = shuffle_args(c, dir, elem_size)) return rc;
    if (!n) return LFX_OK;
    if (!in || !out) { c->set_error("a buffer is NULL"); return LFX_E_ARG; }
    (void)hipSetDevice(c->device);
    int rc;
    if ((rc = c->d_io_out.reserve(n))) return rc;
    if ((rc = stage_in(c, in, n))) return rc;
    // (a page-locked `in` was only queued for DMA: no return before the stream has passed the copy, on any path)
    if ((rc = shuffle_impl(c, dir, elem_size, {ShufRec{0, 0, n}}, c->d_io_in.p, c->d_io_out.p))) { (void)hipStreamSynchronize(c->stream); return rc; }
    if ((rc = device_to_host(c, out, c->d_io_out.p, n, c->stream))) { c->set_error("device to host copy failed"); return rc; }
    return LFX_OK;
} LFX_ABI_CATCH

// ---- members encode: one buffer as back-to-back gzip members / BGZF, packed at their final offsets ----------
static const uint8_t BGZF_EXTRA[6] = {0x42, 0x43, 0x02, 0x00, 0x00, 0x00};   // 'B' 'C', SLEN 2, BSIZE (per member, on the device)
static const uint32_t BGZF_MAX_MEMBER = 65536, BGZF_EOF_LEN = 28;
static const uint64_t BGZF_MAX_SLICE = 65505;                               // 18 + 5 + 65505 + 8 = 65536: one stored block still fits
// the options and the schedule of a members call: *why names the field that is out of its domain
static int members_check(uint64_t member_size, uint32_t flags, const lfx_encode_opts *o, const lfx_schedule *s, EncodeSpec *sp,
                         const char **why) {
    const int domain = encode_spec(LFX_GZIP, o, sp);
    lfx_encode_opts *d = &sp->o;
    if (flags & ~(uint32_t)LFX_MEMBERS_BGZF) { *why = "flags: unknown bit"; return LFX_E_ARG; }
    if (member_size == 0) { *why = "member_size: must not be 0"; return LFX_E_ARG; }
    if (domain) { *why = "block_size / max_length: outside the reference's domain"; return LFX_E_ARG; }
    if (int rc = encode_served(ENC_MEMBERS, *sp, DICT_NONE, why)) return rc;
    if (!(flags & LFX_MEMBERS_BGZF)) return LFX_OK;
    if (member_size > BGZF_MAX_SLICE) { *why = "member_size: a BGZF member holds at most 65505 bytes"; return LFX_E_ARG; }
    if (d->extra) { *why = "extra: BGZF carries its own BC subfield"; return LFX_E_ARG; }
    if (d->filename) { *why = "filename: a BGZF header is 18 bytes"; return LFX_E_ARG; }
    if (d->comment) { *why = "comment: a BGZF header is 18 bytes"; return LFX_E_ARG; }
    if (d->hcrc) { *why = "hcrc: a BGZF header is 18 bytes"; return LFX_E_ARG; }
    if (s && s->kind != LFX_SCHED_SINGLE) { *why = "schedule: BGZF needs LFX_SCHED_SINGLE"; return LFX_E_ARG; }
    // block_size <= member_size closes the member with an empty second block: the stored form is then 36 + member_size bytes
    if (d->block_size <= member_size && member_size + 36 > BGZF_MAX_MEMBER) {
        *why = "block_size: with block_size <= member_size a BGZF member holds at most 65500 bytes";
        return LFX_E_ARG;
    }
    d->extra = BGZF_EXTRA;
    d->extra_len = sizeof BGZF_EXTRA;
    return LFX_OK;
}
// slices of a members call: `full` of member_size bytes, then one of `last` bytes when have_last
struct MemberSlices { uint64_t full, last; bool have_last; uint64_t count() const { return full + (have_last ? 1 : 0); } };
static MemberSlices member_slices(uint64_t n, uint64_t member_size, uint32_t flags) {
    MemberSlices m{n / member_size, n % member_size, n % member_size != 0};
    if (n == 0 && !(flags & LFX_MEMBERS_BGZF)) m.have_last = true;     // one member of no bytes (BGZF: the marker alone)
    return m;
}

extern "C" uint64_t lfx_encode_members_bound(uint64_t n, uint64_t member_size, uint32_t flags, const lfx_encode_opts *o,
                                             const lfx_schedule *s) try {
    EncodeSpec sp;
    const char *why = nullptr;
    if (members_check(member_size, flags, o, s, &sp, &why)) return 0;
    const bool bgzf = (flags & LFX_MEMBERS_BGZF) != 0;
    const MemberSlices ms = member_slices(n, member_size, flags);
    // (BGZF: the caller's options, without the BC subfield — lfx_encode_bound leaves 64 bytes for the 10 fixed ones of a header)
    auto term = [&](uint64_t len) { const uint64_t b = lfx_encode_bound(len, o, s); return bgzf ? std::min<uint64_t>(b, BGZF_MAX_MEMBER) : b; };
    return (ms.full ? ms.full * term(member_size) : 0) + (ms.have_last ? term(ms.last) : 0) + (bgzf ? BGZF_EOF_LEN : 0);
} catch (...) { return 0; }

// The merged plan of a members call: a full slice and the last slice are planned once each (the schedule applies to a slice
// alone), the full slice's descriptors are repeated, shifted into the shared index spaces.  bpm[2]: blocks of a full and of
// the last member.  *why names what is out of the domain.
static int members_plan(const PlanOpts &po, const lfx_schedule *s, const MemberSlices &ms, uint64_t member_size, bool bgzf, Plan &plan,
                        uint32_t bpm[2], const char **why) {
    Plan pfull, plast;
    if (ms.full) { Planner pl(po); apply_schedule(pl, s, member_size); pfull = std::move(pl.finish()); }
    if (ms.have_last) { Planner pl(po); apply_schedule(pl, s, ms.last); plast = std::move(pl.finish()); }
    if (bgzf) {
        // the stored form of a member (no_compression = 1) must have the compressed form's blocks, byte for byte the same
        // ranges: the device turns one into the other by the blocks' type alone.  (One write of at most 65505 bytes: a block
        // holding all of it, and an empty final one behind it when block_size <= the slice — in both forms.)
        PlanOpts ps = po;
        ps.no_compression = true;
        for (int k = 0; k < 2; k++) {
            if (k == 0 ? !ms.full : !ms.have_last) continue;
            const Plan &pc = k == 0 ? pfull : plast;
            Planner pl(ps);
            apply_schedule(pl, s, k == 0 ? member_size : ms.last);
            const Plan &pr = pl.finish();
            bool same = pr.blocks.size() == pc.blocks.size();
            for (size_t b = 0; same && b < pr.blocks.size(); b++)
                same = pr.blocks[b].in_off == pc.blocks[b].in_off && pr.blocks[b].in_len == pc.blocks[b].in_len &&
                       pr.blocks[b].final == pc.blocks[b].final && pr.blocks[b].align_after == pc.blocks[b].align_after;
            if (!same) { *why = "block_size: the stored form of a member has other blocks than the compressed form"; return LFX_E_UNSUPPORTED; }
        }
    }
    if ((uint64_t)ms.full * pfull.chunks.size() + plast.chunks.size() > 0xFFFFFFF0ull ||
        (uint64_t)ms.full * pfull.blocks.size() + plast.blocks.size() > 0xFFFFFFF0ull ||
        (uint64_t)ms.full * pfull.n_segs + plast.n_segs > 0xFFFFFFF0ull) {
        *why = "member_size: too many blocks for one call";
        return LFX_E_ARG;
    }
    plan.chunks.reserve(ms.full * pfull.chunks.size() + plast.chunks.size());
    plan.blocks.reserve(ms.full * pfull.blocks.size() + plast.blocks.size());
    for (uint64_t m = 0; m < ms.full; m++) plan.append(pfull, m * member_size);
    if (ms.have_last) plan.append(plast, ms.full * member_size);
    bpm[0] = (uint32_t)(ms.full ? pfull.blocks.size() : plast.blocks.size());
    bpm[1] = (uint32_t)(ms.have_last ? plast.blocks.size() : pfull.blocks.size());
    return LFX_OK;
}

extern "C" int lfx_encode_members_device(lfx_ctx *cc, const lfx_encode_opts *o, const lfx_schedule *s, uint64_t member_size,
                                         uint32_t flags, const void *d_in, uint64_t n, void *d_out, uint64_t cap, uint64_t *out_len,
                                         lfx_member *members, uint32_t max_members, uint32_t *n_members) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    if (out_len) *out_len = 0;
    if (n_members) *n_members = 0;
    EncodeSpec sp;
    const char *why = nullptr;
    int rc = members_check(member_size, flags, o, s, &sp, &why);
    if (rc) { c->set_error(why); return rc; }
    if (((uintptr_t)d_out & 3) != 0) { c->set_error("output buffer must be 4-byte aligned"); return LFX_E_ARG; }
    const bool bgzf = (flags & LFX_MEMBERS_BGZF) != 0;
    std::vector<uint8_t> hdr;
    if ((rc = container_header(LFX_GZIP, sp.o, hdr))) { c->set_error("extra: longer than 65535 bytes"); return rc; }
    const MemberSlices ms = member_slices(n, member_size, flags);
    if (ms.count() >= 0xFFFFFFFFull) { c->set_error("member_size: more than 2^32 - 2 members"); return LFX_E_ARG; }
    const uint32_t count = (uint32_t)ms.count();
    (void)hipSetDevice(c->device);
    hipStream_t st = c->stream;
    if (!count) {
        // BGZF of no bytes: the end-of-file marker alone
        static const uint8_t eof[BGZF_EOF_LEN] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43,
                                                  0x02, 0,    0x1b, 0,    3, 0, 0, 0, 0, 0,    0,    0, 0,    0};
        if (cap < BGZF_EOF_LEN) { c->set_error("output capacity too small"); return LFX_E_NOSPACE; }
        HIP_TRY(hipMemcpyAsync(d_out, eof, BGZF_EOF_LEN, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (out_len) *out_len = BGZF_EOF_LEN;
        return LFX_OK;
    }
    Plan plan;
    uint32_t bpm[2];
    if ((rc = members_plan(sp.plan, s, ms, member_size, bgzf, plan, bpm, &why))) { c->set_error(why); return rc; }
    MembersGeom g{};
    g.n = n; g.member_size = member_size; g.count = count;
    g.bpm = bpm[0]; g.bpm_last = bpm[1];
    g.hdr_len = (uint32_t)hdr.size(); g.bgzf = bgzf ? 1u : 0u;
    const uint64_t bound = lfx_encode_members_bound(n, member_size, flags, o, s);
    EncodeResult res{};
    const MembersCall call{g, hdr, (const uint8_t *)d_in, (uint8_t *)d_out, cap, std::min(cap, bound), members,
                           members ? std::min(count, max_members) : 0};
    if ((rc = encode_members(c, plan, sp, call, res))) return rc;
    if (n_members) *n_members = count;
    if (res.status) { c->set_error("output capacity too small"); return LFX_E_NOSPACE; }
    if (out_len) *out_len = res.out_bytes;
    return LFX_OK;
} LFX_ABI_CATCH

extern "C" int lfx_encode_members_host(lfx_ctx *cc, const lfx_encode_opts *o, const lfx_schedule *s, uint64_t member_size,
                                       uint32_t flags, const void *in, uint64_t n, void *out, uint64_t cap, uint64_t *out_len,
                                       lfx_member *members, uint32_t max_members, uint32_t *n_members) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    (void)hipSetDevice(c->device);
    if (out_len) *out_len = 0;
    if (n_members) *n_members = 0;
    EncodeSpec sp;
    const char *why = nullptr;
    int rc = members_check(member_size, flags, o, s, &sp, &why);
    if (rc) { c->set_error(why); return rc; }
    const uint64_t bound = lfx_encode_members_bound(n, member_size, flags, o, s);
    return encode_staged(c, in, n, std::max<uint64_t>(bound, 4), out, cap, out_len, [&](uint64_t &len) {
        return lfx_encode_members_device(cc, o, s, member_size, flags, c->d_io_in.p, n, c->d_io_out.p, std::min(cap, bound), &len, members,
                                         max_members, n_members);
    });
} LFX_ABI_CATCH

extern "C" int lfx_members_gzi(const lfx_member *members, uint32_t n_members, void *buf, uint64_t cap, uint64_t *len) {
    if (n_members && !members) return LFX_E_ARG;
    const uint64_t pairs = n_members ? n_members - 1 : 0, need = 8 + 16 * pairs;
    if (len) *len = need;
    if (cap < need || !buf) return cap < need ? LFX_E_NOSPACE : LFX_E_ARG;
    uint8_t *p = (uint8_t *)buf;
    auto put64 = [&](uint64_t v) { for (int i = 0; i < 8; i++) *p++ = (uint8_t)(v >> (8 * i)); };
    put64(pairs);
    for (uint32_t i = 1; i < n_members; i++) { put64(members[i].out_off); put64(members[i].in_off); }
    return LFX_OK;
}

// ---- sharded encode -------------------------------------------------------------------------
// Where lfx_encode_shard_emit will write: zero-filled on the side stream NOW, beside the match kernel of the prepare call, as
// lfx_encode_device does for its own output (the pack kernels OR into zeros; on the main stream the fill of a 130 MB shard was
// 0.07 ms in front of them).  (NULL, 0): wait for a fill in flight and forget it — the emit call is not going to come.
extern "C" int lfx_encode_shard_prezero(lfx_ctx *cc, void *d_out, uint64_t cap) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    c->prezero.settle();
    if (!d_out || ((uintptr_t)d_out & 3) != 0 || cap < 16) return LFX_OK;
    (void)hipSetDevice(c->device);
    c->prezero.start(d_out, cap / 4 * 4);
    return LFX_OK;
} LFX_ABI_CATCH

extern "C" int lfx_encode_shard_prepare(lfx_ctx *cc, int format, const lfx_encode_opts *o, const lfx_schedule *s,
                                        const void *d_in, uint64_t n, int is_first, int is_last,
                                        lfx_shard_info *info) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    EncodeSpec sp;
    int rc = encode_spec(format, o, &sp);
    if (rc) return rc;
    if ((rc = served(c, ENC_SHARD, sp))) return rc;
    Planner pl(sp.plan);
    apply_schedule(pl, s, n);
    Plan *plan;
    if (is_last) {
        plan = &pl.finish();
    } else {
        // a non-last shard must end on a block boundary with nothing buffered: close the block
        // exactly as the stream would have (block_size reached) — otherwise the shards would not
        // concatenate to what one encoder emits
        plan = &pl.plan();
        Planner probe = pl;
        Plan &fin = probe.finish();
        if (fin.blocks.size() != plan->blocks.size() + 1 || fin.blocks.back().in_len != 0) {
            c->set_error("shard boundary is not a block boundary under this write schedule");
            return LFX_E_ARG;
        }
        plan->n_codes_cap = fin.n_codes_cap;
        plan->n_tiles = plan->chunks.empty() ? 0 : plan->chunks.back().tile_base + div_up(plan->chunks.back().len + 1, PACK_TILE);
    }
    c->shard_hdr.clear();
    if (is_first && (rc = container_header(format, sp.o, c->shard_hdr))) return rc;
    c->shard_format = format;
    c->shard_last = is_last != 0;
    hipStream_t st = c->stream;
    EncodeResult r{};
    rc = with_match_fallback(c, r, [&]() -> int {
        if (int rc2 = encode_prepare(c, *plan, sp, (const uint8_t *)d_in, n, 3)) return rc2;
        // total bits at bit phase 0 (compressed blocks only → independent of the phase)
        LAUNCH_TRY(launch_offsets(st, (const BlockDesc *)c->d_blocks.p, c->cur_nblocks, (const BlockCodes *)c->d_bc.p,
                                  0, ~0ull, (uint64_t *)c->d_block_start.p, (EncodeResult *)c->d_res.p));
        HIP_TRY(hipMemcpyAsync(c->h_res, c->d_res.p, sizeof(EncodeResult), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        r = *(EncodeResult *)c->h_res;
        return LFX_OK;
    });
    if (rc) return rc;
    // For the LAST shard the figure includes the final byte alignment as seen from phase 0; its true value depends on
    // the shard's start phase and is settled by emit().  Layouts only ever sum the bits of the shards in front of a
    // shard, so the last shard's own figure is informative.
    info->total_bits = r.end_bit;
    info->n_bytes = n;
    info->crc32 = r.crc32;
    info->adler32 = r.adler32;
    return LFX_OK;
} LFX_ABI_CATCH

extern "C" int lfx_encode_shard_emit(lfx_ctx *cc, uint64_t start_bit, uint32_t combined_check, uint64_t total_n,
                                     void *d_out, uint64_t cap, uint64_t *out_len) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    // d_out[0] is byte start_bit/8 of the member; a first shard carries the container header
    const uint64_t rel_start = c->shard_hdr.empty() ? (start_bit & 7) : start_bit;
    EncodeResult res;
    int rc = encode_emit(c, c->shard_format, c->shard_last, combined_check, false, total_n,
                         c->shard_hdr.data(), (uint32_t)c->shard_hdr.size(), rel_start, (uint8_t *)d_out, cap, &res);
    if (rc) return rc;
    if (out_len) *out_len = c->shard_last ? res.out_bytes : (res.end_bit + 7) / 8;
    return LFX_OK;
} LFX_ABI_CATCH

extern "C" int lfx_shard_place_device(lfx_ctx *cc, void *d_member, uint64_t cap, const void *d_part, uint64_t part_len,
                                      uint64_t start_bit, int is_first) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    (void)hipSetDevice(c->device);
    const uint64_t at = is_first ? 0 : start_bit / 8;
    if (at + part_len > cap) { c->set_error("member buffer too small"); return LFX_E_NOSPACE; }
    if (part_len == 0) return LFX_OK;
    uint8_t *dst = (uint8_t *)d_member + at;
    const uint8_t *src = (const uint8_t *)d_part;
    const bool shared = !is_first && (start_bit & 7) != 0;      // the first byte also holds the last bits of the shard in front
    if (shared) {
        LAUNCH_TRY(launch_or_byte(c->stream, dst, src));
        if (part_len > 1) HIP_TRY(hipMemcpyAsync(dst + 1, src + 1, part_len - 1, hipMemcpyDeviceToDevice, c->stream));
    } else {
        HIP_TRY(hipMemcpyAsync(dst, src, part_len, hipMemcpyDeviceToDevice, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return LFX_OK;
} LFX_ABI_CATCH

// ------------------------------------------------------------------------------------------------
// Lz77Encode plug-in
struct lfx_lz77 {
    Ctx *c;
    uint32_t window, max_len;
    std::vector<uint8_t> buf;
    DevBuf d_in;
    std::vector<uint32_t> host_codes;
};
extern "C" lfx_lz77 *lfx_lz77_new(lfx_ctx *cc, uint32_t window_size, uint32_t max_length, int *status) try {
    if (!cc) { if (status) *status = LFX_E_DEVICE; return nullptr; }
    if (max_length < 3) { if (status) *status = LFX_E_ARG; return nullptr; }
    lfx_lz77 *z = new lfx_lz77();
    z->c = reinterpret_cast<Ctx *>(cc);
    z->window = std::min(window_size, MAX_WINDOW);
    z->max_len = std::min(max_length, MAX_LENGTH);
    if (status) *status = LFX_OK;
    return z;
} LFX_ABI_CATCH_NEW
extern "C" int lfx_lz77_flush(lfx_lz77 *z, lfx_sink_cb sink, void *user) try {
    // DefaultLz77Encoder::flush default.rs:69-109 — one chunk through match + parse
    Ctx *c = z->c;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    (void)hipSetDevice(c->device);
    const uint64_t n = z->buf.size();
    if (n == 0) return LFX_OK;
    EncodeSpec sp;                 // DefaultLz77Encoder: the default options with the handle's window and length
    (void)encode_spec(LFX_DEFLATE, nullptr, &sp);
    sp.plan.window_size = z->window;
    sp.plan.max_length = z->max_len;
    Plan plan;
    ChunkDesc ch{};
    ch.len = n;
    ch.n_seg = (uint32_t)div_up(n, PARSE_SEG);
    plan.n_segs = ch.n_seg;
    plan.n_vis = (uint64_t)ch.n_seg * 64;
    plan.chunks.push_back(ch);
    BlockDesc bd{};
    bd.type = BT_DYNAMIC;
    bd.n_chunks = 1;
    plan.blocks.push_back(bd);
    plan.n_codes_cap = n + 1;
    plan.n_tiles = div_up(n + 1, PACK_TILE);
    int rc;
    if ((rc = z->d_in.reserve(std::max<uint64_t>(n, 4)))) return rc;
    HIP_TRY(hipMemcpyAsync(z->d_in.p, z->buf.data(), n, hipMemcpyHostToDevice, c->stream));
    EncodeResult r{};
    rc = with_match_fallback(c, r, [&]() -> int {
        if (int rc2 = encode_prepare(c, plan, sp, (const uint8_t *)z->d_in.p, n, 0)) return rc2;
        HIP_TRY(hipMemcpy(&r, c->d_res.p, sizeof r, hipMemcpyDeviceToHost));
        return LFX_OK;
    });
    if (rc) return rc;
    uint32_t nc = 0;
    HIP_TRY(hipMemcpy(&nc, c->d_ncodes.p, 4, hipMemcpyDeviceToHost));
    z->host_codes.resize(nc);
    if (nc) HIP_TRY(hipMemcpy(z->host_codes.data(), c->d_codes.p, 4ull * nc, hipMemcpyDeviceToHost));
    z->buf.clear();  // default.rs:108
    if (sink && nc) sink(user, z->host_codes.data(), nc);
    return LFX_OK;
} LFX_ABI_CATCH
extern "C" int lfx_lz77_encode(lfx_lz77 *z, const uint8_t *buf, size_t len, lfx_sink_cb sink, void *user) try {
    z->buf.insert(z->buf.end(), buf, buf + len);                     // default.rs:64
    if (z->buf.size() >= (size_t)z->window * 8) return lfx_lz77_flush(z, sink, user);  // default.rs:65-67
    return LFX_OK;
} LFX_ABI_CATCH
extern "C" uint32_t lfx_lz77_window_size(const lfx_lz77 *z) { return z->window; }
extern "C" int lfx_lz77_compression_level(const lfx_lz77 *) { return LFX_LEVEL_BALANCE; }
extern "C" void lfx_lz77_free(lfx_lz77 *z) {
    if (!z) return;
    (void)hipSetDevice(z->c->device);
    z->d_in.release();
    delete z;
}

// ------------------------------------------------------------------------------------------------
// test hooks (include/lfx_testhooks.h) for the CPU test-suite: run the SAME host/device-shared code on the host.
// Not a product path (no compression work can be reached through them).
extern "C" int lfx_debug_huff_block(const uint32_t *hist320, uint32_t type, uint32_t *lit288, uint32_t *dist32,
                                    uint32_t *hdr160, uint32_t *hdr_bits, uint64_t *body_bits) try {
    static HuffScratch S;
    static BlockCodes bc;
    memset(&bc, 0, sizeof bc);
    huff_block_build(hist320, type, &bc, S, 0, 1);
    memcpy(lit288, bc.lit, sizeof bc.lit);
    memcpy(dist32, bc.dist, sizeof bc.dist);
    memcpy(hdr160, bc.hdr, sizeof bc.hdr);
    *hdr_bits = bc.hdr_bits;
    *body_bits = bc.body_bits;
    return 0;
} LFX_ABI_CATCH
extern "C" int lfx_debug_plan(int format, const lfx_encode_opts *o, const lfx_schedule *s, uint64_t n,
                              uint64_t *chunk_out /* in_off,len,block,flags per chunk */, size_t max_chunks,
                              size_t *n_chunks, uint64_t *block_out /* type,final,first,n,in_off,in_len */,
                              size_t max_blocks, size_t *n_blocks) try {
    EncodeSpec sp;
    if (encode_spec(format, o, &sp)) return LFX_E_ARG;
    Planner pl(sp.plan);
    apply_schedule(pl, s, n);
    Plan &p = pl.finish();
    *n_chunks = p.chunks.size();
    *n_blocks = p.blocks.size();
    for (size_t i = 0; i < p.chunks.size() && i < max_chunks; i++) {
        chunk_out[4 * i] = p.chunks[i].in_off; chunk_out[4 * i + 1] = p.chunks[i].len;
        chunk_out[4 * i + 2] = p.chunks[i].block; chunk_out[4 * i + 3] = p.chunks[i].flags;
    }
    for (size_t i = 0; i < p.blocks.size() && i < max_blocks; i++) {
        block_out[6 * i] = p.blocks[i].type; block_out[6 * i + 1] = p.blocks[i].final;
        block_out[6 * i + 2] = p.blocks[i].first_chunk; block_out[6 * i + 3] = p.blocks[i].n_chunks;
        block_out[6 * i + 4] = p.blocks[i].in_off; block_out[6 * i + 5] = p.blocks[i].in_len;
    }
    return 0;
} LFX_ABI_CATCH
// the same plan, but collected the way the stream encoder does: closed blocks are taken out after every
// `take_every`-th event and the remainder is rebased; the pieces are stitched back together here
extern "C" int lfx_debug_plan_incremental(int format, const lfx_encode_opts *o, const lfx_schedule *s, uint64_t n,
                                          uint32_t take_every, uint64_t *chunk_out, size_t max_chunks, size_t *n_chunks,
                                          uint64_t *block_out, size_t max_blocks, size_t *n_blocks) try {
    EncodeSpec sp;
    if (encode_spec(format, o, &sp) || !s || s->kind != LFX_SCHED_LIST) return LFX_E_ARG;
    Planner pl(sp.plan);
    Plan all;
    uint64_t byte0 = 0;
    auto stitch = [&](Plan &p, uint64_t bytes) { all.append(p, byte0); byte0 += bytes; };
    const std::vector<ChunkDesc> &chunks = all.chunks;
    const std::vector<BlockDesc> &blocks = all.blocks;
    uint64_t used = 0;
    for (size_t i = 0; i < s->n_writes; i++) {
        if (s->writes[i] == LFX_SCHED_FLUSH) pl.flush();
        else { const uint64_t w = std::min(s->writes[i], n - used); pl.write(w); used += w; }
        if (take_every && (i + 1) % take_every == 0) {
            const uint64_t cut = pl.closed_bytes();
            Plan p = pl.take_closed();
            stitch(p, cut);
        }
    }
    if (used < n) pl.write(n - used);
    Plan &fin = pl.finish();
    stitch(fin, 0);
    *n_chunks = chunks.size();
    *n_blocks = blocks.size();
    for (size_t i = 0; i < chunks.size() && i < max_chunks; i++) {
        chunk_out[4 * i] = chunks[i].in_off; chunk_out[4 * i + 1] = chunks[i].len;
        chunk_out[4 * i + 2] = chunks[i].block; chunk_out[4 * i + 3] = chunks[i].flags;
    }
    for (size_t i = 0; i < blocks.size() && i < max_blocks; i++) {
        block_out[6 * i] = blocks[i].type; block_out[6 * i + 1] = blocks[i].final;
        block_out[6 * i + 2] = blocks[i].first_chunk; block_out[6 * i + 3] = blocks[i].n_chunks;
        block_out[6 * i + 4] = blocks[i].in_off; block_out[6 * i + 5] = blocks[i].in_len;
    }
    return 0;
} LFX_ABI_CATCH
// the types block_choose_kernel left the blocks of the context's last encode_prepare with (LFX_HUFFMAN_AUTO)
extern "C" int lfx_debug_block_choices(lfx_ctx *cc, uint8_t *out, size_t max_blocks, size_t *n_blocks) try {
    if (!cc || !n_blocks) return LFX_E_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    (void)hipSetDevice(c->device);
    *n_blocks = c->n_choices;
    const size_t n = std::min<size_t>(c->n_choices, max_blocks);
    if (n && !out) return LFX_E_ARG;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (n) HIP_TRY(hipMemcpy(out, c->d_choice.p, n, hipMemcpyDeviceToHost));
    return LFX_OK;
} LFX_ABI_CATCH
// the block every block of the context's last encode_prepare ended up in (block_merge)
extern "C" int lfx_debug_block_merges(lfx_ctx *cc, uint32_t *out, size_t max_blocks, size_t *n_blocks) try {
    if (!cc || !n_blocks) return LFX_E_ARG;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    (void)hipSetDevice(c->device);
    *n_blocks = c->n_merges;
    const size_t n = std::min<size_t>(c->n_merges, max_blocks);
    if (n && !out) return LFX_E_ARG;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (n) HIP_TRY(hipMemcpy(out, c->d_merge.p, 4 * n, hipMemcpyDeviceToHost));
    return LFX_OK;
} LFX_ABI_CATCH
extern "C" void lfx_debug_symbols(uint32_t length, uint32_t distance, uint32_t *out6) {
    out6[0] = len_symbol(length, out6[1], out6[2]);
    out6[3] = dist_symbol(distance, out6[4], out6[5]);
}
