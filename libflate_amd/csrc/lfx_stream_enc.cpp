// lfx_stream_enc.cpp — the stream encoder on the GPU (C ABI: lfx_encoder_*): the state machine of lfx_stream_enc.h over
// page-locked buffers, with the encode core (encode_prepare / encode_emit) as its batch backend.
#include "../../include/lfx.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>

#include "lfx_encode_int.h"
#include "lfx_hostio.h"
#include "lfx_stream_enc.h"
#include "lfx_abi_guard.h"

using namespace lfx;

namespace {

// One batch in flight on the context's stream.  The only part of the encoder that takes the context's lock and its device.
struct GpuBatches {
    Ctx *c = nullptr;
    int format = 0;
    const EncodeSpec *spec = nullptr;   // the encoder's (StreamEnc::spec)
    const lfx_dict *dict = nullptr;     // the encoder's preset dictionary (lfx_encoder_new_dict): for the batch that is `primed`, no other
    DevBuf d_in, d_out;
    PinVec h_out;                       // a batch's output lands here (page-locked) and goes to the sink from here: no copy between
    PinVec h_res;                       // result slot + the shared byte
    hipEvent_t ev_out = nullptr, ev_small = nullptr;
    EncBatch cur;                       // the batch in flight, its plan kept: a match violation runs it again

    // prepare + emit of `cur` over d_in into d_out, the bits behind the partial byte the batch before left.  The container
    // trailer is written by the host (the checksum spans batches).  async_slot: as encode_emit's — the call returns without waiting.
    int encode(EncodeResult *res, EncodeResult *async_slot, std::string &err) {
        const uint8_t prefix[1] = {cur.carry};
        const HostCodes hc{cur.codes, cur.n_codes, cur.chunk_codes};
        int rc = encode_prepare(c, cur.plan, *spec, (const uint8_t *)d_in.p, cur.n, ck_mode_of(format), cur.coded ? &hc : nullptr,
                                cur.primed ? dict : nullptr);
        if (!rc) rc = encode_emit(c, LFX_DEFLATE, false, 0, true, 0, prefix, cur.carry_bits ? 1 : 0, cur.carry_bits, (uint8_t *)d_out.p,
                                  cur.bound & ~3ull, res, async_slot);
        if (rc) err = c->err;
        return rc;
    }
    int launch(EncBatch &b, std::string &err) {
        std::lock_guard<std::recursive_mutex> lock(c->mu);
        (void)hipSetDevice(c->device);
        if (!ev_out && (hipEventCreateWithFlags(&ev_out, hipEventDisableTiming) != hipSuccess ||
                        hipEventCreateWithFlags(&ev_small, hipEventDisableTiming) != hipSuccess)) return LFX_E_DEVICE;
        int rc;
        if ((rc = d_in.reserve(std::max<uint64_t>(b.n, 4)))) return rc;
        if ((rc = d_out.reserve(b.bound))) return rc;
        if (h_res.size() < 256) h_res.resize(256);
        cur = std::move(b);
        // H2D straight out of the page-locked input: one DMA transfer, reading until the batch is collected
        if (cur.n && hipMemcpyAsync(d_in.p, cur.in, cur.n, hipMemcpyHostToDevice, c->stream) != hipSuccess) return LFX_E_DEVICE;
        return encode(nullptr, (EncodeResult *)h_res.data(), err);
    }
    int collect(EncDone &done, std::string &err) {
        std::lock_guard<std::recursive_mutex> lock(c->mu);
        (void)hipSetDevice(c->device);
        if (hipStreamSynchronize(c->stream) != hipSuccess) return LFX_E_DEVICE;
        EncodeResult res{};
        // the first pass is the batch in flight, its result in the slot; (never observed) a violation: the batch's bytes are still
        // in d_in — once more, on the fallback kernel, synchronously
        bool in_flight = true;
        int rc = with_match_fallback(c, res, [&]() -> int {
            if (in_flight) { in_flight = false; res = *(const EncodeResult *)h_res.data(); return LFX_OK; }
            return encode(&res, nullptr, err);
        });
        if (rc) return rc;
        done.status = res.status;
        done.end_bit = res.end_bit;
        done.crc32 = res.crc32;
        done.adler32 = res.adler32;
        if (res.status != 0) { c->set_error("output capacity too small"); return LFX_OK; }
        const uint64_t whole = whole_bytes(res.end_bit, cur.final);
        h_out.resize(whole + 1);
        // the shared byte first (the next batch's launch needs it), then the bulk — which travels while that launch is prepared
        uint8_t *slot = h_res.data() + 128;
        if (hipMemcpyAsync(slot, (const uint8_t *)d_out.p + whole, 1, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipEventRecord(ev_small, c->stream) != hipSuccess ||
            (whole && hipMemcpyAsync(h_out.data(), d_out.p, whole, hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
            hipEventRecord(ev_out, c->stream) != hipSuccess || hipEventSynchronize(ev_small) != hipSuccess) return LFX_E_DEVICE;
        done.shared = *slot;
        return LFX_OK;
    }
    int bytes(uint64_t, const uint8_t **p) {
        std::lock_guard<std::recursive_mutex> lock(c->mu);
        (void)hipSetDevice(c->device);
        if (hipEventSynchronize(ev_out) != hipSuccess) return LFX_E_DEVICE;
        *p = h_out.data();
        return LFX_OK;
    }
    // (an encoder freed without finish, or after a failed launch: the DMA engine may still read the buffers) — the device
    // buffers go back to the context's pool
    void settle() {
        (void)hipSetDevice(c->device);
        c->give_dev(d_in);
        c->give_dev(d_out);
        (void)hipStreamSynchronize(c->stream);
        if (ev_out) (void)hipEventDestroy(ev_out);
        if (ev_small) (void)hipEventDestroy(ev_small);
        ev_out = ev_small = nullptr;
    }
    PinVec take_out() { return std::move(h_out); }
};

}  // namespace

struct lfx_encoder : StreamEnc<PinVec, GpuBatches> {
    using StreamEnc::StreamEnc;
};

extern "C" void lfx_encoder_free(lfx_encoder *e);
// lfx_encoder_new and lfx_encoder_new_dict behind their argument checks.  dict == nullptr: the dictionary-less encoder, which
// asks the table with DICT_NONE, writes container_header's bytes and never marks a chunk.
static lfx_encoder *encoder_new(lfx_ctx *cc, int format, const lfx_encode_opts *o, const lfx_dict *dict, lfx_write_cb w,
                                lfx_flush_cb f, void *user, int *status) {
    if (!cc || !w) { if (status) *status = cc ? LFX_E_ARG : LFX_E_DEVICE; return nullptr; }
    EncodeSpec sp;
    const char *why;
    int rc = encode_spec(format, o, &sp);
    if (!rc) rc = encode_served(ENC_STREAM, sp, !dict ? DICT_NONE : dict->chain ? DICT_CHAIN : DICT_PLAIN, &why);
    if (rc) {
        if (rc == LFX_E_UNSUPPORTED) {           // (no handle to ask: the reason goes to the context, as for the one-shot calls)
            Ctx *rc_ctx = reinterpret_cast<Ctx *>(cc);
            std::lock_guard<std::recursive_mutex> lock(rc_ctx->mu);
            rc_ctx->set_error(why);
        }
        if (status) *status = rc;
        return nullptr;
    }
    lfx_encoder *e = new lfx_encoder(format, sp);
    Ctx *c = e->backend.c = reinterpret_cast<Ctx *>(cc);
    e->backend.format = format;
    e->backend.spec = &e->spec;
    if (dict) {
        e->backend.dict = dict;
        e->set_dict(dict, dict->id, dict->usable != 0);
    }
    if (c->diag.enc_batch_mb > 0) e->pol.batch_bytes = (uint64_t)c->diag.enc_batch_mb << 20;
    // (page-locked and device buffers of an earlier encoder of this context, when there are any)
    e->pending = c->take_pin();
    e->backend.h_out = c->take_pin();
    e->inflight_buf = c->take_pin();
    e->backend.d_in = c->take_dev();
    e->backend.d_out = c->take_dev();
    e->w = w;
    e->f = f;
    e->user = user;
    rc = enc_open(e);
    if (rc) { if (status) *status = rc; lfx_encoder_free(e); return nullptr; }
    if (status) *status = LFX_OK;
    return e;
}
extern "C" lfx_encoder *lfx_encoder_new(lfx_ctx *cc, int format, const lfx_encode_opts *o, lfx_write_cb w,
                                        lfx_flush_cb f, void *user, int *status) try {
    return encoder_new(cc, format, o, nullptr, w, f, user, status);
} LFX_ABI_CATCH_NEW
//  the dictionary comes with the constructor: the zlib header — FDICT, DICTID — is written in it
extern "C" lfx_encoder *lfx_encoder_new_dict(lfx_ctx *cc, int format, const lfx_encode_opts *o, const lfx_dict *dict,
                                             lfx_write_cb w, lfx_flush_cb f, void *user, int *status) try {
    if (format == LFX_GZIP) { if (status) *status = LFX_E_ARG; return nullptr; }      // (gzip has no preset dictionary)
    if (!cc) { if (status) *status = LFX_E_DEVICE; return nullptr; }
    if (dict && (dict->c != reinterpret_cast<Ctx *>(cc) || (format != LFX_ZLIB && format != LFX_DEFLATE))) {
        if (status) *status = LFX_E_ARG;
        return nullptr;
    }
    return encoder_new(cc, format, o, dict, w, f, user, status);
} LFX_ABI_CATCH_NEW

extern "C" int64_t lfx_encoder_write(lfx_encoder *e, const uint8_t *p, size_t n) try {
    if (!e) return -(int64_t)LFX_E_ARG;
    return enc_write(e, p, n);
} LFX_ABI_CATCH_NEG
extern "C" int lfx_encoder_write_codes(lfx_encoder *e, const uint32_t *codes, size_t n_codes, const uint8_t *raw, size_t n_raw,
                                       int end_block) try {
    if (!e) return LFX_E_ARG;
    return enc_write_codes(e, codes, n_codes, raw, n_raw, end_block);
} LFX_ABI_CATCH
extern "C" int lfx_encoder_flush(lfx_encoder *e) try {
    if (!e) return LFX_E_ARG;
    return enc_flush(e);
} LFX_ABI_CATCH
extern "C" int lfx_encoder_finish(lfx_encoder *e) try {
    if (!e) return LFX_E_ARG;
    return enc_finish(e);
} LFX_ABI_CATCH
extern "C" const char *lfx_encoder_last_error(const lfx_encoder *e) { return e ? e->err.c_str() : "null"; }
extern "C" void lfx_encoder_free(lfx_encoder *e) {
    if (!e) return;
    Ctx *c = e->backend.c;
    enc_close(e, [c](PinVec &&v) { c->give_pin(std::move(v)); });
}
