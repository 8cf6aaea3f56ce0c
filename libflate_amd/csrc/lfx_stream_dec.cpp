// lfx_stream_dec.cpp — the stream decoder on the GPU (C ABI: lfx_decoder_*): the state machine of lfx_stream_dec.h over
// page-locked buffers, with the member decode (inflate_member, partial) as its window backend.
#include "../../include/lfx.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <mutex>

#include "lfx_decode_int.h"
#include "lfx_device.h"
#include "lfx_hostio.h"
#include "lfx_stream_dec.h"
#include "lfx_dict.h"
#include "lfx_abi_guard.h"

using namespace lfx;

namespace {

// one window on the GPU (the context's scratch is shared: one decode at a time per context): wi.in[0, n) from bit bit_off with
// the history → W.out, W.mr, the window's checksums.  → a device-level failure of the attempt
int gpu_window(Ctx *c, const WindowIn &wi, DecWindow<PinVec> &W) {
    const uint64_t n = wi.n, H = wi.hist_len;
    MemberResult mr;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    (void)hipSetDevice(c->device);
    c->n_ev = 0;
    c->phase("start");
    int rc;
    if ((rc = c->d_io_in.reserve(std::max<uint64_t>(n, 4)))) return rc;
    if ((rc = c->d_io_out.reserve(MAX_WINDOW + wi.out_cap))) return rc;
    if ((rc = c->d_res.reserve(256))) return rc;
    uint8_t *d_out = (uint8_t *)c->d_io_out.p + MAX_WINDOW;          // the history lies right in front of it
    if (n && hipMemcpyAsync(c->d_io_in.p, wi.in, n, hipMemcpyHostToDevice, c->stream) != hipSuccess) return LFX_E_DEVICE;
    if (H && hipMemcpyAsync(d_out - H, wi.hist, H, hipMemcpyHostToDevice, c->stream) != hipSuccess) return LFX_E_DEVICE;
    const auto tw0 = std::chrono::steady_clock::now();
    // (a preset dictionary's tail came with wi.hist and lies in front of d_out like earlier output; it counts for the reach bound)
    rc = inflate_member(c, (const uint8_t *)c->d_io_in.p, n, 0, d_out, wi.out_cap, mr, wi.bit_off, ~0ull, wi.partial(),
                        wi.dict_len + wi.member_out);
    if (rc) return rc;
    const auto tw1 = std::chrono::steady_clock::now();
    W.mr.status = mr.status; W.mr.out_len = mr.out_len; W.mr.blk_out_start = mr.blk_out_start; W.mr.end_byte = mr.end_byte;
    W.mr.end_bit = mr.end_bit; W.mr.final_seen = mr.final_seen; W.mr.need_cap = mr.need_cap; W.mr.msg = mr.msg;
    if (mr.status == LFX_E_NOSPACE && !wi.partial()) return LFX_OK;   // (the policy calls again with more room: nothing to fetch)
    const uint64_t keep = mr.out_len;                 // bytes produced (also on failure)
    const bool ck = keep && mr.status == LFX_OK && trailer_len(wi.format);
    if (ck) {
        const uint64_t nspans = ck_nspans(keep);
        if ((rc = c->d_ck.reserve(12 * nspans))) return rc;
        uint32_t *p = (uint32_t *)c->d_ck.p;
        if (int e_ = launch_checksum(c->stream, d_out, keep, p, p + nspans, p + 2 * nspans, (EncodeResult *)c->d_res.p, ck_mode_of(wi.format))) {
            c->set_error(hipGetErrorString((hipError_t)e_));
            return LFX_E_DEVICE;
        }
        if (hipMemcpyAsync(c->h_res, c->d_res.p, sizeof(EncodeResult), hipMemcpyDeviceToHost, c->stream) != hipSuccess) return LFX_E_DEVICE;
    }
    W.out.resize(keep);
    if (keep && hipMemcpyAsync(W.out.data(), d_out, keep, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return LFX_E_DEVICE;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return LFX_E_DEVICE;
    if (ck) {
        const EncodeResult er = *(EncodeResult *)c->h_res;
        W.crc = er.crc32;
        W.adler = er.adler32;
    }
    if (c->diag.debug) {
        fprintf(stderr, "[lfx] window gpu: in=%llu out=%llu inflate_member %.3f ms, checksum + D2H %.3f ms", (unsigned long long)n,
                (unsigned long long)keep, std::chrono::duration<double, std::milli>(tw1 - tw0).count(),
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tw1).count());
        if (c->timing_on)          // (the kernels' own brackets of this window; the first one holds the H2D copy too)
            for (int i = 0; i + 1 < c->n_ev; i++) {
                float ms = 0;
                (void)hipEventSynchronize(c->ev[i + 1]);
                if (hipEventElapsedTime(&ms, c->ev[i], c->ev[i + 1]) == hipSuccess) fprintf(stderr, " %s=%.3f", c->ev_name[i + 1], ms);
            }
        fprintf(stderr, "\n");
    }
    return LFX_OK;
}

struct GpuWindows {
    Ctx *c = nullptr;
    void operator()(const WindowIn &wi, DecWindow<PinVec> &W) const { W.rc = gpu_window(c, wi, W); }
};

}  // namespace

struct lfx_decoder : StreamDec<PinVec, GpuWindows> {
    Ctx *ctx() const { return backend.c; }
};

extern "C" void lfx_decoder_free(lfx_decoder *d);
extern "C" lfx_decoder *lfx_decoder_new(lfx_ctx *cc, int format, uint32_t flags, lfx_read_cb r, void *user, int *status) try {
    if (!cc || !r || format < 0 || format > 2) { if (status) *status = cc ? LFX_E_ARG : LFX_E_DEVICE; return nullptr; }
    lfx_decoder *d = new lfx_decoder();
    Ctx *c = d->backend.c = reinterpret_cast<Ctx *>(cc);
    d->debug = c->diag.debug;
    d->out = c->take_pin();         // (page-locked buffers of an earlier decoder of this context, when there are any)
    d->next.out = c->take_pin();
    d->in = c->take_pin();
    d->format = format;
    d->flags = flags;
    d->r = r;
    d->user = user;
    const int rc = dec_open(d);
    if (rc) {
        if (status) *status = rc;
        c->set_error(d->err);
        lfx_decoder_free(d);
        return nullptr;
    }
    if (status) *status = LFX_OK;
    return d;
} LFX_ABI_CATCH_NEW

extern "C" int64_t lfx_decoder_read(lfx_decoder *d, uint8_t *out, size_t cap) try {
    if (!d) return -(int64_t)LFX_E_ARG;
    const int64_t k = dec_read(d, out, cap);
    // (a window that failed on the device, not in the stream: the text is on the context)
    if (k < 0 && d->next.rc && k == -(int64_t)d->next.rc && d->err.empty()) d->err = d->ctx()->err;
    return k;
} LFX_ABI_CATCH_NEG
extern "C" int lfx_decoder_set_dict(lfx_decoder *d, const lfx_dict *dict) try {
    if (!d || !dict || dict->c != d->ctx()) return LFX_E_ARG;
    return dec_set_dict(d, dict->tail.data(), dict->usable, dict->id);
} LFX_ABI_CATCH
extern "C" int lfx_decoder_unread(lfx_decoder *d, const uint8_t **p, size_t *n) try {
    if (!d) return LFX_E_ARG;
    dec_unread(d, p, n);
    return LFX_OK;
} LFX_ABI_CATCH
extern "C" int lfx_decoder_surplus(lfx_decoder *d, const uint8_t **p, size_t *n) try {
    if (!d) return LFX_E_ARG;
    dec_surplus(d, p, n);
    return LFX_OK;
} LFX_ABI_CATCH
extern "C" int lfx_decoder_header(lfx_decoder *d, lfx_header *h) try {
    if (!d || !h) return LFX_E_ARG;
    return dec_header_get(d, h);
} LFX_ABI_CATCH
extern "C" uint64_t lfx_decoder_consumed(const lfx_decoder *d) { return d ? d->consumed_total : 0; }
extern "C" uint64_t lfx_decoder_buffered(const lfx_decoder *d) { return d ? dec_buffered(const_cast<lfx_decoder *>(d)) : 0; }
extern "C" const char *lfx_decoder_last_error(const lfx_decoder *d) { return d ? d->err.c_str() : "null"; }
extern "C" void lfx_decoder_free(lfx_decoder *d) {
    if (!d) return;
    Ctx *c = d->ctx();
    dec_close(d, [c](PinVec &&v) { c->give_pin(std::move(v)); });
}
