// lfx_decode.cpp — host orchestration of the inflate path (C ABI: lfx_decode_*; the stream decoder: lfx_stream_dec.cpp).
// Every compressed bit is decoded on the GPU; the host only sequences kernels, chains block
// boundaries and formats error messages.
#include "../../include/lfx.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "lfx_decode_int.h"
#include "lfx_container.h"
#include "lfx_index.h"
#include "lfx_bgzf.h"
#include "lfx_dict.h"
#include "lfx_batch_unpack.h"

static_assert(offsetof(lfx::DecStream, out_off) == 16 && sizeof(lfx::DecStream) % 8 == 0, "checksum_ranges stride");
static_assert(offsetof(lfx::InflateResult, out_len) == 8 && sizeof(lfx::InflateResult) % 8 == 0, "checksum_ranges stride");
#include "lfx_device.h"
#include "lfx_abi_guard.h"

using namespace lfx;

namespace {

int size_member(Ctx *c, const uint8_t *d_in, uint64_t n, uint64_t off0, MemberResult &mr);
int batch_size_walk(Ctx *c, int format, uint32_t count, const uint8_t *d_in, const uint64_t *in_off, const uint64_t *in_len,
                    const std::vector<DecHeader> &hdrs, std::vector<InflateResult> &res, std::vector<uint64_t> &used_out,
                    const lfx_dict *dict = nullptr);

// the container checksum of the member's output d_out[0, mr.out_len) against the trailer at d_in[tpos, tpos + need)
int verify_trailer(Ctx *c, int format, const uint8_t *d_in, uint64_t tpos, uint64_t need, const uint8_t *d_out, const MemberResult &mr,
                   DecodeOutcome &oc) {
    hipStream_t st = c->stream;
    uint8_t t[8];
    EncodeResult er{};
    if (mr.ck_done) {                   // (came back with the materialisation's verdict)
        er.crc32 = mr.crc32; er.adler32 = mr.adler32;
        memcpy(t, mr.trailer, need);
    } else {
        const uint64_t nspans = ck_nspans(mr.out_len);
        int rc;
        if ((rc = c->d_ck.reserve(12 * nspans))) return rc;
        uint32_t *ck = (uint32_t *)c->d_ck.p;
        LAUNCH_TRY(launch_checksum(st, d_out, mr.out_len, ck, ck + nspans, ck + 2 * nspans, (EncodeResult *)c->d_res.p,
                                   format == LFX_GZIP ? 1 : format == LFX_ZLIB ? 2 : 3));
        HIP_TRY(hipMemcpyAsync(c->h_res, c->d_res.p, sizeof(EncodeResult), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(t, d_in + tpos, need, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        c->phase("checksum");
        er = *(EncodeResult *)c->h_res;
    }
    if (const int bad = check_trailer(format, t, er.crc32, er.adler32, oc.msg)) oc.status = bad;
    return LFX_OK;
}

// The member loop from input byte `base` on, its output from d_out[out_at] on (the members in front of `base` were decoded
// into d_out[0, out_at) and verified by the caller; base == 0 is the first member).  one_member: return behind the first
// member whose trailer was verified (oc.more), without looking at what follows.  members: the verified members are appended.
// sizes_only: the loop of the size calls — no output and no checksum comparison (a trailer must be THERE); d_out is not used.
// dict (the dictionary calls, zlib / raw DEFLATE, not with sizes_only): a zlib header's FDICT is judged against it, and a
// member that uses it is decoded with its tail as detached history.
int member_loop(Ctx *c, int format, uint32_t flags, const uint8_t *d_in, uint64_t n, uint8_t *d_out, uint64_t cap, bool sizes_only,
                DecodeOutcome &oc, uint64_t base, uint64_t out_at, bool one_member, std::vector<lfx_member> *members,
                const lfx_dict *dict = nullptr) {
    (void)hipSetDevice(c->device);
    hipStream_t st = c->stream;
    bool first = base == 0;
    oc.consumed = base;
    oc.out_len = oc.delivered_len = out_at;
    int rc;
    if (!sizes_only && (rc = c->d_res.reserve(256))) return rc;
    if ((rc = c->d_small.reserve(70000))) return rc;
    for (;;) {
        // ---- container header (device parse, one lane)
        uint64_t off0 = 0;
        uint64_t dict_hist = dict && format == LFX_DEFLATE ? dict->usable : 0;    // (raw DEFLATE: always the history in front of byte 0)
        if (format != LFX_DEFLATE) {
            DecStream ds{base, n - base, 0, 0};
            DecHeader dh{};
            c->pin_reset();       // (page-locked slots for the two small transfers, lfx_ctx.h)
            HIP_TRY(c->small_up(c->d_small.p, &ds, sizeof ds, st));
            if (dict)
                LAUNCH_TRY(launch_container_dict(st, 1, d_in, (const DecStream *)c->d_small.p,
                                                 (DecHeader *)((uint8_t *)c->d_small.p + 256), dict->id));
            else
            LAUNCH_TRY(launch_container(st, format, 1, d_in, (const DecStream *)c->d_small.p,
                                        (DecHeader *)((uint8_t *)c->d_small.p + 256)));
            HIP_TRY(c->small_down(&dh, (uint8_t *)c->d_small.p + 256, sizeof dh, st));
            HIP_TRY(c->small_sync(st));
            if (dh.status != 0) {
                if (!first && dh.status == 2) {  // MultiDecoder: UnexpectedEof on the next header = clean end
                    oc.consumed = n;             // (gzip.rs:1150-1156; the partial header bytes were read)
                    break;
                }
                oc.status = map_status(dh.status);
                oc.header_failed = first;
                oc.msg = format_error(dh.err, dh.a0, dh.a1);
                oc.consumed = base + dh.deflate_off;
                oc.out_len = oc.delivered_len = out_at;
                return LFX_OK;
            }
            off0 = dh.deflate_off;
            if (dict && (dh.flags & HDR_DICT)) dict_hist = dict->usable;          // (zlib without FDICT: the dictionary is not used)
        }
        if (c->idx && !sizes_only) {   // (an index build: the member's first block is an access point)
            c->idx->bit_base = base * 8;
            c->idx->out_base = out_at;
            c->idx->cand.push_back(IdxCand{(base + off0) * 8, (base + off0) * 8, out_at, IDX_BTYPE_READ});
        }
        MemberResult mr;
        if (sizes_only) rc = size_member(c, d_in + base, n - base, off0, mr);
        else {
            mr.ck_mode = ck_mode_of(format);
            mr.trailer_len = trailer_len(format);
            rc = inflate_member(c, d_in + base, n - base, off0, d_out + out_at, cap - out_at, mr, ~0ull, ~0ull, false, dict_hist,
                                dict_hist ? dict->d_win : nullptr);
        }
        if (rc) return rc;
        oc.out_len = out_at + mr.out_len;
        oc.delivered_len = out_at + mr.blk_out_start;
        oc.consumed = base + mr.end_byte;
        if (mr.status != LFX_OK) { oc.status = mr.status; oc.msg = mr.msg; return LFX_OK; }
        // ---- trailer
        if (format != LFX_DEFLATE) {
            const uint64_t need = trailer_len(format);
            const uint64_t tpos = base + mr.end_byte;
            if (n - tpos < need) {
                oc.status = LFX_E_UNEXPECTED_EOF;
                oc.msg = "failed to fill whole buffer";
                oc.consumed = n;
                return LFX_OK;
            }
            oc.consumed = tpos + need;
            if (!sizes_only) {
                if ((rc = verify_trailer(c, format, d_in, tpos, need, d_out + out_at, mr, oc))) return rc;
                if (oc.status != LFX_OK) return LFX_OK;
            }
        }
        if (members) members->push_back(lfx_member{base, oc.consumed - base, out_at, mr.out_len});
        out_at = oc.out_len;
        if (one_member) { oc.more = true; break; }
        if (!(format == LFX_GZIP && (flags & LFX_DEC_MULTI))) break;
        base = oc.consumed;
        first = false;
    }
    oc.out_len = oc.delivered_len = out_at;
    return LFX_OK;
}

int decode_stream(Ctx *c, int format, uint32_t flags, const uint8_t *d_in, uint64_t n, uint8_t *d_out,
                  uint64_t cap, DecodeOutcome &oc, uint64_t base = 0, uint64_t out_at = 0, bool one_member = false,
                  std::vector<lfx_member> *members = nullptr, const lfx_dict *dict = nullptr) {
    return member_loop(c, format, flags, d_in, n, d_out, cap, false, oc, base, out_at, one_member, members, dict);
}

// The container headers of a list of streams in one launch: hdrs[i] = stream i's parse.  The streams and the headers stay in
// d_dec_blocks (*d_streams, *d_hdrs, with extra_bytes of room behind the headers) for the kernels of a caller that go on from
// them.  LFX_DEFLATE has no header: all-zero ones, on the device too, without a round trip.
int parse_headers(Ctx *c, int format, const uint8_t *d_in, const std::vector<DecStream> &streams, std::vector<DecHeader> &hdrs,
                  size_t extra_bytes = 0, DecStream **d_streams = nullptr, DecHeader **d_hdrs = nullptr, const lfx_dict *dict = nullptr) {
    hipStream_t st = c->stream;
    const uint32_t count = (uint32_t)streams.size();
    const size_t sz_streams = sizeof(DecStream) * count, sz_hdr = sizeof(DecHeader) * count;
    int rc;
    if ((rc = c->d_dec_blocks.reserve(sz_streams + sz_hdr + extra_bytes))) return rc;
    DecStream *ds = (DecStream *)c->d_dec_blocks.p;
    DecHeader *dh = (DecHeader *)((uint8_t *)c->d_dec_blocks.p + sz_streams);
    HIP_TRY(hipMemcpyAsync(ds, streams.data(), sz_streams, hipMemcpyHostToDevice, st));
    if (dict && format == LFX_ZLIB) LAUNCH_TRY(launch_container_dict(st, count, d_in, ds, dh, dict->id));
    else LAUNCH_TRY(launch_container(st, format, count, d_in, ds, dh));
    hdrs.assign(count, DecHeader{});
    if (format != LFX_DEFLATE) {
        HIP_TRY(hipMemcpyAsync(hdrs.data(), dh, sz_hdr, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    } else {
        HIP_TRY(hipMemsetAsync(dh, 0, sz_hdr, st));
    }
    if (d_streams) *d_streams = ds;
    if (d_hdrs) *d_hdrs = dh;
    return LFX_OK;
}

}  // namespace

extern "C" int lfx_decode_device(lfx_ctx *cc, int format, uint32_t flags, const void *d_in, uint64_t n,
                                 void *d_out, uint64_t cap, uint64_t *out_len, uint64_t *consumed) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    if (format < 0 || format > 2) return LFX_E_ARG;
    (void)hipSetDevice(c->device);
    c->n_ev = 0;
    c->phase("start");
    DecodeOutcome oc;
    int rc = decode_stream(c, format, flags, (const uint8_t *)d_in, n, (uint8_t *)d_out, cap, oc);
    if (rc) return rc;
    if (oc.status == LFX_OK) c->phase("done");
    if (oc.out_len > cap) oc.out_len = cap;  // defensive: never report more than the buffer holds
    if (out_len) *out_len = oc.out_len;
    if (consumed) *consumed = oc.consumed;
    if (oc.status != LFX_OK) c->set_error(oc.msg);
    return oc.status;
} LFX_ABI_CATCH

// ---- the dictionary calls: the same loop with the dictionary; without one, the dictionary-less twin itself
extern "C" int lfx_decode_dict_device(lfx_ctx *cc, int format, const lfx_dict *dict, const void *d_in, uint64_t n, void *d_out,
                                      uint64_t cap, uint64_t *out_len, uint64_t *consumed) try {
    if (!cc) return LFX_E_DEVICE;
    if (format != LFX_ZLIB && format != LFX_DEFLATE) return LFX_E_ARG;      // (gzip has no preset dictionary)
    if (!dict) return lfx_decode_device(cc, format, 0, d_in, n, d_out, cap, out_len, consumed);
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    if (dict->c != c) return LFX_E_ARG;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    (void)hipSetDevice(c->device);
    c->n_ev = 0;
    c->phase("start");
    DecodeOutcome oc;
    int rc = decode_stream(c, format, 0, (const uint8_t *)d_in, n, (uint8_t *)d_out, cap, oc, 0, 0, false, nullptr, dict);
    if (rc) return rc;
    if (oc.status == LFX_OK) c->phase("done");
    if (oc.out_len > cap) oc.out_len = cap;
    if (out_len) *out_len = oc.out_len;
    if (consumed) *consumed = oc.consumed;
    if (oc.status != LFX_OK) c->set_error(oc.msg);
    return oc.status;
} LFX_ABI_CATCH

extern "C" int lfx_decode_dict_host(lfx_ctx *cc, int format, const lfx_dict *dict, const void *in, uint64_t n, void *out,
                                    uint64_t cap, uint64_t *out_len, uint64_t *consumed) try {
    if (!cc) return LFX_E_DEVICE;
    if (format != LFX_ZLIB && format != LFX_DEFLATE) return LFX_E_ARG;
    if (!dict) return lfx_decode_host(cc, format, 0, in, n, out, cap, out_len, consumed);
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    if (dict->c != c) return LFX_E_ARG;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    (void)hipSetDevice(c->device);
    int rc;       // (staged as lfx_decode_host stages)
    if ((rc = c->d_io_in.reserve(std::max<uint64_t>(n, 4)))) return rc;
    if ((rc = c->d_io_out.reserve(std::max<uint64_t>(cap, 4)))) return rc;
    if (int hr = host_to_device(c, c->d_io_in.p, in, n, c->stream)) { c->set_error("host to device copy failed"); return hr; }
    uint64_t ol = 0;
    rc = lfx_decode_dict_device(cc, format, dict, c->d_io_in.p, n, c->d_io_out.p, cap, &ol, consumed);
    if (rc == LFX_E_DEVICE || rc == LFX_E_OOM || rc == LFX_E_ARG) { (void)hipStreamSynchronize(c->stream); return rc; }
    if (ol) { if (int hr = device_to_host(c, out, c->d_io_out.p, ol, c->stream)) { c->set_error("device to host copy failed"); return hr; } }
    if (out_len) *out_len = ol;
    return rc;
} LFX_ABI_CATCH

// A dictionary belongs to its context.  The id is computed on the device (the checksum kernels of the trailer check) over ALL
// bytes; the last min(len, 32768) of them are kept: at the end of a 32 KiB device window, and on the host (stream decoders).
extern "C" void lfx_dict_free(lfx_dict *d);
static lfx_dict *dict_new(lfx_ctx *cc, const void *bytes, uint64_t len, int on_device, int *status, bool chain) {
    if (status) *status = LFX_OK;
    if (!cc) { if (status) *status = LFX_E_DEVICE; return nullptr; }
    if (!bytes && len) { if (status) *status = LFX_E_ARG; return nullptr; }
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    (void)hipSetDevice(c->device);
    hipStream_t st = c->stream;
    lfx_dict *d = new lfx_dict();
    d->c = c;
    d->chain = chain;
    auto fail = [&](int rc) -> lfx_dict * { if (status) *status = rc; lfx_dict_free(d); return nullptr; };
    if (hipMalloc((void **)&d->d_win, MAX_WINDOW) != hipSuccess) { d->d_win = nullptr; return fail(LFX_E_OOM); }
    if (hipMemsetAsync(d->d_win, 0, MAX_WINDOW, st) != hipSuccess) return fail(LFX_E_DEVICE);
    d->usable = (uint32_t)std::min<uint64_t>(len, MAX_WINDOW);
    if (len) {
        const uint8_t *d_bytes = (const uint8_t *)bytes;
        if (!on_device) {
            if (int rc = c->d_io_in.reserve(len)) return fail(rc);
            if (int hr = host_to_device(c, c->d_io_in.p, bytes, len, st)) { c->set_error("host to device copy failed"); return fail(hr); }
            d_bytes = (const uint8_t *)c->d_io_in.p;
        }
        const uint64_t nspans = ck_nspans(len);
        if (int rc = c->d_ck.reserve(12 * nspans)) return fail(rc);
        if (int rc = c->d_res.reserve(256)) return fail(rc);
        uint32_t *ck = (uint32_t *)c->d_ck.p;
        if (launch_checksum(st, d_bytes, len, ck, ck + nspans, ck + 2 * nspans, (EncodeResult *)c->d_res.p, 2)) return fail(LFX_E_DEVICE);
        d->tail.resize(d->usable);
        if (hipMemcpyAsync(c->h_res, c->d_res.p, sizeof(EncodeResult), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipMemcpyAsync(d->d_win + (MAX_WINDOW - d->usable), d_bytes + (len - d->usable), d->usable, hipMemcpyDeviceToDevice, st) != hipSuccess ||
            hipMemcpyAsync(d->tail.data(), d_bytes + (len - d->usable), d->usable, hipMemcpyDeviceToHost, st) != hipSuccess)
            return fail(LFX_E_DEVICE);
    }
    if (hipStreamSynchronize(st) != hipSuccess) return fail(LFX_E_DEVICE);
    if (len) d->id = ((const EncodeResult *)c->h_res)->adler32;
    return d;
}
extern "C" lfx_dict *lfx_dict_new(lfx_ctx *cc, const void *bytes, uint64_t len, int on_device, int *status) try {
    return dict_new(cc, bytes, len, on_device, status, false);
} LFX_ABI_CATCH_NEW
// a chain dictionary: the same object, marked; its chain is the first chained encode's to build
extern "C" lfx_dict *lfx_dict_new_chain(lfx_ctx *cc, const void *bytes, uint64_t len, int on_device, int *status) try {
    return dict_new(cc, bytes, len, on_device, status, true);
} LFX_ABI_CATCH_NEW
extern "C" uint32_t lfx_dict_id(const lfx_dict *d) { return d ? d->id : 1; }
extern "C" void lfx_dict_free(lfx_dict *d) {
    if (!d) return;
    if (d->d_win) {
        std::lock_guard<std::recursive_mutex> lock(d->c->mu);
        (void)hipSetDevice(d->c->device);
        (void)hipStreamSynchronize(d->c->stream);
        (void)hipFree(d->d_win);
        if (d->d_tab) (void)hipFree(d->d_tab);      // (the encode's prefix table)
        if (d->d_cdt) (void)hipFree(d->d_cdt);      // (a chain dictionary's chain)
    }
    delete d;
}

extern "C" int lfx_decode_shard_device(lfx_ctx *cc, const void *d_in, uint64_t n, uint64_t start_bit,
                                       uint64_t total_bits, int is_last, void *d_out, uint64_t cap,
                                       uint64_t *out_len) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    (void)hipSetDevice(c->device);
    c->n_ev = 0;
    c->phase("start");
    MemberResult mr;
    int rc = inflate_member(c, (const uint8_t *)d_in, n, start_bit >> 3, (uint8_t *)d_out, cap, mr, start_bit,
                            is_last ? ~0ull : start_bit + total_bits);
    if (rc) return rc;
    if (out_len) *out_len = mr.out_len;
    if (mr.status != LFX_OK) c->set_error(mr.msg);
    return mr.status;
} LFX_ABI_CATCH

// ------------------------------------------------------------------------------------------------
// N-GPU decode of ONE member without the encoder's help: the member is cut by compressed BYTES;
// every rank finds and scans the blocks that START in its byte range (lfx_decode_range_scan), the ranks exchange one
// tuple per candidate (one all-gather), every rank walks the same chain over the gathered table (lfx_decode_chain) and
// materialises the blocks it owns into its slice of the output (lfx_decode_range_emit).  The container checksum is
// folded from the ranks' slice checksums (lfx_crc32_combine / lfx_adler32_combine).
static_assert(sizeof(lfx_blk_tuple) == 56, "tuple layout (all-gathered as raw bytes)");

extern "C" int lfx_decode_range_scan(lfx_ctx *cc, const void *d_part_, uint64_t n_part, uint64_t lo_byte, uint64_t hi_byte,
                                     uint64_t first_bit, uint64_t final_from_bit, uint32_t rank, lfx_blk_tuple *tuples, uint32_t cap,
                                     uint32_t *count) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    (void)hipSetDevice(c->device);
    hipStream_t st = c->stream;
    const uint8_t *d_in = (const uint8_t *)d_part_;
    if (!count || hi_byte < lo_byte || n_part < hi_byte - lo_byte) return LFX_E_ARG;
    *count = 0;
    c->n_ev = 0;
    c->phase("start");
    const uint64_t n = n_part, range_bits = (hi_byte - lo_byte) * 8, base_bit = lo_byte * 8;
    // ---- block-start candidates in the local bytes (the tail behind hi_byte is searched too: a false candidate there
    //      still ends the range guess of the last real block early, exactly as on one GPU)
    int rc;
    c->pin_reset();        // (the page-locked slots of the small transfers: nothing of an earlier call is in flight)
    std::vector<uint64_t> starts;
    if (n >= 16) {
        // headers with BFINAL set are reported from member bit `final_from_bit` on (the finder's tail rule, inflate_member: a
        // member's last block is the only one that carries the flag — everywhere else the offsets whose bit 0 is set are
        // dropped, which halves the candidates of both stages and the scan jobs).  The chain is walked on tuples, so a last
        // block that starts in front of that bit breaks the chain: the caller then scans again with final_from_bit = 0.
        const uint64_t final_local = final_from_bit <= base_bit ? 0 : std::min<uint64_t>(final_from_bit - base_bit, ~0ull >> 1);
        FindBufs fb;
        Found fd;
        if ((rc = find_launch(c, d_in, n, 0, final_local, fb))) return rc;
        if ((rc = find_collect(c, d_in, n, fb, fd))) return rc;
        if (fd.overflow) { c->set_error("block finder overflow"); return LFX_E_UNSUPPORTED; }
        starts = std::move(fd.cand);
    }
    c->phase("find");
    if (first_bit != ~0ull) {            // the member's first block (its start is known: right behind the container header)
        if (first_bit < base_bit || first_bit - base_bit >= n * 8) return LFX_E_ARG;
        starts.push_back(first_bit - base_bit);
    }
    std::sort(starts.begin(), starts.end());
    starts.erase(std::unique(starts.begin(), starts.end()), starts.end());
    // jobs: the candidates that start inside the range; a job's range guess ends at the next candidate (inside or behind it)
    uint32_t nc = 0;
    while (nc < starts.size() && starts[nc] < range_bits) nc++;
    if (nc > cap) { c->set_error("more candidates than the caller's tuple buffer holds"); return LFX_E_NOSPACE; }
    const size_t tab_bytes = blk_tabs_bytes();
    c->range_stored.clear();
    if (nc) {
        auto start_at = [&](uint32_t i) { return i < starts.size() ? starts[i] : n * 8; };
        std::vector<BlkJob> bj(nc);
        for (uint32_t i = 0; i < nc; i++) bj[i] = BlkJob{starts[i], start_at(i + 1)};
        if ((rc = c->d_dec_streams.reserve(sizeof(BlkJob) * (nc + 1)))) return rc;
        if ((rc = c->d_dec_state.reserve(sizeof(BlkInfo) * (nc + 1)))) return rc;
        if ((rc = c->d_dec_blocks.reserve(sizeof(BlkLanes) * (size_t)(nc + 1)))) return rc;
        if ((rc = c->d_dec_tabs.reserve(tab_bytes * (nc + 1)))) return rc;
        // ONE Huffman pass for large blocks, as in inflate_member (round 6): the scan stores every lane's code words in a region of
        // its own, lfx_decode_range_emit moves the owned blocks' codes into place (blk_place_kernel) instead of decoding them again
        const bool store_mode = !c->diag.two_pass && (n * 8) / nc >= (1ull << 20) && plan_store(c, bj.data(), nc);
        HIP_TRY(hipMemcpyAsync(c->d_dec_streams.p, bj.data(), sizeof(BlkJob) * nc, hipMemcpyHostToDevice, st));
        if (store_mode)
            LAUNCH_TRY(launch_blk_scan_store(st, d_in, n, (const BlkJob *)c->d_dec_streams.p, nc, (BlkInfo *)c->d_dec_state.p,
                                             (BlkLanes *)c->d_dec_blocks.p, c->d_dec_tabs.p, (uint32_t *)c->d_dec_temp.p,
                                             (BlkLanesX *)c->d_dec_lanesx.p));
        else
            LAUNCH_TRY(launch_blk_scan(st, d_in, n, (const BlkJob *)c->d_dec_streams.p, nc, (BlkInfo *)c->d_dec_state.p,
                                       (BlkLanes *)c->d_dec_blocks.p, c->d_dec_tabs.p));
        std::vector<BlkInfo> bi(nc);
        HIP_TRY(hipMemcpyAsync(bi.data(), c->d_dec_state.p, sizeof(BlkInfo) * nc, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (BlkInfo &b : bi) if (b.status == BLK_OK && b.end_bit > n * 8) b.status = BLK_NO_EOB;
        c->range_stored.assign(nc, 0);
        c->range_temp_off.assign(nc, 0);
        c->range_cap.assign(nc, 0);
        if (store_mode)
            for (uint32_t j = 0; j < nc; j++) {
                // (a compressed block that scanned to its EndOfBlock and whose lanes' codes all fitted their regions; a job that is
                //  scanned again below loses the mark: the plain scan rewrites its lanes)
                c->range_stored[j] = bi[j].status == BLK_OK && bi[j].btype != 0 && bi[j]._pad == 0;
                c->range_temp_off[j] = bj[j].temp_off;
                c->range_cap[j] = bj[j].cap;
            }
        // a false candidate inside a block cuts that block's range guess short (no EndOfBlock): rescan with wider ranges (every
        // candidate's result lives in its own slot; a job that is scanned again loses its mark)
        std::vector<uint32_t> slot(nc);
        for (uint32_t i = 0; i < nc; i++) slot[i] = i;
        if ((rc = rescan_widen(c, d_in, n, starts, nc, bi, slot, c->range_stored, false))) return rc;
        for (uint32_t i = 0; i < nc; i++) {
            lfx_blk_tuple &t = tuples[i];
            t = lfx_blk_tuple{};
            t.start_bit = base_bit + starts[i];
            t.end_bit = base_bit + bi[i].end_bit;
            t.n_out = bi[i].n_out;
            t.n_codes = bi[i].n_codes;
            t.btype = (uint8_t)bi[i].btype;
            t.bfinal = (uint8_t)bi[i].bfinal;
            // (a block cut by the end of the local bytes is incomplete whatever its scan says — see inflate_member)
            t.status = (uint8_t)(bi[i].status == BLK_OK && bi[i].end_bit > n * 8 ? (uint32_t)BLK_NO_EOB : bi[i].status);
            t._pad = 0;
            t.slot = i;
            t.rank = (uint16_t)rank;
            t._pad2 = 0;
            t.nlanes = bi[i].nlanes;
            t.data_bit = base_bit + bi[i].data_bit;
        }
    }
    c->phase("blk_scan");
    *count = nc;
    return LFX_OK;
} LFX_ABI_CATCH

extern "C" int lfx_decode_chain(const lfx_blk_tuple *all, uint32_t n_all, uint64_t first_bit, uint32_t *chain, uint32_t cap,
                                uint32_t *n_chain, uint64_t *total_out) try {
    if (!all || !chain || !n_chain) return LFX_E_ARG;
    // the true block list: from the known first block, every block starts where the one before it ended; false candidates
    // (inside a block) are never reached.  Deterministic: every rank computes the same list from the same table.
    std::vector<uint32_t> order(n_all);
    for (uint32_t i = 0; i < n_all; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        return all[a].start_bit != all[b].start_bit ? all[a].start_bit < all[b].start_bit : all[a].rank < all[b].rank;
    });
    uint64_t pos = first_bit, total = 0;
    uint32_t k = 0;
    for (;;) {
        auto it = std::lower_bound(order.begin(), order.end(), pos, [&](uint32_t a, uint64_t v) { return all[a].start_bit < v; });
        if (it == order.end() || all[*it].start_bit != pos) return LFX_E_UNSUPPORTED;     // a block the finder cannot see (stored / fixed), or damage
        const lfx_blk_tuple &t = all[*it];
        if (t.status != BLK_OK || t.end_bit <= pos) return LFX_E_UNSUPPORTED;
        if (k >= cap) return LFX_E_NOSPACE;
        chain[k++] = *it;
        total += t.n_out;
        if (t.bfinal) break;
        pos = t.end_bit;
    }
    *n_chain = k;
    if (total_out) *total_out = total;
    return LFX_OK;
} LFX_ABI_CATCH

extern "C" int lfx_decode_range_emit(lfx_ctx *cc, const void *d_part_, uint64_t n_part, uint64_t lo_byte, const lfx_blk_tuple *all,
                                     const uint32_t *chain, uint32_t n_chain, uint32_t rank, void *d_out_, uint64_t cap,
                                     uint64_t *out_len, uint64_t *out_base, uint32_t *state) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    (void)hipSetDevice(c->device);
    hipStream_t st = c->stream;
    const uint8_t *d_in = (const uint8_t *)d_part_;
    uint8_t *d_out = (uint8_t *)d_out_;
    const uint64_t base_bit = lo_byte * 8;
    c->range = RangeState{};
    // the chain blocks this rank owns (consecutive in stream order: ownership goes by start position)
    std::vector<BlkEmit> emit;
    uint64_t before = 0, total = 0, total_codes = 0;
    uint32_t n_placed = 0;
    bool seen = false;
    for (uint32_t q = 0; q < n_chain; q++) {
        const lfx_blk_tuple &t = all[chain[q]];
        if (t.rank != rank) { if (!seen) before += t.n_out; continue; }
        seen = true;
        BlkInfo r{};                         // (what this rank's scan of the block found, back from the gathered tuple)
        r.data_bit = t.data_bit - base_bit; r.n_out = t.n_out; r.n_codes = t.n_codes; r.nlanes = t.nlanes; r.btype = t.btype;
        // (hist: the bytes of the member in front of the block bound its back-references)
        BlkEmit e = blk_emit_of(r, t.start_bit - base_bit, t.slot, total, total_codes, before + total);
        if (t.slot < c->range_stored.size() && c->range_stored[t.slot]) {      // (this rank's scan kept the block's code words)
            e.placed = 1; e.temp_off = c->range_temp_off[t.slot]; e.cap = c->range_cap[t.slot]; n_placed++;
        }
        emit.push_back(e);
        total += t.n_out;
        total_codes += t.n_codes;
    }
    if (out_base) *out_base = before;
    if (out_len) *out_len = total;
    if (state) *state = 0;
    if (total > cap) { c->set_error("output capacity too small"); return LFX_E_NOSPACE; }
    c->range.state = 0; c->range.total = total; c->range.d_out = d_out; c->range.before = before;
    if (emit.empty()) return LFX_OK;
    const uint32_t ne = (uint32_t)emit.size();
    int rc;
    c->pin_reset();
    EmitBufs eb;     // (marker units as on one GPU: two resident per CU, as large as that allows)
    if ((rc = emit_codes(c, d_in, n_part, emit, total_codes, n_placed, marker_unit_shift(total, c->n_cu), false, eb))) return rc;
    uint32_t *d_flags = eb.d_flags;
    const BlkEmit *d_emit = eb.d_emit;
    // small blocks smell of another encoder: look at the flags before materialising (as inflate_member does); the reference's
    // 1 MiB blocks are materialised at once and the flags read afterwards
    const bool probe = total / ne < (256u << 10);
    uint32_t fl = 0;
    if (probe) {
        HIP_TRY(hipMemcpyAsync(&fl, d_flags, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (!(probe && fl)) {
        LAUNCH_TRY(launch_blk_materialize(st, d_in, d_emit, ne, (const BlkLanes *)c->d_dec_blocks.p, (const BlkUnits *)c->d_hist.p,
                                          (const uint32_t *)c->d_codes.p, d_out, nullptr));
        HIP_TRY(hipMemcpyAsync(&fl, d_flags, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    c->phase("lz77_copy");
    if (fl & 1) {
        c->range.state = -1;
        c->set_error("a back-reference reaches in front of the member's first byte: decode it with lfx_decode_device for the exact error");
        return LFX_E_INVALID_DATA;
    }
    if (fl == 2) {
        // blocks that read the output of earlier blocks (another encoder's member), possibly of blocks another rank owns: the
        // slice is materialised as 16-bit symbols (a byte, or "byte j of the 32 KiB in front of my unit"); the window in front
        // of the slice arrives with lfx_decode_range_finish
        std::vector<BlkUnits> uv(ne);
        HIP_TRY(hipMemcpyAsync(uv.data(), c->d_hist.p, sizeof(BlkUnits) * ne, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        std::vector<SymUnit> su;
        const uint64_t max_len = sym_units(emit, uv, su);
        const uint32_t nsu = (uint32_t)su.size();
        if ((rc = c->d_dec_sym.reserve(2 * std::max<uint64_t>(total, 1)))) return rc;
        if ((rc = c->d_dec_win.reserve(32768ull * (std::max<uint32_t>(nsu, 1) + 1) + sizeof(SymUnit) * (size_t)nsu + 64))) return rc;
        if ((rc = c->d_dec_maps.reserve(window_prefix_scratch_bytes(std::max<uint32_t>(nsu, 1))))) return rc;
        SymUnit *d_su = (SymUnit *)((uint8_t *)c->d_dec_win.p + 32768ull * (std::max<uint32_t>(nsu, 1) + 1));
        HIP_TRY(hipMemcpyAsync(d_su, su.data(), sizeof(SymUnit) * nsu, hipMemcpyHostToDevice, st));
        LAUNCH_TRY(launch_blk_materialize_sym(st, d_in, d_emit, ne, (const BlkUnits *)c->d_hist.p, (const uint32_t *)c->d_codes.p,
                                              (uint16_t *)c->d_dec_sym.p, nsu <= (uint32_t)std::max(c->n_cu, 1)));
        HIP_TRY(hipStreamSynchronize(st));     // (su must outlive its copy)
        c->phase("lz77_sym");
        c->range.state = 1; c->range.nsu = nsu; c->range.max_len = max_len;
        if (state) *state = 1;
    }
    return LFX_OK;
} LFX_ABI_CATCH

extern "C" int lfx_decode_range_map(lfx_ctx *cc, void *d_map) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    (void)hipSetDevice(c->device);
    if (c->range.state < 0 || !d_map) { c->set_error("lfx_decode_range_map: no range_emit on this context"); return LFX_E_ARG; }
    if (c->range.state == 1) {
        const uint32_t nsu = c->range.nsu;
        const SymUnit *d_su = (const SymUnit *)((uint8_t *)c->d_dec_win.p + 32768ull * (std::max<uint32_t>(nsu, 1) + 1));
        LAUNCH_TRY(launch_window_rank_map(c->stream, (const uint16_t *)c->d_dec_sym.p, d_su, nsu, c->d_dec_maps.p, (uint16_t *)d_map));
    } else LAUNCH_TRY(launch_bytes_to_map(c->stream, c->range.d_out, c->range.total, (uint16_t *)d_map));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return LFX_OK;
} LFX_ABI_CATCH

extern "C" int lfx_decode_range_finish(lfx_ctx *cc, const void *d_maps, uint32_t rank, uint32_t *crc32, uint32_t *adler32) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    (void)hipSetDevice(c->device);
    hipStream_t st = c->stream;
    if (crc32) *crc32 = 0;
    if (adler32) *adler32 = 1;
    if (c->range.state < 0) { c->set_error("lfx_decode_range_finish: no range_emit on this context"); return LFX_E_ARG; }
    const uint64_t total = c->range.total;
    uint8_t *d_out = c->range.d_out;
    int rc;
    if (c->range.state == 1) {
        const uint32_t nsu = c->range.nsu;
        uint8_t *d_win = (uint8_t *)c->d_dec_win.p;
        uint8_t *d_init = d_win + 32768ull * std::max<uint32_t>(nsu, 1);        // the window in front of the slice
        const SymUnit *d_su = (const SymUnit *)(d_init + 32768);
        const uint8_t *init_win = nullptr;
        if (c->range.before) {
            if (!d_maps || !rank) { c->set_error("this slice reads the output of the ranks in front of it: their maps are needed"); return LFX_E_ARG; }
            if ((uintptr_t)d_maps & 15) { c->set_error("the gathered maps must be 16-byte aligned"); return LFX_E_ARG; }
            LAUNCH_TRY(launch_window_ranks(st, (const uint16_t *)d_maps, rank, d_init));
            init_win = d_init;
        }
        if (nsu >= 16)
            LAUNCH_TRY(launch_window_prefix(st, (const uint16_t *)c->d_dec_sym.p, d_su, nsu, c->d_dec_maps.p, d_win, init_win));
        else LAUNCH_TRY(launch_window_chain(st, (const uint16_t *)c->d_dec_sym.p, d_su, nsu, d_win, init_win));
        c->phase("win_chain");
        LAUNCH_TRY(launch_sym_substitute(st, (const uint16_t *)c->d_dec_sym.p, d_su, nsu, d_win, d_out, c->range.max_len, init_win));
        c->phase("substitute");
        c->range.state = 0;        // the slice holds bytes now
    }
    if (total) {
        if ((rc = c->d_res.reserve(256))) return rc;
        const uint64_t nspans = ck_nspans(total);
        if ((rc = c->d_ck.reserve(12 * nspans))) return rc;
        uint32_t *ck = (uint32_t *)c->d_ck.p;
        LAUNCH_TRY(launch_checksum(st, d_out, total, ck, ck + nspans, ck + 2 * nspans, (EncodeResult *)c->d_res.p, 3));
        HIP_TRY(hipMemcpyAsync(c->h_res, c->d_res.p, sizeof(EncodeResult), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const EncodeResult er = *(EncodeResult *)c->h_res;
        if (crc32) *crc32 = er.crc32;
        if (adler32) *adler32 = er.adler32;
    } else HIP_TRY(hipStreamSynchronize(st));
    c->phase("checksum");
    return LFX_OK;
} LFX_ABI_CATCH

extern "C" int lfx_decode_host(lfx_ctx *cc, int format, uint32_t flags, const void *in, uint64_t n, void *out,
                               uint64_t cap, uint64_t *out_len, uint64_t *consumed) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    (void)hipSetDevice(c->device);
    int rc;
    if ((rc = c->d_io_in.reserve(std::max<uint64_t>(n, 4)))) return rc;
    if ((rc = c->d_io_out.reserve(std::max<uint64_t>(cap, 4)))) return rc;
    // (lfx_hostio.h: page-locked buffers — lfx_host_alloc — go to the DMA engine as they are, pageable ones through slabs)
    if (int hr = host_to_device(c, c->d_io_in.p, in, n, c->stream)) { c->set_error("host to device copy failed"); return hr; }
    uint64_t ol = 0;
    rc = lfx_decode_device(cc, format, flags, c->d_io_in.p, n, c->d_io_out.p, cap, &ol, consumed);
    // (a page-locked `in` was only queued for DMA: no return before the stream has passed the copy, on any path)
    if (rc == LFX_E_DEVICE || rc == LFX_E_OOM || rc == LFX_E_ARG) { (void)hipStreamSynchronize(c->stream); return rc; }
    if (ol) { if (int hr = device_to_host(c, out, c->d_io_out.p, ol, c->stream)) { c->set_error("device to host copy failed"); return hr; } }
    if (out_len) *out_len = ol;
    return rc;
} LFX_ABI_CATCH

// Batch fast path: every stream's blocks go through the lane-parallel kernels, one block per stream and
// round (a block's start is only known once the block before it has been scanned; reference-made streams
// have two blocks).  A stream leaves the fast path — and is decoded again, exactly, by the serial kernel —
// on any anomaly: undecodable block, a block that runs past the stream's end or its output capacity, a
// back-reference that reaches in front of its block, more than BLOCK_ROUNDS blocks.
// fast[i] = 1: d_out holds the stream's bytes and res[i] is filled in.
namespace lfx {
// dict_end (the dictionary batch): a job's hist_avail = dict_len bytes of history lie in front of its first byte, ending there.
static int batch_fast(Ctx *c, const uint8_t *d_in, uint64_t n_in, uint8_t *d_out, uint32_t count,
                      const std::vector<InflateJob> &jobs, std::vector<uint8_t> &fast, std::vector<InflateResult> &res,
                      const uint8_t *dict_end = nullptr) {
    struct Live { uint32_t stream; uint64_t bit, produced; uint32_t nblocks; };
    std::vector<Live> live;
    fast.assign(count, 0);
    res.assign(count, InflateResult{});
    for (uint32_t i = 0; i < count; i++)
        if (jobs[i].in_len >= 64 && jobs[i].in_off + jobs[i].in_len <= n_in)
            live.push_back(Live{i, jobs[i].in_off * 8 + jobs[i].start_bit, 0, 0});
    int rc;
    for (uint32_t round = 0; round < BLOCK_ROUNDS && !live.empty(); round++) {
        const uint32_t nj = (uint32_t)live.size();
        std::vector<BlkJob> bj(nj);
        for (uint32_t k = 0; k < nj; k++) {
            const InflateJob &j = jobs[live[k].stream];
            bj[k] = BlkJob{live[k].bit, (j.in_off + j.in_len) * 8};
        }
        // (phase brackets of the first rounds only: the timer holds sixteen, and "fast" / "inflate" / "verify" close the call)
        const bool stamp = c->n_ev + 6 < Ctx::MAX_EV;
        std::vector<BlkInfo> bi;
        bool small = false;
        if ((rc = scan_round(c, d_in, n_in, bj, true, bi, small, stamp))) return rc;
        // blocks that scanned cleanly and fit are emitted; the others drop their stream out of the fast path
        std::vector<BlkEmit> emit;
        std::vector<uint32_t> owner;
        uint64_t total_codes = 0;
        for (uint32_t k = 0; k < nj; k++) {
            const InflateJob &j = jobs[live[k].stream];
            const BlkInfo &r = bi[k];
            if (r.status != BLK_OK || r.end_bit <= live[k].bit || r.end_bit > (j.in_off + j.in_len) * 8 ||
                live[k].produced + r.n_out > j.out_cap)
                continue;
            BlkEmit e = blk_emit_of(r, live[k].bit, k, j.out_off + live[k].produced, total_codes, j.hist_avail + live[k].produced);
            e.preload = e.hist != 0;
            e.dict_len = j.dict_len;
            emit.push_back(e);
            owner.push_back(k);
            total_codes += r.n_codes;
        }
        const uint32_t ne = (uint32_t)emit.size();
        std::vector<uint32_t> jf;
        if (ne && (rc = emit_round(c, d_in, n_in, emit, total_codes, small, d_out, jf, stamp, dict_end))) return rc;
        if (c->idx && ne) {   // (an index build: the blocks this round proved)
            std::vector<BlkEmit> ok;
            for (uint32_t q = 0; q < ne; q++) if (!jf[q]) ok.push_back(emit[q]);
            if ((rc = idx_record_chain(c, ok.data(), (uint32_t)ok.size(), (const BlkLanes *)c->d_dec_cand.p, 0, 0, false))) return rc;
        }
        std::vector<Live> next;
        for (uint32_t q = 0; q < ne; q++) {
            if (jf[q]) continue;                                 // reads in front of the block: serial kernel
            Live l = live[owner[q]];
            const BlkInfo &r = bi[owner[q]];
            l.produced += r.n_out;
            l.nblocks++;
            if (r.bfinal) {
                const InflateJob &j = jobs[l.stream];
                InflateResult &o = res[l.stream];
                o.end_bit = r.end_bit - j.in_off * 8;
                o.out_len = l.produced;
                o.blk_out_start = l.produced;
                o.final_seen = 1;
                o.nblocks = l.nblocks;
                fast[l.stream] = 1;
            } else { l.bit = r.end_bit; next.push_back(l); }
        }
        if (c->diag.debug) {
            uint32_t bad = 0, nfl = 0;
            for (uint32_t k = 0; k < nj; k++) bad += bi[k].status != BLK_OK;
            for (uint32_t q = 0; q < ne; q++) nfl += jf[q];
            fprintf(stderr, "[lfx] batch round %u: jobs=%u scan-not-ok=%u emitted=%u cross-block=%u continuing=%zu\n", round, nj, bad,
                    ne, nfl, next.size());
        }
        live.swap(next);
    }
    return LFX_OK;
}
}  // namespace lfx

namespace {
// behind the headers of a batch decode, in parse_headers' extra room: each stream's checksums and its bytes consumed
constexpr size_t batch_extra_bytes(uint32_t count) { return 16ull * count + 64; }

// The decode half of a batch: the streams placed (out_off / out_cap, here and in d_streams) and their headers parsed (hdrs, and
// d_hdrs with batch_extra_bytes of room behind them) → res[i] = stream i's verdict (trailer included), used[i] = its bytes
// consumed.
int decode_batch_placed(Ctx *c, int format, uint32_t count, const void *d_in, const uint64_t *in_off, const uint64_t *in_len,
                        void *d_out, const uint64_t *out_off, const uint64_t *out_cap, const std::vector<DecHeader> &hdrs,
                        DecStream *d_streams, DecHeader *d_hdrs, std::vector<InflateResult> &res, std::vector<uint64_t> *used,
                        const lfx_dict *dict) {
    hipStream_t st = c->stream;
    int rc;
    uint32_t *d_crc = (uint32_t *)(d_hdrs + count);
    uint32_t *d_adler = d_crc + count;
    uint64_t *d_consumed = (uint64_t *)(d_adler + count);
    std::vector<InflateJob> jobs(count);
    for (uint32_t i = 0; i < count; i++) {
        if (c->idx && (format == LFX_DEFLATE || hdrs[i].status == 0)) {   // (an index build: a member's first block)
            const uint64_t b = (in_off[i] + (format == LFX_DEFLATE ? 0 : hdrs[i].deflate_off)) * 8;
            c->idx->cand.push_back(IdxCand{b, b, out_off[i], IDX_BTYPE_READ});
        }
        InflateJob j{};
        j.in_off = in_off[i];
        j.in_len = in_len[i];
        j.start_bit = (format == LFX_DEFLATE ? 0 : hdrs[i].deflate_off) * 8;
        if (format != LFX_DEFLATE && hdrs[i].status != 0) j.in_len = 0;  // header failed: nothing to decode
        j.out_off = out_off[i];
        j.out_cap = out_cap[i];
        j.flags = 0;
        // (the dictionary batch: raw DEFLATE always reads it, zlib when FDICT was set and matched)
        if (dict && (format == LFX_DEFLATE || (hdrs[i].flags & HDR_DICT))) j.hist_avail = j.dict_len = dict->usable;
        jobs[i] = j;
    }
    // ---- lane-parallel path first; whatever it could not take goes through the exact serial kernel
    uint64_t n_in = 0;
    for (uint32_t i = 0; i < count; i++) n_in = std::max(n_in, in_off[i] + in_len[i]);
    std::vector<uint8_t> fast;
    std::vector<InflateResult> fres;
    if (c->diag.batch_serial) { fast.assign(count, 0); fres.assign(count, InflateResult{}); }
    else if ((rc = batch_fast(c, (const uint8_t *)d_in, n_in, (uint8_t *)d_out, count, jobs, fast, fres, dict ? dict->d_end() : nullptr))) return rc;
    c->phase("fast");
    std::vector<InflateJob> slow_jobs;
    std::vector<uint32_t> slow_idx;
    for (uint32_t i = 0; i < count; i++)
        if (!fast[i]) { slow_jobs.push_back(jobs[i]); slow_idx.push_back(i); }
    const uint32_t nslow = (uint32_t)slow_jobs.size();
    // d_dec_state holds the per-stream results the checksum / trailer kernels read: [count] then [nslow] scratch
    if ((rc = c->d_dec_streams.reserve(sizeof(InflateJob) * std::max<uint32_t>(nslow, 1)))) return rc;
    if ((rc = c->d_dec_state.reserve(sizeof(InflateResult) * ((size_t)count + nslow)))) return rc;
    InflateResult *d_res = (InflateResult *)c->d_dec_state.p, *d_slow = d_res + count;
    HIP_TRY(hipMemcpyAsync(d_res, fres.data(), sizeof(InflateResult) * count, hipMemcpyHostToDevice, st));
    if (nslow) {
        HIP_TRY(hipMemcpyAsync(c->d_dec_streams.p, slow_jobs.data(), sizeof(InflateJob) * nslow, hipMemcpyHostToDevice, st));
        if (dict)
            LAUNCH_TRY(launch_inflate_dict(st, (const uint8_t *)d_in, (uint8_t *)d_out, (const InflateJob *)c->d_dec_streams.p, d_slow, nslow,
                                           dict->d_end()));
        else
        LAUNCH_TRY(launch_inflate(st, (const uint8_t *)d_in, (uint8_t *)d_out, (const InflateJob *)c->d_dec_streams.p, d_slow, nslow));
        if (nslow == count) HIP_TRY(hipMemcpyAsync(d_res, d_slow, sizeof(InflateResult) * count, hipMemcpyDeviceToDevice, st));
        else for (uint32_t q = 0; q < nslow; q++)
            HIP_TRY(hipMemcpyAsync(d_res + slow_idx[q], d_slow + q, sizeof(InflateResult), hipMemcpyDeviceToDevice, st));
    }
    HIP_TRY(hipStreamSynchronize(st));   // (host vectors above must outlive the copies)
    c->phase("inflate");
    if (format != LFX_DEFLATE)
        LAUNCH_TRY(launch_checksum_ranges(st, (const uint8_t *)d_out, count, (const uint64_t *)d_streams + 2,
                                          sizeof(DecStream) / 8, (const uint64_t *)c->d_dec_state.p + 1,
                                          sizeof(InflateResult) / 8, d_crc, d_adler));   // out_off / out_len fields
    LAUNCH_TRY(launch_verify_trailers(st, format, count, (const uint8_t *)d_in, d_streams, d_hdrs,
                                      (InflateResult *)c->d_dec_state.p, d_crc, d_adler, d_consumed));
    res.resize(count);
    HIP_TRY(hipMemcpyAsync(res.data(), c->d_dec_state.p, sizeof(InflateResult) * count, hipMemcpyDeviceToHost, st));
    if (used) {
        used->resize(count);
        HIP_TRY(hipMemcpyAsync(used->data(), d_consumed, 8ull * count, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    c->phase("verify");
    return LFX_OK;
}

// the body of lfx_decode_batch_device: the headers, then the decode half at the caller's places
int decode_batch(Ctx *c, int format, uint32_t count, const void *d_in, const uint64_t *in_off, const uint64_t *in_len,
                 void *d_out, const uint64_t *out_off, const uint64_t *out_cap, std::vector<InflateResult> &res,
                 std::vector<uint64_t> *used = nullptr, const lfx_dict *dict = nullptr) {
    std::vector<DecStream> streams(count);
    for (uint32_t i = 0; i < count; i++) streams[i] = DecStream{in_off[i], in_len[i], out_off[i], out_cap[i]};
    int rc;
    std::vector<DecHeader> hdrs;
    DecStream *d_streams;
    DecHeader *d_hdrs;
    if ((rc = parse_headers(c, format, (const uint8_t *)d_in, streams, hdrs, batch_extra_bytes(count), &d_streams, &d_hdrs, dict))) return rc;
    c->phase("headers");
    return decode_batch_placed(c, format, count, d_in, in_off, in_len, d_out, out_off, out_cap, hdrs, d_streams, d_hdrs, res, used, dict);
}
}  // namespace

extern "C" int lfx_decode_batch_device(lfx_ctx *cc, int format, uint32_t count, const void *d_in,
                                       const uint64_t *in_off, const uint64_t *in_len, void *d_out,
                                       const uint64_t *out_off, const uint64_t *out_cap, uint64_t *out_len,
                                       int32_t *status) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    (void)hipSetDevice(c->device);
    c->n_ev = 0;
    c->phase("start");
    if (!count) return LFX_OK;
    std::vector<InflateResult> res;
    int rc = decode_batch(c, format, count, d_in, in_off, in_len, d_out, out_off, out_cap, res);
    if (rc) return rc;
    int worst = LFX_OK;
    for (uint32_t i = 0; i < count; i++) {
        if (out_len) out_len[i] = res[i].out_len;
        const int s = map_status(res[i].status);
        if (status) status[i] = s;
        if (s != LFX_OK && worst == LFX_OK) { worst = s; c->set_error(format_error(res[i].err, res[i].a0, res[i].a1)); }
    }
    return LFX_OK;  // per-stream results are in status[]
} LFX_ABI_CATCH

extern "C" int lfx_decode_batch_dict_device(lfx_ctx *cc, int format, const lfx_dict *dict, uint32_t count, const void *d_in,
                                            const uint64_t *in_off, const uint64_t *in_len, void *d_out, const uint64_t *out_off,
                                            const uint64_t *out_cap, uint64_t *out_len, int32_t *status) try {
    if (!cc) return LFX_E_DEVICE;
    if (format != LFX_ZLIB && format != LFX_DEFLATE) return LFX_E_ARG;
    if (!dict) return lfx_decode_batch_device(cc, format, count, d_in, in_off, in_len, d_out, out_off, out_cap, out_len, status);
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    if (dict->c != c) return LFX_E_ARG;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    (void)hipSetDevice(c->device);
    c->n_ev = 0;
    c->phase("start");
    if (!count) return LFX_OK;
    std::vector<InflateResult> res;
    int rc = decode_batch(c, format, count, d_in, in_off, in_len, d_out, out_off, out_cap, res, nullptr, dict);
    if (rc) return rc;
    int worst = LFX_OK;
    for (uint32_t i = 0; i < count; i++) {
        if (out_len) out_len[i] = res[i].out_len;
        const int s = map_status(res[i].status);
        if (status) status[i] = s;
        if (s != LFX_OK && worst == LFX_OK) { worst = s; c->set_error(format_error(res[i].err, res[i].a0, res[i].a1)); }
    }
    return LFX_OK;  // per-stream results are in status[]
} LFX_ABI_CATCH

// ------------------------------------------------------------------------------------------------
// gzip::MultiDecoder as one batch (lfx_decode_members_device).  Five steps: the candidate finder
// (lfx_members.hip), a header parse and a block walk of every candidate that produce no output, the chain from byte 0 on the
// host, ONE batch decode of the chained members, and the sequential member loop (decode_stream) for the rest of the input
// from the first member the batch did not settle.  Every error, every partial output and the clean end come from that loop,
// so the result is lfx_decode_device(LFX_GZIP, LFX_DEC_MULTI)'s by construction; the batch only settles members that loop
// would have decoded without a fault.
namespace {
constexpr uint32_t MEMBER_DENSE = 64;          // a tile with more candidates than this (one per 256 bytes) is not listed: a chain
                                               // start inside it goes through the sequential loop (a stored member full of magic)
constexpr uint32_t MEMBER_GROUP = 4096;        // candidates parsed and walked together, members decoded by one batch call
constexpr uint64_t MEMBER_HDR_BYTES = 64ull << 10;   // header bytes a candidate's parse may read (a longer header: sequential)

// the nested decodes record phases of their own: the members path names only its five (and "start")
struct PhaseMute {
    Ctx *c;
    int saved;
    explicit PhaseMute(Ctx *c_) : c(c_), saved(c_->timing_on) { c->timing_on = 0; }
    ~PhaseMute() { c->timing_on = saved; }
};

struct MemberWalk {
    uint64_t end_byte = 0;   // byte behind the member's last DEFLATE byte (its trailer starts here)
    uint64_t n_out = 0;
    uint8_t state = 0;       // 0 not walked, 1 walked to its BFINAL block, 2 not a member the walk could follow
};

// cand = the candidate offsets of d_in[0, n) in input order, without those of tiles denser than MEMBER_DENSE
int member_candidates(Ctx *c, const uint8_t *d_in, uint64_t n, std::vector<uint64_t> &cand) {
    hipStream_t st = c->stream;
    cand.clear();
    const uint64_t ntiles = member_tiles(n);
    if (!ntiles) return LFX_OK;
    int rc;
    if ((rc = c->d_dec_tmp.reserve(4 * ntiles))) return rc;
    LAUNCH_TRY(launch_member_count(st, d_in, n, (uint32_t *)c->d_dec_tmp.p));
    std::vector<uint32_t> cnt(ntiles);
    HIP_TRY(hipMemcpyAsync(cnt.data(), c->d_dec_tmp.p, 4 * ntiles, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<uint64_t> pos(ntiles);
    uint64_t total = 0;
    for (uint64_t t = 0; t < ntiles; t++) {
        if (cnt[t] > MEMBER_DENSE || cnt[t] == 0) { pos[t] = MEMBER_SKIP; continue; }
        pos[t] = total;
        total += cnt[t];
    }
    if (!total) return LFX_OK;
    if ((rc = c->d_dec_tmp.reserve(8 * ntiles + 8 * total))) return rc;
    uint64_t *d_pos = (uint64_t *)c->d_dec_tmp.p, *d_cand = d_pos + ntiles;
    HIP_TRY(hipMemcpyAsync(d_pos, pos.data(), 8 * ntiles, hipMemcpyHostToDevice, st));
    LAUNCH_TRY(launch_member_emit(st, d_in, n, d_pos, d_cand, total));
    cand.resize(total);
    HIP_TRY(hipMemcpyAsync(cand.data(), d_cand, 8 * total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return LFX_OK;
}

// the size path's pieces, defined with the size calls below
int run_walk(Ctx *c, const uint8_t *d_in, uint64_t n, const std::vector<WalkJob> &jobs, std::vector<WalkResult> &res);
bool walk_settled(const WalkResult &r, uint64_t out_before);
int size_stream(Ctx *c, int format, uint32_t flags, const uint8_t *d_in, uint64_t n, DecodeOutcome &oc, uint64_t base = 0,
                uint64_t out_at = 0, bool one_member = false, std::vector<lfx_member> *members = nullptr);

// header parse and block walk of candidates [k0, k1): walk[k] for each.  The decode follows a member's blocks with the scan
// kernel of the batch path, a block per round (no output); sizes_only: ONE launch of the size calls' walker.
int member_walk(Ctx *c, const uint8_t *d_in, uint64_t n, const std::vector<uint64_t> &cand, size_t k0, size_t k1, bool sizes_only,
                std::vector<MemberWalk> &walk) {
    const uint32_t cnt = (uint32_t)(k1 - k0);
    if (!cnt) return LFX_OK;
    int rc;
    std::vector<DecStream> ds(cnt);
    for (uint32_t i = 0; i < cnt; i++) ds[i] = DecStream{cand[k0 + i], std::min(n - cand[k0 + i], MEMBER_HDR_BYTES), 0, 0};
    std::vector<DecHeader> dh;
    if ((rc = parse_headers(c, LFX_GZIP, d_in, ds, dh))) return rc;
    struct Live { size_t k; uint64_t bit, end_bit, produced; };
    std::vector<Live> live;
    for (uint32_t i = 0; i < cnt; i++) {
        const size_t k = k0 + i;
        walk[k].state = 2;
        if (dh[i].status != 0) continue;
        const uint64_t data = cand[k] + dh[i].deflate_off, lim = member_walk_limit(cand, k, data, n);
        if (lim > data) live.push_back(Live{k, data * 8, lim * 8, 0});
    }
    auto settle = [&](const Live &l, uint64_t end_bit, uint64_t n_out) {
        MemberWalk &w = walk[l.k];
        w.end_byte = (end_bit + 7) / 8;
        w.n_out = n_out;
        w.state = 1;
    };
    if (sizes_only) {
        std::vector<WalkJob> jobs;
        for (const Live &l : live) jobs.push_back(WalkJob{l.bit, l.end_bit, 0});
        std::vector<WalkResult> wr;
        if ((rc = run_walk(c, d_in, n, jobs, wr))) return rc;
        for (size_t q = 0; q < jobs.size(); q++)
            if (wr[q].status == WALK_FINAL && walk_settled(wr[q], 0)) settle(live[q], wr[q].end_bit, wr[q].n_out);
        return LFX_OK;
    }
    for (uint32_t round = 0; round < BLOCK_ROUNDS && !live.empty(); round++) {
        std::vector<BlkJob> bj;
        for (const Live &l : live) bj.push_back(BlkJob{l.bit, l.end_bit});
        std::vector<BlkInfo> bi;
        bool small = false;
        if ((rc = scan_round(c, d_in, n, bj, false, bi, small))) return rc;
        std::vector<Live> next;
        for (size_t q = 0; q < live.size(); q++) {
            Live l = live[q];
            const BlkInfo &r = bi[q];
            if (r.status != BLK_OK || r.end_bit <= l.bit || r.end_bit > l.end_bit) continue;    // state stays 2
            l.produced += r.n_out;
            if (r.bfinal) settle(l, r.end_bit, l.produced);
            else { l.bit = r.end_bit; next.push_back(l); }
        }
        live.swap(next);
    }
    return LFX_OK;   // (still live after the last round: a long member, state 2)
}

// the chained members that the walk settled through the batch decoder, MEMBER_GROUP at a time: keep = the first one it does
// not verify (or that comes out other than walked)
int members_batch(Ctx *c, const uint8_t *d_in, uint8_t *d_out, const std::vector<lfx_member> &chain, const std::vector<uint8_t> &walked,
                  size_t &keep) {
    int rc;
    for (size_t e0 = 0; e0 < chain.size() && keep == chain.size();) {
        std::vector<size_t> idx;
        size_t e1 = e0;
        for (; e1 < chain.size() && idx.size() < MEMBER_GROUP; e1++)
            if (walked[e1]) idx.push_back(e1);
        e0 = e1;
        if (idx.empty()) continue;
        const uint32_t nb = (uint32_t)idx.size();
        std::vector<uint64_t> in_off(nb), in_len(nb), out_off(nb), out_cap(nb), used;
        for (uint32_t q = 0; q < nb; q++) {
            const lfx_member &m = chain[idx[q]];
            in_off[q] = m.in_off; in_len[q] = m.in_len; out_off[q] = m.out_off; out_cap[q] = m.out_len;
        }
        std::vector<InflateResult> res;
        {
            PhaseMute mute(c);
            if ((rc = decode_batch(c, LFX_GZIP, nb, d_in, in_off.data(), in_len.data(), d_out, out_off.data(), out_cap.data(), res,
                                   &used)))
                return rc;
        }
        for (uint32_t q = 0; q < nb; q++)
            if (res[q].status != 0 || used[q] != in_len[q] || res[q].out_len != out_cap[q]) { keep = idx[q]; break; }
    }
    return LFX_OK;
}

// The members of d_in[0, n) and the verdict of the sequential member loop over them.  Candidates; the header parse and the
// walk of a group of candidates at a time, from the one the chain has reached; the chain from byte 0 on the host; then, for
// the decode, the chained members through the batch decoder; the member loop from the first member not settled.
// sizes_only: the chain of the size calls — the walker instead of scan rounds, no output, no capacity and no batch; a start the
// walk did not settle goes through size_stream for one member instead of decode_stream.
int members_chain(Ctx *c, const uint8_t *d_in, uint64_t n, uint8_t *d_out, uint64_t cap, bool sizes_only, DecodeOutcome &oc,
                  std::vector<lfx_member> &members) {
    auto loop = [&](DecodeOutcome &o, uint64_t base, uint64_t out_at, bool one_member, std::vector<lfx_member> *got) {
        PhaseMute mute(c);
        return sizes_only ? size_stream(c, LFX_GZIP, LFX_DEC_MULTI, d_in, n, o, base, out_at, one_member, got)
                          : decode_stream(c, LFX_GZIP, LFX_DEC_MULTI, d_in, n, d_out, cap, o, base, out_at, one_member, got);
    };
    int rc;
    // ---- 1. candidates
    std::vector<uint64_t> cand;
    if ((rc = member_candidates(c, d_in, n, cand))) return rc;
    c->phase("candidates");
    // ---- 2.-4. header parse and walk, the chain
    std::vector<MemberWalk> walk(cand.size());
    std::vector<lfx_member> chain;
    std::vector<uint8_t> walked;   // chain[e] was settled by the walk (else: already decoded and verified by the sequential loop)
    uint64_t base = 0, out_at = 0;
    size_t walked_to = 0;   // candidates in front of this one were walked or passed over
    while (base < n) {
        const size_t k = (size_t)(std::lower_bound(cand.begin(), cand.end(), base) - cand.begin());
        const bool is_cand = k < cand.size() && cand[k] == base;
        if (is_cand && k >= walked_to) {
            const size_t k1 = std::min<size_t>(cand.size(), k + MEMBER_GROUP);
            if ((rc = member_walk(c, d_in, n, cand, k, k1, sizes_only, walk))) return rc;
            walked_to = k1;
            if (c->n_ev + 6 < Ctx::MAX_EV) c->phase(sizes_only ? "walk_size" : "walk");
        }
        if (is_cand && walk[k].state == 1) {
            const MemberWalk &w = walk[k];
            // a cut trailer, output that does not fit: the tail says so
            if (n - w.end_byte < 8 || (!sizes_only && w.n_out > cap - out_at)) break;
            chain.push_back(lfx_member{base, w.end_byte + 8 - base, out_at, w.n_out});
            walked.push_back(1);
            base = w.end_byte + 8;
            out_at += w.n_out;
            continue;
        }
        // no candidate here (a dense tile, reserved FLG bits, not a header at all), or one the walk could not follow (a long
        // member, a damaged one): ONE member through the sequential loop; anything but a verified member ends the chain
        DecodeOutcome one;
        std::vector<lfx_member> got;
        if ((rc = loop(one, base, out_at, true, &got))) return rc;
        if (!one.more || got.size() != 1) break;
        chain.push_back(got[0]);
        walked.push_back(0);
        base = one.consumed;
        out_at = one.out_len;
    }
    c->phase("chain");
    // ---- 5. the decode: the batch; the tail starts at the first member it does not settle
    size_t keep = chain.size();
    if (!sizes_only) {
        if ((rc = members_batch(c, d_in, d_out, chain, walked, keep))) return rc;
        c->phase("batch");
    }
    if (keep < chain.size()) { base = chain[keep].in_off; out_at = chain[keep].out_off; }
    // ---- 6. the sequential member loop from there on: the exact verdict, partial output and clean end
    members.assign(chain.begin(), chain.begin() + keep);
    if ((rc = loop(oc, base, out_at, false, &members))) return rc;
    c->phase("tail");
    return LFX_OK;
}

// what the four members entry points hand back
int members_out(Ctx *c, const DecodeOutcome &oc, const std::vector<lfx_member> &got, uint64_t *out_len, uint64_t *consumed,
                lfx_member *members, uint32_t max_members, uint32_t *n_members) {
    if (out_len) *out_len = oc.out_len;
    if (consumed) *consumed = oc.consumed;
    if (n_members) *n_members = (uint32_t)std::min<size_t>(got.size(), 0xFFFFFFFFu);
    if (members) memcpy(members, got.data(), sizeof(lfx_member) * std::min<size_t>(got.size(), max_members));
    if (oc.status != LFX_OK) c->set_error(oc.msg);
    return oc.status;
}
}  // namespace

extern "C" int lfx_decode_members_device(lfx_ctx *cc, const void *d_in, uint64_t n, void *d_out, uint64_t cap,
                                         uint64_t *out_len, uint64_t *consumed, lfx_member *members, uint32_t max_members,
                                         uint32_t *n_members) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    (void)hipSetDevice(c->device);
    c->n_ev = 0;
    c->phase("start");
    DecodeOutcome oc;
    std::vector<lfx_member> got;
    int rc = members_chain(c, (const uint8_t *)d_in, n, (uint8_t *)d_out, cap, false, oc, got);
    if (rc) return rc;
    if (oc.out_len > cap) oc.out_len = cap;  // (as lfx_decode_device)
    return members_out(c, oc, got, out_len, consumed, members, max_members, n_members);
} LFX_ABI_CATCH

extern "C" int lfx_decode_members_host(lfx_ctx *cc, const void *in, uint64_t n, void *out, uint64_t cap, uint64_t *out_len,
                                       uint64_t *consumed, lfx_member *members, uint32_t max_members, uint32_t *n_members) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    (void)hipSetDevice(c->device);
    int rc;
    if ((rc = c->d_io_out.reserve(std::max<uint64_t>(cap, 4)))) return rc;
    if ((rc = stage_in(c, in, n))) return rc;
    uint64_t ol = 0;
    rc = lfx_decode_members_device(cc, c->d_io_in.p, n, c->d_io_out.p, cap, &ol, consumed, members, max_members, n_members);
    if (rc == LFX_E_DEVICE || rc == LFX_E_OOM || rc == LFX_E_ARG) { (void)hipStreamSynchronize(c->stream); return rc; }
    if (ol) { if (int hr = device_to_host(c, out, c->d_io_out.p, ol, c->stream)) { c->set_error("device to host copy failed"); return hr; } }
    if (out_len) *out_len = ol;
    return rc;
} LFX_ABI_CATCH

// ------------------------------------------------------------------------------------------------
// BGZF reads by virtual offset (lfx_bgzf_read_*).  Four steps: the walk of every read's BSIZE chain (on the
// device by bgzf_hop_kernel, in the host call on the CPU — the same bgzf_walk of lfx_bgzf.h) that settles out_len, next_voff
// and n_blocks from headers and ISIZEs alone and lists the (read, block) segments; the plan on the host (the distinct blocks
// in file order); per group of MEMBER_GROUP blocks ONE decode_batch into scratch, which verifies each block's CRC-32; and the
// gather of the wanted bytes into the reads' output ranges.
namespace {
struct BgzfBlock {
    uint64_t coffset, in_off;   // in the file; in the buffer the decode reads
    uint32_t blen, isize;
};

std::string bgzf_walk_message(const BgzfWalk &w) {
    char b[160];
    switch (w.err) {
    case BGZF_ERR_RANGE: snprintf(b, sizeof b, "BGZF read: coffset %llu lies outside the bytes held", (unsigned long long)w.err_coff); break;
    case BGZF_ERR_HEADER: snprintf(b, sizeof b, "BGZF read: no BGZF block header at coffset %llu", (unsigned long long)w.err_coff); break;
    case BGZF_ERR_ISIZE: snprintf(b, sizeof b, "BGZF read: the block at coffset %llu has an ISIZE above 65536", (unsigned long long)w.err_coff); break;
    case BGZF_ERR_CUT: snprintf(b, sizeof b, "BGZF read: the block at coffset %llu does not end inside the bytes held", (unsigned long long)w.err_coff); break;
    case BGZF_ERR_UOFFSET: snprintf(b, sizeof b, "BGZF read: uoffset lies behind the ISIZE of the block at coffset %llu", (unsigned long long)w.err_coff); break;
    default: snprintf(b, sizeof b, "BGZF read failed at coffset %llu", (unsigned long long)w.err_coff);
    }
    return b;
}

// rules 7 and 11 (include/lfx.h): what needs no device
int bgzf_check_args(Ctx *c, uint32_t count, const lfx_bgzf_read *reads, const lfx_bgzf_result *res) {
    if (!reads || !res) { c->set_error("BGZF read: reads and res must not be NULL"); return LFX_E_ARG; }
    std::vector<std::pair<uint64_t, uint64_t>> rg;
    rg.reserve(count);
    for (uint32_t i = 0; i < count; i++) {
        if (!reads[i].len) continue;
        const uint64_t end = reads[i].out_off + reads[i].len;
        rg.emplace_back(reads[i].out_off, end < reads[i].out_off ? ~0ull : end);
    }
    std::sort(rg.begin(), rg.end());
    for (size_t k = 1; k < rg.size(); k++)
        if (rg[k].first < rg[k - 1].second) {
            char b[128];
            snprintf(b, sizeof b, "BGZF read: two output ranges overlap at byte %llu", (unsigned long long)rg[k].first);
            c->set_error(b);
            return LFX_E_ARG;
        }
    return LFX_OK;
}

// the walk on the device: walk[i] for every read, and (want_segs) the segments of all reads, each read's in walk order.  At
// most three round trips whatever the reads are: the walk with a list sized by a guess, the walk again with the exact sizes
// when a read had more segments than guessed, the list.
int bgzf_hop_device(Ctx *c, const uint8_t *d_in, uint64_t in_base, uint64_t n, uint32_t count, const lfx_bgzf_read *reads,
                    bool want_segs, std::vector<BgzfWalk> &walk, std::vector<BgzfSeg> &segs) {
    hipStream_t st = c->stream;
    int rc;
    walk.resize(count);
    segs.clear();
    std::vector<uint64_t> off(count + 1, 0);
    if (want_segs) {
        // a block of 64 KiB of output seldom takes less than 8 KiB of input
        constexpr uint64_t GUESS_CAP = 1ull << 20;
        uint64_t total = 0;
        for (uint32_t i = 0; i < count && total <= GUESS_CAP; i++) {
            const uint64_t co = reads[i].voff >> 16;
            const uint64_t by_in = co >= in_base && co - in_base <= n ? (in_base + n - co) / 8192 + 2 : 0;
            total += std::min(reads[i].len / 32768 + 2, by_in);
            off[i + 1] = total;
        }
        if (total > GUESS_CAP) std::fill(off.begin(), off.end(), 0);    // count first, then list
    }
    const size_t sz_reads = sizeof(lfx_bgzf_read) * count, sz_off = 8ull * (count + 1), sz_walk = sizeof(BgzfWalk) * count;
    for (int pass = 0; pass < 2; pass++) {
        const uint64_t slots = off[count];
        if ((rc = c->d_bgzf_meta.reserve(sz_reads + sz_off + sz_walk + sizeof(BgzfSeg) * slots + 64))) return rc;
        uint8_t *base = (uint8_t *)c->d_bgzf_meta.p;
        lfx_bgzf_read *d_reads = (lfx_bgzf_read *)base;
        uint64_t *d_off = (uint64_t *)(base + sz_reads);
        BgzfWalk *d_walk = (BgzfWalk *)(base + sz_reads + sz_off);
        BgzfSeg *d_segs = (BgzfSeg *)(base + sz_reads + sz_off + sz_walk);
        HIP_TRY(hipMemcpyAsync(d_reads, reads, sz_reads, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_off, off.data(), sz_off, hipMemcpyHostToDevice, st));
        LAUNCH_TRY(launch_bgzf_hop(st, d_in, in_base, n, count, d_reads, d_off, want_segs && slots ? d_segs : nullptr, d_walk));
        HIP_TRY(hipMemcpyAsync(walk.data(), d_walk, sz_walk, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (!want_segs) return LFX_OK;
        bool fits = true;
        for (uint32_t i = 0; i < count; i++) fits = fits && walk[i].n_blocks <= off[i + 1] - off[i];
        if (fits) {
            if (!slots) return LFX_OK;
            std::vector<BgzfSeg> all(slots);
            HIP_TRY(hipMemcpyAsync(all.data(), d_segs, sizeof(BgzfSeg) * slots, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            for (uint32_t i = 0; i < count; i++) segs.insert(segs.end(), all.begin() + off[i], all.begin() + off[i] + walk[i].n_blocks);
            return LFX_OK;
        }
        for (uint32_t i = 0; i < count; i++) off[i + 1] = off[i] + walk[i].n_blocks;
    }
    c->set_error("BGZF read: the segment list did not fit its exact size");
    return LFX_E_DEVICE;
}

// segs sorted by (coffset, read) — a read's segments stay in walk order, the walk only moves forward — and the distinct blocks
void bgzf_plan(std::vector<BgzfSeg> &segs, std::vector<BgzfBlock> &blocks) {
    std::sort(segs.begin(), segs.end(), [](const BgzfSeg &a, const BgzfSeg &b) {
        return a.coffset != b.coffset ? a.coffset < b.coffset : a.read < b.read;
    });
    blocks.clear();
    for (const BgzfSeg &s : segs)
        if (blocks.empty() || blocks.back().coffset != s.coffset) blocks.push_back(BgzfBlock{s.coffset, 0, s.blen, s.isize});
}

// decode and gather: blocks[i].in_off is block i's first byte in d_src; read r's bytes go to d_out + dst[r].  A block that
// fails ends every read that touches it there (rule 5): walk[r] becomes that verdict, msg[r] its message.
int bgzf_run(Ctx *c, const uint8_t *d_src, const std::vector<BgzfSeg> &segs, const std::vector<BgzfBlock> &blocks, uint8_t *d_out,
             const std::vector<uint64_t> &dst, std::vector<BgzfWalk> &walk, std::vector<std::string> &msg) {
    hipStream_t st = c->stream;
    int rc;
    std::vector<uint8_t> failed(walk.size(), 0);
    size_t s0 = 0;
    for (size_t g0 = 0; g0 < blocks.size(); g0 += MEMBER_GROUP) {
        const uint32_t nb = (uint32_t)std::min<size_t>(MEMBER_GROUP, blocks.size() - g0);
        std::vector<uint64_t> in_off(nb), in_len(nb), out_off(nb), out_cap(nb), used;
        uint64_t at = 0;
        for (uint32_t q = 0; q < nb; q++) {
            const BgzfBlock &b = blocks[g0 + q];
            in_off[q] = b.in_off; in_len[q] = b.blen; out_off[q] = at; out_cap[q] = b.isize;
            at += (b.isize + 15u) & ~15u;       // (16-byte aligned: the gather's dword loads never leave a block's slot)
        }
        if ((rc = c->d_bgzf_scratch.reserve(std::max<uint64_t>(at, 16)))) return rc;
        uint8_t *d_scratch = (uint8_t *)c->d_bgzf_scratch.p;
        std::vector<InflateResult> res;
        {
            PhaseMute mute(c);
            if ((rc = decode_batch(c, LFX_GZIP, nb, d_src, in_off.data(), in_len.data(), d_scratch, out_off.data(), out_cap.data(), res,
                                   &used)))
                return rc;
        }
        if (c->n_ev + 2 < Ctx::MAX_EV) c->phase("batch");
        std::vector<BgzfCopy> tasks;
        const uint64_t last_co = blocks[g0 + nb - 1].coffset;
        uint32_t q = 0;
        for (; s0 < segs.size() && segs[s0].coffset <= last_co; s0++) {
            const BgzfSeg &s = segs[s0];
            while (blocks[g0 + q].coffset < s.coffset) q++;
            if (failed[s.read]) continue;
            const InflateResult &r = res[q];
            if (r.status != 0 || r.out_len != s.isize || used[q] != s.blen) {
                failed[s.read] = 1;
                BgzfWalk &w = walk[s.read];
                w.status = LFX_E_INVALID_DATA;
                w.out_len = s.out_pos;
                w.n_blocks = s.ord;
                w.next_voff = s.coffset << 16 | s.first;
                w.err_coff = s.coffset;
                char b[96];
                snprintf(b, sizeof b, "BGZF block at coffset %llu: ", (unsigned long long)s.coffset);
                if (r.status != 0 && r.status != 3) msg[s.read] = b + format_error(r.err, r.a0, r.a1);
                else if (r.status == 3 || r.out_len != s.isize) msg[s.read] = std::string(b) + "the decoded length differs from ISIZE";
                else msg[s.read] = std::string(b) + "the member does not end at BSIZE + 1";
                continue;
            }
            for (uint32_t p = s.first; p < s.last; p += BGZF_GATHER_PIECE)
                tasks.push_back(BgzfCopy{out_off[q] + p, dst[s.read] + s.out_pos + (p - s.first), std::min(BGZF_GATHER_PIECE, s.last - p), 0});
        }
        if (!tasks.empty()) {
            if ((rc = c->d_bgzf_tasks.reserve(sizeof(BgzfCopy) * tasks.size()))) return rc;
            HIP_TRY(hipMemcpyAsync(c->d_bgzf_tasks.p, tasks.data(), sizeof(BgzfCopy) * tasks.size(), hipMemcpyHostToDevice, st));
            LAUNCH_TRY(launch_bgzf_gather(st, d_scratch, d_out, (const BgzfCopy *)c->d_bgzf_tasks.p, (uint32_t)tasks.size()));
        }
        HIP_TRY(hipStreamSynchronize(st));     // (the task list must outlive its copy; the next group decodes into the same scratch)
        if (c->n_ev + 1 < Ctx::MAX_EV) c->phase("gather");
    }
    return LFX_OK;
}

// res[] and the call's return value from the walks (rule 8).  The ONLY place that writes res: every return in front of it — a
// refusal of the call, a device error — leaves res as the caller set it (include/lfx.h; Context._bgzf_call relies on it)
int bgzf_finish(Ctx *c, uint32_t count, const std::vector<BgzfWalk> &walk, const std::vector<std::string> &msg, lfx_bgzf_result *res) {
    int worst = LFX_OK;
    for (uint32_t i = 0; i < count; i++) {
        res[i].out_len = walk[i].out_len;
        res[i].next_voff = walk[i].next_voff;
        res[i].status = walk[i].status;
        res[i].n_blocks = walk[i].n_blocks;
        if (walk[i].status != LFX_OK && worst == LFX_OK) {
            worst = walk[i].status;
            c->set_error(msg[i].empty() ? bgzf_walk_message(walk[i]) : msg[i]);
        }
    }
    return worst;
}
}  // namespace

extern "C" int lfx_bgzf_read_device(lfx_ctx *cc, const void *d_in, uint64_t in_base, uint64_t n, uint32_t count,
                                    const lfx_bgzf_read *reads, void *d_out, lfx_bgzf_result *res, uint64_t *blocks_decoded) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    (void)hipSetDevice(c->device);
    c->n_ev = 0;
    c->phase("start");
    if (blocks_decoded) *blocks_decoded = 0;
    if (!count) return LFX_OK;
    int rc;
    if ((rc = bgzf_check_args(c, count, reads, res))) return rc;
    if (in_base + n < in_base || (in_base + n) >> 48) { c->set_error("BGZF read: the bytes held end behind coffset 2^48"); return LFX_E_ARG; }
    std::vector<BgzfWalk> walk;
    std::vector<BgzfSeg> segs;
    if ((rc = bgzf_hop_device(c, (const uint8_t *)d_in, in_base, n, count, reads, d_out != nullptr, walk, segs))) return rc;
    c->phase("hop");
    std::vector<std::string> msg(count);
    if (d_out && !segs.empty()) {
        std::vector<BgzfBlock> blocks;
        bgzf_plan(segs, blocks);
        for (BgzfBlock &b : blocks) b.in_off = b.coffset - in_base;
        std::vector<uint64_t> dst(count);
        for (uint32_t i = 0; i < count; i++) dst[i] = reads[i].out_off;
        c->phase("plan");
        if ((rc = bgzf_run(c, (const uint8_t *)d_in, segs, blocks, (uint8_t *)d_out, dst, walk, msg))) return rc;
        if (blocks_decoded) *blocks_decoded = blocks.size();
    }
    return bgzf_finish(c, count, walk, msg, res);
} LFX_ABI_CATCH

extern "C" int lfx_bgzf_read_host(lfx_ctx *cc, const void *in_, uint64_t in_base, uint64_t n, uint32_t count,
                                  const lfx_bgzf_read *reads, void *out, lfx_bgzf_result *res, uint64_t *blocks_decoded) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    (void)hipSetDevice(c->device);
    c->n_ev = 0;
    c->phase("start");
    if (blocks_decoded) *blocks_decoded = 0;
    if (!count) return LFX_OK;
    int rc;
    if ((rc = bgzf_check_args(c, count, reads, res))) return rc;
    if (in_base + n < in_base || (in_base + n) >> 48) { c->set_error("BGZF read: the bytes held end behind coffset 2^48"); return LFX_E_ARG; }
    // the walk on the CPU over the caller's bytes: the file is not uploaded
    const uint8_t *in = (const uint8_t *)in_;
    const uint64_t lo = in_base, hi = in_base + n;
    std::vector<BgzfWalk> walk(count);
    std::vector<BgzfSeg> segs;
    auto fetch = [&](uint64_t p, uint8_t *w) {
        for (uint32_t k = 0; k < BGZF_WINDOW; k++) {
            const uint64_t a = p + k - 4;
            w[k] = a >= lo && a < hi ? in[a - lo] : 0;
        }
    };
    for (uint32_t i = 0; i < count; i++) {
        if (out) bgzf_walk(reads[i], i, lo, hi, fetch, [&](const BgzfSeg &s) { segs.push_back(s); }, walk[i]);
        else bgzf_walk(reads[i], i, lo, hi, fetch, [](const BgzfSeg &) {}, walk[i]);
    }
    c->phase("hop");
    std::vector<std::string> msg(count);
    if (out && !segs.empty()) {
        // only the distinct covered blocks cross the link, packed back to back
        std::vector<BgzfBlock> blocks;
        bgzf_plan(segs, blocks);
        uint64_t packed = 0, total = 0;
        for (BgzfBlock &b : blocks) { b.in_off = packed; packed += b.blen; }
        std::vector<uint8_t> pack(packed);
        for (const BgzfBlock &b : blocks) memcpy(pack.data() + b.in_off, in + (b.coffset - lo), b.blen);
        std::vector<uint64_t> dst(count);
        for (uint32_t i = 0; i < count; i++) { dst[i] = total; total += walk[i].out_len; }
        if ((rc = c->d_bgzf_pack.reserve(std::max<uint64_t>(packed, 4)))) return rc;
        if ((rc = c->d_io_out.reserve(std::max<uint64_t>(total, 4)))) return rc;
        if (int hr = host_to_device(c, c->d_bgzf_pack.p, pack.data(), packed, c->stream)) { c->set_error("host to device copy failed"); return hr; }
        c->phase("plan");
        if ((rc = bgzf_run(c, (const uint8_t *)c->d_bgzf_pack.p, segs, blocks, (uint8_t *)c->d_io_out.p, dst, walk, msg))) return rc;
        if (blocks_decoded) *blocks_decoded = blocks.size();
        // the reads' byte ranges come back: a few long reads each straight into its range, many reads in one transfer
        const uint8_t *d_res = (const uint8_t *)c->d_io_out.p;
        if (count <= 8) {
            for (uint32_t i = 0; i < count; i++)
                if (walk[i].out_len)
                    if (int hr = device_to_host(c, (uint8_t *)out + reads[i].out_off, d_res + dst[i], walk[i].out_len, c->stream)) {
                        c->set_error("device to host copy failed");
                        return hr;
                    }
        } else if (total) {
            std::vector<uint8_t> back(total);
            if (int hr = device_to_host(c, back.data(), d_res, total, c->stream)) { c->set_error("device to host copy failed"); return hr; }
            for (uint32_t i = 0; i < count; i++)
                if (walk[i].out_len) memcpy((uint8_t *)out + reads[i].out_off, back.data() + dst[i], walk[i].out_len);
        }
    }
    return bgzf_finish(c, count, walk, msg, res);
} LFX_ABI_CATCH

// host only: uncompressed offset -> virtual offset through a member table
extern "C" int lfx_members_voffset(const lfx_member *members, uint32_t n_members, int swapped, uint64_t uoff, uint64_t *voff) {
    if (!voff || (n_members && !members)) return LFX_E_ARG;
    auto u_off = [&](uint32_t i) { return swapped ? members[i].out_off : members[i].in_off; };
    auto u_len = [&](uint32_t i) { return swapped ? members[i].out_len : members[i].in_len; };
    auto c_off = [&](uint32_t i) { return swapped ? members[i].in_off : members[i].out_off; };
    auto c_len = [&](uint32_t i) { return swapped ? members[i].in_len : members[i].out_len; };
    const uint64_t total = n_members ? u_off(n_members - 1) + u_len(n_members - 1) : 0;
    if (uoff > total) return LFX_E_ARG;
    uint64_t co, uo = 0;
    if (uoff == total) co = n_members ? c_off(n_members - 1) + c_len(n_members - 1) : 0;
    else {
        uint32_t lo = 0, hi = n_members;        // the last member that starts at or in front of uoff
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (u_off(mid) <= uoff) lo = mid; else hi = mid;
        }
        co = c_off(lo);
        uo = uoff - u_off(lo);
    }
    if (uo > 0xffff || co >> 48) return LFX_E_ARG;     // not a BGZF table: the position has no virtual offset
    *voff = co << 16 | uo;
    return LFX_OK;
}

// ------------------------------------------------------------------------------------------------
// Decoded size without decoding (lfx_decode_size_*).  The verdict of the matching decode call — status,
// bytes produced, bytes consumed, message — without an output buffer: the blocks are walked on the device by
// blk_walk_size_kernel (no output, no code words, no checksum), and whatever the walker does not settle is decided by the
// exact serial kernel in its count-only mode, from the stream's start, as the decode paths fall back to it.
namespace {
int run_walk(Ctx *c, const uint8_t *d_in, uint64_t n, const std::vector<WalkJob> &jobs, std::vector<WalkResult> &res) {
    const size_t nj = jobs.size();
    res.resize(nj);
    if (!nj) return LFX_OK;
    int rc;
    if ((rc = c->d_dec_streams.reserve(sizeof(WalkJob) * nj))) return rc;
    if ((rc = c->d_dec_state.reserve(sizeof(WalkResult) * nj))) return rc;
    // (ranges of a few tens of KB: 256 lanes a job, as batch_fast picks the scan's instance)
    uint64_t range_bits = 0;
    for (const WalkJob &j : jobs) {
        const uint64_t e = j.stop_bit > j.start_bit && j.stop_bit < j.end_bit ? j.stop_bit : j.end_bit;
        range_bits += e > j.start_bit ? e - j.start_bit : 0;
    }
    const bool small = range_bits / nj < (512ull << 10);
    HIP_TRY(hipMemcpyAsync(c->d_dec_streams.p, jobs.data(), sizeof(WalkJob) * nj, hipMemcpyHostToDevice, c->stream));
    LAUNCH_TRY(launch_blk_walk_size(c->stream, d_in, n, (const WalkJob *)c->d_dec_streams.p, (uint32_t)nj,
                                    (WalkResult *)c->d_dec_state.p, small));
    HIP_TRY(hipMemcpyAsync(res.data(), c->d_dec_state.p, sizeof(WalkResult) * nj, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return LFX_OK;
}
bool walk_settled(const WalkResult &r, uint64_t out_before) {
    return r.status != WALK_STUCK && (r.reach == INT64_MAX || (int64_t)out_before + r.reach >= 0);
}

}  // namespace

namespace lfx {
// `consumed` behind an "Invalid huffman coded stream" verdict.  The reference's decoder skips 16 bits it never read when a
// code is unassigned (huffman.rs:157-179), and inflate_kernel's end_bit counts them as the decode's `consumed` does; what
// the reference's reader has pulled from its input at that point is the shortest prefix of the stream that still gives the
// same verdict.  That prefix is found with the exact kernel itself: the failing block again, count-only, on the two or three
// candidate lengths in ONE launch (only on this rare verdict).  probes[i]: stream base, stream length, the exact path's
// result → used[i] = bytes of the stream consumed.
int huff_consumed(Ctx *c, const uint8_t *d_in, const std::vector<HuffProbe> &probes, std::vector<uint64_t> &used) {
    used.assign(probes.size(), 0);
    std::vector<InflateJob> jobs;
    std::vector<size_t> owner;
    for (size_t i = 0; i < probes.size(); i++) {
        const HuffProbe &p = probes[i];
        const uint64_t hi = std::min<uint64_t>((p.r.end_bit + 7) / 8, p.in_len);
        const uint64_t before = p.r.end_bit >= 16 ? p.r.end_bit - 16 : 0;
        used[i] = hi;
        for (uint64_t k = std::max<uint64_t>((before + 7) / 8, (p.r.blk_start_bit + 7) / 8); k < hi; k++) {
            InflateJob j{};
            j.in_off = p.in_off; j.in_len = k; j.start_bit = p.r.blk_start_bit;
            j.out_cap = ~0ull; j.hist_avail = p.hist + p.r.blk_out_start; j.flags = JOB_COUNT_ONLY;
            jobs.push_back(j);
            owner.push_back(i);
        }
    }
    std::vector<InflateResult> res;
    if (int rc = run_jobs(c, d_in, nullptr, jobs, res)) return rc;
    for (size_t q = jobs.size(); q-- > 0;) {      // (descending lengths: the shortest prefix with the same verdict wins)
        const InflateResult &r = probes[owner[q]].r, &t = res[q];
        if (t.status == r.status && t.err == r.err && t.end_bit == r.end_bit && t.out_len == r.out_len - r.blk_out_start &&
            used[owner[q]] == jobs[q].in_len + 1)
            used[owner[q]] = jobs[q].in_len;
    }
    return LFX_OK;
}
}  // namespace lfx

namespace {

// inflate_member for sizes: mr.status / out_len / end_byte / msg of the DEFLATE stream at byte off0 of d_in[0, n)
int size_member(Ctx *c, const uint8_t *d_in, uint64_t n, uint64_t off0, MemberResult &mr) {
    const uint64_t first_bit = off0 * 8;
    const uint64_t comp = n > off0 ? n - off0 : 0;
    c->pin_reset();        // (the finder's transfer goes through the page-locked slots: nothing of an earlier member is in flight)
    bool done = false;
    int rc;
    std::vector<WalkResult> wr;
    uint64_t total = 0, end_bit = 0;
    if (comp >= 64 && comp < (256u << 10)) {
        // a short stream: one workgroup follows its blocks from the known first one
        if ((rc = run_walk(c, d_in, n, {WalkJob{first_bit, n * 8, 0}}, wr))) return rc;
        c->phase("walk_size");
        if (wr[0].status == WALK_FINAL && walk_settled(wr[0], 0)) { done = true; total = wr[0].n_out; end_bit = wr[0].end_bit; }
    } else if (comp >= 64) {
        // a long stream: the finder's candidates, one walk from each up to the next, the chain on the host
        // (the last block is looked for in the stream's tail only, as in the decode: a walk that meets it earlier follows it anyway)
        FindBufs fb;
        Found fd;
        if ((rc = find_launch(c, d_in, n, off0, find_final_from(n, comp), fb))) return rc;
        c->phase("find1");
        if ((rc = find_collect(c, d_in, n, fb, fd))) return rc;
        c->phase("find2");
        std::vector<uint64_t> starts{first_bit};       // (an overflow: the known first block alone, the rest walked on demand)
        for (uint64_t b : fd.cand) if (b > first_bit) starts.push_back(b);
        std::sort(starts.begin(), starts.end());
        starts.erase(std::unique(starts.begin(), starts.end()), starts.end());
        std::vector<WalkJob> jobs(starts.size());
        for (size_t i = 0; i < starts.size(); i++) jobs[i] = WalkJob{starts[i], n * 8, i + 1 < starts.size() ? starts[i + 1] : 0};
        if ((rc = run_walk(c, d_in, n, jobs, wr))) return rc;
        c->phase("walk_size");
        uint64_t pos = first_bit;
        uint32_t on_demand = 0;
        for (;;) {
            const auto it = std::lower_bound(starts.begin(), starts.end(), pos);
            WalkResult r;
            if (it != starts.end() && *it == pos) r = wr[(size_t)(it - starts.begin())];
            else {
                // a block the finder did not report (stored, fixed, a final block in front of the tail): walked on demand
                if (on_demand++ >= 64) break;
                std::vector<WalkResult> one;
                if ((rc = run_walk(c, d_in, n, {WalkJob{pos, n * 8, it != starts.end() ? *it : 0}}, one))) return rc;
                r = one[0];
            }
            if (!walk_settled(r, total) || r.end_bit <= pos) break;      // the exact path decides, from the stream's start
            total += r.n_out;
            if (r.status == WALK_FINAL) { done = true; end_bit = r.end_bit; break; }
            pos = r.end_bit;
        }
        c->phase("chain");
    }
    if (done) {
        mr.status = LFX_OK;
        mr.out_len = mr.blk_out_start = total;
        mr.end_bit = end_bit;
        mr.end_byte = (end_bit + 7) / 8;
        mr.final_seen = true;
        return LFX_OK;
    }
    // ---- the exact path: the serial kernel, count-only (no stores; its own error codes and message arguments)
    InflateJob j{};
    j.in_off = 0; j.in_len = n; j.start_bit = first_bit;
    j.out_off = 0; j.out_cap = ~0ull; j.hist_avail = 0; j.stop_bit = 0; j.flags = JOB_COUNT_ONLY;
    std::vector<InflateResult> res;
    if ((rc = run_jobs(c, d_in, nullptr, {j}, res))) return rc;
    c->phase("serial");
    const InflateResult &r = res[0];
    mr.status = map_status(r.status);
    mr.out_len = r.out_len;
    mr.blk_out_start = r.status ? r.blk_out_start : r.out_len;
    mr.end_byte = std::min<uint64_t>((r.end_bit + 7) / 8, n);
    if (huff_verdict(r)) {
        std::vector<uint64_t> used;
        if ((rc = huff_consumed(c, d_in, {HuffProbe{0, n, r}}, used))) return rc;
        mr.end_byte = used[0];
    }
    mr.end_bit = r.end_bit;
    mr.final_seen = r.status == 0 && r.final_seen;
    mr.msg = format_error(r.err, r.a0, r.a1);
    return LFX_OK;
}

// decode_stream for sizes: the member loop without output and without the checksum comparison (a trailer must be THERE)
int size_stream(Ctx *c, int format, uint32_t flags, const uint8_t *d_in, uint64_t n, DecodeOutcome &oc, uint64_t base,
                uint64_t out_at, bool one_member, std::vector<lfx_member> *members) {
    return member_loop(c, format, flags, d_in, n, nullptr, 0, true, oc, base, out_at, one_member, members);
}
}  // namespace

extern "C" int lfx_decode_size_device(lfx_ctx *cc, int format, uint32_t flags, const void *d_in, uint64_t n,
                                      uint64_t *out_len, uint64_t *consumed) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    if (format < 0 || format > 2) return LFX_E_ARG;
    (void)hipSetDevice(c->device);
    c->n_ev = 0;
    c->phase("start");
    DecodeOutcome oc;
    int rc = size_stream(c, format, flags, (const uint8_t *)d_in, n, oc);
    if (rc) return rc;
    if (oc.status == LFX_OK) c->phase("done");
    if (out_len) *out_len = oc.out_len;
    if (consumed) *consumed = oc.consumed;
    if (oc.status != LFX_OK) c->set_error(oc.msg);
    return oc.status;
} LFX_ABI_CATCH

extern "C" int lfx_decode_size_host(lfx_ctx *cc, int format, uint32_t flags, const void *in, uint64_t n,
                                    uint64_t *out_len, uint64_t *consumed) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    (void)hipSetDevice(c->device);
    if (int rc = stage_in(c, in, n)) return rc;
    const int rc = lfx_decode_size_device(cc, format, flags, c->d_io_in.p, n, out_len, consumed);
    (void)hipStreamSynchronize(c->stream);   // (a page-locked `in` was only queued for DMA)
    return rc;
} LFX_ABI_CATCH

extern "C" int lfx_decode_batch_size_device(lfx_ctx *cc, int format, uint32_t count, const void *d_in_, const uint64_t *in_off,
                                            const uint64_t *in_len, uint64_t *out_len, uint64_t *consumed, int32_t *status) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    (void)hipSetDevice(c->device);
    c->n_ev = 0;
    c->phase("start");
    if (!count) return LFX_OK;
    if (format < 0 || format > 2) return LFX_E_ARG;
    const uint8_t *d_in = (const uint8_t *)d_in_;
    int rc;
    // ---- container headers (container_kernel)
    std::vector<DecStream> streams(count);
    for (uint32_t i = 0; i < count; i++) streams[i] = DecStream{in_off[i], in_len[i], 0, 0};
    std::vector<DecHeader> hdrs(count, DecHeader{});
    if (format != LFX_DEFLATE && (rc = parse_headers(c, format, d_in, streams, hdrs))) return rc;
    c->phase("headers");
    std::vector<InflateResult> res;
    std::vector<uint64_t> used;
    if ((rc = batch_size_walk(c, format, count, d_in, in_off, in_len, hdrs, res, used))) return rc;
    int worst = LFX_OK;
    for (uint32_t i = 0; i < count; i++) {
        const InflateResult &r = res[i];
        if (out_len) out_len[i] = r.out_len;
        if (consumed) consumed[i] = used[i];
        const int s = map_status(r.status);
        if (status) status[i] = s;
        if (s != LFX_OK && worst == LFX_OK) { worst = s; c->set_error(format_error(r.err, r.a0, r.a1)); }
    }
    c->phase("trailers");
    return LFX_OK;   // per-stream results are in status[]
} LFX_ABI_CATCH

namespace {
// The size half of a batch behind its headers: res[i] = what the decode of stream i would report with room enough — status,
// error, out_len — and used[i] = its bytes consumed, the trailer's presence included (verify_trailers_kernel without the
// checksum comparison).  The walker for every stream of at least 64 bytes whose header stands, the count-only serial kernel
// for the rest, the probes behind a Huffman verdict.  dict (lfx_decode_batch_packed_device): the streams that read it — raw
// DEFLATE always, zlib when its header said so (HDR_DICT) — have its usable bytes as history in front of their first byte.
int batch_size_walk(Ctx *c, int format, uint32_t count, const uint8_t *d_in, const uint64_t *in_off, const uint64_t *in_len,
                    const std::vector<DecHeader> &hdrs, std::vector<InflateResult> &res, std::vector<uint64_t> &used_out,
                    const lfx_dict *dict) {
    int rc;
    auto hist_of = [&](uint32_t i) -> uint64_t { return dict && (format == LFX_DEFLATE || (hdrs[i].flags & HDR_DICT)) ? dict->usable : 0; };
    uint64_t n_in = 0;
    for (uint32_t i = 0; i < count; i++) n_in = std::max(n_in, in_off[i] + in_len[i]);
    // ---- the walker for every stream of at least 64 bytes whose header stands
    res.assign(count, InflateResult{});
    std::vector<uint8_t> settled(count, 0);
    std::vector<WalkJob> wj;
    std::vector<uint32_t> widx;
    for (uint32_t i = 0; i < count; i++) {
        if (hdrs[i].status != 0 || in_len[i] < 64) continue;
        wj.push_back(WalkJob{(in_off[i] + hdrs[i].deflate_off) * 8, (in_off[i] + in_len[i]) * 8, 0});
        widx.push_back(i);
    }
    std::vector<WalkResult> wr;
    if ((rc = run_walk(c, d_in, n_in, wj, wr))) return rc;
    uint64_t walk_blocks = 0;
    for (size_t q = 0; q < wj.size(); q++) {
        walk_blocks += wr[q].nblocks;
        if (wr[q].status != WALK_FINAL || !walk_settled(wr[q], hist_of(widx[q]))) continue;
        InflateResult &o = res[widx[q]];
        o.end_bit = wr[q].end_bit - in_off[widx[q]] * 8;
        o.out_len = o.blk_out_start = wr[q].n_out;
        o.final_seen = 1;
        o.nblocks = wr[q].nblocks;
        settled[widx[q]] = 1;
    }
    c->phase("walk_size");
    // ---- the exact path for the rest
    std::vector<InflateJob> slow;
    std::vector<uint32_t> slow_idx;
    for (uint32_t i = 0; i < count; i++) {
        if (settled[i]) continue;
        InflateJob j{};
        j.in_off = in_off[i];
        j.in_len = hdrs[i].status != 0 ? 0 : in_len[i];     // (header failed: nothing to decode)
        j.start_bit = hdrs[i].deflate_off * 8;
        j.out_cap = ~0ull;
        j.hist_avail = hist_of(i);          // (count-only: the reach of a match is judged, no byte of the history is read)
        j.flags = JOB_COUNT_ONLY;
        slow.push_back(j);
        slow_idx.push_back(i);
    }
    std::vector<InflateResult> sres;
    if ((rc = run_jobs(c, d_in, nullptr, slow, sres))) return rc;
    for (size_t q = 0; q < slow.size(); q++) res[slow_idx[q]] = sres[q];
    std::vector<HuffProbe> probes;
    std::vector<uint32_t> probe_idx;
    for (size_t q = 0; q < slow.size(); q++)
        if (huff_verdict(sres[q])) {
            probes.push_back(HuffProbe{slow[q].in_off, slow[q].in_len, sres[q], slow[q].hist_avail});
            probe_idx.push_back(slow_idx[q]);
        }
    std::vector<uint64_t> probe_used;
    if ((rc = huff_consumed(c, d_in, probes, probe_used))) return rc;
    std::vector<uint64_t> huff_used(count, ~0ull);
    for (size_t q = 0; q < probes.size(); q++) huff_used[probe_idx[q]] = probe_used[q];
    c->phase("serial");
    if (c->diag.debug) fprintf(stderr, "[lfx] batch size: %zu streams walked (%llu blocks), %zu through the exact path\n", wj.size(),
                               (unsigned long long)walk_blocks, slow.size());
    // ---- the trailer's presence and `consumed`
    used_out.assign(count, 0);
    for (uint32_t i = 0; i < count; i++) {
        InflateResult &r = res[i];
        const DecHeader &h = hdrs[i];
        const uint64_t n = in_len[i];
        uint64_t used = h.deflate_off;
        if (h.status != 0) { r.status = h.status; r.err = h.err; r.a0 = h.a0; r.a1 = h.a1; r.out_len = 0; }
        else {
            used = std::min<uint64_t>((r.end_bit + 7) >> 3, n);
            if (huff_used[i] != ~0ull) used = huff_used[i];
            if (r.status == 0 && format != LFX_DEFLATE) {
                const uint64_t need = trailer_len(format);
                if (n - used < need) { r.status = 2; r.err = ERR_EOF; used = n; }
                else used += need;
            }
        }
        used_out[i] = used;
    }
    return LFX_OK;
}
}  // namespace

// ---- the batch decoded back to back: the headers once, the size half, the layout from a device scan of the
// decoded sizes (lfx_batch_unpack.hip), the decode half at those places
extern "C" int lfx_decode_batch_packed_device(lfx_ctx *cc, int format, const lfx_dict *dict, uint32_t count, const void *d_in_,
                                              const uint64_t *in_off, const uint64_t *in_len, const void *d_in_table, uint32_t align,
                                              void *d_out, uint64_t cap, uint64_t *out_off, uint64_t *out_len, uint64_t *consumed,
                                              int32_t *status, uint64_t *total, void *d_table) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    if (format < 0 || format > 2) return LFX_E_ARG;
    if (dict && ((format != LFX_ZLIB && format != LFX_DEFLATE) || dict->c != c)) return LFX_E_ARG;
    if (!bpack_align_ok(align)) { c->set_error("align: a power of two in 1..4096"); return LFX_E_ARG; }
    if (!d_out && cap) { c->set_error("d_out: NULL with a capacity (the size query is d_out = NULL, cap = 0)"); return LFX_E_ARG; }
    if ((((uintptr_t)d_table | (uintptr_t)d_in_table) & 7) != 0) { c->set_error("d_table and d_in_table must be 8-byte aligned"); return LFX_E_ARG; }
    if (count > BPACK_MAX_COUNT) { c->set_error("count: too many streams for one call"); return LFX_E_ARG; }
    if ((in_off == nullptr) != (in_len == nullptr) || (in_off && d_in_table) || (count && !in_off && !d_in_table)) {
        c->set_error("the streams' places: either in_off and in_len (host) or d_in_table (device), not both");
        return LFX_E_ARG;
    }
    (void)hipSetDevice(c->device);
    hipStream_t st = c->stream;
    c->n_ev = 0;
    c->phase("start");
    if (total) *total = 0;
    if (!count) return LFX_OK;
    const uint8_t *d_in = (const uint8_t *)d_in_;
    int rc;
    // ---- the streams' places in the input: the caller's arrays, or the device table copied here
    std::vector<uint64_t> io(count), il(count);
    if (d_in_table) {
        std::vector<uint64_t> tab(2 * (size_t)count);
        HIP_TRY(hipMemcpyAsync(tab.data(), d_in_table, 16ull * count, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (uint32_t i = 0; i < count; i++) { io[i] = tab[2 * (size_t)i]; il[i] = tab[2 * (size_t)i + 1]; }
    } else {
        io.assign(in_off, in_off + count);
        il.assign(in_len, in_len + count);
    }
    // ---- container headers, once for both halves; behind them the decode half's words, then the layout's scratch
    const BunpackScratch w = bunpack_scratch(count);
    std::vector<DecStream> streams(count);
    for (uint32_t i = 0; i < count; i++) streams[i] = DecStream{io[i], il[i], 0, 0};
    std::vector<DecHeader> hdrs;
    DecStream *d_streams;
    DecHeader *d_hdrs;
    if ((rc = parse_headers(c, format, d_in, streams, hdrs, batch_extra_bytes(count) + 8 * w.words, &d_streams, &d_hdrs, dict))) return rc;
    uint64_t *scratch = (uint64_t *)((uint8_t *)(d_hdrs + count) + batch_extra_bytes(count));
    c->phase("headers");
    // ---- the size half
    std::vector<InflateResult> sres;
    std::vector<uint64_t> sused;
    if ((rc = batch_size_walk(c, format, count, d_in, io.data(), il.data(), hdrs, sres, sused, dict))) return rc;
    std::vector<uint64_t> size(count);
    for (uint32_t i = 0; i < count; i++) size[i] = sres[i].out_len;
    uint64_t fits = 0;
    if (!bpack_bound_sum(size.data(), count, align, &fits)) { c->set_error("the streams' decoded sizes exceed 64 bits"); return LFX_E_ARG; }
    c->phase("sizes");
    // ---- the layout: sizes up, three kernels, the pairs and the total back in one transfer
    HIP_TRY(hipMemcpyAsync(scratch + w.size, size.data(), 8ull * count, hipMemcpyHostToDevice, st));
    LAUNCH_TRY(launch_batch_unpack_layout(st, d_streams, count, align, scratch, (uint64_t *)d_table));
    std::vector<uint64_t> back(bunpack_back_words(count));
    HIP_TRY(hipMemcpyAsync(back.data(), scratch + w.pairs, 8ull * back.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    c->phase("layout");
    std::vector<uint64_t> off(count);
    for (uint32_t i = 0; i < count; i++) off[i] = back[2 * (size_t)i];
    const uint64_t need = back[2 * (size_t)count];
    if (out_off) std::copy(off.begin(), off.end(), out_off);
    if (total) *total = need;
    if (need > cap || !d_out) {
        // nothing is decoded: the size half's verdicts (d_out == NULL with nothing to write is the size query's answer too)
        int worst = LFX_OK;
        for (uint32_t i = 0; i < count; i++) {
            if (out_len) out_len[i] = size[i];
            if (consumed) consumed[i] = sused[i];
            const int s = map_status(sres[i].status);
            if (status) status[i] = s;
            if (s != LFX_OK && worst == LFX_OK) { worst = s; c->set_error(format_error(sres[i].err, sres[i].a0, sres[i].a1)); }
        }
        if (need <= cap) return LFX_OK;
        c->set_error("output capacity too small (*total says what the streams need): no stream was decoded");
        return LFX_E_NOSPACE;
    }
    // ---- the decode half at those places, out_cap = the size
    std::vector<InflateResult> res;
    if ((rc = decode_batch_placed(c, format, count, d_in, io.data(), il.data(), d_out, off.data(), size.data(), hdrs, d_streams, d_hdrs, res,
                                  nullptr, dict)))
        return rc;
    int worst = LFX_OK;
    for (uint32_t i = 0; i < count; i++) {
        if (out_len) out_len[i] = res[i].out_len;
        if (consumed) consumed[i] = sused[i];
        const int s = map_status(res[i].status);
        if (status) status[i] = s;
        if (s != LFX_OK && worst == LFX_OK) { worst = s; c->set_error(format_error(res[i].err, res[i].a0, res[i].a1)); }
    }
    return LFX_OK;  // per-stream results are in status[]
} LFX_ABI_CATCH

extern "C" int lfx_decode_members_size_device(lfx_ctx *cc, const void *d_in, uint64_t n, uint64_t *out_len, uint64_t *consumed,
                                              lfx_member *members, uint32_t max_members, uint32_t *n_members) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    (void)hipSetDevice(c->device);
    c->n_ev = 0;
    c->phase("start");
    DecodeOutcome oc;
    std::vector<lfx_member> got;
    int rc = members_chain(c, (const uint8_t *)d_in, n, nullptr, 0, true, oc, got);
    if (rc) return rc;
    return members_out(c, oc, got, out_len, consumed, members, max_members, n_members);
} LFX_ABI_CATCH

extern "C" int lfx_decode_members_size_host(lfx_ctx *cc, const void *in, uint64_t n, uint64_t *out_len, uint64_t *consumed,
                                            lfx_member *members, uint32_t max_members, uint32_t *n_members) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    (void)hipSetDevice(c->device);
    if (int rc = stage_in(c, in, n)) return rc;
    const int rc = lfx_decode_members_size_device(cc, c->d_io_in.p, n, out_len, consumed, members, max_members, n_members);
    (void)hipStreamSynchronize(c->stream);
    return rc;
} LFX_ABI_CATCH

// ------------------------------------------------------------------------------------------------
// seek index: the decode of lfx_decode_device (LFX_DEC_MULTI: of lfx_decode_members_device), unchanged, with
// Ctx::idx set — its chains record their block starts and the lanes of their large blocks — then the index from those
// candidates (lfx_index.hip)
namespace {
struct IdxScope {      // Ctx::idx for the length of the decode, whatever way it is left
    Ctx *c;
    IdxScope(Ctx *c_, IdxCollect *col) : c(c_) { c->idx = col; }
    ~IdxScope() { c->idx = nullptr; }
};
}  // namespace

extern "C" int lfx_decode_index_device(lfx_ctx *cc, int format, uint32_t flags, const void *d_in, uint64_t n, void *d_out,
                                       uint64_t cap, uint64_t *out_len, uint64_t *consumed, uint64_t spacing, lfx_index **idx) try {
    if (!cc) return LFX_E_DEVICE;
    Ctx *c = reinterpret_cast<Ctx *>(cc);
    if (idx) *idx = nullptr;
    if (format < 0 || format > 2 || spacing < 4096 || !idx) return LFX_E_ARG;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    (void)hipSetDevice(c->device);
    c->n_ev = 0;
    c->phase("start");
    const bool multi = format == LFX_GZIP && (flags & LFX_DEC_MULTI);
    IdxCollect col;
    col.spacing = spacing;
    DecodeOutcome oc;
    std::vector<lfx_member> members;
    int rc;
    {
        IdxScope scope(c, &col);
        PhaseMute mute(c);
        if (multi) rc = members_chain(c, (const uint8_t *)d_in, n, (uint8_t *)d_out, cap, false, oc, members);
        else rc = decode_stream(c, format, flags, (const uint8_t *)d_in, n, (uint8_t *)d_out, cap, oc, 0, 0, false, &members);
    }
    if (rc) return rc;
    c->phase("decode");
    if (oc.out_len > cap) oc.out_len = cap;  // (as lfx_decode_device)
    if (out_len) *out_len = oc.out_len;
    if (consumed) *consumed = oc.consumed;
    if (oc.status != LFX_OK) { c->set_error(oc.msg); return oc.status; }
    if ((rc = idx_finish(c, col, format, multi ? LFX_DEC_MULTI : 0u, (const uint8_t *)d_in, oc.consumed, (const uint8_t *)d_out,
                         oc.out_len, members, idx)))
        return rc;
    c->phase("done");
    return LFX_OK;
} LFX_ABI_CATCH
