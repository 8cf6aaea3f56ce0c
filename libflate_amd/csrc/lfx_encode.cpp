// lfx_encode.cpp — the encode core behind every encode entry point of lfx_api.cpp: encode_prepare as a sequence of stages,
// encode_emit, and the steps the entry points share.  Every byte of compression work runs on the GPU.
#include "lfx_encode_int.h"

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "lfx_chain.h"
#include "lfx_cost.h"
#include "lfx_dict_enc.h"
#include "lfx_encode_stages.h"

namespace lfx {

// ------------------------------------------------------------------------------------------------
// the side-stream zero fill of an output buffer
bool Ctx::Prezero::start(void *d_out, uint64_t n) {
    ptr = nullptr;
    if (!n) return false;
    if (hipEventRecord(c->ev_fork, c->stream) != hipSuccess || hipStreamWaitEvent(c->side_stream, c->ev_fork, 0) != hipSuccess ||
        hipMemsetAsync(d_out, 0, n, c->side_stream) != hipSuccess || hipEventRecord(c->ev_zero, c->side_stream) != hipSuccess)
        return false;
    ptr = d_out;
    bytes = n;
    return true;
}
hipError_t Ctx::Prezero::join(hipStream_t st, void *d_out, uint64_t n) {
    hipError_t e = hipSuccess;
    if (ptr && ptr == d_out && bytes == n) e = hipStreamWaitEvent(st, c->ev_zero, 0);
    else if (n) e = hipMemsetAsync(d_out, 0, n, st);
    if (e == hipSuccess) ptr = nullptr;      // (a failure leaves the fill to settle())
    return e;
}
void Ctx::Prezero::settle() {
    if (ptr) (void)hipEventSynchronize(c->ev_zero);
    ptr = nullptr;
}

namespace {

// typed views of the context's buffers for one encode_prepare call (valid behind reserve_scratch)
struct EncView {
    const ChunkDesc *chunks;
    const BlockDesc *blocks;
    const SegDesc *segs;
    const ParseWg *pwgs;
    uint16_t *cd;
    uint32_t *codes, *ncodes, *stage, *segtmp, *hist, *ck;
    uint64_t *vis;
    EncodeResult *res;
    uint32_t *tile_map, *seg_map, *d_match_flags;
    uint64_t *mdbg;               // LFX_DEBUG: per-wavefront cycle counters of workgroup 0
};
// one encode_prepare call: its arguments, its geometry and what the stages hand on
struct EncCall {
    const Plan &plan;
    const PlanOpts &po;
    const uint8_t *d_in;
    uint64_t n;
    int ck_mode;
    const HostCodes *hc;
    const lfx_dict *dict;         // a preset dictionary with a usable tail, or nullptr
    bool match_v1;                // the first-generation match kernel: it once saw a lane-order violation (or LFX_MATCH_V1 is set)
    uint32_t chain_depth;         // ChainLz77Encoder's or LazyLz77Encoder's depth; 0: any other kind — no chain stage, no second candidate buffer
    bool lazy;                    // LazyLz77Encoder: the chain stage keeps the lengths and demotes behind them (§20)
    bool tuned;                   // LFX_LZ77_LEVEL (§23): the chain stage's tuned instances, with ...
    LevelTune tune;               // ... the level's nice, max_lazy and too_far (chain_depth and lazy above are the level's too)
    bool cost;                    // LFX_LZ77_COST (§27): the level's candidates, no lazy demotion; a first pass for the block's code, the cost kernel, the parse again
    bool auto_blocks;             // LFX_HUFFMAN_AUTO (§22): block_choose_kernel behind the Huffman kernel; any other call: no launch, no buffer
    bool merge_blocks;            // block_merge (§24): block_merge_kernel and a second Huffman pass behind the first; any other call: no launch, no buffer
    EncodeGeom g;
    bool pack_by_chunk = false;   // the geometry's flag, and nothing behind the Huffman stage rewrites the blocks' codes (LFX_HUFFMAN_AUTO), joins blocks (block_merge) or reads tile starts (the encode index)
    uint64_t nspans = 0;          // partial results of the checksum kernels
    bool forked = false;          // the first half of the checksum's sweep is on the side stream already
    EncView v{};
};

// ---- LFX_DEBUG dumps (each behind a synchronous copy, where the stage that calls it stands in the stream)
void dbg_match(const EncCall &k) {
    uint64_t hv[256];
    (void)hipMemcpy(hv, k.v.mdbg, sizeof hv, hipMemcpyDeviceToHost);
    if (!k.match_v1) {
        // lfx_match7: wave 0 = exchange on head, wave 1 = exchange on second, waves 2..15 = helpers
        for (int w = 0; w < 16; w++)
            fprintf(stderr, "[lfx] match7 wave%d: work=%llu barrier-wait=%llu tiles=%llu\n", w, (unsigned long long)hv[w * 8],
                    (unsigned long long)hv[w * 8 + 1], (unsigned long long)hv[w * 8 + 5]);
    } else {
        for (int w = 0; w < 16; w++)
            fprintf(stderr, "[lfx] match1 wave%d: load=%llu work=%llu wait=%llu tiles=%llu\n", w, (unsigned long long)hv[w * 8],
                    (unsigned long long)hv[w * 8 + 1], (unsigned long long)hv[w * 8 + 2], (unsigned long long)hv[w * 8 + 5]);
    }
}
// the parse's two launchers over a call's views: the persistent walk, and the chaining kernels behind it (counted: with the
// blocks' symbol counts where the geometry fuses them)
int parse_walk(Ctx *c, const EncCall &k, const uint32_t *mflags, uint64_t *dbg) {
    const EncView &v = k.v;
    LAUNCH_TRY(launch_parse_walk(c->stream, k.d_in, k.n, v.chunks, k.plan.n_segs, v.pwgs, (uint32_t)k.g.pwgs.size(),
                                 (uint32_t)(c->n_cu > 0 ? c->n_cu : 256), v.cd, k.po.max_length, v.vis, v.segtmp, v.stage, mflags, dbg,
                                 k.dict ? k.dict->d_win : nullptr, k.dict ? k.dict->usable : 0u));
    return LFX_OK;
}
int parse_chain(Ctx *c, const EncCall &k, bool counted, bool fixseg_only = false) {
    const EncView &v = k.v;
    LAUNCH_TRY(launch_parse_chain(c->stream, k.d_in, k.n, v.chunks, c->cur_nchunks, k.plan.n_segs, v.cd, k.po.max_length, v.vis, v.segtmp,
                                  v.codes, v.ncodes, v.stage, v.seg_map, counted && k.g.fused_hist ? v.hist : nullptr, k.g.emit_per,
                                  k.g.emit_parts, k.dict ? k.dict->d_win : nullptr, fixseg_only, k.pack_by_chunk));
    return LFX_OK;
}
// LFX_DUMP_SEG: the parse state of one segment behind the walk, behind fixseg and at the end
int dbg_dump_seg(Ctx *c, const EncCall &k) {
    const EncView &v = k.v;
    hipStream_t st = c->stream;
    const uint32_t sg = (uint32_t)c->diag.dump_seg;
    for (int stage_no = 1; stage_no <= 3 && sg < k.plan.n_segs; stage_no++) {
        if (int rc = parse_walk(c, k, nullptr, nullptr)) return rc;
        if (stage_no != 1)
            if (int rc = parse_chain(c, k, false, stage_no == 2)) return rc;
        (void)hipStreamSynchronize(st);
        uint64_t vw[4];
        uint32_t t[6];
        uint16_t cdv[64];
        (void)hipMemcpy(vw, v.vis + (uint64_t)sg * 64, sizeof vw, hipMemcpyDeviceToHost);
        for (int q = 0; q < 6; q++) (void)hipMemcpy(&t[q], v.segtmp + (size_t)q * k.plan.n_segs + sg, 4, hipMemcpyDeviceToHost);
        (void)hipMemcpy(cdv, v.cd + (uint64_t)sg * PARSE_SEG, sizeof cdv, hipMemcpyDeviceToHost);
        fprintf(stderr, "[lfx] seg %u stage %d: vis %016llx %016llx %016llx %016llx exit=%u count=%u off=%u exit2=%u mpos=%u kspec=%u\n", sg,
                stage_no, (unsigned long long)vw[0], (unsigned long long)vw[1], (unsigned long long)vw[2], (unsigned long long)vw[3], t[0],
                t[1], t[2], t[3], t[4], t[5]);
        if (stage_no == 1) { fprintf(stderr, "[lfx]  cd:"); for (int q = 0; q < 64; q++) fprintf(stderr, " %u", cdv[q]); fprintf(stderr, "\n"); }
    }
    return LFX_OK;
}
void dbg_walk(const EncCall &k) {
    uint64_t hv[32];
    (void)hipMemcpy(hv, k.v.mdbg + 256, sizeof hv, hipMemcpyDeviceToHost);
    for (int w = 0; w < 4; w++)
        fprintf(stderr, "[lfx] walk wave%d: fill=%llu spec=%llu resolve+chain=%llu emit=%llu cycles\n", w, (unsigned long long)hv[w * 8],
                (unsigned long long)hv[w * 8 + 1], (unsigned long long)hv[w * 8 + 2], (unsigned long long)hv[w * 8 + 3]);
}
void dbg_huffman(const EncCall &k) {
    uint64_t hv[24];
    (void)hipMemcpy(hv, k.v.mdbg + 512, sizeof hv, hipMemcpyDeviceToHost);
    static const char *nm[10] = {"lit: rank sort", "lit: depth", "lit: package-merge", "lit: widths", "lit: codes", "dist tree", "run lengths",
                                 "code-length tree", "header bits", "body size"};
    fprintf(stderr, "[lfx] huffman block 0 (cycles):");
    for (int q = 0; q < 10; q++) fprintf(stderr, " %s=%llu", nm[q], (unsigned long long)(hv[q + 1] - hv[q]));
    fprintf(stderr, "\n");
}

// ---- the stages of encode_prepare
int reserve_scratch(Ctx *c, EncCall &k) {
    const Plan &plan = k.plan;
    const bool hc = k.hc != nullptr, match_v1 = k.match_v1;
    const uint32_t nchunks = c->cur_nchunks, nblocks = c->cur_nblocks;
    const uint64_t n = k.n, lnk_units = k.g.lnk_units;
    const size_t nsegs = k.g.segs.size();
    int rc;
    if ((rc = c->d_chunks.reserve(sizeof(ChunkDesc) * std::max<size_t>(nchunks, 1)))) return rc;
    if ((rc = c->d_blocks.reserve(sizeof(BlockDesc) * std::max<size_t>(nblocks, 1)))) return rc;
    if ((rc = c->d_segs.reserve(sizeof(SegDesc) * std::max<size_t>(nsegs, 1)))) return rc;
    if ((rc = c->d_pwgs.reserve(sizeof(ParseWg) * std::max<size_t>(k.g.pwgs.size(), 1)))) return rc;
    if (!hc && (rc = c->d_cd.reserve(2 * n + 64))) return rc;                   // candidate distances, 16 bits per position
    if (!hc && k.chain_depth && (rc = c->d_cd2.reserve(2 * n + 64))) return rc;  // ... and the chain stage's, which the parse then reads
    if (!hc && k.chain_depth && (k.lazy || k.tuned) && (rc = c->d_len.reserve(n + 64))) return rc;   // ... and LazyLz77Encoder's length byte per position (the tuned instances write it at every level)
    if (!hc && !match_v1 && (rc = c->d_glnk.reserve(264 * std::max<uint64_t>(lnk_units, 1)))) return rc;   // lfx_match7: link records (4 bytes) + ballot words (8 bytes per 64)
    if (!hc && !match_v1 && (rc = c->d_ucount.reserve(4 * std::max<size_t>(nsegs, 1)))) return rc;   // lfx_match7: unresolved positions per segment
    if (!hc && match_v1 && (rc = c->d_md.reserve(4 * std::max<uint64_t>(n, 1)))) return rc;   // first-generation kernel: (length, distance) words
    if ((rc = c->d_codes.reserve(4 * std::max<uint64_t>(plan.n_codes_cap, 1)))) return rc;
    if ((rc = c->d_ncodes.reserve(4 * std::max<size_t>(nchunks, 1)))) return rc;
    if ((rc = c->d_vis.reserve(8 * std::max<uint64_t>(plan.n_vis, 1)))) return rc;
    if ((rc = c->d_segtmp.reserve(24ull * std::max<uint32_t>(plan.n_segs, 1)))) return rc;
    if (!hc && (rc = c->d_stage.reserve(4ull * (n + 64)))) return rc;   // code words staged by the speculative parse walk
    if ((rc = c->d_chunkmap.reserve(4ull * (plan.n_tiles + plan.n_segs + 2)))) return rc;   // tile → chunk, segment → chunk
    if ((rc = c->d_hist.reserve(4ull * 320 * std::max<size_t>(nblocks, 1)))) return rc;
    if (k.pack_by_chunk && (rc = c->d_hist_chunk.reserve(4ull * SYM_ROW * nchunks))) return rc;   // pack by chunk: the symbol counts per chunk ...
    if (k.pack_by_chunk && (rc = c->d_chunk_bits.reserve(16ull * nchunks))) return rc;            // ... every chunk's packed size and first bit
    if ((rc = c->d_bc.reserve(sizeof(BlockCodes) * std::max<size_t>(nblocks, 1)))) return rc;
    if ((rc = c->d_block_start.reserve(8 * std::max<size_t>(nblocks, 1)))) return rc;
    if (k.auto_blocks && (rc = c->d_choice.reserve(std::max<size_t>(nblocks, 1)))) return rc;   // LFX_HUFFMAN_AUTO: the chosen type per block
    if (k.merge_blocks) {                                                                      // block_merge: the regions, and every block's head
        merge_regions(plan.blocks, c->merge_regions);
        if ((rc = c->d_merge_regions.reserve(sizeof(MergeRegion) * std::max<size_t>(c->merge_regions.size(), 1)))) return rc;
        if ((rc = c->d_merge.reserve(4 * std::max<size_t>(nblocks, 1)))) return rc;
    }
    if ((rc = c->d_tile_bits.reserve(4 * std::max<uint64_t>(plan.n_tiles, 1)))) return rc;
    if ((rc = c->d_tile_start.reserve(8 * std::max<uint64_t>(plan.n_tiles, 1)))) return rc;
    k.nspans = ck_nspans(n);
    if ((rc = c->d_ck.reserve(12 * k.nspans))) return rc;
    if ((rc = c->d_res.reserve(256))) return rc;
    if ((rc = c->d_small.reserve(70000))) return rc;
    EncView &v = k.v;
    v.chunks = (const ChunkDesc *)c->d_chunks.p; v.blocks = (const BlockDesc *)c->d_blocks.p;
    v.segs = (const SegDesc *)c->d_segs.p; v.pwgs = (const ParseWg *)c->d_pwgs.p;
    v.cd = (uint16_t *)c->d_cd.p; v.codes = (uint32_t *)c->d_codes.p; v.ncodes = (uint32_t *)c->d_ncodes.p;
    v.stage = (uint32_t *)c->d_stage.p; v.segtmp = (uint32_t *)c->d_segtmp.p;
    v.hist = (uint32_t *)(k.pack_by_chunk ? c->d_hist_chunk.p : c->d_hist.p);
    v.ck = (uint32_t *)c->d_ck.p; v.vis = (uint64_t *)c->d_vis.p; v.res = (EncodeResult *)c->d_res.p;
    v.tile_map = (uint32_t *)c->d_chunkmap.p; v.seg_map = v.tile_map + plan.n_tiles;
    v.d_match_flags = (uint32_t *)((uint8_t *)c->d_res.p + offsetof(EncodeResult, match_flags));
    v.mdbg = c->diag.debug ? (uint64_t *)((uint8_t *)c->d_small.p + 32768) : nullptr;
    return LFX_OK;
}

// A plan table: uploaded from a shadow kept on the context (it outlives the asynchronous copy: no synchronisation), and not
// at all when the same table already sits in the same device buffer (an encode loop over equal-sized inputs)
hipError_t upload_table(Ctx *c, int slot, DevBuf &b, const void *src, size_t bytes) {
    std::vector<uint8_t> &sh = c->up_shadow[slot];
    const uint64_t tag = (uint64_t)(uintptr_t)b.p ^ ((uint64_t)b.gen << 48) ^ (1ull << 63);
    if (c->up_dev[slot] == tag && sh.size() == bytes && (bytes == 0 || memcmp(sh.data(), src, bytes) == 0)) return hipSuccess;
    sh.assign((const uint8_t *)src, (const uint8_t *)src + bytes);
    c->up_dev[slot] = tag;
    return bytes ? hipMemcpyAsync(b.p, sh.data(), bytes, hipMemcpyHostToDevice, c->stream) : hipSuccess;
}
int upload_tables(Ctx *c, const EncCall &k) {
    HIP_TRY(upload_table(c, 0, c->d_chunks, k.plan.chunks.data(), sizeof(ChunkDesc) * k.plan.chunks.size()));
    HIP_TRY(upload_table(c, 1, c->d_blocks, k.plan.blocks.data(), sizeof(BlockDesc) * k.plan.blocks.size()));
    HIP_TRY(upload_table(c, 2, c->d_segs, k.g.segs.data(), sizeof(SegDesc) * k.g.segs.size()));
    HIP_TRY(upload_table(c, 3, c->d_pwgs, k.g.pwgs.data(), sizeof(ParseWg) * k.g.pwgs.size()));
    c->phase("upload");
    return LFX_OK;
}

// tile → chunk and segment → chunk.  The call's first kernel also clears the blocks' symbol counters, the result record and the
// match stage's per-segment counts (three fill operations in front of the match kernel before: 22 us of a 4.6 ms step)
int chunk_maps(Ctx *c, const EncCall &k) {
    const bool ucount_here = !k.hc && !k.match_v1;
    const ZeroSpan z_hist{k.v.hist, (uint32_t)(320 * (k.pack_by_chunk ? (size_t)c->cur_nchunks : std::max<size_t>(c->cur_nblocks, 1)))}, z_res{(uint32_t *)c->d_res.p, 64u},
        z_ucount{ucount_here ? (uint32_t *)c->d_ucount.p : nullptr, ucount_here ? (uint32_t)std::max<size_t>(k.g.segs.size(), 1) : 0u};
    c->cur_tile_map = k.v.tile_map;
    if (int e_ = launch_chunk_maps(c->stream, k.v.chunks, c->cur_nchunks, k.plan.n_tiles, k.plan.n_segs, k.v.tile_map, k.v.seg_map, z_hist,
                                   z_res, z_ucount)) {
        c->set_error(hipGetErrorString((hipError_t)e_));
        return LFX_E_DEVICE;
    }
    return LFX_OK;
}

// the caller's own Lz77Encode produced the code words (EncodeOptions::with_lz77(E), encode.rs:59-65): they take the place of
// the match + parse stages' output — one chunk per block, EndOfBlock included; everything from the histogram on
// (CompressBuf::flush, encode.rs:416-425) runs as for the built-in encoders
int upload_codes(Ctx *c, const EncCall &k) {
    hipStream_t st = c->stream;
    if (k.hc->n_codes) HIP_TRY(hipMemcpyAsync(c->d_codes.p, k.hc->codes, 4ull * k.hc->n_codes, hipMemcpyHostToDevice, st));
    if (c->cur_nchunks) HIP_TRY(hipMemcpyAsync(c->d_ncodes.p, k.hc->chunk_codes, 4ull * c->cur_nchunks, hipMemcpyHostToDevice, st));
    c->phase("codes_upload");
    return LFX_OK;
}

// lfx_match7: the candidate kernel, then the positions it leaves open (0.5 % of a text): ballot words → lists → walks.
// Both on the main stream, one launch each.  (Measured, round 5: the segments in four parts, the resolver of a part on the
// side stream beside the next part's kernel, 1.10 ms against 1.15 in one piece at 256 MiB: a part of 256 workgroups ends
// with its slowest segment, and the compaction waits for slots behind the kernel.  The resolver with four walks in flight
// per lane made the overlap pointless.)
int match7(Ctx *c, const EncCall &k) {
    const EncView &v = k.v;
    hipStream_t st = c->stream;
    const uint32_t ns = (uint32_t)k.g.segs.size();
    uint32_t *d_glnk = (uint32_t *)c->d_glnk.p;
    uint64_t *d_umask = (uint64_t *)((uint8_t *)c->d_glnk.p + 256 * std::max<uint64_t>(k.g.lnk_units, 1));
    uint32_t *d_ucount = (uint32_t *)c->d_ucount.p;     // (cleared by the call's first kernel, launch_chunk_maps)
    LAUNCH_TRY(launch_match7(st, k.d_in, k.n, v.chunks, v.segs, ns, k.po.window_size, v.cd, d_glnk, d_umask, v.d_match_flags, v.mdbg));
    if (c->timing_fine()) c->phase("lz77_cand");
    LAUNCH_TRY(launch_resolve7(st, v.chunks, v.segs, ns, k.po.window_size, v.cd, d_glnk, d_umask, v.stage, d_ucount));
    return LFX_OK;
}

// candidate distances for every position: lfx_match7 unless the context fell back to (or LFX_MATCH_V1 asks for) the
// first-generation kernel
int stage_match(Ctx *c, const EncCall &k) {
    const EncView &v = k.v;
    hipStream_t st = c->stream;
    const uint32_t ns = (uint32_t)k.g.segs.size();
    if (k.match_v1) {
        LAUNCH_TRY(launch_match(st, k.d_in, k.n, v.chunks, v.segs, ns, k.po.window_size, k.po.max_length, (uint32_t *)c->d_md.p, v.mdbg));
        LAUNCH_TRY(launch_md_to_cd(st, (const uint32_t *)c->d_md.p, k.n, v.cd));
    } else {
        if (int rc = match7(c, k)) return rc;
    }
    if (v.mdbg) dbg_match(k);
    c->phase(c->timing_fine() ? "lz77_resolve" : "lz77_match");
    return LFX_OK;
}

// A call with a preset dictionary, behind the match stage whichever generation ran: the candidates it left
// open among the first min(end, window_size) positions of every primed chunk are filled from the dictionary — its prefix table
// is built here the first time the dictionary is used for an encode, and kept.  One launch for all primed chunks of the call.
int stage_dict(Ctx *c, const EncCall &k) {
    const lfx_dict *d = k.dict;
    hipStream_t st = c->stream;
    dict_items(k.plan.chunks, k.po.window_size, c->dict_items);
    if (c->dict_items.empty()) return LFX_OK;
    if (!d->d_tab) {
        if (hipMalloc((void **)&d->d_tab, DICT_TAB_BYTES) != hipSuccess) { d->d_tab = nullptr; c->set_error("out of device memory"); return LFX_E_OOM; }
        d->tab_built = false;
    }
    if (!d->tab_built) {
        LAUNCH_TRY(launch_dict_table(st, d->d_win, d->usable, d->d_tab));
        d->tab_built = true;
    }
    const size_t bytes = sizeof(DictItem) * c->dict_items.size();
    if (int rc = c->d_dict_items.reserve(bytes)) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_dict_items.p, c->dict_items.data(), bytes, hipMemcpyHostToDevice, st));
    LAUNCH_TRY(launch_dict_cand(st, k.d_in, k.v.chunks, (const DictItem *)c->d_dict_items.p, (uint32_t)c->dict_items.size(),
                                k.po.window_size, d->d_end(), d->usable, d->d_tab, k.v.cd));
    c->phase("lz77_dict");
    return LFX_OK;
}

// ChainLz77Encoder, behind the match stage whichever generation ran: the longest of the first chain_depth
// candidates on every position's chain through cd → cd2, which the parse reads from here on.  One launch for all chunks.
// LazyLz77Encoder (§20): the same launch also keeps the lengths, and a second one over the same work list takes the candidate
// from every position whose successor's is longer.
//
// A chain dictionary (§21): stage_dict has run in front and left, in cd, every primed position's first dictionary candidate.
// The tiles of the primed chunks within window_size of their start form a second run of the work list and go to the
// dictionary instance, which follows the chain on into the dictionary's tail — through the tail's own chain, built here the
// first time the dictionary serves a chained encode, and kept.
//
// LFX_LZ77_LEVEL (§23): the same two launches over the same work list, through the tuned instances — the walk stops at a nice
// match and drops a far 3-byte one, the demotion spares a length of max_lazy or more.  The greedy levels (1..3) run the
// length-writing instance too, leave the lengths unread and launch no demotion.
int stage_chain(Ctx *c, EncCall &k) {
    hipStream_t st = c->stream;
    const lfx_dict *d = k.dict;
    const bool small = chain_small(k.plan.chunks);
    uint32_t n_plain = 0;
    chain_items_dict(k.plan.chunks, small ? CHAIN_TILE_SMALL : CHAIN_TILE, k.po.window_size, d != nullptr, c->chain_items, n_plain);
    uint16_t *cd2 = (uint16_t *)c->d_cd2.p;
    ChainDict cdict{nullptr, nullptr, nullptr, 0u};
    const ChainTune ctune{k.tune.nice, k.tune.too_far};
    if (n_plain < c->chain_items.size()) {
        if (!d->d_cdt) {
            if (hipMalloc((void **)&d->d_cdt, DICT_CHAIN_BYTES) != hipSuccess) { d->d_cdt = nullptr; c->set_error("out of device memory"); return LFX_E_OOM; }
            d->cdt_built = false;
        }
        if (!d->cdt_built) {
            LAUNCH_TRY(launch_dict_chain(st, d->d_win, d->usable, d->d_cdt));
            d->cdt_built = true;
        }
        cdict = ChainDict{d->d_win, d->d_cdt, (const unsigned long long *)d->d_tab, d->usable};   // (d_tab: stage_dict's, the chunks are the same)
    }
    if (!c->chain_items.empty()) {
        const size_t bytes = sizeof(ChainItem) * c->chain_items.size();
        if (int rc = c->d_chain_items.reserve(bytes)) return rc;
        HIP_TRY(hipMemcpyAsync(c->d_chain_items.p, c->chain_items.data(), bytes, hipMemcpyHostToDevice, st));
        LAUNCH_TRY(launch_chain(st, k.d_in, k.n, k.v.chunks, (const ChainItem *)c->d_chain_items.p, (uint32_t)c->chain_items.size(), small,
                                k.po.window_size, k.po.max_length, k.chain_depth, k.v.cd, cd2,
                                k.lazy || k.tuned ? (uint8_t *)c->d_len.p : nullptr, n_plain, cdict.win ? &cdict : nullptr,
                                k.tuned ? &ctune : nullptr));
    }
    k.v.cd = cd2;
    c->phase("lz77_chain_cand");
    if (k.lazy) {
        if (!c->chain_items.empty())
            LAUNCH_TRY(launch_demote(st, k.v.chunks, (const ChainItem *)c->d_chain_items.p, (uint32_t)c->chain_items.size(), small,
                                     (const uint8_t *)c->d_len.p, cd2, k.tuned ? k.tune.max_lazy : 0u));
        c->phase("lz77_lazy_demote");
    }
    return LFX_OK;
}

// the greedy walk → code words per chunk (and, fused_hist, the blocks' symbol counts); with a checksum the first half of its
// sweep goes to the side stream from behind the walk kernel on
int stage_parse(Ctx *c, EncCall &k) {
    const EncView &v = k.v;
    hipStream_t st = c->stream;
    const bool want_checksum = k.ck_mode != 0;
    if (c->diag.debug && c->diag.dump_seg >= 0)
        if (int rc = dbg_dump_seg(c, k)) return rc;
    if (int rc = parse_walk(c, k, v.d_match_flags, v.mdbg ? v.mdbg + 256 : nullptr)) return rc;
    // The side stream's fork point: behind the walk kernel, in front of the chaining kernels.  Recorded HERE, whatever the walk
    // launched — a plan without chunks (stored blocks) launches nothing, and the side stream must still wait for what the main
    // stream holds in front: a caller's H2D copy of the input (the stream encoder's batch).
    if (want_checksum) HIP_TRY(hipEventRecord(c->ev_fork, st));
    if (c->timing_fine()) c->phase("lz77_walk");     // (fine timing: the walk kernel in a bracket of its own)
    if (int rc = parse_chain(c, k, true)) return rc;
    if (want_checksum) {
        // the first half of the container checksum's sweep: on the side stream from behind the walk kernel on, beside the
        // chaining kernels (one wavefront per segment and a handful of steps each: they leave most of the GPU idle); the
        // second half beside the Huffman kernel (checksum_fork).  (Measured, round 6: all of it here ran into parse_emit — both
        // want the memory system — parse + Huffman 1.13 ms; all of it behind the parse no longer fits under the Huffman
        // kernel now that the histogram kernel is gone.)
        HIP_TRY(hipStreamWaitEvent(c->side_stream, c->ev_fork, 0));
        LAUNCH_TRY(launch_checksum_part(c->side_stream, k.d_in, k.n, v.ck, v.ck + k.nspans, v.ck + 2 * k.nspans, v.res, k.ck_mode, 0, 2));
        k.forked = true;
    }
    if (v.mdbg) dbg_walk(k);
    c->phase(c->timing_fine() ? "lz77_chain" : "lz77_parse");
    return LFX_OK;
}

// CostLz77Encoder, behind the chain stage — cd2 and d_len hold the level's candidates, nothing demoted — and in
// front of the call's parse:
//   [ parse → plain Huffman ]  the first pass: the greedy walk over the undemoted candidates, the blocks' symbol counts and
//                              their plain dynamic codes (no block_merge, no LFX_HUFFMAN_AUTO: d_bc is all the cost kernel
//                              reads of it).  Skipped under fixed codes, whose widths the kernel knows.
//   cost_demote                cd ← cd2 without the candidates that lose by cost (out of place, lfx_cost.hip): the array the
//                              match stage wrote, free since the chain stage read it.  The call's parse reads it.
// Between the passes, everything the parse and the histogram accumulate:
//   d_hist / d_hist_chunk      counted by atomic adds: cleared HERE, the one buffer that needs it;
//   d_ucount                   the match stage's open positions per segment: no parse touches it;
//   d_ncodes, d_segtmp         the code counts and the six per-segment words: every walk and every fold stores all of them
//                              anew (the debug dump of a segment has always walked twice);
//   d_vis                      the visited masks: the walk stores every word of every segment, zero where nothing is visited;
//   d_stage, d_codes           stored, never combined; a shorter second list leaves stale words behind its end, unread;
//   the result record          its parse-side field is match_flags, the MATCH stage's verdict, which the second walk must
//                              still see; end_bit, status and the checksums are written behind the prepare stage.
// The checksum forks once, in the call's parse; with_match_fallback re-runs the prepare stage and with it all of this.
int stage_cost(Ctx *c, EncCall &k) {
    const EncView &v = k.v;
    hipStream_t st = c->stream;
    const bool fixed = !k.po.dynamic_huffman;
    cost_items(k.plan.chunks, c->cost_items);
    if (!fixed && !c->cost_items.empty()) {
        if (int rc = parse_walk(c, k, v.d_match_flags, nullptr)) return rc;
        if (int rc = parse_chain(c, k, true)) return rc;
        if (!k.g.fused_hist) LAUNCH_TRY(launch_histogram(st, v.chunks, c->cur_nchunks, k.g.split, v.codes, v.ncodes, v.hist));
        if (k.pack_by_chunk)
            LAUNCH_TRY(launch_huffman_chunks(st, v.blocks, c->cur_nblocks, c->cur_nchunks, v.hist, (BlockCodes *)c->d_bc.p,
                                             (uint64_t *)c->d_chunk_bits.p, nullptr));
        else
            LAUNCH_TRY(launch_huffman(st, v.blocks, c->cur_nblocks, v.hist, (BlockCodes *)c->d_bc.p, nullptr));
        HIP_TRY(hipMemsetAsync(v.hist, 0, 4ull * SYM_ROW * (k.pack_by_chunk ? (size_t)c->cur_nchunks : std::max<size_t>(c->cur_nblocks, 1)), st));
    }
    c->phase("lz77_cost_pass1");
    if (!c->cost_items.empty()) {
        const size_t bytes = sizeof(CostItem) * c->cost_items.size();
        if (int rc = c->d_cost_items.reserve(bytes)) return rc;
        HIP_TRY(hipMemcpyAsync(c->d_cost_items.p, c->cost_items.data(), bytes, hipMemcpyHostToDevice, st));
        LAUNCH_TRY(launch_cost_demote(st, k.d_in, v.chunks, (const CostItem *)c->d_cost_items.p, (uint32_t)c->cost_items.size(),
                                      (const BlockCodes *)c->d_bc.p, fixed, (const uint8_t *)c->d_len.p, (const uint16_t *)c->d_cd2.p,
                                      (uint16_t *)c->d_cd.p));
        k.v.cd = (uint16_t *)c->d_cd.p;
    }
    c->phase("lz77_cost_demote");
    return LFX_OK;
}

// the container checksum reads only the input: it runs on the side stream, beside the parse's chaining kernels (one wavefront
// per segment, a handful of steps each) and the one-workgroup-per-block Huffman kernel, which leave most of the GPU idle
// (forked: its first half went there behind the walk kernel, stage_parse).  The join: ev_join, waited for behind the Huffman kernel.
int checksum_fork(Ctx *c, const EncCall &k) {
    const EncView &v = k.v;
    HIP_TRY(hipEventRecord(c->ev_fork, c->stream));
    HIP_TRY(hipStreamWaitEvent(c->side_stream, c->ev_fork, 0));
    if (k.forked) LAUNCH_TRY(launch_checksum_part(c->side_stream, k.d_in, k.n, v.ck, v.ck + k.nspans, v.ck + 2 * k.nspans, v.res, k.ck_mode, 1, 2));
    else LAUNCH_TRY(launch_checksum(c->side_stream, k.d_in, k.n, v.ck, v.ck + k.nspans, v.ck + 2 * k.nspans, v.res, k.ck_mode));
    HIP_TRY(hipEventRecord(c->ev_join, c->side_stream));
    return LFX_OK;
}

// the blocks' symbol counts where the parse did not take them (a caller's own code words, LFX_HIST_SEPARATE, very unequal
// chunks), then one workgroup per block builds its codes
int stage_huffman(Ctx *c, const EncCall &k) {
    const EncView &v = k.v;
    hipStream_t st = c->stream;
    if (!k.g.fused_hist) LAUNCH_TRY(launch_histogram(st, v.chunks, c->cur_nchunks, k.g.split, v.codes, v.ncodes, v.hist));
    c->phase("histogram");
    // (pack by chunk: the counts are a row per chunk — the kernel sums a block's rows first and sizes every chunk behind its codes)
    if (k.pack_by_chunk)
        LAUNCH_TRY(launch_huffman_chunks(st, v.blocks, c->cur_nblocks, c->cur_nchunks, v.hist, (BlockCodes *)c->d_bc.p,
                                         (uint64_t *)c->d_chunk_bits.p, v.mdbg ? v.mdbg + 512 : nullptr));
    else
        LAUNCH_TRY(launch_huffman(st, v.blocks, c->cur_nblocks, v.hist, (BlockCodes *)c->d_bc.p, v.mdbg ? v.mdbg + 512 : nullptr));
    c->phase("huffman");
    if (v.mdbg) dbg_huffman(k);
    if (k.merge_blocks) {
        // block_merge: the first pass left every candidate's exact dynamic size in bc[].body_bits.  The merge
        // kernel rewrites the device's block AND chunk tables (and the code counts and counter rows, which every call makes
        // anew): neither equals its shadow any more, the next prepare uploads both, whatever its plan — a pass repeated by
        // with_match_fallback included.  The second pass builds the codes of the blocks that are left; absorbed ones are skipped.
        c->merge_ident.resize(c->cur_nblocks);
        for (uint32_t b = 0; b < c->cur_nblocks; b++) c->merge_ident[b] = b;
        if (c->cur_nblocks) HIP_TRY(hipMemcpyAsync(c->d_merge.p, c->merge_ident.data(), 4ull * c->cur_nblocks, hipMemcpyHostToDevice, st));
        c->n_merges = c->cur_nblocks;
        if (!c->merge_regions.empty()) {
            HIP_TRY(hipMemcpyAsync(c->d_merge_regions.p, c->merge_regions.data(), sizeof(MergeRegion) * c->merge_regions.size(),
                                   hipMemcpyHostToDevice, st));
            LAUNCH_TRY(launch_block_merge(st, (const MergeRegion *)c->d_merge_regions.p, (uint32_t)c->merge_regions.size(),
                                          (BlockDesc *)c->d_blocks.p, (ChunkDesc *)c->d_chunks.p, v.ncodes, v.hist, (BlockCodes *)c->d_bc.p,
                                          (uint32_t *)c->d_merge.p));
            c->up_dev[0] = 0;
            c->up_dev[1] = 0;
        }
        c->phase("block_merge");
        if (!c->merge_regions.empty())
            LAUNCH_TRY(launch_huffman(st, v.blocks, c->cur_nblocks, v.hist, (BlockCodes *)c->d_bc.p, nullptr));
        c->phase("huffman_merged");
    }
    if (k.auto_blocks) {
        // LFX_HUFFMAN_AUTO: in front of everything that reads a block's size or type — tile_bits, the offset
        // folds, the members' sizes.  Stored is a candidate only where the blocks have input bytes behind them (not for a
        // caller's own code words).  The device's block table no longer equals its shadow: the next prepare uploads it, whatever
        // its plan (as behind a BGZF fallback, encode_members).
        LAUNCH_TRY(launch_block_choose(st, (BlockDesc *)c->d_blocks.p, c->cur_nblocks, v.hist, (BlockCodes *)c->d_bc.p, k.hc == nullptr,
                                       (uint8_t *)c->d_choice.p));
        c->up_dev[1] = 0;
        c->n_choices = c->cur_nblocks;
        c->phase("block_choose");
    }
    return LFX_OK;
}

}  // namespace

int encode_prepare(Ctx *c, const Plan &plan, const EncodeSpec &sp, const uint8_t *d_in, uint64_t n, int ck_mode, const HostCodes *hc,
                   const lfx_dict *dict) {
    (void)hipSetDevice(c->device);
    c->n_ev = 0;
    c->phase("start");
    EncCall k{plan, sp.plan, d_in, n, ck_mode, hc, dict && dict->usable && !hc ? dict : nullptr, c->force_match_v1 || c->diag.match_v1,
              hc ? 0u : sp.chain_depth,     // (a caller's own code words switch the chain stage off)
              sp.lazy, sp.tuned, sp.tune, sp.cost && !hc, sp.auto_blocks, sp.merge_blocks,
              encode_geometry(plan, hc != nullptr, (uint32_t)std::max(c->n_cu, 1), c->diag.hist_separate, c->diag.pack_by_chunk)};
    if (k.g.err) { c->set_error(geom_error(k.g.err)); return LFX_E_ARG; }
    k.pack_by_chunk = k.g.pack_by_chunk && !k.auto_blocks && !k.merge_blocks && !c->idx_enc;
    c->cur_pack_by_chunk = k.pack_by_chunk;
    if (c->force_match_v1 && !hc) c->match_fallbacks++;      // (a silent fallback must be visible)
    c->cur_nchunks = (uint32_t)plan.chunks.size();
    c->cur_nblocks = (uint32_t)plan.blocks.size();
    c->cur_ntiles = plan.n_tiles;
    c->cur_n = n;
    c->cur_in = d_in;
    c->n_choices = 0;
    c->n_merges = 0;
    int rc;
    if ((rc = reserve_scratch(c, k))) return rc;
    if ((rc = upload_tables(c, k))) return rc;
    if ((rc = chunk_maps(c, k))) return rc;
    if (hc) rc = upload_codes(c, k);
    else {
        rc = stage_match(c, k);
        if (!rc && k.dict) rc = stage_dict(c, k);
        if (!rc && k.chain_depth) rc = stage_chain(c, k);
        if (!rc && k.cost) rc = stage_cost(c, k);
        if (!rc) rc = stage_parse(c, k);
    }
    if (rc) return rc;
    if (ck_mode && (rc = checksum_fork(c, k))) return rc;
    if ((rc = stage_huffman(c, k))) return rc;
    if (ck_mode) {
        HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_join, 0));
        c->phase("checksum");
    }
    return LFX_OK;
}

// LFX_DEBUG, pack by chunk: pack_chunk_kernel raised bit 1 of the result record's status — every tail that packs reports it
static const char *const PACK_MISMATCH = "pack by chunk: a chunk's packed size differs from its counted size";

int pack_blocks(Ctx *c, void *d_out) {
    if (c->cur_pack_by_chunk) {
        LAUNCH_TRY(launch_pack_chunks(c->stream, c->cur_in, c->cur_n, (const ChunkDesc *)c->d_chunks.p, c->cur_nchunks,
                                      (const BlockDesc *)c->d_blocks.p, c->cur_nblocks, (const uint32_t *)c->d_codes.p,
                                      (const uint32_t *)c->d_ncodes.p, (const BlockCodes *)c->d_bc.p, (const uint64_t *)c->d_block_start.p,
                                      (const uint64_t *)c->d_chunk_bits.p, c->diag.debug, (EncodeResult *)c->d_res.p, 0, (uint32_t *)d_out,
                                      (uint32_t)std::max(c->n_cu, 1)));
        return LFX_OK;
    }
    LAUNCH_TRY(launch_pack(c->stream, c->cur_in, c->cur_n, (const ChunkDesc *)c->d_chunks.p, c->cur_nchunks,
                           (const BlockDesc *)c->d_blocks.p, c->cur_nblocks, c->cur_ntiles,
                           (const uint32_t *)c->d_codes.p, (const uint32_t *)c->d_ncodes.p,
                           (const BlockCodes *)c->d_bc.p, (const uint64_t *)c->d_block_start.p,
                           (uint32_t *)c->d_tile_bits.p, (uint64_t *)c->d_tile_start.p, (const EncodeResult *)c->d_res.p, 0,
                           (uint32_t *)d_out, c->cur_tile_map));
    return LFX_OK;
}

int encode_emit(Ctx *c, int format, bool with_trailer, uint32_t trailer_check, bool use_device_check,
                uint64_t total_n, const uint8_t *prefix, uint32_t prefix_len, uint64_t start_bit,
                uint8_t *d_out, uint64_t cap, EncodeResult *host_res, EncodeResult *async_slot) {
    (void)hipSetDevice(c->device);
    hipStream_t st = c->stream;
    if (((uintptr_t)d_out & 3) != 0) { c->set_error("output buffer must be 4-byte aligned"); return LFX_E_ARG; }
    const uint64_t trailer = with_trailer ? trailer_len(format) : 0;
    if (cap < prefix_len + trailer + 8) { c->set_error("output capacity too small"); return LFX_E_NOSPACE; }
    const uint64_t cap_words = cap / 4;  // whole dwords only (kernels write dwords)
    const uint64_t cap_bits = (cap_words * 4 - trailer) * 8;
    HIP_TRY(c->prezero.join(st, d_out, cap_words * 4));
    c->phase("memset_out");
    EncodeResult *dres = (EncodeResult *)c->d_res.p;
    LAUNCH_TRY(launch_offsets(st, (const BlockDesc *)c->d_blocks.p, c->cur_nblocks, (const BlockCodes *)c->d_bc.p,
                              start_bit, cap_bits, (uint64_t *)c->d_block_start.p, dres));
    if (int rc = pack_blocks(c, d_out)) return rc;
    c->phase("pack");
    if (prefix_len) {
        // (a gzip header holds an unbounded file name / comment: its own buffer, sized to fit)
        int rcp = c->d_hdr.reserve(prefix_len);
        if (rcp) return rcp;
        HIP_TRY(hipMemcpyAsync(c->d_hdr.p, prefix, prefix_len, hipMemcpyHostToDevice, st));
        LAUNCH_TRY(launch_put_bytes(st, (const uint8_t *)c->d_hdr.p, prefix_len, 0, (uint32_t *)d_out));
    }
    if (!use_device_check) {
        // combined checksum supplied by the caller (sharded encode): patch the device result
        HIP_TRY(hipMemcpyAsync((uint8_t *)dres + offsetof(EncodeResult, crc32), &trailer_check, 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync((uint8_t *)dres + offsetof(EncodeResult, adler32), &trailer_check, 4, hipMemcpyHostToDevice, st));
    }
    LAUNCH_TRY(launch_trailer(st, with_trailer ? format : LFX_DEFLATE, (uint32_t)total_n, 0, dres, (uint32_t *)d_out));
    HIP_TRY(hipMemcpyAsync(async_slot ? (void *)async_slot : c->h_res, dres, sizeof(EncodeResult), hipMemcpyDeviceToHost, st));
    c->phase("frame");
    if (async_slot) return LFX_OK;
    HIP_TRY(hipStreamSynchronize(st));
    *host_res = *(EncodeResult *)c->h_res;
    if (host_res->status & 2u) { c->set_error(PACK_MISMATCH); return LFX_E_DEVICE; }
    if (host_res->status != 0) { c->set_error("output capacity too small"); return LFX_E_NOSPACE; }
    return LFX_OK;
}

int encode_batch(Ctx *c, const Plan &plan, const EncodeSpec &sp, const BatchCall &b, std::vector<uint64_t> &h_len,
                 std::vector<int32_t> &h_status, EncodeResult &res) {
    (void)hipSetDevice(c->device);
    hipStream_t st = c->stream;
    const uint32_t count = (uint32_t)b.streams.size();
    const uint32_t trailer = trailer_len(b.format);
    // per-stream scratch: descriptors, checksums, end bits, status, lengths (+ the header bytes)
    const size_t sz_streams = sizeof(BatchStream) * count;
    DevBuf &sb = c->d_dec_streams;     // (decode scratch: free during an encode)
    if (int rc = sb.reserve(sz_streams + (4 + 4 + 8 + 4 + 8) * (size_t)count + b.hdr.size() + 64)) return rc;
    BatchStream *d_streams = (BatchStream *)sb.p;
    uint64_t *d_end = (uint64_t *)((uint8_t *)sb.p + sz_streams);
    uint64_t *d_len = d_end + count;
    uint32_t *d_crc = (uint32_t *)(d_len + count), *d_adler = d_crc + count;
    int32_t *d_status = (int32_t *)(d_adler + count);
    uint8_t *d_hdr = (uint8_t *)(d_status + count);
    h_len.resize(count);
    h_status.resize(count);
    return with_match_fallback(c, res, [&]() -> int {
        if (int rc = encode_prepare(c, plan, sp, b.d_in, b.in_extent, 0, nullptr, b.dict)) return rc;
        HIP_TRY(hipMemcpyAsync(d_streams, b.streams.data(), sz_streams, hipMemcpyHostToDevice, st));
        if (!b.hdr.empty()) HIP_TRY(hipMemcpyAsync(d_hdr, b.hdr.data(), b.hdr.size(), hipMemcpyHostToDevice, st));
        if (trailer)
            LAUNCH_TRY(launch_checksum_ranges(st, b.d_in, count, (const uint64_t *)d_streams, sizeof(BatchStream) / 8,
                                              (const uint64_t *)d_streams + 1, sizeof(BatchStream) / 8, d_crc, d_adler));
        c->phase("checksum");
        // (the span of all streams' ranges, on the main stream: the one fill that does not go through Prezero)
        HIP_TRY(hipMemsetAsync(b.d_out + b.out_lo, 0, b.out_hi - b.out_lo, st));
        EncodeResult *dres = (EncodeResult *)c->d_res.p;
        LAUNCH_TRY(launch_offsets_batch(st, d_streams, count, (const BlockDesc *)c->d_blocks.p, (const BlockCodes *)c->d_bc.p,
                                        (uint32_t)b.hdr.size(), trailer, (uint64_t *)c->d_block_start.p, d_end, d_status, dres));
        if (int rc = pack_blocks(c, b.d_out)) return rc;
        c->phase("pack");
        LAUNCH_TRY(launch_frame_batch(st, b.format, d_streams, count, d_hdr, (uint32_t)b.hdr.size(), d_end, d_crc, d_adler, dres,
                                      (uint32_t *)b.d_out, d_len));
        HIP_TRY(hipMemcpyAsync(c->h_res, dres, sizeof(EncodeResult), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h_len.data(), d_len, 8ull * count, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h_status.data(), d_status, 4ull * count, hipMemcpyDeviceToHost, st));
        c->phase("frame");
        HIP_TRY(hipStreamSynchronize(st));
        res = *(EncodeResult *)c->h_res;
        if (res.status & 2u) { c->set_error(PACK_MISMATCH); return LFX_E_DEVICE; }
        return LFX_OK;
    });
}

int encode_batch_packed(Ctx *c, const Plan &plan, const EncodeSpec &sp, const BatchPackedCall &b, std::vector<uint64_t> &h_pairs,
                        EncodeResult &res) {
    (void)hipSetDevice(c->device);
    hipStream_t st = c->stream;
    const uint32_t count = (uint32_t)b.streams.size();
    const uint32_t trailer = trailer_len(b.format), nwg = (count + 255) / 256;
    // per-stream scratch: descriptors; end bits, offsets inside the workgroup, lengths, the {off, len} pairs, the frame kernel's
    // lengths; the workgroup sums; checksums (+ the header bytes)
    const size_t sz_streams = sizeof(BatchStream) * count;
    DevBuf &sb = c->d_dec_streams;     // (decode scratch: free during an encode)
    if (int rc = sb.reserve(sz_streams + (8 * 6 + 4 + 4) * (size_t)count + 8 * (size_t)nwg + b.hdr.size() + 64)) return rc;
    BatchStream *d_streams = (BatchStream *)sb.p;
    uint64_t *d_end = (uint64_t *)((uint8_t *)sb.p + sz_streams);
    uint64_t *d_local = d_end + count, *d_slen = d_local + count, *d_pairs = d_slen + count, *d_len = d_pairs + 2 * (size_t)count;
    uint64_t *d_wg = d_len + count;
    uint32_t *d_crc = (uint32_t *)(d_wg + nwg), *d_adler = d_crc + count;
    uint8_t *d_hdr = (uint8_t *)(d_adler + count);
    h_pairs.resize(2 * (size_t)count);
    // the kernels OR into zeros: [0, fill) is filled once, beside the match kernel; no stream can end behind the sum of the
    // bounds, and nothing is written when the total exceeds cap
    c->prezero.start(b.d_out, b.fill);
    const int rc = with_match_fallback(c, res, [&]() -> int {
        if (int rc2 = encode_prepare(c, plan, sp, b.d_in, b.in_extent, 0, nullptr, b.dict)) return rc2;
        HIP_TRY(hipMemcpyAsync(d_streams, b.streams.data(), sz_streams, hipMemcpyHostToDevice, st));
        if (!b.hdr.empty()) HIP_TRY(hipMemcpyAsync(d_hdr, b.hdr.data(), b.hdr.size(), hipMemcpyHostToDevice, st));
        if (trailer)
            LAUNCH_TRY(launch_checksum_ranges(st, b.d_in, count, (const uint64_t *)d_streams, sizeof(BatchStream) / 8,
                                              (const uint64_t *)d_streams + 1, sizeof(BatchStream) / 8, d_crc, d_adler));
        c->phase("checksum");
        EncodeResult *dres = (EncodeResult *)c->d_res.p;
        LAUNCH_TRY(launch_batch_pack_layout(st, d_streams, count, (const BlockDesc *)c->d_blocks.p, (const BlockCodes *)c->d_bc.p,
                                            (uint32_t)b.hdr.size(), trailer, b.align, b.cap, d_local, d_slen, d_wg,
                                            (uint64_t *)c->d_block_start.p, d_end, d_pairs, b.d_table, dres));
        c->phase("batch_layout");
        HIP_TRY(c->prezero.join(st, b.d_out, b.fill));
        if (int rc2 = pack_blocks(c, b.d_out)) return rc2;
        c->phase("pack");
        LAUNCH_TRY(launch_frame_batch(st, b.format, d_streams, count, d_hdr, (uint32_t)b.hdr.size(), d_end, d_crc, d_adler, dres,
                                      (uint32_t *)b.d_out, d_len));
        HIP_TRY(hipMemcpyAsync(c->h_res, dres, sizeof(EncodeResult), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h_pairs.data(), d_pairs, 16ull * count, hipMemcpyDeviceToHost, st));
        c->phase("frame");
        HIP_TRY(hipStreamSynchronize(st));
        res = *(EncodeResult *)c->h_res;
        if (res.status & 2u) { c->set_error(PACK_MISMATCH); return LFX_E_DEVICE; }
        return LFX_OK;
    });
    c->prezero.settle();     // (failed before the stream waited for the fill: it is on the caller's buffer)
    return rc;
}

int encode_members(Ctx *c, const Plan &plan, const EncodeSpec &sp, const MembersCall &m, EncodeResult &res) {
    hipStream_t st = c->stream;
    const MembersGeom &g = m.g;
    const uint32_t count = g.count;
    // per-member scratch: records, offsets inside the workgroup, lengths, checksums; the workgroup sums; the header
    const uint32_t nwg = (count + 255) / 256;
    const size_t cnt = std::max<uint32_t>(count, 1);
    DevBuf &sb = c->d_dec_streams;     // (decode scratch: free during an encode)
    if (int rc = sb.reserve((sizeof(lfx_member) + 8 + 8 + 4 + 4) * cnt + 8 * (size_t)std::max<uint32_t>(nwg, 1) + m.hdr.size() + 64)) return rc;
    lfx_member *d_members = (lfx_member *)sb.p;
    uint64_t *d_local = (uint64_t *)(d_members + cnt), *d_mlen = d_local + cnt, *d_wg = d_mlen + cnt;
    uint32_t *d_crc = (uint32_t *)(d_wg + std::max<uint32_t>(nwg, 1)), *d_adler = d_crc + cnt;
    uint8_t *d_hdr = (uint8_t *)(d_adler + cnt);
    // the kernels OR into zeros: [0, min(cap, bound)) is filled once, beside the match kernel; no member can end behind the
    // bound, and nothing is written when the total exceeds cap
    c->prezero.start(m.d_out, m.fill);
    const int rc = with_match_fallback(c, res, [&]() -> int {
        if (int rc2 = encode_prepare(c, plan, sp, m.d_in, g.n, 0, nullptr, nullptr)) return rc2;
        HIP_TRY(hipMemcpyAsync(d_hdr, m.hdr.data(), m.hdr.size(), hipMemcpyHostToDevice, st));
        EncodeResult *dres = (EncodeResult *)c->d_res.p;
        LAUNCH_TRY(launch_members_layout(st, g, (BlockDesc *)c->d_blocks.p, (const BlockCodes *)c->d_bc.p, d_local, d_mlen, d_wg, m.cap,
                                         (uint64_t *)c->d_block_start.p, d_members, dres));
        if (g.bgzf) c->up_dev[1] = 0;      // the device's block table no longer equals its shadow: the next prepare uploads it
        c->phase("members_layout");
        LAUNCH_TRY(launch_checksum_ranges(st, m.d_in, count, (const uint64_t *)d_members, sizeof(lfx_member) / 8,
                                          (const uint64_t *)d_members + 1, sizeof(lfx_member) / 8, d_crc, d_adler));
        c->phase("checksum");
        HIP_TRY(c->prezero.join(st, m.d_out, m.fill));
        if (int rc2 = pack_blocks(c, m.d_out)) return rc2;
        c->phase("pack");
        LAUNCH_TRY(launch_members_frame(st, g, d_hdr, d_members, d_crc, dres, (uint32_t *)m.d_out));
        HIP_TRY(hipMemcpyAsync(c->h_res, dres, sizeof(EncodeResult), hipMemcpyDeviceToHost, st));
        if (m.n_rec) HIP_TRY(hipMemcpyAsync(m.members, d_members, sizeof(lfx_member) * (size_t)m.n_rec, hipMemcpyDeviceToHost, st));
        c->phase("frame");
        HIP_TRY(hipStreamSynchronize(st));
        res = *(EncodeResult *)c->h_res;
        if (res.status & 2u) { c->set_error(PACK_MISMATCH); return LFX_E_DEVICE; }
        return LFX_OK;
    });
    c->prezero.settle();     // (failed before the stream waited for the fill: it is on the caller's buffer)
    return rc;
}

}  // namespace lfx
