// lfx_ctx.h — per-GPU context: HIP stream, grow-only scratch in HBM, last error, phase timers.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <vector>

#include "lfx_chain.h"
#include "lfx_common.h"
#include "lfx_cost.h"
#include "lfx_device.h"
#include "lfx_dict_enc.h"
#include <string.h>

#include "lfx_hostio.h"
#include "lfx_merge.h"

namespace lfx {

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    uint32_t gen = 0;           // bumped by every (re)allocation: a cached "this table is already there" must not survive one
    int reserve(size_t bytes);  // grow-only; contents are NOT preserved
    void release();
};

// Diagnostic switches, read from the environment ONCE when the context is created — never on the
// encode / decode paths.
struct Diag {
    bool debug = false;          // LFX_DEBUG: per-stage counters and cycle stamps on stderr
    bool match_v1 = false;       // LFX_MATCH_V1: first-generation match kernel (+ md → cd)
    bool no_serial = false;      // LFX_NO_SERIAL: the serial fallback of the single-stream decoder is an error
    bool batch_serial = false;   // LFX_BATCH_SERIAL: every stream of a batch through the serial kernel
    bool no_pieces = false;      // LFX_NO_PIECES
    bool no_final_cand = false;  // LFX_NO_FINAL_CAND: the finder reports no BFINAL header at all (the chain walk scans the last block on demand)
    bool no_small_scan = false;  // LFX_NO_SMALL_SCAN: 1024 slices a block also for small blocks (round 5's geometry)
    bool two_pass = false;       // LFX_TWO_PASS: every block through blk_emit_kernel (no storing scan)
    bool no_pin_slots = false;   // LFX_NO_PIN_SLOTS: the decode's small transfers as plain pageable copies (the path of a full arena)
    bool hist_separate = false;  // LFX_HIST_SEPARATE: the blocks' symbol counts by histogram_kernel (round 5) instead of inside parse_emit
    int pack_by_chunk = -1;      // LFX_PACK_BY_CHUNK: 0 the tile-parallel pack kernels always, 1 pack_chunk_kernel wherever it is legal (unset: by the geometry)
    bool store_tight = false;    // LFX_STORE_TIGHT: the storing scan's regions sized for 16 bits a code (tests: lanes overflow, blocks fall back)
    int enc_batch_mb = 0;        // LFX_ENC_BATCH_MB: the stream encoder encodes closed blocks once so many MiB wait (0: the default, 8)
    int dump_seg = -1;           // LFX_DUMP_SEG=<n> (with LFX_DEBUG): the parse state of segment n on stderr (-1: none)
    void read();
};

// N-GPU member decode: what lfx_decode_range_emit leaves for lfx_decode_range_map / lfx_decode_range_finish
struct RangeState {
    int state = -1;            // -1 none, 0 the slice holds bytes, 1 the slice is held as 16-bit symbols (d_dec_sym) and waits for its window
    uint64_t total = 0, before = 0, max_len = 0;   // slice bytes, member bytes in front of it, longest symbol unit
    uint8_t *d_out = nullptr;
    uint32_t nsu = 0;          // symbol units (their table lives in d_dec_win behind the windows)
};

struct Ctx {
    int device = 0;
    RangeState range;
    // lfx_decode_range_scan → lfx_decode_range_emit: which scan jobs stored their code words (the storing scan), and where
    std::vector<uint8_t> range_stored;
    std::vector<uint64_t> range_temp_off;
    std::vector<uint32_t> range_cap;
    Diag diag;
    int n_cu = 0;   // compute units of the device
    hipStream_t own_stream = nullptr, stream = nullptr;
    // work that only depends on the input (the container checksum) runs beside the thin kernels of the
    // main stream: fork / join through these two events
    hipStream_t side_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_zero = nullptr;
    // The pack kernels OR into a zero-filled output: the fill runs on the side stream, beside the match kernel, instead of
    // between the Huffman and the pack kernels (every entry point is synchronous, so nothing else is using the buffer).  While
    // `ptr` is set a fill may still be running on the caller's buffer: no entry point returns before join() or settle().
    struct Prezero {
        Ctx *c;
        const void *ptr = nullptr;
        uint64_t bytes = 0;
        // forget what was noted; bytes != 0: fork from c->stream (behind whatever the caller's stream still has queued on d_out: a
        // consumer of the previous encode, an allocator-reused block), fill on the side stream, record ev_zero → whether it took
        bool start(void *d_out, uint64_t bytes);
        // `st` waits for the fill of exactly d_out[0, bytes) — or fills it itself when no such fill is in flight
        hipError_t join(hipStream_t st, void *d_out, uint64_t bytes);
        // the host waits for a fill in flight and forgets it
        void settle();
    } prezero{this};
    // Every entry point that touches the context's scratch holds this lock: handles (encoders, decoders, LZ77 plug-ins)
    // of one context may live on different threads, they simply take turns on the GPU (SURVEY §8b threading row).
    std::recursive_mutex mu;
    std::string err;
    void set_error(const std::string &e) { err = e; }

    // encode scratch
    DevBuf d_chunks, d_blocks, d_segs, d_pwgs, d_cd, d_md, d_codes, d_ncodes, d_hist, d_bc, d_block_start, d_tile_bits,
        d_tile_start, d_ck, d_res, d_small, d_hdr, d_io_in, d_io_out, d_vis, d_segtmp, d_stage, d_chunkmap, d_glnk, d_ucount;
    // an encode with a preset dictionary: the work list of the dictionary candidate kernel, and its host copy
    // (it outlives the asynchronous upload: every encode entry point synchronises before it returns)
    DevBuf d_dict_items;
    std::vector<DictItem> dict_items;
    // an encode with ChainLz77Encoder: the refined candidates the parse reads, the chain kernel's work list and
    // its host copy.  Sized only by calls of that kind.  d_len: LazyLz77Encoder's (§20) length byte per position, sized only by
    // calls of that kind.
    DevBuf d_cd2, d_chain_items, d_len;
    // an encode with CostLz77Encoder: the cost kernel's work list and its host copy.  Sized only by calls of
    // that kind.
    DevBuf d_cost_items;
    std::vector<CostItem> cost_items;
    // lfx_dict_train_device: the counters, the picks, the record table and index, the step's prefix words
    // (lfx_dict_train.h: dtrain_scratch).  Sized only by calls of that kind.
    DevBuf d_dict_train;
    // lfx_shuffle_* (DESIGN.md §30): the record table and the tile list of one call (lfx_shuffle.h).  Sized only by calls of
    // that kind.
    DevBuf d_shuffle;
    // an encode with LFX_HUFFMAN_AUTO: the type every block left block_choose_kernel with, one byte per block.
    // Sized only by calls of that kind; n_choices: its entries of the last prepare (0: that call was not one) — read by the
    // test hook lfx_debug_block_choices alone, no encode path looks at either.
    DevBuf d_choice;
    uint32_t n_choices = 0;
    // an encode with block_merge: the regions block_merge_kernel works on, and for every block of the plan the
    // block its code words ended up in.  Sized only by calls of that kind; the host vectors outlive the asynchronous uploads
    // (every encode entry point synchronises before it returns).  n_merges: the entries of d_merge of the last prepare (0: that
    // call was not one) — read by the test hook lfx_debug_block_merges alone.
    DevBuf d_merge_regions, d_merge;
    std::vector<MergeRegion> merge_regions;
    std::vector<uint32_t> merge_ident;
    uint32_t n_merges = 0;
    // an encode that packs by chunk: 320 symbol counters per chunk, and every chunk's packed size and first bit
    // (16 bytes).  Sized only by calls of that kind.
    DevBuf d_hist_chunk, d_chunk_bits;
    std::vector<ChainItem> chain_items;
    // decode scratch
    // host shadows of the plan tables last uploaded (chunks, blocks, segments, parse workgroups) and the device buffers they
    // went to: an encode with the same plan (same size, schedule and options — every step of a loop) uploads nothing, and a
    // different plan is copied from the shadow, which outlives the asynchronous copy (no synchronisation either way)
    std::vector<uint8_t> up_shadow[4];
    uint64_t up_dev[4] = {0, 0, 0, 0};      // (buffer address ^ allocation generation << 48)
    DevBuf d_dec_streams, d_dec_state, d_dec_tmp, d_dec_cand, d_dec_blocks, d_dec_tabs, d_dec_sym, d_dec_win, d_dec_maps,
        d_dec_temp, d_dec_lanesx;     // round 6: the storing scan's per-lane code regions and BlkLanesX records
    // seek index (lfx_index.hip): copy tasks, probe results, the read path's staging areas
    DevBuf d_idx_tasks, d_idx_probe, d_idx_stage;
    DevBuf d_idx_enc;                   // lfx_encode_index_device: the candidate kernels' slots and per-tile sums (lfx_index_enc.hip)
    // BGZF reads by virtual offset (lfx_bgzf.hip): the walk's reads, results and segment list; the gather's tasks; the blocks a
    // group decodes into (at most 4096 x 64 KiB); the covered blocks of a host call, packed
    DevBuf d_bgzf_meta, d_bgzf_tasks, d_bgzf_scratch, d_bgzf_pack;
    struct IdxCollect *idx = nullptr;   // while lfx_decode_index_device runs: what the decode records for the index
    struct IdxCollect *idx_enc = nullptr;   // while lfx_encode_index_device runs: the encode leaves its candidates there
    std::vector<DevBuf *> all_bufs() {
        return {&d_chunks, &d_blocks, &d_segs, &d_pwgs, &d_cd, &d_md, &d_codes, &d_ncodes, &d_hist, &d_bc, &d_block_start,
                &d_tile_bits, &d_tile_start, &d_ck, &d_res, &d_small, &d_hdr, &d_io_in, &d_io_out, &d_vis, &d_segtmp, &d_stage, &d_chunkmap, &d_glnk, &d_ucount,
                &d_dec_streams, &d_dec_state, &d_dec_tmp, &d_dec_cand, &d_dec_blocks, &d_dec_tabs, &d_dec_sym, &d_dec_win, &d_dec_maps,
                &d_dec_temp, &d_dec_lanesx, &d_idx_tasks, &d_idx_probe, &d_idx_stage, &d_idx_enc,
                &d_bgzf_meta, &d_bgzf_tasks, &d_bgzf_scratch, &d_bgzf_pack, &d_dict_items, &d_cd2, &d_chain_items, &d_len, &d_choice, &d_hist_chunk, &d_chunk_bits,
                &d_merge_regions, &d_merge, &d_cost_items, &d_dict_train, &d_shuffle};
    }
    void *h_res = nullptr;  // pinned, 4 KiB (+ the arena below)
    // Small transfers of the decode paths (job lists up, scan results and counters down) go through page-locked memory: a
    // pageable hipMemcpyAsync is staged by the runtime on the calling thread, 20-45 us of idle GPU per transfer in the kernel
    // trace (round 6: 170 us of a 2.4 ms decode).  An arena behind h_res, handed out in slots, reset per member; a transfer
    // that does not fit goes the old way.
    static constexpr size_t PIN_ARENA = 1u << 20;
    size_t pin_used = 0;
    struct PinDown { void *slot, *dst; size_t n; };
    std::vector<PinDown> pin_pending;
    void pin_reset() { pin_used = 0; pin_pending.clear(); }
    void *pin_take(size_t n) {
        const size_t at = (pin_used + 63) & ~(size_t)63;
        if (!h_res || diag.no_pin_slots || at + n > PIN_ARENA) return nullptr;
        pin_used = at + n;
        return (uint8_t *)h_res + 4096 + at;
    }
    hipError_t small_up(void *dev, const void *host, size_t n, hipStream_t st) {
        if (!n) return hipSuccess;
        void *slot = pin_take(n);
        if (!slot) return hipMemcpyAsync(dev, host, n, hipMemcpyHostToDevice, st);
        memcpy(slot, host, n);
        return hipMemcpyAsync(dev, slot, n, hipMemcpyHostToDevice, st);
    }
    // host[0, n) <- dev[0, n): complete behind small_sync()
    hipError_t small_down(void *host, const void *dev, size_t n, hipStream_t st) {
        if (!n) return hipSuccess;
        void *slot = pin_take(n);
        if (!slot) return hipMemcpyAsync(host, dev, n, hipMemcpyDeviceToHost, st);
        pin_pending.push_back({slot, host, n});
        return hipMemcpyAsync(slot, dev, n, hipMemcpyDeviceToHost, st);
    }
    hipError_t small_sync(hipStream_t st) {
        const hipError_t e = hipStreamSynchronize(st);
        for (const PinDown &d : pin_pending) memcpy(d.dst, d.slot, d.n);
        pin_pending.clear();
        return e;
    }

    // state between encode_prepare and encode_emit (lfx_encode.cpp)
    uint32_t cur_nchunks = 0, cur_nblocks = 0;
    uint64_t cur_ntiles = 0, cur_n = 0;
    const uint32_t *cur_tile_map = nullptr;   // tile → chunk table of the prepared encode (lives in d_chunkmap)
    const uint8_t *cur_in = nullptr;
    bool cur_pack_by_chunk = false;           // the prepared encode counted its symbols per chunk: pack_blocks launches pack_chunk_kernel
    bool force_match_v1 = false;   // sticky: the second-generation match kernel reported a lane-order violation
    uint64_t match_fallbacks = 0;  // encode passes this context ran on the fallback kernel because of it (lfx_ctx_match_fallbacks)
    HostIo hostio;                 // copy streams and page-locked slabs for callers' pageable buffers (lfx_hostio.h), made on first use
    // Buffers of stream encoders / decoders that were freed, kept for the next handle of this context: page-locking 16 .. 64 MiB
    // and a hipMalloc per handle cost more than encoding a small stream (an encoder per file is the reference's own usage,
    // examples/flate.rs:89-110).  Taken and given back under `mu`; at most POOL_MAX of each kind are kept.
    static constexpr size_t POOL_MAX = 8;
    std::vector<PinVec> pin_pool;
    std::vector<DevBuf> dev_pool;
    PinVec take_pin() {            // the roomiest one (a handle's first buffer is its largest: pending input, window output)
        std::lock_guard<std::recursive_mutex> lock(mu);
        if (pin_pool.empty()) return PinVec();
        size_t best = 0;
        for (size_t i = 1; i < pin_pool.size(); i++)
            if (pin_pool[i].capacity() > pin_pool[best].capacity()) best = i;
        PinVec v = std::move(pin_pool[best]);
        pin_pool.erase(pin_pool.begin() + (std::ptrdiff_t)best);
        v.clear();
        return v;
    }
    void give_pin(PinVec &&v) {
        std::lock_guard<std::recursive_mutex> lock(mu);
        if (v.capacity() && pin_pool.size() < POOL_MAX) { v.clear(); pin_pool.push_back(std::move(v)); }
    }
    DevBuf take_dev() {
        std::lock_guard<std::recursive_mutex> lock(mu);
        if (dev_pool.empty()) return DevBuf();
        DevBuf b = dev_pool.back();
        dev_pool.pop_back();
        return b;
    }
    void give_dev(DevBuf &b) {
        std::lock_guard<std::recursive_mutex> lock(mu);
        if (b.p && dev_pool.size() < POOL_MAX) dev_pool.push_back(b);
        else b.release();
        b = DevBuf();
    }
    std::vector<uint8_t> shard_hdr;
    int shard_format = 0;
    bool shard_last = false;

    // phase timers
    int timing_on = 0;      // 0: no events; 1: an event behind every phase; 2..5: only the two events around ONE kernel's phase (the bench's
                            // timed steps: an event record between two kernels is ~6 us of idle GPU, two dozen of them 3 % of a 256 MiB
                            // round trip) — 2: lz77_walk, 3: blk_scan, 4: lz77_cand, 5: lz77_copy; 6: every phase, the encode's match and
                            // parse phases split by kernel (lz77_cand + lz77_resolve for lz77_match, lz77_walk + lz77_chain for lz77_parse)
    bool timing_fine() const { return timing_on >= 2; }
    static constexpr int MAX_EV = 17;   // events a call can record: who stamps several phases at once asks for the room first
    hipEvent_t ev[MAX_EV] = {};
    char ev_name[MAX_EV][24] = {};
    int n_ev = 0;
    void phase(const char *name);
};

}  // namespace lfx
