// lfx_member.cpp — the decode of ONE DEFLATE member on the GPU (inflate_member) as a sequence of stages: the block finder,
// the two piece scans, the block scan with its repairs and the chain walk, the emit of the code words, the materialisation,
// and the exact serial walk that every anomaly falls back to.  The stages that the N-GPU range calls and the size path run
// too are declared in lfx_decode_int.h; the host arithmetic without a HIP call lives in lfx_stages.h.
#include "lfx_decode_int.h"

#include <algorithm>
#include <cstdio>
#include <cstring>

#include "lfx_index.h"

namespace lfx {

int run_jobs(Ctx *c, const uint8_t *d_in, uint8_t *d_out, const std::vector<InflateJob> &jobs,
             std::vector<InflateResult> &res, const uint8_t *dict_end) {
    const size_t n = jobs.size();
    res.resize(n);
    if (!n) return LFX_OK;
    int rc;
    if ((rc = c->d_dec_streams.reserve(sizeof(InflateJob) * n))) return rc;
    if ((rc = c->d_dec_state.reserve(sizeof(InflateResult) * n))) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_dec_streams.p, jobs.data(), sizeof(InflateJob) * n, hipMemcpyHostToDevice, c->stream));
    if (dict_end)
        LAUNCH_TRY(launch_inflate_dict(c->stream, d_in, d_out, (const InflateJob *)c->d_dec_streams.p,
                                       (InflateResult *)c->d_dec_state.p, (uint32_t)n, dict_end));
    else
        LAUNCH_TRY(launch_inflate(c->stream, d_in, d_out, (const InflateJob *)c->d_dec_streams.p,
                                  (InflateResult *)c->d_dec_state.p, (uint32_t)n));
    HIP_TRY(hipMemcpyAsync(res.data(), c->d_dec_state.p, sizeof(InflateResult) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return LFX_OK;
}

// ------------------------------------------------------------------------------------------------
// shared stages (lfx_decode_int.h)

// ---- speculative block-start search
// survivors of stage 1 are ~0.1 % of the bit offsets (more on incompressible data): room for 0.4 % of them, so
// that a gibibyte-sized stream does not overflow the lists and fall back to the serial walk
int find_launch(Ctx *c, const uint8_t *d_in, uint64_t n, uint64_t off0, uint64_t final_from, FindBufs &fb) {
    hipStream_t st = c->stream;
    const uint64_t comp = n - off0;
    fb.shard_cap = find_shard_cap(comp);
    fb.final_cap = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1u << 16, comp / 4096), 1u << 24);
    int rc;
    if ((rc = c->d_dec_cand.reserve(8ull * fb.shard_cap * FIND_SHARDS + 8ull * fb.final_cap + 4 * FIND_HDR_WORDS))) return rc;
    fb.d_count = (uint32_t *)c->d_dec_cand.p;                       // the header (lfx_decode.h), the results, the lists
    fb.d_final = (uint64_t *)((uint8_t *)c->d_dec_cand.p + 4 * FIND_HDR_WORDS);   // (behind the header: both come back in ONE transfer)
    fb.d_cand = fb.d_final + fb.final_cap;
    HIP_TRY(hipMemsetAsync(fb.d_count, 0, 4 * FIND_HDR_WORDS, st));
    LAUNCH_TRY(launch_find_stage1(st, d_in, n, off0, fb.d_count, fb.d_cand, fb.shard_cap, final_from, (uint32_t)std::max(c->n_cu, 1)));
    return LFX_OK;
}

int find_collect(Ctx *c, const uint8_t *d_in, uint64_t n, const FindBufs &fb, Found &out) {
    hipStream_t st = c->stream;
    uint32_t *d_count = fb.d_count, *d_final_count = d_count + FIND_HDR_FINAL;
    const uint32_t n_cu = (uint32_t)std::max(c->n_cu, 1);
    // stage 2 takes the survivor counts from the device (persistent grid): no host round trip between the stages; the
    // counts, the overflow marker, the number of results and the first results come back in ONE round trip
    LAUNCH_TRY(launch_find_stage2(st, d_in, n, fb.d_cand, fb.shard_cap, d_count, d_count + FIND_HDR_WORK, d_final_count, fb.d_final,
                                  fb.final_cap, n_cu, c->diag.debug ? (uint64_t *)(d_count + FIND_HDR_DBG) : nullptr));
    constexpr uint32_t HEAD_N = 1024;      // (results that come back with the counts; a stream has a few hundred)
    const uint32_t head_n = std::min<uint32_t>(HEAD_N, fb.final_cap);
    std::vector<uint64_t> back(FIND_HDR_WORDS / 2 + head_n);      // header words, then the first results
    HIP_TRY(c->small_down(back.data(), d_count, 8ull * back.size(), st));
    HIP_TRY(c->small_sync(st));
    const uint32_t *hc = (const uint32_t *)back.data();
    out.overflow = hc[FIND_SHARDS] != 0;
    out.n1 = 0;
    for (uint32_t k = 0; k < FIND_SHARDS; k++) { if (hc[k] > fb.shard_cap) out.overflow = true; out.n1 += hc[k]; }
    if (c->diag.debug) {
        uint64_t d[7];
        memcpy(d, hc + FIND_HDR_DBG, sizeof d);
        fprintf(stderr, "[lfx] finder stage 2: batches=%llu cycles per batch: stage+fields=%llu table=%llu walk=%llu; steps per batch=%.1f "
                "restagings=%llu; wavefront lives (sum)=%llu\n", (unsigned long long)d[5], (unsigned long long)(d[0] / (d[5] ? d[5] : 1)),
                (unsigned long long)(d[1] / (d[5] ? d[5] : 1)), (unsigned long long)(d[2] / (d[5] ? d[5] : 1)),
                (double)d[3] / (double)(d[5] ? d[5] : 1), (unsigned long long)d[4], (unsigned long long)d[6]);
    }
    out.cand.clear();
    if (out.overflow) return LFX_OK;
    const uint32_t nf = std::min(hc[FIND_HDR_FINAL], fb.final_cap);
    out.cand.assign(back.begin() + FIND_HDR_WORDS / 2, back.begin() + FIND_HDR_WORDS / 2 + std::min(nf, head_n));
    out.cand.resize(nf);
    if (nf > head_n) HIP_TRY(hipMemcpy(out.cand.data() + head_n, fb.d_final + head_n, 8ull * (nf - head_n), hipMemcpyDeviceToHost));
    return LFX_OK;
}

// ---- ONE Huffman pass for a stream's own large blocks (round 6): the scan stores every lane's code words in a
//      region of its own (lfx_stages.h), blk_place_kernel moves them.  Not when the regions would not fit 16 GiB.
bool plan_store(Ctx *c, BlkJob *bj, uint32_t nj) {
    const uint64_t off = plan_store_regions(bj, nj, c->diag.store_tight);
    if (off * 4 > (16ull << 30) || c->d_dec_temp.reserve(off * 4) || c->d_dec_lanesx.reserve(sizeof(BlkLanesX) * (size_t)(nj + 1))) {
        clear_store_regions(bj, nj);
        return false;
    }
    return true;
}

int rescan_widen(Ctx *c, const uint8_t *d_in, uint64_t n, const std::vector<uint64_t> &starts, uint32_t nc,
                 std::vector<BlkInfo> &bi, std::vector<uint32_t> &slot, std::vector<uint8_t> &stored, bool scan_small) {
    hipStream_t st = c->stream;
    const size_t tab_bytes = blk_tabs_bytes();
    auto start_at = [&](size_t i) { return i < starts.size() ? starts[i] : n * 8; };
    for (uint32_t widen = 2; widen <= 6; widen++) {
        std::vector<uint32_t> redo;
        for (uint32_t i = 0; i < nc; i++) if (bi[slot[i]].status == BLK_NO_EOB && i + widen <= starts.size()) redo.push_back(i);
        if (redo.empty()) break;
        std::vector<BlkJob> rj(redo.size());
        for (size_t q = 0; q < redo.size(); q++) rj[q] = BlkJob{starts[redo[q]], start_at(redo[q] + widen)};
        int rc;
        if ((rc = c->d_dec_tmp.reserve(sizeof(BlkJob) * redo.size()))) return rc;
        BlkJob *d_rj = (BlkJob *)c->d_dec_tmp.p;
        HIP_TRY(hipMemcpyAsync(d_rj, rj.data(), sizeof(BlkJob) * redo.size(), hipMemcpyHostToDevice, st));
        for (size_t q = 0; q < redo.size(); q++) {
            slot[redo[q]] = redo[q];
            stored[redo[q]] = 0;            // (a classic scan takes the slot over: what its lanes stored before is stale)
            LAUNCH_TRY(launch_blk_scan(st, d_in, n, d_rj + q, 1, (BlkInfo *)c->d_dec_state.p + redo[q],
                                       (BlkLanes *)c->d_dec_blocks.p + redo[q],
                                       (uint8_t *)c->d_dec_tabs.p + tab_bytes * redo[q], scan_small));
        }
        for (size_t q = 0; q < redo.size(); q++)
            HIP_TRY(hipMemcpyAsync(&bi[redo[q]], (BlkInfo *)c->d_dec_state.p + redo[q], sizeof(BlkInfo), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return LFX_OK;
}

int emit_codes(Ctx *c, const uint8_t *d_in, uint64_t n, const std::vector<BlkEmit> &emit, uint64_t total_codes, uint32_t n_placed,
               uint32_t free_shift, bool scan_small, EmitBufs &eb) {
    hipStream_t st = c->stream;
    const uint32_t ne = (uint32_t)emit.size();
    int rc;
    if ((rc = c->d_dec_tmp.reserve(sizeof(BlkEmit) * (size_t)ne + 64))) return rc;
    if ((rc = c->d_hist.reserve(sizeof(BlkUnits) * (size_t)ne + 64))) return rc;
    if ((rc = c->d_codes.reserve(4 * std::max<uint64_t>(total_codes, 1)))) return rc;
    eb.d_flags = (uint32_t *)c->d_dec_tmp.p;
    eb.d_emit = (BlkEmit *)((uint8_t *)c->d_dec_tmp.p + 64);
    {
        // the flags (64 zero bytes) and the emit jobs behind them in ONE transfer (a fill and a copy of their own were
        // two launches with ten microseconds of idle GPU in front of each, between the scan and the place kernel)
        std::vector<uint8_t> upl(64 + sizeof(BlkEmit) * (size_t)ne, 0);
        memcpy(upl.data() + 64, emit.data(), sizeof(BlkEmit) * (size_t)ne);
        HIP_TRY(c->small_up(eb.d_flags, upl.data(), upl.size(), st));
    }
    const uint32_t unit_target = emit_unit_target(total_codes, c->n_cu);
    // (blocks whose codes the scan stored are moved into place; the others are decoded a second time)
    if (n_placed)
        LAUNCH_TRY(launch_blk_place(st, eb.d_emit, ne, (const BlkLanes *)c->d_dec_blocks.p, (const BlkLanesX *)c->d_dec_lanesx.p,
                                    (const uint32_t *)c->d_dec_temp.p, (uint32_t *)c->d_codes.p, eb.d_flags,
                                    (BlkUnits *)c->d_hist.p, unit_target, nullptr, free_shift));
    if (n_placed < ne)
        LAUNCH_TRY(launch_blk_emit(st, d_in, n, eb.d_emit, ne, (const BlkLanes *)c->d_dec_blocks.p,
                                   (uint32_t *)c->d_codes.p, eb.d_flags, (BlkUnits *)c->d_hist.p, unit_target, nullptr,
                                   c->d_dec_tabs.p, free_shift, total_codes >= 32768ull * ne, scan_small));
    c->phase("blk_emit");
    return LFX_OK;
}

// ---- block rounds
int scan_round(Ctx *c, const uint8_t *d_in, uint64_t n, const std::vector<BlkJob> &bj, bool want_tabs, std::vector<BlkInfo> &bi,
               bool &small, bool stamp) {
    hipStream_t st = c->stream;
    const uint32_t nj = (uint32_t)bj.size();
    int rc;
    if ((rc = c->d_dec_streams.reserve(sizeof(BlkJob) * nj))) return rc;
    if ((rc = c->d_dec_state.reserve(sizeof(BlkInfo) * nj))) return rc;
    if ((rc = c->d_dec_cand.reserve(sizeof(BlkLanes) * (size_t)nj))) return rc;
    if (want_tabs && (rc = c->d_dec_tabs.reserve(blk_tabs_bytes() * nj))) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_dec_streams.p, bj.data(), sizeof(BlkJob) * nj, hipMemcpyHostToDevice, st));
    // (ranges of a few tens of KB: the 256-lane instances of the scan and the emit kernel — a 32 KB block in 1024 slices is
    //  17 symbols a lane; LFX_NO_SMALL_SCAN=1 keeps 1024.  A job that continues a block covers the bits from lo_bit on.)
    uint64_t range_bits = 0;
    for (const BlkJob &j : bj) range_bits += j.end_bit - std::max(j.start_bit, j.lo_bit);
    small = !c->diag.no_small_scan && range_bits / nj < (512ull << 10);
    LAUNCH_TRY(launch_blk_scan(st, d_in, n, (const BlkJob *)c->d_dec_streams.p, nj, (BlkInfo *)c->d_dec_state.p,
                               (BlkLanes *)c->d_dec_cand.p, want_tabs ? c->d_dec_tabs.p : nullptr, small));
    if (stamp) c->phase("blk_scan");
    bi.resize(nj);
    HIP_TRY(hipMemcpyAsync(bi.data(), c->d_dec_state.p, sizeof(BlkInfo) * nj, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return LFX_OK;
}

int emit_round(Ctx *c, const uint8_t *d_in, uint64_t n, const std::vector<BlkEmit> &emit, uint64_t total_codes, bool small,
               uint8_t *d_out, std::vector<uint32_t> &jf, bool stamp, const uint8_t *dict_end) {
    hipStream_t st = c->stream;
    const uint32_t ne = (uint32_t)emit.size();
    const EmitTmp t = emit_tmp_layout(ne);
    int rc;
    if ((rc = c->d_dec_tmp.reserve(t.total))) return rc;
    if ((rc = c->d_hist.reserve(sizeof(BlkUnits) * (size_t)ne + 64))) return rc;
    if ((rc = c->d_codes.reserve(4 * std::max<uint64_t>(total_codes, 1)))) return rc;
    uint8_t *tmp = (uint8_t *)c->d_dec_tmp.p;
    uint32_t *d_flags = (uint32_t *)(tmp + t.flags), *d_jf = (uint32_t *)(tmp + t.job_flags);
    BlkEmit *d_emit = (BlkEmit *)(tmp + t.jobs);
    HIP_TRY(hipMemsetAsync(d_flags, 0, 64 + 4ull * ne, st));
    HIP_TRY(hipMemcpyAsync(d_emit, emit.data(), sizeof(BlkEmit) * ne, hipMemcpyHostToDevice, st));
    LAUNCH_TRY(launch_blk_emit(st, d_in, n, d_emit, ne, (const BlkLanes *)c->d_dec_cand.p, (uint32_t *)c->d_codes.p, d_flags,
                               (BlkUnits *)c->d_hist.p, emit_unit_target(total_codes, c->n_cu), d_jf, c->d_dec_tabs.p, 17, false, small));
    if (stamp) c->phase("blk_emit");
    if (dict_end)
        LAUNCH_TRY(launch_blk_materialize_dict(st, d_in, d_emit, ne, (const BlkUnits *)c->d_hist.p, (const uint32_t *)c->d_codes.p,
                                               d_out, dict_end));
    else
        LAUNCH_TRY(launch_blk_materialize(st, d_in, d_emit, ne, (const BlkLanes *)c->d_dec_cand.p, (const BlkUnits *)c->d_hist.p,
                                          (const uint32_t *)c->d_codes.p, d_out, nullptr));
    if (stamp) c->phase("lz77_copy");
    jf.resize(ne);
    HIP_TRY(hipMemcpyAsync(jf.data(), d_jf, 4ull * ne, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return LFX_OK;
}

// ------------------------------------------------------------------------------------------------
// the member decode

namespace {

// what one inflate_member call decodes (fixed for the call)
struct Member {
    Ctx *c;
    const uint8_t *d_in;
    uint64_t n, off0;
    uint8_t *d_out;
    uint64_t cap;
    uint64_t first_bit, stop_bit;
    bool partial;
    uint64_t hist;
    const uint8_t *hist_win;   // null: the history lies in front of d_out; else a detached 32 KiB window that ends with it
    uint64_t comp;         // compressed bytes from off0 on
    uint64_t end_bits() const { return n * 8; }
};

// the chain of blocks (or pieces) under construction: what a scan stage leaves for the emit and the materialisation
struct Chain {
    std::vector<BlkEmit> emit;
    uint64_t pos;                   // header bit of the block the chain stands in front of
    uint64_t total = 0, total_codes = 0;
    uint64_t last_end = 0;          // end bit of the last block of the chain
    bool ok = false, final = false; // the chain is complete; its last block is the member's final one
    bool front_bad = false;         // the window's FIRST block does not scan: damaged rather than incomplete
    bool pieces = false;            // the entries are pieces (a piece scan built the chain)
    bool pieces_multi = false;      // some block was scanned in more than one piece (its pieces read each other's output)
    bool units_per_piece = false;   // (pieces over candidate ranges that fill the GPU: one symbol unit per piece)
    bool scan_small = false;        // the 256-lane instances of scan and emit (small blocks)
    uint32_t n_placed = 0;          // blocks whose codes the scan stored (blk_place_kernel instead of blk_emit_kernel)
    uint32_t n_on_demand = 0;       // blocks of the chain the finder did not report (scanned one by one)
    explicit Chain(uint64_t first_bit) : pos(first_bit) {}
    // the block (or piece) at `pos`, scanned into `slot`, joins the chain
    BlkEmit &push(const BlkInfo &r, uint32_t slot, uint64_t hist) {
        emit.push_back(blk_emit_of(r, pos, slot, total, total_codes, hist + total));
        total += r.n_out;
        total_codes += r.n_codes;
        return emit.back();
    }
    // the block whose last (or only) piece is `r` is complete
    void close_block(const BlkInfo &r) {
        last_end = r.end_bit;
        if (r.bfinal) { ok = true; final = true; } else pos = r.end_bit;
    }
};

// the finder for this member: the sorted block starts, the known first one among them
int find_starts(const Member &m, std::vector<uint64_t> &starts, Found &fd) {
    Ctx *c = m.c;
    FindBufs fb;
    int rc;
    const uint64_t final_from = c->diag.no_final_cand ? ~0ull >> 1 : find_final_from(m.n, m.comp);
    if ((rc = find_launch(c, m.d_in, m.n, m.off0, final_from, fb))) return rc;
    c->phase("find1");
    if ((rc = find_collect(c, m.d_in, m.n, fb, fd))) return rc;
    starts.clear();
    starts.push_back(m.first_bit);  // the first block's start is known
    if (fd.overflow) return LFX_OK;
    c->phase("find2");
    for (uint64_t b : fd.cand) if (b != m.first_bit) starts.push_back(b);
    std::sort(starts.begin(), starts.end());
    return LFX_OK;
}

// scan jobs [slot0, slot0 + jobs.size()) of the piece stages: upload, one launch, results back
int scan_pieces(const Member &m, const std::vector<BlkJob> &jobs, uint32_t slot0, std::vector<BlkInfo> &infos) {
    Ctx *c = m.c;
    hipStream_t st = c->stream;
    const uint32_t nj = (uint32_t)jobs.size();
    infos.resize(nj);
    HIP_TRY(hipMemcpyAsync((BlkJob *)c->d_dec_streams.p + slot0, jobs.data(), sizeof(BlkJob) * nj, hipMemcpyHostToDevice, st));
    LAUNCH_TRY(launch_blk_scan(st, m.d_in, m.n, (const BlkJob *)c->d_dec_streams.p + slot0, nj, (BlkInfo *)c->d_dec_state.p + slot0,
                               (BlkLanes *)c->d_dec_blocks.p + slot0, (uint8_t *)c->d_dec_tabs.p + blk_tabs_bytes() * slot0));
    HIP_TRY(hipMemcpyAsync(infos.data(), (BlkInfo *)c->d_dec_state.p + slot0, sizeof(BlkInfo) * nj, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return LFX_OK;
}
int reserve_scan_slots(Ctx *c, size_t nslots) {
    int rc;
    if ((rc = c->d_dec_streams.reserve(sizeof(BlkJob) * nslots))) return rc;
    if ((rc = c->d_dec_state.reserve(sizeof(BlkInfo) * nslots))) return rc;
    if ((rc = c->d_dec_blocks.reserve(sizeof(BlkLanes) * nslots))) return rc;
    return c->d_dec_tabs.reserve(blk_tabs_bytes() * nslots);
}

// ---- a stream of a FEW ordinary blocks (round 4: 2 … 32 candidates, at least 128 KiB of stream each — a 16 MiB
// member is 16 blocks for 256 CUs: K1 and K2 ran on sixteen of them, K3 on sixty-four chunk units, 2.3 ms): every
// candidate's range [start, next candidate) is scanned in pieces at once, with the tables of the block that
// starts there.  Accepted only if every block's pieces chain, the piece that holds its EndOfBlock ends exactly
// where the next candidate starts, and the last block is final; anything else (a false candidate, a stored or
// fixed block in between, damage) leaves the stream to the one-workgroup-per-block path.
// (Measured, profiles/r04_small_sizes.json: 16 MiB 2.25 -> 1.75 ms; at 64 blocks the marker path's fixed costs — window
//  resolution 0.6 ms, symbol units — outweigh what K1 / K2 gain: 2.87 against 2.40 ms.  Hence up to 32 candidates.)
int pieces_over_ranges(const Member &m, const std::vector<uint64_t> &starts, Chain &ch) {
    Ctx *c = m.c;
    const uint32_t nc = (uint32_t)starts.size();
    const uint64_t end_bits = m.end_bits();
    auto start_at = [&](uint32_t i) { return i < nc ? starts[i] : end_bits; };
    // two pieces per CU over the whole stream, every block split EVENLY — the blocks' rounding taken off the target, so that
    // the pieces, one symbol unit each, are all resident at once
    const uint64_t ptarget = (uint64_t)std::max<int64_t>(2ll * std::max(c->n_cu, 1) - (int64_t)nc, (int64_t)nc);
    const uint64_t PIECE_BITS = piece_bits(end_bits - m.first_bit, ptarget), OVERLAP = piece_overlap(PIECE_BITS);
    std::vector<BlkJob> pj;
    std::vector<uint32_t> first_piece(nc + 1, 0);
    for (uint32_t i = 0; i < nc; i++) {
        first_piece[i] = (uint32_t)pj.size();
        add_pieces(pj, starts[i], start_at(i + 1), PIECE_BITS, OVERLAP);
    }
    first_piece[nc] = (uint32_t)pj.size();
    const uint32_t npj = (uint32_t)pj.size();
    ch.units_per_piece = npj >= (uint32_t)std::max(c->n_cu, 1);
    // (+ slots for the repair launches below: a range cut in two by a false candidate is scanned again as one)
    constexpr uint32_t REPAIRS = 2;
    const uint32_t repair_slots = REPAIRS * (2 * (uint32_t)((end_bits - m.first_bit) / nc / PIECE_BITS + 2) + 4);
    const uint32_t nslots = npj + repair_slots;
    int rc;
    if ((rc = reserve_scan_slots(c, nslots))) return rc;
    std::vector<BlkInfo> pi;
    if ((rc = scan_pieces(m, pj, 0, pi))) return rc;
    bool fail = false;
    // the pieces of one range in order → emit entries.  0: the block closed (pos / ok updated); 1: every piece is
    // open (no EndOfBlock in the range); 2: damaged, or the pieces do not chain
    auto walk_range = [&](const BlkInfo *infos, uint32_t cnt, uint32_t slot0) -> int {
        uint64_t prev_end = 0;
        for (uint32_t q = 0; q < cnt; q++) {
            const BlkInfo &r = infos[q];
            if (r.status == BLK_BAD || r.btype == 0 || (q && r.data_bit != prev_end) || r.end_bit <= ch.pos || r.end_bit > end_bits) return 2;
            ch.push(r, slot0 + q, m.hist);
            prev_end = r.end_bit;
            if (r.status == BLK_OK) {
                ch.pieces_multi |= q > 0;
                ch.close_block(r);
                return 0;
            }
        }
        return 1;
    };
    uint32_t repairs = 0, rslot = npj;
    for (uint32_t i = 0; i < nc && !fail && !ch.ok; i++) {
        if (starts[i] != ch.pos) { fail = true; break; }             // (the chain must pass through every candidate)
        const size_t emit_mark = ch.emit.size();
        const uint64_t total_mark = ch.total, codes_mark = ch.total_codes;
        int res = walk_range(&pi[first_piece[i]], first_piece[i + 1] - first_piece[i], first_piece[i]);
        if (res == 1 && i + 1 < nc && repairs < REPAIRS) {
            // No EndOfBlock up to the next candidate: that candidate is a false one inside this block (about one
            // per 30 MB of stream survives the finder), and the pieces behind it were scanned with tables read from
            // data.  The block's true range — up to the candidate after it — is scanned again, alone.
            ch.emit.resize(emit_mark); ch.total = total_mark; ch.total_codes = codes_mark;
            std::vector<BlkJob> rj;
            add_pieces(rj, starts[i], start_at(i + 2), PIECE_BITS, OVERLAP);
            const uint32_t nr = (uint32_t)rj.size();
            if (rslot + nr > nslots) { fail = true; break; }
            std::vector<BlkInfo> ri;
            if ((rc = scan_pieces(m, rj, rslot, ri))) return rc;
            res = walk_range(ri.data(), nr, rslot);
            if (c->diag.debug) fprintf(stderr, "[lfx]  pieces: candidate %u (bit %llu) is a false one, its block scanned again in %u pieces: %d\n", i + 1,
                                       (unsigned long long)starts[i + 1], nr, res);
            rslot += nr;
            repairs++;
            i++;                      // (the false candidate is not a block)
        }
        if (res != 0) fail = true;
    }
    if (c->diag.debug) fprintf(stderr, "[lfx]  pieces over %u candidate ranges: ok=%d fail=%d pieces=%zu of %u total=%llu\n", nc, (int)ch.ok, (int)fail,
                               ch.emit.size(), npj, (unsigned long long)ch.total);
    if (fail || !ch.ok) ch = Chain(m.first_bit);
    else ch.pieces = true;
    c->phase("pieces");
    return LFX_OK;
}

// ---- few candidates in a long stream = few, huge blocks (schedule S1: ONE block for the whole input).
// One workgroup per block would scan it alone; instead the block is scanned in PIECES of 4 Mbit, one
// workgroup each, all with the block's tables.  A piece finds its first symbol boundary by a warm-up
// decode that starts a few Kbit early; it is accepted iff that boundary equals the exit of the piece in
// front of it (piece 0 starts exactly behind the header), so the chain of pieces is proven, not assumed.
// Pieces behave like blocks from here on (their back-references cross pieces: marker path).
// Piece size (round 4): a 1 MiB stream is ONE block too — one workgroup in K1 and K2, four units in K3 (2.1 ms).
// Pieces adapt to the stream: enough of them to give every CU two, between 256 Kbit and 4 Mbit each.
// (few candidates in a long stream = few, huge blocks — at least 2 MiB of stream per candidate; a 4 MiB stream of four
//  ordinary blocks is not that case: walking it block by block costs a dependent step per block)
// small_first: a small stream walked from its known first block without the finder; when it turns out to have many blocks
// (more than the walk pays for), the finder runs after all and `starts` / `fd` are its verdict.
int pieces_block_walk(const Member &m, bool small_first, std::vector<uint64_t> &starts, Found &fd, Chain &ch) {
    Ctx *c = m.c;
    const uint64_t end_bits = m.end_bits();
    const uint64_t PIECE_BITS = piece_bits(end_bits - m.first_bit, 2ull * (uint64_t)std::max(c->n_cu, 1)), OVERLAP = piece_overlap(PIECE_BITS);
    const uint32_t cap_slots = (uint32_t)std::min<uint64_t>((end_bits - m.first_bit) / PIECE_BITS * 2 + 64, 1u << 20);
    int rc;
    if ((rc = reserve_scan_slots(c, cap_slots))) return rc;
    uint32_t base = 0;
    bool fail = false;
    for (uint32_t iter = 0; iter < (small_first ? 4u : 64u) && !fail && !ch.ok; iter++) {
        std::vector<BlkJob> pj;
        add_fixed_pieces(pj, ch.pos, end_bits, PIECE_BITS, OVERLAP);
        const uint32_t np = (uint32_t)pj.size();
        if (np == 0 || base + np > cap_slots) { fail = true; break; }
        std::vector<BlkInfo> pi;
        if ((rc = scan_pieces(m, pj, base, pi))) return rc;
        uint32_t used = 0;
        bool closed = false;
        uint64_t prev_end = 0;
        for (uint32_t q = 0; q < np && !closed; q++) {
            const BlkInfo &r = pi[q];
            if (c->diag.debug && (q < 3 || r.status != BLK_NO_EOB))
                fprintf(stderr, "[lfx]   piece %u/%u: status=%u btype=%u data=%llu end=%llu prev_end=%llu lanes=%u codes=%u out=%llu rounds=%u cyc_hdr=%u cyc_total=%u\n", q, np,
                        r.status, r.btype, (unsigned long long)r.data_bit, (unsigned long long)r.end_bit,
                        (unsigned long long)prev_end, r.nlanes, r.n_codes, (unsigned long long)r.n_out, r.rounds, r.cyc_hdr, r.cyc_total);
            if (r.status == BLK_BAD || (q && r.data_bit != prev_end) || r.end_bit <= ch.pos || r.end_bit > end_bits) { fail = true; break; }
            if (q == 0 && r.btype == 0 && r.status != BLK_OK) { fail = true; break; }
            ch.push(r, base + q, m.hist);   // (a stream decoder's last window arrives with history)
            used = q + 1;
            prev_end = r.end_bit;
            if (r.status == BLK_OK) {          // the piece that holds EndOfBlock (or a whole stored block)
                closed = true;
                ch.pieces_multi |= q > 0;
                ch.close_block(r);
            }
        }
        if (!closed) fail = true;
        base += used;
    }
    if (c->diag.debug) fprintf(stderr, "[lfx]  pieces: ok=%d fail=%d pieces=%zu total=%llu\n", (int)ch.ok, (int)fail, ch.emit.size(), (unsigned long long)ch.total);
    if (fail || !ch.ok) ch = Chain(m.first_bit);
    else ch.pieces = true;
    c->phase("pieces");
    if (small_first && !ch.pieces) return find_starts(m, starts, fd);     // many blocks after all: the finder, then one workgroup per block
    return LFX_OK;
}

// ---- K1: every candidate block is scanned by a 1024-lane workgroup (speculative slices, chained exits) for its end
//      bit, byte and code counts; then the chain from the known first block through the candidates' end bits
int block_scan(const Member &m, const std::vector<uint64_t> &starts, uint32_t n1, Chain &ch, MemberResult &mr) {
    Ctx *c = m.c;
    hipStream_t st = c->stream;
    const uint8_t *d_in = m.d_in;
    const uint64_t n = m.n;
    const uint32_t nc = (uint32_t)starts.size();
    const size_t tab_bytes = blk_tabs_bytes();
    int rc;
    std::vector<BlkJob> bj(nc);
    for (uint32_t i = 0; i < nc; i++) bj[i] = BlkJob{starts[i], i + 1 < nc ? starts[i + 1] : n * 8};
    const std::vector<int32_t> alt = add_alt_jobs(bj, starts, n * 8, m.comp);
    const uint32_t nj = (uint32_t)bj.size();
    // (+ EXTRA slots for blocks the finder cannot see — fixed-Huffman and stored blocks of other encoders —
    // which the chain walk below scans on demand)
    constexpr uint32_t EXTRA = 64, MAX_ON_DEMAND = 1u << 16;
    if ((rc = c->d_dec_streams.reserve(sizeof(BlkJob) * (nj + 1)))) return rc;
    if ((rc = c->d_dec_state.reserve(sizeof(BlkInfo) * (nj + EXTRA + 1)))) return rc;
    if ((rc = c->d_dec_blocks.reserve(sizeof(BlkLanes) * (size_t)(nj + EXTRA + 1)))) return rc;
    if ((rc = c->d_dec_tabs.reserve(tab_bytes * (nj + EXTRA + 1)))) return rc;
    // ---- ONE Huffman pass for a stream's own large blocks (round 6): the scan stores every lane's code words in a
    //      region of its own (cap = half a code per bit of the slice + a head's worth + slack: a slice whose codes
    //      average less than two bits overflows, is flagged, and takes the emit kernel as before), blk_place_kernel
    //      moves them.  Only the first batch of jobs stores; rescans and on-demand scans are the classic ones.
    //      Not for thousands of small blocks (the regions' fixed part would dominate) or when the regions would
    //      not fit 16 GiB; LFX_TWO_PASS=1 keeps the emit kernel for everything.
    std::vector<uint8_t> stored(nj + EXTRA + 1, 0);
    // another encoder's blocks of a few tens of KB: the 256-lane instances of the scan and the emit kernel — for EVERY scan
    // of this call (rescans and on-demand scans too: the emit launch takes all blocks in one geometry)
    ch.scan_small = !c->diag.no_small_scan && nj && (n * 8) / nj < (512ull << 10);
    const bool store_mode = !c->diag.two_pass && nj && (n * 8) / nj >= (1ull << 20) && plan_store(c, bj.data(), nj);
    HIP_TRY(c->small_up(c->d_dec_streams.p, bj.data(), sizeof(BlkJob) * nj, st));
    if (store_mode)
        LAUNCH_TRY(launch_blk_scan_store(st, d_in, n, (const BlkJob *)c->d_dec_streams.p, nj, (BlkInfo *)c->d_dec_state.p,
                                         (BlkLanes *)c->d_dec_blocks.p, c->d_dec_tabs.p, (uint32_t *)c->d_dec_temp.p,
                                         (BlkLanesX *)c->d_dec_lanesx.p));
    else
        LAUNCH_TRY(launch_blk_scan(st, d_in, n, (const BlkJob *)c->d_dec_streams.p, nj, (BlkInfo *)c->d_dec_state.p,
                                   (BlkLanes *)c->d_dec_blocks.p, c->d_dec_tabs.p, ch.scan_small));
    std::vector<BlkInfo> bi(nj);
    HIP_TRY(c->small_down(bi.data(), c->d_dec_state.p, sizeof(BlkInfo) * nj, st));
    HIP_TRY(c->small_sync(st));
    for (BlkInfo &b : bi) if (b.status == BLK_OK && b.end_bit > n * 8) b.status = BLK_NO_EOB;   // (cut by the input's end)
    if (store_mode) for (uint32_t j = 0; j < nj; j++) stored[j] = bi[j].status == BLK_OK && bi[j].btype != 0 && bi[j]._pad == 0;
    c->phase("blk_scan");
    // slot[i]: where candidate i's scan result and lanes live (its own slot or the wider job's)
    std::vector<uint32_t> slot(nc);
    for (uint32_t i = 0; i < nc; i++)
        slot[i] = (bi[i].status == BLK_NO_EOB && alt[i] >= 0 && bi[alt[i]].status == BLK_OK) ? (uint32_t)alt[i] : i;
    if (c->diag.debug) {
        fprintf(stderr, "[lfx] finder: stage1=%u candidates=%u scan jobs=%u (alternatives: %u)\n", n1, nc, nj, nj - nc);
        for (uint32_t i = 0; i < nc && i < 12; i++)
            fprintf(stderr, "[lfx]  cand %u start=%llu status=%u btype=%u final=%u end=%llu n_out=%llu n_codes=%u lanes=%u rounds=%u cyc_hdr=%u cyc_total=%u\n",
                    i, (unsigned long long)starts[i], bi[i].status, bi[i].btype, bi[i].bfinal,
                    (unsigned long long)bi[i].end_bit, (unsigned long long)bi[i].n_out, bi[i].n_codes,
                    bi[i].nlanes, bi[i].rounds, bi[i].cyc_hdr, bi[i].cyc_total);
        uint32_t nbad = 0, maxr = 0;
        for (uint32_t i = 0; i < nc; i++) { nbad += bi[i].status != BLK_OK; maxr = std::max(maxr, bi[i].rounds); }
        fprintf(stderr, "[lfx]  not-ok=%u max_rounds=%u\n", nbad, maxr);
    }
    // still without an end-of-block: rescan those together with wider and wider ranges
    if ((rc = rescan_widen(c, d_in, n, starts, nc, bi, slot, stored, ch.scan_small))) return rc;
    c->phase("repair");
    // ---- chain from the known first block
    uint32_t n_extra = 0;
    for (;;) {
        if (ch.pos == m.stop_bit && !ch.emit.empty()) { ch.ok = true; break; }
        auto it = std::lower_bound(starts.begin(), starts.end(), ch.pos);
        uint32_t k;
        BlkInfo r;
        if (it != starts.end() && *it == ch.pos) { k = slot[(uint32_t)(it - starts.begin())]; r = bi[k]; }
        else {
            // not a dynamic-block start the finder knows: scan the block that starts here on demand
            // (stored blocks need no slot; fixed / late dynamic ones keep one of the EXTRA slots)
            if (ch.pos >= n * 8 || ch.n_on_demand++ >= MAX_ON_DEMAND || n_extra >= EXTRA) break;
            k = nj + n_extra;
            const BlkJob one{ch.pos, it != starts.end() ? *it : n * 8};
            BlkJob *d_one = (BlkJob *)c->d_dec_streams.p + nj;
            HIP_TRY(hipMemcpyAsync(d_one, &one, sizeof one, hipMemcpyHostToDevice, st));
            LAUNCH_TRY(launch_blk_scan(st, d_in, n, d_one, 1, (BlkInfo *)c->d_dec_state.p + k,
                                       (BlkLanes *)c->d_dec_blocks.p + k, (uint8_t *)c->d_dec_tabs.p + tab_bytes * k, ch.scan_small));
            HIP_TRY(hipMemcpyAsync(&r, (BlkInfo *)c->d_dec_state.p + k, sizeof r, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (r.status == BLK_OK && r.btype != 0) n_extra++;   // the slot stays in use
        }
        //  a block the end of the input cuts in half is INCOMPLETE even when its scan reports an EndOfBlock:
        // the last lane decodes a few symbols past the input (the bit source repeats the last dword there) and one
        // of them may read as EndOfBlock — end_bit then lies behind the input and n_out counts garbage symbols
        if (r.status == BLK_OK && r.end_bit > n * 8) r.status = BLK_NO_EOB;
        if (r.status != BLK_OK || r.end_bit <= ch.pos) { ch.front_bad = ch.emit.empty() && r.status == BLK_BAD; break; }
        if (m.partial && ch.total + r.n_out > m.cap) { mr.need_cap = ch.emit.empty(); break; }   // (the next window takes it)
        BlkEmit &e = ch.push(r, k, m.hist);      // (hist = 0: a member starts with an empty window)
        if (k < nj && stored[k]) { e.placed = 1; e.temp_off = bj[k].temp_off; e.cap = bj[k].cap; ch.n_placed++; }
        ch.close_block(r);
        if (ch.ok) break;
    }
    // a window: the blocks in front of the first incomplete one are what this call delivers
    if (m.partial && !ch.ok && !ch.emit.empty()) ch.ok = true;
    return LFX_OK;
}

void debug_emit_stats(Ctx *c, uint32_t ne, uint32_t fl, const uint64_t *dbgbuf) {
    fprintf(stderr, "[lfx]  emit flags=%u\n", fl);
    std::vector<BlkUnits> uv(ne);
    (void)hipMemcpy(uv.data(), c->d_hist.p, sizeof(BlkUnits) * ne, hipMemcpyDeviceToHost);
    for (uint32_t u = 0; u < 3 && u < ne; u++)
        fprintf(stderr, "[lfx]  K2 block %u: units=%u hdr=%u decode=%u cut=%u select=%u\n", u, uv[u].n, uv[u].cyc[0],
                uv[u].cyc[1], uv[u].cyc[2], uv[u].cyc[3]);
    std::vector<uint64_t> dv(64ull * ne);
    (void)hipMemcpy(dv.data(), dbgbuf, 64ull * 8 * ne, hipMemcpyDeviceToHost);
    uint32_t nunits = 0;
    uint64_t maxcyc = 0, tmin = ~0ull, tmax = 0;
    for (uint32_t u = 0; u < 8 * ne; u++) {
        if (!dv[u * 8 + 1]) continue;
        nunits++;
        maxcyc = std::max(maxcyc, dv[u * 8]);
        tmin = std::min(tmin, dv[u * 8 + 6]); tmax = std::max(tmax, dv[u * 8 + 6]);
    }
    fprintf(stderr, "[lfx]  K3: units=%u max_cycles=%llu end-time spread=%.1f us (100 MHz clock)\n", nunits,
            (unsigned long long)maxcyc, (double)(tmax - tmin) / 100.0);
    for (uint32_t u = 0; u < 8 && u < 8 * ne; u++)
        fprintf(stderr, "[lfx]  K3 unit %u: cycles=%llu batches=%llu nseq=%llu seq_cycles=%llu codes=%llu bytes=%llu\n", u,
                (unsigned long long)dv[u * 8], (unsigned long long)dv[u * 8 + 1], (unsigned long long)dv[u * 8 + 2],
                (unsigned long long)dv[u * 8 + 3], (unsigned long long)dv[u * 8 + 4], (unsigned long long)dv[u * 8 + 5]);
}

// Blocks read the output of earlier blocks (streams of other encoders; the reference's own
// blocks never do).  Marker-based materialisation: every block, cut into units at slice
// boundaries, is materialised at once into 16-bit symbols (a byte, or a reference into the
// unknown 32 KiB in front of the unit); one workgroup then walks the units in order resolving
// only each unit's last 32 KiB; a last pass replaces every marker.
int materialise_markers(const Member &m, const Chain &ch, const BlkEmit *d_emit) {
    Ctx *c = m.c;
    hipStream_t st = c->stream;
    const uint32_t ne = (uint32_t)ch.emit.size();
    int rc;
    // (a later window of a member: the 32 KiB in front of d_out hold the member's earlier output — the markers of
    //  the first unit resolve through them; bytes in front of what `hist` covers are never looked up: a reference
    //  that far back raised flag 1 in the emit step)
    const uint8_t *init_win = m.hist_win ? m.hist_win : m.hist ? m.d_out - MAX_WINDOW : nullptr;
    std::vector<BlkUnits> uv(ne);
    HIP_TRY(hipMemcpyAsync(uv.data(), c->d_hist.p, sizeof(BlkUnits) * ne, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<SymUnit> su;
    const uint64_t max_len = sym_units(ch.emit, uv, su);
    const uint32_t nsu = (uint32_t)su.size();
    if ((rc = c->d_dec_sym.reserve(2 * std::max<uint64_t>(ch.total, 1)))) return rc;
    if ((rc = c->d_dec_win.reserve(32768ull * std::max<uint32_t>(nsu, 1) + sizeof(SymUnit) * (size_t)nsu + 64))) return rc;
    uint8_t *d_win = (uint8_t *)c->d_dec_win.p;
    SymUnit *d_su = (SymUnit *)(d_win + 32768ull * std::max<uint32_t>(nsu, 1));
    HIP_TRY(hipMemcpyAsync(d_su, su.data(), sizeof(SymUnit) * nsu, hipMemcpyHostToDevice, st));
    LAUNCH_TRY(launch_blk_materialize_sym(st, m.d_in, d_emit, ne, (const BlkUnits *)c->d_hist.p,
                                          (const uint32_t *)c->d_codes.p, (uint16_t *)c->d_dec_sym.p,
                                          nsu <= (uint32_t)std::max(c->n_cu, 1)));
    c->phase("lz77_sym");
    if (nsu >= 16) {   // blocked parallel prefix over the units (groups of about sqrt(nsu))
        if ((rc = c->d_dec_maps.reserve(window_prefix_scratch_bytes(nsu)))) return rc;
        LAUNCH_TRY(launch_window_prefix(st, (const uint16_t *)c->d_dec_sym.p, d_su, nsu, c->d_dec_maps.p, d_win, init_win));
    } else LAUNCH_TRY(launch_window_chain(st, (const uint16_t *)c->d_dec_sym.p, d_su, nsu, d_win, init_win));
    c->phase("win_chain");
    LAUNCH_TRY(launch_sym_substitute(st, (const uint16_t *)c->d_dec_sym.p, d_su, nsu, d_win, m.d_out, max_len, init_win));
    HIP_TRY(hipStreamSynchronize(st));
    c->phase("substitute");
    if (c->diag.debug) fprintf(stderr, "[lfx]  cross-block references: %u blocks, %u units through markers\n", ne, nsu);
    return LFX_OK;
}

// ---- K2 + K3: validated lanes emit codes, one wavefront per block materialises them.  done: the member is decoded
//      (mr filled); otherwise a back-reference reaches in front of the member and the serial walk gives the verdict.
int emit_and_materialise(const Member &m, const Chain &ch, MemberResult &mr, bool &done) {
    Ctx *c = m.c;
    hipStream_t st = c->stream;
    const uint8_t *d_in = m.d_in;
    const uint32_t ne = (uint32_t)ch.emit.size();
    const uint64_t total = ch.total;
    int rc;
    uint64_t *dbgbuf = nullptr;
    if (c->diag.debug) {
        if ((rc = c->d_ck.reserve(64ull * 8 * ne + 64))) return rc;
        dbgbuf = (uint64_t *)c->d_ck.p;
        HIP_TRY(hipMemsetAsync(dbgbuf, 0, 64ull * 8 * ne, st));
    }
    EmitBufs eb;
    const uint32_t free_shift = ch.pieces && ch.units_per_piece ? 20 : marker_unit_shift(total, c->n_cu);
    if ((rc = emit_codes(c, d_in, m.n, ch.emit, ch.total_codes, ch.n_placed, free_shift, ch.scan_small && !ch.pieces, eb))) return rc;
    // a huge block (a schedule-S1 stream is ONE block) rarely has enough legal cuts: it goes straight to
    // the marker path, which may cut anywhere
    bool giant = ch.pieces_multi;   // (pieces of one block read each other's output; blocks scanned in ONE piece each are ordinary blocks)
    for (const BlkEmit &e : ch.emit) giant |= e.n_out >= (8ull << 20);   // (a block that big has too few legal cuts for K3's resident units)
    // small blocks smell of another encoder (zlib cuts every ~50-100 KiB of output; the reference at
    // block_size = 1 MiB): look at the emit flags BEFORE materialising, so that a stream which needs
    // the marker path does not pay for a discarded direct pass (costs one round trip otherwise saved)
    const bool probe = !giant && total / ne < (256u << 10);
    uint32_t fl = 0;
    if (probe) {
        HIP_TRY(c->small_down(&fl, eb.d_flags, 4, st));
        HIP_TRY(c->small_sync(st));
    }
    const uint64_t end_bit = ch.pos == m.stop_bit ? ch.pos : ch.last_end, end_byte = end_bit / 8 + ((end_bit & 7) ? 1 : 0);
    bool ck_spec = false;
    if (!giant && !(probe && fl == 2)) {
        LAUNCH_TRY(launch_blk_materialize(st, d_in, eb.d_emit, ne, (const BlkLanes *)c->d_dec_blocks.p,
                                          (const BlkUnits *)c->d_hist.p, (const uint32_t *)c->d_codes.p, m.d_out, dbgbuf));
        if (mr.ck_mode && total && !m.partial && !c->diag.debug && end_byte + mr.trailer_len <= m.n) {
            // the checksum of what is being materialised, and the trailer bytes, behind the same synchronisation
            c->phase("lz77_copy");
            const uint64_t nspans = ck_nspans(total);
            if ((rc = c->d_ck.reserve(12 * nspans))) return rc;
            if ((rc = c->d_res.reserve(256))) return rc;
            uint32_t *ck = (uint32_t *)c->d_ck.p;
            LAUNCH_TRY(launch_checksum(st, m.d_out, total, ck, ck + nspans, ck + 2 * nspans, (EncodeResult *)c->d_res.p, mr.ck_mode));
            HIP_TRY(hipMemcpyAsync(c->h_res, c->d_res.p, sizeof(EncodeResult), hipMemcpyDeviceToHost, st));
            if (mr.trailer_len) HIP_TRY(hipMemcpyAsync((uint8_t *)c->h_res + 256, d_in + end_byte, mr.trailer_len, hipMemcpyDeviceToHost, st));
            ck_spec = true;
        }
    }
    HIP_TRY(c->small_down(&fl, eb.d_flags, 4, st));
    HIP_TRY(c->small_sync(st));
    if (ck_spec && fl == 0) {
        const EncodeResult er = *(EncodeResult *)c->h_res;
        mr.ck_done = true; mr.crc32 = er.crc32; mr.adler32 = er.adler32;
        memcpy(mr.trailer, (uint8_t *)c->h_res + 256, mr.trailer_len);
        c->phase("checksum");
    }
    if (giant && !(fl & 1)) fl = 2;
    else if (giant) {   // (an invalid reference: materialise normally / fall back)
        LAUNCH_TRY(launch_blk_materialize(st, d_in, eb.d_emit, ne, (const BlkLanes *)c->d_dec_blocks.p,
                                          (const BlkUnits *)c->d_hist.p, (const uint32_t *)c->d_codes.p, m.d_out, dbgbuf));
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (!ck_spec) c->phase("lz77_copy");
    if (c->diag.debug) debug_emit_stats(c, ne, fl, dbgbuf);
    if (fl == 2) {
        if ((rc = materialise_markers(m, ch, eb.d_emit))) return rc;
        fl = 0;
    }
    if (fl != 0) return LFX_OK;      // a back-reference reached before its member's first byte
    // (an index build: the chain's block starts and its large blocks' lanes, before a later step reuses the slots)
    if (c->idx && (rc = idx_record_chain(c, ch.emit.data(), ne, (const BlkLanes *)c->d_dec_blocks.p, c->idx->bit_base,
                                         c->idx->out_base, true)))
        return rc;
    mr.status = LFX_OK;
    mr.out_len = total;
    mr.blk_out_start = total;
    mr.end_byte = end_byte;
    mr.end_bit = end_bit;
    mr.final_seen = ch.final;
    done = true;
    return LFX_OK;
}

// ---- serial walk of the whole stream by one wavefront (exact error / partial-output semantics)
int serial_walk(const Member &m, MemberResult &mr) {
    Ctx *c = m.c;
    const uint64_t n = m.n;
    InflateJob j{};
    j.in_off = 0; j.in_len = n; j.start_bit = m.first_bit;
    j.out_off = 0; j.out_cap = m.cap; j.hist_avail = m.hist; j.flags = 0;
    j.dict_len = m.hist_win ? (uint32_t)m.hist : 0;      // (a detached history is a dictionary's tail: the dictionary instance)
    j.stop_bit = m.stop_bit == ~0ull ? 0 : m.stop_bit;   // (small or irregular shards: the exact walk, ended at the shard's last bit)
    std::vector<InflateResult> res;
    int rc;
    if ((rc = run_jobs(c, m.d_in, m.d_out, {j}, res, m.hist_win ? m.hist_win + MAX_WINDOW : nullptr))) return rc;
    c->phase("serial");
    InflateResult &r = res[0];
    // an unassigned code in a whole member: `consumed` is what the reference's reader has pulled by then, as in the size call
    // (end_bit counts the 16 bits the reference skips without reading them)
    uint64_t huff_used = ~0ull;
    if (huff_verdict(r) && m.stop_bit == ~0ull && !m.partial && (m.hist == 0 || m.hist_win)) {
        std::vector<uint64_t> used;
        if ((rc = huff_consumed(c, m.d_in, {HuffProbe{0, n, r}}, used))) return rc;
        huff_used = used[0];
    }
    if (m.stop_bit != ~0ull && r.status == 0 && (r.final_seen || r.end_bit != m.stop_bit)) {
        // a shard without the BFINAL block must end exactly where the next shard starts
        r.status = 1; r.err = ERR_HUFF; r.a0 = r.a1 = 0;
    }
    mr.status = map_status(r.status);
    mr.out_len = r.out_len;
    mr.blk_out_start = r.status ? r.blk_out_start : r.out_len;
    mr.end_byte = huff_used != ~0ull ? huff_used : std::min<uint64_t>((r.end_bit + 7) / 8, n);
    mr.end_bit = r.end_bit;
    mr.final_seen = r.status == 0 && r.final_seen;
    mr.msg = format_error(r.err, r.a0, r.a1);
    // a window: running out of input (or of output capacity) inside a block is not a verdict — deliver the blocks in
    // front of it and let the caller come back with more.  An error in the very last bits of the window may be an
    // artefact of the cut (the reference's BitReader reads zeros past the end before it reports UnexpectedEof) and
    // is treated the same way; the caller repeats it without `partial` once the reader has ended.
    if (m.partial && r.status != 0 && (r.status == 2 || r.status == 3 || r.end_bit + 64 >= n * 8)) {
        mr.status = LFX_OK;
        mr.out_len = mr.blk_out_start = r.blk_out_start;
        mr.end_bit = r.blk_start_bit;
        mr.end_byte = r.blk_start_bit / 8;
        mr.final_seen = false;
        mr.need_cap = r.status == 3 && r.blk_out_start == 0;
        mr.msg.clear();
    }
    return LFX_OK;
}

}  // namespace

int inflate_member(Ctx *c, const uint8_t *d_in, uint64_t n, uint64_t off0, uint8_t *d_out, uint64_t cap, MemberResult &mr,
                   uint64_t start_bit0, uint64_t stop_bit, bool partial, uint64_t hist, const uint8_t *hist_win) {
    const Member m{c, d_in, n, off0, d_out, cap, start_bit0 == ~0ull ? off0 * 8 : start_bit0, stop_bit, partial, hist, hist ? hist_win : nullptr,
                   n > off0 ? n - off0 : 0};
    mr.end_bit = m.first_bit;
    c->pin_reset();        // (the page-locked slots of the small transfers, lfx_ctx.h: nothing of an earlier member is in flight)
    bool done = false;
    // (below a few KiB the exact serial kernel is faster than the parallel path's fixed cost of about 2 ms; measured:
    //  a 32 KiB stream takes 17 ms on the serial kernel)
    if (m.comp >= (4u << 10)) {
        int rc;
        std::vector<uint64_t> starts;
        Found fd;
        const bool may_piece = stop_bit == ~0ull && !partial && !c->diag.no_pieces;
        // A small stream (round 4) does not start with the finder (0.23 ms of fixed cost): reference-made streams of this
        // size are one block plus the empty final one, which the piece walk goes through from the known first block in two
        // steps.  A stream that turns out to have many blocks (another encoder's) gets the finder after all.
        // (measured, profiles/r04_small_sizes.json: every dependent block step costs about 0.2 ms — header parse and table
        //  build of one workgroup — so the walk pays for up to three blocks: streams below 1.5 MiB)
        const bool small_first = m.comp < (1536u << 10) && may_piece;
        if (small_first) starts.push_back(m.first_bit);
        else if ((rc = find_starts(m, starts, fd))) return rc;
        if (!fd.overflow) {
            Chain ch(m.first_bit);
            const uint32_t nc = (uint32_t)starts.size();
            const bool giant_blocks = nc <= 8 && m.comp / nc >= (2u << 20);     // (schedule S1: the block-by-block piece walk)
            if (may_piece && !small_first && !giant_blocks && nc >= 2 && nc <= PIECE_RANGES_MAX && m.comp / nc >= (128u << 10) &&
                (rc = pieces_over_ranges(m, starts, ch)))
                return rc;
            if (!ch.pieces && may_piece && (small_first || giant_blocks) && (rc = pieces_block_walk(m, small_first, starts, fd, ch))) return rc;
            if (!ch.pieces && !fd.overflow && (rc = block_scan(m, starts, fd.n1, ch, mr))) return rc;
            if (c->diag.debug) fprintf(stderr, "[lfx]  chain ok=%d blocks=%zu pos=%llu total=%llu on_demand=%u\n", (int)ch.ok, ch.emit.size(), (unsigned long long)ch.pos, (unsigned long long)ch.total, ch.n_on_demand);
            if (partial && ch.emit.empty() && !ch.front_bad) {
                // a window without one complete block (or whose first block does not fit `cap`): nothing to deliver — the
                // caller widens the window (the exact serial walk of the whole window would only find out the same, slowly).
                // A first block that does not even scan is different: the serial walk below says at once whether the
                // stream is damaged there (a verdict) or merely cut (nothing to deliver).
                mr.status = LFX_OK; mr.out_len = 0; mr.blk_out_start = 0; mr.final_seen = false;
                mr.end_bit = m.first_bit; mr.end_byte = m.first_bit / 8;
                return LFX_OK;
            }
            if (ch.ok && ch.total <= cap && (rc = emit_and_materialise(m, ch, mr, done))) return rc;
        }
    }
    if (done) return LFX_OK;
    if (c->diag.no_serial) { c->set_error("serial fallback disabled (LFX_NO_SERIAL)"); return LFX_E_UNSUPPORTED; }
    return serial_walk(m, mr);
}

}  // namespace lfx
