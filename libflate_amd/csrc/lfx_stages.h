// lfx_stages.h — the host arithmetic of the member decode's stages (lfx_member.cpp, lfx_decode_range_*): how a range is cut
// into pieces, which scan ranges get an alternative job, where the storing scan's lane regions lie, which symbol units the
// marker path walks.  Pure index arithmetic on the descriptors of lfx_blk.h — no HIP call, no context: compiles with a plain
// host compiler (tests/c/plan_stages.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "lfx_blk.h"

namespace lfx {

// most candidate ranges that are scanned in pieces at once (measured, profiles/r04_small_sizes.json: at 64 blocks the marker
// path's fixed costs outweigh what the scan and the emit kernel gain; the sweep up to 100: HISTORY.md)
constexpr uint32_t PIECE_RANGES_MAX = 100;

// ---- pieces
// Piece size for `span_bits` of stream that should become about `want` pieces: between 256 Kbit and 4 Mbit, a multiple of 64.
inline uint64_t piece_bits(uint64_t span_bits, uint64_t want) {
    return std::min<uint64_t>(4ull << 20, std::max<uint64_t>(256ull << 10, (span_bits / want + 63) & ~63ull));
}
// warm-up in front of a piece: ONE lane decodes it, 0.2 us per symbol on an otherwise idle CU — 8 Kbit are 550
// symbols, 115 us, most of a small stream's scan step (round 4, profiles/r04_small_sizes.json).  A speculative
// decode is in step within a few dozen symbols; small pieces get 2 Kbit.  (A piece whose warm-up did not get in
// step is rejected by the chain check of its stage, and the stream takes the one-workgroup-per-block path.)
inline uint64_t piece_overlap(uint64_t piece) { return piece <= (1ull << 20) ? 2048 : 8192; }

// the pieces of one range [s0, s1), scanned with the tables of the block whose header is at s0: the range split EVENLY (a
// block of 4.7 Mbit in pieces of 4 Mbit is a long piece and a short one: the symbol kernel's time is that of its largest unit)
inline void add_pieces(std::vector<BlkJob> &jobs, uint64_t s0, uint64_t s1, uint64_t piece, uint64_t overlap) {
    const uint64_t len = s1 - s0;
    const uint64_t np0 = std::max<uint64_t>((len + piece - 1) / piece, 1);
    const uint64_t pb = std::max<uint64_t>(((len + np0 - 1) / np0 + 63) & ~63ull, 64);     // this block's piece
    const uint32_t np = (uint32_t)std::max<uint64_t>((len + pb - 1) / pb, 1);
    for (uint32_t q = 0; q < np; q++) {
        const uint64_t lo = s0 + q * pb;
        jobs.push_back(BlkJob{s0, std::min(lo + pb, s1), q ? lo : 0, q ? lo - overlap : 0, 1u, 0u});
    }
}
// the pieces of [pos, end_bits) at the full piece size (the block-by-block walk: the block at pos ends somewhere in there)
inline void add_fixed_pieces(std::vector<BlkJob> &jobs, uint64_t pos, uint64_t end_bits, uint64_t piece, uint64_t overlap) {
    const uint32_t np = (uint32_t)((end_bits - pos + piece - 1) / piece);
    for (uint32_t q = 0; q < np; q++) {
        const uint64_t lo = pos + q * piece;
        jobs.push_back(BlkJob{pos, std::min(lo + piece, end_bits), q ? lo : 0, q ? lo - overlap : 0, 1u, 0u});
    }
}

// ---- alternative jobs of the block scan
// bj[0, nc) are the candidates' ranges [starts[i], starts[i + 1]).  A false candidate inside a block cuts that block's range
// in two, and the first part then has no end-of-block.  Ranges much shorter than the median are the suspects: the candidate
// in front of each (and the suspect itself) also gets a job that ignores one candidate, in the same launch; what is still
// unresolved afterwards goes through the widening rescans.  Returns alt[i] = index of candidate i's wider job in bj, or -1.
inline std::vector<int32_t> add_alt_jobs(std::vector<BlkJob> &bj, const std::vector<uint64_t> &starts, uint64_t end_bits, uint64_t comp) {
    const uint32_t nc = (uint32_t)starts.size();
    auto start_at = [&](uint32_t i) { return i < nc ? starts[i] : end_bits; };
    std::vector<int32_t> alt(nc, -1);
    std::vector<uint64_t> len(nc);
    for (uint32_t i = 0; i < nc; i++) len[i] = bj[i].end_bit - bj[i].start_bit;
    std::vector<uint64_t> sorted = len;
    std::nth_element(sorted.begin(), sorted.begin() + nc / 2, sorted.end());
    const uint64_t median = sorted[nc / 2], thresh = median / 5 * 3;
    const uint32_t max_extra = nc / 4 + 4;
    for (uint32_t i = 0; i + 1 < nc && bj.size() - nc < max_extra; i++) {
        if (len[i] >= thresh && len[i + 1] >= thresh) continue;
        // (the LAST range is short because the stream ends there — a member's final block is often tiny or empty —
        //  not because a false candidate cut it: a full-size alternative job for it is a second workgroup on one
        //  CU, and that CU decides the kernel's duration: 0.74 against 0.62 ms at 256 blocks on 256 CUs)
        if (i + 2 == nc && len[i] >= thresh) continue;
        // a block cut in two is about one block long when put together; anything much longer
        // would only be a slow job that decides the kernel's duration
        if (len[i] + len[i + 1] > median + median / 4) continue;
        alt[i] = (int32_t)bj.size();
        bj.push_back(BlkJob{starts[i], start_at(i + 2)});
    }
    // few candidates = few, huge blocks (schedule S1: one): a false candidate would cost a full rescan of
    // such a block, so the known first block also gets a job that runs to the end of the stream
    if (nc > 1 && nc <= 8 && alt[0] < 0 && comp / nc >= (2u << 20)) {
        alt[0] = (int32_t)bj.size();
        bj.push_back(BlkJob{starts[0], end_bits});
    }
    return alt;
}

// ---- block rounds (scan_round / emit_round: one block per live stream and round)
constexpr uint32_t BLOCK_ROUNDS = 4;                 // blocks of a stream the batch's fast path decodes and a members walk follows ...
constexpr uint64_t MEMBER_WALK_BYTES = 4ull << 20;   // ... and input bytes that walk covers; a member beyond either is "long"
// The byte the blocks of the member at candidate cand[k], whose DEFLATE data starts at `data`, must end in front of: the next
// candidate behind `data` (a member's trailer lies in front of the next member's header), at most MEMBER_WALK_BYTES from the
// member's start, inside d_in[0, n).  A limit <= data: nothing to walk.
inline uint64_t member_walk_limit(const std::vector<uint64_t> &cand, size_t k, uint64_t data, uint64_t n) {
    uint64_t lim = std::min<uint64_t>(n, cand[k] + MEMBER_WALK_BYTES);
    const auto nx = std::upper_bound(cand.begin(), cand.end(), data);
    if (nx != cand.end() && *nx < lim) lim = *nx;
    return lim;
}

// ---- the storing scan's lane regions
// Every lane of job j stores its code words at temp + temp_off + lane * cap (dwords): cap = half a code per bit of the slice +
// a head's worth + slack (a slice whose codes average less than two bits overflows, is flagged, and takes the emit kernel);
// tight: sized for 16 bits a code (LFX_STORE_TIGHT: lanes overflow, blocks fall back).  Returns the dwords all regions take.
inline uint64_t plan_store_regions(BlkJob *bj, uint32_t nj, bool tight) {
    uint64_t off = 0;
    for (uint32_t j = 0; j < nj; j++) {
        const uint64_t bits = bj[j].end_bit > bj[j].start_bit ? bj[j].end_bit - bj[j].start_bit : 0;
        const uint64_t slice = std::max<uint64_t>((bits + 1023) / 1024, 128);
        const uint64_t cap = (slice / (tight ? 16 : 2) + 448 + 64 + 3) & ~3ull;   // (448 = SCAN_HEADCAP, lfx_inflate_fast.hip)
        bj[j].temp_off = off;
        bj[j].cap = (uint32_t)cap;
        off += 1024 * cap;
    }
    return off;
}
inline void clear_store_regions(BlkJob *bj, uint32_t nj) {
    for (uint32_t j = 0; j < nj; j++) { bj[j].temp_off = 0; bj[j].cap = 0; }
}

// ---- emit jobs and units
// The emit job of a scanned block (or piece) `r` whose header is at start_bit: scan slot, first output byte and code slot,
// and the bytes of the member in front of it (they bound its back-references).
inline BlkEmit blk_emit_of(const BlkInfo &r, uint64_t start_bit, uint32_t slot, uint64_t out_off, uint64_t code_off, uint64_t hist) {
    BlkEmit e{};
    e.start_bit = start_bit; e.data_bit = r.data_bit; e.code_off = code_off; e.out_off = out_off;
    e.n_out = r.n_out; e.n_codes = r.n_codes; e.nlanes = r.nlanes; e.btype = r.btype; e.cand = slot;
    e.hist = hist;
    e.end_limit = r.status == BLK_NO_EOB ? r.end_bit : 0;   // an open piece ends where its last lane stopped
    return e;
}
// K3 keeps four units resident per CU (LDS): size the units so that all of them are resident at once
inline uint32_t emit_unit_target(uint64_t total_codes, int n_cu) {
    const uint64_t slots = 4ull * (uint64_t)std::max(n_cu, 1);
    return (uint32_t)std::min<uint64_t>((total_codes + slots - 1) / slots + 1, 0x7FFFFFFFu);
}
// emit_round's d_dec_tmp for `ne` emit jobs: 64 flag bytes, a flag per job, padding to 8, the jobs (byte offsets)
struct EmitTmp { uint64_t flags, job_flags, jobs, total; };
inline EmitTmp emit_tmp_layout(uint32_t ne) {
    EmitTmp t{0, 64, (64 + 4ull * ne + 7) & ~7ull, 0};
    t.total = t.jobs + sizeof(BlkEmit) * (uint64_t)ne;
    return t;
}
// marker units (used only when blocks read earlier blocks): two symbol units are resident per CU and the
// symbol kernel's time does not depend on the unit size as long as every slot has a unit, while every
// unit costs the window resolution 32 Ki lookups (256 MiB: 128 KiB units 1.31 + 0.74 ms, 512 KiB units
// 0.59 + 0.64 ms for window resolution + substitution).  Units of 2^shift output bytes.
inline uint32_t marker_unit_shift(uint64_t total, int n_cu) {
    uint32_t free_shift = 15;
    while (free_shift < 20 && (total >> (free_shift + 1)) >= 2ull * (uint64_t)std::max(n_cu, 1)) free_shift++;
    return free_shift;
}
// the marker path's units in stream order, from the free cuts the emit step left per block; returns the longest unit
inline uint64_t sym_units(const std::vector<BlkEmit> &emit, const std::vector<BlkUnits> &uv, std::vector<SymUnit> &su) {
    uint64_t max_len = 0;
    su.clear();
    for (size_t q = 0; q < emit.size(); q++)
        for (uint32_t b = 0; b < uv[q].fn && b < MAX_FREE_UNITS; b++) {
            const uint64_t len = uv[q].fout0[b + 1] - uv[q].fout0[b];
            if (!len) continue;
            su.push_back(SymUnit{emit[q].out_off + uv[q].fout0[b], len});
            max_len = std::max(max_len, len);
        }
    return max_len;
}

}  // namespace lfx
