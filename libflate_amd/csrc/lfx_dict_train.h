// lfx_dict_train.h — lfx_dict_train_device / _host (include/lfx.h "training a preset dictionary"): a simplified
// FASTCOVER over sample records.  What the HIP kernels (lfx_dict_train.hip), the entry points and the host test
// (tests/c/dict_train.cpp) share, stated ONCE: the constants, the hash, the argument checks with the record table they
// leave, the places of the call's scratch, the cursor that finds a position's record through the per-tile index, the lane's
// walk over consecutive positions, and the pick's key.  dtrain_host_walk runs the kernels' steps on the host with the same
// cursor and the same lane walk — the test holds it against tests/dict_train_model.py.  Nothing here needs a device.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/lfx.h"
#include "lfx_common.h"

namespace lfx {

constexpr uint32_t DTRAIN_D = 8, DTRAIN_F = 20;                 // d-mer bytes, bits of the counter index
constexpr uint64_t DTRAIN_PRIME = 0x9E3779B185EBCA87ull;
constexpr uint64_t DTRAIN_MAX_N = 1ull << 31;                   // positions of one call: every position fits 32 bits
constexpr uint32_t DTRAIN_MIN_DICT = 64, DTRAIN_MAX_DICT = 32768, DTRAIN_MIN_SEG = 16, DTRAIN_DEFAULT_SEG = 128;
constexpr uint32_t DTRAIN_MAX_PICKS = DTRAIN_MAX_DICT / DTRAIN_MIN_SEG;   // 2048: what the gather kernel sorts in LDS
constexpr uint32_t DTRAIN_TILE = 256;         // positions per entry of the record index
constexpr uint32_t DTRAIN_WG = 256;           // lanes of every kernel's workgroup
constexpr uint32_t DTRAIN_PPL = 8;            // count kernel: consecutive positions of a lane (two 8-byte loads; at most 8)
constexpr uint32_t DTRAIN_SPL = 4;            // epoch step: consecutive positions of a lane
constexpr uint32_t DTRAIN_CHUNK = 4096;       // epoch step: candidates of one workgroup pass
constexpr uint32_t DTRAIN_STEP_GRID = 512;    // epoch step: workgroups at most (each owns CHUNK + k prefix words)
constexpr uint32_t DTRAIN_COUNT_GRID = 1024;  // count kernel: workgroups at most (grid-stride behind them)

LFX_HD inline uint32_t dtrain_hash(uint64_t v) { return (uint32_t)((v * DTRAIN_PRIME) >> (64 - DTRAIN_F)); }
LFX_HD inline uint64_t dtrain_load8(const uint8_t *a) {
    uint64_t v;
    memcpy(&v, a, 8);
    return v;
}
// epoch e of E owns [dtrain_epoch_lo(e), dtrain_epoch_lo(e + 1))
LFX_HD inline uint32_t dtrain_epoch_lo(uint32_t e, uint32_t epochs, uint64_t n) { return (uint32_t)((uint64_t)e * n / epochs); }
// the word the candidates of an epoch fold into by a 64-bit maximum: the highest score, among equal scores the lowest
// position; 0 = no pick (a score of 0 never enters)
LFX_HD inline uint64_t dtrain_pick_key(uint64_t sum, uint32_t pos_in_epoch) {
    const uint64_t score = sum > 0xFFFFFFFFull ? 0xFFFFFFFFull : sum;
    return score << 32 | (uint32_t)~pos_in_epoch;
}
LFX_HD inline uint32_t dtrain_pick_pos(uint64_t key) { return ~(uint32_t)key; }
// the gather's order: score ascending, among equal scores the earlier epoch later
LFX_HD inline uint64_t dtrain_sort_key(uint64_t pick, uint32_t epoch) { return (pick & 0xFFFFFFFF00000000ull) | (uint32_t)~epoch; }

// ---- the arguments, and the record table the kernels read: empty records dropped, pos[i] = the first position of record i,
// pos[nrec] = N, off[i] = its first byte in the samples buffer
struct DtrainPlan {
    uint32_t k = 0, epochs = 0;
    uint64_t n = 0, extent_lo = 0, extent_hi = 0;      // positions; the bytes [extent_lo, extent_hi) of the buffer hold every record
    std::vector<uint32_t> pos;
    std::vector<uint64_t> off;
    uint32_t nrec() const { return (uint32_t)off.size(); }
};
// → LFX_OK, LFX_E_ARG or LFX_E_NOSPACE; *why: the reason, for the context's error text
inline int dtrain_check(uint32_t count, const uint64_t *off, const uint64_t *len, uint32_t dict_size, uint32_t segment, const void *dict,
                        uint64_t cap, DtrainPlan *pl, const char **why) {
    const uint32_t k = segment ? segment : DTRAIN_DEFAULT_SEG;
    *why = "";
    if (dict_size < DTRAIN_MIN_DICT || dict_size > DTRAIN_MAX_DICT) { *why = "dict_size: 64..32768"; return LFX_E_ARG; }
    if (k < DTRAIN_MIN_SEG || k > dict_size) { *why = "segment: 16..dict_size"; return LFX_E_ARG; }
    if (count && (!off || !len)) { *why = "off, len: NULL with records"; return LFX_E_ARG; }
    pl->k = k;
    pl->epochs = dict_size / k;
    pl->n = 0;
    pl->pos.clear();
    pl->off.clear();
    uint64_t prev_end = 0;
    for (uint32_t i = 0; i < count; i++) {
        if (off[i] + len[i] < off[i]) { *why = "off + len exceeds 64 bits"; return LFX_E_ARG; }
        if (i && off[i] < prev_end) { *why = "records must not overlap and must come in ascending order of off"; return LFX_E_ARG; }
        prev_end = off[i] + len[i];
        if (!len[i]) continue;
        if (len[i] > DTRAIN_MAX_N || pl->n + len[i] > DTRAIN_MAX_N) { *why = "more than 2^31 sample bytes"; return LFX_E_ARG; }
        if (pl->off.empty()) pl->extent_lo = off[i];
        pl->extent_hi = prev_end;
        pl->pos.push_back((uint32_t)pl->n);
        pl->off.push_back(off[i]);
        pl->n += len[i];
    }
    pl->pos.push_back((uint32_t)pl->n);
    if (cap < dict_size) { *why = "cap < dict_size"; return LFX_E_NOSPACE; }
    if (pl->n && !dict) { *why = "the dictionary buffer is NULL"; return LFX_E_ARG; }
    return LFX_OK;
}

// ---- the call's scratch, in bytes from its base, every region 256-byte aligned: the counters, one pick word per epoch and
// the dictionary's length behind them, the record table, the per-tile record index, the step's prefix words
struct DtrainScratch {
    uint64_t freq, slots, out_len, pos, off, tile_rec, prefix, bytes;
    uint32_t ntiles, step_grid;
    uint64_t prefix_words;       // per workgroup of the step
};
LFX_HD inline uint64_t dtrain_up256(uint64_t x) { return (x + 255) & ~255ull; }
LFX_HD inline uint32_t dtrain_ntiles(uint64_t n) { return (uint32_t)((n + DTRAIN_TILE - 1) / DTRAIN_TILE); }
// the longest epoch has n / epochs + 1 positions at most
LFX_HD inline uint32_t dtrain_step_grid(uint64_t n, uint32_t epochs) {
    const uint64_t chunks = (n / epochs + 1 + DTRAIN_CHUNK - 1) / DTRAIN_CHUNK;
    return (uint32_t)(chunks < DTRAIN_STEP_GRID ? chunks : DTRAIN_STEP_GRID);
}
LFX_HD inline DtrainScratch dtrain_scratch(uint64_t n, uint32_t nrec, uint32_t epochs, uint32_t k) {
    DtrainScratch s;
    s.ntiles = dtrain_ntiles(n);
    s.step_grid = dtrain_step_grid(n, epochs);
    s.prefix_words = (uint64_t)DTRAIN_CHUNK + k;
    s.freq = 0;
    s.slots = s.freq + dtrain_up256(4ull << DTRAIN_F);
    s.out_len = s.slots + 8ull * epochs;                // (behind the slots: one fill clears both)
    s.pos = dtrain_up256(s.out_len + 8);
    s.off = dtrain_up256(s.pos + 4ull * (nrec + 1));
    s.tile_rec = dtrain_up256(s.off + 8ull * nrec);
    s.prefix = dtrain_up256(s.tile_rec + 4ull * s.ntiles);
    s.bytes = s.prefix + 8ull * s.prefix_words * s.step_grid;
    return s;
}

// ---- a position's record.  tile_rec[t] = the record that holds position t * DTRAIN_TILE; from there a cursor walks forward.
struct DtrainRecs {
    const uint32_t *pos;
    const uint64_t *off;
    const uint32_t *tile_rec;
    const uint8_t *base;
    uint32_t nrec;
    uint32_t n;             // (2^31 at most)
};
// the record index's entry: the last record that starts at or in front of p (records are not empty: exactly one holds p)
LFX_HD inline uint32_t dtrain_owner_search(const uint32_t *pos, uint32_t nrec, uint32_t p) {
    uint32_t lo = 0, hi = nrec;          // pos[lo] <= p < pos[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (pos[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}
struct DtrainCursor {
    uint32_t r, end;        // the record, and its end in positions
    LFX_HD void seek(const DtrainRecs &R, uint32_t p) {
        r = R.tile_rec[p / DTRAIN_TILE];
        end = R.pos[r + 1];
        advance(R, p);
    }
    LFX_HD void advance(const DtrainRecs &R, uint32_t p) {      // p < n: pos[nrec] = n ends the walk
        while (end <= p) end = R.pos[++r + 1];
    }
    LFX_HD const uint8_t *at(const DtrainRecs &R, uint32_t p) const { return R.base + R.off[r] + (p - R.pos[r]); }
};

// A lane's consecutive positions [p, pe), pe - p <= 8, pe <= n: fn(q, avail, defined, v) for each, avail = the bytes of q's
// record from q on, defined = avail >= 8, v = the d-mer's eight bytes (little-endian) where defined.  LOAD: whether v is wanted
// at all.  Per record the lane touches, two 8-byte loads serve up to eight positions; the second one is read byte by byte where
// the record ends inside it — no byte outside a record is read.
template <bool LOAD, class Fn>
LFX_HD inline void dtrain_lane(const DtrainRecs &R, uint32_t p, uint32_t pe, Fn fn) {
    if (p >= pe) return;
    DtrainCursor c;
    c.seek(R, p);
    while (p < pe) {
        c.advance(R, p);
        const uint32_t avail = c.end - p;
        const uint32_t seg = pe - p < avail ? pe - p : avail;
        uint64_t lo = 0, hi = 0;
        if (LOAD && avail >= DTRAIN_D) {
            const uint8_t *a = c.at(R, p);
            lo = dtrain_load8(a);
            if (seg > 1) {
                if (avail >= 16) hi = dtrain_load8(a + 8);
                else for (uint32_t b = 8; b < avail; b++) hi |= (uint64_t)a[b] << (8 * (b - 8));
            }
        }
        for (uint32_t j = 0; j < seg; j++) {
            const uint64_t v = j == 0 ? lo : lo >> (8 * j) | hi << (64 - 8 * j);
            fn(p + j, avail - j, avail - j >= DTRAIN_D, v);
        }
        p += seg;
    }
}

// ---- the kernels' steps on the host, one lane after the other, with the cursor and the lane walk above: record index, counts,
// every epoch's prefix words chunk by chunk, pick and zeroing, the gather's rank sort.  → the dictionary's length in `out`
// (dict_size bytes of room).  For the host test; the library does not call it.
inline uint64_t dtrain_host_walk(const DtrainPlan &pl, const uint8_t *samples, uint8_t *out) {
    if (!pl.n) return 0;
    const uint32_t n = (uint32_t)pl.n, k = pl.k, E = pl.epochs, span_k = k - DTRAIN_D + 1;
    std::vector<uint32_t> tile_rec(dtrain_ntiles(pl.n));
    for (uint32_t t = 0; t < tile_rec.size(); t++) tile_rec[t] = dtrain_owner_search(pl.pos.data(), pl.nrec(), t * DTRAIN_TILE);
    const DtrainRecs R{pl.pos.data(), pl.off.data(), tile_rec.data(), samples, pl.nrec(), n};
    std::vector<uint32_t> freq(1u << DTRAIN_F, 0);
    for (uint64_t p = 0; p < n; p += DTRAIN_PPL)
        dtrain_lane<true>(R, (uint32_t)p, (uint32_t)std::min<uint64_t>(p + DTRAIN_PPL, n), [&](uint32_t, uint32_t, bool def, uint64_t v) {
            if (def) freq[dtrain_hash(v)]++;
        });
    std::vector<uint64_t> slots(E, 0), x((size_t)DTRAIN_CHUNK + k);
    for (uint32_t e = 0; e < E; e++) {
        const uint32_t lo = dtrain_epoch_lo(e, E, n), hi = dtrain_epoch_lo(e + 1, E, n);
        for (uint32_t c0 = lo; c0 < hi; c0 += DTRAIN_CHUNK) {
            const uint32_t c1 = std::min(c0 + DTRAIN_CHUNK, hi), s1 = (uint32_t)std::min<uint64_t>((uint64_t)c1 + k - DTRAIN_D, n);
            uint64_t run = 0;
            for (uint32_t q0 = c0; q0 < s1; q0 += DTRAIN_SPL)
                dtrain_lane<true>(R, q0, std::min(q0 + DTRAIN_SPL, s1), [&](uint32_t q, uint32_t, bool def, uint64_t v) {
                    x[q - c0] = run;
                    run += def ? freq[dtrain_hash(v)] : 0;
                });
            x[s1 - c0] = run;
            for (uint32_t p0 = c0; p0 < c1; p0 += DTRAIN_SPL)
                dtrain_lane<false>(R, p0, std::min(p0 + DTRAIN_SPL, c1), [&](uint32_t q, uint32_t avail, bool, uint64_t) {
                    if (avail < k) return;
                    const uint64_t sum = x[q - c0 + span_k] - x[q - c0];
                    if (sum) slots[e] = std::max(slots[e], dtrain_pick_key(sum, q - lo));
                });
        }
        if (slots[e] >> 32) {
            const uint32_t p = lo + dtrain_pick_pos(slots[e]);
            DtrainCursor c;
            c.seek(R, p);
            for (uint32_t j = 0; j < span_k; j++) freq[dtrain_hash(dtrain_load8(c.at(R, p) + j))] = 0;
        }
    }
    std::vector<uint64_t> key;
    std::vector<uint32_t> at;
    for (uint32_t e = 0; e < E; e++)
        if (slots[e] >> 32) { key.push_back(dtrain_sort_key(slots[e], e)); at.push_back(dtrain_epoch_lo(e, E, n) + dtrain_pick_pos(slots[e])); }
    for (size_t i = 0; i < key.size(); i++) {
        size_t rank = 0;
        for (size_t j = 0; j < key.size(); j++) rank += key[j] < key[i];
        DtrainCursor c;
        c.seek(R, at[i]);
        memcpy(out + rank * k, c.at(R, at[i]), k);
    }
    return (uint64_t)key.size() * k;
}

// the kernels' launcher (lfx_dict_train.hip): everything on `st`, no host wait; d_scratch holds dtrain_scratch's regions with
// pos and off already on their way up on `st`.  *d_out_len (in the scratch) receives the dictionary's length.
int launch_dict_train(void *st, const DtrainPlan &pl, const DtrainScratch &w, uint8_t *d_scratch, const uint8_t *d_samples, uint8_t *d_dict);

}  // namespace lfx
