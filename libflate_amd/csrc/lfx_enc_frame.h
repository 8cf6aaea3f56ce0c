// lfx_enc_frame.h — host only, no HIP: what the encode entry points and the stream encoder's state machine (lfx_stream_enc.h,
// built by a plain host compiler) share of the framing — the options resolved once into an EncodeSpec, the table of which entry
// point serves which spec, the container header, and the arithmetic that folds two checksums into one.  The C ABI's wrappers
// around it stay in lfx_api.cpp.
#pragma once
#include <stdint.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "../../include/lfx.h"
#include "lfx_common.h"
#include "lfx_plan.h"

namespace lfx {

inline uint32_t host_crc32(const uint8_t *p, size_t n) {
    static uint32_t tab[256];
    static std::once_flag once;
    std::call_once(once, [] {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1)));
            tab[i] = c;
        }
    });
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) c = (c >> 8) ^ tab[(c ^ p[i]) & 0xFF];
    return ~c;
}
inline uint32_t gf2_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & 0x80000000u) p ^= b;
        a <<= 1;
        b = (b >> 1) ^ (0xEDB88320u & (0u - (b & 1)));
    }
    return p;
}
inline uint32_t gf2_xpow8n(uint64_t nbytes) {
    uint32_t r = 0x80000000u, sq = 0x00800000u;
    while (nbytes) {
        if (nbytes & 1) r = gf2_mulmod(r, sq);
        sq = gf2_mulmod(sq, sq);
        nbytes >>= 1;
    }
    return r;
}
// CRC(A||B) from CRC(A), CRC(B), |B| (the reference never combines)
inline uint32_t crc32_combine(uint32_t crc1, uint32_t crc2, uint64_t len2) { return gf2_mulmod(crc1, gf2_xpow8n(len2)) ^ crc2; }
inline uint32_t adler32_combine(uint32_t ad1, uint32_t ad2, uint64_t len2) {
    const uint32_t M = 65521u;
    uint32_t a1 = ad1 & 0xFFFF, b1 = ad1 >> 16, a2 = ad2 & 0xFFFF, b2 = ad2 >> 16;
    uint32_t rem = (uint32_t)(len2 % M);
    uint32_t a = (a1 + a2 + M - 1) % M;
    uint32_t b = (uint32_t)((b1 + b2 + (uint64_t)rem * ((a1 + M - 1) % M)) % M);
    return (b << 16) | a;
}

inline void encode_opts_default(lfx_encode_opts *o) {
    memset(o, 0, sizeof *o);
    o->block_size = 1u << 20;
    o->dynamic_huffman = 1;
    o->window_size = MAX_WINDOW;
    o->max_length = MAX_LENGTH;
    o->os = 3;
}
// lz77_kind: the kind in bits 0..7; LFX_LZ77_CHAIN and LFX_LZ77_LAZY carry their depth in bits 8..15, LFX_LZ77_LEVEL its level
// (include/lfx.h).  The bits above bit 7 are not read for the kinds 0 and 1.
inline int lz77_kind_of(const lfx_encode_opts &o) { return (int)((uint32_t)o.lz77_kind & 0xFFu); }
// the kinds that carry a chain depth of the caller's in bits 8..15
inline bool lz77_chained(int kind) { return kind == LFX_LZ77_CHAIN || kind == LFX_LZ77_LAZY; }
// the kinds that run the chain stage: those, and LFX_LZ77_LEVEL, whose depth comes from the level table below (§23)
inline bool lz77_chain_stage(int kind) { return lz77_chained(kind) || kind == LFX_LZ77_LEVEL; }
// the kinds that carry a level 1..9 in bits 8..15: LFX_LZ77_LEVEL and LFX_LZ77_COST (§27), which is that level's encoder with
// the lazy rule replaced by the cost rule.  (5 stays refused: tests/c/level_opts.cpp pins !lz77_chain_stage(5); the kind is 6.)
inline bool lz77_leveled(int kind) { return kind == LFX_LZ77_LEVEL || kind == LFX_LZ77_COST; }
// "runs the chain stage", LFX_LZ77_COST included
inline bool lz77_runs_chain(int kind) { return lz77_chain_stage(kind) || kind == LFX_LZ77_COST; }

// LFX_LZ77_LEVEL: what a level 1..9 resolves into — zlib's configuration_table (deflate.c) without good_length,
// which makes a position's length depend on its predecessor's and stays out.  max_lazy and too_far are read by the lazy levels
// alone; for the greedy ones they hold "never" (no position is kept for its length, no 3-byte match is dropped).
struct LevelTune {
    uint32_t depth;               // K: chain depth (1..4096: a kernel argument, not the bit field of the kinds 2 and 3)
    bool lazy;                    // the lazy walk (levels 4..9) or ChainLz77Encoder's greedy one (1..3)
    uint32_t nice;                // N: a chain walk ends behind the first candidate of min(N, lim) bytes or more
    uint32_t max_lazy;            // Z: a position with L >= Z is not deferred
    uint32_t too_far;             // F: a 3-byte match farther than F is dropped
};
constexpr uint32_t LEVEL_NEVER = 0xFFFFFFFFu;
// level 1..9 → its tuning; any other level: depth 0
inline LevelTune level_tune(uint32_t level) {
    static const LevelTune T[10] = {{0, false, 0, 0, 0},
                                    {4, false, 8, LEVEL_NEVER, LEVEL_NEVER},
                                    {8, false, 16, LEVEL_NEVER, LEVEL_NEVER},
                                    {32, false, 32, LEVEL_NEVER, LEVEL_NEVER},
                                    {16, true, 16, 4, 4096},
                                    {32, true, 32, 16, 4096},
                                    {128, true, 128, 16, 4096},
                                    {256, true, 128, 32, 4096},
                                    {1024, true, 258, 128, 4096},
                                    {4096, true, 258, 258, 4096}};
    return T[level <= 9 ? level : 0];
}
// E::compression_level() as lz77_level holds it (1 + LFX_LEVEL_*, 0: the kind's own): ChainLz77Encoder and LazyLz77Encoder are
// Best unless the caller says otherwise, LFX_LZ77_LEVEL is Fast for the levels 1..3, Balance for 4..6 and Best for 7..9 (a level
// outside 1..9 is refused by encode_spec: Balance here); no_compression() resets the header's level like any other
// (zlib.rs:471-475, gzip.rs:703)
inline uint8_t lz77_level_of(const lfx_encode_opts &o) {
    if (o.lz77_level == 0 && (lz77_chained(lz77_kind_of(o)) || lz77_kind_of(o) == LFX_LZ77_COST) && !o.no_compression) return 1 + LFX_LEVEL_BEST;
    if (o.lz77_level == 0 && lz77_kind_of(o) == LFX_LZ77_LEVEL && !o.no_compression) {
        const uint32_t level = ((uint32_t)o.lz77_kind >> 8) & 0xFFu;
        return (uint8_t)(1 + (level <= 3 ? LFX_LEVEL_FAST : level >= 7 ? LFX_LEVEL_BEST : LFX_LEVEL_BALANCE));
    }
    return o.lz77_level;
}

// What one encode call does, resolved ONCE from the caller's options (encode_spec) and handed on whole: the entry points plan
// from `plan`, the encode core (encode_prepare) takes the rest.
struct EncodeSpec {
    lfx_encode_opts o;            // normalised: window_size and max_length clamped, the defaults for a NULL
    PlanOpts plan;                // what the planner reads
    uint32_t chain_depth = 0;     // ChainLz77Encoder's or LazyLz77Encoder's depth; 0: any other kind, no chain stage
    bool lazy = false;            // LazyLz77Encoder: the chain stage also demotes a position whose successor matches longer (§20)
    bool tuned = false;           // LFX_LZ77_LEVEL (§23): chain_depth and lazy come from the level, and the chain stage runs its tuned instances with ...
    LevelTune tune{0, false, 0, 0, 0};   // ... this (tune.depth == chain_depth, tune.lazy == lazy); all 0 for any other kind
    bool cost = false;            // LFX_LZ77_COST (§27): the level's candidates (tuned, tune), the cost rule in place of the lazy one (lazy is false)
    bool auto_blocks = false;     // LFX_HUFFMAN_AUTO (§22): every dynamic block's form chosen on the device; never under no_compression
    bool merge_blocks = false;    // block_merge (§24): neighbouring dynamic blocks joined on the device; never under no_compression or fixed codes
};
// → LFX_OK, or LFX_E_ARG for options outside the domain.  *out is filled either way (lfx_encode_index_device asks
// encode_served before it answers for the domain).
inline int encode_spec(int format, const lfx_encode_opts *o, EncodeSpec *out) {
    lfx_encode_opts &d = out->o;
    if (o) d = *o; else encode_opts_default(&d);
    if (d.window_size > MAX_WINDOW) d.window_size = MAX_WINDOW;  // default.rs:228
    if (d.max_length > MAX_LENGTH) d.max_length = MAX_LENGTH;    // default.rs:240
    const int kind = lz77_kind_of(d);
    out->cost = kind == LFX_LZ77_COST;
    out->tuned = lz77_leveled(kind);
    out->tune = level_tune(out->tuned ? ((uint32_t)d.lz77_kind >> 8) & 0xFFu : 0u);
    out->chain_depth = lz77_chained(kind) ? ((uint32_t)d.lz77_kind >> 8) & 0xFFu : out->tune.depth;
    out->lazy = kind == LFX_LZ77_LAZY || (out->tune.lazy && !out->cost);
    out->auto_blocks = d.dynamic_huffman == LFX_HUFFMAN_AUTO && !d.no_compression;
    out->merge_blocks = d.block_merge == 1 && d.dynamic_huffman != 0 && !d.no_compression;
    PlanOpts &p = out->plan;
    p.block_size = d.block_size;
    p.dynamic_huffman = d.dynamic_huffman != 0;
    p.no_compression = d.no_compression != 0;
    p.lz77_kind = out->cost ? (int)LFX_LZ77_LEVEL : kind;   // (without the depth; LFX_LZ77_COST buffers and flushes as its level does: the plan is kind 4's)
    p.window_size = d.window_size;
    p.max_length = d.max_length;
    p.zlib_sync = format == LFX_ZLIB && d.zlib_flush_mode == LFX_FLUSH_SYNC;
    if (d.block_size == 0) return LFX_E_ARG;  // `while len >= 0` never terminates in the reference
    if (d.max_length < 3) return LFX_E_ARG;   // default.rs:125 underflows
    if (kind == 5) return LFX_E_ARG;           // no kind: the number between LFX_LZ77_LEVEL and LFX_LZ77_COST names no encoder
    if (lz77_runs_chain(kind) && (out->chain_depth == 0 || ((uint32_t)d.lz77_kind >> 16) != 0)) return LFX_E_ARG;
    if (d.block_merge > 1) return LFX_E_ARG;
    return LFX_OK;
}

// Which entry point serves which spec and dictionary: THE table (the public contract: include/lfx.h, and
// tests/c/encode_spec.cpp holds one against the other).  Nothing else answers LFX_E_UNSUPPORTED for a combination of options
// and dictionary.
enum EncodeEntry { ENC_DEVICE, ENC_BATCH, ENC_DICT_DEVICE, ENC_DICT_BATCH, ENC_STREAM, ENC_MEMBERS, ENC_INDEX, ENC_SHARD, ENC_LZ77,
                   // lfx_encode_batch_packed_device (§26), with or without a dictionary: the rows of ENC_BATCH / ENC_DICT_BATCH —
                   // none of its own, the dictionary rows by the dictionary's kind
                   ENC_BATCH_PACKED };
enum DictKind { DICT_NONE, DICT_PLAIN, DICT_CHAIN };     // lfx_dict_new / lfx_dict_new_chain (§18, §21)
// → LFX_OK (*why = nullptr), or LFX_E_UNSUPPORTED with *why.  Where a call has two reasons, the first row wins.
inline int encode_served(EncodeEntry e, const EncodeSpec &sp, DictKind dict, const char **why) {
    const bool chained = lz77_chain_stage(sp.plan.lz77_kind), level = sp.plan.lz77_kind == LFX_LZ77_LEVEL;
    *why = e == ENC_SHARD && sp.o.no_compression ? "sharded encode of stored blocks is not supported (their size depends on the bit phase)"
         // LFX_LZ77_COST (§27; its plan is kind 4's, so its rows stand in front of LFX_LZ77_LEVEL's): a second parse would list
         // the encode index's candidates twice
         : e == ENC_SHARD && sp.cost ? "lz77_kind: the N-GPU encode does not serve LFX_LZ77_COST"
         : e == ENC_INDEX && sp.cost ? "lz77_kind: lfx_encode_index_device does not serve LFX_LZ77_COST (its second parse would list the candidates twice)"
         : e == ENC_SHARD && level ? "lz77_kind: the N-GPU encode does not serve LFX_LZ77_LEVEL"
         : e == ENC_SHARD && chained ? (sp.lazy ? "lz77_kind: the N-GPU encode does not serve LFX_LZ77_LAZY" : "lz77_kind: the N-GPU encode does not serve LFX_LZ77_CHAIN")
         : e == ENC_SHARD && sp.auto_blocks ? "dynamic_huffman: the N-GPU encode does not serve LFX_HUFFMAN_AUTO (a stored block's size depends on the bit phase)"
         : e == ENC_INDEX && sp.auto_blocks ? "dynamic_huffman: lfx_encode_index_device does not serve LFX_HUFFMAN_AUTO (the candidates are laid out from the host plan's block types)"
         // block_merge (§24): the entry points that read the host plan's blocks behind the Huffman stage, or promise a block boundary
         : e == ENC_SHARD && sp.merge_blocks ? "block_merge: the N-GPU encode does not serve block_merge (a shard's blocks are laid out from the host plan)"
         : e == ENC_INDEX && sp.merge_blocks ? "block_merge: lfx_encode_index_device does not serve block_merge (the candidates are laid out from the host plan's blocks)"
         : e == ENC_MEMBERS && sp.merge_blocks ? "block_merge: lfx_encode_members_* does not serve block_merge (a member's blocks are laid out from the host plan)"
         : e == ENC_STREAM && sp.merge_blocks ? "block_merge: the stream encoder does not serve block_merge (a merge across a flush would break what a flush promises)"
         // ChainLz77Encoder and LazyLz77Encoder have no chain behind a plain dictionary's candidate (§19); a chain dictionary brings its own
         : dict == DICT_PLAIN && sp.cost ? "lz77_kind: LFX_LZ77_COST with a preset dictionary is not supported (a dictionary made by lfx_dict_new_chain serves it)"
         : dict == DICT_PLAIN && level ? "lz77_kind: LFX_LZ77_LEVEL with a preset dictionary is not supported (a dictionary made by lfx_dict_new_chain serves it)"
         : dict == DICT_PLAIN && chained ? (sp.lazy ? "lz77_kind: LFX_LZ77_LAZY with a preset dictionary is not supported (a dictionary made by lfx_dict_new_chain serves it)"
                                                    : "lz77_kind: LFX_LZ77_CHAIN with a preset dictionary is not supported (a dictionary made by lfx_dict_new_chain serves it)")
         : nullptr;
    return *why ? LFX_E_UNSUPPORTED : LFX_OK;
}

// gzip Header::write_to gzip.rs:368-389 (+flags 343-355, crc16 356-367)
inline void gzip_header(const lfx_encode_opts &o, bool with_hcrc, std::vector<uint8_t> &b) {
    uint8_t flg = (uint8_t)((o.is_text ? 1 : 0) | (with_hcrc ? 2 : 0) | (o.extra ? 4 : 0) |
                            (o.filename ? 8 : 0) | (o.comment ? 16 : 0));
    // XFL is the level of the header the options hold when the encoder is made (gzip.rs:368-389): DefaultLz77Encoder →
    // Balance → Unknown(0); NoCompression → None → Unknown(0); a caller's E: Fast → Fastest(4), Best → Slowest(2)
    // (gzip.rs:84-92,684).  no_compression() resets it to Unknown WHEN IT IS CALLED (gzip.rs:703) and a later header(h)
    // replaces it again (gzip.rs:717-720): the option builders above this ABI apply both in call order and pass the result in
    // lz77_level — it is not overridden here (no_compression().header(h with Fastest) writes XFL 4).
    const uint8_t lvl = lz77_level_of(o);
    const uint8_t xfl = lvl == 1 + LFX_LEVEL_FAST ? 4 : lvl == 1 + LFX_LEVEL_BEST ? 2 : 0;
    const uint8_t h[10] = {31, 139, 8, flg, (uint8_t)o.mtime, (uint8_t)(o.mtime >> 8),
                           (uint8_t)(o.mtime >> 16), (uint8_t)(o.mtime >> 24), xfl, o.os};
    b.insert(b.end(), h, h + 10);
    if (o.extra) {
        b.push_back((uint8_t)o.extra_len);
        b.push_back((uint8_t)(o.extra_len >> 8));
        b.insert(b.end(), o.extra, o.extra + o.extra_len);
    }
    if (o.filename) b.insert(b.end(), o.filename, o.filename + strlen(o.filename) + 1);
    if (o.comment) b.insert(b.end(), o.comment, o.comment + strlen(o.comment) + 1);
    if (with_hcrc) {
        // the reference checksums the header serialised with is_verified = false (FLG.HCRC clear)
        std::vector<uint8_t> t;
        gzip_header(o, false, t);
        uint32_t c = host_crc32(t.data(), t.size());
        b.push_back((uint8_t)c);
        b.push_back((uint8_t)(c >> 8));
    }
}
inline int container_header(int format, const lfx_encode_opts &o, std::vector<uint8_t> &b) {
    if (format == LFX_GZIP) {
        if (o.extra && o.extra_len > 0xFFFF) return LFX_E_INVALID_DATA;  // gzip.rs:490-492
        gzip_header(o, o.hcrc != 0, b);
    } else if (format == LFX_ZLIB) {
        // zlib Header::write_to zlib.rs:267-279; from_lz77 212-220; Lz77WindowSize::from_u16 132-151
        uint32_t ws = o.window_size;
        uint8_t cinfo = ws > 16384 ? 7 : ws > 8192 ? 6 : ws > 4096 ? 5 : ws > 2048 ? 4 : ws > 1024 ? 3
                        : ws > 512 ? 2 : ws > 256 ? 1 : 0;
        uint8_t level = (o.no_compression || lz77_kind_of(o) == LFX_LZ77_NOCOMPRESSION) ? 0 : 2;
        if (lz77_level_of(o) && !o.no_compression) level = (uint8_t)((lz77_level_of(o) - 1) & 3);   // lz77 None/Fast/Balance/Best → 0..3 (zlib.rs:59-68)
        uint8_t cmf = (uint8_t)((cinfo << 4) | 8), flg = (uint8_t)(level << 6);
        uint32_t check = ((uint32_t)cmf << 8) + flg;
        if (check % 31 != 0) flg = (uint8_t)(flg + (31 - check % 31));
        b.push_back(cmf);
        b.push_back(flg);
    } else if (format != LFX_DEFLATE) {
        return LFX_E_ARG;
    }
    return LFX_OK;
}

// A preset dictionary in the container and in the plan (the stream encoder: §25).  zlib: FDICT set, FCHECK
// recomputed, DICTID behind the two header bytes (RFC 1950 2.2); raw DEFLATE: nothing.  hdr: what container_header wrote.
inline void dict_header(int format, uint32_t dict_id, std::vector<uint8_t> &hdr) {
    if (format != LFX_ZLIB || hdr.size() != 2) return;
    uint8_t flg = (uint8_t)((hdr[1] & 0xC0) | 0x20);
    const uint32_t check = ((uint32_t)hdr[0] << 8) + flg;
    if (check % 31 != 0) flg = (uint8_t)(flg + (31 - check % 31));
    hdr[1] = flg;
    for (int sh = 24; sh >= 0; sh -= 8) hdr.push_back((uint8_t)(dict_id >> sh));
}
// p: a plan that starts with a stream's first LZ77 flush unit, the one a dictionary with bytes to offer primes — where the
// options match at all.  → whether a chunk was marked
inline bool dict_prime_first(Plan &p) {
    if (p.chunks.empty() || (p.chunks[0].flags & CH_LITERALS)) return false;
    p.chunks[0].flags |= CH_DICT;
    return true;
}

}  // namespace lfx
