// encode_spec.cpp — the resolver of the encode options (encode_spec) and the table of which entry point serves what
// (encode_served), both lfx_enc_frame.h, under a plain host compiler.  The whole matrix — every entry point, lz77 kind and depth,
// dynamic_huffman, no_compression, and no, a plain or a chain dictionary — against what include/lfx.h promises, written out
// here by hand; the spec's fields for every option set; the options outside the domain; and the one place where the table
// answers before the domain does (lfx_encode_index_device).  No HIP, no device.
//   g++ -O2 -std=c++17 -Wall [-fsanitize=address,undefined] -o encode_spec tests/c/encode_spec.cpp && ./encode_spec
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../libflate_amd/csrc/lfx_enc_frame.h"

using namespace lfx;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "encode_spec: line %d: %s  [%s]\n", __LINE__, #c, g_cell); exit(1); } } while (0)
static char g_cell[160] = "";

static const EncodeEntry ENTRIES[9] = {ENC_DEVICE, ENC_BATCH, ENC_DICT_DEVICE, ENC_DICT_BATCH, ENC_STREAM, ENC_MEMBERS, ENC_INDEX, ENC_SHARD, ENC_LZ77};
static const char *const ENTRY_NAMES[9] = {"device", "batch", "dict-device", "dict-batch", "stream", "members", "index", "shard", "lz77"};
static const DictKind DICTS[3] = {DICT_NONE, DICT_PLAIN, DICT_CHAIN};
static const int32_t KINDS[8] = {LFX_LZ77_DEFAULT, LFX_LZ77_NOCOMPRESSION, LFX_LZ77_CHAIN_DEPTH(1), LFX_LZ77_CHAIN_DEPTH(8), LFX_LZ77_CHAIN_DEPTH(255),
                                 LFX_LZ77_LAZY_DEPTH(1), LFX_LZ77_LAZY_DEPTH(8), LFX_LZ77_LAZY_DEPTH(255)};

// include/lfx.h, read out.  A cell is refused (LFX_E_UNSUPPORTED, this message) or served (nullptr):
//  - LFX_LZ77_CHAIN, and LFX_LZ77_LAZY "by the same entry points": served by lfx_encode_device / _host, lfx_encode_batch_device,
//    lfx_encoder_*, lfx_encode_members_* and lfx_encode_index_device, and by the dictionary encode calls with a chain dictionary;
//    LFX_E_UNSUPPORTED from the dictionary encode calls with a plain dictionary and from the N-GPU encode.
//  - LFX_HUFFMAN_AUTO: served by lfx_encode_device / _host, lfx_encode_batch_device, the dictionary encode calls (plain and chain
//    dictionaries), lfx_encoder_* and lfx_encode_members_*, with the lz77 kinds 0, 2 and 3; LFX_E_UNSUPPORTED from
//    lfx_encode_index_device and from the N-GPU encode.  Stored blocks are not touched: under no_compression the value is a
//    plain "non-zero", refused nowhere.
//  - lfx_encode_shard_prepare: no_compression is LFX_E_UNSUPPORTED.
//  - the lfx_lz77 plug-in takes no options: nothing to refuse.
// Where a call has two reasons: the N-GPU encode names no_compression, then the kind, then AUTO; an entry point's own reason
// comes before the dictionary's.  (A plain dictionary has no chain whoever asks: the cells of the entry points that take no
// dictionary say so too, though no call reaches them.)
static const char *expected(EncodeEntry e, int kind, int huffman, int no_compression, DictKind dict) {
    const bool chain = kind == 2, lazy = kind == 3, aut = huffman == 2 && !no_compression;
    if (e == ENC_SHARD) {
        if (no_compression) return "sharded encode of stored blocks is not supported (their size depends on the bit phase)";
        if (chain) return "lz77_kind: the N-GPU encode does not serve LFX_LZ77_CHAIN";
        if (lazy) return "lz77_kind: the N-GPU encode does not serve LFX_LZ77_LAZY";
        if (aut) return "dynamic_huffman: the N-GPU encode does not serve LFX_HUFFMAN_AUTO (a stored block's size depends on the bit phase)";
    }
    if (e == ENC_INDEX && aut)
        return "dynamic_huffman: lfx_encode_index_device does not serve LFX_HUFFMAN_AUTO (the candidates are laid out from the host plan's block types)";
    if (dict == DICT_PLAIN && chain) return "lz77_kind: LFX_LZ77_CHAIN with a preset dictionary is not supported (a dictionary made by lfx_dict_new_chain serves it)";
    if (dict == DICT_PLAIN && lazy) return "lz77_kind: LFX_LZ77_LAZY with a preset dictionary is not supported (a dictionary made by lfx_dict_new_chain serves it)";
    return nullptr;
}

static lfx_encode_opts options(int32_t kind, int32_t huffman, int32_t no_compression) {
    lfx_encode_opts o;
    encode_opts_default(&o);
    o.lz77_kind = kind;
    o.dynamic_huffman = huffman;
    o.no_compression = no_compression;
    return o;
}
static int resolve(int format, const lfx_encode_opts &o, EncodeSpec *sp) { return encode_spec(format, &o, sp); }

int main() {
    int cells = 0, refused = 0, specs = 0;
    // ---- the matrix, and the spec's fields of every option set in it
    for (int32_t kind_word : KINDS)
        for (int32_t huffman = 0; huffman <= 3; huffman++)
            for (int32_t nc = 0; nc <= 1; nc++) {
                const int kind = kind_word & 0xFF, depth = kind_word >> 8;
                snprintf(g_cell, sizeof g_cell, "kind %d depth %d huffman %d no_compression %d", kind, depth, huffman, nc);
                const lfx_encode_opts o = options(kind_word, huffman, nc);
                EncodeSpec sp;
                CHECK(resolve(LFX_ZLIB, o, &sp) == LFX_OK);
                CHECK(sp.chain_depth == (uint32_t)(kind >= 2 ? depth : 0));
                CHECK(sp.lazy == (kind == 3));
                CHECK(sp.auto_blocks == (huffman == 2 && !nc));                 // (never under no_compression)
                CHECK(sp.plan.lz77_kind == kind);                               // the plan's kind: without the depth
                CHECK(sp.plan.dynamic_huffman == (huffman != 0) && sp.plan.no_compression == (nc != 0));
                CHECK(sp.plan.block_size == (1u << 20) && sp.plan.window_size == 32768 && sp.plan.max_length == 258 && !sp.plan.zlib_sync);
                CHECK(sp.o.lz77_kind == kind_word && sp.o.dynamic_huffman == huffman && sp.o.no_compression == nc);
                // the level: the kinds 2 and 3 are Best unless the caller names one; no_compression resets it
                CHECK(lz77_level_of(sp.o) == (kind >= 2 && !nc ? 1 + LFX_LEVEL_BEST : 0));
                lfx_encode_opts named = o;
                named.lz77_level = 1 + LFX_LEVEL_FAST;
                EncodeSpec sn;
                CHECK(resolve(LFX_ZLIB, named, &sn) == LFX_OK && lz77_level_of(sn.o) == 1 + LFX_LEVEL_FAST);
                specs++;
                for (int ei = 0; ei < 9; ei++)
                    for (DictKind dict : DICTS) {
                        snprintf(g_cell, sizeof g_cell, "%s: kind %d depth %d huffman %d no_compression %d dict %d", ENTRY_NAMES[ei], kind, depth,
                                 huffman, nc, (int)dict);
                        const char *want = expected(ENTRIES[ei], kind, huffman, nc, dict);
                        const char *why = nullptr;
                        const int rc = encode_served(ENTRIES[ei], sp, dict, &why);
                        if (want) { CHECK(rc == LFX_E_UNSUPPORTED && why && strcmp(why, want) == 0); refused++; }
                        else CHECK(rc == LFX_OK && why == nullptr);
                        cells++;
                    }
            }
    // the walk's size, counted by hand from the lists above.  Of the 64 option sets: shard refuses 32 (no_compression) + 24 (kinds
    // 2, 3) + 2 (AUTO, kinds 0, 1), under each dictionary: 174; index 8 (AUTO) under each dictionary and 42 more (kinds 2, 3
    // without AUTO) under a plain one: 66; each of the other seven the 48 sets of the kinds 2, 3 under a plain one: 336
    CHECK(cells == 8 * 4 * 2 * 9 * 3 && refused == 174 + 66 + 336);
    g_cell[0] = 0;

    // ---- NULL options are the defaults; the clamps; the zlib sync flush belongs to the zlib container alone
    {
        EncodeSpec sp, sd;
        lfx_encode_opts o;
        encode_opts_default(&o);
        CHECK(encode_spec(LFX_GZIP, nullptr, &sp) == LFX_OK && resolve(LFX_GZIP, o, &sd) == LFX_OK);
        CHECK(memcmp(&sp.o, &sd.o, sizeof o) == 0 && sp.chain_depth == 0 && !sp.lazy && !sp.auto_blocks && sp.plan.lz77_kind == 0);
        CHECK(sp.plan.dynamic_huffman && !sp.plan.no_compression && sp.plan.block_size == (1u << 20));
        o.window_size = 1u << 20;
        o.max_length = 1000;
        o.zlib_flush_mode = LFX_FLUSH_SYNC;
        o.block_size = 12345;
        CHECK(resolve(LFX_ZLIB, o, &sp) == LFX_OK);
        CHECK(sp.o.window_size == 32768 && sp.o.max_length == 258 && sp.plan.window_size == 32768 && sp.plan.max_length == 258);
        CHECK(sp.plan.zlib_sync && sp.plan.block_size == 12345);
        CHECK(resolve(LFX_GZIP, o, &sp) == LFX_OK && !sp.plan.zlib_sync);
        CHECK(resolve(LFX_DEFLATE, o, &sp) == LFX_OK && !sp.plan.zlib_sync);
        o.window_size = 1024;
        o.max_length = 3;
        CHECK(resolve(LFX_ZLIB, o, &sp) == LFX_OK && sp.plan.window_size == 1024 && sp.plan.max_length == 3);
        specs += 6;
    }

    // ---- outside the domain: LFX_E_ARG
    {
        EncodeSpec sp;
        for (int kind = 2; kind <= 3; kind++) {
            CHECK(resolve(LFX_ZLIB, options(kind, 1, 0), &sp) == LFX_E_ARG);                             // depth 0: there is no default depth
            for (int bit = 16; bit < 32; bit++)
                CHECK(resolve(LFX_ZLIB, options((int32_t)((uint32_t)(kind | 8 << 8) | 1u << bit), 1, 0), &sp) == LFX_E_ARG);
        }
        for (int kind = 0; kind <= 1; kind++)                                                           // kinds 0, 1: the upper bits are not read
            CHECK(resolve(LFX_ZLIB, options((int32_t)((uint32_t)kind | 0xFFFFFF00u), 1, 0), &sp) == LFX_OK && sp.chain_depth == 0 && sp.plan.lz77_kind == kind);
        lfx_encode_opts o = options(0, 1, 0);
        o.block_size = 0;
        CHECK(resolve(LFX_ZLIB, o, &sp) == LFX_E_ARG);
        for (uint32_t ml = 0; ml < 3; ml++) {
            o = options(0, 1, 0);
            o.max_length = ml;
            CHECK(resolve(LFX_ZLIB, o, &sp) == LFX_E_ARG);
        }
        // each of them under every kind that is itself inside the domain
        for (int32_t kind_word : KINDS) {
            o = options(kind_word, 2, 0);
            o.block_size = 0;
            CHECK(resolve(LFX_GZIP, o, &sp) == LFX_E_ARG);
            o = options(kind_word, 0, 1);
            o.max_length = 2;
            CHECK(resolve(LFX_DEFLATE, o, &sp) == LFX_E_ARG);
        }
    }

    // ---- lfx_encode_index_device refuses LFX_HUFFMAN_AUTO before the options are range-checked: AUTO with block_size 0 is
    //      LFX_E_UNSUPPORTED there, and LFX_E_ARG everywhere else
    {
        lfx_encode_opts o = options(0, LFX_HUFFMAN_AUTO, 0);
        o.block_size = 0;
        EncodeSpec sp;
        CHECK(resolve(LFX_GZIP, o, &sp) == LFX_E_ARG && sp.auto_blocks);         // (the spec is filled whatever the status)
        const char *why = nullptr;
        CHECK(encode_served(ENC_INDEX, sp, DICT_NONE, &why) == LFX_E_UNSUPPORTED &&
              strcmp(why, "dynamic_huffman: lfx_encode_index_device does not serve LFX_HUFFMAN_AUTO (the candidates are laid out from the host plan's block types)") == 0);
        o.no_compression = 1;                                                    // no AUTO to refuse: the domain answers
        why = nullptr;
        CHECK(resolve(LFX_GZIP, o, &sp) == LFX_E_ARG && !sp.auto_blocks && encode_served(ENC_INDEX, sp, DICT_NONE, &why) == LFX_OK && !why);
    }
    printf("encode_spec ok: %d cells, %d refused, %d specs\n", cells, refused, specs);
    return 0;
}
