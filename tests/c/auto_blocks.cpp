// auto_blocks.cpp — the host-only parts of LFX_HUFFMAN_AUTO under a plain host compiler: how dynamic_huffman is
// decoded (lfx_enc_frame.h), that the plan of the value 2 is the plan of the value 1, and what a stored choice makes
// load-bearing — every compressed block's in_off / in_len are its chunks' bytes, in the planner (write, write_repeat, flush), in
// a plan taken out piecewise (the stream encoder's batches) and behind Plan::append (the batch and members calls).  No HIP, no
// device.
//   g++ -O2 -std=c++17 -Wall [-fsanitize=address,undefined] -o auto_blocks tests/c/auto_blocks.cpp && ./auto_blocks
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../libflate_amd/csrc/lfx_enc_frame.h"

using namespace lfx;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "auto_blocks: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static lfx_encode_opts with_huffman(int32_t v) {
    lfx_encode_opts o;
    encode_opts_default(&o);
    o.dynamic_huffman = v;
    return o;
}
// the options resolved (encode_spec): the status beside the spec
struct Resolved { int rc; EncodeSpec sp; };
static Resolved resolve(int format, const lfx_encode_opts &o) { Resolved r; r.rc = encode_spec(format, &o, &r.sp); return r; }
static bool same_plan(const Plan &a, const Plan &b) {
    if (a.chunks.size() != b.chunks.size() || a.blocks.size() != b.blocks.size() || a.n_codes_cap != b.n_codes_cap ||
        a.n_tiles != b.n_tiles || a.n_vis != b.n_vis || a.n_segs != b.n_segs) return false;
    for (size_t i = 0; i < a.chunks.size(); i++)
        if (a.chunks[i].in_off != b.chunks[i].in_off || a.chunks[i].len != b.chunks[i].len || a.chunks[i].flags != b.chunks[i].flags ||
            a.chunks[i].block != b.chunks[i].block || a.chunks[i].code_off != b.chunks[i].code_off) return false;
    for (size_t i = 0; i < a.blocks.size(); i++)
        if (a.blocks[i].in_off != b.blocks[i].in_off || a.blocks[i].in_len != b.blocks[i].in_len || a.blocks[i].type != b.blocks[i].type ||
            a.blocks[i].final != b.blocks[i].final || a.blocks[i].first_chunk != b.blocks[i].first_chunk ||
            a.blocks[i].align_after != b.blocks[i].align_after) return false;
    return true;
}
// every compressed block covers exactly its chunks' bytes, which lie back to back from its in_off on; `base`: where the
// plan's byte 0 lies.  Returns the blocks checked.
static int check_ranges(const Plan &p, uint64_t base, uint64_t *end_out = nullptr) {
    int n = 0;
    uint64_t at = base;
    for (size_t b = 0; b < p.blocks.size(); b++) {
        const BlockDesc &bd = p.blocks[b];
        if (bd.type == BT_RAW) { CHECK(bd.n_chunks == 0 && bd.in_off == at); at += bd.in_len; continue; }
        CHECK(bd.n_chunks >= 1 && bd.first_chunk + bd.n_chunks <= p.chunks.size());
        CHECK(bd.in_off == p.chunks[bd.first_chunk].in_off && bd.in_off == at);
        uint64_t sum = 0;
        for (uint32_t c = bd.first_chunk; c < bd.first_chunk + bd.n_chunks; c++) {
            CHECK(p.chunks[c].block == b && p.chunks[c].in_off == bd.in_off + sum);
            sum += p.chunks[c].len;
        }
        CHECK(bd.in_len == sum);
        at += sum;
        n++;
    }
    if (end_out) *end_out = at;
    return n;
}

int main() {
    // ---- the value: 0 fixed, 2 AUTO, everything else dynamic; the layout is unchanged
    CHECK(LFX_HUFFMAN_FIXED == 0 && LFX_HUFFMAN_DYNAMIC == 1 && LFX_HUFFMAN_AUTO == 2 && sizeof(lfx_encode_opts) == 72);
    const int32_t values[5] = {0, 1, 2, 3, -1};
    for (int32_t v : values) {
        const lfx_encode_opts o = with_huffman(v);
        const Resolved r = resolve(LFX_ZLIB, o);
        CHECK(r.rc == LFX_OK);
        CHECK(r.sp.plan.dynamic_huffman == (v != 0) && r.sp.auto_blocks == (v == 2));
        std::vector<uint8_t> h1, hv;
        CHECK(container_header(LFX_ZLIB, with_huffman(1), h1) == LFX_OK && container_header(LFX_ZLIB, o, hv) == LFX_OK && h1 == hv);
        h1.clear(); hv.clear();
        CHECK(container_header(LFX_GZIP, with_huffman(1), h1) == LFX_OK && container_header(LFX_GZIP, o, hv) == LFX_OK && h1 == hv);
    }
    {
        lfx_encode_opts o = with_huffman(LFX_HUFFMAN_AUTO);
        o.no_compression = 1;                                      // stored blocks have no form to choose
        CHECK(resolve(LFX_DEFLATE, o).rc == LFX_OK && !resolve(LFX_DEFLATE, o).sp.auto_blocks);
        CHECK(!EncodeSpec().auto_blocks);
    }

    // ---- seeded plans: the plan of 2 is the plan of 1; in_off / in_len of every compressed block; Plan::append; take_closed
    std::mt19937_64 rng(22);
    int plans = 0, blocks = 0;
    for (int it = 0; it < 2000; it++) {
        lfx_encode_opts o1 = with_huffman(1), o2 = with_huffman(2);
        o1.window_size = o2.window_size = 1u << (8 + rng() % 8);
        o1.block_size = o2.block_size = 1 + rng() % (1u << (10 + rng() % 11));
        o1.lz77_kind = o2.lz77_kind = (int32_t)(rng() % 4 == 0 ? LFX_LZ77_LAZY_DEPTH(8) : rng() % 4 == 1 ? LFX_LZ77_CHAIN_DEPTH(8) : 0);
        o1.zlib_flush_mode = o2.zlib_flush_mode = rng() % 3 == 0 ? LFX_FLUSH_SYNC : LFX_FLUSH_NONE;
        const PlanOpts p1 = resolve(LFX_ZLIB, o1).sp.plan, p2 = resolve(LFX_ZLIB, o2).sp.plan;
        Planner a(p1), b(p2), c(p2), d(p2);
        Plan stitched;
        uint64_t byte0 = 0;
        const int events = 1 + (int)(rng() % 12);
        for (int e = 0; e < events; e++) {
            const uint64_t w = rng() % 3 == 0 ? rng() % 9 : rng() % (1u << (4 + rng() % 16)), cnt = 1 + rng() % 40;
            if (rng() % 7 == 0) { a.flush(); b.flush(); c.flush(); d.flush(); }
            else {
                a.write_repeat(w, cnt);
                b.write_repeat(w, cnt);
                for (uint64_t q = 0; q < cnt; q++) { c.write(w); d.write(w); }
            }
            if (rng() % 3 == 0) {                                  // the stream encoder's batch: offsets relative to the batch
                const uint64_t cut = d.closed_bytes();
                Plan piece = d.take_closed();
                uint64_t end = 0;
                blocks += check_ranges(piece, 0, &end);
                CHECK(end == cut);
                stitched.append(piece, byte0);
                byte0 += cut;
            }
        }
        const Plan &pa = a.finish(), &pb = b.finish(), &pc = c.finish();
        CHECK(same_plan(pa, pb) && same_plan(pb, pc));
        blocks += check_ranges(pb, 0);
        Plan &pd = d.finish();
        check_ranges(pd, 0);
        stitched.append(pd, byte0);
        CHECK(same_plan(stitched, pb));
        // Plan::append: a batch of three streams at arbitrary offsets
        Plan merged;
        const uint64_t offs[3] = {rng() % 1000, 5000000 + rng() % 1000, 1ull << 33};
        for (uint64_t off : offs) merged.append(pb, off);
        for (int s = 0; s < 3; s++) {
            Plan one;
            const size_t nb = pb.blocks.size(), nc = pb.chunks.size();
            one.blocks.assign(merged.blocks.begin() + (std::ptrdiff_t)(s * nb), merged.blocks.begin() + (std::ptrdiff_t)((s + 1) * nb));
            one.chunks.assign(merged.chunks.begin() + (std::ptrdiff_t)(s * nc), merged.chunks.begin() + (std::ptrdiff_t)((s + 1) * nc));
            for (BlockDesc &bd : one.blocks) bd.first_chunk -= (uint32_t)(s * nc);
            for (ChunkDesc &ch : one.chunks) ch.block -= (uint32_t)(s * nb);
            check_ranges(one, offs[s]);
        }
        plans++;
    }
    printf("auto_blocks ok: %d plans, %d blocks\n", plans, blocks);
    return 0;
}
