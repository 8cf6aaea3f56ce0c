// CPU: which pack path the encode's geometry (libflate_amd/csrc/lfx_encode_stages.h) takes for one plan of the real Planner under
// LFX_PACK_BY_CHUNK=1 and =0, for 256 compute units.  tests/test_huff_cases.py runs it over the catalogue's byte inputs: the GPU
// test of the same cases relies on =1 taking the chunk path (huffman_chunk_kernel, pack_chunk_kernel) for chunks of
// lz77_kind = 1 as for parsed ones.
//   huff_geom <lz77_kind> <window_size> <block_size> <write...>     a write is a byte count, or f for Write::flush
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../libflate_amd/csrc/lfx_encode_stages.h"

using namespace lfx;

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    PlanOpts o;
    o.lz77_kind = atoi(argv[1]);
    o.window_size = (uint32_t)strtoul(argv[2], nullptr, 10);
    o.block_size = strtoull(argv[3], nullptr, 10);
    Planner pl(o);
    for (int i = 4; i < argc; i++) {
        if (!strcmp(argv[i], "f")) pl.flush();
        else pl.write(strtoull(argv[i], nullptr, 10));
    }
    const Plan &plan = pl.finish();
    const EncodeGeom on = encode_geometry(plan, false, 256, false, PACK_BY_CHUNK_ON), off = encode_geometry(plan, false, 256, false, PACK_BY_CHUNK_OFF);
    uint32_t literal_chunks = 0;
    for (const ChunkDesc &ch : plan.chunks) literal_chunks += (ch.flags & CH_LITERALS) ? 1u : 0u;
    printf("chunks=%zu blocks=%zu literal_chunks=%u fused_hist=%d on=%d off=%d err=%d\n", plan.chunks.size(), plan.blocks.size(), literal_chunks,
           (int)on.fused_hist, (int)on.pack_by_chunk, (int)off.pack_by_chunk, on.err | off.err);
    return 0;
}
