// lfx_index.h — the seek index (lfx_decode_index_device and friends): what the decode records for it, the
// index object, and the launchers of lfx_index.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <memory>
#include <string>
#include <vector>

#include "../../include/lfx.h"
#include "lfx_decode.h"

namespace lfx {

struct Ctx;
struct Plan;

constexpr uint32_t IDX_CRC_BYTES = 64;          // lfx_index_point::in_crc covers so many input bytes from in_bit / 8
constexpr uint32_t IDX_WINDOW = 32768;
constexpr uint64_t IDX_COPY_CHUNK = 256u << 10;  // bytes one workgroup of idx_copy_kernel moves

// an access-point candidate (bits relative to input byte 0, output relative to the decode's output)
struct IdxCand {
    uint64_t in_bit, hdr_bit, out_off;
    uint32_t btype;   // IDX_BTYPE_READ: a block start whose BTYPE the probe kernel reads from the input
};
constexpr uint32_t IDX_BTYPE_READ = 0xFF;

// What the decode records while an index is being built (Ctx::idx): block starts of every proved chain, and the lanes of its
// blocks larger than `spacing`, gathered on the device before the next chain reuses their slots.
struct IdxCollect {
    uint64_t spacing = 0;
    bool in_order = false;                   // cand is sorted by in_bit, without repeats (lfx_encode_index_device): no sort
    uint64_t bit_base = 0, out_base = 0;     // where the current inflate_member call's d_in / d_out start (decode_stream sets them)
    std::vector<IdxCand> cand;
    struct Grab {
        void *dev = nullptr;                  // n x 2048 u64: lane starts, then lane output offsets (idx_lanes_kernel)
        std::vector<uint32_t> slots;          // (the upload's source: lives until the copy is done)
        struct Meta { uint64_t hdr_bit, bit_base, out_base; uint32_t btype, nlanes; bool skip0; };
        std::vector<Meta> meta;
    };
    std::vector<Grab> grabs;
    ~IdxCollect() { for (Grab &g : grabs) if (g.dev) (void)hipFree(g.dev); }
};

// Records the proved chain emit[0, ne) of one decode step: its block starts and the lanes of its large blocks (lanes: the
// scan's BlkLanes, indexed by BlkEmit::cand).  bit_base / out_base: added to the entries' bits and output offsets.
// pieces: the entries are the pieces of inflate_member (an entry continues its block when the one in front ended open).
int idx_record_chain(Ctx *c, const BlkEmit *emit, uint32_t ne, const BlkLanes *d_lanes, uint64_t bit_base, uint64_t out_base,
                     bool pieces);

struct IdxCopy {
    const uint8_t *src;
    uint8_t *dst;
    uint64_t len;   // <= IDX_COPY_CHUNK
};
int launch_idx_copy(hipStream_t st, const IdxCopy *d_tasks, uint32_t n);
int launch_idx_lanes(hipStream_t st, const BlkLanes *lanes, const uint32_t *slots, uint32_t n, uint64_t *out);
int launch_idx_probe(hipStream_t st, const uint8_t *in, uint64_t n, const uint64_t *bits, uint32_t np, uint32_t *crc, uint32_t *btype);
// the copies (src, dst, len) of any length, split into IDX_COPY_CHUNK tasks, through ONE launch (scratch: Ctx::d_idx_tasks);
// `tasks` is the upload's source: it must live until the stream has passed the copy
int idx_copy(Ctx *c, const std::vector<IdxCopy> &copies, std::vector<IdxCopy> &tasks);

// lfx_encode_index_device (lfx_index_enc.hip): the candidates of the stream the last encode_emit wrote with `plan` — every block
// start, and in blocks larger than Ctx::idx_enc->spacing the first code start of each grain — into Ctx::idx_enc->cand
int idx_encode_cand(Ctx *c, const Plan &plan);

uint32_t idx_crc32(const void *p, uint64_t n, uint32_t crc = 0);
// Builds the index from the candidates and the member table of a finished decode (d_in / d_out as the decode saw them)
int idx_finish(Ctx *c, IdxCollect &col, int format, uint32_t flags, const uint8_t *d_in, uint64_t consumed, const uint8_t *d_out,
               uint64_t out_len, const std::vector<lfx_member> &members, lfx_index **out);

}  // namespace lfx

struct lfx_index {
    lfx::Ctx *c = nullptr;
    lfx_index_info info{};
    std::vector<lfx_index_point> pts;
    std::vector<uint64_t> member_end;   // output byte behind each member (the last segment of a member ends there)
    std::vector<uint64_t> win_at;       // device offset of each point's window in d_win (16-byte phase of its out_off - win_len)
    uint8_t *d_win = nullptr;
    uint64_t win_bytes = 0;
    lfx_index() = default;
    lfx_index(const lfx_index &) = delete;
    lfx_index &operator=(const lfx_index &) = delete;
    ~lfx_index();       // frees d_win on the context's device
};
