// lfx_decode.h — descriptors of the inflate kernels (lfx_decode_kernels.hip) and their launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfx_common.h"
#include "lfx_blk.h"

namespace lfx {

struct DecStream {
    uint64_t in_off, in_len;
    uint64_t out_off, out_cap;
};
enum : uint32_t { JOB_SINGLE_BLOCK = 1, JOB_COUNT_ONLY = 2 };
struct InflateJob {
    uint64_t in_off;      // stream base
    uint64_t in_len;      // bytes available from in_off
    uint64_t start_bit;   // first bit to decode, relative to in_off
    uint64_t out_off, out_cap;
    uint64_t hist_avail;  // bytes of this member already produced before this job
    uint64_t stop_bit;    // != 0: the walk ends cleanly when a block ends exactly at this bit (a shard without BFINAL)
    uint32_t flags;
    uint32_t dict_len;    // inflate_dict_kernel only: of hist_avail, so many bytes are the preset dictionary's tail (not in `out`)
};
struct InflateResult {
    uint64_t end_bit;  // bit after the last consumed bit (stored blocks: after the data)
    uint64_t out_len;
    uint32_t status;   // 0 ok, 1 InvalidData, 2 UnexpectedEof, 3 output capacity
    uint32_t final_seen;
    uint32_t err, a0, a1;
    uint32_t needs_hist;
    uint32_t nblocks;
    uint32_t _pad;
    uint64_t blk_out_start;  // output bytes before the block that was being decoded last
    uint64_t blk_start_bit;  // ... and the bit its header started at (a windowed decode resumes there)
};

// the block walker of the size calls (blk_walk_size_kernel): one job = one workgroup that follows a stream's blocks on the device
enum : uint32_t { WALK_FINAL = 0,    // walked to the end of the BFINAL block
                  WALK_STOP = 1,     // a block ended at or behind stop_bit (no BFINAL block so far)
                  WALK_STUCK = 2 };  // the block at stuck_bit is not one the walker settles (the exact path decides what it is)
struct WalkJob {
    uint64_t start_bit;  // header bit of the first block (relative to `in`)
    uint64_t end_bit;    // the stream's end: a block that runs past it is not settled
    uint64_t stop_bit;   // != 0: the walk ends behind the first block that ends at or behind this bit (the next candidate)
};
struct WalkResult {
    uint64_t end_bit;    // bit behind the last settled block
    uint64_t n_out;      // bytes the settled blocks produce
    uint64_t stuck_bit, stuck_out;   // header bit of the last block the walk stood at, and the bytes produced in front of it
    int64_t reach;       // smallest (bytes produced so far - distance) over the matches of the settled blocks, relative to the
                         //   job's first output byte; INT64_MAX: no match.  reach + (bytes in front of the job) < 0: the decode
                         //   fails there with "Too long backword reference"
    uint32_t status, nblocks;
};
int launch_blk_walk_size(hipStream_t st, const uint8_t *in, uint64_t nbytes, const WalkJob *jobs, uint32_t njobs,
                         WalkResult *results, bool small_blocks);   // small_blocks: 256 lanes a job instead of 1024
// tabs: njobs * blk_tabs_bytes() bytes: the decode tables of every scanned block, reused by launch_blk_emit
size_t blk_tabs_bytes();
int launch_blk_scan(hipStream_t st, const uint8_t *in, uint64_t nbytes, const BlkJob *jobs, uint32_t njobs,
                    BlkInfo *infos, BlkLanes *lanes, void *tabs = nullptr,
                    bool small_blocks = false);      // round 6: 256 slices (and threads) a block instead of 1024: blocks of a few tens of KB
int launch_blk_scan_store(hipStream_t st, const uint8_t *in, uint64_t nbytes, const BlkJob *jobs, uint32_t njobs,
                          BlkInfo *infos, BlkLanes *lanes, void *tabs, uint32_t *temp, BlkLanesX *lanesx);
int launch_blk_place(hipStream_t st, const BlkEmit *jobs, uint32_t njobs, const BlkLanes *lanes, const BlkLanesX *lanesx,
                     const uint32_t *temp, uint32_t *codes, uint32_t *flags, BlkUnits *units, uint32_t unit_target,
                     uint32_t *job_flags, uint32_t free_shift);
int launch_blk_emit(hipStream_t st, const uint8_t *in, uint64_t nbytes, const BlkEmit *jobs, uint32_t njobs,
                    const BlkLanes *lanes, uint32_t *codes, uint32_t *flags, BlkUnits *units, uint32_t unit_target,
                    uint32_t *job_flags = nullptr,   // job_flags[j] = 1: block j reads bytes in front of itself
                    const void *tabs = nullptr,      // tables from launch_blk_scan, indexed by BlkEmit::cand
                    uint32_t free_shift = 17,        // marker units: 2^free_shift output bytes each (>= 15)
                    bool large_blocks = false,       // the kernel instance whose lanes read their bits through LDS rings (round 5): one
                                                     // workgroup per CU, faster per symbol — for blocks of tens of thousands of codes
                    bool small_blocks = false);      // the 256-lane instance: exactly the blocks that launch_blk_scan(small_blocks) scanned
int launch_blk_materialize(hipStream_t st, const uint8_t *in, const BlkEmit *jobs, uint32_t njobs,
                           const BlkLanes *lanes, const BlkUnits *units, const uint32_t *codes, uint8_t *out,
                           uint64_t *dbg);
// the dictionary instance: a preloading job's history is BlkEmit::dict_len bytes that end at dict_end, then `out`
int launch_blk_materialize_dict(hipStream_t st, const uint8_t *in, const BlkEmit *jobs, uint32_t njobs, const BlkUnits *units,
                                const uint32_t *codes, uint8_t *out, const uint8_t *dict_end);

// marker-based materialisation (streams whose blocks read earlier blocks):
//  sym: one 16-bit symbol per output byte — a byte value, or 256 + j = byte j of the 32 KiB in front of the unit
int launch_blk_materialize_sym(hipStream_t st, const uint8_t *in, const BlkEmit *jobs, uint32_t njobs,
                               const BlkUnits *units, const uint32_t *codes, uint16_t *sym,
                               bool few_units = false /* at most one unit per CU: the 1024-lane variant */);
//  windows[u] = the final 32 KiB of output up to the end of unit u (units in stream order, one workgroup walks them)
// init_win: the 32 KiB of output in front of the first unit (a later window of a member), or null (start of a member)
int launch_window_chain(hipStream_t st, const uint16_t *sym, const SymUnit *units, uint32_t nunits, uint8_t *windows,
                        const uint8_t *init_win = nullptr);
//  the same windows by a blocked parallel prefix over the units' index maps (long streams)
size_t window_prefix_scratch_bytes(uint32_t nunits);
int launch_window_prefix(hipStream_t st, const uint16_t *sym, const SymUnit *units, uint32_t nunits, void *scratch,
                         uint8_t *windows, const uint8_t *init_win = nullptr);
//  N-GPU decode, window hand-over: a rank's slice as ONE index map on the 32 KiB in front of it (from its symbol units, or
//  from its bytes when the slice was materialised directly), and the window in front of rank `nranks` from the maps of
//  the ranks before it (maps: nranks x 32768 entries in rank order)
int launch_window_rank_map(hipStream_t st, const uint16_t *sym, const SymUnit *units, uint32_t nunits, void *scratch, uint16_t *out_map);
int launch_bytes_to_map(hipStream_t st, const uint8_t *out, uint64_t len, uint16_t *map);
int launch_window_ranks(hipStream_t st, const uint16_t *maps, uint32_t nranks, uint8_t *win);
//  out = sym with every marker replaced through the window in front of its unit
int launch_sym_substitute(hipStream_t st, const uint16_t *sym, const SymUnit *units, uint32_t nunits,
                          const uint8_t *windows, uint8_t *out, uint64_t max_len, const uint8_t *init_win = nullptr);   // max_len: longest unit

int launch_container(hipStream_t st, int format, uint32_t count, const uint8_t *in,
                     const DecStream *streams, DecHeader *hdrs);
int launch_inflate(hipStream_t st, const uint8_t *in, uint8_t *out, const InflateJob *jobs,
                   InflateResult *results, uint32_t njobs);
// the dictionary instances: a zlib header with FDICT is accepted when its DICTID is dict_id (DecHeader::flags =
// HDR_DICT), and refused with ERR_DICT_MISMATCH when not; a job's history is InflateJob::dict_len bytes that end at dict_end
int launch_container_dict(hipStream_t st, uint32_t count, const uint8_t *in, const DecStream *streams, DecHeader *hdrs,
                          uint32_t dict_id);
int launch_inflate_dict(hipStream_t st, const uint8_t *in, uint8_t *out, const InflateJob *jobs, InflateResult *results,
                        uint32_t njobs, const uint8_t *dict_end);
// The finder's survivor lists: FIND_SHARDS lists of shard_cap entries — since round 6 a list holds ONE class of survivors
// (lfx_decode_kernels.hip: FIND_CLASSES classes x FIND_SUB lists each; a device-scope counter serialises at ~11 ns per atomic,
// and a workgroup of stage 1 now adds to about ten of them instead of one).  The buffer starts with FIND_HDR_WORDS 32-bit
// words: [0, FIND_SHARDS) the lists' counts, [FIND_SHARDS] a workgroup overflowed, FIND_HDR_FINAL the number of headers stage 2
// found, FIND_HDR_WORK.. its batch counters, FIND_HDR_DBG.. seven 64-bit LFX_DEBUG counters.
constexpr uint32_t FIND_SHARDS = 256;
constexpr uint32_t FIND_HDR_WORDS = 1024, FIND_HDR_FINAL = 320, FIND_HDR_DBG = 360, FIND_HDR_READ = 512 /* words the host reads back */;
// stage 2's batch counters: FIND2_GROUPS of them, 128 bytes apart.  ONE counter for all batches was the kernel's floor: eight
// thousand device-scope atomics on one address at ~20 ns each are 0.19 ms whatever the batches cost (measured in round 6
// with batches that did nothing) — the wavefronts of group k deal the batches k, k + GROUPS, ... among themselves.
constexpr uint32_t FIND2_GROUPS = 16, FIND_HDR_WORK = 512, FIND_HDR_WORK_STRIDE = 32;
inline uint32_t find_shard_cap(uint64_t comp_bytes) {      // survivors are ~0.4 % of the bytes: room for 16 x a list's expected share
    const uint64_t want = comp_bytes / 4000;
    return (uint32_t)(want < 4096 ? 4096 : want > (1u << 23) ? (1u << 23) : want);
}
// count: FIND_SHARDS + 1 words (the last one marks a workgroup overflow)
int launch_find_stage1(hipStream_t st, const uint8_t *in, uint64_t nbytes, uint64_t first_byte,
                       uint32_t *count, uint64_t *cand, uint32_t shard_cap, uint64_t final_from_bit, uint32_t n_cu);
// survivors of the full header check are appended to final[] (final_count = number appended)
int launch_find_stage2(hipStream_t st, const uint8_t *in, uint64_t nbytes, const uint64_t *cand,
                       uint32_t shard_cap, const uint32_t *count /* device: stage 1's FIND_SHARDS + 1 words */,
                       uint32_t *work /* device, zero: the batch counter of the persistent grid */,
                       uint32_t *final_count, uint64_t *final_list, uint32_t final_cap, uint32_t n_cu,
                       uint64_t *dbg = nullptr /* device, zero: seven counters (LFX_DEBUG) */);
// multi-member decode (lfx_members.hip): gzip member candidates (1f 8b 08, reserved FLG bits clear) per tile of MEMBER_TILE
// input bytes — counted, then written in input order to the positions the host gives each tile (MEMBER_SKIP: none)
constexpr uint64_t MEMBER_TILE = 16384;
constexpr uint64_t MEMBER_SKIP = ~0ull;
inline uint64_t member_tiles(uint64_t n) { return (n + MEMBER_TILE - 1) / MEMBER_TILE; }
int launch_member_count(hipStream_t st, const uint8_t *in, uint64_t n, uint32_t *tile_count /* member_tiles(n) */);
int launch_member_emit(hipStream_t st, const uint8_t *in, uint64_t n, const uint64_t *tile_pos /* member_tiles(n) */,
                       uint64_t *out, uint64_t cap);
int launch_verify_trailers(hipStream_t st, int format, uint32_t count, const uint8_t *in,
                           const DecStream *streams, const DecHeader *hdrs, InflateResult *results,
                           const uint32_t *crc, const uint32_t *adler, uint64_t *consumed);
// lfx_decode_batch_packed_device (lfx_batch_unpack.hip): the device-wide scan of bpack_term(size, s, count, align)
// over the decoded sizes at scratch[bunpack_scratch(count).size ..], then per stream streams[].out_off / out_cap = its offset
// and size, the pairs {off, len} and behind them the total at scratch[.pairs ..] (and the pairs in `table`, device memory, when
// it is not null).  scratch: bunpack_scratch(count).words 64-bit words (lfx_batch_unpack.h).
int launch_batch_unpack_layout(hipStream_t st, DecStream *streams, uint32_t count, uint32_t align, uint64_t *scratch, uint64_t *table);
}  // namespace lfx
