// lfx_inflate_serial.inc — the text of the exact serial inflate kernel (lfx_decode_kernels.hip includes it once per instance).
//   LFX_INFLATE_KERNEL  the kernel's name
//   LFX_INFLATE_DICT    0: inflate_kernel — its text is what the kernel's was before it moved here, so its code is too;
//                       1: inflate_dict_kernel (DESIGN §17): one more argument, dict_end.  Of the job's hist_avail bytes of
//                          history, the first dict_len are the tail of a preset dictionary that ends at dict_end — somewhere
//                          else, shared by every job — and only the rest lies in front of the job's output.  A match whose
//                          source starts in front of that is resolved byte by byte: dictionary, then output.
// Why text and not a template: the plain instance must compile to the code it had as a kernel of its own, and a template body
// shared by two __global__ wrappers does not (the wrapper alone changes the register allocation of the plain kernel).
__global__ __launch_bounds__(64) void LFX_INFLATE_KERNEL(const uint8_t *__restrict__ in,
                                                     uint8_t *__restrict__ out,
                                                     const InflateJob *__restrict__ jobs,
                                                     InflateResult *__restrict__ results
#if LFX_INFLATE_DICT
                                                     , const uint8_t *__restrict__ dict_end
#endif
                                                     ) {
    __shared__ uint32_t win[WIN_BYTES / 4 + 2];
    __shared__ uint16_t lit_pri[1u << LIT_PRI], dist_pri[1u << DIST_PRI], cl_pri[128];
    __shared__ uint16_t lit_sorted[288], dist_sorted[32], cl_sorted[19];
    __shared__ uint8_t lens[640];
    __shared__ uint8_t clw[19];
    __shared__ uint32_t q[QN];
    __shared__ HuffTab T_lit, T_dist, T_cl;
    __shared__ uint32_t s_ctl[8];  // 0: queue count, 1: block done, 2: stop, 3: btype, 4: stored len
    __shared__ uint16_t l_len_base[29], l_dist_base[30];
    __shared__ uint8_t l_len_extra[29], l_dist_extra[30];
    if (threadIdx.x < 29) { l_len_base[threadIdx.x] = c_len_base[threadIdx.x]; l_len_extra[threadIdx.x] = c_len_extra[threadIdx.x]; }
    if (threadIdx.x < 30) { l_dist_base[threadIdx.x] = c_dist_base[threadIdx.x]; l_dist_extra[threadIdx.x] = c_dist_extra[threadIdx.x]; }

    const uint32_t lane = threadIdx.x;
    const InflateJob job = jobs[blockIdx.x];
    BitIn b;
    b.g = (gptr_u8)(in + job.in_off);
    b.nbits = job.in_len * 8;
    b.pos = job.start_bit;
    b.win = win;
    b.win_base = ~0ull >> 1;  // force the first fill
    b.err = 0; b.ecode = 0; b.ea0 = 0; b.ea1 = 0;
    uint8_t *o = out + job.out_off;
    const bool do_write = !(job.flags & JOB_COUNT_ONLY);
    uint64_t produced = 0;        // bytes produced by this job
    uint32_t status = 0, final_seen = 0, needs_hist = 0, nblocks = 0;
    uint64_t blk_out_start = 0, blk_start_bit = job.start_bit;
    uint64_t hist_avail = job.hist_avail;  // bytes of the member already produced before this job

    if (lane == 0) {
        T_lit.pri = lit_pri; T_lit.sorted = lit_sorted; T_lit.pri_bits = LIT_PRI;
        T_dist.pri = dist_pri; T_dist.sorted = dist_sorted; T_dist.pri_bits = DIST_PRI;
        T_cl.pri = cl_pri; T_cl.sorted = cl_sorted; T_cl.pri_bits = 7;
    }
    __syncthreads();

    for (;;) {
        // ---- block header: deflate::Decoder::read decode.rs:146-162
        blk_out_start = produced;
        blk_start_bit = b.pos;
        win_ensure(b, 700, lane);
        if (lane == 0) {
            s_ctl[2] = 0;
            const uint32_t bfinal = bi_read_unchecked(b, 1);
            uint32_t btype = 0;
            if (!b.err) btype = bi_read_unchecked(b, 2);
            if (b.err) s_ctl[2] = 1;
            s_ctl[3] = btype;
            s_ctl[5] = bfinal;
        }
        __syncthreads();
        b.pos = __shfl(b.pos, 0);
        if (s_ctl[2]) break;
        const uint32_t btype = s_ctl[3];
        final_seen = s_ctl[5];
        nblocks++;
        if (btype == 3) {
            if (lane == 0) { b.err = 1; b.ecode = ERR_BTYPE3; }
            break;
        }
        if (btype == 0) {
            // read_non_compressed_block decode.rs:81-111
            uint64_t byte = (b.pos + 7) >> 3;  // bit_reader.reset(): drop the partial byte
            const uint64_t nb = job.in_len;
            uint32_t len = 0;
            int bad = 0;
            if (nb < byte || nb - byte < 2) { bad = 2; byte = nb; }
            else {
                len = ld1(b.g + byte) | ld1(b.g + byte + 1) << 8;
                byte += 2;
                if (nb - byte < 2) { bad = 2; byte = nb; }
                else {
                    const uint32_t nlen = ld1(b.g + byte) | ld1(b.g + byte + 1) << 8;
                    byte += 2;
                    if (((~len) & 0xFFFF) != nlen) { bad = 1; b.ea0 = len; b.ea1 = nlen; }
                }
            }
            if (bad) {
                if (lane == 0) { b.err = bad; b.ecode = bad == 2 ? ERR_EOF : ERR_LEN_NLEN; }
                b.pos = byte << 3;
                break;
            }
            const uint64_t avail = nb - byte;
            const uint32_t take = len < avail ? len : (uint32_t)avail;
            if (do_write) {
                if (produced + take > job.out_cap) { if (lane == 0) { b.err = 3; b.ecode = ERR_NOSPACE; } break; }
                for (uint32_t k = lane; k < take; k += 64) o[produced + k] = b.g[byte + k];
                __threadfence_block();
            }
            produced += take;
            b.pos = (byte + take) << 3;
            if (take != len) {
                if (lane == 0) { b.err = 2; b.ecode = ERR_STORED_SHORT; b.ea0 = len; b.ea1 = take; }
                break;
            }
        } else {
            // ---- code tables
            int rc = 0;
            uint32_t csym = 0;
            uint32_t nl = 288, nd = 30;
            if (btype == 1) {
                // FixedHuffmanCodec::load symbol.rs:290-315
                for (uint32_t s = lane; s < 288; s += 64) lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
                for (uint32_t s = lane; s < 30; s += 64) lens[288 + s] = 5;
                __syncthreads();
            } else {
                // DynamicHuffmanCodec::load symbol.rs:387-456 (checked reads)
                if (lane == 0) {
                    s_ctl[2] = 0;
                    uint32_t hl = bi_read_unchecked(b, 5);
                    uint32_t hd = b.err ? 0 : bi_read_unchecked(b, 5);
                    uint32_t hc = b.err ? 0 : bi_read_unchecked(b, 4);
                    if (b.err) s_ctl[2] = 1;
                    else if (hd + 1 > 30) { b.err = 1; b.ecode = ERR_HDIST; b.ea0 = hd + 1; s_ctl[2] = 1; }
                    else {
                        for (int k = 0; k < 19; ++k) clw[k] = 0;
                        for (uint32_t k = 0; k < hc + 4 && !b.err; ++k) clw[c_clen_order[k]] = (uint8_t)bi_read_unchecked(b, 3);
                        if (b.err) s_ctl[2] = 1;
                    }
                    s_ctl[6] = hl + 257;
                    s_ctl[7] = hd + 1;
                }
                __syncthreads();
                if (s_ctl[2]) break;
                nl = s_ctl[6]; nd = s_ctl[7];
                rc = tab_build(T_cl, clw, 19, 1, 1, -1, lane, &csym);
                if (rc) { if (lane == 0) { b.err = 1; b.ecode = ERR_CONFLICT; b.ea0 = csym; } break; }
                if (lane == 0) {
                    // code length sequences (load_bitwidthes symbol.rs:459-484); one contiguous array:
                    // literal overflow spills into the distance list (symbol.rs:422-424)
                    uint32_t have = 0;
                    s_ctl[2] = 0;
                    for (int phase = 0; phase < 2 && !s_ctl[2]; ++phase) {
                        const uint32_t target = phase ? nl + nd : nl;
                        while (have < target) {
                            const uint32_t c = tab_decode(T_cl, b);
                            if (b.err) { s_ctl[2] = 1; break; }
                            if (c <= 15) lens[have++] = (uint8_t)c;
                            else if (c == 16) {
                                const uint32_t r = bi_read_unchecked(b, 2);
                                if (b.err) { s_ctl[2] = 1; break; }
                                if (have == 0) { b.err = 1; b.ecode = ERR_NO_PREV; s_ctl[2] = 1; break; }
                                const uint8_t last = lens[have - 1];
                                for (uint32_t k = 0; k < r + 3; ++k) lens[have++] = last;
                            } else if (c == 17) {
                                const uint32_t r = bi_read_unchecked(b, 3);
                                if (b.err) { s_ctl[2] = 1; break; }
                                for (uint32_t k = 0; k < r + 3; ++k) lens[have++] = 0;
                            } else {
                                const uint32_t r = bi_read_unchecked(b, 7);
                                if (b.err) { s_ctl[2] = 1; break; }
                                for (uint32_t k = 0; k < r + 11; ++k) lens[have++] = 0;
                            }
                        }
                    }
                    if (!s_ctl[2] && have - nl > nd) {
                        b.err = 1; b.ecode = ERR_DIST_LIST; b.ea0 = have - nl; b.ea1 = nd; s_ctl[2] = 1;
                    }
                }
                __syncthreads();
                if (s_ctl[2]) break;
            }
            const uint32_t dist_at = btype == 1 ? 288 : nl;
            rc = tab_build(T_lit, lens, nl, 0, 0, 256, lane, &csym);
            if (rc) { if (lane == 0) { b.err = 1; b.ecode = ERR_CONFLICT; b.ea0 = csym; } break; }
            rc = tab_build(T_dist, lens + dist_at, nd, 1, T_lit.safe_bw, -1, lane, &csym);
            if (rc) { if (lane == 0) { b.err = 1; b.ecode = ERR_CONFLICT; b.ea0 = csym; } break; }
            // ---- symbols: read_compressed_block decode.rs:112-130
            bool stop = false, nospace = false;
            for (;;) {
                win_ensure(b, QN * 6 + 16, lane);
                if (lane == 0) {
                    uint32_t n = 0, done = 0;
                    uint64_t prod = produced;
                    while (n < QN) {
                        // symbol::Decoder::decode_unchecked symbol.rs:193-244
                        const uint32_t d = tab_decode(T_lit, b);
                        uint32_t entry;
                        bool eob = false;
                        if (d <= 255) entry = d;
                        else if (d == 256) { eob = true; entry = 0; }
                        else if (d >= 286) { b.err = 1; b.ecode = ERR_286; b.ea0 = d; eob = true; entry = 0; }
                        else {
                            const uint32_t length = l_len_base[d - 257] + bi_read_unchecked(b, l_len_extra[d - 257]);
                            const uint32_t dc = tab_decode(T_dist, b);
                            const uint32_t distance = l_dist_base[dc % 30] + bi_read_unchecked(b, l_dist_extra[dc % 30]);
                            entry = 0x80000000u | (length << 16) | distance;  // distance <= 32768 fits 16 bits
                            if (!b.err) {
                                // Lz77Decoder::decode lib.rs:173-185
                                const uint64_t blen = hist_avail + prod;
                                if (blen < distance) {
                                    if (job.flags & JOB_SINGLE_BLOCK && (job.flags & JOB_COUNT_ONLY)) {
                                        needs_hist = 1;  // history unknown in the speculative pass
                                    } else {
                                        b.err = 1; b.ecode = ERR_BACKREF; b.ea0 = (uint32_t)blen; b.ea1 = distance;
                                    }
                                }
                            }
                            if (!b.err) prod += length;
                        }
                        if (b.err) { done = 2; break; }  // check_last_error after every symbol
                        if (eob) { done = 1; break; }
                        if (d <= 255) prod += 1;
                        q[n++] = entry;
                    }
                    s_ctl[0] = n;
                    s_ctl[1] = done;
                }
                __syncthreads();
                b.pos = __shfl(b.pos, 0);
                needs_hist = __shfl(needs_hist, 0);
                const uint32_t n = s_ctl[0], done = s_ctl[1];
                // ---- materialise the queue
                const uint32_t e = lane < n ? q[lane] : 0;
                const bool is_match = lane < n && (e >> 31);
                const uint32_t mylen = lane < n ? (is_match ? ((e >> 16) & 0x1FF) : 1) : 0;
                uint32_t x = mylen;  // inclusive scan
                for (int ofs = 1; ofs < 64; ofs <<= 1) {
                    const uint32_t y = __shfl_up(x, ofs);
                    if ((int)lane >= ofs) x += y;
                }
                const uint32_t total = __shfl(x, 63);
                const uint64_t at = produced + x - mylen;
                if (do_write && n) {
                    if (produced + total > job.out_cap) { if (lane == 0) { b.err = 3; b.ecode = ERR_NOSPACE; } stop = true; nospace = true; }
                    else {
                        if (lane < n && !is_match) o[at] = (uint8_t)e;
                        __threadfence_block();
                        uint64_t mm = __ballot(is_match);
                        while (mm) {
                            const uint32_t src_lane = (uint32_t)__builtin_ctzll(mm);
                            mm &= mm - 1;
                            const uint32_t me = __shfl(e, src_lane);
                            const uint64_t mat = __shfl(at, src_lane);
                            const uint32_t len = (me >> 16) & 0x1FF;
                            const uint32_t dist = me & 0xFFFF;
                            const uint8_t *srcp = o + mat - dist;
#if LFX_INFLATE_DICT
                            {
                                // bytes of the member that lie in front of `o` (a whole stream: none); the source starts
                                // `into` bytes inside the dictionary's tail (the reach check above: into <= dict_len)
                                const uint64_t own = job.hist_avail - job.dict_len;
                                if (mat + own < dist) {
                                    const uint32_t into = (uint32_t)(dist - (mat + own));
                                    for (uint32_t k = lane; k < len; k += 64) {
                                        const uint32_t j = dist >= len ? k : k % dist;      // src[k mod dist], as below
                                        o[mat + k] = j < into ? dict_end[(int64_t)j - (int64_t)into] : srcp[j];
                                    }
                                    __threadfence_block();
                                    continue;
                                }
                            }
#endif
                            // out[k] = src[k mod dist] reproduces the overlapping forward copy (rle_decode)
                            if (dist >= len) { for (uint32_t k = lane; k < len; k += 64) o[mat + k] = srcp[k]; }
                            else { for (uint32_t k = lane; k < len; k += 64) o[mat + k] = srcp[k % dist]; }
                            __threadfence_block();
                        }
                    }
                }
                if (!nospace) produced += total;  // never report bytes that were not written
                __syncthreads();
                if (stop || done) { if (done == 2) stop = true; break; }
            }
            if (stop) break;
        }
        if (final_seen || (job.flags & JOB_SINGLE_BLOCK)) break;
        if (job.stop_bit != 0 && b.pos == job.stop_bit) break;   // end of a shard that holds no BFINAL block
    }
    // ---- result
    b.err = __shfl(b.err, 0);
    if (lane == 0) {
        status = b.err;
        InflateResult r;
        r.end_bit = b.pos;
        r.out_len = produced;
        r.status = status;
        r.final_seen = final_seen;
        r.err = b.ecode; r.a0 = b.ea0; r.a1 = b.ea1;
        r.needs_hist = needs_hist;
        r.nblocks = nblocks;
        r._pad = 0;
        r.blk_out_start = blk_out_start;
        r.blk_start_bit = blk_start_bit;
        results[blockIdx.x] = r;
    }
}
