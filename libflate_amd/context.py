"""Device context (lfx_ctx): one per GPU, owns a HIP stream and cached HBM scratch."""
import ctypes as C

from . import _ffi


class Context:
    def __init__(self, device=0):
        st = C.c_int(0)
        self._h = _ffi.lib().lfx_ctx_new(device, C.byref(st))
        if not self._h:
            raise _ffi.DeviceError(st.value, "no usable MI355X device %d (there is no CPU fallback)" % device)
        self.device = device
        self._users = 0          # native handles (encoders, decoders, LZ77 encoders) made from this context and not yet freed
        self._closing = False

    # A native handle uses its context until it is freed (it takes the context's mutex in lfx_*_free).  A Python reference from
    # the handle's wrapper to this object is not enough: the garbage collector runs the finalizers of an unreachable group in
    # an undefined order (PEP 442) — at interpreter exit Context.__del__ ran before a decoder's, whose free then locked a mutex
    # in freed memory ("std::system_error: Invalid argument" under MALLOC_PERTURB_, a corrupted heap without).  So the wrappers
    # count themselves in and out, and the native context is freed by whoever comes last.
    def _retain(self):
        self._users += 1

    def _release(self):
        self._users -= 1
        if self._users <= 0 and self._closing:
            self._free_now()

    def _free_now(self):
        if self._h:
            _ffi.lib().lfx_ctx_free(self._h)
            self._h = None

    def close(self):
        self._closing = True
        if self._users <= 0:
            self._free_now()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def last_error(self):
        return (_ffi.lib().lfx_ctx_last_error(self._h) or b"").decode("utf-8", "replace")

    def set_stream(self, hip_stream_ptr):
        _ffi.lib().lfx_ctx_set_stream(self._h, hip_stream_ptr)

    def enable_timing(self, on=True):
        """True / 1: an event behind every phase; 2..5: only the two events around one kernel's phase (2: lz77_walk, 3: blk_scan,
        4: lz77_cand, 5: lz77_copy); 6: every phase, the encode's match and parse phases split by kernel; False / 0: none."""
        _ffi.lib().lfx_ctx_enable_timing(self._h, int(on) if on is not True and on is not False and 2 <= int(on) <= 6 else (1 if on else 0))

    def last_timing(self):
        t = _ffi.Timing()
        if _ffi.lib().lfx_ctx_last_timing(self._h, C.byref(t)) != 0:
            return None
        return {"total_ms": t.total_ms,
                "phases": [(bytes(t.phase_name[i]).split(b"\0")[0].decode(), t.phase_ms[i])
                           for i in range(t.n_phases)]}

    def match_fallbacks(self):
        """encode passes that ran on the fallback match kernel (lfx_ctx_match_fallbacks): 0 unless the default kernel's
        hardware assumption was seen violated on this part"""
        return int(_ffi.lib().lfx_ctx_match_fallbacks(self._h))

    # ---- one-shot calls on raw HOST pointers (ints: numpy buffers, lfx_host_alloc blocks) — no Python-side copies --------
    def encode_host_ptr(self, fmt, in_ptr, n, out_ptr, cap, opts=None, schedule=None):
        out_len = C.c_uint64(0)
        rc = _ffi.lib().lfx_encode_host(self._h, fmt, C.byref(opts) if opts is not None else None,
                                        C.byref(schedule) if schedule is not None else None, in_ptr, n, out_ptr, cap, C.byref(out_len))
        if rc:
            raise (_ffi.DeviceError if rc == _ffi.E_DEVICE else _ffi.LfxError)(rc, self.last_error())
        return out_len.value

    def decode_host_ptr(self, fmt, in_ptr, n, out_ptr, cap, flags=0):
        """→ (status, out_len, consumed, message)"""
        out_len, consumed = C.c_uint64(0), C.c_uint64(0)
        rc = _ffi.lib().lfx_decode_host(self._h, fmt, flags, in_ptr, n, out_ptr, cap, C.byref(out_len), C.byref(consumed))
        if rc in (_ffi.E_DEVICE, _ffi.E_OOM, _ffi.E_ARG):
            raise (_ffi.DeviceError if rc == _ffi.E_DEVICE else _ffi.LfxError)(rc, self.last_error())
        return rc, out_len.value, consumed.value, self.last_error() if rc else ""

    # ---- one-shot calls on raw device pointers (ints) -------------------------------------------
    def encode_device(self, fmt, d_in, n, d_out, cap, opts=None, schedule=None):
        out_len = C.c_uint64(0)
        rc = _ffi.lib().lfx_encode_device(self._h, fmt, C.byref(opts) if opts is not None else None,
                                          C.byref(schedule) if schedule is not None else None,
                                          d_in, n, d_out, cap, C.byref(out_len))
        if rc:
            raise (_ffi.DeviceError if rc == _ffi.E_DEVICE else _ffi.LfxError)(rc, self.last_error())
        return out_len.value

    def encode_index_device(self, fmt, d_in, n, d_out, cap, opts=None, schedule=None, spacing=1 << 20):
        """lfx_encode_device plus a seek index of the stream it writes (lfx_encode_index_device) → (out_len, index_handle);
        index_handle is a native lfx_index* — libflate_amd.index.Index wraps it.  Raises as encode_device does."""
        out_len, h = C.c_uint64(0), C.c_void_p(None)
        rc = _ffi.lib().lfx_encode_index_device(self._h, fmt, C.byref(opts) if opts is not None else None,
                                                C.byref(schedule) if schedule is not None else None,
                                                d_in, n, d_out, cap, C.byref(out_len), spacing, C.byref(h))
        if rc:
            raise (_ffi.DeviceError if rc == _ffi.E_DEVICE else _ffi.LfxError)(rc, self.last_error())
        return out_len.value, h.value

    def decode_device(self, fmt, d_in, n, d_out, cap, flags=0):
        """→ (status, out_len, consumed, message)"""
        out_len, consumed = C.c_uint64(0), C.c_uint64(0)
        rc = _ffi.lib().lfx_decode_device(self._h, fmt, flags, d_in, n, d_out, cap, C.byref(out_len),
                                          C.byref(consumed))
        if rc in (_ffi.E_DEVICE, _ffi.E_OOM, _ffi.E_ARG):
            raise (_ffi.DeviceError if rc == _ffi.E_DEVICE else _ffi.LfxError)(rc, self.last_error())
        return rc, out_len.value, consumed.value, self.last_error() if rc else ""

    def decode_members_device(self, d_in, n, d_out, cap, max_members=None):
        """gzip::MultiDecoder over device bytes, the members decoded as one batch (lfx_decode_members_device)
        → (status, out_len, consumed, members, message); members = [(in_off, in_len, out_off, out_len)] of the verified
        members, at most max_members of them (None: room for every member n bytes can hold)"""
        return self._members(_ffi.lib().lfx_decode_members_device, d_in, n, d_out, cap, max_members)

    def decode_index_device(self, fmt, d_in, n, d_out, cap, spacing=1 << 20, flags=0):
        """lfx_decode_device plus a seek index (lfx_decode_index_device) → (status, out_len, consumed, index_handle, message);
        index_handle is a native lfx_index* (None unless status is 0) — libflate_amd.index.Index wraps it"""
        out_len, consumed, h = C.c_uint64(0), C.c_uint64(0), C.c_void_p(None)
        rc = _ffi.lib().lfx_decode_index_device(self._h, fmt, flags, d_in, n, d_out, cap, C.byref(out_len), C.byref(consumed),
                                                spacing, C.byref(h))
        if rc in (_ffi.E_DEVICE, _ffi.E_OOM, _ffi.E_ARG):
            raise (_ffi.DeviceError if rc == _ffi.E_DEVICE else _ffi.LfxError)(rc, self.last_error())
        return rc, out_len.value, consumed.value, h.value, self.last_error() if rc else ""

    def index_read_device(self, index_handle, d_in, in_base, n, offs, lens, d_out, out_offs):
        """count reads through a seek index (lfx_index_read_device) → (status, out_lens, statuses, message)"""
        k = len(offs)
        a = lambda v: (C.c_uint64 * max(k, 1))(*v)
        o, ln, oo = a(offs), a(lens), a(out_offs)
        out_len, st = (C.c_uint64 * max(k, 1))(), (C.c_int32 * max(k, 1))()
        rc = _ffi.lib().lfx_index_read_device(self._h, index_handle, d_in, in_base, n, k, o, ln, d_out, oo, out_len, st)
        if rc in (_ffi.E_DEVICE, _ffi.E_OOM) or (rc == _ffi.E_ARG and not any(st[i] == _ffi.E_ARG for i in range(k))):
            raise (_ffi.DeviceError if rc == _ffi.E_DEVICE else _ffi.LfxError)(rc, self.last_error())
        return rc, list(out_len[:k]), list(st[:k]), self.last_error() if rc else ""

    def _members(self, fn, src, n, dst, cap, max_members):
        if max_members is None:
            max_members = n // 20 + 1           # (a gzip member takes at least 20 bytes)
        table = (_ffi.Member * max(int(max_members), 1))()
        out_len, consumed, count = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
        rc = fn(self._h, src, n, dst, cap, C.byref(out_len), C.byref(consumed), table, int(max_members), C.byref(count))
        if rc in (_ffi.E_DEVICE, _ffi.E_OOM, _ffi.E_ARG):
            raise (_ffi.DeviceError if rc == _ffi.E_DEVICE else _ffi.LfxError)(rc, self.last_error())
        members = [(m.in_off, m.in_len, m.out_off, m.out_len) for m in table[:min(count.value, int(max_members))]]
        return rc, out_len.value, consumed.value, members, self.last_error() if rc else ""

    def decode_members_host(self, data, cap=None, max_members=None):
        """the same on host bytes (lfx_decode_members_host) → (status, output_so_far, consumed, members, message); like
        decode_host, a cap left to None grows while the output does not fit"""
        data = bytes(data)
        grow = cap is None
        cap = cap if cap is not None else max(1 << 16, len(data) * 16)
        while True:
            out = C.create_string_buffer(cap)
            rc, ol, used, members, msg = self._members(_ffi.lib().lfx_decode_members_host, data, len(data), out, cap, max_members)
            if grow and rc == _ffi.E_NOSPACE and cap < len(data) * 1040 + (1 << 20):
                cap *= 8
                continue
            return rc, out.raw[:ol], used, members, msg

    # ---- BGZF reads by virtual offset (lfx_bgzf_read_*) ---------------------------------------------
    @staticmethod
    def _bgzf_reads(reads):
        """reads: (voff, length, end_voff, out_off) each → the lfx_bgzf_read array"""
        k = len(reads)
        arr = (_ffi.BgzfRead * max(k, 1))()
        for i, (voff, length, end_voff, out_off) in enumerate(reads):
            arr[i].voff, arr[i].len, arr[i].end_voff, arr[i].out_off = voff, length, end_voff, out_off
        return arr

    def _bgzf_call(self, fn, src, in_base, n, reads, arr, dst):
        k = len(reads)
        res = (_ffi.BgzfResult * max(k, 1))()
        res[0].status = unwritten = 0x7fffffff          # (no LFX_* code)
        decoded = C.c_uint64(0)
        rc = fn(self._h, src, in_base, n, k, arr, dst, res, C.byref(decoded))
        # LFX_E_ARG is a read's own verdict (a coffset outside the bytes held) or a refusal of the whole call; res is written
        # all at once and a refused call leaves it as it was (include/lfx.h, rule 8)
        if rc in (_ffi.E_DEVICE, _ffi.E_OOM) or (rc == _ffi.E_ARG and res[0].status == unwritten):
            raise (_ffi.DeviceError if rc == _ffi.E_DEVICE else _ffi.LfxError)(rc, self.last_error())
        out = [(r.out_len, r.next_voff, r.status, r.n_blocks) for r in res[:k]]
        return rc, out, decoded.value, self.last_error() if rc else ""

    def bgzf_read_device(self, d_in_ptr, in_base, n, reads, d_out_ptr):
        """`reads` of a BGZF file by virtual offset (lfx_bgzf_read_device): d_in_ptr holds file bytes [in_base, in_base + n),
        reads = [(voff, length, end_voff, out_off)], the bytes go to d_out_ptr + out_off (d_out_ptr = None: size mode)
        → (rc, [(out_len, next_voff, status, n_blocks)], blocks_decoded, None, message)"""
        rc, out, decoded, msg = self._bgzf_call(_ffi.lib().lfx_bgzf_read_device, d_in_ptr, in_base, n, reads, self._bgzf_reads(reads),
                                                d_out_ptr)
        return rc, out, decoded, None, msg

    def bgzf_read_host(self, data, reads, in_base=0, sizes_only=False):
        """the same on host bytes (lfx_bgzf_read_host; only the covered blocks are uploaded): reads = [(voff, length)] or [(voff,
        length, end_voff)] → (rc, [(out_len, next_voff, status, n_blocks)], blocks_decoded, [bytes per read] or None, message)"""
        data = bytes(data)
        full, at = [], 0
        for r in reads:
            full.append((r[0], r[1], r[2] if len(r) > 2 else _ffi.VOFF_NONE, at))
            at += r[1]
        buf = None if sizes_only else C.create_string_buffer(max(at, 1))
        rc, out, decoded, msg = self._bgzf_call(_ffi.lib().lfx_bgzf_read_host, data, in_base, len(data), full, self._bgzf_reads(full), buf)
        got = None if sizes_only else [buf.raw[f[3]:f[3] + o[0]] for f, o in zip(full, out)]
        return rc, out, decoded, got, msg

    def _raise_fatal(self, rc):
        if rc in (_ffi.E_DEVICE, _ffi.E_OOM, _ffi.E_ARG):
            raise (_ffi.DeviceError if rc == _ffi.E_DEVICE else _ffi.LfxError)(rc, self.last_error())

    def decode_size_device(self, fmt, d_in, n, flags=0):
        """what decode_device would report with a large enough cap, without an output buffer (lfx_decode_size_device; the
        checksums are not computed) → (status, out_len, consumed, message)"""
        out_len, consumed = C.c_uint64(0), C.c_uint64(0)
        rc = _ffi.lib().lfx_decode_size_device(self._h, fmt, flags, d_in, n, C.byref(out_len), C.byref(consumed))
        self._raise_fatal(rc)
        return rc, out_len.value, consumed.value, self.last_error() if rc else ""

    def decode_size_host(self, fmt, data, flags=0):
        """the same on host bytes (lfx_decode_size_host) → (status, out_len, consumed, message)"""
        data = bytes(data)
        out_len, consumed = C.c_uint64(0), C.c_uint64(0)
        rc = _ffi.lib().lfx_decode_size_host(self._h, fmt, flags, data, len(data), C.byref(out_len), C.byref(consumed))
        self._raise_fatal(rc)
        return rc, out_len.value, consumed.value, self.last_error() if rc else ""

    def decode_batch_size_device(self, fmt, d_in, in_offs, in_lens):
        """the decoded sizes of len(in_offs) independent streams (lfx_decode_batch_size_device) → (out_lens, consumed, statuses):
        what decode_batch_device needs as out_caps"""
        k = len(in_offs)
        a = lambda v: (C.c_uint64 * max(k, 1))(*v)
        io, il = a(in_offs), a(in_lens)
        ol, used, st = (C.c_uint64 * max(k, 1))(), (C.c_uint64 * max(k, 1))(), (C.c_int32 * max(k, 1))()
        rc = _ffi.lib().lfx_decode_batch_size_device(self._h, fmt, k, d_in, io, il, ol, used, st)
        if rc:
            raise (_ffi.DeviceError if rc == _ffi.E_DEVICE else _ffi.LfxError)(rc, self.last_error())
        return list(ol[:k]), list(used[:k]), list(st[:k])

    def _members_size(self, fn, src, n, max_members):
        if max_members is None:
            max_members = n // 20 + 1           # (a gzip member takes at least 20 bytes)
        table = (_ffi.Member * max(int(max_members), 1))()
        out_len, consumed, count = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
        rc = fn(self._h, src, n, C.byref(out_len), C.byref(consumed), table, int(max_members), C.byref(count))
        self._raise_fatal(rc)
        members = [(m.in_off, m.in_len, m.out_off, m.out_len) for m in table[:min(count.value, int(max_members))]]
        return rc, out_len.value, consumed.value, members, self.last_error() if rc else ""

    def decode_members_size_device(self, d_in, n, max_members=None):
        """the member table and total size decode_members_device would report, without an output buffer
        (lfx_decode_members_size_device) → (status, out_len, consumed, members, message)"""
        return self._members_size(_ffi.lib().lfx_decode_members_size_device, d_in, n, max_members)

    def decode_members_size_host(self, data, max_members=None):
        """the same on host bytes (lfx_decode_members_size_host)"""
        data = bytes(data)
        return self._members_size(_ffi.lib().lfx_decode_members_size_host, data, len(data), max_members)

    def _encode_members(self, fn, src, n, dst, cap, member_size, flags, opts, schedule, max_members):
        count = 0 if (flags & _ffi.MEMBERS_BGZF and n == 0) else max(1, -(-n // member_size)) if member_size else 0
        if max_members is None:
            max_members = count
        table = (_ffi.Member * max(int(max_members), 1))()
        out_len, got = C.c_uint64(0), C.c_uint32(0)
        rc = fn(self._h, C.byref(opts) if opts is not None else None, C.byref(schedule) if schedule is not None else None,
                member_size, flags, src, n, dst, cap, C.byref(out_len), table, int(max_members), C.byref(got))
        if rc in (_ffi.E_DEVICE, _ffi.E_OOM, _ffi.E_ARG, _ffi.E_UNSUPPORTED):
            raise (_ffi.DeviceError if rc == _ffi.E_DEVICE else _ffi.LfxError)(rc, self.last_error())
        members = [(m.in_off, m.in_len, m.out_off, m.out_len) for m in table[:min(got.value, int(max_members))]]
        return rc, out_len.value, got.value, members, self.last_error() if rc else ""

    def encode_members_device(self, d_in, n, d_out, cap, member_size=1 << 20, flags=0, opts=None, schedule=None, max_members=None):
        """device bytes as gzip members lying back to back, all encoded in one launch set (lfx_encode_members_device;
        flags = _ffi.MEMBERS_BGZF: BGZF) → (status, out_len, n_members, members, message); members = [(in_off, in_len, out_off,
        out_len)]: the slice in d_in, the member in d_out — at most max_members of them (None: all)"""
        return self._encode_members(_ffi.lib().lfx_encode_members_device, d_in, n, d_out, cap, member_size, flags, opts, schedule,
                                    max_members)

    def encode_members_host(self, data, member_size=1 << 20, flags=0, opts=None, schedule=None, cap=None, max_members=None):
        """the same on host bytes (lfx_encode_members_host) → (status, output, n_members, members, message); cap = None: the bound"""
        data = bytes(data)
        if cap is None:
            cap = _ffi.lib().lfx_encode_members_bound(len(data), member_size, flags, C.byref(opts) if opts is not None else None,
                                                      C.byref(schedule) if schedule is not None else None)
        out = C.create_string_buffer(max(cap, 1))
        rc, ol, count, members, msg = self._encode_members(_ffi.lib().lfx_encode_members_host, data, len(data), out, cap, member_size,
                                                           flags, opts, schedule, max_members)
        return rc, out.raw[:ol], count, members, msg

    def encode_host(self, fmt, data, opts=None, schedule=None):
        data = bytes(data)
        bound = _ffi.lib().lfx_encode_bound(len(data), C.byref(opts) if opts is not None else None,
                                            C.byref(schedule) if schedule is not None else None)
        if bound == 0:
            raise _ffi.LfxError(_ffi.E_ARG, "option outside the reference's domain")
        out = C.create_string_buffer(bound)
        out_len = C.c_uint64(0)
        rc = _ffi.lib().lfx_encode_host(self._h, fmt, C.byref(opts) if opts is not None else None,
                                        C.byref(schedule) if schedule is not None else None,
                                        data, len(data), out, bound, C.byref(out_len))
        if rc:
            raise (_ffi.DeviceError if rc == _ffi.E_DEVICE else _ffi.LfxError)(rc, self.last_error())
        return out.raw[:out_len.value]

    def decode_host(self, fmt, data, cap=None, flags=0):
        """→ (status, output_so_far, consumed, message)"""
        data = bytes(data)
        cap = cap if cap is not None else max(1 << 16, len(data) * 16)
        while True:
            out = C.create_string_buffer(cap)
            out_len, consumed = C.c_uint64(0), C.c_uint64(0)
            rc = _ffi.lib().lfx_decode_host(self._h, fmt, flags, data, len(data), out, cap,
                                            C.byref(out_len), C.byref(consumed))
            if rc in (_ffi.E_DEVICE, _ffi.E_OOM, _ffi.E_ARG):
                raise (_ffi.DeviceError if rc == _ffi.E_DEVICE else _ffi.LfxError)(rc, self.last_error())
            if rc == _ffi.E_NOSPACE and cap < len(data) * 1040 + (1 << 20):
                cap *= 8
                continue
            return rc, out.raw[:out_len.value], consumed.value, self.last_error() if rc else ""

    # ---- preset dictionaries (lfx_decode_dict_*) ------------------------------------------
    @staticmethod
    def _dict_handle(zdict):
        return zdict.handle if zdict is not None else None

    def decode_dict_device(self, fmt, zdict, d_in, n, d_out, cap):
        """lfx_decode_dict_device: zlib / raw DEFLATE with a Dictionary (None: exactly decode_device)
        → (status, out_len, consumed, message)"""
        out_len, consumed = C.c_uint64(0), C.c_uint64(0)
        rc = _ffi.lib().lfx_decode_dict_device(self._h, fmt, self._dict_handle(zdict), d_in, n, d_out, cap, C.byref(out_len),
                                               C.byref(consumed))
        if rc in (_ffi.E_DEVICE, _ffi.E_OOM, _ffi.E_ARG):
            raise (_ffi.DeviceError if rc == _ffi.E_DEVICE else _ffi.LfxError)(rc, self.last_error())
        return rc, out_len.value, consumed.value, self.last_error() if rc else ""

    def decode_dict_host(self, fmt, zdict, data, cap=None):
        """lfx_decode_dict_host → (status, output_so_far, consumed, message); a cap left to None grows while the output does
        not fit, as in decode_host"""
        data = bytes(data)
        grow = cap is None
        cap = cap if cap is not None else max(1 << 16, len(data) * 16)
        while True:
            out = C.create_string_buffer(cap)
            out_len, consumed = C.c_uint64(0), C.c_uint64(0)
            rc = _ffi.lib().lfx_decode_dict_host(self._h, fmt, self._dict_handle(zdict), data, len(data), out, cap,
                                                 C.byref(out_len), C.byref(consumed))
            if rc in (_ffi.E_DEVICE, _ffi.E_OOM, _ffi.E_ARG):
                raise (_ffi.DeviceError if rc == _ffi.E_DEVICE else _ffi.LfxError)(rc, self.last_error())
            if grow and rc == _ffi.E_NOSPACE and cap < len(data) * 1040 + (1 << 20):
                cap *= 8
                continue
            return rc, out.raw[:out_len.value], consumed.value, self.last_error() if rc else ""

    def decode_batch_dict_device(self, fmt, zdict, d_in, in_offs, in_lens, d_out, out_offs, out_caps):
        """lfx_decode_batch_dict_device: the streams d_in[in_offs[i], +in_lens[i]) into d_out[out_offs[i], +out_caps[i]), one
        Dictionary for all of them; the offsets and lengths are host-side lists → [(status, out_len)] per stream"""
        k = len(in_offs)
        a = lambda v: (C.c_uint64 * max(k, 1))(*v)
        io, il, oo, oc = a(in_offs), a(in_lens), a(out_offs), a(out_caps)
        out_len, st = (C.c_uint64 * max(k, 1))(), (C.c_int32 * max(k, 1))()
        rc = _ffi.lib().lfx_decode_batch_dict_device(self._h, fmt, self._dict_handle(zdict), k, d_in, io, il, d_out, oo, oc, out_len, st)
        if rc:
            raise (_ffi.DeviceError if rc == _ffi.E_DEVICE else _ffi.LfxError)(rc, self.last_error())
        return [(st[i], out_len[i]) for i in range(k)]

    # ---- training a preset dictionary (lfx_dict_train_*) --------------------------------
    def _dict_train(self, fn, src, offs, lens, size, segment, dst, cap):
        k = len(offs)
        a = lambda v: (C.c_uint64 * max(k, 1))(*v)
        got = C.c_uint64(0)
        rc = fn(self._h, src, k, a(offs), a(lens), size, segment, dst, cap, C.byref(got))
        if rc:
            raise (_ffi.DeviceError if rc == _ffi.E_DEVICE else _ffi.LfxError)(rc, self.last_error())
        return got.value

    def dict_train_device(self, d_samples, offs, lens, size, segment, d_dict, cap):
        """lfx_dict_train_device: a dictionary of at most `size` bytes trained from the records d_samples[offs[i], +lens[i]) into
        d_dict[0, cap), cap >= size; the offsets and lengths are host-side lists, ascending and not overlapping → its length"""
        return self._dict_train(_ffi.lib().lfx_dict_train_device, d_samples, offs, lens, size, segment, d_dict, cap)

    def dict_train_host(self, data, offs, lens, size, segment=128):
        """lfx_dict_train_host: the records data[offs[i], +lens[i]) of host bytes → the dictionary"""
        data = bytes(data)
        out = C.create_string_buffer(max(size, 1))
        n = self._dict_train(_ffi.lib().lfx_dict_train_host, data, offs, lens, size, segment, out, size)
        return out.raw[:n]

    # ---- the byte-shuffle filter for numeric records (lfx_shuffle_*) --------------------
    def _shuffle_rc(self, rc):
        if rc:
            raise (_ffi.DeviceError if rc == _ffi.E_DEVICE else _ffi.LfxError)(rc, self.last_error())

    def shuffle_device(self, d_in, n, d_out, elem_size, inverse=False):
        """lfx_shuffle_device: d_in[0, n) byte-shuffled with elements of elem_size bytes (HDF5's shuffle filter) into d_out[0, n);
        inverse=True: unshuffled.  The two ranges must not meet."""
        self._shuffle_rc(_ffi.lib().lfx_shuffle_device(self._h, _ffi.UNSHUFFLE if inverse else _ffi.SHUFFLE, elem_size, d_in, n, d_out))

    def shuffle_batch_device(self, d_in, in_offs, lens, d_out, elem_size, *, inverse=False, out_offs=None, d_table=None):
        """lfx_shuffle_batch_device: the records d_in[in_offs[i], +lens[i]) shuffled (inverse=True: unshuffled), each on its own,
        into d_out[out_offs[i], +lens[i]) in one launch; out_offs=None: at the input offsets.  d_table: device memory holding the
        {off, len} pairs instead — what encode_batch_packed_device / decode_batch_packed_device wrote to their d_table; in_offs
        then only says how many records there are (a count, or a list whose length is the count), lens and out_offs are None."""
        if d_table is not None:
            k = int(in_offs) if isinstance(in_offs, int) else len(in_offs)
            io = il = None
        else:
            k = len(in_offs)
            io, il = (C.c_uint64 * max(k, 1))(*in_offs), (C.c_uint64 * max(k, 1))(*lens)
        oo = (C.c_uint64 * max(k, 1))(*out_offs) if out_offs is not None else None
        self._shuffle_rc(_ffi.lib().lfx_shuffle_batch_device(self._h, _ffi.UNSHUFFLE if inverse else _ffi.SHUFFLE, elem_size, k, d_in, io, il,
                                                             d_table, d_out, oo))

    def shuffle_host(self, data, elem_size, inverse=False):
        """lfx_shuffle_host on host bytes → the shuffled (inverse=True: unshuffled) bytes"""
        data = bytes(data)
        out = C.create_string_buffer(max(len(data), 1))
        self._shuffle_rc(_ffi.lib().lfx_shuffle_host(self._h, _ffi.UNSHUFFLE if inverse else _ffi.SHUFFLE, elem_size, data, len(data), out))
        return out.raw[:len(data)]

    # ---- encoding with a preset dictionary (lfx_encode_dict_*) ---------------------------
    def encode_dict_device(self, fmt, zdict, d_in, n, d_out, cap, opts=None, schedule=None):
        """lfx_encode_dict_device: zlib (FDICT + DICTID) / raw DEFLATE whose first chunk is primed by a Dictionary (None: exactly
        encode_device) → out_len"""
        out_len = C.c_uint64(0)
        rc = _ffi.lib().lfx_encode_dict_device(self._h, fmt, C.byref(opts) if opts is not None else None,
                                               C.byref(schedule) if schedule is not None else None, self._dict_handle(zdict),
                                               d_in, n, d_out, cap, C.byref(out_len))
        if rc:
            raise (_ffi.DeviceError if rc == _ffi.E_DEVICE else _ffi.LfxError)(rc, self.last_error())
        return out_len.value

    def encode_dict_host(self, fmt, zdict, data, opts=None, schedule=None):
        """lfx_encode_dict_host on host bytes → the stream"""
        data = bytes(data)
        bound = _ffi.lib().lfx_encode_dict_bound(len(data), C.byref(opts) if opts is not None else None,
                                                 C.byref(schedule) if schedule is not None else None)
        if bound == 0:
            raise _ffi.LfxError(_ffi.E_ARG, "option outside the reference's domain")
        out = C.create_string_buffer(bound)
        out_len = C.c_uint64(0)
        rc = _ffi.lib().lfx_encode_dict_host(self._h, fmt, C.byref(opts) if opts is not None else None,
                                             C.byref(schedule) if schedule is not None else None, self._dict_handle(zdict),
                                             data, len(data), out, bound, C.byref(out_len))
        if rc:
            raise (_ffi.DeviceError if rc == _ffi.E_DEVICE else _ffi.LfxError)(rc, self.last_error())
        return out.raw[:out_len.value]

    def encode_batch_dict_device(self, fmt, zdict, d_in, in_offs, in_lens, d_out, out_offs, out_caps, opts=None, schedule=None):
        """lfx_encode_batch_dict_device: the records d_in[in_offs[i], +in_lens[i]) as streams at d_out[out_offs[i], +out_caps[i]),
        every one primed by the one Dictionary (None: lfx_encode_batch_device); the offsets and lengths are host-side lists
        → (rc, [(status, out_len)] per stream); rc is LFX_OK or LFX_E_NOSPACE (the call is void, status says which streams did
        not fit), anything else raises"""
        k = len(in_offs)
        a = lambda v: (C.c_uint64 * max(k, 1))(*v)
        io, il, oo, oc = a(in_offs), a(in_lens), a(out_offs), a(out_caps)
        out_len, st = (C.c_uint64 * max(k, 1))(), (C.c_int32 * max(k, 1))()
        rc = _ffi.lib().lfx_encode_batch_dict_device(self._h, fmt, C.byref(opts) if opts is not None else None,
                                                     C.byref(schedule) if schedule is not None else None, self._dict_handle(zdict),
                                                     k, d_in, io, il, d_out, oo, oc, out_len, st)
        if rc and rc != _ffi.E_NOSPACE:
            raise (_ffi.DeviceError if rc == _ffi.E_DEVICE else _ffi.LfxError)(rc, self.last_error())
        return rc, [(st[i], out_len[i]) for i in range(k)]

    # ---- a batch packed back to back (lfx_encode_batch_packed_device) -------------------
    def encode_batch_packed_device(self, fmt, d_in, in_offs, in_lens, d_out, cap, *, zdict=None, opts=None, schedule=None, align=1,
                                   d_table=None):
        """lfx_encode_batch_packed_device: the records d_in[in_offs[i], +in_lens[i]) as the streams the batch call writes, laid
        out on the device back to back in d_out[0, cap), every stream's start a multiple of `align`; zdict: one Dictionary for
        all of them (zlib / raw DEFLATE); d_table: device memory for count {off, len} pairs of uint64, or None
        → (rc, total, [(off, len)] per stream); rc is LFX_OK or LFX_E_NOSPACE (total > cap: the call is void, total and the
        layout say what it needs; d_out = None with cap = 0 is the size query), anything else raises"""
        k = len(in_offs)
        a = lambda v: (C.c_uint64 * max(k, 1))(*v)
        io, il = a(in_offs), a(in_lens)
        oo, ol, total = (C.c_uint64 * max(k, 1))(), (C.c_uint64 * max(k, 1))(), C.c_uint64(0)
        rc = _ffi.lib().lfx_encode_batch_packed_device(self._h, fmt, C.byref(opts) if opts is not None else None,
                                                       C.byref(schedule) if schedule is not None else None, self._dict_handle(zdict),
                                                       k, d_in, io, il, align, d_out, cap, oo, ol, C.byref(total), d_table)
        if rc and rc != _ffi.E_NOSPACE:
            raise (_ffi.DeviceError if rc == _ffi.E_DEVICE else _ffi.LfxError)(rc, self.last_error())
        return rc, total.value, [(oo[i], ol[i]) for i in range(k)]

    def encode_batch_packed_host(self, fmt, records, zdict=None, opts=None, schedule=None, shuffle=None):
        """a list of bytes → the list of their streams: one upload, one lfx_encode_batch_packed_device call with cap = the sum
        of the bounds, one download of `total` bytes.  shuffle: an element size — every record is byte-shuffled on the device in
        front of the encode (lfx_shuffle_batch_device); None: no such call is made"""
        import torch
        records = [bytes(r) for r in records]
        if not records:
            return []
        bound = _ffi.lib().lfx_encode_dict_bound if zdict is not None else _ffi.lib().lfx_encode_bound
        op, sp = C.byref(opts) if opts is not None else None, C.byref(schedule) if schedule is not None else None
        known, cap, offs, at = {}, 0, [], 0
        for r in records:
            if len(r) not in known:
                known[len(r)] = bound(len(r), op, sp)
                if known[len(r)] == 0:
                    raise _ffi.LfxError(_ffi.E_ARG, "option outside the reference's domain")
            cap += known[len(r)]
            offs.append(at)
            at += len(r)
        dev = torch.device("cuda", self.device)
        d_in = torch.frombuffer(bytearray(b"".join(records) or b"\0"), dtype=torch.uint8).to(dev)
        d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        if shuffle is not None:
            d_plain, d_in = d_in, torch.empty_like(d_in)
            torch.cuda.current_stream(dev).synchronize()
            self.shuffle_batch_device(d_plain.data_ptr(), offs, [len(r) for r in records], d_in.data_ptr(), shuffle)
        rc, total, layout = self.encode_batch_packed_device(fmt, d_in.data_ptr(), offs, [len(r) for r in records], d_out.data_ptr(), cap,
                                                            zdict=zdict, opts=opts, schedule=schedule)
        if rc:
            raise _ffi.LfxError(rc, self.last_error())
        out = d_out[:total].cpu().numpy().tobytes()
        return [out[o:o + n] for o, n in layout]

    # ---- a batch decoded back to back (lfx_decode_batch_packed_device) ------------------
    def decode_batch_packed_device(self, fmt, d_in, in_offs, in_lens, d_out, cap, *, zdict=None, align=1, d_in_table=None,
                                   d_table=None):
        """lfx_decode_batch_packed_device: the streams d_in[in_offs[i], +in_lens[i]) decoded back to back into d_out[0, cap),
        every stream's start a multiple of `align`, placed on the device by their decoded sizes; zdict: one Dictionary for all
        of them (zlib / raw DEFLATE).  d_in_table: device memory holding the {off, len} pairs instead — what
        encode_batch_packed_device wrote to its d_table; in_offs then only says how many streams there are (a count, or a list
        whose length is the count, or None with in_lens a count).  d_table: device memory for count {off, size} pairs, or None
        → (rc, out_offs, out_lens, consumed, statuses, total); rc is LFX_OK (the verdicts are in statuses) or LFX_E_NOSPACE
        (total > cap: nothing was decoded, the layout and the sizes say what it needs; d_out = None with cap = 0 is the size
        query), anything else raises"""
        if d_in_table is not None:
            n = in_offs if in_offs is not None else in_lens
            k = int(n) if isinstance(n, int) else len(n)
            io = il = None
        else:
            k = len(in_offs)
            a = lambda v: (C.c_uint64 * max(k, 1))(*v)
            io, il = a(in_offs), a(in_lens)
        u64s = lambda: (C.c_uint64 * max(k, 1))()
        oo, ol, used, st, total = u64s(), u64s(), u64s(), (C.c_int32 * max(k, 1))(), C.c_uint64(0)
        rc = _ffi.lib().lfx_decode_batch_packed_device(self._h, fmt, self._dict_handle(zdict), k, d_in, io, il, d_in_table, align,
                                                       d_out, cap, oo, ol, used, st, C.byref(total), d_table)
        if rc and rc != _ffi.E_NOSPACE:
            raise (_ffi.DeviceError if rc == _ffi.E_DEVICE else _ffi.LfxError)(rc, self.last_error())
        return rc, list(oo[:k]), list(ol[:k]), list(used[:k]), list(st[:k]), total.value

    def decode_batch_packed_host(self, fmt, records, zdict=None):
        """a list of streams (bytes) → (the list of their decoded bytes, statuses): one upload, the size query (d_out = None,
        cap = 0) for `total`, one allocation of exactly that, the decode, one download.  A failed stream's entry holds what it
        produced before the fault, and last_error() is the first failed stream's message."""
        return self._decode_batch_packed_host(fmt, records, zdict, None)

    def decode_batch_unshuffle_host(self, fmt, records, elem_size, zdict=None):
        """decode_batch_packed_host with every record unshuffled on the device behind the decode (elements of elem_size bytes),
        fed from the decode's device table without the layout passing through the caller (lfx_shuffle_batch_device, DESIGN.md
        §30) → (the list of their bytes, statuses)"""
        return self._decode_batch_packed_host(fmt, records, zdict, elem_size)

    def _decode_batch_packed_host(self, fmt, records, zdict, shuffle):
        import torch
        records = [bytes(r) for r in records]
        if not records:
            return [], []
        offs, at = [], 0
        for r in records:
            offs.append(at)
            at += len(r)
        lens = [len(r) for r in records]
        dev = torch.device("cuda", self.device)
        d_in = torch.frombuffer(bytearray(b"".join(records) or b"\0"), dtype=torch.uint8).to(dev)
        torch.cuda.current_stream(dev).synchronize()
        rc, _offs, _lens, _used, st, total = self.decode_batch_packed_device(fmt, d_in.data_ptr(), offs, lens, None, 0, zdict=zdict)
        if total == 0:
            return [b""] * len(records), st
        d_out = torch.empty(total, dtype=torch.uint8, device=dev)
        d_table = torch.empty(2 * len(records), dtype=torch.int64, device=dev) if shuffle is not None else None
        torch.cuda.current_stream(dev).synchronize()
        rc, out_offs, out_lens, _used, st, total = self.decode_batch_packed_device(fmt, d_in.data_ptr(), offs, lens, d_out.data_ptr(),
                                                                                 total, zdict=zdict,
                                                                                 d_table=d_table.data_ptr() if shuffle is not None else None)
        if rc:
            raise _ffi.LfxError(rc, self.last_error())
        if shuffle is not None:                 # (a successful call leaves last_error() as the decode left it)
            d_plain = torch.empty_like(d_out)
            torch.cuda.current_stream(dev).synchronize()
            self.shuffle_batch_device(d_out.data_ptr(), len(records), None, d_plain.data_ptr(), shuffle, inverse=True, d_table=d_table.data_ptr())
            d_out = d_plain
        out = d_out.cpu().numpy().tobytes()
        return [out[o:o + n] for o, n in zip(out_offs, out_lens)], st


class Dictionary:
    """A preset dictionary (lfx_dict): what zlib.compressobj(zdict=...) was given.  The last 32 KiB are the
    usable history; `id` is the Adler-32 of all bytes (RFC 1950's DICTID).  `data`: bytes-like, or a contiguous CUDA uint8
    tensor.  Belongs to its Context and counts itself in and out of it like the other native handles.  chain=True
    (lfx_dict_new_chain): the dictionary also carries the hash chain of its own tail, and the encode_dict_* calls
    serve lz77.ChainLz77Encoder / LazyLz77Encoder with it; for everything else it is the same dictionary."""

    def __init__(self, data, context=None, chain=False):
        self._h = None
        self._ctx = context if context is not None else default_context()
        self.chain = bool(chain)
        new = _ffi.lib().lfx_dict_new_chain if chain else _ffi.lib().lfx_dict_new
        st = C.c_int(0)
        if hasattr(data, "data_ptr"):
            if not data.is_cuda or data.dtype.itemsize != 1 or not data.is_contiguous():
                raise TypeError("Dictionary: a tensor must be a contiguous CUDA uint8 tensor")
            import torch
            torch.cuda.current_stream(data.device).synchronize()
            self._h = new(self._ctx.handle, data.data_ptr(), data.numel(), 1, C.byref(st))
        else:
            data = bytes(data)
            self._h = new(self._ctx.handle, data, len(data), 0, C.byref(st))
        if not self._h:
            raise (_ffi.DeviceError if st.value == _ffi.E_DEVICE else _ffi.LfxError)(st.value, self._ctx.last_error())
        self._ctx._retain()
        self.id = int(_ffi.lib().lfx_dict_id(self._h))

    @classmethod
    def train(cls, records, size=32768, segment=128, context=None, chain=False):
        """A dictionary of at most `size` bytes trained on the device from sample records (lfx_dict_train_*):
        segments of `segment` bytes whose 8-byte substrings are the most frequent across the records, the best one last.
        records: a list of bytes, or (tensor, offsets, lengths) — a contiguous CUDA uint8 tensor and host-side lists naming the
        records inside it, ascending and not overlapping; the dictionary then never leaves the device.  `trained` holds its
        length; chain as in Dictionary()."""
        ctx = context if context is not None else default_context()
        if isinstance(records, tuple) and len(records) == 3 and hasattr(records[0], "data_ptr"):
            import torch
            t, offs, lens = records
            if not t.is_cuda or t.dtype.itemsize != 1 or not t.is_contiguous():
                raise TypeError("Dictionary.train: a tensor must be a contiguous CUDA uint8 tensor")
            d_dict = torch.empty(size, dtype=torch.uint8, device=t.device)
            torch.cuda.current_stream(t.device).synchronize()
            n = ctx.dict_train_device(t.data_ptr(), list(offs), list(lens), size, segment, d_dict.data_ptr(), size)
            data = d_dict[:n]
        else:
            data = train_dictionary(records, size, segment, context=ctx)
            n = len(data)
        d = cls(data, ctx, chain)
        d.trained = n
        return d

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None):
            _ffi.lib().lfx_dict_free(self._h)
            self._h = None
            self._ctx._release()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def train_dictionary(records, size=32768, segment=128, context=None):
    """a list of bytes → the bytes of a dictionary of at most `size` bytes trained from them on the device
    (lfx_dict_train_host) — what zlib.compressobj(zdict=...), compress(zdict=...) and Dictionary() take"""
    ctx = context if context is not None else default_context()
    records = [bytes(r) for r in records]
    offs, at = [], 0
    for r in records:
        offs.append(at)
        at += len(r)
    return ctx.dict_train_host(b"".join(records), offs, [len(r) for r in records], size, segment)


_default = {}


def default_context(device=0):
    if device not in _default:
        _default[device] = Context(device)
    return _default[device]
