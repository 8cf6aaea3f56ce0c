"""Seek index: random-access reads of a DEFLATE / zlib / gzip stream on the GPU (lfx_decode_index_device and friends,
DESIGN.md §12).

    decoded, idx = Index.build(data, format="gzip", spacing=1 << 20)     # one decode builds the index
    encoded, idx = Index.encode(data, format="gzip", spacing=1 << 20)    # or the encode that writes the stream (§13)
    piece = idx.read(data, offset, length)                              # decodes from the access point in front of offset
    blob = idx.to_bytes(); idx2 = Index.from_bytes(blob)                # persistence

`data` is bytes or a CUDA uint8 tensor holding the whole compressed input (for encode(): the bytes to compress); reads return
CUDA uint8 tensors.
"""
import ctypes as C

from . import _ffi
from ._stream import StreamError
from .context import default_context

_FORMATS = {"deflate": _ffi.DEFLATE, "zlib": _ffi.ZLIB, "gzip": _ffi.GZIP}


def _device_bytes(data, device):
    import torch
    if isinstance(data, torch.Tensor):
        if data.dtype != torch.uint8 or not data.is_cuda:
            raise TypeError("a CUDA uint8 tensor is expected")
        return data.contiguous()
    raw = bytes(data)
    t = torch.empty(max(len(raw), 1), dtype=torch.uint8, device="cuda:%d" % device)
    if raw:
        t[:len(raw)].copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))
    return t[:len(raw)]


class Index:
    """A seek index made on a Context; freed with close() (or when collected).  It counts itself in and out of its Context."""

    def __init__(self, handle, ctx):
        self._h = handle
        self._ctx = ctx
        self._src = None       # (bytes object, its device copy): reads of the same bytes upload them once
        ctx._retain()

    def close(self):
        self._src = None
        if self._h:
            _ffi.lib().lfx_index_free(self._h)
            self._h = None
            self._ctx._release()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- build / persistence
    @classmethod
    def build(cls, data, format="gzip", multi=False, spacing=1 << 20, ctx=None, cap=None):
        """Decode `data` and index it → (decoded CUDA uint8 tensor, Index).  Raises StreamError where the decode fails."""
        import torch
        ctx = ctx if ctx is not None else default_context()
        fmt = _FORMATS[format] if isinstance(format, str) else int(format)
        src = _device_bytes(data, ctx.device)
        n = src.numel()
        grow = cap is None
        cap = cap if cap is not None else max(1 << 16, n * 8)
        while True:
            out = torch.empty(max(cap, 1), dtype=torch.uint8, device=src.device)
            rc, ol, _used, h, msg = ctx.decode_index_device(fmt, src.data_ptr(), n, out.data_ptr(), cap, spacing,
                                                             _ffi.DEC_MULTI if multi else 0)
            if grow and rc == _ffi.E_NOSPACE and cap < n * 1040 + (1 << 20):
                cap *= 8
                continue
            if rc != _ffi.OK:
                raise StreamError(rc, msg)
            return out[:ol], cls(h, ctx)

    @classmethod
    def encode(cls, data, format="gzip", spacing=1 << 20, options=None, schedule=None, ctx=None, lz77=None):
        """Compress `data` and index the stream written (lfx_encode_index_device) → (encoded CUDA uint8 tensor, Index).
        options: an lfx_encode_opts or a {deflate,zlib,gzip}.EncodeOptions; schedule: an lfx_schedule (None: one write_all).
        The encoded bytes are exactly lfx_encode_device's.  Raises LfxError where the encode fails."""
        import torch
        ctx = ctx if ctx is not None else default_context()
        fmt = _FORMATS[format] if isinstance(format, str) else int(format)
        if lz77 is not None:        # (an Lz77Encode of this package for the options, e.g. lz77.ChainLz77Encoder(8))
            from . import deflate, gzip as _gzip
            options = deflate._with_lz77(options, lz77, _gzip.EncodeOptions if fmt == _ffi.GZIP else deflate.EncodeOptions)
        opts = options._to_c() if hasattr(options, "_to_c") else options
        src = _device_bytes(data, ctx.device)
        n = src.numel()
        cap = _ffi.lib().lfx_encode_bound(n, C.byref(opts) if opts is not None else None,
                                          C.byref(schedule) if schedule is not None else None)
        cap = (max(cap, 64) + 3) & ~3       # (0 for options outside the domain: the encode itself reports them)
        out = torch.empty(cap, dtype=torch.uint8, device=src.device)
        ol, h = ctx.encode_index_device(fmt, src.data_ptr(), n, out.data_ptr(), cap, opts, schedule, spacing)
        return out[:ol], cls(h, ctx)

    def to_bytes(self):
        L = _ffi.lib()
        n = C.c_uint64(0)
        L.lfx_index_export(self._ctx.handle, self._h, None, 0, C.byref(n))
        buf = C.create_string_buffer(max(n.value, 1))
        rc = L.lfx_index_export(self._ctx.handle, self._h, buf, n.value, C.byref(n))
        if rc:
            raise _ffi.LfxError(rc, self._ctx.last_error())
        return buf.raw[:n.value]

    @classmethod
    def from_bytes(cls, blob, ctx=None):
        ctx = ctx if ctx is not None else default_context()
        blob = bytes(blob)
        st = C.c_int32(0)
        h = _ffi.lib().lfx_index_import(ctx.handle, blob, len(blob), C.byref(st))
        if not h:
            raise _ffi.LfxError(st.value, "not a valid serialised index")
        return cls(h, ctx)

    @staticmethod
    def check(blob):
        """→ the info dict of a valid serialised index; raises LfxError otherwise"""
        blob = bytes(blob)
        info = _ffi.IndexInfo()
        rc = _ffi.lib().lfx_index_check(blob, len(blob), C.byref(info))
        if rc:
            raise _ffi.LfxError(rc, "not a valid serialised index")
        return _info_dict(info)

    # ---- what it holds
    @property
    def info(self):
        info = _ffi.IndexInfo()
        _ffi.lib().lfx_index_get_info(self._h, C.byref(info))
        return _info_dict(info)

    @property
    def points(self):
        """[(in_bit, hdr_bit, out_off, member, win_len, in_crc, btype)] in stream order"""
        p = _ffi.IndexPoint()
        out = []
        for i in range(self.info["n_points"]):
            _ffi.lib().lfx_index_get_point(self._h, i, C.byref(p))
            out.append((p.in_bit, p.hdr_bit, p.out_off, p.member, p.win_len, p.in_crc, p.btype))
        return out

    def span(self, offset, length):
        """the input bytes (lo, hi) a read of [offset, offset + length) needs"""
        lo, hi = C.c_uint64(0), C.c_uint64(0)
        rc = _ffi.lib().lfx_index_span(self._h, offset, length, C.byref(lo), C.byref(hi))
        if rc:
            raise _ffi.LfxError(rc, "offset past the end of the output")
        return lo.value, hi.value

    # ---- reads
    def read_many(self, data, ranges, in_base=0):
        """[(offset, length)] → [CUDA uint8 tensor] in ONE call.  `data` holds input bytes [in_base, in_base + len(data)):
        a CUDA uint8 tensor is read where it lies; a bytes object is uploaded once and kept for further reads of the same
        object.  Raises StreamError with the first failing read's status."""
        import torch
        if isinstance(data, bytes) and self._src is not None and self._src[0] is data:
            src = self._src[1]
        else:
            src = _device_bytes(data, self._ctx.device)
            self._src = (data, src) if isinstance(data, bytes) else None
        ol = self.info["out_len"]
        lens = [max(0, min(o + ln, ol) - o) if o <= ol else 0 for o, ln in ranges]
        offs, total = [], 0
        for ln in lens:
            offs.append(total)
            total += ln
        out = torch.empty(max(total, 1), dtype=torch.uint8, device=src.device)
        rc, got, _st, msg = self._ctx.index_read_device(self._h, src.data_ptr(), in_base, src.numel(), [o for o, _ in ranges],
                                                        [ln for _, ln in ranges], out.data_ptr(), offs)
        if rc != _ffi.OK:
            raise StreamError(rc, msg)
        return [out[a:a + g] for a, g in zip(offs, got)]

    def read(self, data, offset, length, in_base=0):
        return self.read_many(data, [(offset, length)], in_base)[0]


def _info_dict(info):
    return {k: getattr(info, k) for k, _ in _ffi.IndexInfo._fields_}
