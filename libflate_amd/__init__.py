"""libflate_amd — MI355X-native DEFLATE hot path behind libflate's own API shape.

Modules mirror the reference crate layout: `deflate`, `zlib`, `gzip`, `lz77`.
The work runs in hand-written HIP kernels reached through the C ABI in include/lfx.h; there is no
CPU fallback.
"""
from . import _ffi  # noqa: F401
from .context import Context, Dictionary, default_context, train_dictionary  # noqa: F401
from . import bgzf, deflate, filters, gzip, lz77, non_blocking, zlib  # noqa: F401
from .index import Index  # noqa: F401
from ._stream import StreamError  # noqa: F401


def decoded_size(data, format="gzip", multi=False, context=None):
    """The number of bytes `data` (bytes, or a CUDA uint8 tensor) decodes to, found without decoding it and without an
    output buffer (lfx_decode_size_*; the checksum is not verified).  format: "deflate", "zlib" or "gzip"; multi: every
    member of a multi-member gzip input.  Raises StreamError where the stream is damaged."""
    fmt = {"deflate": _ffi.DEFLATE, "zlib": _ffi.ZLIB, "gzip": _ffi.GZIP}[format]
    ctx = context if context is not None else default_context()
    flags = _ffi.DEC_MULTI if multi else 0
    if hasattr(data, "data_ptr"):
        if not data.is_cuda or data.dtype.itemsize != 1 or not data.is_contiguous():
            raise TypeError("decoded_size: a tensor must be a contiguous CUDA uint8 tensor")
        import torch
        torch.cuda.current_stream(data.device).synchronize()
        rc, out_len, _used, msg = ctx.decode_size_device(fmt, data.data_ptr(), data.numel(), flags)
    else:
        rc, out_len, _used, msg = ctx.decode_size_host(fmt, data, flags)
    if rc != _ffi.OK:
        raise StreamError(rc, msg)
    return out_len

__all__ = ["Context", "Dictionary", "default_context", "train_dictionary", "Index", "decoded_size", "StreamError", "bgzf", "deflate", "zlib", "gzip", "lz77", "non_blocking", "filters"]
