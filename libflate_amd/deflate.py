"""libflate::deflate — Encoder, Decoder, EncodeOptions, DEFAULT_BLOCK_SIZE
(reference src/deflate/mod.rs:22-25, src/deflate/encode.rs, src/deflate/decode.rs)."""
from . import _ffi
from ._stream import StreamError, _DecoderBase, _EncoderBase  # noqa: F401

DEFAULT_BLOCK_SIZE = 1024 * 1024  # encode.rs:11


class EncodeOptions:
    """deflate::EncodeOptions (encode.rs:17-128): builder methods return self."""

    def __init__(self, lz77=None):
        self._kw = {}
        self._foreign = None
        if lz77 is not None:
            self.with_lz77(lz77)

    @classmethod
    def new(cls):
        return cls()

    def with_lz77(self, lz77):  # encode.rs:59-65
        """`lz77`: one of this package's encoders (DefaultLz77Encoder, NoCompressionLz77Encoder: the whole path runs on the
        GPU) or ANY object with the Lz77Encode methods encode(buf, sink) / flush(sink) / compression_level() /
        window_size() (lib.rs:83-107): it then runs on the caller's side and the GPU Huffman-codes what it emits
        (lfx_encoder_write_codes)."""
        if hasattr(lz77, "_opts"):
            self._kw.update(lz77._opts())
            self._foreign = None
        else:
            self._foreign = lz77
            self._kw.update({"lz77_kind": _ffi.LZ77_DEFAULT, "window_size": min(int(lz77.window_size()), 32768),
                             "lz77_level": 1 + int(lz77.compression_level())})
        return self

    def no_compression(self):  # encode.rs:77-80
        self._kw["no_compression"] = 1
        return self

    def block_size(self, size):  # encode.rs:93-96
        self._kw["block_size"] = size
        return self

    def fixed_huffman_codes(self):  # encode.rs:107-110
        self._kw["dynamic_huffman"] = 0
        return self

    def auto_huffman_codes(self):
        """not a reference option (LFX_HUFFMAN_AUTO): per block the smallest of the dynamic, the fixed and the
        stored form; the blocks and the LZ77 code words stay those of the default options"""
        self._kw["dynamic_huffman"] = _ffi.HUFFMAN_AUTO
        return self

    def merge_blocks(self):
        """not a reference option (block_merge): neighbouring dynamic blocks are joined on the device wherever
        one Huffman code for both is no longer than two — block_size becomes the smallest block; the LZ77 code words stay
        those of the same options without it.  One-shot, batch and dictionary encodes; the stream encoder refuses it."""
        self._kw["block_merge"] = 1
        return self

    def _to_c(self):
        return _ffi.make_opts(**self._kw)


class Encoder(_EncoderBase):
    """deflate::Encoder (encode.rs:130-249)."""
    FORMAT = _ffi.DEFLATE

    @classmethod
    def new(cls, inner, context=None, options=None, zdict=None):
        """zdict: a preset dictionary, bytes or a libflate_amd.Dictionary (what zlib.compressobj(zdict=...) takes; DESIGN.md
        §25).  options: EncodeOptions, e.g. EncodeOptions(lz77.LevelLz77Encoder(6)) — with zdict as bytes and a chained, lazy or
        level parse the encoder makes the chain dictionary itself, as compress(data, zdict=bytes, level=6) does."""
        return cls(inner, options, context, zdict)

    @classmethod
    def with_options(cls, inner, options, context=None, zdict=None):
        return cls(inner, options, context, zdict)


def _with_lz77(options, lz77, cls, level=None):
    """options with `lz77` (an Lz77Encode of this package, e.g. lz77.ChainLz77Encoder(8)) put in; None: options as they are.
    level: shorthand for lz77=lz77.LevelLz77Encoder(level), exclusive with lz77"""
    if level is not None:
        if lz77 is not None:
            raise ValueError("level= and lz77= exclude each other: level=n is lz77=LevelLz77Encoder(n)")
        from .lz77 import LevelLz77Encoder
        lz77 = LevelLz77Encoder(level)
    if lz77 is None:
        return options
    return (options if options is not None else cls()).with_lz77(lz77)


def _compress(fmt, data, zdict, options, context, lz77=None, level=None, merge_blocks=False, shuffle=None):
    if shuffle is not None:     # (the batch of one record: the same stream, with the shuffle in front of it on the device)
        return _compress_batch(fmt, [data], zdict, options, context, lz77, level, merge_blocks, shuffle)[0]
    from .context import Dictionary, default_context
    ctx = context if context is not None else default_context()
    options = _with_lz77(options, lz77, EncodeOptions, level)
    if merge_blocks:
        options = (options if options is not None else EncodeOptions()).merge_blocks()
    opts = options._to_c() if options is not None else None
    if zdict is None:
        return ctx.encode_host(fmt, data, opts)
    own = not hasattr(zdict, "handle")
    # (bytes: the dictionary is made here, with a chain of its own when the parse is a chained one; a caller's
    # Dictionary is taken as it was made)
    chained = opts is not None and (opts.lz77_kind & 0xFF) in (_ffi.LZ77_CHAIN, _ffi.LZ77_LAZY, _ffi.LZ77_LEVEL, _ffi.LZ77_COST)
    d = Dictionary(zdict, ctx, chain=chained) if own else zdict
    try:
        return ctx.encode_dict_host(fmt, d, data, opts)
    finally:
        if own:
            d.close()


def _compress_batch(fmt, records, zdict, options, context, lz77=None, level=None, merge_blocks=False, shuffle=None):
    from .context import Dictionary, default_context
    ctx = context if context is not None else default_context()
    options = _with_lz77(options, lz77, EncodeOptions, level)
    if merge_blocks:
        options = (options if options is not None else EncodeOptions()).merge_blocks()
    opts = options._to_c() if options is not None else None
    own = zdict is not None and not hasattr(zdict, "handle")
    chained = opts is not None and (opts.lz77_kind & 0xFF) in (_ffi.LZ77_CHAIN, _ffi.LZ77_LAZY, _ffi.LZ77_LEVEL, _ffi.LZ77_COST)
    d = Dictionary(zdict, ctx, chain=chained) if own else zdict     # (as in _compress)
    try:
        if shuffle is not None:
            return ctx.encode_batch_packed_host(fmt, records, d, opts, shuffle=shuffle)
        return ctx.encode_batch_packed_host(fmt, records, d, opts)
    finally:
        if own:
            d.close()


def _decompress(fmt, data, zdict, context, shuffle=None):
    """the one-shot inverse of _compress: the size call in front for the capacity (lfx_decode_size_host), then decode_host;
    with a dictionary decode_dict_host, whose capacity grows (the size calls take no dictionary).  shuffle: the batch of one
    record, which unshuffles on the device"""
    if shuffle is not None:
        return _decompress_batch(fmt, [data], zdict, context, shuffle)[0]
    from .context import Dictionary, default_context
    ctx = context if context is not None else default_context()
    data = bytes(data)
    if zdict is None:
        _rc, size, _used, _msg = ctx.decode_size_host(fmt, data)
        rc, out, _used, msg = ctx.decode_host(fmt, data, cap=max(size, 1))
    else:
        own = not hasattr(zdict, "handle")
        d = Dictionary(zdict, ctx) if own else zdict
        try:
            rc, out, _used, msg = ctx.decode_dict_host(fmt, d, data)
        finally:
            if own:
                d.close()
    if rc != _ffi.OK:
        raise StreamError(rc, msg)
    return out


def _decompress_batch(fmt, records, zdict, context, shuffle=None):
    """the inverse of _compress_batch: Context.decode_batch_packed_host; the first failed record raises StreamError with its
    index in front of the library's message"""
    from .context import Dictionary, default_context
    ctx = context if context is not None else default_context()
    own = zdict is not None and not hasattr(zdict, "handle")
    d = Dictionary(zdict, ctx) if own else zdict
    try:
        if shuffle is not None:
            outs, statuses = ctx.decode_batch_unshuffle_host(fmt, records, shuffle, d)
        else:
            outs, statuses = ctx.decode_batch_packed_host(fmt, records, d)
        msg = ctx.last_error()
    finally:
        if own:
            d.close()
    for i, st in enumerate(statuses):
        if st != _ffi.OK:
            raise StreamError(st, "record %d: %s" % (i, msg))
    return outs


def decompress(data, zdict=None, context=None, shuffle=None):
    """compress's inverse: one raw DEFLATE stream → its bytes.  zdict: the preset dictionary the stream was made with, bytes or
    a libflate_amd.Dictionary (what zlib.decompressobj(wbits=-15, zdict=...) takes).  Raises StreamError where the stream fails.
    shuffle: the element size the decoded bytes were shuffled with — they are unshuffled on the device behind the decode
    (libflate_amd.filters.unshuffle); None: no such step."""
    return _decompress(_ffi.DEFLATE, data, zdict, context, shuffle)


def decompress_batch(records, zdict=None, context=None, shuffle=None):
    """compress_batch's inverse: a list of raw DEFLATE streams (bytes) → the list of their bytes, in one upload, one decode of
    all records placed back to back by their decoded sizes (lfx_decode_batch_packed_device) and one download.
    One zdict serves every record.  A failed record raises StreamError; the message names its index.
    shuffle: the element size the decoded bytes were shuffled with — they are unshuffled on the device behind the decode
    (libflate_amd.filters.unshuffle); None: no such step."""
    return _decompress_batch(_ffi.DEFLATE, records, zdict, context, shuffle)


def compress_batch(records, zdict=None, options=None, context=None, lz77=None, level=None, merge_blocks=False, shuffle=None):
    """[compress(r, ...) for r in records] — a list of bytes to the list of their raw DEFLATE streams — in one upload, one
    encode of all records (lfx_encode_batch_packed_device) and one download of the streams packed back to
    back.  The keywords are compress's; one zdict serves every record.
    shuffle: an element size, 1..256 — the input is byte-shuffled on the device in front of the encode (HDF5's shuffle filter,
    libflate_amd.filters.shuffle); None: no such step."""
    return _compress_batch(_ffi.DEFLATE, records, zdict, options, context, lz77, level, merge_blocks, shuffle)


def compress(data, zdict=None, options=None, context=None, lz77=None, level=None, merge_blocks=False, shuffle=None):
    """`data` as one raw DEFLATE stream, encoded in one call (one write_all + finish).  zdict: a preset dictionary, bytes or a
    libflate_amd.Dictionary — the stream then starts with the dictionary as history, what
    zlib.decompressobj(wbits=-15, zdict=...) reads (lfx_encode_dict_host).  lz77: an Lz77Encode of this package
    for the options, e.g. lz77.ChainLz77Encoder(8).  level: 1..9, shorthand for lz77=lz77.LevelLz77Encoder(level)
    (DESIGN.md §23), exclusive with lz77.  merge_blocks=True: the options with merge_blocks().
    shuffle: an element size, 1..256 — the input is byte-shuffled on the device in front of the encode (HDF5's shuffle filter,
    libflate_amd.filters.shuffle); None: no such step."""
    return _compress(_ffi.DEFLATE, data, zdict, options, context, lz77, level, merge_blocks, shuffle)


class Decoder(_DecoderBase):
    """deflate::Decoder (decode.rs:8-164)."""
    FORMAT = _ffi.DEFLATE

    @classmethod
    def new(cls, inner, context=None, zdict=None):
        """zdict: a preset dictionary, bytes or a libflate_amd.Dictionary (what zlib.decompressobj(zdict=...) takes)"""
        return cls(inner, context, zdict)
