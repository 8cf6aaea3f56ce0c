"""libflate::zlib — Encoder, Decoder, EncodeOptions, FlushMode (reference src/zlib.rs)."""
from . import _ffi
from . import deflate as _deflate
from ._stream import StreamError, _DecoderBase, _EncoderBase  # noqa: F401


class FlushMode:  # zlib.rs:184-195
    NONE = _ffi.FLUSH_NONE
    SYNC = _ffi.FLUSH_SYNC


class EncodeOptions(_deflate.EncodeOptions):
    """zlib::EncodeOptions (zlib.rs:414-518)."""

    def flush_mode(self, mode):  # zlib.rs:504-507
        self._kw["zlib_flush_mode"] = mode
        return self


class Encoder(_EncoderBase):
    """zlib::Encoder (zlib.rs:522-681)."""
    FORMAT = _ffi.ZLIB

    @classmethod
    def new(cls, inner, context=None, options=None, zdict=None):
        """zdict: a preset dictionary, bytes or a libflate_amd.Dictionary (what zlib.compressobj(zdict=...) takes; DESIGN.md
        §25).  options: EncodeOptions, e.g. EncodeOptions(lz77.LevelLz77Encoder(6)) — with zdict as bytes and a chained, lazy or
        level parse the encoder makes the chain dictionary itself, as compress(data, zdict=bytes, level=6) does."""
        return cls(inner, options, context, zdict)

    @classmethod
    def with_options(cls, inner, options, context=None, zdict=None):
        return cls(inner, options, context, zdict)


def compress(data, zdict=None, options=None, context=None, lz77=None, level=None, merge_blocks=False, shuffle=None):
    """`data` as one zlib stream, encoded in one call (one write_all + finish).  zdict: a preset dictionary, bytes or a
    libflate_amd.Dictionary — the stream then carries FDICT and the dictionary's id, what zlib.decompressobj(zdict=...)
    reads (lfx_encode_dict_host).  lz77: an Lz77Encode of this package for the options, e.g.
    lz77.ChainLz77Encoder(8).  level: 1..9, shorthand for lz77=lz77.LevelLz77Encoder(level),
    exclusive with lz77; with zdict as bytes the dictionary is made with a chain of its own, as for a chained lz77.
    merge_blocks=True: the options with merge_blocks().
    shuffle: an element size, 1..256 — the input is byte-shuffled on the device in front of the encode (HDF5's shuffle filter,
    libflate_amd.filters.shuffle); None: no such step."""
    if (lz77 is not None or level is not None or merge_blocks) and options is None:
        options = EncodeOptions()
    return _deflate._compress(_ffi.ZLIB, data, zdict, options, context, lz77, level, merge_blocks, shuffle)


def compress_batch(records, zdict=None, options=None, context=None, lz77=None, level=None, merge_blocks=False, shuffle=None):
    """[compress(r, zdict=..., ...) for r in records] — a list of bytes to the list of their zlib streams — in one upload, one
    encode of all records (lfx_encode_batch_packed_device) and one download of the streams packed back to
    back.  The keywords are compress's; one zdict serves every record.
    shuffle: an element size, 1..256 — the input is byte-shuffled on the device in front of the encode (HDF5's shuffle filter,
    libflate_amd.filters.shuffle); None: no such step."""
    if (lz77 is not None or level is not None or merge_blocks) and options is None:
        options = EncodeOptions()
    return _deflate._compress_batch(_ffi.ZLIB, records, zdict, options, context, lz77, level, merge_blocks, shuffle)


def decompress(data, zdict=None, context=None, shuffle=None):
    """compress's inverse: one zlib stream → its bytes, Adler-32 checked.  zdict: the preset dictionary, bytes or a
    libflate_amd.Dictionary (what zlib.decompressobj(zdict=...) takes); a stream without FDICT is decoded without it.  Raises
    StreamError where the stream fails.
    shuffle: the element size the decoded bytes were shuffled with — they are unshuffled on the device behind the decode
    (libflate_amd.filters.unshuffle); None: no such step."""
    return _deflate._decompress(_ffi.ZLIB, data, zdict, context, shuffle)


def decompress_batch(records, zdict=None, context=None, shuffle=None):
    """compress_batch's inverse: a list of zlib streams (bytes) → the list of their bytes, in one upload, one decode of all
    records placed back to back by their decoded sizes (lfx_decode_batch_packed_device) and one download.  One
    zdict serves every record.  A failed record raises StreamError; the message names its index.
    shuffle: the element size the decoded bytes were shuffled with — they are unshuffled on the device behind the decode
    (libflate_amd.filters.unshuffle); None: no such step."""
    return _deflate._decompress_batch(_ffi.ZLIB, records, zdict, context, shuffle)


class Decoder(_DecoderBase):
    """zlib::Decoder (zlib.rs:284-410)."""
    FORMAT = _ffi.ZLIB

    @classmethod
    def new(cls, inner, context=None, zdict=None):
        """zdict: a preset dictionary, bytes or a libflate_amd.Dictionary (what zlib.decompressobj(zdict=...) takes)"""
        return cls(inner, context, zdict)
