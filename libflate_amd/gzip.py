"""libflate::gzip — Encoder, Decoder, MultiDecoder, EncodeOptions, HeaderBuilder (reference src/gzip.rs)."""
import struct

from . import _ffi
from . import deflate as _deflate
from ._stream import StreamError, _DecoderBase, _EncoderBase  # noqa: F401
from .context import default_context


class ExtraSubField:  # gzip.rs:507-541
    def __init__(self, id, data):
        self.id = bytes(id)
        self.data = bytes(data)

    def _bytes(self):
        return self.id + struct.pack("<H", len(self.data)) + self.data


class HeaderBuilder:
    """gzip::HeaderBuilder (gzip.rs:126-288).  modification_time defaults to 0 here (the reference
    uses `now`, gzip.rs:148-151) — set it explicitly for reproducible bytes."""

    def __init__(self):
        self._kw = {"mtime": 0}

    @classmethod
    def new(cls):
        return cls()

    def modification_time(self, t):
        self._kw["mtime"] = t
        return self

    def os(self, os_code):
        self._kw["os"] = os_code
        return self

    def text(self):
        self._kw["is_text"] = 1
        return self

    def verify(self):
        self._kw["hcrc"] = 1
        return self

    def extra_field(self, subfields):
        self._kw["extra"] = b"".join(f._bytes() for f in subfields)
        return self

    def filename(self, name):
        self._kw["filename"] = bytes(name)
        return self

    def comment(self, text):
        self._kw["comment"] = bytes(text)
        return self

    def finish(self):
        return dict(self._kw)


class EncodeOptions(_deflate.EncodeOptions):
    """gzip::EncodeOptions (gzip.rs:639-751)."""

    def __init__(self, lz77=None):
        super().__init__(lz77)
        self._kw.setdefault("mtime", 0)

    def no_compression(self):  # gzip.rs:700-705
        """stored blocks; the header's compression level goes back to Unknown at this point (gzip.rs:703) — a header()
        call AFTER it brings its own level along again"""
        super().no_compression()
        self._kw["lz77_level"] = 1 + 2
        return self

    def header(self, header):  # gzip.rs:717-720
        """`header`: what HeaderBuilder.finish() returns, or the dict a Decoder's header() returns (gzip.rs:959).  The header
        REPLACES the one the options held, its compression level included: the XFL byte written is the header's
        own — Unknown for a builder's header (gzip.rs:157), Fastest / Slowest kept for one cloned from a decoder."""
        h = dict(header)
        if "modification_time" in h:        # a decoder's header: the reference's field names
            h = {k: v for k, v in {"mtime": h["modification_time"], "os": h.get("os", 3), "is_text": int(bool(h.get("is_text"))),
                                   "hcrc": int(bool(h.get("is_verified"))), "extra": h.get("extra_field"),
                                   "filename": h.get("filename"), "comment": h.get("comment"), "xfl": h.get("xfl", 0)}.items()
                 if v is not None}
        xfl = h.pop("xfl", 0)
        self._kw.update(h)
        # (lz77_level = 1 + libflate_lz77::CompressionLevel: Fast → XFL 4, Best → XFL 2, Balance → XFL 0, gzip.rs:84-92)
        self._kw["lz77_level"] = {4: 1 + 1, 2: 1 + 3}.get(xfl, 1 + 2)
        return self


class Encoder(_EncoderBase):
    """gzip::Encoder (gzip.rs:754-908)."""
    FORMAT = _ffi.GZIP

    def __init__(self, inner, options=None, context=None):
        super().__init__(inner, options if options is not None else EncodeOptions(), context)

    @classmethod
    def new(cls, inner, context=None):
        return cls(inner, None, context)

    @classmethod
    def with_options(cls, inner, options, context=None):
        return cls(inner, options, context)


class Decoder(_DecoderBase):
    """gzip::Decoder (gzip.rs:912-1047): one member; trailing bytes are left unread."""
    FORMAT = _ffi.GZIP

    @classmethod
    def new(cls, inner, context=None):
        return cls(inner, context)


class MultiDecoder(_DecoderBase):
    """gzip::MultiDecoder (gzip.rs:1052-1167): concatenated members."""
    FORMAT = _ffi.GZIP
    FLAGS = _ffi.DEC_MULTI

    @classmethod
    def new(cls, inner, context=None):
        return cls(inner, context)


def decode_members(data, context=None):
    """What MultiDecoder reads from `data` (concatenated members: BGZF, `cat a.gz b.gz`), the members decoded on the GPU as
    one batch (lfx_decode_members_host) → (bytes, [(in_off, in_len, out_off, out_len)] per member).  Raises StreamError
    where MultiDecoder's read_to_end would fail."""
    ctx = context if context is not None else default_context()
    rc, out, _used, members, msg = ctx.decode_members_host(data)
    if rc != _ffi.OK:
        raise StreamError(rc, msg)
    return out, members


def list_members(data, context=None):
    """`gzip -l` over concatenated members (BGZF, `cat a.gz b.gz`): the member table decode_members would return, without
    decoding (lfx_decode_members_size_host; the CRCs are not checked) → [(in_off, in_len, out_off, out_len)].  Raises
    StreamError where the walk fails."""
    ctx = context if context is not None else default_context()
    rc, _out_len, _used, members, msg = ctx.decode_members_size_host(data)
    if rc != _ffi.OK:
        raise StreamError(rc, msg)
    return members


def compress(data, options=None, context=None, lz77=None, level=None, merge_blocks=False, shuffle=None):
    """`data` as one gzip member, encoded in one call (one write_all + finish; modification time 0 unless the options say
    otherwise).  lz77: an Lz77Encode of this package for the options, e.g. lz77.ChainLz77Encoder(8).  level:
    1..9, shorthand for lz77=lz77.LevelLz77Encoder(level), exclusive with lz77.  merge_blocks=True: the options
    with merge_blocks().
    shuffle: an element size, 1..256 — the input is byte-shuffled on the device in front of the encode (HDF5's shuffle filter,
    libflate_amd.filters.shuffle); None: no such step."""
    if options is None:
        options = EncodeOptions()
    return _deflate._compress(_ffi.GZIP, data, None, options, context, lz77, level, merge_blocks, shuffle)


def compress_batch(records, options=None, context=None, lz77=None, level=None, merge_blocks=False, shuffle=None):
    """[compress(r, ...) for r in records] — a list of bytes to the list of their gzip members — in one upload, one encode of
    all records (lfx_encode_batch_packed_device) and one download of the members packed back to back.  The
    keywords are compress's.
    shuffle: an element size, 1..256 — the input is byte-shuffled on the device in front of the encode (HDF5's shuffle filter,
    libflate_amd.filters.shuffle); None: no such step."""
    if options is None:
        options = EncodeOptions()
    return _deflate._compress_batch(_ffi.GZIP, records, None, options, context, lz77, level, merge_blocks, shuffle)


def decompress(data, context=None, shuffle=None):
    """compress's inverse: one gzip member → its bytes, CRC-32 checked (bytes behind the member are left unread, as by
    Decoder; concatenated members: decode_members).  Raises StreamError where the member fails.
    shuffle: the element size the decoded bytes were shuffled with — they are unshuffled on the device behind the decode
    (libflate_amd.filters.unshuffle); None: no such step."""
    return _deflate._decompress(_ffi.GZIP, data, None, context, shuffle)


def decompress_batch(records, context=None, shuffle=None):
    """compress_batch's inverse: a list of gzip members (bytes) → the list of their bytes, in one upload, one decode of all
    records placed back to back by their decoded sizes (lfx_decode_batch_packed_device) and one download.  A
    failed record raises StreamError; the message names its index.
    shuffle: the element size the decoded bytes were shuffled with — they are unshuffled on the device behind the decode
    (libflate_amd.filters.unshuffle); None: no such step."""
    return _deflate._decompress_batch(_ffi.GZIP, records, None, context, shuffle)


def encode_members(data, member_size=1 << 20, bgzf=False, options=None, context=None, lz77=None):
    """`data` as gzip members of member_size input bytes each, lying back to back: what decode_members, zcat and Python's gzip
    read, and with bgzf=True (member_size at most 65505; bgzip's own is _ffi.BGZF_MEMBER_SIZE = 65280) a BGZF file with its
    end-of-file marker.  All members are encoded on the GPU in one pass (lfx_encode_members_host) → (bytes, [(in_off, in_len,
    out_off, out_len)] per member: the slice of `data`, the member in the result).  members_to_gzi(members) is bgzip's index of
    them.  lz77: an Lz77Encode of this package for the options, e.g. lz77.ChainLz77Encoder(8).  Raises StreamError where the call
    fails."""
    ctx = context if context is not None else default_context()
    opts = _deflate._with_lz77(options if options is not None else EncodeOptions(), lz77, EncodeOptions)._to_c()
    try:
        rc, out, _count, members, msg = ctx.encode_members_host(data, member_size, _ffi.MEMBERS_BGZF if bgzf else 0, opts)
    except _ffi.DeviceError:
        raise
    except _ffi.LfxError as e:          # (an argument out of its domain: the message names the field)
        raise StreamError(e.status, e.message)
    if rc != _ffi.OK:
        raise StreamError(rc, msg)
    return out, members


members_to_gzi = _ffi.members_to_gzi
