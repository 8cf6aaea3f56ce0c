"""BGZF by virtual offset: what htslib's bgzf_seek + bgzf_read serve, batched on the GPU and with no index of ours
(lfx_bgzf_read_host).  A virtual offset is coffset << 16 | uoffset: the byte at which a block starts in the
file, and a byte inside that block's output — the addresses .bai, .tbi, .csi and .gzi indexes hold."""
from . import _ffi
from ._stream import StreamError
from .context import default_context

VOFF_NONE = _ffi.VOFF_NONE


def voffset(coffset, uoffset):
    if not (0 <= coffset < 1 << 48 and 0 <= uoffset < 1 << 16):
        raise ValueError("voffset: coffset must fit 48 bits, uoffset 16")
    return coffset << 16 | uoffset


def split(voff):
    """→ (coffset, uoffset)"""
    return voff >> 16, voff & 0xffff


def _call(data, reads, context, sizes_only):
    ctx = context if context is not None else default_context()
    rc, res, _decoded, got, msg = ctx.bgzf_read_host(data, list(reads), sizes_only=sizes_only)
    if rc != _ffi.OK:
        raise StreamError(rc, msg)
    return res, got


def read(data, reads, context=None):
    """`reads` = [(voff, length)] or [(voff, length, end_voff)] over the BGZF file `data`, all in one call: every covered block is
    decoded once and its CRC-32 verified → [(bytes, next_voff)]; a read is short where the file ends.  Raises StreamError with the
    first failing read's status and message."""
    res, got = _call(data, reads, context, False)
    return [(b, r[1]) for b, r in zip(got, res)]


def sizes(data, reads, context=None):
    """what read() would deliver, from the block headers alone (nothing is decoded, no CRC is checked)
    → [(out_len, next_voff, n_blocks)]"""
    res, _ = _call(data, reads, context, True)
    return [(r[0], r[1], r[3]) for r in res]


def locate(members, uoff, swapped=False):
    """the virtual offset of uncompressed byte `uoff` through a member table: the one gzip.encode_members(bgzf=True) returns, or
    with swapped=True the one of gzip.decode_members / gzip.list_members (lfx_members_voffset)"""
    try:
        return _ffi.members_voffset(members, uoff, swapped)
    except _ffi.LfxError as e:
        raise StreamError(e.status, e.message)


def read_range(data, members, off, length, swapped=False, context=None):
    """uncompressed bytes [off, off + length) of the BGZF file `data`, clipped to its end: locate + read"""
    return read(data, [(locate(members, off, swapped), length)], context)[0][0]
