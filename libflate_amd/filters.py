"""Filters in front of DEFLATE for numeric records.

shuffle / unshuffle: HDF5's H5Z_FILTER_SHUFFLE, which is numcodecs' Shuffle — byte 0 of every element, then byte 1 of every
element, and so on; the bytes behind the last whole element are copied.  The work runs on the GPU (lfx_shuffle_host); the
compress / decompress calls of gzip, zlib and deflate take the same filter as their shuffle= keyword and keep the bytes on the
device between the filter and the codec.
"""
from .context import default_context


def shuffle(data, elem_size, context=None):
    """`data` (bytes) byte-shuffled with elements of elem_size bytes, 1..256 → bytes of the same length"""
    ctx = context if context is not None else default_context()
    return ctx.shuffle_host(data, elem_size)


def unshuffle(data, elem_size, context=None):
    """shuffle's inverse"""
    ctx = context if context is not None else default_context()
    return ctx.shuffle_host(data, elem_size, inverse=True)
