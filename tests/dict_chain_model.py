"""The contract of the chained and the lazy parse through a chain dictionary (include/lfx.h "a chain dictionary", DESIGN.md
§21) restated in plain Python, and the stream it implies.  Test infrastructure: checked against chain_model, lazy_model,
dict_encode_model and python-zlib (test_dict_chain_model.py), never against the library.

T is the usable tail of the dictionary, buf the stream's first chunk, b = T ‖ buf, end = max(3, |b|) - 3.  Every position
< end counts as inserted once, in order — every position of T, |T|-2 and |T|-1 among them.  primed_lengths is
lazy_model._lengths over b with the candidates evaluated only for i >= |T|: the first `depth` earlier occurrences of
b[i..i+3], most recent first, cut off at the first one farther than `window`; the longest wins, among equal lengths the
nearest.  The walk starts at |T| — greedy for LFX_LZ77_CHAIN, zlib's lazy rule for LFX_LZ77_LAZY (position i is a literal when
L(i + 1) > L(i), L = 0 from end on) — and the tail literals are taken from max(i, |T|).  A code word is (val << 16) | dist,
dist == 0 a literal — the oracle's lz77_chunk format."""
import functools
import zlib

import chain_model
import lazy_model
from chain_model import LEVEL_BEST, MAX_LENGTH, MAX_WINDOW
from dict_encode_model import py_inflate, usable_tail  # noqa: F401  (py_inflate: for the tests)

CHAIN, LAZY = 2, 3            # lz77_kind & 0xFF of the library (never handed to the oracle)


@functools.lru_cache(maxsize=64)      # (the formats and the kinds of one case share the lengths; tuples, never changed)
def _primed_lengths(T, buf, depth, window, max_len):
    t, b = len(T), T + buf
    n = len(b)
    end = max(3, n) - 3
    L, D, occ = [0] * (n + 1), [0] * (n + 1), {}
    for i in range(end):
        earlier = occ.setdefault(b[i:i + 3], [])
        if i >= t:
            for c in earlier[-depth:][::-1]:              # c1 > c2 > ... > cK
                if i - c > window:
                    break                                 # the cut-off: nothing older is tried
                length = lazy_model._length(b, i, c, max_len)
                if length > L[i]:                         # (equal lengths: the nearest, met first, stays)
                    L[i], D[i] = length, i - c
        earlier.append(i)
    return tuple(L), tuple(D)


def primed_lengths(T, buf, depth, window=MAX_WINDOW, max_len=MAX_LENGTH):
    """→ (L, D) over the positions of T ‖ buf (0 for every position < |T| and >= end)"""
    return _primed_lengths(usable_tail(T), bytes(buf), depth, window, max_len)


def primed_codes(T, buf, kind, depth, window=MAX_WINDOW, max_len=MAX_LENGTH):
    T, buf = usable_tail(T), bytes(buf)
    L, D = _primed_lengths(T, buf, depth, window, max_len)
    t, b = len(T), T + buf
    end = max(3, len(b)) - 3
    out, i = [], t
    while i < end:
        if L[i] and not (kind == LAZY and L[i + 1] > L[i]):
            out.append((L[i] << 16) | D[i])
            i += L[i]
        else:
            out.append(b[i] << 16)
            i += 1
    return out + [x << 16 for x in b[max(i, t):]]


def later_codes(buf, kind, depth, window=MAX_WINDOW, max_len=MAX_LENGTH):
    """a chunk behind the first one: not primed, §19's / §20's parse"""
    return (lazy_model.lazy_codes if kind == LAZY else chain_model.chain_codes)(bytes(buf), depth, window, max_len)


class PrimedChainLz77(chain_model.ChainLz77):
    """ChainLz77's buffering with the first flush primed by T — an Lz77Encode for the oracle's generic encoder"""

    def __init__(self, T, kind, depth, window=MAX_WINDOW, max_len=MAX_LENGTH, level=LEVEL_BEST):
        super().__init__(depth, window, max_len, level)
        self.T, self.kind, self.first = usable_tail(T), kind, True

    def flush(self, sink):
        if self.first:
            codes = primed_codes(self.T, bytes(self.buf), self.kind, self.depth, self.window, self.max_len)
        else:
            codes = later_codes(self.buf, self.kind, self.depth, self.window, self.max_len)
        self.first = False
        self.buf = bytearray()
        for c in codes:
            sink.append(("Pointer", c >> 16, c & 0xFFFF) if c & 0xFFFF else ("Literal", c >> 16))


def _events(oracle, fmt, enc, data, write_size, writes, opts):
    okw = dict(opts, **oracle.custom_lz77(enc))
    if writes is None:
        return oracle.encode(fmt, data, write_size, **okw)
    e, at = oracle.Encoder(fmt, **okw), 0
    for w in writes:
        if w is None:
            e.flush()
        else:
            e.write(data[at:at + w])
            at += w
    if at < len(data):
        e.write(data[at:])
    return e.finish()


def expected_stream(oracle, fmt, zdict, data, kind, depth, write_size=0, window_size=MAX_WINDOW, max_length=MAX_LENGTH, writes=None,
                    **opts):
    """fmt: "zlib" or "deflate" → the bytes lfx_encode_dict_* must write for `data` behind the chain dictionary `zdict` with
    LFX_LZ77_CHAIN_DEPTH(depth) (kind 2) or LFX_LZ77_LAZY_DEPTH(depth) (kind 3): the oracle's generic encoder over the model's
    code words; the zlib container is the dictionary-less one of the same kind (FLEVEL 3) with FDICT set, FCHECK recomputed and
    DICTID in front of the body.  writes: an explicit schedule (sizes, None is Write::flush()).  opts: the oracle's other
    options (block_size, dynamic_huffman, no_compression ...)."""
    data = bytes(data)
    window, max_len = min(window_size, MAX_WINDOW), min(max_length, MAX_LENGTH)
    mk = lambda: PrimedChainLz77(zdict, kind, depth, window, max_len)
    if fmt == "deflate":
        return _events(oracle, oracle.DEFLATE, mk(), data, write_size, writes, opts)
    z = _events(oracle, oracle.ZLIB, mk(), data, write_size, writes, opts)
    cmf, flg = z[0], (z[1] & 0xC0) | 0x20                                  # FDICT
    if ((cmf << 8) + flg) % 31:
        flg += 31 - ((cmf << 8) + flg) % 31                                # FCHECK
    return bytes([cmf, flg]) + zlib.adler32(bytes(zdict)).to_bytes(4, "big") + z[2:]
