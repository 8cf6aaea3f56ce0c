"""The contract of LazyLz77Encoder (include/lfx.h LFX_LZ77_LAZY) restated in plain Python, and the stream it
implies.  Test infrastructure: checked against chain_model and python-zlib (test_lazy_model.py), never against the library.

lengths(buf, depth, window, max_len) → (L, D): for every position p < end with candidates the length and the distance
ChainLz77Encoder emits there (chain_model: the longest of the first `depth` earlier occurrences of buf[p..p+3], most recent
first, cut off at the first one farther than `window`; among equal lengths the nearest); L = 0 where there is none and for every
p >= end.  They do not depend on the parse: every position < end is inserted once, in order.

lazy_codes: the walk.  At a visited i < end with L(i) != 0 and L(i + 1) <= L(i): Pointer{L(i), D(i)}, i += L(i); otherwise
Literal(buf[i]), i += 1 — zlib's deflate_slow rule without max_lazy, good_length or TOO_FAR.  greedy_codes walks the same
(L, D) the way chain_model does, which is how the two models are shown to share their candidates.  A code word is
(val << 16) | dist, dist == 0 a literal — the oracle's lz77_chunk format.

As in chain_model, the library's LFX_LZ77_LAZY = 3 (libflate_amd._ffi.LZ77_LAZY) and the oracle's LZ77_CUSTOM never meet."""

import functools

import chain_model
from chain_model import LEVEL_BEST, MAX_LENGTH, MAX_WINDOW, replay  # noqa: F401  (replay: for the tests)


def _length(b, i, c, max_len):
    """chain_model._length, sixteen bytes at a time while they agree (every position is measured here, not only the visited)"""
    k, limit = 3, min(max_len, len(b) - i)
    while k + 16 <= limit and b[i + k:i + k + 16] == b[c + k:c + k + 16]:
        k += 16
    while k < limit and b[i + k] == b[c + k]:
        k += 1
    return k


@functools.lru_cache(maxsize=64)      # (the formats and the walks of one case share the lengths; tuples, never changed)
def _lengths(b, depth, window, max_len):
    n = len(b)
    end = max(3, n) - 3                                   # default.rs:75
    L, D, occ = [0] * (n + 1), [0] * (n + 1), {}
    for i in range(end):
        earlier = occ.setdefault(b[i:i + 3], [])
        for c in earlier[-depth:][::-1]:                  # c1 > c2 > ... > cK
            if i - c > window:
                break                                     # the cut-off: nothing older is tried
            length = _length(b, i, c, max_len)
            if length > L[i]:                             # (equal lengths: the nearest, met first, stays)
                L[i], D[i] = length, i - c
        earlier.append(i)
    return tuple(L), tuple(D)


def lengths(buf, depth, window=MAX_WINDOW, max_len=MAX_LENGTH):
    return _lengths(bytes(buf), depth, window, max_len)


def _walk(b, L, D, lazy):
    n = len(b)
    end = max(3, n) - 3
    out, i = [], 0
    while i < end:
        if L[i] and not (lazy and L[i + 1] > L[i]):
            out.append((L[i] << 16) | D[i])
            i += L[i]
        else:
            out.append(b[i] << 16)
            i += 1
    return out + [x << 16 for x in b[i:]]                 # default.rs:105-107


def lazy_codes(buf, depth, window=MAX_WINDOW, max_len=MAX_LENGTH):
    b = bytes(buf)
    return _walk(b, *_lengths(b, depth, window, max_len), lazy=True)


def greedy_codes(buf, depth, window=MAX_WINDOW, max_len=MAX_LENGTH):
    b = bytes(buf)
    return _walk(b, *_lengths(b, depth, window, max_len), lazy=False)


class LazyLz77(chain_model.ChainLz77):
    """LazyLz77Encoder as an Lz77Encode for the oracle's generic encoder: ChainLz77's buffering, lazy_codes as its flush"""

    def flush(self, sink):
        codes = lazy_codes(bytes(self.buf), self.depth, self.window, self.max_len)
        self.buf = bytearray()
        for c in codes:
            sink.append(("Pointer", c >> 16, c & 0xFFFF) if c & 0xFFFF else ("Literal", c >> 16))


def expected_stream(oracle, fmt, data, depth, write_size=0, window_size=MAX_WINDOW, max_length=MAX_LENGTH, level=LEVEL_BEST, **opts):
    """fmt: the oracle's format number → the bytes the library must write for `data` with LFX_LZ77_LAZY_DEPTH(depth): the
    oracle's generic encoder over the model's code words.  opts: the oracle's other options (block_size, dynamic_huffman,
    no_compression, mtime ...)."""
    enc = LazyLz77(depth, min(window_size, MAX_WINDOW), min(max_length, MAX_LENGTH), level)
    return oracle.encode(fmt, bytes(data), write_size, **dict(opts, **oracle.custom_lz77(enc)))


def expected_scheduled(oracle, fmt, data, depth, writes, window_size=MAX_WINDOW, max_length=MAX_LENGTH, level=LEVEL_BEST, **opts):
    """the same for an explicit schedule: `writes` holds sizes, None is Write::flush()"""
    enc = LazyLz77(depth, min(window_size, MAX_WINDOW), min(max_length, MAX_LENGTH), level)
    e = oracle.Encoder(fmt, **dict(opts, **oracle.custom_lz77(enc)))
    data, at = bytes(data), 0
    for w in writes:
        if w is None:
            e.flush()
        else:
            e.write(data[at:at + w])
            at += w
    if at < len(data):
        e.write(data[at:])
    return e.finish()
