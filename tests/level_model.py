"""The contract of LevelLz77Encoder (include/lfx.h LFX_LZ77_LEVEL) restated in plain Python, and the stream it
implies.  Test infrastructure: checked against chain_model, lazy_model and python-zlib (test_level_model.py), never against the
library.

TABLE: level → (depth K, lazy, nice N, max_lazy Z, too_far F) — zlib's configuration_table without good_length.  NEVER stands
for "the rule does not apply": the greedy levels have no Z and no F.

lengths(buf, depth, nice, too_far, window, max_len) → (L, D): lazy_model's per-position lengths with two more rules.  The walk
along the candidates c1 > c2 > ... (the first `depth` earlier occurrences of buf[p..p+3], cut off at the first one farther than
`window`) ends behind the first candidate whose length is >= min(nice, lim), lim = min(max_len, n - p), that candidate included;
the greatest length among the candidates walked wins, among equal lengths the nearest.  Then, too_far: L == 3 and D > too_far
is no candidate, L = 0.  L = 0 for every p >= end.  Both are functions of the position alone.

walk: greedy (max_lazy None: chain_model's walk over L, D) or lazy — at a visited i < end a Pointer when L(i) != 0 and
(L(i) >= max_lazy or L(i + 1) <= L(i)), otherwise a literal.  The tail is the reference's.  A code word is (val << 16) | dist,
dist == 0 a literal — the oracle's lz77_chunk format.  good_length is not modelled (include/lfx.h says why).

The dictionary functions mirror dict_chain_model: the same rules over T ‖ buf, candidates from position |T| on."""
import functools
import zlib

import chain_model
import lazy_model
from chain_model import MAX_LENGTH, MAX_WINDOW, replay  # noqa: F401  (replay: for the tests)
from dict_encode_model import usable_tail

NEVER = 1 << 32
LEVEL_KIND = 4                # lz77_kind & 0xFF of the library (never handed to the oracle)
#        level: (K, lazy, N, Z, F)
TABLE = {1: (4, False, 8, NEVER, NEVER),
         2: (8, False, 16, NEVER, NEVER),
         3: (32, False, 32, NEVER, NEVER),
         4: (16, True, 16, 4, 4096),
         5: (32, True, 32, 16, 4096),
         6: (128, True, 128, 16, 4096),
         7: (256, True, 128, 32, 4096),
         8: (1024, True, 258, 128, 4096),
         9: (4096, True, 258, 258, 4096)}


def header_level(level):
    """libflate_lz77::CompressionLevel of a level: Fast (1) for 1..3, Balance (2) for 4..6, Best (3) for 7..9"""
    return 1 if level <= 3 else 3 if level >= 7 else 2


@functools.lru_cache(maxsize=128)     # (the formats and the levels of one case share the lengths; tuples, never changed)
def _lengths(b, t, depth, nice, too_far, window, max_len):
    """over b, candidates evaluated from position t on (t = 0: a buffer of its own; t = |T|: behind a dictionary's tail)"""
    n = len(b)
    end = max(3, n) - 3                                   # default.rs:75
    L, D, occ = [0] * (n + 1), [0] * (n + 1), {}
    for i in range(end):
        earlier = occ.setdefault(b[i:i + 3], [])
        if i >= t:
            stop = min(nice, max_len, n - i)
            for c in earlier[-depth:][::-1]:              # c1 > c2 > ... > cK
                if i - c > window:
                    break                                 # the cut-off: nothing older is tried
                length = lazy_model._length(b, i, c, max_len)
                if length > L[i]:                         # (equal lengths: the nearest, met first, stays)
                    L[i], D[i] = length, i - c
                if length >= stop:
                    break                                 # a nice match: the walk ends behind it
            if L[i] == 3 and D[i] > too_far:
                L[i], D[i] = 0, 0                         # too far
        earlier.append(i)
    return tuple(L), tuple(D)


def lengths(buf, depth, nice=MAX_LENGTH, too_far=NEVER, window=MAX_WINDOW, max_len=MAX_LENGTH):
    return _lengths(bytes(buf), 0, depth, nice, too_far, window, max_len)


def _walk(b, L, D, max_lazy, start=0):
    """max_lazy None: the greedy walk"""
    end = max(3, len(b)) - 3
    out, i = [], start
    while i < end:
        if L[i] and (max_lazy is None or L[i] >= max_lazy or L[i + 1] <= L[i]):
            out.append((L[i] << 16) | D[i])
            i += L[i]
        else:
            out.append(b[i] << 16)
            i += 1
    return out + [x << 16 for x in b[max(i, start):]]     # default.rs:105-107


def tuned_codes(buf, depth, lazy, nice, max_lazy, too_far, window=MAX_WINDOW, max_len=MAX_LENGTH):
    """the five values spelled out (the tests set them apart from the table)"""
    b = bytes(buf)
    L, D = _lengths(b, 0, depth, nice, too_far if lazy else NEVER, window, max_len)
    return _walk(b, L, D, max_lazy if lazy else None)


def level_codes(buf, level, window=MAX_WINDOW, max_len=MAX_LENGTH):
    depth, lazy, nice, max_lazy, too_far = TABLE[level]
    return tuned_codes(buf, depth, lazy, nice, max_lazy, too_far, window, max_len)


def level_lengths(buf, level, window=MAX_WINDOW, max_len=MAX_LENGTH):
    depth, lazy, nice, _max_lazy, too_far = TABLE[level]
    return _lengths(bytes(buf), 0, depth, nice, too_far if lazy else NEVER, window, max_len)


def primed_codes(T, buf, level, window=MAX_WINDOW, max_len=MAX_LENGTH):
    """the first chunk behind a chain dictionary's usable tail T (dict_chain_model.primed_codes under the level's rules)"""
    depth, lazy, nice, max_lazy, too_far = TABLE[level]
    T, buf = usable_tail(T), bytes(buf)
    b = T + buf
    L, D = _lengths(b, len(T), depth, nice, too_far if lazy else NEVER, window, max_len)
    return _walk(b, L, D, max_lazy if lazy else None, start=len(T))


class LevelLz77(chain_model.ChainLz77):
    """LevelLz77Encoder as an Lz77Encode for the oracle's generic encoder: ChainLz77's buffering, level_codes as its flush;
    T: a chain dictionary, which primes the first flush"""

    def __init__(self, level, window=MAX_WINDOW, max_len=MAX_LENGTH, header=None, T=None):
        super().__init__(TABLE[level][0], window, max_len, header_level(level) if header is None else header)
        self.lvl, self.T = level, T

    def flush(self, sink):
        if self.T is not None:
            codes, self.T = primed_codes(self.T, bytes(self.buf), self.lvl, self.window, self.max_len), None
        else:
            codes = level_codes(bytes(self.buf), self.lvl, self.window, self.max_len)
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


def expected_stream(oracle, fmt, data, level, write_size=0, window_size=MAX_WINDOW, max_length=MAX_LENGTH, header=None, writes=None,
                    **opts):
    """fmt: the oracle's format number → the bytes the library must write for `data` with LFX_LZ77_LEVEL_N(level): the oracle's
    generic encoder over the model's code words.  header: a caller's lz77_level - 1 (None: the level's own).  writes: an
    explicit schedule (sizes, None is Write::flush()).  opts: the oracle's other options (block_size, dynamic_huffman,
    no_compression, mtime ...)."""
    enc = LevelLz77(level, min(window_size, MAX_WINDOW), min(max_length, MAX_LENGTH), header)
    return _events(oracle, fmt, enc, bytes(data), write_size, writes, opts)


def expected_dict_stream(oracle, fmt, zdict, data, level, write_size=0, window_size=MAX_WINDOW, max_length=MAX_LENGTH, writes=None, **opts):
    """fmt: "zlib" or "deflate" → the bytes lfx_encode_dict_* must write behind the chain dictionary `zdict` (the container as
    in dict_chain_model.expected_stream: FDICT set, FCHECK recomputed, DICTID in front of the body)"""
    mk = lambda: LevelLz77(level, min(window_size, MAX_WINDOW), min(max_length, MAX_LENGTH), None, bytes(zdict))
    if fmt == "deflate":
        return _events(oracle, oracle.DEFLATE, mk(), bytes(data), write_size, writes, opts)
    z = _events(oracle, oracle.ZLIB, mk(), bytes(data), write_size, writes, opts)
    cmf, flg = z[0], (z[1] & 0xC0) | 0x20                                  # FDICT
    if ((cmf << 8) + flg) % 31:
        flg += 31 - ((cmf << 8) + flg) % 31                                # FCHECK
    return bytes([cmf, flg]) + zlib.adler32(bytes(zdict)).to_bytes(4, "big") + z[2:]
