"""The contract of ChainLz77Encoder (include/lfx.h LFX_LZ77_CHAIN) restated in plain Python, and the stream it
implies.  Test infrastructure: checked against the oracle (test_chain_model.py), never against the library.

chain_codes(buf, depth, window, max_len): DefaultLz77Encoder::flush (default.rs:69-109) with one change at a visited position
i < end — instead of the most recent earlier occurrence of buf[i..i+3] alone, the first `depth` of them (most recent first, cut
off at the first one farther than `window`) are measured, and the longest is emitted; among equal lengths the nearest.  Every
position < end is inserted once, in order, as in the reference.  A code word is (val << 16) | dist, dist == 0 a literal — the
oracle's lz77_chunk format.

Two enums meet in this file and share a number by coincidence: the library's LFX_LZ77_CHAIN = 2 (libflate_amd._ffi.LZ77_CHAIN,
which the tests pass to the library) and the oracle's LZ77_CUSTOM = 2 (lfo_oracle.LZ77_CUSTOM, "the caller's own Lz77Encode",
which custom_lz77() below sets for the oracle).  Neither is ever handed to the other side."""

import functools

MAX_WINDOW = 32768
MAX_LENGTH = 258
LEVEL_BEST = 3          # libflate_lz77::CompressionLevel::Best (lib.rs:44-58)


def _length(b, i, c, max_len):
    """3 + longest_common_prefix(buf, i + 3, c + 3) (default.rs:82-87, 122-129): at most max_len, bounded by the end of b"""
    n, k = len(b), 3
    limit = min(max_len, n - i)
    while k < limit and b[i + k] == b[c + k]:
        k += 1
    return k


def chain_codes(buf, depth, window=MAX_WINDOW, max_len=MAX_LENGTH):
    return list(_chain_codes(bytes(buf), depth, window, max_len))


@functools.lru_cache(maxsize=64)      # (the three formats of one case share the parse; the result is a tuple, never changed)
def _chain_codes(b, depth, window, max_len):
    n = len(b)
    end = max(3, n) - 3                                   # default.rs:75
    occ = {}                                              # prefix → its positions so far, in order
    out = []

    def insert(k):
        occ.setdefault(b[k:k + 3], []).append(k)

    i = 0
    while i < end:
        earlier = occ.get(b[i:i + 3], ())
        best_len, best_dist = 0, 0
        for c in earlier[-depth:][::-1]:                  # c1 > c2 > ... > cK
            if i - c > window:
                break                                     # the cut-off: nothing older is tried
            length = _length(b, i, c, max_len)
            if length > best_len:                         # (equal lengths: the nearest, met first, stays)
                best_len, best_dist = length, i - c
        insert(i)
        if best_len:
            out.append((best_len << 16) | best_dist)
            for k in range(i + 1, min(i + best_len, end)):    # default.rs:92-97
                insert(k)
            i += best_len
            continue
        out.append(b[i] << 16)
        i += 1
    for x in b[i:]:                                       # default.rs:105-107
        out.append(x << 16)
    return tuple(out)


def replay(codes):
    """the bytes a decoder makes of the code words"""
    out = bytearray()
    for c in codes:
        c = int(c)
        if c & 0xFFFF:
            d = c & 0xFFFF
            for _ in range(c >> 16):
                out.append(out[-d])
        else:
            out.append(c >> 16)
    return bytes(out)


class ChainLz77:
    """ChainLz77Encoder as an Lz77Encode for the oracle's generic encoder (lfo_oracle.custom_lz77): DefaultLz77Encoder's
    buffering (default.rs:60-68), chain_codes as its flush.  level: what compression_level() answers (Best unless a test
    plays a caller's lz77_level)."""

    def __init__(self, depth, window=MAX_WINDOW, max_len=MAX_LENGTH, level=LEVEL_BEST):
        self.depth, self.window, self.max_len, self.level = depth, window, max_len, level
        self.buf = bytearray()

    def encode(self, buf, sink):
        self.buf += buf
        if len(self.buf) >= self.window * 8:
            self.flush(sink)

    def flush(self, sink):
        codes = chain_codes(bytes(self.buf), self.depth, self.window, self.max_len)
        self.buf = bytearray()
        for c in codes:
            sink.append(("Pointer", c >> 16, c & 0xFFFF) if c & 0xFFFF else ("Literal", c >> 16))

    def compression_level(self):
        return self.level

    def window_size(self):
        return self.window


def expected_stream(oracle, fmt, data, depth, write_size=0, window_size=MAX_WINDOW, max_length=MAX_LENGTH, level=LEVEL_BEST, **opts):
    """fmt: the oracle's format number → the bytes the library must write for `data` with LFX_LZ77_CHAIN_DEPTH(depth): the
    oracle's generic encoder over the model's code words.  opts: the oracle's other options (block_size, dynamic_huffman,
    no_compression, mtime ...)."""
    enc = ChainLz77(depth, min(window_size, MAX_WINDOW), min(max_length, MAX_LENGTH), level)
    return oracle.encode(fmt, bytes(data), write_size, **dict(opts, **oracle.custom_lz77(enc)))


def expected_scheduled(oracle, fmt, data, depth, writes, window_size=MAX_WINDOW, max_length=MAX_LENGTH, level=LEVEL_BEST, **opts):
    """the same for an explicit schedule: `writes` holds sizes, None is Write::flush()"""
    enc = ChainLz77(depth, min(window_size, MAX_WINDOW), min(max_length, MAX_LENGTH), level)
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
