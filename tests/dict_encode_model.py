"""The contract of the dictionary-primed encode (include/lfx.h "encoding with a preset dictionary") restated in
plain Python, and the stream it implies.  Test infrastructure: checked against the oracle (test_dict_encode_model.py), never
against the library.

primed_codes(T, buf, window, max_len): the code words DefaultLz77Encoder::flush (default.rs:69-109) writes for the buffer
T ‖ buf when its prefix table already holds every position < |T|, each inserted once, in order, and its walk starts at |T|.
A code word is (val << 16) | dist, dist == 0 a literal — the oracle's lz77_chunk format."""
import zlib

MAX_WINDOW = 32768


def usable_tail(zdict):
    return bytes(zdict)[-MAX_WINDOW:] if len(zdict) else b""


def _lcp(b, i, j, limit):
    """longest_common_prefix (default.rs:122-129): b[i..] against b[j..], at most `limit` bytes, bounded by the end of b"""
    n, k = len(b), 0
    limit = min(limit, n - i)
    while k < limit and b[i + k] == b[j + k]:
        k += 1
    return k


def primed_codes(T, buf, window=32768, max_len=258):
    T = usable_tail(T)
    t = len(T)
    b = T + bytes(buf)
    n = len(b)
    end = max(3, n) - 3                                   # default.rs:75
    table = {}
    for j in range(t):                                    # the table as the walk finds it: every position of T, in order
        if j + 3 <= n:
            table[b[j:j + 3]] = j
    out = []
    i = t
    while i < end:
        key = b[i:i + 3]
        j = table.get(key)
        table[key] = i                                    # PrefixTable::insert returns the old position (default.rs:78)
        if j is not None and i - j <= window:
            length = 3 + _lcp(b, i + 3, j + 3, max_len - 3)
            out.append((length << 16) | (i - j))
            for k in range(i + 1, min(i + length, end)):  # default.rs:92-97
                table[b[k:k + 3]] = k
            i += length
            continue
        out.append(b[i] << 16)
        i += 1
    for x in b[max(i, t):]:                               # default.rs:105-107
        out.append(x << 16)
    return out


def boundary_at(codes, t):
    """→ the index of the first code word behind input position t of a parse, or None when a match runs across t"""
    pos = 0
    for k, c in enumerate(codes):
        if pos == t:
            return k
        if pos > t:
            return None
        c = int(c)
        pos += (c >> 16) if (c & 0xFFFF) else 1
    return len(codes) if pos == t else None


class PrimedLz77:
    """DefaultLz77Encoder's buffering (default.rs:60-68) with the first flush primed by T — an Lz77Encode for the oracle's
    generic encoder (lfo_oracle.custom_lz77)."""

    def __init__(self, oracle, T, window=32768, max_len=258):
        self.o, self.T, self.window, self.max_len = oracle, usable_tail(T), window, max_len
        self.buf = bytearray()
        self.first = True

    def encode(self, buf, sink):
        self.buf += buf
        if len(self.buf) >= self.window * 8:
            self.flush(sink)

    def flush(self, sink):
        if self.first:
            codes = primed_codes(self.T, bytes(self.buf), self.window, self.max_len)
        else:
            codes = [int(c) for c in self.o.lz77_chunk(bytes(self.buf), self.window, self.max_len)]
        self.first = False
        self.buf = bytearray()
        for c in codes:
            sink.append(("Pointer", c >> 16, c & 0xFFFF) if c & 0xFFFF else ("Literal", c >> 16))

    def compression_level(self):
        return 2

    def window_size(self):
        return self.window


def expected_stream(oracle, fmt, zdict, data, write_size=0, window_size=32768, max_length=258, **opts):
    """fmt: "zlib" or "deflate" → the bytes lfx_encode_dict_* must write for `data` behind the dictionary `zdict` (all its
    bytes: the id covers them, the tail primes).  The body is the oracle's generic encoder over the model's code words for the
    first chunk and lz77_chunk's for the rest; options that do no matching keep the oracle's own body."""
    data = bytes(data)
    plain = dict(opts, window_size=window_size, max_length=max_length)
    if opts.get("no_compression") or opts.get("lz77_kind") == oracle.LZ77_NOCOMPRESSION:
        body = oracle.encode(oracle.DEFLATE, data, write_size, **plain)
    else:
        body = oracle.encode(oracle.DEFLATE, data, write_size,
                             **dict(opts, **oracle.custom_lz77(PrimedLz77(oracle, zdict, window_size, max_length))))
    if fmt == "deflate":
        return body
    head = oracle.encode(oracle.ZLIB, data, write_size, **plain)[:2]      # CMF and FLEVEL as the dictionary-less call writes them
    cmf, flg = head[0], (head[1] & 0xC0) | 0x20                           # FDICT
    if ((cmf << 8) + flg) % 31:
        flg += 31 - ((cmf << 8) + flg) % 31                               # FCHECK
    return bytes([cmf, flg]) + zlib.adler32(bytes(zdict)).to_bytes(4, "big") + body + zlib.adler32(data).to_bytes(4, "big")


def py_inflate(fmt, stream, zdict):
    """python-zlib's reading of a stream with a preset dictionary → the bytes (raises zlib.error)"""
    d = zlib.decompressobj(15 if fmt == "zlib" else -15, zdict=bytes(zdict))
    out = d.decompress(bytes(stream)) + d.flush()
    assert d.eof and not d.unused_data
    return out
