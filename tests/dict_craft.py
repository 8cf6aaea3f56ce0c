"""Fixtures of the preset-dictionary tests (test_dict_abi.py proves them on the CPU, test_gpu_dict_decode.py decodes them on the
GPU): dictionaries, streams written by python-zlib with zdict, and hand-written fixed-Huffman raw DEFLATE for what no encoder
emits on demand.  Everything is deterministic; cases() builds the whole set once per process.

A case: name, fmt ("zlib" / "raw"), zdict (bytes), stream, and either want (the decoded bytes) or err = (status name, message)."""
import random
import zlib
from collections import namedtuple

import deflate_craft as dc

Case = namedtuple("Case", "name fmt zdict stream want err")
WORDS = ("the of and to in is that for it as was with be by on not he this are or his from at which but have an had they you "
         "were their one all we can her has there been if more when will would who so no record field value status error "
         "request response timestamp user session message level info warning host port path query result count total").split()


def text(n, seed):
    """n bytes of word soup (compresses like log lines; the same vocabulary everywhere, so a dictionary of it helps)"""
    rng = random.Random(seed)
    out, size = [], 0
    while size < n:
        w = rng.choice(WORDS) if rng.random() < 0.9 else str(rng.randrange(100000))
        out.append(w)
        size += len(w) + 1
    return " ".join(out).encode()[:n]


D32 = text(32768, 1)
D40 = text(40000, 2)           # longer than the window: the id covers all of it, only the last 32768 bytes are reachable
D300 = text(300, 3)
DAB = text(500, 4) + b"ab"
D1 = b"q"
D0 = b""


def wbits(fmt):
    return 15 if fmt == "zlib" else -15


def compress(fmt, data, zdict, level=9):
    co = zlib.compressobj(level, zlib.DEFLATED, wbits(fmt), zdict=zdict) if zdict is not None else \
        zlib.compressobj(level, zlib.DEFLATED, wbits(fmt))
    return co.compress(data) + co.flush()


def py_inflate(fmt, stream, zdict):
    """python-zlib's verdict: the bytes, or raises zlib.error"""
    d = zlib.decompressobj(wbits(fmt), zdict=zdict)
    return d.decompress(stream) + d.flush()


def crafted(tokens, zdict):
    """one final fixed-Huffman block of `tokens` as raw DEFLATE, and what it decodes to behind zdict's usable tail"""
    bits = dc.BitWriter()
    dc.fixed_block(bits, tokens, True)
    hist = zdict[-32768:]
    return bits.getvalue(), dc.expand(tokens, hist)[len(hist):]


def record(i, lo=100, hi=2000):
    rng = random.Random(1000 + i)
    return text(rng.randrange(lo, hi + 1), 5000 + i)


def large_text():
    """1.5 MiB of text behind 3000 bytes of D32's tail"""
    return D32[-3000:] + text((3 << 19) - 3000, 77)


_cases = None


def cases():
    global _cases
    if _cases is not None:
        return _cases
    out = []

    def gen(name, fmt, data, zdict, level=9):
        out.append(Case(name, fmt, zdict, compress(fmt, data, zdict, level), data, None))

    # ---- serial kernel: small records, both containers
    body = text(1100, 10)
    for fmt in ("zlib", "raw"):
        for n in (1, 100, 1100):
            gen("rec%d_%s_d32" % (n, fmt), fmt, body[:n], D32)
        gen("rec1100_%s_d1" % fmt, fmt, (b"q" * 40 + body)[:1100], D1)
        gen("rec1100_%s_d0" % fmt, fmt, body, D0)
        gen("rec1100_%s_d40" % fmt, fmt, D40[8000:8600] + body[:500], D40)       # (reaches near the oldest usable byte)
    # ---- hand-written: what no encoder emits on demand
    for name, tokens, zd in (("first_byte_258", [(258, 300)], D300),                 # reads the dictionary's first usable byte
                             ("dist_32768", [(258, 32768)], D32),
                             ("dist_32768_d40", [(258, 32768), 65, (4, 32768)], D40),
                             ("overlap_ab", [(258, 2), 120, (10, 261)], DAB),         # starts in the dictionary, runs on into the output
                             ("legal_after_5", [104, 101, 108, 108, 111, (3, 301)], D300)):
        z, want = crafted(tokens, zd)
        out.append(Case("craft_" + name, "raw", zd, z, want, None))
    bits = dc.BitWriter()
    dc.fixed_block(bits, [(3, 301)], True)       # distance = usable length + 1 at output 0
    out.append(Case("craft_too_far", "raw", D300, bits.getvalue(), b"",
                    ("E_INVALID_DATA", "Too long backword reference: buffer.len=300, distance=301")))
    # ---- block rounds
    head = D32[-3000:] + text(65536 - 3000, 20)
    gen("blk64k_zlib", "zlib", head, D32, 6)
    gen("blk64k_raw", "raw", head, D32, 6)
    co = zlib.compressobj(9, zlib.DEFLATED, -15, zdict=D32)
    a = text(5000, 21)
    s = co.compress(a) + co.flush(zlib.Z_SYNC_FLUSH) + co.compress(D32[20000:24000]) + co.flush()
    out.append(Case("sync_flush_reach", "raw", D32, s, a + D32[20000:24000], None))   # the second block reaches across the first
    # ---- large member (the finder path)
    big = large_text()
    gen("large_zlib", "zlib", big, D32, 6)
    _cases = out
    return out


def by_name(name):
    return next(c for c in cases() if c.name == name)


def batch_records(n):
    """n zlib records of 100-2000 bytes that share D32 → [(stream, record)]"""
    return [(compress("zlib", record(i), D32), record(i)) for i in range(n)]
