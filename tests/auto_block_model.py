"""The contract of LFX_HUFFMAN_AUTO (include/lfx.h) restated in plain Python, and the stream it implies.  Test
infrastructure: checked against the oracle and python-zlib (test_auto_block_model.py), never against the library.

The plan, the code words and the block boundaries are those of dynamic_huffman = 1, so the `= 1` and the `= 0` encode of one
call have the same blocks, and a block chosen dynamic (fixed) carries exactly its bits of the `= 1` (`= 0`) encode.  The model
therefore takes those two streams, cuts both at the oracle's scan_blocks, and splices:

  D = the block's bits in the `= 1` stream, F = its bits in the `= 0` stream, S = 8 * in_len + 42 (in_len: the bytes the block
  decodes to).  Stored when it is eligible (bytes mode, 1 <= in_len <= 65535) and S < min(D, F); otherwise fixed when F <= D;
  otherwise dynamic.  A block that is stored in the `= 1` stream already (no_compression, the zlib sync marker) is copied.
"""
import struct

STORED, FIXED, DYNAMIC = 0, 1, 2
TRAILER = {"deflate": 0, "zlib": 4, "gzip": 8}


def header_len(fmt, stream):
    """bytes in front of the DEFLATE data"""
    if fmt == "deflate":
        return 0
    if fmt == "zlib":
        return 6 if stream[1] & 0x20 else 2
    flg, at = stream[3], 10
    if flg & 4:
        at += 2 + struct.unpack_from("<H", stream, at)[0]
    for bit in (8, 16):
        if flg & bit:
            at = stream.index(b"\0", at) + 1
    return at + (2 if flg & 2 else 0)


def choose(D, F, in_len, stored_ok=True):
    """the rule of the contract → STORED, FIXED or DYNAMIC"""
    if stored_ok and 1 <= in_len <= 65535 and 8 * in_len + 42 < min(D, F):
        return STORED
    return FIXED if F <= D else DYNAMIC


class _Bits:
    """an LSB-first bit string (BitWriter, bit.rs:25-49) as one Python integer"""

    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, bits, width):
        self.v |= bits << self.n
        self.n += width

    def align(self):
        self.n = (self.n + 7) & ~7

    def bytes(self):
        self.align()
        return self.v.to_bytes(self.n // 8, "little")


def scan(oracle, raw, zdict=None):
    """the oracle's scan_blocks; behind a preset dictionary the stream reads history it does not hold, so the dictionary's tail
    goes in front as a stored block (it ends on a byte boundary) and is taken off the answer again"""
    if not zdict:
        return oracle.scan_blocks(raw)
    tail = bytes(zdict)[-32768:]
    pre = b"\x00" + struct.pack("<HH", len(tail), len(tail) ^ 0xFFFF) + tail
    return [(s - 8 * len(pre), e - 8 * len(pre), btype, bfinal, n) for s, e, btype, bfinal, n in oracle.scan_blocks(pre + raw)[1:]]


def splice(oracle, dyn_raw, fix_raw, data, stored_ok=True, zdict=None):
    """dyn_raw / fix_raw: the raw DEFLATE data of the `= 1` and the `= 0` encode of `data` → (raw DEFLATE of the AUTO encode,
    [the chosen form per block], [(D, F, in_len) per candidate block, None for a copied one])"""
    bd, bf = scan(oracle, dyn_raw, zdict), scan(oracle, fix_raw, zdict)
    assert len(bd) == len(bf) and [b[3:] for b in bd] == [b[3:] for b in bf], "the two encodes have different blocks"
    vd, vf = int.from_bytes(dyn_raw, "little"), int.from_bytes(fix_raw, "little")
    out, choices, sizes, at = _Bits(), [], [], 0
    for (s, e, btype, bfinal, n), (sf, ef, ftype, _, _) in zip(bd, bf):
        if btype == STORED:
            assert ftype == STORED
            pick, stored_bytes = STORED, data[at:at + n]
            sizes.append(None)
        else:
            assert btype == DYNAMIC and ftype == FIXED
            pick, stored_bytes = choose(e - s, ef - sf, n, stored_ok), data[at:at + n]
            sizes.append((e - s, ef - sf, n))
        if pick == DYNAMIC:
            out.put((vd >> s) & ((1 << (e - s)) - 1), e - s)
        elif pick == FIXED:
            out.put((vf >> sf) & ((1 << (ef - sf)) - 1), ef - sf)
        else:                                   # RawBuf::flush encode.rs:364-382: BFINAL, BTYPE 00, byte-align, LEN, NLEN, bytes
            out.put(bfinal, 3)
            out.align()
            out.put(n | ((n ^ 0xFFFF) << 16), 32)
            out.put(int.from_bytes(stored_bytes, "little"), 8 * n)
        choices.append(pick)
        at += n
    assert at == len(data)
    return out.bytes(), choices, sizes


def expected_stream(oracle, fmt, dyn, fix, data, stored_ok=True, zdict=None):
    """fmt: "deflate", "zlib" or "gzip"; dyn / fix: the whole `= 1` / `= 0` streams (container included) of one call over `data`
    → (the bytes the LFX_HUFFMAN_AUTO call must write, choices, sizes).  The container header and the trailer are the `= 1`
    stream's: neither depends on the blocks' forms."""
    h, t = header_len(fmt, dyn), TRAILER[fmt]
    assert dyn[:h] == fix[:h] and (t == 0 or dyn[-t:] == fix[-t:])
    raw, choices, sizes = splice(oracle, dyn[h:len(dyn) - t], fix[h:len(fix) - t], bytes(data), stored_ok, zdict)
    return dyn[:h] + raw + (dyn[-t:] if t else b""), choices, sizes


def expected(oracle, fmt, data, stored_ok=True, encode=None, zdict=None, **opts):
    """the same over the oracle's own encodes; encode(fmt name, data, **opts) → bytes: another source of the two streams (a
    model of a preset dictionary or of an opt-in LZ77 kind), called with dynamic_huffman=1 and =0; zdict: the preset dictionary those
    streams were written behind"""
    data = bytes(data)
    if encode is None:
        code = {"deflate": oracle.DEFLATE, "zlib": oracle.ZLIB, "gzip": oracle.GZIP}[fmt]
        encode = lambda f, d, **kw: oracle.encode(code, d, **kw)
    dyn, fix = encode(fmt, data, **dict(opts, dynamic_huffman=1)), encode(fmt, data, **dict(opts, dynamic_huffman=0))
    return expected_stream(oracle, fmt, dyn, fix, data, stored_ok, zdict)


def oracle_writes(oracle, fmt, data, writes, **opts):
    """the oracle's stream for an explicit schedule: sizes, None is Write::flush(); what is left goes in one last write"""
    code = {"deflate": oracle.DEFLATE, "zlib": oracle.ZLIB, "gzip": oracle.GZIP}[fmt]
    e, at = oracle.Encoder(code, **opts), 0
    for w in writes:
        if w is None:
            e.flush()
        else:
            e.write(data[at:at + w])
            at += w
    if at < len(data):
        e.write(data[at:])
    return e.finish()


def expected_writes(oracle, fmt, data, writes, stored_ok=True, **opts):
    return expected(oracle, fmt, data, stored_ok, encode=lambda f, d, **kw: oracle_writes(oracle, f, d, writes, **kw), **opts)
