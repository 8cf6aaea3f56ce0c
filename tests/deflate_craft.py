"""A DEFLATE writer for tests: legal streams that neither this library's encoder nor python-zlib writes, and rejects decided in a
header or by one symbol.  Every header field of a dynamic block can be overridden; `expand` is the plain model of what a token
list decodes to.  CASES is the list the CPU test (test_craft_streams.py) fixes against the oracle and the GPU test
(test_gpu_craft_decode.py) then feeds to the decode entry points.  All randomness is a seeded random.Random."""
import bisect
import functools
import random
import struct
import zlib
from collections import namedtuple

KIB = 1 << 10
MIB = 1 << 20

# ------------------------------------------------------------------------------------------------ the symbol tables (RFC 1951 §3.2.5-7)
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8          # 288 lengths: 286 and 287 have codes
FIXED_DIST = [5] * 32                                           # 30 and 31 have codes
# every code-length symbol has a code: thirteen of 4 bits, six of 5 — complete
DEFAULT_CL = [4] * 10 + [5] * 6 + [4] * 3

Sym = namedtuple("Sym", "kind sym extra")       # a raw symbol of the literal/length ("L") or distance ("D") alphabet, for rejects


def len_symbol(length, len258_as_284=False):
    """→ (symbol, extra bits, extra value)"""
    if length == 258 and not len258_as_284:
        return 285, 0, 0
    i = bisect.bisect_right(LEN_BASE, length, 0, 28) - 1
    return 257 + i, LEN_EXTRA[i], length - LEN_BASE[i]


def dist_symbol(distance):
    i = bisect.bisect_right(DIST_BASE, distance) - 1
    return i, DIST_EXTRA[i], distance - DIST_BASE[i]


# ------------------------------------------------------------------------------------------------ bits
class BitWriter:
    """LSB first (RFC 1951 §3.1.1)"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, w):
        self.acc |= v << self.n
        self.n += w
        if self.n >= 512:
            k = self.n >> 3
            self.out += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def bitpos(self):
        return len(self.out) * 8 + self.n

    def align(self):
        if self.n & 7:
            self.put(0, 8 - (self.n & 7))

    def put_bytes(self, data):
        assert self.n & 7 == 0
        self.out += self.acc.to_bytes(self.n >> 3, "little")
        self.acc, self.n = 0, 0
        self.out += data

    def getvalue(self):
        self.align()
        self.put_bytes(b"")
        return bytes(self.out)


def canonical(lengths):
    """the canonical codes (RFC 1951 §3.2.2) of a list of lengths, MSB first as the RFC prints them; None where the length is 0.
    An over-subscribed list gives codes wider than their lengths: `code_table` keeps their low bits."""
    code, out, prev = 0, [None] * len(lengths), 0
    for w in range(1, 16):
        for s, l in enumerate(lengths):
            if l == w:
                code <<= w - prev
                prev = w
                out[s] = code
                code += 1
    return out


def _reverse(v, w):
    r = 0
    for _ in range(w):
        r = (r << 1) | (v & 1)
        v >>= 1
    return r


def code_table(lengths):
    """[(bit-reversed code, length) or None]: a code goes out in one BitWriter.put"""
    return [None if c is None else (_reverse(c & ((1 << l) - 1), l), l) for c, l in zip(canonical(lengths), lengths)]


def flat_lengths(n):
    """a complete code for n ≥ 2 symbols: lengths ⌈log2 n⌉ - 1 and ⌈log2 n⌉"""
    k = (n - 1).bit_length()
    short = (1 << k) - n
    return [k - 1] * short + [k] * (n - short)


def sparse(size, assign):
    """lengths list of `size` with assign = {symbol: length}"""
    out = [0] * size
    for s, l in assign.items():
        out[s] = l
    return out


# ------------------------------------------------------------------------------------------------ blocks
def _tokens(bits, lit, dist, tokens, len258_as_284=False):
    put = bits.put
    for t in tokens:
        if isinstance(t, int):
            put(*lit[t])
        elif isinstance(t, Sym):
            put(*(lit if t.kind == "L" else dist)[t.sym])
            if t.extra:
                put(*t.extra)
        else:
            s, eb, ev = len_symbol(t[0], len258_as_284)
            put(*lit[s])
            if eb:
                put(ev, eb)
            s, eb, ev = dist_symbol(t[1])
            put(*dist[s])
            if eb:
                put(ev, eb)


def rle(lengths, use_repeat_codes=True):
    """the code-length symbols of a list of lengths → [(symbol, extra value)]"""
    out, i, n = [], 0, len(lengths)
    while i < n:
        v, run = lengths[i], 1
        while i + run < n and lengths[i + run] == v:
            run += 1
        i += run
        if not use_repeat_codes:
            out += [(v, 0)] * run
        elif v == 0:
            while run >= 11:
                k = min(run, 138)
                out.append((18, k - 11))
                run -= k
            if run >= 3:
                out.append((17, run - 3))
                run = 0
            out += [(0, 0)] * run
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append((16, k - 3))
                run -= k
            out += [(v, 0)] * run
    return out


_CL_EXTRA = {16: 2, 17: 3, 18: 7}


def dyn_block(bits, lit_lengths, dist_lengths, tokens, final, *, nl=None, nd=None, use_repeat_codes=True, cl_lengths=None, hclen=None,
              header_symbols=None, len258_as_284=False, write_eob=True):
    """A dynamic-Huffman block.  nl / nd: how many literal/length and distance lengths the header announces (default: up to the
    last one that is not 0, at least 257 / 1); cl_lengths: the 19 lengths of the code-length code; hclen: how many of them have a
    field; header_symbols: the [(symbol, extra value)] list written in place of the run-length coding of the nl + nd lengths."""
    if nl is None:
        nl = max(257, max(i + 1 for i, l in enumerate(lit_lengths) if l))
    if nd is None:
        nd = max([1] + [i + 1 for i, l in enumerate(dist_lengths) if l])
    ll = (list(lit_lengths) + [0] * nl)[:nl]
    dl = (list(dist_lengths) + [0] * nd)[:nd]
    cl = list(DEFAULT_CL if cl_lengths is None else cl_lengths)
    if hclen is None:
        hclen = max(4, max(k + 1 for k, s in enumerate(CLEN_ORDER) if cl[s]))
    if header_symbols is None:
        header_symbols = rle(ll + dl, use_repeat_codes)
    bits.put(1 if final else 0, 1)
    bits.put(2, 2)
    bits.put(nl - 257, 5)
    bits.put(nd - 1, 5)
    bits.put(hclen - 4, 4)
    for s in CLEN_ORDER[:hclen]:
        bits.put(cl[s], 3)
    clt = code_table(cl)
    for s, extra in header_symbols:
        bits.put(*clt[s])
        if s >= 16:
            bits.put(extra, _CL_EXTRA[s])
    lit, dist = code_table(ll), code_table(dl)
    _tokens(bits, lit, dist, tokens, len258_as_284)
    if write_eob:
        bits.put(*lit[256])


_FIXED = (code_table(FIXED_LIT), code_table(FIXED_DIST))


def fixed_block(bits, tokens, final, write_eob=True):
    bits.put(1 if final else 0, 1)
    bits.put(1, 2)
    _tokens(bits, _FIXED[0], _FIXED[1], tokens)
    if write_eob:
        bits.put(*_FIXED[0][256])


def stored_block(bits, data, final):
    assert len(data) <= 65535
    bits.put(1 if final else 0, 1)
    bits.put(0, 2)
    bits.align()
    bits.put_bytes(len(data).to_bytes(2, "little") + (len(data) ^ 0xFFFF).to_bytes(2, "little") + bytes(data))


def expand(tokens, history=b""):
    """the plain model: what `tokens` decode to behind `history` (returned in front of the new bytes)"""
    out = bytearray(history)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            length, distance = t
            assert 3 <= length <= 258 and 1 <= distance <= 32768 and distance <= len(out), t
            for _ in range(length):
                out.append(out[-distance])
    return bytes(out)


def coded(tokens, lit_lengths, dist_lengths):
    """the tokens whose symbols all have codes"""
    def ok(t):
        if isinstance(t, int):
            return lit_lengths[t] > 0
        return lit_lengths[len_symbol(t[0])[0]] > 0 and dist_lengths[dist_symbol(t[1])[0]] > 0
    return [t for t in tokens if ok(t)]


def bounded(tokens, have=0):
    """drops the matches that would reach in front of the output (`have` bytes exist already)"""
    out = []
    for t in tokens:
        if isinstance(t, int):
            have += 1
        elif t[1] <= have:
            have += t[0]
        else:
            continue
        out.append(t)
    return out


# ------------------------------------------------------------------------------------------------ containers
def zwrap(raw, body):
    """the raw DEFLATE `body` of `raw` as a zlib stream"""
    return b"\x78\x9c" + body + struct.pack(">I", zlib.adler32(raw) & 0xFFFFFFFF)


def gzwrap(raw, body):
    """... as a gzip member"""
    return b"\x1f\x8b\x08\0\0\0\0\0\0\x03" + body + struct.pack("<II", zlib.crc32(raw) & 0xFFFFFFFF, len(raw))


# ------------------------------------------------------------------------------------------------ the cases
def _finish(bits, parts):
    return bits.getvalue(), b"".join(parts)


# ---- A: both codes at depth 15
A_LITS = [ord(c) for c in "etaoin shrdl"]
A_LIT = sparse(286, dict(zip(A_LITS + [257, 256, 270, 285], list(range(1, 15)) + [15, 15])))
A_DIST = sparse(30, dict(zip(list(range(0, 29, 2)) + [29], list(range(1, 15)) + [15, 15])))
A_MATCHES = [(3, d) for d in [1, 2, 3] + [(1 << k) + 1 for k in range(2, 15)] + [24577, 32768]] + [(258, 1), (258, 32768), (35, 7), (4, 4)]


def a_tokens(rng, n_lit, n_match, matches_first=False):
    lits = rng.choices(A_LITS, k=n_lit)
    mixed = []
    for _ in range(n_match):
        mixed += [rng.choice(A_MATCHES), rng.choice(A_LITS)]
    return coded(mixed + lits if matches_first else lits + mixed, A_LIT, A_DIST)


def build_A(n_lit=40000, n_match=3000):
    rng = random.Random(0xA)
    tokens = bounded(a_tokens(rng, n_lit, n_match))
    bits = BitWriter()
    dyn_block(bits, A_LIT, A_DIST, tokens, True)
    return bits.getvalue(), expand(tokens)


# ---- B: an incomplete literal/length code (five of sixteen 4-bit codes unassigned), an empty distance code
B_LIT = sparse(257, dict((s, 4) for s in list(range(65, 75)) + [256]))


def b_block(bits, rng, n, final):
    tokens = rng.choices(range(65, 75), k=n)
    dyn_block(bits, B_LIT, [0], tokens, final, nd=1)
    return bytes(tokens)


def build_B(n=60000):
    rng = random.Random(0xB)
    bits = BitWriter()
    head = rng.choices(range(32, 127), k=50)
    fixed_block(bits, head, False)
    return _finish(bits, [bytes(head), b_block(bits, rng, n, True)])


# ---- C1 / E1: a distance code of one symbol, symbol 0: long self-overlapping runs at distance 1
C1_SYMS = [120, 121, 256, 257, 258, 259, 260, 265, 284, 285]
C1_LIT = sparse(286, dict(zip(C1_SYMS, flat_lengths(len(C1_SYMS)))))
C1_POOL = [(3, 1), (4, 1), (5, 1), (6, 1), (11, 1), (227, 1), (258, 1), 120, 121]


def c1_tokens(n):
    rng = random.Random(0xC1)
    return bounded([120] + rng.choices(C1_POOL, k=n - 1))


def build_C1(n=20000):
    tokens = c1_tokens(n)
    bits = BitWriter()
    dyn_block(bits, C1_LIT, [1], tokens, True)
    return bits.getvalue(), expand(tokens)


def build_E1(n=20000):
    tokens = c1_tokens(n)
    bits = BitWriter()
    dyn_block(bits, C1_LIT, [1], tokens, True, use_repeat_codes=False, len258_as_284=True)
    return bits.getvalue(), expand(tokens)


# ---- C2: a distance code of one symbol, symbol 29 (HDIST = 29)
C2_SYMS = list(range(48, 56)) + [256, 257, 260, 285]
C2_LIT = sparse(286, dict(zip(C2_SYMS, flat_lengths(len(C2_SYMS)))))


def build_C2(n_lit=33000, n=5000):
    rng = random.Random(0xC2)
    tokens = rng.choices(range(48, 56), k=n_lit) + rng.choices([(3, 32768), (258, 32768), (6, 24577), 50], k=n)
    bits = BitWriter()
    dyn_block(bits, C2_LIT, sparse(30, {29: 1}), tokens, True)
    return bits.getvalue(), expand(tokens)


# ---- D: HLIT = 31: the fixed code's 288 lengths as a dynamic header, thirty 5-bit distance codes
def build_D(n=50000):
    rng = random.Random(0xD)
    tokens = list(rng.randbytes(n))
    bits = BitWriter()
    dyn_block(bits, FIXED_LIT, [5] * 30, tokens, True, nl=288, nd=30)
    return bits.getvalue(), bytes(tokens)


# ---- E2: HLIT = 0; a zero run that starts right behind the last literal/length width, or spans the boundary
E2_LIT = sparse(257, dict([(s, 4) for s in range(8)] + [(s, 5) for s in range(248, 256)] + [(256, 2)]))
E2_DIST = [0] * 20 + [1, 1]
E2_CL = sparse(19, {0: 1, 4: 2, 5: 3, 2: 4, 1: 5, 16: 6, 17: 7, 18: 7})        # symbol 18: 7 + 7 bits, the widest header step


def e2_tokens(n):
    rng = random.Random(0xE2)
    return rng.choices(list(range(8)) + list(range(248, 256)), k=n)      # (HLIT = 0: no length symbol, the distance code idles)


def build_E2(n=12000, nl=257):
    tokens = e2_tokens(n)
    bits = BitWriter()
    symbols = rle(E2_LIT + [0] * (nl - 257) + E2_DIST)
    zero_runs = [s for s in symbols if s[0] == 18]
    assert zero_runs[-1] == (18, nl - 257 + 20 - 11)        # one run: the zeros on both sides of the boundary
    dyn_block(bits, E2_LIT, E2_DIST, tokens, True, nl=nl, header_symbols=symbols)
    return bits.getvalue(), expand(tokens)


# ---- E3: a symbol-16 repeat whose previous length is the last literal/length width, its copies the first distance widths
E3_LIT = sparse(258, dict((s, 4) for s in list(range(14)) + [256, 257]))
E3_DIST = [4] * 16


def build_E3(n=12000):
    rng = random.Random(0xE3)
    tokens = rng.choices(range(14), k=3000) + rng.choices(list(range(14)) + [(3, d) for d in (1, 2, 4, 6, 12, 24, 48, 96, 192, 255)], k=n - 3000)
    symbols = rle(E3_LIT) + [(16, 3), (16, 3), (16, 1)]      # 6 + 6 + 4 copies of the width of symbol 257
    assert rle(E3_LIT)[-1] == (4, 0)
    bits = BitWriter()
    dyn_block(bits, E3_LIT, E3_DIST, tokens, True, header_symbols=symbols)
    return bits.getvalue(), expand(tokens)


# ---- E4: code-length code extremes
def build_E4_hclen5(n=6000):
    """Four fields (16, 17, 18, 0) can only spell lengths of 0, and a block needs a code for 256: five fields (… and 8) are the
    fewest a valid block can have."""
    rng = random.Random(0xE4)
    tokens = list(rng.choices(range(255), k=n))
    bits = BitWriter()
    dyn_block(bits, sparse(257, dict((s, 8) for s in list(range(255)) + [256])), [0], tokens, True,
              cl_lengths=sparse(19, {0: 2, 8: 2, 18: 2, 17: 3, 16: 3}), hclen=5)
    return bits.getvalue(), bytes(tokens)


def build_E4_hclen_field4(n=6000):
    """the HCLEN field = 4: eight fields (16, 17, 18, 0, 8, 7, 9, 6)"""
    rng = random.Random(0xE5)
    tokens = list(rng.choices(range(159), k=n))
    bits = BitWriter()
    dyn_block(bits, sparse(257, dict([(s, 6) for s in range(32)] + [(s, 8) for s in list(range(32, 159)) + [256]])), [0], tokens, True,
              cl_lengths=sparse(19, {0: 2, 8: 2, 18: 3, 17: 3, 16: 3, 6: 3}), hclen=8)
    return bits.getvalue(), bytes(tokens)


def build_E4_hclen19(n=12000):
    """nineteen fields, the last two (symbols 1 and 15) zero"""
    rng = random.Random(0xE6)
    syms = list(range(100, 120)) + [256, 257, 258]
    lit = sparse(259, dict(zip(syms, flat_lengths(len(syms)))))
    tokens = bounded(rng.choices(list(range(100, 120)) + [(3, 3), (4, 2), (4, 4)], k=n))
    cl = sparse(19, dict([(s, 4) for s in [0] + list(range(2, 13)) + [16, 17, 18]] + [(13, 5), (14, 5)]))
    bits = BitWriter()
    dyn_block(bits, lit, flat_lengths(4), tokens, True, cl_lengths=cl, hclen=19)
    return bits.getvalue(), expand(tokens)


def build_E4_wide_step(n=12000):
    tokens = e2_tokens(n)
    bits = BitWriter()
    dyn_block(bits, E2_LIT, E2_DIST, tokens, True, cl_lengths=E2_CL)
    return bits.getvalue(), expand(tokens)


# ---- G: hundreds of empty blocks in a row
def build_G(n_empty=300, n_lit=3000):
    rng = random.Random(0x6)
    bits = BitWriter()
    head = rng.choices(range(32, 127), k=100)
    fixed_block(bits, head, False)
    for i in range(n_empty):
        if i % 3 == 0:
            fixed_block(bits, [], False)
        elif i % 3 == 1:
            stored_block(bits, b"", False)
        else:
            dyn_block(bits, sparse(257, {0: 1, 256: 1}), [0], [], False)
    tail = rng.choices(range(64, 127), k=n_lit)
    dyn_block(bits, sparse(257, dict((s, 6) for s in list(range(64, 127)) + [256])), [0], tail, False)
    fixed_block(bits, [], True)
    return _finish(bits, [bytes(head), bytes(tail)])


# ---- H: a stored block's header at every bit phase
def build_H(phases=None):
    """phases (a list) receives the bit position mod 8 of every stored block's header"""
    rng = random.Random(0x8)
    bits = BitWriter()
    parts = []
    for phase in range(8):
        lits = [200 + phase] * phase + [65 + phase]             # `phase` 9-bit literals and one of 8 bits
        fixed_block(bits, lits, False)
        if phases is not None:
            phases.append(bits.bitpos() % 8)
        data = rng.randbytes(65535 if phase == 5 else 1000 + phase)
        stored_block(bits, data, False)
        parts += [bytes(lits), data]
    fixed_block(bits, [], True)
    return _finish(bits, parts)


# ---- M: crafted blocks inside another encoder's stream
@functools.lru_cache(maxsize=None)
def m_text():
    rng = random.Random(0x77)
    letters = "etaoinshrdlcumwfgypbvkjxqz"
    words = ["".join(rng.choices(letters, k=rng.randint(2, 10))) for _ in range(30000)]
    return (" ".join(rng.choices(words, k=820000)) + "\n").encode()


@functools.lru_cache(maxsize=None)
def build_M():
    text = m_text()
    cut = len(text) - 200 * KIB
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    head = co.compress(text[:cut]) + co.flush(zlib.Z_FULL_FLUSH)
    assert len(head) >= 3 * MIB // 2
    rng = random.Random(0x3)
    bits = BitWriter()
    a = a_tokens(rng, 40000, 3000, matches_first=True)          # its first (…, 32768) read the head's bytes
    assert (258, 32768) in a[:40] and (3, 32768) in a[:40]
    dyn_block(bits, A_LIT, A_DIST, a, False)
    plain = expand(a, history=text[:cut])
    b = b_block(bits, rng, 60000, False)
    stored_block(bits, b"", False)
    tail = zlib.compressobj(6, zlib.DEFLATED, -15)
    return head + bits.getvalue() + tail.compress(text[cut:]) + tail.flush(), plain + b + text[cut:]


# ---- N: the shapes above as ONE stream of unlike neighbours, stored blocks at four bit phases between them
N_PHASES = (1, 4, 6, 7)
E2_SYMBOLS = rle(E2_LIT + E2_DIST)
E3_SYMBOLS = rle(E3_LIT) + [(16, 3), (16, 3), (16, 1)]
N_WRITERS = {
    "A": lambda bits, t: dyn_block(bits, A_LIT, A_DIST, t, False),
    "C1": lambda bits, t: dyn_block(bits, C1_LIT, [1], t, False),
    "C2": lambda bits, t: dyn_block(bits, C2_LIT, sparse(30, {29: 1}), t, False),
    "D": lambda bits, t: dyn_block(bits, FIXED_LIT, [5] * 30, t, False, nl=288, nd=30),
    "E2": lambda bits, t: dyn_block(bits, E2_LIT, E2_DIST, t, False, nl=257, header_symbols=E2_SYMBOLS),
    "E3": lambda bits, t: dyn_block(bits, E3_LIT, E3_DIST, t, False, header_symbols=E3_SYMBOLS),
    "E4": lambda bits, t: dyn_block(bits, E2_LIT, E2_DIST, t, False, cl_lengths=E2_CL),
}


def n_c1_tokens(rng, groups):
    """forty short codes at distance 1, then a run of one to three matches of 258 bytes, `groups` times"""
    tokens = [120]
    for _ in range(groups):
        tokens += rng.choices([120, 121, (3, 1), (4, 1), (5, 1), (6, 1), (11, 1)], k=40) + [(258, 1)] * rng.randint(1, 3)
    return tokens


def build_N_chain(phases=None, kinds=None):
    """phases (a list) receives the bit position mod 8 of every stored block's header, kinds the blocks' names in order.  A
    block in front of a stored one gets up to seven more literals of a width that shifts its end to the wanted phase."""
    rng = random.Random(0x4E)
    bits = BitWriter()
    plain = bytearray()
    stored = iter(N_PHASES)

    def block(kind, tokens, filler=None):
        if filler is not None:            # a stored block follows: end this one at its phase
            want = next(stored)
            for k in range(8):
                probe = BitWriter()
                N_WRITERS[kind](probe, tokens + [filler] * k)
                if (bits.bitpos() + probe.bitpos()) % 8 == want:
                    break
            else:
                raise AssertionError((kind, want))
            tokens = tokens + [filler] * k
        N_WRITERS[kind](bits, tokens)
        plain.extend(expand(tokens, history=bytes(plain[-32768:]))[min(len(plain), 32768):])
        if kinds is not None:
            kinds.append(kind)
        if filler is not None:
            if phases is not None:
                phases.append(bits.bitpos() % 8)
            data = rng.randbytes(rng.randint(1000, 3000))
            stored_block(bits, data, False)
            plain.extend(data)
            if kinds is not None:
                kinds.append("stored")

    def a_first():
        return [(258, 32768), (3, 32768)] + a_tokens(rng, 25000, 3000, matches_first=True)

    block("D", list(rng.randbytes(20000)))
    block("C1", n_c1_tokens(rng, 420), filler=120)                       # (3 bits a literal)
    block("A", a_first(), filler=ord("e"))                               # its (…, 32768) read across the stored block (1 bit)
    plain.extend(b_block(bits, rng, 20000, False))
    if kinds is not None:
        kinds.append("B")
    block("C2", rng.choices(range(48, 56), k=20000) + rng.choices([(3, 32768), (258, 32768), (6, 24577), 50], k=1500), filler=48)
    block("E2", e2_tokens(20000))
    block("E3", rng.choices(range(14), k=3000) + rng.choices(list(range(14)) + [(3, d) for d in (1, 2, 4, 6, 12, 24, 48, 96, 192, 255)], k=17000))
    block("E4", e2_tokens(20000), filler=248)                            # (5 bits)
    block("A", a_first())
    block("A", a_first())
    fixed_block(bits, [], True)
    return bits.getvalue(), bytes(plain)


# ---- rejects: alone, and behind the block of B (≥ 8 KiB compressed)
def _front(bits, behind):
    if not behind:
        return b""
    return b_block(bits, random.Random(0xF), 20000, False)


def build_I1(behind=False):
    bits = BitWriter()
    _front(bits, behind)
    fixed_block(bits, list(b"0123456789"), False)
    fixed_block(bits, [97, Sym("L", 286, None)], True)
    return bits.getvalue(), None


def build_I2(behind=False):
    bits = BitWriter()
    _front(bits, behind)
    fixed_block(bits, [97, Sym("L", 257, None), Sym("D", 30, None)], True)
    return bits.getvalue(), None


def build_J(behind=False):
    bits = BitWriter()
    _front(bits, behind)
    fixed_block(bits, list(b"0123456789"), False)
    over = sparse(257, dict((s, 4) for s in list(range(65, 83)) + [256]))          # 19 codes of 4 bits
    dyn_block(bits, over, [0], [65, 66, 67] * 20, True)
    return bits.getvalue(), None


def build_K(behind=False):
    rng = random.Random(0xCC)
    bits = BitWriter()
    _front(bits, behind)
    dyn_block(bits, sparse(257, dict((s, 4) for s in range(65, 81))), [0], rng.choices(range(65, 81), k=2000), True, nl=257, write_eob=False)
    return bits.getvalue(), None


def build_L(behind=False):
    bits = BitWriter()
    _front(bits, behind)
    dyn_block(bits, B_LIT, [0], [65, 66, 67] * 20, True, nd=1, header_symbols=[(16, 0)] + rle(B_LIT + [0]))
    return bits.getvalue(), None


def valid_prefix(name):
    """the blocks of a reject in front of the block that holds its fault, closed by an empty final block: a valid stream"""
    bits = BitWriter()
    _front(bits, name.endswith("_behind"))
    if name.split("_")[0] in ("I1", "J"):
        fixed_block(bits, list(b"0123456789"), False)
    fixed_block(bits, [], True)
    return bits.getvalue()


def same_bits(a, b, nbits):
    """the first `nbits` bits of two streams are equal"""
    k, r = divmod(nbits, 8)
    return a[:k] == b[:k] and (r == 0 or (a[k] ^ b[k]) & ((1 << r) - 1) == 0)


def takes_windows(blocks, n, step, head=0):
    """Whether the stream decoder MUST decode a stream of `n` bytes in more than one window when its reader hands over `step`
    bytes a call, decided from the oracle's block list alone.  With E the byte at which the first block ends (`head`: the
    container header's bytes in front), an attempt is due once the input has grown by a quarter since the last one that
    found no complete block, and one read may lie on either side of it: the first window is decoded in front of the stream's
    end when 1.25 E + 2 step < n."""
    assert not blocks[0][3]
    e = head + (blocks[0][1] + 7) // 8
    return 1.25 * e + 2 * step < n


VALID_ZLIB_AGREES = ["A", "C1", "C2", "E1", "E2", "E2_span", "E3", "E4_hclen5", "E4_hclen_field4", "E4_hclen19", "E4_wide_step", "G", "H"]
VALID_ZLIB_REFUSES = ["B", "D"]
VALID_ORACLE_ONLY = ["M", "N_chain"]
SMALL = ["A_small", "B_small", "C1_small", "G_small"]
REJECT_PREFIX = {"I1": "The value 286 must not occur in compressed data", "I2": "Invalid huffman coded stream", "J": "Bit region conflict",
                 "K": "failed to fill whole buffer", "L": "No preceding value"}

CASES = [
    ("A", build_A), ("B", build_B), ("C1", build_C1), ("C2", build_C2), ("D", build_D), ("E1", build_E1),
    ("E2", build_E2), ("E2_span", functools.partial(build_E2, nl=270)), ("E3", build_E3),
    ("E4_hclen5", build_E4_hclen5), ("E4_hclen_field4", build_E4_hclen_field4), ("E4_hclen19", build_E4_hclen19),
    ("E4_wide_step", build_E4_wide_step), ("G", build_G), ("H", build_H), ("M", build_M), ("N_chain", build_N_chain),
    ("A_small", functools.partial(build_A, 300, 100)), ("B_small", functools.partial(build_B, 600)),
    ("C1_small", functools.partial(build_C1, 400)), ("G_small", functools.partial(build_G, 30, 300)),
]
for _name, _fn in (("I1", build_I1), ("I2", build_I2), ("J", build_J), ("K", build_K), ("L", build_L)):
    CASES += [(_name, _fn), (_name + "_behind", functools.partial(_fn, True))]

VALID = VALID_ZLIB_AGREES + VALID_ZLIB_REFUSES + VALID_ORACLE_ONLY + SMALL
REJECTS = [n for n, _ in CASES if n not in VALID]


@functools.lru_cache(maxsize=None)
def built():
    """{name: (raw DEFLATE, expected plain or None)}, every case built once"""
    return dict((name, fn()) for name, fn in CASES)
