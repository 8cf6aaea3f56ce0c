"""The contract of CostLz77Encoder (include/lfx.h LFX_LZ77_COST) restated in plain Python, and the stream it
implies.  Test infrastructure: checked against level_model, a brute-force shortest path and python-zlib (test_cost_model.py),
never against the library.

Candidates: level_model's L(p), D(p) at the same level (depth, nice, too_far of its row; max_lazy is not used).

Widths: for every block (lw[286], dw[30]) — the fixed code's under dynamic_huffman = 0, otherwise the code of the FIRST PASS:
the greedy walk over the undemoted (L, D) of every buffer of the block, the block's symbol counts with EndOfBlock, the oracle's
length-limited code (distance symbol 0 counted once when the block has no pointer, as the reference does).  A symbol without a
code costs one bit more than the longest code of its alphabet in that block; an alphabet without any code 9 (literal/length) or
5 (distance).

demote(b, L, D, lw, dw, start) → L': the buffer's positions [start, end) are cut on a grid of COST_SEG from `start`; for a
segment [a, bb) the recurrence starts at top = min(bb + COST_WARM, end) with cost 0 and runs backward,
    cost[p] = min(lit(p) + cost[p + 1], mat(p) + cost[min(p + L(p), top)])       the match term only where L(p) != 0,
a tie goes to the match, and L'(p) = 0 for the p in [a, bb) where the literal won.  Plain integers here; the kernel keeps the
costs modulo 2^16 and compares by the sign of the 16-bit difference, which is the same thing: all costs within max_length + 1
positions lie within 16 * 258 bits of each other (lfx_cost.h).  The walk is level_model's greedy one over (L', D).

COST_SEG = 4096 and COST_WARM = 512: the values the contract names.  demote's seg / warm arguments made the sweep of DESIGN.md
§27: on text a warm-up of 128 or more already gives the uncut chunk's bits at every segment length tried."""
import zlib

import chain_model
import level_model
from chain_model import LEVEL_BEST, MAX_LENGTH, MAX_WINDOW, replay  # noqa: F401  (replay: for the tests)
from dict_encode_model import usable_tail
from level_model import TABLE, NEVER

COST_SEG = 4096
COST_WARM = 512
COST_KIND = 6                 # lz77_kind & 0xFF of the library (never handed to the oracle); 5 names no kind
NONE_LIT, NONE_DIST = 9, 5


def len_symbol(length):
    """→ (symbol 257..285, extra bits) — Symbol::code / extra_lengh, symbol.rs:95-125"""
    if length <= 10:
        return 254 + length, 0
    if length == 258:
        return 285, 0
    l = length - 3
    e = l.bit_length() - 3
    return 261 + 4 * e + ((l >> e) & 3), e


def dist_symbol(distance):
    """→ (symbol 0..29, extra bits) — Symbol::distance, symbol.rs:126-154"""
    x = distance - 1
    if x < 4:
        return x, 0
    e = x.bit_length() - 2
    return 2 * e + 2 + ((x >> e) & 1), e


FIXED = (tuple(8 if s < 144 else 9 if s < 256 else 7 if s < 280 else 8 for s in range(286)), (5,) * 30)


def first_pass_widths(oracle, codes):
    """codes: every code word of a block's first pass, EndOfBlock not included → (lw, dw)"""
    lc, dc = [0] * 286, [0] * 30
    for c in codes:
        if c & 0xFFFF:
            lc[len_symbol(c >> 16)[0]] += 1
            dc[dist_symbol(c & 0xFFFF)[0]] += 1
        else:
            lc[c >> 16] += 1
    lc[256] += 1
    if not any(dc):
        dc[0] = 1                                         # symbol.rs:332-337
    return tuple(int(w) for w in oracle.huff_widths(lc, 15)), tuple(int(w) for w in oracle.huff_widths(dc, 15))


class Costs:
    """lit(byte), mat(L, D) under (lw, dw) with the absent-symbol rule"""

    def __init__(self, lw, dw):
        al = max(lw) + 1 if max(lw) else NONE_LIT
        ad = max(dw) + 1 if max(dw) else NONE_DIST
        self.lit = [lw[s] or al for s in range(256)]
        self.length = [0] * 259
        for L in range(3, 259):
            s, e = len_symbol(L)
            self.length[L] = (lw[s] or al) + e
        self.dsym = [(dw[s] or ad) + (0 if s < 4 else (s - 2) >> 1) for s in range(30)]

    def mat(self, L, D):
        return self.length[L] + self.dsym[dist_symbol(D)[0]]

    def code(self, c):
        return self.mat(c >> 16, c & 0xFFFF) if c & 0xFFFF else self.lit[c >> 16]


def demote(b, L, D, lw, dw, start=0, seg=COST_SEG, warm=COST_WARM):
    """→ L' as a list; seg / warm: the contract's constants (other values: the experiments of DESIGN.md §27 only)"""
    end = max(3, len(b)) - 3
    k = Costs(lw, dw)
    out = list(L)
    a = start
    while a < end:
        bb = min(a + seg, end)
        top = min(bb + warm, end)
        cost = [0] * (top - a + 1)                        # cost[q - a]
        for p in range(top - 1, a - 1, -1):
            c = k.lit[b[p]] + cost[p + 1 - a]
            literal = True
            if L[p]:
                m = k.mat(L[p], D[p]) + cost[min(p + L[p], top) - a]
                if m <= c:                                # a tie: the match
                    c, literal = m, False
            cost[p - a] = c
            if literal and p < bb:
                out[p] = 0
        a += seg
    return out


def cost_codes(buf, level, lw, dw, window=MAX_WINDOW, max_len=MAX_LENGTH):
    b = bytes(buf)
    L, D = level_model.level_lengths(b, level, window, max_len)
    return level_model._walk(b, demote(b, L, D, lw, dw), D, None)


def first_codes(buf, level, window=MAX_WINDOW, max_len=MAX_LENGTH):
    """the first pass: the greedy walk over the level's candidates, nothing demoted"""
    b = bytes(buf)
    L, D = level_model.level_lengths(b, level, window, max_len)
    return level_model._walk(b, L, D, None)


def _primed(T, buf, level, window, max_len):
    depth, lazy, nice, _max_lazy, too_far = TABLE[level]
    T, buf = usable_tail(T), bytes(buf)
    b = T + buf
    L, D = level_model._lengths(b, len(T), depth, nice, too_far if lazy else NEVER, window, max_len)
    return b, len(T), L, D


def total_bits(codes, lw, dw):
    k = Costs(lw, dw)
    return sum(k.code(int(c)) for c in codes)


def visited_bits(buf, codes, lw, dw):
    """the bits of the code words that begin in the visited range [0, end): what the rule minimises.  The tail's literals (at
    most three, default.rs:105-107) are outside it — a last match may reach over some of them, and the recurrence, which ends
    at `end` with cost 0, does not see that"""
    end, k, at, total = max(3, len(buf)) - 3, Costs(lw, dw), 0, 0
    for c in codes:
        if at >= end:
            break
        total += k.code(int(c))
        at += (c >> 16) if c & 0xFFFF else 1
    return total


def brute_force_bits(buf, level, lw, dw, window=MAX_WINDOW, max_len=MAX_LENGTH):
    """the cheapest path through the same choice set, FORWARD: dist[q] = the fewest bits that reach position q from 0, over the
    edges p → p + 1 (literal) and p → p + L(p) (the level's match) for p < end → the cheapest way to reach `end` or beyond"""
    b = bytes(buf)
    n, end = len(b), max(3, len(b)) - 3
    L, D = level_model.level_lengths(b, level, window, max_len)
    k = Costs(lw, dw)
    INF = 1 << 60
    dist = [INF] * (n + 1)
    dist[0] = 0
    for p in range(end):
        if dist[p] == INF:
            continue
        dist[p + 1] = min(dist[p + 1], dist[p] + k.lit[b[p]])
        if L[p]:
            dist[p + L[p]] = min(dist[p + L[p]], dist[p] + k.mat(L[p], D[p]))
    return min(dist[end:])


class CostLz77(chain_model.ChainLz77):
    """CostLz77Encoder as an Lz77Encode for the oracle's generic encoder: ChainLz77's buffering.  The oracle calls flush() at
    the end of a block and nowhere else, so a block's buffers are those between two flush() calls.
    widths None: the first pass — the greedy codes, and `found` collects every block's (lw, dw).
    widths a list: the final pass, block i under widths[i]; a tuple (lw, dw): every block under it (fixed codes).
    T: a chain dictionary, which primes the first buffer."""

    def __init__(self, level, window=MAX_WINDOW, max_len=MAX_LENGTH, header=None, T=None, widths=None, oracle=None):
        super().__init__(TABLE[level][0], window, max_len, LEVEL_BEST if header is None else header)
        self.lvl, self.T, self.widths, self.oracle = level, T, widths, oracle
        self.block, self.block_codes, self.found = 0, [], []

    def _chunk(self, sink):
        buf, self.buf = bytes(self.buf), bytearray()
        if self.T is not None:
            b, t, L, D = _primed(self.T, buf, self.lvl, self.window, self.max_len)
            self.T = None
        else:
            b, t = buf, 0
            L, D = level_model.level_lengths(b, self.lvl, self.window, self.max_len)
        if self.widths is None:
            codes = level_model._walk(b, L, D, None, start=t)
            self.block_codes += codes
        else:
            lw, dw = self.widths if isinstance(self.widths, tuple) else self.widths[self.block]
            codes = level_model._walk(b, demote(b, L, D, lw, dw, start=t), D, None, start=t)
        for c in codes:
            sink.append(("Pointer", c >> 16, c & 0xFFFF) if c & 0xFFFF else ("Literal", c >> 16))

    def encode(self, buf, sink):
        self.buf += buf
        if len(self.buf) >= self.window * 8:
            self._chunk(sink)

    def flush(self, sink):
        self._chunk(sink)
        if self.widths is None:
            self.found.append(first_pass_widths(self.oracle, self.block_codes))
            self.block_codes = []
        self.block += 1


def _stream(oracle, fmt, data, level, write_size, window_size, max_length, header, writes, T, opts):
    window, max_len = min(window_size, MAX_WINDOW), min(max_length, MAX_LENGTH)
    widths = FIXED
    opts = dict(opts)
    # cost_first_pass (not an option of the oracle's): the first pass' widths although this encode writes fixed codes — the `= 0`
    # stream LFX_HUFFMAN_AUTO's model splices from holds the code words of the call, which were chosen under the dynamic code
    forced = opts.pop("cost_first_pass", False)
    if (forced or opts.get("dynamic_huffman", 1) != 0) and not opts.get("no_compression"):
        first = CostLz77(level, window, max_len, header, T, None, oracle)
        level_model._events(oracle, fmt, first, data, write_size, writes, dict(opts, dynamic_huffman=1))
        widths = first.found
    enc = CostLz77(level, window, max_len, header, T, widths, oracle)
    return level_model._events(oracle, fmt, enc, data, write_size, writes, opts)


def expected_stream(oracle, fmt, data, level, write_size=0, window_size=MAX_WINDOW, max_length=MAX_LENGTH, header=None, writes=None,
                    **opts):
    """fmt: the oracle's format number → the bytes the library must write for `data` with LFX_LZ77_COST_N(level): the oracle's
    generic encoder over the model's code words, twice under dynamic codes (the first pass yields every block's widths).
    header: a caller's lz77_level - 1 (None: Best).  writes: an explicit schedule (sizes, None is Write::flush()).  opts: the
    oracle's other options (block_size, dynamic_huffman, no_compression, mtime ...)."""
    return _stream(oracle, fmt, bytes(data), level, write_size, window_size, max_length, header, writes, None, opts)


def expected_dict_stream(oracle, fmt, zdict, data, level, write_size=0, window_size=MAX_WINDOW, max_length=MAX_LENGTH, writes=None, **opts):
    """fmt: "zlib" or "deflate" → the bytes lfx_encode_dict_* must write behind the chain dictionary `zdict` (the container as
    in level_model.expected_dict_stream)"""
    run = lambda f: _stream(oracle, f, bytes(data), level, write_size, window_size, max_length, None, writes, bytes(zdict), opts)
    if fmt == "deflate":
        return run(oracle.DEFLATE)
    z = run(oracle.ZLIB)
    cmf, flg = z[0], (z[1] & 0xC0) | 0x20                                  # FDICT
    if ((cmf << 8) + flg) % 31:
        flg += 31 - ((cmf << 8) + flg) % 31                                # FCHECK
    return bytes([cmf, flg]) + zlib.adler32(bytes(zdict)).to_bytes(4, "big") + z[2:]
