"""Crafted symbol counts for the encoder's Huffman stage (libflate_amd/csrc/lfx_huff.h), shared by test_huff_cases.py (CPU: every
case is what it claims, and the one-lane build reproduces the oracle on it) and test_gpu_huff_crafted.py (GPU: the same cases
through the kernels that run the stage on 320 lanes).  No GPU and no library import here: numpy and fixed seeds only.

A case is (name, group, driver, make, claim).  make() builds the input; claim is a dict of the properties the case is in the
catalogue for — test_huff_cases.py checks every one of them with the oracle alone.  Three drivers:

  "bytes"  bytes through lz77_kind = 1 (NoCompressionLz77Encoder: every byte a literal).  A block's histogram is exactly its
           byte histogram and one EndOfBlock, the distance alphabet is the dist[0] dummy.  make() → dict(data, write_size,
           writes, opts).  The planner closes a chunk of such an encoder only with its block (it does not buffer: lfx_plan.h,
           buffers()), so a block is ONE chunk row however it is written.
  "parse"  bytes through the default parse with window_size = 1024: an LZ77 flush every 8192 buffered bytes, so a block is many
           chunk rows.  The block's histogram is that of the oracle's own code words, chunk by chunk (oracle.lz77_chunk).
  "codes"  a list of code words handed out by a caller's Lz77Encode, one final raw DEFLATE block: the length and distance
           alphabets and the header shapes.  make() → the list.  At most MAX_CODES words: they cross Python callbacks.

claim keys (all of block `block`, default 0): lit_n / dist_n (used symbols; dist_n = 0: the dummy), lit_clamp / dist_clamp /
clen_clamp (the unconstrained depth exceeds 15 / 15 / 7), tie_run (the longest run of equal weights at the head of the depth
queue is at least this long and holds unequal depths; tie_alpha "lit" or "dist"), pm_tie (package-merge meets a package and a
leaf of equal weight), pm_odd (a list of odd length loses its tail), big (a count of 2^23 or more), tied ({count: how many
symbols have exactly it}), nl / nd, blocks / chunks (of the plan), rows (chunks of block 0), zero_run / width_run (a run of
exactly that length in the header's width sequence).
"""
import bisect
import functools
from collections import namedtuple

import numpy as np

MAX_CODES = 20000
LENS = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
DISTS = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
         6145, 8193, 12289, 16385, 24577]

Case = namedtuple("Case", "name group driver make claim")


# ---- code words and histograms ----------------------------------------------------------------------------------------
def len_symbol(length):
    return 285 if length == 258 else 256 + bisect.bisect_right(LENS, length)


def dist_symbol(distance):
    return bisect.bisect_right(DISTS, distance) - 1


def hist_of_codes(codes):
    """code tuples (without the EndOfBlock) → the block's 320 counters, EndOfBlock included"""
    hist = np.zeros(320, np.int64)
    for c in codes:
        if c[0] == "Literal":
            hist[c[1]] += 1
        else:
            hist[len_symbol(c[1])] += 1
            hist[288 + dist_symbol(c[2])] += 1
    hist[256] += 1
    return hist


def codes_of_hist(hist, cap=MAX_CODES):
    """320 counters with hist[256] == 1 → a code list with exactly that histogram.  Realisable only if the length symbols count
    as many code words as the distance symbols: every pointer is one of each."""
    hist = [int(x) for x in hist]
    assert len(hist) == 320 and hist[256] == 1 and not any(hist[286:288]) and not any(hist[318:])
    lens = [LENS[s - 257] for s in range(257, 286) for _ in range(hist[s])]
    dists = [DISTS[d] for d in range(30) for _ in range(hist[288 + d])]
    assert len(lens) == len(dists), "sum of hist[257..285] != sum of hist[288..317]"
    codes = [("Literal", v) for v in range(256) for _ in range(hist[v])] + [("Pointer", l, d) for l, d in zip(lens, dists)]
    assert len(codes) <= cap
    return codes


def fib(k):
    v = [1, 1]
    while len(v) < k:
        v.append(v[-1] + v[-2])
    return v[:k]


def bytes_of_counts(counts, seed=0):
    """{byte: count} or a 256-list → bytes with exactly those counts, shuffled by `seed`"""
    if isinstance(counts, dict):
        full = np.zeros(256, np.int64)
        for k, v in counts.items():
            full[k] = v
        counts = full
    a = np.repeat(np.arange(256, dtype=np.uint8), np.asarray(counts, dtype=np.int64))
    np.random.RandomState(seed).shuffle(a)
    return a.tobytes()


def oracle_stream(oracle, ofmt, spec):
    """the oracle's stream (format ofmt) of a bytes / parse case: its writes one by one, None is Write::flush()"""
    data = spec["data"]
    if spec["writes"] is None:
        return oracle.encode(ofmt, data, write_size=spec["write_size"], **spec["opts"])
    e, at = oracle.Encoder(ofmt, **spec["opts"]), 0
    for w in spec["writes"]:
        if w is None:
            e.flush()
        else:
            e.write(data[at:at + w])
            at += w
    assert at == len(data)
    return e.finish()


# The whole alphabet in use AND the limit 15 in force — the largest shape of the build's scratch: every level of the package-merge
# over all the symbols.  `ones` symbols of count 1 make a balanced subtree of weight `ones`; a chain of k symbols on top of it,
# ones, 2 ones, 3 ones, 5 ones, ... (each the weight of everything below it or just under), adds a level per symbol.
FULL_CHAIN = (1, 2, 3, 5, 8, 13, 21, 34)


def full_clamped_bytes(seed):
    """{byte: count}: 248 bytes of count 1 (with EndOfBlock: 249 ones, eight levels) and eight bytes of 249 x 1, 2, 3, 5, 8, 13, 21, 34:
    257 used symbols, 21 912 bytes, unconstrained depth 16"""
    heavy = _scatter(8, seed)
    counts = {b: 1 for b in range(256)}
    counts.update(zip(heavy, [249 * f for f in FULL_CHAIN]))
    return counts


FULL_CLAMPED_LEN = 248 + 249 * sum(FULL_CHAIN)           # 21 912


def one_block(data):
    """bytes driver: one write_all, a block_size beyond the input → one final block, one chunk"""
    return dict(data=data, write_size=0, writes=None, opts=dict(lz77_kind=1, block_size=len(data) + 1))


# ---- the header generator of test_host_pipeline.test_block_headers_of_crafted_alphabets (moved here unchanged) ---------
@functools.lru_cache(maxsize=None)
def header_code_lists():
    """alphabets made to hit every branch of the run-length code (symbol.rs:486-540): zero runs of 1..2, 3..10, 11..138, 139,
    148, 149 and more, runs of equal widths of every length around the groups of six, a run that ends where the distance table
    starts, one-symbol and empty tables; then sixty seeded random mixtures"""
    rng = np.random.default_rng(23)
    cases = []

    # literal i used iff it lies in one of the ranges; every used literal once → long runs of one width
    def lits(ranges, rep=1):
        out = []
        for lo, hi in ranges:
            for v in range(lo, hi):
                out.extend([("Literal", v)] * rep)
        return out
    for gap in (1, 2, 3, 4, 10, 11, 12, 137, 138, 139, 140, 148, 149, 150, 200, 254):
        cases.append(lits([(0, 1), (gap + 1, min(gap + 3, 256))]))           # a zero run of `gap` between used literals
    for run in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 64, 65, 128, 255, 256):
        cases.append(lits([(0, run)]) + [("Literal", 0)] * 3)                 # `run` literals, equal widths for most
    cases.append(lits([(0, 256)]))                                            # 256 equal widths + EOB
    cases.append([])                                                          # the empty block: EOB only, dist[0] dummy
    cases.append([("Pointer", 258, 32768)] * 5 + [("Literal", 255)])
    cases.append([("Pointer", LENS[k], DISTS[k]) for k in range(29)] + [("Pointer", 3, DISTS[29])])   # every length / distance symbol once
    cases.append(lits([(0, 256)]) + [("Pointer", LENS[k], DISTS[k]) for k in range(29)] + [("Pointer", 3, DISTS[29])])
    cases.append(lits([(250, 256)]) + [("Pointer", 258, 1)])                  # widths up to symbol 285, one distance
    cases.append(lits([(250, 256)], rep=2) + [("Pointer", 258, 24577)] * 2)   # ... the last distance symbol: zero run of 29 in the distance table
    for trial in range(60):
        codes = []
        k = int(rng.integers(1, 6))
        for _ in range(k):
            lo = int(rng.integers(0, 256)); hi = min(256, lo + int(rng.integers(1, 80)))
            codes += lits([(lo, hi)], rep=int(rng.integers(1, 4)))
        for _ in range(int(rng.integers(0, 40))):
            codes.append(("Pointer", int(rng.choice(LENS)) if rng.random() < 0.7 else int(rng.integers(3, 259)),
                          int(rng.choice(DISTS)) if rng.random() < 0.7 else int(rng.integers(1, 32769))))
        rng.shuffle(codes)
        cases.append([tuple(c) for c in codes])
    return [[(c[0], int(c[1])) if c[0] == "Literal" else (c[0], int(c[1]), int(c[2])) for c in codes] for codes in cases]


# ---- the catalogue ------------------------------------------------------------------------------------------------------
def _lit_fib_counts(k, syms):
    """Fibonacci counts over k literal-alphabet symbols: EndOfBlock is the first 1, `syms` (k - 1 of them) take 1, 2, 3, 5, ..."""
    assert len(syms) == k - 1
    return dict(zip(syms, fib(k)[1:]))


def _scatter(k, seed, lo=0, hi=256):
    return sorted(int(x) for x in np.random.RandomState(seed).permutation(np.arange(lo, hi))[:k])


def _hist(lit=None, dist=None):
    h = np.zeros(320, np.int64)
    for k, v in (lit or {}).items():
        h[k] = v
    for k, v in (dist or {}).items():
        h[288 + k] = v
    h[256] = 1
    return h


def _group_a():
    out = [
        Case("a_lit_n1_empty_input", "a", "bytes", lambda: one_block(b""), dict(lit_n=1, dist_n=0, nl=257, nd=1, blocks=1, chunks=1)),
        Case("a_lit_n2_one_byte", "a", "bytes", lambda: one_block(b"a"), dict(lit_n=2, dist_n=0, nl=257, nd=1)),
        Case("a_lit_n257_all_equal", "a", "bytes", lambda: one_block(bytes_of_counts([1] * 256, 1)), dict(lit_n=257, dist_n=0, nl=257)),
        # 256 literals, EndOfBlock and every length symbol once; the 29 pointers share distance symbol 0
        Case("a_lit_n286_ones_dist_n1_sym0", "a", "codes",
             lambda: codes_of_hist(_hist({s: 1 for s in range(286)}, {0: 29})), dict(lit_n=286, dist_n=1, nl=286, nd=1)),
        Case("a_dist_n1_sym29", "a", "codes", lambda: codes_of_hist(_hist({65: 3, 257: 4}, {29: 4})), dict(dist_n=1, nd=30, lit_n=3)),
        Case("a_dist_n2", "a", "codes", lambda: codes_of_hist(_hist({65: 2, 258: 3, 285: 4}, {3: 2, 17: 5})), dict(dist_n=2, nd=18, nl=286)),
        Case("a_dist_n30", "a", "codes",
             lambda: codes_of_hist(_hist({257 + d % 29: 1 + (d == 0) for d in range(29)}, {d: 1 for d in range(30)})),
             dict(dist_n=30, nd=30, lit_n=30, nl=286)),
    ]
    return out


def _group_b():
    out = []
    for k in (17, 18, 20):
        for where, syms in (("low", list(range(k - 1))), ("high", list(range(256 - (k - 1), 256))), ("scatter", _scatter(k - 1, 40 + k))):
            out.append(Case("b_lit_fib%d_%s" % (k, where), "b", "bytes",
                            lambda k=k, syms=syms: one_block(bytes_of_counts(_lit_fib_counts(k, syms), k)),
                            dict(lit_clamp=True, lit_n=k, dist_n=0, pm_tie=True)))
    # through the length symbols: EndOfBlock 1, literal 7 1, then fifteen length symbols 2, 3, 5, ... 1597; one distance symbol
    lens17 = dict(zip(_scatter(15, 3, 257, 286), fib(17)[2:]))
    out.append(Case("b_lit_fib17_length_symbols", "b", "codes",
                    lambda: codes_of_hist(_hist({**lens17, 7: 1}, {5: sum(lens17.values())})),
                    dict(lit_clamp=True, lit_n=17, dist_n=1, dist_clamp=False)))
    lens18 = dict(zip(list(range(257, 273)), fib(18)[2:]))
    out.append(Case("b_lit_fib18_length_symbols_low", "b", "codes",
                    lambda: codes_of_hist(_hist({**lens18, 255: 1}, {0: sum(lens18.values())})),
                    dict(lit_clamp=True, lit_n=18, dist_n=1)))
    # the full alphabets, clamped (see full_clamped_bytes): all 257 symbols of a block of literals ...
    out.append(Case("b_lit_full257_clamped", "b", "bytes", lambda: one_block(bytes_of_counts(full_clamped_bytes(70), 70)),
                    dict(lit_clamp=True, lit_n=257, dist_n=0, nl=257, pm_tie=True)))
    # ... and all 286: 278 symbols of count 1 with EndOfBlock (every length symbol among them: 29 pointers on one distance symbol;
    # 279 ones are nine levels) and seven literals of 279 x 1, 2, 3, 5, 8, 13, 21 — 15 065 code words
    heavy286 = _scatter(7, 71)
    full286 = {s_: 1 for s_ in range(286)}
    full286.update(zip(heavy286, [279 * f for f in FULL_CHAIN[:7]]))
    out.append(Case("b_lit_full286_clamped", "b", "codes", lambda: codes_of_hist(_hist(full286, {0: 29})),
                    dict(lit_clamp=True, lit_n=286, dist_n=1, nl=286, nd=1)))
    return out


def _group_c():
    out = []
    for k, syms in ((17, list(range(17))), (18, list(range(12, 30))), (19, _scatter(19, 9, 0, 30)), (20, _scatter(20, 10, 0, 30))):
        d = dict(zip(syms, fib(k)))
        out.append(Case("c_dist_fib%d" % k, "c", "codes", lambda d=d: codes_of_hist(_hist({257: sum(d.values())}, d)),
                        dict(dist_clamp=True, dist_n=k, lit_clamp=False, lit_n=2)))
    # both alphabets clamp in one block.  Literal alphabet: Fibonacci over 18 symbols — EndOfBlock 1, fifteen literals 1, 2, ... 987,
    # two length symbols 1597 and 2584 (4181 pointers).  Distance alphabet: Fibonacci over 17 symbols with the largest one up
    # (1598), so that the sums agree
    f18, dd = fib(18), fib(17)
    dd[-1] += 1
    lit = dict(zip(_scatter(15, 4), f18[1:16]))
    lit.update({260: f18[16], 283: f18[17]})
    out.append(Case("c_both_clamp", "c", "codes", lambda: codes_of_hist(_hist(lit, dict(zip(_scatter(17, 6, 0, 30), dd)))),
                    dict(lit_clamp=True, dist_clamp=True, lit_n=18, dist_n=17)))
    return out


def _group_e():
    out = [
        Case("e_ones_64", "e", "bytes", lambda: one_block(bytes_of_counts({s: 1 for s in _scatter(63, 1)}, 2)),
             dict(lit_n=64, tie_run=4, tie_unequal=False)),
        Case("e_ones_200", "e", "bytes", lambda: one_block(bytes_of_counts({s: 1 for s in _scatter(199, 2)}, 3)),
             dict(lit_n=200, tie_run=4, tie_unequal=False)),
        # 1 (EndOfBlock), 1, 2, 4, ... 4096: at every level the new internal node ties with the next leaf
        Case("e_pow2_chain", "e", "bytes", lambda: one_block(bytes_of_counts(dict(zip(_scatter(13, 5), [1 << i for i in range(13)])), 4)),
             dict(lit_n=14, pm_tie=True, lit_clamp=False)),
        # k symbols each of 1, 2, 4, 8 (EndOfBlock is one of the ones)
        Case("e_groups_of_6", "e", "bytes",
             lambda: one_block(bytes_of_counts(dict(zip(_scatter(23, 6), [1] * 5 + [2] * 6 + [4] * 6 + [8] * 6)), 5)),
             dict(lit_n=24, tie_run=4, pm_tie=True)),
        Case("e_groups_of_11", "e", "bytes",
             lambda: one_block(bytes_of_counts(dict(zip(_scatter(43, 7), [1] * 10 + [2] * 11 + [4] * 11 + [8] * 11)), 6)),
             dict(lit_n=44, tie_run=4, pm_tie=True, pm_odd=True)),
        # 1, 1, 2, 2, 4, 4, ... 512, 512: two leaves and an internal node of one weight at every level
        Case("e_pairs_pow2", "e", "bytes",
             lambda: one_block(bytes_of_counts(dict(zip(_scatter(19, 8), [1] + [1 << (i // 2) for i in range(2, 20)])), 7)),
             dict(lit_n=20, pm_tie=True)),
        # the same through the distance alphabet: thirty distance symbols in groups of 1, 2, 4 — and ones in the literal one
        Case("e_dist_groups", "e", "codes",
             lambda: codes_of_hist(_hist({257 + i: 70 // 29 + (i < 70 % 29) for i in range(29)}, dict(zip(range(30), [1] * 10 + [2] * 10 + [4] * 10)))),
             dict(dist_n=30, tie_run=4, tie_alpha="dist", pm_tie=True)),
        # forty symbols each of 1, 2 and 4: a run of 35 equal weights with unequal depths walks the queue in LDS
        Case("e_groups_124_of_40", "e", "bytes",
             lambda: one_block(bytes_of_counts(dict(zip(_scatter(119, 10), [1] * 39 + [2] * 40 + [4] * 40)), 9)),
             dict(lit_n=120, tie_run=30, pm_tie=True)),
    ]
    # every list length 2 ... 9 (odd and even n): EndOfBlock 1 and n - 1 bytes of 1, 2, 2, 3, 4, 4, 5, 6
    small = [1, 2, 2, 3, 4, 4, 5, 6]
    for n in range(2, 10):
        out.append(Case("e_n%d" % n, "e", "bytes", lambda n=n: one_block(bytes_of_counts(dict(zip(_scatter(n - 1, 20 + n), small)), n)),
                        dict(lit_n=n, pm_odd=(n % 2 == 1 or None))))
    return out


def _big(counts_big, small):
    """two interleaved big symbols (or one) and a handful of small counts behind them"""
    parts = []
    syms = sorted(counts_big)
    if len(syms) == 2 and counts_big[syms[0]] == counts_big[syms[1]]:
        a = np.empty(2 * counts_big[syms[0]], np.uint8)
        a[0::2], a[1::2] = syms[0], syms[1]
        parts.append(a)
    else:
        parts += [np.full(counts_big[s], s, np.uint8) for s in syms]
    parts.append(np.frombuffer(bytes_of_counts(small, 1), np.uint8))
    return np.concatenate(parts).tobytes()


def _group_f():
    small = {3: 1, 9: 1, 200: 1, 17: 3, 18: 3, 250: 3, 40: 70000, 41: 70000}
    return [
        # two symbols of exactly 2^23: the pair compare decides their order by the symbol; 16 MiB + 140 KB in ONE block
        Case("f_two_equal_2p23", "f", "bytes", lambda: one_block(_big({97: 1 << 23, 98: 1 << 23}, small)),
             dict(big=True, lit_n=11, blocks=1, chunks=1, tied={1 << 23: 2, 70000: 2, 3: 3, 1: 4})),
        # one symbol of 2^23 - 1: the largest count of the one-key path
        Case("f_one_below_2p23", "f", "bytes", lambda: one_block(_big({97: (1 << 23) - 1}, small)), dict(big=False, lit_n=10, max_count=(1 << 23) - 1, tied={(1 << 23) - 1: 1, 70000: 2, 3: 3, 1: 4})),
    ]


def _lits(ranges, rep=1):
    return [("Literal", v) for lo, hi in ranges for v in range(lo, hi) for _ in range(rep)]


def _wrun(run):
    return _lits([(100, 100 + run)]) + [("Literal", 2 * i) for i in range(32 - run - 1)]


def _group_g():
    out = [Case("g_hdr_%03d" % i, "g", "codes", lambda i=i: header_code_lists()[i], dict()) for i in range(N_HEADER_LISTS)]
    every = [("Pointer", LENS[k], DISTS[k]) for k in range(29)] + [("Pointer", 3, DISTS[29])]
    out += [
        # (symbol 256 is always used: the longest zero run there is holds the 256 literals, 138 + 118 — 138 + 138 + 2 cannot occur)
        Case("g_zero_run_256", "g", "codes", lambda: [("Pointer", 4, 1)] * 3, dict(zero_run=256, nl=259, nd=1)),
        Case("g_zero_run_255", "g", "codes", lambda: [("Literal", 0)] * 2, dict(zero_run=255, nl=257, nd=1)),
        Case("g_zero_run_141", "g", "codes", lambda: _lits([(0, 1), (142, 144)]), dict(zero_run=141)),         # 138 + 3: an 18 and a 17
        Case("g_zero_run_3", "g", "codes", lambda: _lits([(0, 1), (4, 6)]), dict(zero_run=3)),
        Case("g_zero_run_in_dist_28", "g", "codes", lambda: [("Pointer", 3, 1), ("Pointer", 3, 24577)], dict(zero_run=28, nd=30)),
        # runs of one width of 1 + 6 k + 2 and 1 + 6 k + 3 entries: 32 symbols of count 1 (every width 5), `run` of them in a row
        Case("g_width_run_21", "g", "codes", lambda: _wrun(21), dict(width_run=21)),
        Case("g_width_run_27", "g", "codes", lambda: _wrun(27), dict(width_run=27)),
        Case("g_width_run_22", "g", "codes", lambda: _wrun(22), dict(width_run=22)),
        # a run that ends exactly at nl: the last symbols of the table share a width, the distance table starts a run of its own
        Case("g_run_ends_at_nl_257", "g", "codes", lambda: _lits([(249, 256)]), dict(nl=257, nd=1, width_run=8)),
        Case("g_run_ends_at_nl_286", "g", "codes",
             lambda: [("Literal", v) for v in (0, 2, 4, 6, 8)] + [("Pointer", LENS[k], 1) for k in range(19, 29)], dict(nl=286, nd=1, width_run=10)),
        Case("g_nl286_nd30", "g", "codes", lambda: every, dict(nl=286, nd=30)),
        Case("g_nl258_nd30", "g", "codes", lambda: _lits([(0, 256)]) + [("Pointer", 3, 24577)], dict(nl=258, nd=30)),
    ]
    return out


N_HEADER_LISTS = 104


# ---- group h: rows of unlike chunks (the default parse, window_size = 1024, 4096-byte writes: a chunk per 8192 bytes) ----
def _alpha(n, lo, hi, seed):
    return np.random.RandomState(seed).randint(lo, hi, size=n, dtype=np.uint8)


def _h_disjoint():
    # chunk 0: bytes 0..63, chunk 1: one distinct byte, chunk 2: 128..191, chunk 3: 192..255, chunk 4: one byte; the block closes
    # with that byte (block_size = 32769), the empty final block follows
    data = np.concatenate([_alpha(8192, 0, 64, 1), np.full(8192, 0x55, np.uint8), _alpha(8192, 128, 192, 2), _alpha(8192, 192, 256, 3),
                           np.array([0x41], np.uint8)]).tobytes()
    return dict(data=data, write_size=0, writes=[4096] * 8 + [1], opts=dict(window_size=1024, block_size=32769))


def _h_rows(n_chunks, seed):
    # n_chunks chunks of 8192 bytes in one block: random bytes, every third a nibble (some matches, all three alphabets in use)
    def make():
        n = 8192 * n_chunks
        a = _alpha(n, 0, 256, seed)
        a[::3] &= 0x0F
        return dict(data=a.tobytes(), write_size=4096, writes=None, opts=dict(window_size=1024, block_size=n + 1))
    return make


def _h_skewed():
    # Fibonacci counts over 22 bytes, shuffled: 46367 bytes, six chunks whose rows are mostly pointers — the literal, length and
    # distance alphabets are all skewed (the parse's matches keep the literal alphabet from clamping: asserted)
    data = bytes_of_counts(dict(zip(range(100, 122), fib(22))), 1)
    return dict(data=data, write_size=4096, writes=None, opts=dict(window_size=1024, block_size=len(data) + 1))


def _group_h():
    return [
        Case("h_disjoint_chunks", "h", "parse", _h_disjoint, dict(blocks=2, chunks=6, rows=5, disjoint_rows=True)),
        Case("h_rows_40", "h", "parse", _h_rows(40, 11), dict(blocks=1, chunks=40, rows=40)),
        Case("h_rows_6_skewed", "h", "parse", _h_skewed, dict(blocks=1, chunks=6, rows=6, lit_clamp=False)),
    ]


# ---- group i: 350 blocks of unlike shapes, one after the other ---------------------------------------------------------
I_BS = FULL_CLAMPED_LEN


def i_blocks():
    """the byte strings of the blocks, in order: the full alphabet with counts that clamp (21 912 bytes: closed by the block size;
    a clamped full alphabet does not fit a smaller block), nothing (EndOfBlock alone), one byte, two distinct bytes, the full
    alphabet with skewed counts, 256 equal counts, a short Fibonacci tail; fifty times over, with other symbols and another order
    of the bytes each time"""
    out = []
    for r in range(50):
        out.append(bytes_of_counts(full_clamped_bytes(500 + r), 100 + r))                      # n = 257, clamped: 21 912 bytes
        out.append(b"")                                      # n = 1
        out.append(bytes([r]))                               # n = 2
        out.append(bytes([r, 255 - r, r]))                   # n = 3, counts 2, 1, 1
        out.append(bytes_of_counts(1 + (np.random.RandomState(r).pareto(1.0, 256) * 2).astype(np.int64) % 300, r))   # n = 257, skewed
        out.append(bytes_of_counts([1] * 256, 200 + r))      # n = 257, all equal
        out.append(bytes_of_counts(dict(zip(_scatter(9, 300 + r), fib(10)[1:])), r))   # n = 10
    assert all(len(b) == I_BS for b in out[::7]) and all(len(b) < I_BS for i, b in enumerate(out) if i % 7)
    return out


def i_schedule():
    """→ (data, writes): every block of i_blocks() as one write; a 4096-byte write closes its block by the block size, every
    other block is closed by a flush (None) — an empty block by a flush alone"""
    blocks = i_blocks()
    writes = []
    for b in blocks:
        if len(b):
            writes.append(len(b))
        if len(b) != I_BS:
            writes.append(None)
    return b"".join(blocks), writes


def _group_i():
    def make():
        data, writes = i_schedule()
        return dict(data=data, write_size=0, writes=writes, opts=dict(lz77_kind=1, block_size=I_BS))
    return [Case("i_350_unlike_blocks", "i", "bytes", make, dict(blocks=351, chunks=351, lit_clamp=True, lit_n=257))]


# ---- group d: the code-length alphabet deeper than 7 --------------------------------------------------------------------
def header_entries(lit_widths, dist_widths):
    """build_bitwidth_codes (symbol.rs:486-540) restated: the code-length symbols (0..18) that the nl literal widths and the nd
    distance widths are written with, in order.  A run never crosses from the first table into the second."""
    out = []
    for tab in (list(lit_widths), list(dist_widths)):
        runs = []
        for i, w in enumerate(tab):
            if i > 0 and runs[-1][0] == w:
                runs[-1][1] += 1
            else:
                runs.append([int(w), 1])
        for v, c in runs:
            if v == 0:
                while c >= 11:
                    out.append(18)
                    c -= min(138, c)
                if c >= 3:
                    out.append(17)
                    c = 0
                out += [0] * c
            else:
                out.append(v)
                c -= 1
                while c >= 3:
                    out.append(16)
                    c -= min(6, c)
                out += [v] * c
    return out


def d_counts(seed, n_used, total):
    """byte counts for group d: n_used bytes at seeded places, counts that fall off like a Pareto tail, `total` bytes in all"""
    r = np.random.RandomState(seed)
    idx = r.permutation(256)[:n_used]
    c = (r.pareto(0.6, n_used) * 3).astype(np.int64) + 1
    c = np.maximum(1, c * total // c.sum())
    full = np.zeros(256, np.int64)
    full[idx] = c
    return full


# (seed, used bytes, bytes in all): found by a search over the seed with the oracle's widths and header_entries() — the counts
# of the code-length symbols these blocks' headers are written with make an unconstrained Huffman tree deeper than 7
D_SEEDS = ((11, 100, 4000), (12, 100, 4000))
D_CASES = [Case("d_clen_clamp_%d" % s, "d", "bytes", lambda s=s, n=n, t=t: one_block(bytes_of_counts(d_counts(s, n, t), s)), dict(clen_clamp=True))
           for s, n, t in D_SEEDS]


def catalogue():
    return _group_a() + _group_b() + _group_c() + D_CASES + _group_e() + _group_f() + _group_g() + _group_h() + _group_i()


CASES = catalogue()
NAMES = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
