"""LZ77 token streams for tests: legal sequences of literals and matches that no encoder at hand writes, and the rejects whose
first bad token is a match in front of the first byte.  The headers are deliberately ordinary: every dynamic block codes all
286 literal/length and all 30 distance symbols with a flat complete code (python-zlib accepts every valid case).  What is
under test is the materialisation: how a tile picks its codes, how chains of in-tile sources settle, the ring at distance
32768, where a block may be cut into units, and reads in front of a block or of the stream.  The model is
deflate_craft.expand.  A case is a list of blocks; CASES is what the CPU test (test_lz77_craft_streams.py) fixes against the
oracle and proves the coverage of, and what the GPU test (test_gpu_lz77_craft_decode.py) then decodes.

Shapes are chosen against the decoder's size thresholds: a stream under 4 KiB is decoded serially; a block of up to 256 Kbit
in a stream of at most four blocks is scanned in one piece and materialised by the 1024-lane instance; a larger block of such
a stream is scanned in pieces, which read each other through markers.  Hence the one-block cases stay under 256 Kbit (those
that cannot are two self-contained blocks), and the cases that need a larger self-contained block (W_*_lits, U_*_big) carry
four more blocks, which takes them to the scan with one workgroup per block and to the 256-lane instance."""
import functools
import random

from deflate_craft import KIB, BitWriter, dyn_block, expand, fixed_block, flat_lengths, stored_block

LIT = flat_lengths(286)
DIST = flat_lengths(30)
ONE_PIECE_BITS = 256 << 10
GEOMETRIES = ((512, 1024), (2048, 4096))          # (NC, TILE) of the 256- and the 1024-lane instance


# ------------------------------------------------------------------------------------------------ models
def code_lengths(tokens):
    """output bytes per code"""
    return [1 if isinstance(t, int) else t[0] for t in tokens]


def tile_walk(lengths, nc, tile):
    """the tiles of one unit: [(take, total)].  A tile looks at a window of `nc` codes and takes the largest prefix whose bytes
    are at most `tile`; the next window starts `take` further on."""
    out, i, n = [], 0, len(lengths)
    while i < n:
        take = total = 0
        for l in lengths[i:i + nc]:
            if not total + l <= tile:
                break
            total += l
            take += 1
        out.append((take, total))
        i += take
    return out


def tile_slacks(lengths, nc, tile):
    """for every tile that deferred a code of its window: the bytes it had left"""
    out, i = [], 0
    for take, total in tile_walk(lengths, nc, tile):
        if take < nc and i + take < len(lengths):
            out.append(tile - total)
        i += take
    return out


def sources(tokens, have=0):
    """[(position, source position, length)] of the matches; `have` bytes lie in front"""
    out, pos = [], have
    for t in tokens:
        if isinstance(t, int):
            pos += 1
        else:
            out.append((pos, pos - t[1], t[0]))
            pos += t[0]
    return out


def legal_cut_codes(tokens):
    """the code indices c > 0 in front of which a block may be cut: no later match reads a byte in front of that code"""
    starts, pos = [], 0
    for l in code_lengths(tokens):
        starts.append(pos)
        pos += l
    low, reach = pos, [0] * len(tokens)            # reach[c]: the smallest source position of the codes from c on
    for c in range(len(tokens) - 1, -1, -1):
        t = tokens[c]
        if not isinstance(t, int):
            low = min(low, starts[c] - t[1])
        reach[c] = low
    return [c for c in range(1, len(tokens)) if reach[c] >= starts[c]]


def chain_depth(tokens, first_code, take):
    """the deepest chain of sources that stay inside the tile of codes [first_code, first_code + take)"""
    depth = []
    for t in tokens[first_code:first_code + take]:
        if isinstance(t, int):
            depth.append(0)
        else:
            for _ in range(t[0]):
                src = len(depth) - t[1]
                depth.append(depth[src] + 1 if src >= 0 else 0)
    return max(depth) if depth else 0


def hops(blocks):
    """per output byte: how many matches lie between it and the literal it copies"""
    out = []
    for kind, tokens in blocks:
        for t in tokens:
            if isinstance(t, int):
                out.append(0)
            else:
                for _ in range(t[0]):
                    out.append(out[-t[1]] + 1)
    return out


# ------------------------------------------------------------------------------------------------ writing
def write(blocks):
    """[(kind, tokens or bytes)] → raw DEFLATE, the last block final; kind: "dyn", "fixed", "stored" """
    bits = BitWriter()
    for i, (kind, body) in enumerate(blocks):
        final = i + 1 == len(blocks)
        if kind == "dyn":
            dyn_block(bits, LIT, DIST, body, final)
        elif kind == "fixed":
            fixed_block(bits, body, final)
        else:
            stored_block(bits, bytes(body), final)
    return bits.getvalue()


def block_bits(blocks):
    """the size of every block in bits (a stored block's padding included)"""
    out, bits = [], BitWriter()
    for kind, body in blocks:
        at = bits.bitpos()
        if kind == "dyn":
            dyn_block(bits, LIT, DIST, body, False)
        elif kind == "fixed":
            fixed_block(bits, body, False)
        else:
            stored_block(bits, bytes(body), False)
        out.append(bits.bitpos() - at)
    return out


def all_tokens(blocks):
    out = []
    for kind, body in blocks:
        out += list(body)
    return out


def lits(rng, n):
    return list(rng.randbytes(n))


EMPTY_TAIL = [("fixed", [])] * 4          # four empty blocks: a stream of five blocks is scanned one workgroup per block


# ------------------------------------------------------------------------------------------------ T: tile geometry
T_ALL258_PROLOGUE = 2600


def T_all258():
    """Eight turns of 400 matches.  The distances are drawn at random from the four longest, then from one more each turn:
    the prologue's bytes live on in the output (turn by turn from 1 up, the first (258, 1) would leave one byte value for the
    whole rest, and any source would do), and the tokens differ in length (400 equal tokens are a bit pattern of period 21
    in which the scan's lanes, which start at arbitrary bits, never fall into step: the stream would be left to the serial
    walk)."""
    rng = random.Random(0x7A11)
    ds = [259, 258, 257, 129, 7, 3, 2, 1]
    tokens = lits(rng, T_ALL258_PROLOGUE)
    for turn in range(8):
        tokens += [(258, ds[max(turn, 3)])] + [(258, rng.choice(ds[:max(turn, 3) + 1])) for _ in range(399)]
    return [("dyn", tokens)]


def _exact(rng, tokens, nbytes, distance):
    """codes of exactly `nbytes` bytes: matches of 258, then the rest as one match or as one or two literals"""
    tokens += [(258, distance)] * (nbytes // 258)
    rest = nbytes % 258
    tokens += [(rest, distance)] if rest >= 3 else lits(rng, rest)


def T_sweep():
    """Tile s = 0 .. 257 of the wide geometry is four tiles of the narrow one.  The first of the four ends s bytes short of 1024
    with a match of 258 bytes waiting, the others are filled to the last byte: the wide tile ends s bytes short of 4096 with a
    match of 258 bytes waiting, which opens the next tile of both.  The third holds s % 32 literals, a few matches of 258
    and a short one.  Every slack 0 .. 257 for both geometries takes 258 tiles of about 4 KiB: all a case may hold."""
    rng = random.Random(0x75EE)
    tokens, have = [], 0
    for s in range(258):
        distance = 300 + s if have >= 600 else 1
        part = []
        if s == 0:
            part += lits(rng, 1)                                      # (the block's first byte; later tiles open with the match
            _exact(rng, part, 1024 - s - 1, distance)                 #  that the tile before had no room for)
        else:
            _exact(rng, part, 1024 - s - 258, distance)
        part.append((258, distance))                                  # waits: s < 258
        _exact(rng, part, 1024 - 258, distance)
        part += lits(rng, s % 32)
        _exact(rng, part, 1024 - s % 32 - (3 + s % 8), distance)
        part.append((3 + s % 8, distance))
        _exact(rng, part, 1024, distance)
        part.append((258, distance))                                  # waits
        tokens += part
        have += sum(code_lengths(part))
    return [("dyn", tokens)]


T_AVG8_PROLOGUE, T_AVG8_FAR = 2400, 2200          # FAR: more than the longest literal run, so no run can be cut off


def _fill(rng, tokens, ncodes, nbytes, far):
    """`ncodes` codes of `nbytes` bytes in a random order: literals, and matches that read at least `far` bytes back"""
    assert ncodes <= nbytes <= 258 * ncodes
    part, extra = [], nbytes - ncodes
    for _ in range(ncodes):
        take = min(extra, 257)
        if take == 1:
            take = 0            # (a code is 1 byte or 3 .. 258)
        part.append(1 + take)
        extra -= take
    if extra:                   # a single byte is left: a match that has room takes it
        k = next(i for i, l in enumerate(part) if 3 <= l < 258)
        part[k] += 1
        extra -= 1
    assert extra == 0 and sum(part) == nbytes
    rng.shuffle(part)
    for l in part:
        tokens.append(rng.randrange(256) if l == 1 else (l, far + rng.randrange(40)))


def _sync(tokens, nc, tile, far):
    """appends (258, far) until the last of them starts a tile of its own"""
    while True:
        tokens.append((258, far))
        if tile_walk(code_lengths(tokens), nc, tile)[-1] == (1, 258):
            return


def T_avg8():
    """per geometry, twice: a tile of exactly 8.0 bytes a code, a window of literals, a tile of the smallest mean above 8.0
    (one byte more), a window of literals"""
    rng = random.Random(0x7A08)
    tokens = lits(rng, T_AVG8_PROLOGUE)
    far = T_AVG8_FAR
    for nc, tile in GEOMETRIES:
        even = tile // 8                    # so many codes of 8 bytes on average fill a tile exactly
        for rep in range(2):
            _sync(tokens, nc, tile, far)                                       # a tile starts at this match of 258 bytes
            _fill(rng, tokens, even - 1, tile - 258, far)                   # take * 8 == total == TILE
            tokens += lits(rng, nc)                                         # a window of literals: take == NC
            tokens.append((258, far))
            _fill(rng, tokens, even - 2, tile - 7 - 258, far)               # take = even - 1, total = 8 take + 1 ...
            tokens.append((8, far))                                         # ... and the next code is one byte too long
            _fill(rng, tokens, 20, 7 + 20, far)
            tokens += lits(rng, nc)
    tokens.append((258, far))           # (the block's last code is a match: no literal tail that could be cut off)
    return [("dyn", tokens)]


# ------------------------------------------------------------------------------------------------ P: pointer chains
P_RUNS = [(3, 1), (4, 2), (5, 3), (8, 1), (8, 7)]


def P_short_runs():
    """a literal, then a run written as short overlapping matches: about 340 of them (a tile of 1024 bytes deep), and for
    (3, 1) and (8, 1) as many as hold a whole tile of 4096 bytes wherever it starts.  The last code reads the block's first
    byte, so the block cannot be cut into units."""
    rng = random.Random(0x9051)
    tokens = lits(rng, 300)
    for wide in (False, True):
        for length, distance in P_RUNS:
            if not wide or distance == 1:
                tokens += lits(rng, distance) + [(length, distance)] * (2 * 4096 // length + 20 if wide else 340)
    tokens.append((3, sum(code_lengths(tokens))))
    return [("dyn", tokens)]


P_PERIODS_SPLIT = 180


def _period_block(rng, ds, chains):
    tokens = []
    for d in ds:
        tokens += lits(rng, d) + [(258, d), (258, d)]
    for _ in range(chains):
        # a match whose first period is itself match output of the same tile
        tokens += lits(rng, 7) + [(258, 7), (258, 258), (258, 516), (100, 774), (258, 7), (258, 258)]
    return tokens


def P_all_periods():
    rng = random.Random(0x9A11)
    return [("dyn", _period_block(rng, range(1, P_PERIODS_SPLIT + 1), 6)), ("dyn", _period_block(rng, range(P_PERIODS_SPLIT + 1, 259), 6))]


def P_copy_of_copy():
    """(L, L) behind a token of L bytes copies exactly that token's output; a fresh literal now and then starts a new length"""
    rng = random.Random(0x9C0C)
    tokens = lits(rng, 2500)
    steps = 0
    while steps < 5000:
        length = 3 + rng.randrange(6)
        tokens += lits(rng, length)                      # (the seed of the chain; the first (L, L) copies these L bytes)
        run = 1 + rng.randrange(120)
        tokens += [(length, length)] * run
        steps += run
    return [("dyn", tokens)]


# ------------------------------------------------------------------------------------------------ W: window and ring
W_ONE_BLOCK_LITS = 16000


def _window_block(rng, distance_of, nlits):
    """The first 32768 bytes: `nlits` random literals, the rest copies of them from 4000 .. 12000 bytes back (32768 literals
    alone are more than 256 Kbit).  Then 72000 bytes of matches only, their lengths sweeping 3 .. 258, a literal or three
    now and then to shift the tile phase."""
    tokens, pos = lits(rng, nlits), nlits
    while pos < 32768:
        rest = 32768 - pos
        length = 258 if rest >= 261 or rest == 258 else rest if rest <= 258 else rest - 3
        tokens.append((length, 4000 + rng.randrange(8001)))
        pos += length
    made, i = 0, 0
    while made < 72000:
        length = 3 + i % 256
        tokens.append((length, distance_of(i)))
        made += length
        if i % 11 == 10:
            tokens += lits(rng, 1 + i % 3)
        i += 1
    return tokens


def _near_ring(seed):
    pick = random.Random(seed)
    return lambda i: 32768 - (pick.randrange(4097) if i % 16 else 4096 * (i // 16 % 2))


def W_32768():
    """one block under 256 Kbit: the 1024-lane instance, a ring of 32768 + 4096 bytes"""
    return [("dyn", _window_block(random.Random(0x3270), lambda i: 32768 - i % 3, W_ONE_BLOCK_LITS))]


def W_near_ring():
    """... its sources within one tile of 4096 bytes of the ring's seam"""
    return [("dyn", _window_block(random.Random(0x3271), _near_ring(0x3272), W_ONE_BLOCK_LITS))]


def W_32768_lits():
    """32768 literals in front: a block over 256 Kbit, and four empty blocks behind it: the 256-lane instance"""
    return [("dyn", _window_block(random.Random(0x3276), lambda i: 32768 - i % 3, 32768))] + EMPTY_TAIL


def W_near_ring_lits():
    return [("dyn", _window_block(random.Random(0x3277), _near_ring(0x3278), 32768))] + EMPTY_TAIL


# ------------------------------------------------------------------------------------------------ U: unit cuts
def _anchor_block(rng, prologue, region, shift, far):
    """Literals and, as the last code in front of output byte P = prologue + 3, a match that reads `far` bytes back: in front
    of its lane's slice, so that the lane offers the cut at P (and the cuts of the `far` bytes in front of it are illegal).
    Behind P every match's source starts exactly at P - shift."""
    tokens = lits(rng, prologue) + [(3, far)]
    p0 = pos = prologue + 3
    tokens += lits(rng, 4)
    pos += 4
    while pos - p0 < region:
        tokens += lits(rng, 3)
        pos += 3
        length = 3 if rng.randrange(4) else 4 + rng.randrange(7)
        tokens.append((length, pos - p0 + shift))
        pos += length
    return tokens


# (20000 bytes behind P, not 30000: a match of three bytes at these distances costs 27 bits, and the block has to stay under
#  256 Kbit to be one piece; the big twins, which are past that limit anyway, have 32000)
U_PROLOGUE, U_REGION = 1560, 20000
U_BIG_PROLOGUE, U_BIG_REGION = 125000, 32000


def _anchor(shift):
    return [("dyn", _anchor_block(random.Random(0x0A2C), U_PROLOGUE, U_REGION, shift, 100))]


def _anchor_big(shift):
    rng = random.Random(0x0B16)
    return [("dyn", _anchor_block(rng, U_BIG_PROLOGUE, U_BIG_REGION, shift, 400)) for _ in range(5)]


# ------------------------------------------------------------------------------------------------ X: reads across blocks
X_BLOCK = 96 * KIB


def _x_body(rng, tokens, size):
    made = sum(code_lengths(tokens))
    i = 0
    while made < size:
        if i % 7 == 6:
            k = 1 + i % 5
            tokens += lits(rng, k)
            made += k
        else:
            tokens.append((258, 32768))
            made += 258
        i += 1
    return tokens


def _x_first_token(kind):
    rng = random.Random(0x0F17)
    blocks = [(kind, _x_body(rng, lits(rng, 32768), X_BLOCK))]
    for _ in range(2):
        blocks.append((kind, _x_body(rng, [(258, 32768), (258, 1), (3, 32768)], X_BLOCK)))
    return blocks


def X_relay40():
    rng = random.Random(0x0E40)
    relay = [(258, 32768)] * 126 + [(130, 32768)] * 2
    assert sum(code_lengths(relay)) == 32768
    return [("dyn", lits(rng, 32768))] + [("dyn", list(relay)) for _ in range(40)]


def X_over_stored():
    rng = random.Random(0x0570)
    first = lits(rng, 9000)
    third, pos = [], 29000
    for i in range(400):
        length = 3 + i % 40
        lo = max(0, pos - 32768)
        third.append((length, pos - rng.randrange(lo, 9000 - length)))     # a source inside the first block
        pos += length
        if i % 5 == 4:
            third += lits(rng, 2)
            pos += 2
    return [("dyn", first), ("stored", rng.randbytes(20000)), ("dyn", third)]


# ------------------------------------------------------------------------------------------------ R / V: a match in front of the first byte
def _have_small(have):
    rng = random.Random(0x4A00 + have)
    tokens = lits(rng, min(have, 1500))
    rest = have - len(tokens)
    while rest:                           # (4095 literals would not fit 4 KiB: the rest of the bytes are valid matches)
        length = 258 if rest >= 261 or rest == 258 else rest if rest <= 258 else rest - 3
        tokens.append((length, 1500))
        rest -= length
    return [("dyn", tokens + [(3, have + 1)] + lits(rng, 10))]


def _edge(distance, second_block):
    rng = random.Random(0x4ED6)
    front, tail = lits(rng, 20000), lits(rng, 50)
    if second_block:
        return [("dyn", front), ("dyn", [(3, distance)] + tail)]
    return [("dyn", front + [(3, distance)] + tail)]


CASES = [
    ("T_all258", T_all258), ("T_sweep", T_sweep), ("T_avg8", T_avg8),
    ("P_short_runs", P_short_runs), ("P_all_periods", P_all_periods), ("P_copy_of_copy", P_copy_of_copy),
    ("W_32768", W_32768), ("W_near_ring", W_near_ring), ("W_32768_lits", W_32768_lits), ("W_near_ring_lits", W_near_ring_lits),
    ("U_anchor", functools.partial(_anchor, 0)), ("U_anchor_m1", functools.partial(_anchor, 1)),
    ("U_anchor_big", functools.partial(_anchor_big, 0)), ("U_anchor_big_m1", functools.partial(_anchor_big, 1)),
    ("X_first_token", functools.partial(_x_first_token, "dyn")), ("X_relay40", X_relay40), ("X_over_stored", X_over_stored),
    ("X_fixed", functools.partial(_x_first_token, "fixed")),
    ("V_first_block", functools.partial(_edge, 20000, False)), ("V_second_block", functools.partial(_edge, 20000, True)),
    ("R_first_block", functools.partial(_edge, 20001, False)), ("R_second_block", functools.partial(_edge, 20001, True)),
] + [("R_have%d_small" % h, functools.partial(_have_small, h)) for h in (0, 1, 257, 4095)]

REJECTS = [n for n, _ in CASES if n.startswith("R_")]
VALID = [n for n, _ in CASES if n not in REJECTS]
MARKER = [n for n in VALID if n.startswith("X_")]
DIRECT = [n for n in VALID if n not in MARKER]
TWINS = {"V_first_block": "R_first_block", "V_second_block": "R_second_block"}
REJECT_PREFIX = "Too long backword reference"


@functools.lru_cache(maxsize=None)
def blocks_of(name):
    return dict(CASES)[name]()


def model(blocks):
    """→ (expected bytes, or None for a reject; the bytes in front of the first bad token)"""
    out = b""
    for kind, body in blocks:
        if kind == "stored":
            out += bytes(body)
            continue
        pos, good = len(out), len(body)
        for k, t in enumerate(body):
            if isinstance(t, int):
                pos += 1
            elif t[1] > pos:
                good = k
                break
            else:
                pos += t[0]
        out = expand(body[:good], out)
        if good < len(body):
            return None, out
    return out, out


@functools.lru_cache(maxsize=None)
def built():
    """{name: (raw DEFLATE, expected bytes or None)}, every case built once"""
    return dict((name, (write(blocks_of(name)), model(blocks_of(name))[0])) for name, _ in CASES)


def valid_prefix(name):
    """the blocks of a reject in front of the block that holds its bad token, closed by an empty final block: a valid stream"""
    blocks = blocks_of(name)
    k = next(i for i in range(len(blocks)) if model(blocks[:i + 1])[0] is None)
    return write(blocks[:k] + [("fixed", [])])


def front_of(name):
    """the bytes in front of a reject's bad token"""
    return model(blocks_of(name))[1]
