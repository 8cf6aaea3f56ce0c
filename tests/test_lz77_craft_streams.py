"""No GPU: every crafted token stream of lz77_craft.CASES gets its verdict from the oracle here, before a GPU sees it
(test_gpu_lz77_craft_decode.py), and the cases are proven to hit the edges they are named for: by a model of the tile walk
(lz77_craft.tile_walk), by the sources and cut positions computed from the tokens, by the sizes that select the decode paths.
A valid case on which the oracle and the plain model `expand` disagree is a bug in the writer, not a finding."""
import itertools
import zlib

import pytest

import lz77_craft as lc
from deflate_craft import KIB, MIB, same_bits, takes_windows

OK, INVALID_DATA = 0, 1


@pytest.fixture(scope="module")
def verdicts(oracle):
    """{name: (z, expected, (status, output, consumed, message))}"""
    return dict((name, (z, want, oracle.decode(oracle.DEFLATE, z))) for name, (z, want) in lc.built().items())


def _dyn(name):
    """the token lists of a case's blocks that hold any"""
    return [body for kind, body in lc.blocks_of(name) if kind != "stored" and body]


def test_case_list_is_whole():
    names = [n for n, _ in lc.CASES]
    assert len(set(names)) == len(names)
    assert sorted(names) == sorted(lc.VALID + lc.REJECTS) and sorted(lc.VALID) == sorted(lc.DIRECT + lc.MARKER)
    assert sorted(lc.MARKER) == ["X_first_token", "X_fixed", "X_over_stored", "X_relay40"]
    assert sorted(lc.REJECTS) == sorted(["R_first_block", "R_second_block"] + ["R_have%d_small" % h for h in (0, 1, 257, 4095)])
    assert sorted(n[0] for n in lc.DIRECT) == sorted("TTT" + "PPP" + "WWWW" + "UUUU" + "VV")
    for name in names:                  # ordinary headers: every dynamic block codes every symbol with the flat code
        assert all(kind in ("dyn", "fixed", "stored") for kind, _ in lc.blocks_of(name))
    assert min(lc.LIT) == 8 and max(lc.LIT) == 9 and min(lc.DIST) == 4 and max(lc.DIST) == 5


@pytest.mark.parametrize("name", lc.VALID)
def test_valid_cases(verdicts, name):
    z, want, (rc, out, used, msg) = verdicts[name]
    assert want is not None
    assert rc == OK, msg
    assert out == want
    assert used == len(z)
    assert zlib.decompress(z, -15) == want


@pytest.mark.parametrize("name", lc.REJECTS)
def test_reject_cases(verdicts, name):
    z, want, (rc, out, used, msg) = verdicts[name]
    print(name, rc, len(out), used, msg)
    assert want is None
    assert rc == INVALID_DATA
    assert msg.startswith(lc.REJECT_PREFIX), msg
    assert out == lc.front_of(name)            # the model's bytes in front of the bad token
    with pytest.raises(zlib.error):
        zlib.decompress(z, -15)


@pytest.mark.parametrize("name", lc.REJECTS)
def test_reject_prefixes(oracle, verdicts, name):
    """valid_prefix(name) is the reject's own bits up to the block that holds the bad token, and the oracle delivers its bytes"""
    z, _want, (rc, out, used, msg) = verdicts[name]
    prefix = lc.valid_prefix(name)
    prc, pout, pused, _ = oracle.decode(oracle.DEFLATE, prefix)
    blocks = oracle.scan_blocks(prefix)
    assert prc == OK and pused == len(prefix) and blocks[-1][2:] == (1, 1, 0)
    assert same_bits(z, prefix, blocks[-1][0])
    assert out[:len(pout)] == pout and len(pout) == sum(b[4] for b in blocks)


STREAM_STEP = 997           # (test_gpu_craft_stream.py)


def test_cases_that_must_take_several_windows(oracle, verdicts):
    """the stream decoder's tests mean something only where a case cannot be decoded in one window (deflate_craft.takes_windows)"""
    for name in ("X_relay40", "X_over_stored", "U_anchor_big"):
        z = verdicts[name][0]
        assert takes_windows(oracle.scan_blocks(z), len(z), STREAM_STEP), name
    assert len(oracle.scan_blocks(verdicts["X_relay40"][0])) == 41 and len(oracle.scan_blocks(verdicts["U_anchor_big"][0])) == 5


def test_rejects_reach_one_byte_too_far():
    for have in (0, 1, 257, 4095):
        tokens = lc.all_tokens(lc.blocks_of("R_have%d_small" % have))
        bad = [(pos, src) for pos, src, length in lc.sources(tokens) if src < 0]
        assert bad[0] == (have, -1), have
    for name in ("R_first_block", "R_second_block"):
        tokens = lc.all_tokens(lc.blocks_of(name))
        assert [(pos, src) for pos, src, length in lc.sources(tokens)] == [(20000, -1)]
    assert lc.blocks_of("R_second_block")[1][1][0] == (3, 20001)          # the match opens the second block


@pytest.mark.parametrize("valid,reject", sorted(lc.TWINS.items()))
def test_twins_differ_in_one_distance(verdicts, valid, reject):
    v, r = lc.blocks_of(valid), lc.blocks_of(reject)
    assert [k for k, _ in v] == [k for k, _ in r]
    tv, tr = lc.all_tokens(v), lc.all_tokens(r)
    diff = [(a, b) for a, b in zip(tv, tr) if a != b]
    assert len(tv) == len(tr) and diff == [((3, 20000), (3, 20001))]
    assert verdicts[valid][1][:20000] == verdicts[reject][2][1]           # ... and the reject delivers the twin's bytes up to there


def test_sizes(verdicts):
    total = 0
    for name, (z, want, _) in verdicts.items():
        bits = lc.block_bits(lc.blocks_of(name))
        if name.endswith("_small"):
            assert len(z) < 4 * KIB, (name, len(z))           # the serial kernel
        else:
            assert len(z) >= 8 * KIB, (name, len(z))
        # every stream starts with the piece walk from its known first block
        assert len(z) < 3 * MIB // 2, name
        if name.endswith(("_big", "_big_m1")):
            # over 1 Mbit a block AND per block of the stream: the storing scan's condition; five blocks: past the piece walk
            assert len(bits) == 5 and min(bits) > 131072 * 8 and len(z) * 8 // len(bits) >= 1 << 20, (name, bits)
        if want is not None:
            total += len(want)
            # (X_relay40 is 41 windows of 32768 bytes by what it is: forty hops at distance 32768 take 40 * 32768 bytes)
            assert len(want) <= (41 * 32768 if name == "X_relay40" else MIB), (name, len(want))
    assert total <= 8 * MIB


def test_block_sizes_select_the_paths():
    """Read from the member decode: a stream under 1.5 MiB is walked block by block in pieces of 256 Kbit for up to four blocks; a
    block that ends in its first piece is an ordinary block (direct path; at most four blocks: the 1024-lane instance), one that
    takes more pieces goes through markers.  A stream of more blocks is scanned one workgroup per block, whatever their sizes."""
    for name in lc.DIRECT:
        bits = lc.block_bits(lc.blocks_of(name))
        assert len(bits) <= 4 and max(bits) < lc.ONE_PIECE_BITS or len(bits) >= 5, (name, bits)
    for name in ("T_all258", "T_sweep", "T_avg8", "P_short_runs", "P_all_periods", "P_copy_of_copy", "U_anchor", "U_anchor_m1",
                 "W_32768", "W_near_ring", "V_first_block"):
        bits = lc.block_bits(lc.blocks_of(name))
        assert len(bits) <= 4 and max(bits) < lc.ONE_PIECE_BITS, (name, bits)          # the wide instance
    for name in ("W_32768", "W_near_ring"):
        assert len(lc.blocks_of(name)) == 1
    for name in ("W_32768_lits", "W_near_ring_lits"):          # (32768 literals alone are more than 256 Kbit)
        bits = lc.block_bits(lc.blocks_of(name))
        assert bits[0] > lc.ONE_PIECE_BITS and bits[1:] == [10] * 4
    # the direct path needs blocks that read nothing in front of themselves
    for name in lc.DIRECT:
        if name != "V_second_block":
            for tokens in _dyn(name):
                assert min([src for pos, src, length in lc.sources(tokens)] + [0]) == 0, name
    # ... and the marker cases hold blocks that do
    for name in lc.MARKER:
        assert any(min([src for pos, src, length in lc.sources(tokens)] + [0]) < 0 for tokens in _dyn(name)[1:]), name


# ------------------------------------------------------------------------------------------------ coverage by the tile model
def _one_unit(tokens):
    """The tile walk of a block starts at its first code only if the block is ONE unit.  A block is cut at up to seven ideal
    places, multiples of n / 8 codes (n / k for fewer units), each taking a legal cut within n / (2 k) codes: no cut is looked
    for in front of code n / 16."""
    return all(c < len(tokens) // 16 for c in lc.legal_cut_codes(tokens))


def test_tile_model():
    assert lc.tile_walk([258] * 4, 512, 1024) == [(3, 774), (1, 258)]
    assert lc.tile_walk([1] * 1024 + [258], 512, 1024) == [(512, 512), (512, 512), (1, 258)]
    assert lc.tile_walk([256] * 4 + [1], 512, 1024) == [(4, 1024), (1, 1)]           # a tile may be filled to the last byte
    assert lc.tile_slacks([258] * 4, 512, 1024) == [250]
    assert lc.legal_cut_codes([1, 2, 3, (3, 1), 4, 5, (3, 2), 6]) == [1, 2, 4, 7]
    assert lc.chain_depth([7] + [(3, 1)] * 5, 0, 6) == 15 and lc.chain_depth([7] + [(3, 1)] * 5, 1, 5) == 14


@pytest.mark.parametrize("nc,tile", lc.GEOMETRIES)
def test_T_sweep_tile_ends_everywhere(nc, tile):
    totals, slacks = set(), set()
    for tokens in _dyn("T_sweep"):
        assert _one_unit(tokens)
        lengths = lc.code_lengths(tokens)
        totals |= set(total for take, total in lc.tile_walk(lengths, nc, tile))
        slacks |= set(lc.tile_slacks(lengths, nc, tile))
    assert tile in totals and tile - 1 in totals
    assert set(range(1, 258)) <= slacks, sorted(set(range(1, 258)) - slacks)


@pytest.mark.parametrize("nc,tile", lc.GEOMETRIES)
def test_T_all258_is_periodic(nc, tile):
    """every tile behind the prologue takes 3 (15) codes of its window and is of the PERIODIC instance; a unit cut can only
    fall into the prologue, and wherever a unit starts, a window of matches of 258 bytes gives the same tiles"""
    tokens, = _dyn("T_all258")
    assert all(c <= lc.T_ALL258_PROLOGUE for c in lc.legal_cut_codes(tokens))
    lengths = lc.code_lengths(tokens)
    seen, at = 0, 0
    for take, total in lc.tile_walk(lengths, nc, tile):
        if at >= lc.T_ALL258_PROLOGUE:
            assert take * 8 < total and take in (tile // 258, len(lengths) - at), (at, take, total)
            seen += 1
        at += take
    assert tile // 258 in (3, 15) and seen >= 3200 // (tile // 258)
    assert sorted(set(d for l, d in tokens[lc.T_ALL258_PROLOGUE:])) == [1, 2, 3, 7, 129, 257, 258, 259]
    out = lc.built()["T_all258"][1]          # the bytes stay varied up to the turn of distance 1: a wrong source shows
    assert sum(a != b for a, b in zip(out, out[1:])) > 2800 * 258 * 4 // 10
    for start in range(0, lc.T_ALL258_PROLOGUE, 97):          # a unit that starts anywhere in the prologue
        walk = lc.tile_walk(lengths[start:], nc, tile)
        assert all(take * 8 < total for take, total in walk[(lc.T_ALL258_PROLOGUE - start) // nc + 1:])


@pytest.mark.parametrize("nc,tile", lc.GEOMETRIES)
def test_T_avg8_switches_instance(nc, tile):
    tokens, = _dyn("T_avg8")
    assert _one_unit(tokens)
    walk = lc.tile_walk(lc.code_lengths(tokens), nc, tile)
    assert any(take * 8 == total and take < nc for take, total in walk)               # exactly 8.0: not periodic
    assert any(take * 8 + 1 == total for take, total in walk)                         # the smallest mean above 8.0: periodic
    assert any(take == nc for take, total in walk)                                    # a window of literals
    periodic = [take * 8 < total for take, total in walk]
    assert sum(a != b for a, b in zip(periodic, periodic[1:])) >= 4                   # consecutive tiles switch instance
    k = next(i for i, (take, total) in enumerate(walk) if take * 8 == total and take < nc)
    assert walk[k + 1][0] == nc and not periodic[k + 1]


@pytest.mark.parametrize("nc,tile", lc.GEOMETRIES)
def test_P_short_runs_chain_as_deep_as_the_tile(nc, tile):
    tokens, = _dyn("P_short_runs")
    assert _one_unit(tokens)
    deepest, at = 0, 0
    for take, total in lc.tile_walk(lc.code_lengths(tokens), nc, tile):
        if take * 8 >= total:            # the instance that does not fold a match onto its first period
            deepest = max(deepest, lc.chain_depth(tokens, at, take))
        at += take
    assert deepest >= tile - 8, deepest


def test_P_cases_hold_their_shapes():
    tokens = lc.all_tokens(lc.blocks_of("P_all_periods"))
    for d in range(1, 259):           # d fresh literals, then (258, d) twice
        assert any(tokens[k:k + 2] == [(258, d)] * 2 and k >= d and all(isinstance(t, int) for t in tokens[k - d:k])
                   for k in range(len(tokens) - 1)), d
    k = tokens.index((258, 516))
    assert tokens[k - 2:k + 2] == [(258, 7), (258, 258), (258, 516), (100, 774)]
    tokens, = _dyn("P_copy_of_copy")
    copies = [i for i, t in enumerate(tokens) if not isinstance(t, int) and i and not isinstance(tokens[i - 1], int)]
    assert len(copies) >= 3000
    assert all(tokens[i] == tokens[i - 1] and tokens[i][0] == tokens[i][1] and 3 <= tokens[i][0] <= 8 for i in copies)


@pytest.mark.parametrize("name", ["W_32768", "W_near_ring", "W_32768_lits", "W_near_ring_lits"])
def test_W_cases_stay_at_the_ring_seam(name):
    tokens = _dyn(name)[0]
    lengths = lc.code_lengths(tokens)
    starts = [0] + list(itertools.accumulate(lengths))
    k = starts.index(32768)                                                         # the first code behind byte 32768
    assert sum(lengths[:k]) == 32768
    nlits = 32768 if name.endswith("_lits") else lc.W_ONE_BLOCK_LITS
    assert all(isinstance(t, int) for t in tokens[:nlits]) and sum(isinstance(t, int) for t in tokens[:k]) == nlits
    assert all(4000 <= d <= 12000 for l, d in tokens[nlits:k])
    out = lc.built()[name][1]
    assert len(set(out[:32768])) == 256 and sum(a != b for a, b in zip(out, out[1:])) > len(out) * 9 // 10      # varied bytes
    matches = [t for t in tokens[k:] if not isinstance(t, int)]
    assert sum(l for l, d in matches) >= 70000
    assert set(l for l, d in matches) == set(range(3, 259))
    ds = set(d for l, d in matches)
    if name.startswith("W_32768"):
        assert ds == {32766, 32767, 32768}
    else:           # within one tile of the wide instance (4096 bytes) of the seam, both ends included
        assert min(ds) == 32768 - 4096 and max(ds) == 32768 and len(ds) > 400
    assert sum(isinstance(t, int) for t in tokens[k:]) > 30            # literals shift the tile phase


# ------------------------------------------------------------------------------------------------ other coverage
@pytest.mark.parametrize("name,shift", [("U_anchor", 0), ("U_anchor_m1", 1), ("U_anchor_big", 0), ("U_anchor_big_m1", 1)])
def test_U_anchor_sources(name, shift):
    prologue, region = (lc.U_BIG_PROLOGUE, lc.U_BIG_REGION) if "big" in name else (lc.U_PROLOGUE, lc.U_REGION)
    p = prologue + 3
    for tokens in _dyn(name):
        behind = [(pos, src) for pos, src, length in lc.sources(tokens) if pos >= p]
        assert len(behind) > region // 8 and set(src for pos, src in behind) == {p - shift}
        assert sum(lc.code_lengths(tokens)) - p >= region
        # in front of P: literals, and one match that ends at P and reads in front of its lane's slice
        assert [(pos, length) for pos, src, length in lc.sources(tokens) if pos < p] == [(p - 3, 3)]
        # the cuts: at P in the first twin only, never behind it
        k = tokens.index(next(t for t in tokens if not isinstance(t, int))) + 1          # the code at P
        cuts = lc.legal_cut_codes(tokens)
        assert (k in cuts) == (shift == 0) and max(cuts) <= k and k - 1 not in cuts
        # P lies just in front of one of the ideal boundaries b n / 8, within the search's reach of n / 16 codes
        n = len(tokens)
        assert any(0 <= b * n // 8 - k <= n // 16 for b in range(1, 8)), (k, n)


def test_X_relay40_hops():
    blocks = lc.blocks_of("X_relay40")
    assert len(blocks) == 41 and all(isinstance(t, int) for t in blocks[0][1]) and len(blocks[0][1]) == 32768
    for kind, tokens in blocks[1:]:
        assert sum(lc.code_lengths(tokens)) == 32768 and all(not isinstance(t, int) and t[1] == 32768 for t in tokens)
    h = lc.hops(blocks)
    assert set(h[-32768:]) == {40}


def test_X_cases_hold_their_shapes():
    for name in ("X_first_token", "X_fixed"):
        blocks = lc.blocks_of(name)
        assert [k for k, _ in blocks] == ["dyn" if name == "X_first_token" else "fixed"] * 3
        for kind, tokens in blocks:
            assert sum(lc.code_lengths(tokens)) >= 96 * KIB
        for kind, tokens in blocks[1:]:
            assert tokens[:3] == [(258, 32768), (258, 1), (3, 32768)]
            assert sum(l for l in lc.code_lengths(tokens) if l == 258) * 10 >= 9 * sum(lc.code_lengths(tokens))
    assert lc.all_tokens(lc.blocks_of("X_first_token")) == lc.all_tokens(lc.blocks_of("X_fixed"))
    (k1, first), (k2, data), (k3, third) = lc.blocks_of("X_over_stored")
    assert (k1, k2, k3) == ("dyn", "stored", "dyn") and len(data) == 20000
    srcs = [src for pos, src, length in lc.sources(third, len(first) + len(data))]
    assert len(srcs) >= 300 and all(0 <= s < len(first) for s in srcs)
