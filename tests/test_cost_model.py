"""CPU: tests/cost_model.py — the contract of CostLz77Encoder (LFX_LZ77_COST, include/lfx.h) — against a
brute-force shortest path over the same choice set, against level_model (the lazy path is a path of the same graph, so under one
fixed code the cost parse can never be larger), and python-zlib.  The library is not involved."""
import zlib

import pytest

import cost_model as km
import level_model as vm
from test_dict_encode_model import _text
from test_level_model import MIXED, far_case, lazy_case, put

SEG, WARM = km.COST_SEG, km.COST_WARM
LW, DW = km.FIXED
TEXT = _text(3 * SEG, 27)
BUFS = [MIXED[:3000], TEXT[:SEG + 3], TEXT[:SEG + 2], b"a" * 700 + TEXT[:300] + b"a" * 259, put(*lazy_case(15, 22))[0], put(*far_case(1000, 3))[0],
        b"", b"abc", b"abcabcabc", b"a" * 516 + TEXT[:100]]


def bits(codes, lw=LW, dw=DW):
    """of the code words of the visited range (cost_model.visited_bits says why the tail is outside the rule)"""
    return km.visited_bits(km.replay(codes), codes, lw, dw)


@pytest.mark.parametrize("level", [1, 6, 9])
def test_fixed_codes_one_segment_is_the_shortest_path_and_never_above_the_level(level):
    for buf in BUFS:
        for max_len in (258, 16, 3):
            assert max(3, len(buf)) - 3 <= SEG
            codes = km.cost_codes(buf, level, LW, DW, max_len=max_len)
            assert km.replay(codes) == buf
            got = bits(codes)
            assert got == km.brute_force_bits(buf, level, LW, DW, max_len=max_len), (len(buf), max_len)
            assert got <= bits(vm.level_codes(buf, level, max_len=max_len))
            assert got <= bits(km.first_codes(buf, level, max_len=max_len))
            assert all((c >> 16) <= max_len for c in codes if c & 0xFFFF)
    long = km.cost_codes(BUFS[-1], level, LW, DW)                              # a literal and a run of 515 behind it: 258 + 257
    assert [c >> 16 for c in long[:3]] == [ord("a"), 258, 257] and long[1] & 0xFFFF == 1 and long[2] & 0xFFFF == 1
    assert {c >> 16 for c in km.cost_codes(BUFS[3], level, LW, DW) if c & 0xFFFF} >= {258}
    assert bits(km.cost_codes(MIXED[:3000], 6, LW, DW)) < bits(vm.level_codes(MIXED[:3000], 6))      # and on text it is smaller


def _widths(lit=8, length=7, dist=5):
    return tuple([lit] * 256 + [length] * 30), tuple([dist] * 30)


def test_the_tie_goes_to_the_match():
    b = b"a" * 8                                                               # end = 5
    L, D = [0, 3, 0, 0, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0, 0, 0, 0]
    lw, dw = _widths(lit=4, length=7, dist=5)                                 # 3 literals = 12 = the match
    assert km.demote(b, L, D, lw, dw)[1] == 3
    lw, dw = _widths(lit=4, length=8, dist=5)                                 # 13 against 12
    assert km.demote(b, L, D, lw, dw)[1] == 0


def test_a_symbol_without_a_code():
    lw, dw = list(_widths(lit=0, length=0, dist=0)[0]), [0] * 30
    k = km.Costs(lw, dw)
    assert k.lit[65] == 9 and k.mat(3, 1) == 9 + 5 and k.mat(257, 32768) == 9 + 5 + 5 + 13        # no code at all: 9 and 5
    lw[65], lw[256], lw[257], dw[3] = 2, 11, 4, 6
    k = km.Costs(lw, dw)
    assert k.lit[65] == 2 and k.lit[66] == 12 and k.mat(3, 4) == 4 + 6 and k.mat(4, 5) == 12 + 7 + 1   # one more than the longest code
    # the first pass of a block without a pointer: distance symbol 0 is counted once, so it has a code and the others cost 2
    from oracle import lfo_oracle as oracle
    lw, dw = km.first_pass_widths(oracle, [c << 16 for c in b"hello world"])
    assert dw[0] == 1 and not any(dw[1:]) and km.Costs(lw, dw).dsym[1] == 2 and lw[256] > 0


def test_crafted_choices():
    n = 64
    b = bytes(range(n))
    # a short far match loses to three cheap literals, where the level's lazy rule keeps it
    L, D = [0] * (n + 1), [0] * (n + 1)
    L[10], D[10] = 3, 4096
    lw, dw = _widths(lit=6)                                                    # 18 against 7 + 5 + 10
    assert km.demote(b, L, D, lw, dw)[10] == 0 and km.demote(b, L, D, *_widths(lit=8))[10] == 3
    # a match is skipped to reach a longer one two bytes on — one byte further than the lazy rule looks
    L, D = [0] * (n + 1), [0] * (n + 1)
    L[10], D[10], L[12], D[12] = 3, 5, 30, 9
    out = km.demote(b, L, D, *_widths())                                       # 2 literals + 1 match against 1 match + 29 literals
    assert out[10] == 0 and out[12] == 30
    assert vm._walk(b, L, D, 16)[10] >> 16 == 3                                # the lazy walk takes the short one (L(11) = 0)
    # the last visited position: a candidate at end - 1 is decided with cost[end] = 0 — one literal against the match
    L, D = [0] * (n + 1), [0] * (n + 1)
    L[n - 4], D[n - 4] = 4, 1
    assert km.demote(b, L, D, *_widths())[n - 4] == 0 and km.demote(b, L, D, *_widths(lit=12))[n - 4] == 4 and km.demote(b, L, D, *_widths(lit=11))[n - 4] == 0


def test_matches_across_a_segment_end_and_across_the_warm_up():
    run = b"q" * 300
    buf = bytearray(TEXT[:2 * SEG + WARM + 900])
    for at in (SEG - 100, SEG + WARM - 100, 2 * SEG - 3, 2 * SEG + WARM - 2):
        buf[at:at + 300] = run
    buf = bytes(buf)
    L, D = vm.level_lengths(buf, 6)
    assert L[SEG - 99] == 258 and L[SEG + WARM - 99] == 258                    # matches that cross b and b + COST_WARM
    codes = km.cost_codes(buf, 6, LW, DW)
    assert km.replay(codes) == buf
    # cut in segments it is no shortest path any more, but never far from it, and still below the level's
    assert km.brute_force_bits(buf, 6, LW, DW) <= bits(codes) < bits(vm.level_codes(buf, 6))
    # the warm-up only informs: the positions [2 * SEG, 2 * SEG + WARM) are walked by the middle segment too, and keep what a run
    # that knows nothing of that segment — one that starts at 2 * SEG — decides there; the middle segment's own decisions are
    # those of a run that starts at SEG, and they do lean on the warm-up: without it they differ
    whole = km.demote(buf, L, D, LW, DW)
    assert whole[2 * SEG:] == km.demote(buf, L, D, LW, DW, start=2 * SEG)[2 * SEG:]
    assert whole[SEG:2 * SEG] == km.demote(buf, L, D, LW, DW, start=SEG)[SEG:2 * SEG]
    assert whole[:2 * SEG] != km.demote(buf, L, D, LW, DW, warm=0)[:2 * SEG]
    assert whole[2 * SEG:2 * SEG + WARM] != list(L[2 * SEG:2 * SEG + WARM])      # (something is demoted there: the check is not empty)


@pytest.mark.parametrize("level", [1, 6, 9])
def test_streams(oracle, level):
    data = MIXED[:3072]
    for fmt, wbits in ((oracle.DEFLATE, -15), (oracle.ZLIB, 15), (oracle.GZIP, 31)):
        for kw in ({}, {"dynamic_huffman": 0}, {"block_size": 1000, "write_size": 700}, {"max_length": 16}, {"max_length": 3, "window_size": 512}):
            z = km.expected_stream(oracle, fmt, data, level, **kw)
            assert zlib.decompress(z, wbits) == data
            if fmt == oracle.ZLIB:
                assert z[1] >> 6 == 3                                          # FLEVEL 3
            if fmt == oracle.GZIP:
                assert z[8] == 2                                               # XFL 2
    assert len(km.expected_stream(oracle, oracle.DEFLATE, data, level)) <= len(vm.expected_stream(oracle, oracle.DEFLATE, data, level))
    assert km.expected_stream(oracle, oracle.ZLIB, data, level, no_compression=1)[2:] == vm.expected_stream(oracle, oracle.ZLIB, data, level, no_compression=1)[2:]
    zdict = MIXED[4000:7000]
    z = km.expected_dict_stream(oracle, "zlib", zdict, data[:1024], level)
    d = zlib.decompressobj(zdict=zdict)
    assert d.decompress(z) + d.flush() == data[:1024]
