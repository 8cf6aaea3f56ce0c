"""CPU: the model of LazyLz77Encoder (tests/lazy_model.py) against the model of ChainLz77Encoder, which
test_chain_model.py proves on the oracle, and against python-zlib — never against the library.  The per-position lengths, walked
greedily, are chain_model's code words, so the two models share their candidates; the lazy walk replays to the input inside
the window and the cap; crafted buffers pin the rule (the next is longer: a literal; a rising run: literals until it stops
rising; 257 then 258; 258 then 258: no demotion); the stream the model implies is read by python-zlib in all three formats and
is smaller than the chain's on a golden input."""
import gzip
import os
import zlib

import pytest

import chain_model as cm
import lazy_model as lm
from test_chain_model import BUFS

from test_dict_encode_model import _rand, _text

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "issue_52_input.bin")

# In the style of test_chain_model.OLDER_LONGER.  At the last "abcdefghij" the only earlier "abc" is "abcQ" (length 3, 6 back),
# and one byte on "bcdefghij" has a copy of 9 (18 back): greedy takes the 3, lazy a literal and the 9.
HIST = b"bcdefghij" + b"--" + b"abcQ" + b"++"
NEXT_LONGER = HIST + b"abcdefghij" + b"!!!!"
# L = 3, 5, 9 at three positions in a row (each prefix's longest copy is also its nearest): two literals, then the 9
RISE_HIST = b"abcQ" + b"--" + b"bcdefR" + b"++" + b"cdefghijk" + b"=="
RISING = RISE_HIST + b"abcdefghijk" + b"!!!!"


def long_pair(first, second, seed=80):
    """a buffer with L(at) = first and L(at + 1) = second, both of 250..258, and `at`.  Two phrases over disjoint alphabets,
    so that no prefix of one occurs in the other: A = x + B[:k] gives L(at) = 1 + k when the copy of A's first 1 + k bytes is
    followed by another byte, and B gives L(at + 1)"""
    B = bytes(_rand(300, seed, alphabet=20))                       # bytes 0..19
    x = b"\xF0"
    sep = lambda i: bytes([0xE0 + i]) * 2
    hist = sep(0) + x + B[:first - 1] + sep(1) + B[:second] + sep(2)
    return hist + x + B + sep(3) * 3, len(hist)


def place(total, at, tail=b"abcdefghij", seed=90):
    """`total` bytes of filler from 128..255 (no prefix of it occurs in the crafted part) with HIST right in front of `at` and
    `tail` at `at`: the deferred pair sits at at / at + 1"""
    assert at >= len(HIST)
    total = max(total, at + len(tail))
    fill = bytes(128 + (v & 127) for v in _rand(total, seed))
    buf = fill[:at - len(HIST)] + HIST + tail
    return buf + fill[len(buf):]


@pytest.mark.parametrize("depth", [1, 2, 8, 255])
@pytest.mark.parametrize("window,max_len", [(32768, 258), (1024, 258), (32768, 16)])
def test_lengths_walked_greedily_are_the_chain_models_code_words(depth, window, max_len):
    for buf in BUFS:
        assert lm.greedy_codes(buf, depth, window, max_len) == cm.chain_codes(buf, depth, window, max_len), (len(buf), buf[:16])


@pytest.mark.parametrize("depth", [1, 2, 8, 255])
@pytest.mark.parametrize("window,max_len", [(32768, 258), (1024, 258), (32768, 16)])
def test_code_words_replay_inside_window_and_cap(depth, window, max_len):
    for buf in BUFS + [NEXT_LONGER, RISING]:
        codes = lm.lazy_codes(buf, depth, window, max_len)
        assert lm.replay(codes) == buf, (len(buf), buf[:16])
        assert all((c & 0xFFFF) <= window for c in codes)
        assert all((c >> 16) <= max_len for c in codes if c & 0xFFFF)
        L, D = lm.lengths(buf, depth, window, max_len)
        assert all(L[p] == 0 for p in range(max(3, len(buf)) - 3, len(buf) + 1))      # L(p) = 0 for every p >= end


@pytest.mark.parametrize("depth", [1, 8])
def test_max_length_3_is_the_chain(depth):
    assert lm._length(b"abcdefgh" * 40 + b"abcdefgX", 8, 0, 258) == cm._length(b"abcdefgh" * 40 + b"abcdefgX", 8, 0, 258) == 258
    for i, c, m in ((16, 0, 258), (300, 12, 258), (8, 0, 16), (300, 299, 19), (310, 0, 258)):
        assert lm._length(b"abcdefgh" * 40 + b"abcdefgX", i, c, m) == cm._length(b"abcdefgh" * 40 + b"abcdefgX", i, c, m)
    for buf in BUFS + [NEXT_LONGER, RISING]:
        assert lm.lazy_codes(buf, depth, 32768, 3) == cm.chain_codes(buf, depth, 32768, 3)      # nothing can be longer


def test_next_is_longer():
    at = len(HIST)
    for depth in (1, 2, 8):
        L, D = lm.lengths(NEXT_LONGER, depth)
        assert (L[at], D[at], L[at + 1], D[at + 1]) == (3, 6, 9, 18)
        lazy, greedy = lm.lazy_codes(NEXT_LONGER, depth), cm.chain_codes(NEXT_LONGER, depth)
        assert greedy[at:at + 2] == [(3 << 16) | 6, (7 << 16) | 18]
        assert lazy[at:at + 2] == [ord("a") << 16, (9 << 16) | 18]
        assert lm.replay(lazy) == NEXT_LONGER and len(lazy) == len(greedy)
    assert lazy[:at] == greedy[:at] == [x << 16 for x in HIST]


def test_rising_run_of_three():
    at = len(RISE_HIST)
    for depth in (1, 8):
        L, D = lm.lengths(RISING, depth)
        assert L[at:at + 4] == (3, 5, 9, 8)
        lazy = lm.lazy_codes(RISING, depth)
        i = next(k for k, c in enumerate(lazy) if (c >> 16, c & 0xFFFF) == (9, D[at + 2]))
        assert lazy[i - 2:i] == [ord("a") << 16, ord("b") << 16]
        assert lm.replay(lazy) == RISING


def test_257_then_258_and_258_twice():
    buf, at = long_pair(257, 258)
    L, D = lm.lengths(buf, 8)
    assert (L[at], L[at + 1]) == (257, 258)
    lazy = lm.lazy_codes(buf, 8)
    assert (258 << 16) | D[at + 1] in lazy and (257 << 16) | D[at] not in lazy and lm.replay(lazy) == buf
    assert (257 << 16) | D[at] in cm.chain_codes(buf, 8)
    buf, at = long_pair(258, 258)
    L, D = lm.lengths(buf, 8)
    assert (L[at], L[at + 1]) == (258, 258)
    lazy = lm.lazy_codes(buf, 8)
    assert (258 << 16) | D[at] in lazy and lm.replay(lazy) == buf              # no demotion: not strictly longer


def test_placed_pairs():
    """the builder the GPU cases use: the pair sits where it is asked for, also three bytes in front of the end"""
    for total, at in ((200, 17), (40960, 16383), (40960, 16384), (40960, 16385)):
        buf = place(total, at)
        L, _ = lm.lengths(buf, 8)
        assert (L[at], L[at + 1]) == (3, 9), (total, at)
    buf = place(0, 500, tail=b"abcde")                                          # at = end - 2: L(end - 1) is capped by the end
    L, _ = lm.lengths(buf, 8)
    assert len(buf) == 505 and (L[500], L[501], L[502]) == (3, 4, 0)
    assert lm.lazy_codes(buf, 8)[-2:] == [ord("a") << 16, (4 << 16) | 18]


@pytest.mark.parametrize("depth", [1, 8])
def test_python_zlib_reads_the_expected_stream(oracle, depth):
    data = _text(20000, 21) + b"a" * 700 + _rand(500, 22)
    z = lm.expected_stream(oracle, oracle.ZLIB, data, depth)
    assert zlib.decompress(z) == data
    assert z[1] >> 6 == 3                        # FLEVEL: compression_level() is Best
    g = lm.expected_stream(oracle, oracle.GZIP, data, depth, mtime=0)
    assert gzip.decompress(g) == data
    assert g[8] == 2                             # XFL: Slowest
    r = lm.expected_stream(oracle, oracle.DEFLATE, data, depth, write_size=8192)
    assert zlib.decompress(r, -15) == data
    assert r == lm.expected_scheduled(oracle, oracle.DEFLATE, data, depth, [8192] * 3)
    # a caller's level is the one written
    assert lm.expected_stream(oracle, oracle.ZLIB, data, depth, level=1)[1] >> 6 == 1


def test_lazy_is_smaller_than_the_chain_on_a_golden_input(oracle):
    data = open(GOLDEN, "rb").read()
    for depth in (1, 8, 32):
        lazy = lm.expected_stream(oracle, oracle.DEFLATE, data, depth)
        chained = cm.expected_stream(oracle, oracle.DEFLATE, data, depth)
        assert zlib.decompress(lazy, -15) == data
        assert len(lazy) < len(chained), (depth, len(lazy), len(chained))
