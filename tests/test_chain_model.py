"""CPU: the model of ChainLz77Encoder (tests/chain_model.py) against the oracle and python-zlib — never against
the library.  At depth 1 the model is the reference's DefaultLz77Encoder (lz77_chunk); at any depth its code words replay to the
input inside the window and the length cap; two crafted buffers pin the choice rule (the longest, among equals the nearest);
the stream the model implies is read by python-zlib in all three formats, and is smaller than the default one on a golden
input."""
import gzip
import os
import zlib

import pytest

import chain_model as cm
from test_dict_encode_model import _rand, _text

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "issue_52_input.bin")

BUFS = [b"", b"a", b"ab", b"abc", b"abcd", b"abcde", b"aaaaa", b"a" * 600, b"abcabcabcabc", _text(5000, 3), _rand(3000, 4),
        _rand(4000, 5, alphabet=3), b"xyz" * 400 + _text(700, 6), b"abcdefg" * 300]

# the older of two candidates is the longer one: at the last "abcdefgh" the nearest occurrence of "abc" is "abcQ" (length 3, 6
# back), the one behind it "abcdefgh" (length 8, 16 back)
OLDER_LONGER = b"abcdefgh" + b"--" + b"abcQ" + b"++" + b"abcdefgh" + b"!!!!"
# two candidates tie: "abcdY" 7 back and "abcdX" 14 back both give length 4
TIE = b"abcdX" + b"--" + b"abcdY" + b"++" + b"abcdZ" + b"!!!!"


@pytest.mark.parametrize("window,max_len", [(32768, 258), (1024, 258), (32768, 16), (256, 3)])
def test_depth_1_is_lz77_chunk(oracle, window, max_len):
    for buf in BUFS:
        assert cm.chain_codes(buf, 1, window, max_len) == [int(c) for c in oracle.lz77_chunk(buf, window, max_len)], (len(buf), buf[:16])


@pytest.mark.parametrize("depth", [2, 8, 255])
@pytest.mark.parametrize("window,max_len", [(32768, 258), (1024, 258), (32768, 16)])
def test_code_words_replay_inside_window_and_cap(depth, window, max_len):
    for buf in BUFS:
        codes = cm.chain_codes(buf, depth, window, max_len)
        assert cm.replay(codes) == buf, (len(buf), buf[:16])
        assert all((c & 0xFFFF) <= window for c in codes)
        assert all((c >> 16) <= max_len for c in codes if c & 0xFFFF)


def test_older_candidate_is_longer_and_chosen():
    at = OLDER_LONGER.rindex(b"abcdefgh")
    d1, d2 = cm.chain_codes(OLDER_LONGER, 1), cm.chain_codes(OLDER_LONGER, 2)
    assert (3 << 16) | 6 in d1 and (8 << 16) | 16 not in d1
    assert (8 << 16) | 16 in d2
    assert cm.replay(d2) == OLDER_LONGER and len(d2) < len(d1)
    assert at == 16


def test_tie_goes_to_the_nearer():
    for depth in (1, 2, 8):
        codes = cm.chain_codes(TIE, depth)
        assert (4 << 16) | 7 in codes and (4 << 16) | 14 not in codes, depth
        assert cm.replay(codes) == TIE


@pytest.mark.parametrize("depth", [1, 8])
def test_python_zlib_reads_the_expected_stream(oracle, depth):
    data = _text(20000, 21) + b"a" * 700 + _rand(500, 22)
    z = cm.expected_stream(oracle, oracle.ZLIB, data, depth)
    assert zlib.decompress(z) == data
    assert z[1] >> 6 == 3                        # FLEVEL: compression_level() is Best
    g = cm.expected_stream(oracle, oracle.GZIP, data, depth, mtime=0)
    assert gzip.decompress(g) == data
    assert g[8] == 2                             # XFL: Slowest
    r = cm.expected_stream(oracle, oracle.DEFLATE, data, depth, write_size=8192)
    assert zlib.decompress(r, -15) == data
    # a caller's level is the one written
    assert cm.expected_stream(oracle, oracle.ZLIB, data, depth, level=1)[1] >> 6 == 1


def test_depth_8_is_smaller_than_the_default_on_a_golden_input(oracle):
    data = open(GOLDEN, "rb").read()
    default = oracle.encode(oracle.DEFLATE, data)
    chained = cm.expected_stream(oracle, oracle.DEFLATE, data, 8)
    assert zlib.decompress(chained, -15) == data
    assert len(chained) < len(default), (len(chained), len(default))
    assert cm.expected_stream(oracle, oracle.DEFLATE, data, 1) == default
