"""CPU: the model of the chained and the lazy parse through a chain dictionary (tests/dict_chain_model.py)
against what exists already — chain_model, lazy_model, dict_encode_model, python-zlib — never against the library."""
import os
import random
import sys
import zlib

import pytest

import chain_model
import dict_chain_model as dcm
import dict_encode_model as dm
import lazy_model
from test_dict_encode_model import BUFS, _forced, _rand, _text

PARAMS = [(32768, 258), (1024, 258), (32768, 16), (256, 3)]


@pytest.mark.parametrize("window,max_len", PARAMS)
def test_empty_dictionary_is_the_unprimed_parse(window, max_len):
    for buf in BUFS:
        for depth in (1, 8, 255):
            assert dcm.primed_codes(b"", buf, dcm.LAZY, depth, window, max_len) == lazy_model.lazy_codes(buf, depth, window, max_len)
            assert dcm.primed_codes(b"", buf, dcm.CHAIN, depth, window, max_len) == chain_model.chain_codes(buf, depth, window, max_len)


@pytest.mark.parametrize("window,max_len", PARAMS)
def test_depth_1_greedy_is_the_primed_default_parse(window, max_len):
    text = _text(40000, 11)
    pairs = [(text[:300], text[100:900]), (text[:32768], text[20000:23000]), (text[:5], text[:50]), (b"ab", b"cabcabcabc"),
             (b"a" * 100, b"a" * 600), (b"..xyza", b"bcQabcR.."), (b"xyaa", b"a" * 10), (text[:40000], text[39000:40000] + text[:700]),
             (_rand(2000, 21, alphabet=4), _rand(3000, 22, alphabet=4)), (text[:1000], b""), (text[:1000], b"the"), (text[:1000], b"the o")]
    for T, buf in pairs:
        assert dcm.primed_codes(T, buf, dcm.CHAIN, 1, window, max_len) == dm.primed_codes(T, buf, window, max_len), (len(T), buf[:16])


@pytest.mark.parametrize("depth", [2, 8, 255])
@pytest.mark.parametrize("window,max_len", PARAMS[:3])
def test_forced_boundary_is_the_suffix_of_the_whole_parse(depth, window, max_len):
    """T's last byte occurs nowhere else: chain_model's parse of T ‖ buf has a code-word boundary at |T|, and what stands
    behind it is the greedy model's output (every position is inserted once, in order, whatever the parse does)"""
    text = _text(40000, 11)
    pairs = [(text[:300], text[100:900]), (text[:32767], text[20000:23000]), (text[:32767], text[32767:40000]), (text[:5], text[:50]),
             (b"ab", b"abababab"), (b"", b"hello hello"), (_rand(2000, 21, alphabet=4), _rand(3000, 22, alphabet=4)), (text[:1000], b""),
             (text[:1000], b"the "), (b"a" * 300, b"a" * 600), (text[:40000 - 1], text[39000:40000])]
    for T, buf in pairs:
        T = dm.usable_tail(_forced(T, buf))
        whole = chain_model.chain_codes(T + buf, depth, window, max_len)
        k = dm.boundary_at(whole, len(T))
        assert k is not None, ("no code-word boundary at |T|", len(T), buf[:16])
        assert dcm.primed_codes(T, buf, dcm.CHAIN, depth, window, max_len) == whole[k:], (len(T), buf[:16])


def test_contract_corners():
    # the candidate at |T|-2, then the chain |T|-1 → |T|-2 → the dictionary's own
    assert dcm.primed_codes(b"..xyzab", b"cabcabc", dcm.CHAIN, 8)[:2] == [ord("c") << 16, (6 << 16) | 3]
    assert dcm.primed_codes(b"a" * 100, b"a" * 600, dcm.CHAIN, 8) == [(258 << 16) | 1, (258 << 16) | 1, (84 << 16) | 1]
    # an older dictionary occurrence that matches longer wins at depth 2 and not at depth 1
    T = b"0123456789abcdefgh" + b"#" * 40 + b"0123456789zzz" + b"#" * 40
    rec = b"0123456789abcdefgh!"
    assert dcm.primed_codes(T, rec, dcm.CHAIN, 1)[0] == (10 << 16) | 53
    assert dcm.primed_codes(T, rec, dcm.CHAIN, 2)[0] == (18 << 16) | 111
    # an in-chunk and a dictionary candidate of equal length: the nearer one stays
    got = dcm.primed_codes(b"..QRSTUV..", b"QRSTUV--QRSTUV++", dcm.CHAIN, 8)
    assert got[0] == (6 << 16) | 8 and got[3] == (6 << 16) | 8      # (position 8: distance 8 in the chunk, 16 into T)
    # the cut-off is taken from the chunk position: 1024 is a candidate, 1025 is none
    base = bytes(range(33, 123)) * 20
    T = b"@#$%^" + base[:1019]
    assert len(T) == 1024 and dcm.primed_codes(T, b"@#$%^&", dcm.CHAIN, 8, window=1024)[0] == (5 << 16) | 1024
    assert dcm.primed_codes(T, b"~@#$%^&", dcm.CHAIN, 8, window=1024)[:2] == [ord("~") << 16, ord("@") << 16]
    # lazy: L(1) > L(0) where L(1) comes from T; position 0 is a literal
    T = b"..abcd....bcdefghij.."
    got = dcm.primed_codes(T, b"abcdefghij!", dcm.LAZY, 8)
    assert got[0] == ord("a") << 16 and got[1] >> 16 == 9 and dcm.primed_codes(T, b"abcdefghij!", dcm.CHAIN, 8)[0] >> 16 == 4
    # a match that starts in T and runs to the end of a 5-byte chunk (end = |T| + 2)
    assert dcm.primed_codes(b"..hello", b"hello", dcm.CHAIN, 8) == [(5 << 16) | 5]
    # positions < |T| are never visited, and the positions from max(end, |T|) on are literals
    assert dcm.primed_codes(b"abcabc", b"ab", dcm.LAZY, 8) == [ord("a") << 16, ord("b") << 16]


def test_expected_stream_reads_back_with_python_zlib(oracle):
    T = _text(40000, 41)
    data = T[-300:] + _text(3000, 42) + T[1000:1200]
    for kind in (dcm.CHAIN, dcm.LAZY):
        for depth in (1, 8, 255):
            for fmt in ("deflate", "zlib"):
                z = dcm.expected_stream(oracle, fmt, T, data, kind, depth)
                assert dcm.py_inflate(fmt, z, T) == data
            assert z[1] >> 6 == 3 and z[1] & 0x20 and (z[0] * 256 + z[1]) % 31 == 0 and z[2:6] == zlib.adler32(T).to_bytes(4, "big")
        for kw in (dict(dynamic_huffman=0), dict(window_size=1024), dict(max_length=16), dict(max_length=3), dict(block_size=1000)):
            assert dcm.py_inflate("zlib", dcm.expected_stream(oracle, "zlib", T, data, kind, 8, **kw), T) == data, kw
        # two chunks, only the first primed
        big = T[:20000] + _text(300 * 1024 - 20000, 43)
        assert dcm.py_inflate("zlib", dcm.expected_stream(oracle, "zlib", T, big, kind, 8, write_size=8192), T) == big
        # an empty dictionary: FDICT and id 1, the body of the dictionary-less call of the same kind
        model = lazy_model if kind == dcm.LAZY else chain_model
        z = dcm.expected_stream(oracle, "zlib", b"", data, kind, 8)
        assert z[2:6] == b"\0\0\0\1" and z[6:] == model.expected_stream(oracle, oracle.ZLIB, data, 8)[2:]


def test_batch_workload_sizes_with_the_model(oracle):
    """tools/bench_dict_encode.py's records, the first 64: dictionary + lazy 8 < dictionary, default parse < lazy 8 without
    a dictionary (bytes a record)"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import bench_dict_encode as bd
    zdict = bd.text(32768, 1)
    rng = random.Random(7)
    recs = [bd.text(rng.randrange(900, 1200), 100 + i) for i in range(64)]
    size = {"dict": sum(len(dm.expected_stream(oracle, "zlib", zdict, r)) for r in recs) / 64,
            "lazy8": sum(len(lazy_model.expected_stream(oracle, oracle.ZLIB, r, 8)) for r in recs) / 64}
    for name, kind, depth in (("dict+chain8", dcm.CHAIN, 8), ("dict+lazy8", dcm.LAZY, 8), ("dict+lazy32", dcm.LAZY, 32)):
        size[name] = sum(len(dcm.expected_stream(oracle, "zlib", zdict, r, kind, depth)) for r in recs) / 64
    print("model, bytes a record: " + ", ".join("%s %.1f" % kv for kv in sorted(size.items())))
    assert size["dict+lazy8"] < size["dict"] < size["lazy8"]
    for r in recs[:4]:
        assert dcm.py_inflate("zlib", dcm.expected_stream(oracle, "zlib", zdict, r, dcm.LAZY, 8), zdict) == r
