"""CPU: the model of the dictionary-primed encode (tests/dict_encode_model.py) against the oracle — never against the library.
Where the reference's own flush of T ‖ buf has a code-word boundary at |T|, the primed chunk's code words are the suffix of
that flush's output behind the boundary (flush inserts every position once, in order, whatever the parse does); with an empty
T the model is lz77_chunk itself.  Then the expected-stream helper once against python-zlib, and the compressed sizes of the
batch workload (tools/bench_dict.py's records) with and without the dictionary."""
import random
import zlib

import numpy as np
import pytest

import dict_encode_model as dm


def _text(n, seed):
    rng = random.Random(seed)
    words = ("the of and to in is that for it as was with be by on not he this are or record field value status error request "
             "response timestamp user session message level info warning host port path query result count total").split()
    out, size = [], 0
    while size < n:
        w = rng.choice(words) if rng.random() < 0.9 else str(rng.randrange(100000))
        out.append(w)
        size += len(w) + 1
    return " ".join(out).encode()[:n]


def _rand(n, seed, alphabet=256):
    return np.random.RandomState(seed).randint(0, alphabet, size=n, dtype=np.uint8).tobytes()


BUFS = [b"", b"a", b"ab", b"abc", b"abcd", b"abcde", b"aaaaa", b"a" * 600, b"abcabcabcabc", _text(5000, 3), _rand(3000, 4),
        _rand(4000, 5, alphabet=3), b"xyz" * 400 + _text(700, 6)]


@pytest.mark.parametrize("window,max_len", [(32768, 258), (1024, 258), (32768, 16), (256, 3)])
def test_empty_dictionary_is_lz77_chunk(oracle, window, max_len):
    for buf in BUFS:
        assert dm.primed_codes(b"", buf, window, max_len) == [int(c) for c in oracle.lz77_chunk(buf, window, max_len)], (len(buf), buf[:16])


def _suffix_check(oracle, T, buf, window=32768, max_len=258):
    """the pair must really have the boundary: asserted, not skipped"""
    T = dm.usable_tail(T)
    whole = [int(c) for c in oracle.lz77_chunk(T + buf, window, max_len)]
    k = dm.boundary_at(whole, len(T))
    assert k is not None, ("no code-word boundary at |T|", len(T), buf[:16])
    got = dm.primed_codes(T, buf, window, max_len)
    assert got == whole[k:], (len(T), buf[:16])
    return got


def _forced(T, buf, mark=0xFF):
    """a dictionary whose last byte occurs nowhere else in T ‖ buf: no match of the reference's parse can hold it, and none can
    begin in front of it and end behind it"""
    assert mark not in T and mark not in buf
    return T + bytes([mark])


@pytest.mark.parametrize("window,max_len", [(32768, 258), (1024, 258), (32768, 16)])
def test_forced_boundary_pairs(oracle, window, max_len):
    text = _text(40000, 11)
    pairs = [(text[:300], text[100:900]), (text[:32767], text[20000:23000]), (text[:32767], text[:5000]),
             (text[:32767], text[32767:40000]), (text[:5], text[:50]), (b"ab", b"abababab"), (b"", b"hello hello"),
             (_rand(2000, 21, alphabet=4), _rand(3000, 22, alphabet=4)), (text[:1000], b""), (text[:1000], b"t"), (text[:1000], b"th"),
             (text[:1000], b"the"), (text[:1000], b"the "), (text[:1000], b"the o"), (b"a" * 300, b"a" * 600),
             (text[:40000 - 1], text[39000:40000])]                  # (longer than the window: only the tail counts)
    for T, buf in pairs:
        _suffix_check(oracle, _forced(T, buf), buf, window, max_len)


def test_straddling_prefixes_are_candidates(oracle):
    """hand-made pairs whose oracle parse has the boundary and whose candidates are the two positions whose prefix straddles it"""
    # |T|-2 = "abc": buf position 1 finds it at distance 3
    got = _suffix_check(oracle, b"..xyzab", b"cabcab..")
    assert got[0] == ord("c") << 16 and got[1] & 0xFFFF == 3 and got[1] >> 16 >= 3
    # |T|-1 = "abc": buf position 3 finds it at distance 4
    got = _suffix_check(oracle, b"..xyza", b"bcQabcR..")
    assert [c >> 16 for c in got[:3]] == [ord("b"), ord("c"), ord("Q")] and got[3] == (3 << 16) | 4
    # both, and the more recent one wins: T ends "aa", buf "aaaa...": position 0 "aaa" = |T|-2 at distance 2?  no — |T|-1
    # ("a" + buf[0:2]) is the more recent occurrence, distance 1
    got = dm.primed_codes(b"xyaa", b"a" * 10)
    assert got[0] & 0xFFFF == 1
    # a run behind a dictionary that ends in its byte: distance 1 at position 0, capped lengths
    got = dm.primed_codes(b"..a", b"a" * 600)
    assert got == [(258 << 16) | 1, (258 << 16) | 1, (84 << 16) | 1]


def test_contract_corners():
    T = _text(32768, 31)
    # a match starts in the dictionary and runs on into the record: T's tail + the record's head repeat in the record
    rec = b"=" + T[-40:] + b"#!" + T[-40:] + b"#!" + b"~"
    got = dm.primed_codes(T, rec)
    assert got[0] == ord("=") << 16 and got[1] == (40 << 16) | 41              # T[-40:] at distance 40 + 1
    # an in-record occurrence shadows a dictionary one
    rec = b"QQtimestampQQ" + T[100:110] + b"  " + T[100:110]
    got = dm.primed_codes(T, rec)
    assert any(c & 0xFFFF == 12 for c in got)
    # distance exactly 32768 is a match, 32769 a literal although an older occurrence in reach exists
    base = bytes(range(33, 123)) * 400
    T2 = b"@#$%" + base[:32764]
    assert dm.primed_codes(T2, b"@#$") == [ord(c) << 16 for c in "@#$"]        # (end = |T|: nothing is walked)
    assert dm.primed_codes(T2, b"@#$%") == [(4 << 16) | 32768]                 # (end = |T| + 1: position 0 is, bounded by the end)
    got = dm.primed_codes(T2, b"@#$%^&")
    assert got[0] == (4 << 16) | 32768
    got = dm.primed_codes(T2, b"~@#$%^&")
    assert got[:2] == [ord("~") << 16, ord("@") << 16]                         # 32769: a literal
    T3 = b"@#$%" + base[:32000] + b"@#$%" + base[:760]                         # an older occurrence at 32769, the recent one in reach
    assert len(T3) == 32768
    got = dm.primed_codes(T3, b"~@#$%^&")
    assert got[1] & 0xFFFF == 1 + 764
    # window_size: a candidate beyond it is a literal even when the dictionary holds the bytes
    got = dm.primed_codes(T, T[:64], window=1024)
    assert all(c & 0xFFFF <= 1024 for c in got)
    # max_length
    assert max(c >> 16 for c in dm.primed_codes(T, T[-500:], max_len=16) if c & 0xFFFF) == 16


def test_expected_stream_reads_back_with_python_zlib(oracle):
    T = _text(40000, 41)
    data = T[-300:] + _text(3000, 42) + T[1000:1200]
    for fmt in ("zlib", "deflate"):
        z = dm.expected_stream(oracle, fmt, T, data)
        assert dm.py_inflate(fmt, z, T) == data
        if fmt == "zlib":
            assert z[1] & 0x20 and (z[0] * 256 + z[1]) % 31 == 0 and z[2:6] == zlib.adler32(T).to_bytes(4, "big")
            plain = oracle.encode(oracle.ZLIB, data)
            assert z[0] == plain[0] and z[1] & 0xC0 == plain[1] & 0xC0 and len(z) < len(plain)
    # three chunks, only the first primed; stored blocks; every byte a literal
    big = T[:20000] + _text(600 * 1024 - 20000, 43)
    assert dm.py_inflate("zlib", dm.expected_stream(oracle, "zlib", T, big, write_size=8192), T) == big
    for kw in (dict(no_compression=1), dict(lz77_kind=oracle.LZ77_NOCOMPRESSION), dict(dynamic_huffman=0), dict(window_size=1024),
               dict(max_length=16), dict(block_size=1000)):
        assert dm.py_inflate("zlib", dm.expected_stream(oracle, "zlib", T, data, **kw), T) == data, kw
    # an empty dictionary: FDICT and id 1, the body of the dictionary-less call
    z = dm.expected_stream(oracle, "zlib", b"", data)
    assert z[2:6] == b"\0\0\0\1" and z[6:] == oracle.encode(oracle.ZLIB, data)[2:]


def test_batch_workload_sizes_with_the_model(oracle):
    """tools/bench_dict.py's records (a sample of them): the greedy last-occurrence parse with the dictionary must beat the
    same parse without it; python-zlib level 9 makes 373 / 499 bytes a record of the same data"""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import bench_dict_encode as bd
    zdict = bd.text(32768, 1)
    rng = random.Random(7)
    recs = [bd.text(rng.randrange(900, 1200), 100 + i) for i in range(64)]
    with_d = sum(len(dm.expected_stream(oracle, "zlib", zdict, r)) for r in recs)
    plain = sum(len(oracle.encode(oracle.ZLIB, r)) for r in recs)
    print("model, bytes a record: %.1f with the dictionary, %.1f without" % (with_d / 64, plain / 64))
    assert with_d < plain
    for r in recs[:4]:
        assert dm.py_inflate("zlib", dm.expected_stream(oracle, "zlib", zdict, r), zdict) == r
