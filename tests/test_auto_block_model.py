"""CPU: the model of LFX_HUFFMAN_AUTO (auto_block_model.py, the contract of include/lfx.h restated) against the oracle and
python-zlib — every model stream inflates to its input and is no longer than either oracle stream; the case set meets each of
the three forms, an F == D tie, and a block one bit either side of S == min(D, F)."""
import gzip as pygzip
import zlib

import pytest

import auto_block_model as model
import auto_cases as cases
from auto_block_model import DYNAMIC, FIXED, STORED

FORMATS = ("deflate", "zlib", "gzip")


def inflate(fmt, stream):
    if fmt == "gzip":
        return pygzip.decompress(stream)
    return zlib.decompress(stream, -15 if fmt == "deflate" else 15)


def kw_of(fmt, **kw):
    return dict(kw, mtime=0) if fmt == "gzip" else kw


def check(oracle, fmt, data, result, *streams, stored_ok=True):
    out, choices, sizes = result
    assert inflate(fmt, out) == data
    for s in streams:
        assert len(out) <= len(s)
    for pick, sz in zip(choices, sizes):
        if sz is not None:
            assert pick == model.choose(*sz, stored_ok=stored_ok)
    return choices


def both(oracle, fmt, data, **kw):
    code = {"deflate": oracle.DEFLATE, "zlib": oracle.ZLIB, "gzip": oracle.GZIP}[fmt]
    return [oracle.encode(code, data, **dict(kw, dynamic_huffman=dh)) for dh in (1, 0)]


def test_rule():
    assert model.choose(100, 100, 1000) == FIXED                 # the tie goes to fixed
    assert model.choose(100, 101, 1000) == DYNAMIC
    assert model.choose(8 * 7 + 43, 8 * 7 + 50, 7) == STORED     # S = 98 < 99
    assert model.choose(8 * 7 + 42, 8 * 7 + 50, 7) == DYNAMIC    # S == D: not smaller
    assert model.choose(8 * 7 + 50, 8 * 7 + 42, 7) == FIXED
    assert model.choose(10**6, 10**6 + 1, 65535) == STORED and model.choose(10**6, 10**6 + 1, 65536) == DYNAMIC
    assert model.choose(90, 10, 0) == FIXED                      # no bytes: nothing to store
    assert model.choose(10**6, 10**6, 100, stored_ok=False) == FIXED


@pytest.mark.parametrize("fmt", FORMATS)
def test_sizes(oracle, fmt):
    seen = set()
    for n in cases.SIZES:
        data = cases.record(n)
        kw = kw_of(fmt)
        seen |= set(check(oracle, fmt, data, model.expected(oracle, fmt, data, **kw), *both(oracle, fmt, data, **kw)))
    assert seen == {FIXED, DYNAMIC}


def test_empty_stream_is_two_bytes(oracle):
    out, choices, sizes = model.expected(oracle, "deflate", b"")
    assert out == b"\x03\x00" and choices == [FIXED] and sizes == [(90, 10, 0)]


def test_random_and_the_eligibility_edge(oracle):
    for n, want in ((1000, [STORED]), (60000, [STORED]), (65535, [STORED]), (65536, [DYNAMIC])):
        data = cases.rand(n)
        assert check(oracle, "deflate", data, model.expected(oracle, "deflate", data), *both(oracle, "deflate", data)) == want
    data = cases.rand(60000)
    enc = lambda f, d, **kw: oracle.encode(oracle.ZLIB, d, 4096, **kw)       # 4096-byte writes: one block of eight LZ77 chunks
    res = model.expected(oracle, "zlib", data, encode=enc, window_size=1024)
    streams = [enc("zlib", data, window_size=1024, dynamic_huffman=dh) for dh in (1, 0)]
    assert check(oracle, "zlib", data, res, *streams) == [STORED]


def test_tie_goes_to_fixed(oracle):
    data = cases.record(*cases.TIE)
    out, choices, sizes = model.expected(oracle, "deflate", data)
    assert sizes[0][0] == sizes[0][1] and choices == [FIXED]
    check(oracle, "deflate", data, (out, choices, sizes), *both(oracle, "deflate", data))


def test_one_bit_either_side_of_stored(oracle):
    got = []
    for data, want in cases.S_EDGE:
        out, choices, sizes = model.expected(oracle, "deflate", data)
        D, F, n = sizes[0]
        assert min(D, F) - (8 * n + 42) == want
        got.append(choices[0])
        check(oracle, "deflate", data, (out, choices, sizes), *both(oracle, "deflate", data))
    assert got[0] != STORED and got[1] != STORED and got[2] == STORED


@pytest.mark.parametrize("fmt", FORMATS)
def test_mixed_meets_every_form_at_every_bit_phase(oracle, fmt):
    phases = set()
    for length in cases.PHASE_PREFIX:
        data, writes = cases.prefixed(length)
        kw = kw_of(fmt, block_size=4096)
        res = model.expected_writes(oracle, fmt, data, writes, **kw)
        streams = [model.oracle_writes(oracle, fmt, data, writes, **dict(kw, dynamic_huffman=dh)) for dh in (1, 0)]
        assert check(oracle, fmt, data, res, *streams) == [DYNAMIC, STORED, DYNAMIC, FIXED]
        h, t = model.header_len(fmt, res[0]), model.TRAILER[fmt]
        blocks = oracle.scan_blocks(res[0][h:len(res[0]) - t])
        assert [b[2] for b in blocks] == res[1]
        phases.add(blocks[1][0] % 8)
    assert phases == set(range(8))


def test_max_length_3_and_flushes(oracle):
    data = cases.record(3000, 5) + cases.rand(500, 2)
    check(oracle, "zlib", data, model.expected(oracle, "zlib", data, max_length=3), *both(oracle, "zlib", data, max_length=3))
    msgs = cases.messages()
    data = b"".join(msgs)
    writes = [x for m in msgs for x in (len(m), None)]
    for fmt in FORMATS:
        kw = kw_of(fmt)
        res = model.expected_writes(oracle, fmt, data, writes, **kw)
        streams = [model.oracle_writes(oracle, fmt, data, writes, **dict(kw, dynamic_huffman=dh)) for dh in (1, 0)]
        assert set(check(oracle, fmt, data, res, *streams)) == {STORED, FIXED, DYNAMIC}
        coded = model.expected_writes(oracle, fmt, data, writes, stored_ok=False, **kw)
        assert STORED not in check(oracle, fmt, data, coded, *streams, stored_ok=False)
    # zlib sync flush: the marker is a stored block of the plan, copied
    res = model.expected_writes(oracle, "zlib", data, writes, zlib_sync_flush=1)
    assert inflate("zlib", res[0]) == data and res[2].count(None) == len(msgs)


def test_behind_a_preset_dictionary(oracle):
    """the model reads a dictionary stream's blocks with the dictionary's tail put in front; a stored block holds the record alone"""
    import dict_encode_model as dm
    enc = lambda f, d, **kw: dm.expected_stream(oracle, f, cases.DICT, d, **kw)
    seen = set()
    for rec in cases.batch_records()[::9] + [cases.rand(3000, 9)]:
        for fmt in ("deflate", "zlib"):
            out, choices, sizes = model.expected(oracle, fmt, rec, encode=enc, zdict=cases.DICT)
            assert dm.py_inflate(fmt, out, cases.DICT) == rec
            for dh in (1, 0):
                assert len(out) <= len(enc(fmt, rec, dynamic_huffman=dh))
            seen |= set(choices)
    assert seen == {STORED, FIXED, DYNAMIC}
    assert model.expected(oracle, "deflate", cases.rand(3000, 9), encode=enc, zdict=cases.DICT)[0][5:] == cases.rand(3000, 9)
