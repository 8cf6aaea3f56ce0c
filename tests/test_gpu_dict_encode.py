"""GPU: encoding with a preset dictionary (include/lfx.h "encoding with a preset dictionary") through the
one-shot calls, the host call, the batch call and the module helpers.  Every case compares bytes, zlib and raw DEFLATE, with
the stream the contract implies (tests/dict_encode_model.py: the oracle's generic encoder over the model's code words;
test_dict_encode_model.py proves the model against the oracle on the CPU), and every output is read back by python-zlib and
by lfx_decode_dict_device.  Integer work: every comparison is exact."""
import ctypes as C
import random
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import dict_encode_model as dm
from test_dict_encode_model import _rand, _text
from test_gpu_encode_stages import context_with
from test_gpu_parity import ctx, ffi, lfx  # noqa: F401  (fixtures)

KIB = 1 << 10
GUARD = 64


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def _dev(torch, data):
    a = np.frombuffer(bytes(data), dtype=np.uint8).copy() if len(data) else np.zeros(4, dtype=np.uint8)
    return torch.from_numpy(a).to("cuda")


TEXT = _text(48 * KIB, 51)
D32 = TEXT[:32768]


@pytest.fixture(scope="module")
def dicts(lfx, ctx):
    """one Dictionary per distinct dictionary (and context), made once"""
    made = {}

    def get(zdict, c=ctx):
        if (zdict, id(c)) not in made:
            made[(zdict, id(c))] = lfx.Dictionary(zdict, c)
        return made[(zdict, id(c))]
    yield get
    for d in made.values():
        d.close()


def encode(c, ffi, torch, fmt, zd, data, write_size=0, **kw):
    """lfx_encode_dict_device on device buffers, a guard behind the capacity → the stream"""
    opts, sched = ffi.make_opts(**kw), ffi.make_schedule(write_size)
    cap = (ffi.lib().lfx_encode_dict_bound(len(data), C.byref(opts), C.byref(sched)) + 3) & ~3
    d_in = _dev(torch, data)
    d_out = torch.full((cap + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    n = c.encode_dict_device(fmt, zd, d_in.data_ptr(), len(data), d_out.data_ptr(), cap, opts, sched)
    whole = d_out.cpu().numpy().tobytes()
    assert whole[cap:] == b"\xA5" * GUARD, "bytes behind cap were written"
    return whole[:n]


def check(c, ffi, torch, oracle, dicts, zdict, data, write_size=0, **kw):
    """both formats: bytes equal to the expected stream; python-zlib and lfx_decode_dict_device read them back"""
    zd = dicts(zdict, c)
    okw = dict(kw)
    if "lz77_kind" in okw:
        okw["lz77_kind"] = oracle.LZ77_NOCOMPRESSION
    for name, fmt in (("deflate", ffi.DEFLATE), ("zlib", ffi.ZLIB)):
        got = encode(c, ffi, torch, fmt, zd, data, write_size, **kw)
        want = dm.expected_stream(oracle, name, zdict, data, write_size, **okw)
        assert got == want, (name, len(zdict), len(data), kw, len(got), len(want))
        assert dm.py_inflate(name, got, zdict) == data
        d_in = _dev(torch, got)
        d_out = torch.full((max(len(data), 4),), 0x5A, dtype=torch.uint8, device="cuda")
        rc, ol, used, msg = c.decode_dict_device(fmt, zd, d_in.data_ptr(), len(got), d_out.data_ptr(), len(data))
        assert (rc, ol, used) == (ffi.OK, len(data), len(got)), (name, rc, ol, used, msg)
        assert d_out.cpu().numpy().tobytes()[:ol] == data
    return got                  # (the zlib stream)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 300])
def test_record_lengths(ctx, ffi, torch, oracle, dicts, n):
    check(ctx, ffi, torch, oracle, dicts, D32, D32[-5:][:n] if n <= 5 else TEXT[20000:20000 + n])
    check(ctx, ffi, torch, oracle, dicts, D32, TEXT[40000:40000 + n])


@pytest.mark.parametrize("m", [1, 2, 3, 258, 32767, 32768, 32769, 40000])
def test_dictionary_lengths(lfx, ctx, ffi, torch, oracle, dicts, m):
    """for 32769 and 40000 the tail counts and the id covers all bytes"""
    zdict = TEXT[:m]
    rec = zdict[-300:] + TEXT[41000:41300] + zdict[:200] + zdict[-32768:][:64]
    z = check(ctx, ffi, torch, oracle, dicts, zdict, rec)
    assert int.from_bytes(z[2:6], "big") == zlib.adler32(zdict) == dicts(zdict).id


def test_dictionary_id_in_the_zlib_header(ctx, ffi, torch, dicts):
    for zdict in (TEXT[:40000], b"", b"a"):
        z = encode(ctx, ffi, torch, ffi.ZLIB, dicts(zdict), b"hello hello hello")
        assert z[1] & 0x20 and (z[0] * 256 + z[1]) % 31 == 0 and z[2:6] == zlib.adler32(zdict).to_bytes(4, "big")
        assert dm.py_inflate("zlib", z, zdict) == b"hello hello hello"


def test_matches_that_reach_the_dictionary(ctx, ffi, torch, oracle, dicts):
    # a match that starts in the dictionary and runs on into the record, up to the cap of 258
    tail = _rand(200, 77)
    assert dm.primed_codes(D32[:-200] + tail, tail * 3)[0] == (258 << 16) | 200
    check(ctx, ffi, torch, oracle, dicts, D32[:-200] + tail, tail * 3)
    # both straddling prefixes as candidates
    check(ctx, ffi, torch, oracle, dicts, b"..xyzab", b"cabcab..")
    check(ctx, ffi, torch, oracle, dicts, b"..xyza", b"bcQabcR..")
    check(ctx, ffi, torch, oracle, dicts, b"xyaa", b"a" * 10)
    # a run behind a dictionary that ends in its byte: distance 1 at position 0
    assert dm.primed_codes(D32 + b"a", b"a" * 600)[0] == (258 << 16) | 1
    check(ctx, ffi, torch, oracle, dicts, D32 + b"a", b"a" * 600)
    # an occurrence inside the record shadows the dictionary's
    check(ctx, ffi, torch, oracle, dicts, D32, b"QQtimestampQQ" + D32[100:140] + b"  " + D32[100:140] + D32[5000:5100])


def test_distance_32768_and_32769(ctx, ffi, torch, oracle, dicts):
    base = bytes(range(33, 123)) * 400
    T2 = b"@#$%" + base[:32764]
    assert dm.primed_codes(T2, b"@#$%^&")[0] == (4 << 16) | 32768
    check(ctx, ffi, torch, oracle, dicts, T2, b"@#$%^&")                       # exactly 32768: accepted
    check(ctx, ffi, torch, oracle, dicts, T2, b"@#$%")
    T3 = b"@#$%" + base[:32000] + b"@#$%" + base[:760]
    assert dm.primed_codes(T2, b"~@#$%^&")[1] == ord("@") << 16
    check(ctx, ffi, torch, oracle, dicts, T2, b"~@#$%^&")                      # 32769: a literal
    # ... also when the dictionary holds the prefix a second time, in front of the tail (an occurrence older than the most
    # recent one is farther still: the reference tries none, and neither may the table)
    check(ctx, ffi, torch, oracle, dicts, b"@#$%" + base[:5000] + T2, b"~@#$%^&")
    assert dm.primed_codes(T3, b"~@#$%^&")[1] & 0xFFFF == 765
    check(ctx, ffi, torch, oracle, dicts, T3, b"~@#$%^&")                      # a more recent occurrence in reach: a match


@pytest.mark.parametrize("kw", [dict(window_size=1024), dict(max_length=16), dict(no_compression=1), dict(lz77_kind=1),
                                dict(dynamic_huffman=0), dict(block_size=1000)],
                         ids=["window1024", "max16", "stored", "lz77_none", "fixed", "block1000"])
def test_options(ctx, ffi, torch, oracle, dicts, kw):
    rec = D32[-700:] + TEXT[42000:44000] + D32[30000:31500] + D32[:300]
    check(ctx, ffi, torch, oracle, dicts, D32, rec, **kw)


def test_one_chunk_of_100k(ctx, ffi, torch, oracle, dicts):
    """a single write_all: one chunk, longer than a parse workgroup's 39936 positions and longer than the window"""
    data = D32[-3000:] + _text(30 * KIB, 61) + D32[2000:30000] + _text(100 * KIB - 3000 - 30 * KIB - 28000, 62)
    assert len(data) == 100 * KIB
    check(ctx, ffi, torch, oracle, dicts, D32, data)
    mixed = D32[-100:] + _rand(50000, 63, alphabet=3) + D32[:20000] + b"a" * (100 * KIB - 70100)
    check(ctx, ffi, torch, oracle, dicts, D32, mixed)


def test_three_chunks_only_the_first_primed(ctx, ffi, torch, oracle, dicts):
    """600 KiB through 8 KiB writes: chunks of 256 KiB, 256 KiB and 88 KiB"""
    data = D32[-5000:] + _text(600 * KIB - 5000 - 32768, 64) + D32
    check(ctx, ffi, torch, oracle, dicts, D32, data, write_size=8192)


def test_first_generation_match_kernel(lfx, ffi, torch, oracle, dicts):
    c = context_with(lfx, LFX_MATCH_V1="1")
    check(c, ffi, torch, oracle, dicts, D32, D32[-700:] + TEXT[42000:44000] + D32[30000:31500])
    check(c, ffi, torch, oracle, dicts, b"..xyzab", b"cabcab..")
    check(c, ffi, torch, oracle, dicts, D32, D32[-3000:] + _text(50 * KIB, 65) + D32[:9000])
    assert c.match_fallbacks() == 0


def _batch(c, ffi, torch, fmt, zd, recs, caps=None, plain=False):
    L = ffi.lib()
    opts = ffi.make_opts()
    offs, pos = [], 0
    for r in recs:
        offs.append(pos)
        pos += len(r)
    if caps is None:
        caps = [(L.lfx_encode_dict_bound(len(r), C.byref(opts), None) + 3) & ~3 for r in recs]
    out_offs, pos = [], 0
    for cap in caps:
        out_offs.append(pos)
        pos += cap
    d_in = _dev(torch, b"".join(recs))
    d_out = torch.full((pos + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    if plain:
        k = len(recs)
        a = lambda v: (C.c_uint64 * k)(*v)
        ol, st = (C.c_uint64 * k)(), (C.c_int32 * k)()
        rc = L.lfx_encode_batch_device(c.handle, fmt, C.byref(opts), None, k, d_in.data_ptr(), a(offs), a([len(r) for r in recs]),
                                       d_out.data_ptr(), a(out_offs), a(caps), ol, st)
        res = [(st[i], ol[i]) for i in range(k)]
    else:
        rc, res = c.encode_batch_dict_device(fmt, zd, d_in.data_ptr(), offs, [len(r) for r in recs], d_out.data_ptr(), out_offs, caps, opts)
    whole = d_out.cpu().numpy().tobytes()
    assert whole[pos:] == b"\xA5" * GUARD
    return rc, res, whole[:pos], out_offs


def test_batch_of_64_records(ctx, ffi, torch, oracle, dicts):
    rng = random.Random(5)
    lens = [0, 3000, 1, 2, 3, 4, 5] + [rng.randrange(6, 3000) for _ in range(57)]
    recs = []
    for i, n in enumerate(lens):
        a = rng.randrange(0, 30000)
        recs.append((D32[a:a + n // 2] + _text(n, 70 + i))[:n])
    assert len(recs) == 64 and recs[0] == b"" and len(recs[1]) == 3000
    zd = dicts(D32)
    for name, fmt in (("zlib", ffi.ZLIB), ("deflate", ffi.DEFLATE)):
        rc, res, whole, out_offs = _batch(ctx, ffi, torch, fmt, zd, recs)
        assert rc == ffi.OK
        for r, (st, ol), off in zip(recs, res, out_offs):
            z = whole[off:off + ol]
            assert st == ffi.OK and z == encode(ctx, ffi, torch, fmt, zd, r), (name, len(r))        # each equals its one-shot call
            assert z == dm.expected_stream(oracle, name, D32, r), (name, len(r))
            assert dm.py_inflate(name, z, D32) == r
    # one capacity too small: the plain call's LFX_E_NOSPACE pattern
    L = ffi.lib()
    opts = ffi.make_opts()
    caps = [(L.lfx_encode_dict_bound(len(r), C.byref(opts), None) + 3) & ~3 for r in recs]
    caps[1] = 64
    rc, res, whole, _ = _batch(ctx, ffi, torch, ffi.ZLIB, zd, recs, caps)
    prc, pres, pwhole, _ = _batch(ctx, ffi, torch, ffi.ZLIB, None, recs, caps, plain=True)
    assert (rc, res) == (prc, pres) and rc == ffi.E_NOSPACE
    assert [st for st, _ in res] == [ffi.E_NOSPACE if i == 1 else ffi.OK for i in range(64)] and all(ol == 0 for _, ol in res)
    assert whole == pwhole == bytes(len(whole))                     # the span is zero-filled, nothing else is written


def test_without_a_dictionary_and_gzip(lfx, ctx, ffi, torch, oracle, dicts):
    data = TEXT[1000:9000]
    for fmt in (ffi.ZLIB, ffi.DEFLATE):
        assert encode(ctx, ffi, torch, fmt, None, data, 8192) == ctx.encode_host(fmt, data, ffi.make_opts(), ffi.make_schedule(8192)) \
            == oracle.encode(fmt, data, write_size=8192)
        assert ctx.encode_dict_host(fmt, None, data) == oracle.encode(fmt, data)
    rc, res, whole, out_offs = _batch(ctx, ffi, torch, ffi.ZLIB, None, [data, b"", data[:10]])
    assert rc == ffi.OK and [whole[o:o + ol] for (st, ol), o in zip(res, out_offs)] == [oracle.encode(oracle.ZLIB, r) for r in (data, b"", data[:10])]
    for zd in (None, dicts(D32)):
        with pytest.raises(ffi.LfxError) as e:
            encode(ctx, ffi, torch, ffi.GZIP, zd, data)
        assert e.value.status == ffi.E_ARG
        with pytest.raises(ffi.LfxError) as e:
            ctx.encode_dict_host(ffi.GZIP, zd, data)
        assert e.value.status == ffi.E_ARG
        with pytest.raises(ffi.LfxError) as e:
            _batch(ctx, ffi, torch, ffi.GZIP, zd, [data])
        assert e.value.status == ffi.E_ARG
    other = lfx.Context(0)                                          # a dictionary of another context
    with pytest.raises(ffi.LfxError) as e:
        encode(other, ffi, torch, ffi.ZLIB, dicts(D32), data)
    assert e.value.status == ffi.E_ARG


def test_host_call_and_module_helpers(lfx, ctx, ffi, oracle, dicts):
    data = D32[-400:] + TEXT[33000:36000]
    for name, fmt, mod in (("zlib", ffi.ZLIB, lfx.zlib), ("deflate", ffi.DEFLATE, lfx.deflate)):
        want = dm.expected_stream(oracle, name, D32, data)
        assert ctx.encode_dict_host(fmt, dicts(D32), data) == want
        assert mod.compress(data, zdict=D32, context=ctx) == want
        assert mod.compress(data, zdict=dicts(D32), context=ctx) == want
        assert mod.compress(data, context=ctx) == oracle.encode(fmt, data)
        assert mod.compress(data, zdict=D32, options=mod.EncodeOptions().fixed_huffman_codes(), context=ctx) == \
            dm.expected_stream(oracle, name, D32, data, dynamic_huffman=0)
