"""GPU: LFX_LZ77_CHAIN and LFX_LZ77_LAZY through a chain dictionary (include/lfx.h "a chain dictionary") by the
one-shot calls, the host call, the batch call and the module helpers.  Every case compares bytes, zlib and raw DEFLATE, with
the stream the contract implies (tests/dict_chain_model.py: the oracle's generic encoder over the model's code words;
test_dict_chain_model.py proves the model on the CPU), and every output is read back by python-zlib and by
lfx_decode_dict_host.  Integer work: every comparison is exact.  Every case is a few KiB but the ones that need a tile seam of
the chain kernel (16384 positions) or the end of the dictionary's reach (32768)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import dict_chain_model as dcm
import dict_encode_model as dm
import lazy_model as lm
from test_dict_encode_model import _rand, _text
from test_gpu_encode_stages import context_with
from test_gpu_parity import ctx, ffi, lfx  # noqa: F401  (fixtures)

KIB = 1 << 10
GUARD = 64
TEXT = _text(48 * KIB, 81)
D32 = TEXT[:32768]
KINDS = (dcm.CHAIN, dcm.LAZY)
FMTS = (("deflate", 0), ("zlib", 1))


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def _dev(torch, data):
    a = np.frombuffer(bytes(data), dtype=np.uint8).copy() if len(data) else np.zeros(4, dtype=np.uint8)
    return torch.from_numpy(a).to("cuda")


@pytest.fixture(scope="module")
def dicts(lfx, ctx):
    """one Dictionary per distinct dictionary, kind of object and context, made once"""
    made = {}

    def get(zdict, c=ctx, chain=True):
        key = (zdict, id(c), chain)
        if key not in made:
            made[key] = lfx.Dictionary(zdict, c, chain=chain)
        return made[key]
    yield get
    for d in made.values():
        d.close()


def encode(c, ffi, torch, fmt, zd, data, kind, depth, write_size=0, writes=None, **kw):
    """lfx_encode_dict_device on device buffers, a guard behind the capacity → the stream"""
    opts, sched = ffi.make_opts(lz77_kind=kind | depth << 8, **kw), ffi.make_schedule(write_size, writes)
    cap = (ffi.lib().lfx_encode_dict_bound(len(data), C.byref(opts), C.byref(sched)) + 3) & ~3
    d_in = _dev(torch, data)
    d_out = torch.full((cap + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    n = c.encode_dict_device(fmt, zd, d_in.data_ptr(), len(data), d_out.data_ptr(), cap, opts, sched)
    whole = d_out.cpu().numpy().tobytes()
    assert whole[cap:] == b"\xA5" * GUARD, "bytes behind cap were written"
    return whole[:n]


def check(c, ffi, torch, oracle, dicts, zdict, data, depths=(8,), kinds=KINDS, write_size=0, writes=None, **kw):
    """both formats: bytes equal to the expected stream; python-zlib and lfx_decode_dict_host read them back"""
    zd = dicts(zdict, c)
    for kind in kinds:
        for depth in depths:
            for name, fmt in FMTS:
                got = encode(c, ffi, torch, fmt, zd, data, kind, depth, write_size, writes, **kw)
                want = dcm.expected_stream(oracle, name, zdict, data, kind, depth, write_size, writes=writes, **kw)
                assert got == want, (name, kind, depth, len(zdict), len(data), kw, len(got), len(want))
                assert dcm.py_inflate(name, got, zdict) == data
                rc, out, used, msg = c.decode_dict_host(fmt, zd, got, cap=max(len(data), 4))
                assert (rc, out, used) == (ffi.OK, data, len(got)), (name, rc, used, msg)


def first_pointer(T, buf, kind, depth, at, **kw):
    """the model's code word at chunk position `at` (asserted to begin one) → (length, distance)"""
    pos = 0
    for c in dcm.primed_codes(T, buf, kind, depth, **kw):
        if pos == at:
            return c >> 16 if c & 0xFFFF else 1, c & 0xFFFF
        pos += (c >> 16) if c & 0xFFFF else 1
    raise AssertionError("no code word begins at %d" % at)


# ---- formats, kinds, depths, dictionary lengths
@pytest.mark.parametrize("depth", [1, 8, 255])
def test_depths(ctx, ffi, torch, oracle, dicts, depth):
    rec = D32[-300:] + TEXT[40000:41500] + D32[9000:9400] + D32[:200] + b"a" * 300
    check(ctx, ffi, torch, oracle, dicts, D32, rec, depths=(depth,))


@pytest.mark.parametrize("m", [0, 1, 2, 3, 5, 1001, 32767, 32768, 40000])
def test_dictionary_lengths(ctx, ffi, torch, oracle, dicts, m):
    """32768: the whole window; 40000: the tail counts and the id covers all bytes; 1001 and 32767: the tail begins off the
    dword grid of the dictionary's window"""
    zdict = TEXT[:m]
    rec = zdict[-300:] + TEXT[41000:41300] + zdict[:200] + zdict[-32768:][:64] + TEXT[41000:41100]
    check(ctx, ffi, torch, oracle, dicts, zdict, rec)
    check(ctx, ffi, torch, oracle, dicts, zdict, zdict[-2:] + zdict[-5:] * 3 + b"xyz")


def test_straddling_positions(ctx, ffi, torch, oracle, dicts):
    # T ends "ab", the chunk begins "cabcabc": the candidate at |T|-2
    assert first_pointer(b"..xyzab", b"cabcabc..", dcm.CHAIN, 8, 1) == (6, 3)
    check(ctx, ffi, torch, oracle, dicts, b"..xyzab", b"cabcabc..", depths=(1, 8))
    check(ctx, ffi, torch, oracle, dicts, b"..xyza", b"bcQabcR..", depths=(1, 8))
    # the chain runs |T|-1 → |T|-2 → the table → the dictionary's own chain
    assert first_pointer(b"a" * 100, b"a" * 600, dcm.CHAIN, 8, 0) == (258, 1)
    check(ctx, ffi, torch, oracle, dicts, b"a" * 100, b"a" * 600, depths=(1, 2, 3, 8, 255))
    check(ctx, ffi, torch, oracle, dicts, b"xyaa", b"a" * 10, depths=(1, 2, 8))
    # |T|-1 and |T|-2 with different prefixes, both with older occurrences in the dictionary: "bca" and "abc" + longer tails
    T = b"..bcaQRSTUVW..abcaQRST..ab"
    check(ctx, ffi, torch, oracle, dicts, T, b"caQRSTUVWX--bcaQRSTUVW", depths=(1, 2, 8))
    check(ctx, ffi, torch, oracle, dicts, b"ab", b"abababab", depths=(1, 8))
    check(ctx, ffi, torch, oracle, dicts, b"a", b"aaaaaaaa", depths=(1, 8))


def test_choosing_the_winner(ctx, ffi, torch, oracle, dicts):
    # an older dictionary occurrence that matches longer than a younger one: it wins at depth 2 and not at depth 1
    T = b"0123456789abcdefgh" + b"#" * 40 + b"0123456789zzz" + b"#" * 40
    rec = b"0123456789abcdefgh!"
    assert first_pointer(T, rec, dcm.CHAIN, 1, 0) == (10, 53) and first_pointer(T, rec, dcm.CHAIN, 2, 0) == (18, 111)
    check(ctx, ffi, torch, oracle, dicts, T, rec, depths=(1, 2))
    # an in-chunk and a dictionary candidate of equal length: the in-chunk (nearer) one wins
    assert first_pointer(b"..QRSTUV..", b"QRSTUV--QRSTUV++", dcm.CHAIN, 8, 8) == (6, 8)
    check(ctx, ffi, torch, oracle, dicts, b"..QRSTUV..", b"QRSTUV--QRSTUV++")
    # K - 1 in-chunk candidates followed by dictionary ones: the depth count runs on across the boundary
    T = b"..XYZabcdefgh..XYZabcd..XYZab.."
    rec = b"XYZa1XYZa2XYZabcdefgh!"
    assert [first_pointer(T, rec, dcm.CHAIN, k, 10)[0] for k in (2, 3, 4, 5)] == [4, 5, 7, 11]
    check(ctx, ffi, torch, oracle, dicts, T, rec, depths=(2, 3, 4, 5))


def test_window_and_length_limits(ctx, ffi, torch, oracle, dicts):
    # window_size 1024: an occurrence at distance 1024 is a candidate, at 1025 none
    base = bytes(range(33, 123)) * 20
    T = b"@#$%^" + base[:1019]
    assert first_pointer(T, b"@#$%^&", dcm.CHAIN, 8, 0, window=1024) == (5, 1024)
    assert first_pointer(T, b"~@#$%^&", dcm.CHAIN, 8, 1, window=1024) == (1, 0)
    check(ctx, ffi, torch, oracle, dicts, T, b"@#$%^&", window_size=1024)
    check(ctx, ffi, torch, oracle, dicts, T, b"~@#$%^&", window_size=1024)
    check(ctx, ffi, torch, oracle, dicts, b"@#$%^" + T, b"~@#$%^&", window_size=1024)      # (an older one in the tail, farther still)
    # a hop whose target is in reach of the candidate q but not of the position p: the walk ends there
    low = bytes(97 + x % 26 for x in _rand(2000, 5))
    T = low[:400] + b"HOPabcdefgh" + low[400:989]                                         # "HOP" 600 bytes in front of the chunk
    rec = low[1000:1100] + b"HOPab" + low[1100:1595] + b"HOPabcdefgh" + low[1600:1700]
    assert len(T) == 1000 and rec[600:603] == b"HOP"
    assert first_pointer(T, rec, dcm.CHAIN, 8, 600, window=1024) == (5, 500) and first_pointer(T, rec, dcm.CHAIN, 8, 600) == (11, 1200)
    check(ctx, ffi, torch, oracle, dicts, T, rec, window_size=1024)
    check(ctx, ffi, torch, oracle, dicts, T, rec)
    # max_length 16 and 3
    rec = D32[-700:] + TEXT[42000:43000] + D32[30000:30500] + b"a" * 100
    check(ctx, ffi, torch, oracle, dicts, D32, rec, max_length=16)
    check(ctx, ffi, torch, oracle, dicts, D32, rec, max_length=3)
    check(ctx, ffi, torch, oracle, dicts, D32, rec, window_size=1024, depths=(255,))
    # a match that starts in T and runs to the end of a 5-byte chunk
    assert dcm.primed_codes(b"..hello", b"hello", dcm.CHAIN, 8) == [(5 << 16) | 5]
    check(ctx, ffi, torch, oracle, dicts, b"..hello", b"hello")
    for n in range(5):
        check(ctx, ffi, torch, oracle, dicts, D32, D32[-5:][:n])


@pytest.mark.parametrize("cut", [0, 1])
def test_tile_seams(ctx, ffi, torch, oracle, dicts, cut):
    """the second tile of a primed chunk (positions from 16384 on) still reaches the dictionary; a position from 32768 on
    reaches none of it.  cut: the same chunks one byte shorter"""
    noise = _rand(40000, 91)
    DN = D32[:20000] + _rand(12768, 92)                               # (a tail no text repeats: the copy is the only candidate)
    rec = noise[:16384] + DN[-8000:-7300 - cut]
    assert len(rec) == 16384 + 700 - cut
    ln, dist = first_pointer(DN, rec, dcm.CHAIN, 8, 16384)
    assert ln == 258 and dist == 16384 + 8000                         # into the dictionary, from the second tile
    check(ctx, ffi, torch, oracle, dicts, DN, rec)
    rec = noise[:32768] + DN[-300:-68 - cut]
    assert len(rec) == 33000 - cut and first_pointer(DN, rec, dcm.CHAIN, 8, 32768) == (1, 0)    # 33068 away: a literal
    check(ctx, ffi, torch, oracle, dicts, DN, rec)
    rec = noise[:32700] + DN[-60:] + noise[32700:32940 - cut]         # the last positions that reach T's last bytes
    assert first_pointer(DN, rec, dcm.CHAIN, 8, 32700) == (60, 32760)
    check(ctx, ffi, torch, oracle, dicts, DN, rec)


def test_lazy_through_the_dictionary(ctx, ffi, torch, oracle, dicts):
    # L(1) > L(0), and L(1) comes from T: position 0 is a literal
    T = b"..abcd....bcdefghij.."
    assert dcm.primed_codes(T, b"abcdefghij!", dcm.LAZY, 8)[:2] == [ord("a") << 16, (9 << 16) | 12]
    check(ctx, ffi, torch, oracle, dicts, T, b"abcdefghij!", depths=(1, 8))
    # a rising run that starts at position 0
    T = b"abc1....bcde2....cdefg3....defghij4...."
    got = dcm.primed_codes(T, b"abcdefghij!!", dcm.LAZY, 8)
    assert [c & 0xFFFF for c in got[:4]] == [0, 0, 0, 15] and got[3] >> 16 == 7
    check(ctx, ffi, torch, oracle, dicts, T, b"abcdefghij!!", depths=(1, 8))


def test_second_chunk_is_not_primed(ctx, ffi, torch, oracle, dicts):
    """two write events: the chunk behind the primed one is parsed as it is without a dictionary"""
    data = D32[-600:] + TEXT[40000:42000] + D32[5000:5600] + TEXT[40000:41000]
    check(ctx, ffi, torch, oracle, dicts, D32, data, writes=[2600, None, len(data) - 2600])


def _batch(c, ffi, torch, fmt, zd, recs, kind, depth, gaps):
    L = ffi.lib()
    opts = ffi.make_opts(lz77_kind=kind | depth << 8)
    caps = [(L.lfx_encode_dict_bound(len(r), C.byref(opts), None) + 3) & ~3 for r in recs]
    blob, offs = b"", []
    for g, r in zip(gaps, recs):
        blob += b"\xEE" * g
        offs.append(len(blob))
        blob += r
    out_offs = [sum(caps[:i]) for i in range(len(recs))]
    d_in = _dev(torch, blob)
    d_out = torch.full((sum(caps) + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    rc, res = c.encode_batch_dict_device(fmt, zd, d_in.data_ptr(), offs, [len(r) for r in recs], d_out.data_ptr(), out_offs, caps, opts)
    whole = d_out.cpu().numpy().tobytes()
    assert rc == ffi.OK and whole[sum(caps):] == b"\xA5" * GUARD
    return [whole[o:o + ol] for (st, ol), o in zip(res, out_offs) if st == ffi.OK]


@pytest.mark.parametrize("kind", KINDS)
def test_batch(ctx, ffi, torch, oracle, dicts, kind):
    """records of 0..5 bytes, 1 KiB and exactly 8192 bytes behind one dictionary, at odd offsets (every phase of the byte and
    of the candidate grid); a record whose only matches are in T; records that begin with the straddling prefixes"""
    only_t = D32[100:300] + D32[9000:9200] + D32[-150:]
    recs = [D32[-5:][:n] for n in range(6)] + [TEXT[40000:41024], (D32[-3000:] + TEXT[41000:47000])[:8192], only_t,
                                               D32[-1:] * 2 + D32[-2:] * 3 + b"!", D32[-2:] + D32[-2:] + D32[-7:], TEXT[44000:45001]]
    assert len(recs[7]) == 8192
    gaps = [1, 0, 3, 0, 1, 2, 1, 3, 2, 1, 3, 0]
    zd = dicts(D32)
    for name, fmt in FMTS:
        got = _batch(ctx, ffi, torch, fmt, zd, recs, kind, 8, gaps)
        assert len(got) == len(recs)
        for r, z in zip(recs, got):
            assert z == dcm.expected_stream(oracle, name, D32, r, kind, 8), (name, len(r))
            assert dcm.py_inflate(name, z, D32) == r
            rc, out, used, msg = ctx.decode_dict_host(fmt, zd, z, cap=max(len(r), 4))
            assert (rc, out, used) == (ffi.OK, r, len(z)), (name, rc, msg)


def test_nothing_of_a_call_stays(ctx, ffi, torch, oracle, dicts):
    """a chained dictionary call, kind 0 with the same dictionary (§18's bytes), a dictionary-less lazy call (§20's bytes), and
    the other order; one chain dictionary under two window sizes"""
    rec = D32[-400:] + TEXT[33000:35000] + D32[2000:2300]
    zd = dicts(D32)
    want0 = dm.expected_stream(oracle, "zlib", D32, rec)
    want3 = lm.expected_stream(oracle, 1, rec, 8)
    wantd = dcm.expected_stream(oracle, "zlib", D32, rec, dcm.LAZY, 8)
    for _ in range(2):
        assert encode(ctx, ffi, torch, ffi.ZLIB, zd, rec, dcm.LAZY, 8) == wantd
        assert ctx.encode_dict_host(ffi.ZLIB, zd, rec) == want0
        assert ctx.encode_host(ffi.ZLIB, rec, ffi.make_opts(lz77_kind=ffi.LZ77_LAZY | 8 << 8)) == want3
        assert ctx.encode_dict_host(ffi.ZLIB, zd, rec) == want0
        assert encode(ctx, ffi, torch, ffi.ZLIB, zd, rec, dcm.LAZY, 8) == wantd
    for w in (1024, 32768, 4096):
        assert encode(ctx, ffi, torch, ffi.ZLIB, zd, rec, dcm.CHAIN, 8, window_size=w) == \
            dcm.expected_stream(oracle, "zlib", D32, rec, dcm.CHAIN, 8, window_size=w)
    # for the kinds 0 and 1 and for the decode calls a chain dictionary is a plain one
    plain = dicts(D32, chain=False)
    assert ctx.encode_dict_host(ffi.ZLIB, plain, rec) == want0 and zd.id == plain.id
    assert ctx.decode_dict_host(ffi.ZLIB, plain, wantd)[1] == rec


def test_plain_dictionary_keeps_refusing(lfx, ctx, ffi, torch, dicts):
    plain = dicts(D32, chain=False)
    for kind, word in ((ffi.LZ77_CHAIN, "CHAIN"), (ffi.LZ77_LAZY, "LAZY")):
        with pytest.raises(ffi.LfxError) as e:
            ctx.encode_dict_host(ffi.ZLIB, plain, b"hello hello hello", ffi.make_opts(lz77_kind=kind | 8 << 8))
        assert e.value.status == ffi.E_UNSUPPORTED and "dictionary" in e.value.message and word in e.value.message
        with pytest.raises(ffi.LfxError) as e:
            lfx.zlib.compress(b"hello hello hello", zdict=plain, lz77=lfx.lz77.LazyLz77Encoder(8), context=ctx)
        assert e.value.status == ffi.E_UNSUPPORTED
    with pytest.raises(ffi.LfxError) as e:                                   # gzip has no preset dictionary
        encode(ctx, ffi, torch, ffi.GZIP, dicts(D32), b"hello hello hello", dcm.LAZY, 8)
    assert e.value.status == ffi.E_ARG


def test_host_call_and_module_helpers(lfx, ctx, ffi, oracle, dicts):
    data = D32[-400:] + TEXT[33000:36000]
    for name, fmt, mod in (("zlib", ffi.ZLIB, lfx.zlib), ("deflate", ffi.DEFLATE, lfx.deflate)):
        for kind, enc in ((dcm.CHAIN, lfx.lz77.ChainLz77Encoder(8)), (dcm.LAZY, lfx.lz77.LazyLz77Encoder(8))):
            want = dcm.expected_stream(oracle, name, D32, data, kind, 8)
            assert ctx.encode_dict_host(fmt, dicts(D32), data, ffi.make_opts(lz77_kind=kind | 8 << 8)) == want
            assert mod.compress(data, zdict=D32, lz77=enc, context=ctx) == want          # (bytes: a chain dictionary is made)
            assert mod.compress(data, zdict=dicts(D32), lz77=enc, context=ctx) == want
        assert mod.compress(data, zdict=D32, context=ctx) == dm.expected_stream(oracle, name, D32, data)


@pytest.mark.parametrize("env", ["LFX_MATCH_V1"])
def test_match_generations(lfx, ffi, torch, oracle, dicts, env):
    c = context_with(lfx, **{env: "1"})
    check(c, ffi, torch, oracle, dicts, D32, D32[-700:] + TEXT[42000:44000] + D32[30000:31500] + b"a" * 300)
    check(c, ffi, torch, oracle, dicts, b"a" * 100, b"a" * 600, depths=(3,))
