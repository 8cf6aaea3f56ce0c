"""GPU: CostLz77Encoder (LFX_LZ77_COST, include/lfx.h) through every entry point that serves it.  Every case
compares bytes with the stream the contract implies (tests/cost_model.py: the oracle's generic encoder over the model's code
words, the first pass included; test_cost_model.py proves the model on the CPU), python-zlib inflates it and lfx_decode_device
decodes it back.  Integer work: every comparison is exact.

What the cost kernel adds (lfx_cost.hip): one lane per segment of COST_SEG positions with COST_WARM of warm-up, slabs of 32
positions, a table per lane — so the sizes are those around a segment's end and around a warm-up's, chunks of one lane and of
sixty-four, a batch whose lanes belong to different blocks, and a second parse behind the first on scratch that other kinds
left behind."""
import ctypes as C
import gzip as pygzip
import io
import zlib

import pytest

pytestmark = pytest.mark.gpu

import auto_block_model as abm
import chain_model as cm
import cost_model as km
import lazy_model as lm
import level_model as vm
import merge_model
from test_dict_encode_model import _rand, _text
from test_gpu_batch_packed import packed
from test_gpu_chain_encode import _dev, inflate, roundtrip
from test_gpu_encode_stages import context_with
from test_gpu_parity import ctx, ffi, lfx  # noqa: F401  (fixtures)
from test_level_model import MIXED, lazy_case, put

KIB = 1 << 10
GUARD = 64
SEG, WARM = km.COST_SEG, km.COST_WARM
FMT_NAMES = {0: "deflate", 1: "zlib", 2: "gzip"}
TEXT = _text(24 * KIB, 77)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def cost(ffi, n):
    return ffi.LZ77_COST | n << 8               # LFX_LZ77_COST_N(n)


def encode(c, ffi, torch, fmt, data, kind, write_size=0, writes=None, **kw):
    """lfx_encode_device with lz77_kind = kind on device buffers, a guard behind the capacity → the stream"""
    opts, sched = ffi.make_opts(lz77_kind=kind, **kw), ffi.make_schedule(write_size, writes)
    cap = (ffi.lib().lfx_encode_bound(len(data), C.byref(opts), C.byref(sched)) + 3) & ~3
    assert cap
    d_in = _dev(torch, data)
    d_out = torch.full((cap + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    n = c.encode_device(fmt, d_in.data_ptr(), len(data), d_out.data_ptr(), cap, opts, sched)
    whole = d_out.cpu().numpy().tobytes()
    assert whole[cap:] == b"\xA5" * GUARD, "bytes behind cap were written"
    return whole[:n]


def check(c, ffi, torch, oracle, data, lvl, fmts=(0,), write_size=0, **kw):
    out = {}
    for fmt in fmts:
        got = encode(c, ffi, torch, fmt, data, cost(ffi, lvl), write_size, **kw)
        want = km.expected_stream(oracle, fmt, data, lvl, write_size, **kw)
        assert got == want, (fmt, len(data), lvl, kw, len(got), len(want))
        assert inflate(fmt, got) == data
        roundtrip(c, ffi, torch, fmt, got, data)
        out[fmt] = got
    return out


# ---------------------------------------------------------------------------------------------- formats, levels, codes
@pytest.mark.parametrize("lvl", [1, 6, 9])
def test_formats_and_levels(ctx, ffi, torch, oracle, lvl):
    data = MIXED[:3 * KIB]
    for kw in ({}, {"dynamic_huffman": 0}):
        z = check(ctx, ffi, torch, oracle, data, lvl, fmts=(0, 1, 2), **kw)
        assert z[1][1] >> 6 == 3 and z[2][8] == 2                     # Best: FLEVEL 3, XFL 2
        assert z[0] != vm.expected_stream(oracle, 0, data, lvl, **kw)  # not the level's bytes: the cost rule ran
    for n in range(6):
        check(ctx, ffi, torch, oracle, b"abcab"[:n], lvl, fmts=(0, 2))
    check(ctx, ffi, torch, oracle, data, lvl, max_length=16)
    check(ctx, ffi, torch, oracle, data, lvl, max_length=3, window_size=512, fmts=(1,))


@pytest.mark.parametrize("positions", [SEG - 1, SEG, SEG + 1, 2 * SEG + WARM - 1, 2 * SEG + WARM, 2 * SEG + WARM + 1])
def test_segment_and_warm_up_ends(ctx, ffi, torch, oracle, positions):
    """a chunk of that many visited positions (its length - 3): the last segment of one position, the warm-up cut at the end"""
    data = TEXT[:positions + 3]
    check(ctx, ffi, torch, oracle, data, 6)
    check(ctx, ffi, torch, oracle, data, 1, dynamic_huffman=0)


def test_two_chunks_of_256k_behind_stale_lengths(ctx, ffi, torch, oracle):
    """8 KiB writes: two chunks of 256 KiB, 64 lanes each.  The pair at end - 2 / end - 1 of the first: L(end - 1) is capped by
    the chunk's end and nothing at `end` is read — the call in front left lengths of 258 all over the length array"""
    n = 256 * KIB
    stale = b"a" * (2 * n + 100)
    assert inflate(1, encode(ctx, ffi, torch, 1, stale, cost(ffi, 1))) == stale
    hist, tail = lazy_case(3, 9)
    body = _text(n, 78)
    first = body[:n - 5 - len(hist)] + hist + tail[:5]
    assert len(first) == n
    L, _ = vm.level_lengths(first[-4096:], 1)
    assert L[4096 - 5] == 3 and L[4096 - 4] == 4 and L[4096 - 3] == 0
    data = first + _text(n, 79)
    check(ctx, ffi, torch, oracle, data, 1, fmts=(1,), write_size=8192)


# ---------------------------------------------------------------------------------------------- batch, packed batch, dictionary
def test_batch_and_packed_batch(ctx, ffi, torch, oracle):
    """records of 0..5 bytes, of exactly COST_SEG and of COST_SEG + 1 bytes, at odd offsets: every lane another block"""
    recs = [b"", b"a", b"ab", b"abc", b"abca", b"abcab", TEXT[:SEG], TEXT[100:100 + SEG + 1], MIXED[:1 * KIB], MIXED[:3000]]
    gaps = [0, 1, 0, 2, 1, 5, 3, 1, 7, 1]
    L = ffi.lib()
    n = len(recs)
    for fmt, lvl in ((1, 6), (0, 1)):
        opts = ffi.make_opts(lz77_kind=cost(ffi, lvl))
        caps = [(L.lfx_encode_bound(len(r), C.byref(opts), None) + 3) & ~3 for r in recs]
        blob, offs = b"", []
        for g, r in zip(gaps, recs):
            blob += b"\xEE" * g
            offs.append(len(blob))
            blob += r
        out_offs = [sum(caps[:i]) for i in range(n)]
        d_in = _dev(torch, blob)
        d_out = torch.full((sum(caps) + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        a = lambda v: (C.c_uint64 * n)(*v)
        ol, st = (C.c_uint64 * n)(), (C.c_int32 * n)()
        rc = L.lfx_encode_batch_device(ctx.handle, fmt, C.byref(opts), None, n, d_in.data_ptr(), a(offs), a([len(r) for r in recs]),
                                       d_out.data_ptr(), a(out_offs), a(caps), ol, st)
        assert rc == ffi.OK, ctx.last_error()
        whole = d_out.cpu().numpy().tobytes()
        assert whole[sum(caps):] == b"\xA5" * GUARD
        want = [km.expected_stream(oracle, fmt, r, lvl) for r in recs]
        for i, r in enumerate(recs):
            z = whole[out_offs[i]:out_offs[i] + ol[i]]
            assert st[i] == ffi.OK and z == want[i], (fmt, i, len(r), offs[i])
            assert inflate(fmt, z) == r
            roundtrip(ctx, ffi, torch, fmt, z, r)
        rc, total, layout, out, _ = packed(ctx, ffi, torch, fmt, recs, opts)
        assert rc == ffi.OK
        for (off, ln), w, r in zip(layout, want, recs):
            assert out[off:off + ln] == w
            roundtrip(ctx, ffi, torch, fmt, out[off:off + ln], r)


def roundtrip_dict(c, ffi, torch, fmt, zd, z, data):
    """lfx_decode_dict_device back to the input"""
    d_in = _dev(torch, z)
    d_out = torch.full((max(len(data), 4),), 0x5A, dtype=torch.uint8, device="cuda")
    rc, ol, used, msg = c.decode_dict_device(fmt, zd, d_in.data_ptr(), len(z), d_out.data_ptr(), len(data))
    assert (rc, ol, used) == (ffi.OK, len(data), len(z)), (rc, ol, used, msg)
    assert d_out.cpu().numpy().tobytes()[:ol] == data


def test_chain_dictionary(lfx, ctx, ffi, torch, oracle):
    zdict, data = MIXED[3000:8000], MIXED[2500:2500 + KIB]
    zd = lfx.Dictionary(zdict, ctx, chain=True)
    try:
        for fmt in (ffi.ZLIB, ffi.DEFLATE):
            for kw in ({}, {"dynamic_huffman": 0}):
                got = ctx.encode_dict_host(fmt, zd, data, ffi.make_opts(lz77_kind=cost(ffi, 6), **kw))
                assert got == km.expected_dict_stream(oracle, FMT_NAMES[fmt], zdict, data, 6, **kw)
                roundtrip_dict(ctx, ffi, torch, fmt, zd, got, data)
        z = lfx.zlib.compress(data, zdict=zdict, lz77=lfx.lz77.CostLz77Encoder(6), context=ctx)    # bytes: the chain dictionary is made here
        assert z == km.expected_dict_stream(oracle, "zlib", zdict, data, 6)
        roundtrip_dict(ctx, ffi, torch, ffi.ZLIB, zd, z, data)
    finally:
        zd.close()
    dec = zlib.decompressobj(zdict=zdict)
    assert dec.decompress(z) + dec.flush() == data


# ---------------------------------------------------------------------------------------------- entry points
def test_host_call_and_module_helpers(lfx, ctx, ffi, torch, oracle):
    data = MIXED[:5000]
    enc = lfx.lz77.CostLz77Encoder(6)
    assert enc.compression_level() == lfx.lz77.CompressionLevel.BEST and enc.window_size() == 32768
    assert enc._opts()["lz77_kind"] == ffi.LZ77_COST | 6 << 8 == 6 | 6 << 8
    for fmt, mod in ((0, lfx.deflate), (1, lfx.zlib), (2, lfx.gzip)):
        want = km.expected_stream(oracle, fmt, data, 6)
        assert ctx.encode_host(fmt, data, ffi.make_opts(lz77_kind=cost(ffi, 6))) == want
        assert mod.compress(data, lz77=enc, context=ctx) == want
        roundtrip(ctx, ffi, torch, fmt, want, data)


def test_stream_encoder_with_a_flush_inside_a_segment(lfx, ctx, ffi, torch, oracle):
    data = TEXT[:14000]
    writes = [3000, 2000, None, 4096]                  # the flush at 5000: inside the second segment of a buffer that ends there
    for mod, fmt in ((lfx.deflate, 0), (lfx.zlib, 1), (lfx.gzip, 2)):
        sink = io.BytesIO()
        e = mod.Encoder(sink, mod.EncodeOptions(lz77=lfx.lz77.CostLz77Encoder(6)), ctx)
        at = 0
        for w in writes:
            if w is None:
                e.flush()
            else:
                e.write(data[at:at + w])
                at += w
        e.write(data[at:])
        e.finish()
        got = sink.getvalue()
        assert got == km.expected_stream(oracle, fmt, data, 6, writes=writes + [len(data) - at]), fmt
        assert inflate(fmt, got) == data
        roundtrip(ctx, ffi, torch, fmt, got, data)


@pytest.mark.parametrize("bgzf", [False, True], ids=["plain", "bgzf"])
def test_members_of_8k(lfx, ctx, ffi, torch, oracle, bgzf):
    data = TEXT[:20000]
    out, members = lfx.gzip.encode_members(data, 8192, bgzf=bgzf, lz77=lfx.lz77.CostLz77Encoder(6), context=ctx)
    assert pygzip.decompress(out) == data and len(members) == 3
    for in_off, in_len, out_off, out_len in members:
        piece = data[in_off:in_off + in_len]
        kw = {"extra": bytes([0x42, 0x43, 2, 0]) + (out_len - 1).to_bytes(2, "little")} if bgzf else {}
        assert out[out_off:out_off + out_len] == km.expected_stream(oracle, 2, piece, 6, **kw), (in_off, bgzf)
        roundtrip(ctx, ffi, torch, 2, out[out_off:out_off + out_len], piece)
    d_in = _dev(torch, out)
    d_out = torch.full((len(data),), 0x5A, dtype=torch.uint8, device="cuda")
    rc, ol, used, found, msg = ctx.decode_members_device(d_in.data_ptr(), len(out), d_out.data_ptr(), len(data))
    assert (rc, ol, used, len(found)) == (ffi.OK, len(data), len(out), 3 + bgzf), msg     # (BGZF: the empty block that ends the file)
    assert d_out.cpu().numpy().tobytes() == data


def test_auto_huffman_and_merge_blocks_on_top(ctx, ffi, torch, oracle):
    data = MIXED[:6000] + _rand(3000, 71) + b"\x00" * 2000
    for fmt in (0, 1):
        # the `= 0` stream the AUTO model splices from: the call's code words — chosen under the first pass' code — in fixed codes
        src = lambda f, d, write_size=0, **kw: km.expected_stream(oracle, fmt, d, 6, write_size, cost_first_pass=True, **kw)
        want = abm.expected(oracle, FMT_NAMES[fmt], data, block_size=2048, write_size=1024, encode=src)[0]
        got = encode(ctx, ffi, torch, fmt, data, cost(ffi, 6), write_size=1024, dynamic_huffman=2, block_size=2048)
        assert got == want and inflate(fmt, got) == data
        roundtrip(ctx, ffi, torch, fmt, got, data)
        plain = encode(ctx, ffi, torch, fmt, data, cost(ffi, 6), write_size=1024, block_size=2048)
        assert got != plain
        base = km.expected_stream(oracle, fmt, data, 6, 1024, block_size=2048)
        assert plain == base
        merged = encode(ctx, ffi, torch, fmt, data, cost(ffi, 6), write_size=1024, block_size=2048, block_merge=1)
        assert merged == merge_model.expected(oracle, FMT_NAMES[fmt], base, data, None, False)[0]
        assert inflate(fmt, merged) == data and len(merged) <= len(plain)
        roundtrip(ctx, ffi, torch, fmt, merged, data)


# ---------------------------------------------------------------------------------------------- stale state, match generations
def test_stale_state_in_both_orders(lfx, ctx, ffi, torch, oracle):
    """a cost call behind the kinds 0, 3 and 4 and each of them behind a cost call, on one context: the bytes of the models"""
    data = put(*lazy_case(16, 22), at=9000, total=12000)[0]
    want = {"cost": km.expected_stream(oracle, 1, data, 6), 0: oracle.encode(oracle.ZLIB, data),
            3: lm.expected_stream(oracle, 1, data, 8), 4: vm.expected_stream(oracle, 1, data, 6)}
    run = {"cost": lambda: encode(ctx, ffi, torch, 1, data, cost(ffi, 6)), 0: lambda: ctx.encode_host(ffi.ZLIB, data),
           3: lambda: encode(ctx, ffi, torch, 1, data, ffi.LZ77_LAZY | 8 << 8), 4: lambda: encode(ctx, ffi, torch, 1, data, ffi.LZ77_LEVEL | 6 << 8)}
    for other in (0, 3, 4):
        for order in (("cost", other), (other, "cost"), ("cost", "cost")):
            for k in order:
                assert run[k]() == want[k], (order, k)
    check(ctx, ffi, torch, oracle, data[:5000], 6)                       # a cost call on a shorter input
    check(ctx, ffi, torch, oracle, data, 6, dynamic_huffman=0)           # ... and one without a first pass


def test_older_match_generations(lfx, ffi, torch, oracle):
    data = MIXED[:6000]
    check(context_with(lfx, LFX_MATCH_V1="1"), ffi, torch, oracle, data, 6, fmts=(1,))


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals(lfx, ctx, ffi, torch):
    data = MIXED[:5000]
    for bad in (5, 5 | 6 << 8, cost(ffi, 0), cost(ffi, 10), cost(ffi, 255), cost(ffi, 6) | 1 << 16, cost(ffi, 6) | 1 << 30):
        with pytest.raises(ffi.LfxError) as e:
            ctx.encode_host(ffi.ZLIB, data, ffi.make_opts(lz77_kind=bad))
        assert e.value.status == ffi.E_ARG
    zd = lfx.Dictionary(MIXED[5000:9000], ctx)
    try:
        with pytest.raises(ffi.LfxError) as e:
            ctx.encode_dict_host(ffi.ZLIB, zd, data, ffi.make_opts(lz77_kind=cost(ffi, 6)))
        assert e.value.status == ffi.E_UNSUPPORTED and "dictionary" in e.value.message and "LFX_LZ77_COST" in e.value.message
    finally:
        zd.close()
    info = ffi.ShardInfo()
    d_in = _dev(torch, data)
    opts = ffi.make_opts(lz77_kind=cost(ffi, 6))
    rc = ffi.lib().lfx_encode_shard_prepare(ctx.handle, ffi.ZLIB, C.byref(opts), None, d_in.data_ptr(), len(data), 1, 1, C.byref(info))
    assert rc == ffi.E_UNSUPPORTED and "LFX_LZ77_COST" in ctx.last_error()
    with pytest.raises(ffi.LfxError) as e:
        lfx.Index.encode(data, "gzip", spacing=4 * KIB, ctx=ctx, lz77=lfx.lz77.CostLz77Encoder(6))
    assert e.value.status == ffi.E_UNSUPPORTED and "LFX_LZ77_COST" in e.value.message
