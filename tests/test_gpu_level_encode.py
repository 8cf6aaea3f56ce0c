"""GPU: LevelLz77Encoder (LFX_LZ77_LEVEL, include/lfx.h) through every entry point that serves it.  Every case
compares bytes with the stream the contract implies (tests/level_model.py: the oracle's generic encoder over the model's code
words; test_level_model.py proves the model on the CPU), and python-zlib inflates it.  Integer work: every comparison is exact.
Inputs stay small: the Python model measures up to 4096 candidates at every position.

What the tuned instances add to the chain kernel's seams (lfx_chain.hip): the walk's cut at a nice match, the store's test for
a far 3-byte match, and max_lazy in the demotion — each at the last position of a tile of the window instance (16383) and the
first of the next, in the small instance (chunks of at most 8192 bytes), at a chunk's last visited positions, and through a
chain dictionary's tail."""
import ctypes as C
import gzip as pygzip
import io
import zlib

import pytest

pytestmark = pytest.mark.gpu

import auto_block_model as abm
import chain_model as cm
import lazy_model as lm
import level_model as vm
from test_dict_encode_model import _rand, _text
from test_gpu_chain_encode import TILE, TILE_SMALL, _dev, inflate
from test_gpu_parity import ctx, ffi, lfx  # noqa: F401  (fixtures)
from test_level_model import MIXED, deep_case, far_case, lazy_case, nice_case, put

KIB = 1 << 10
GUARD = 64
LEVELS = (1, 3, 4, 6, 9)
FMT_NAMES = {0: "deflate", 1: "zlib", 2: "gzip"}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def level(ffi, n):
    return ffi.LZ77_LEVEL | n << 8              # LFX_LZ77_LEVEL_N(n)


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
        got = encode(c, ffi, torch, fmt, data, level(ffi, lvl), write_size, **kw)
        want = vm.expected_stream(oracle, fmt, data, lvl, write_size, **kw)
        assert got == want, (fmt, len(data), lvl, kw, len(got), len(want))
        assert inflate(fmt, got) == data
        out[fmt] = got
    return out


def crafted():
    """the buffers of test_level_model.py, each rule on both sides of its threshold"""
    bufs = [put(*nice_case(n, r))[0] for n in (8, 16, 32, 128) for r in (n, n - 1)]
    bufs += [put(*far_case(d, k))[0] for d, k in ((4096, 3), (4097, 3), (4097, 4))]
    bufs += [put(*lazy_case(a, b))[0] for a, b in ((3, 9), (4, 9), (15, 22), (16, 22), (257, 258))]
    return bufs + [put(*deep_case(300))[0]]


# ---------------------------------------------------------------------------------------------- formats, levels, crafted buffers
@pytest.mark.parametrize("lvl", LEVELS)
def test_formats_levels_and_crafted_buffers(ctx, ffi, torch, oracle, lvl):
    z = check(ctx, ffi, torch, oracle, MIXED, lvl, fmts=(0, 1, 2))
    flevel, xfl = {1: (1, 4), 2: (2, 0), 3: (3, 2)}[vm.header_level(lvl)]
    assert z[1][1] >> 6 == flevel and z[2][8] == xfl
    for buf in crafted():
        check(ctx, ffi, torch, oracle, buf, lvl)
    check(ctx, ffi, torch, oracle, MIXED, lvl, max_length=6)                   # max_length below nice
    check(ctx, ffi, torch, oracle, MIXED[:4000], lvl, fmts=(1,), window_size=512)
    for n in range(6):
        check(ctx, ffi, torch, oracle, b"abcab"[:n], lvl, fmts=(0, 2))


def test_the_rules_change_the_bytes(ctx, ffi, torch, oracle):
    """each crafted case differs from the untuned kind at the level's depth: the tuned instance ran, not the kinds' 2 and 3"""
    buf = put(*nice_case(16, 16))[0]
    assert check(ctx, ffi, torch, oracle, buf, 4)[0] != lm.expected_stream(oracle, 0, buf, 16)
    buf = put(*nice_case(8, 8))[0]
    assert check(ctx, ffi, torch, oracle, buf, 1)[0] != cm.expected_stream(oracle, 0, buf, 4)
    buf = put(*far_case(4097, 3))[0]
    assert check(ctx, ffi, torch, oracle, buf, 6)[0] != lm.expected_stream(oracle, 0, buf, 128)
    buf = put(*lazy_case(16, 22))[0]
    assert check(ctx, ffi, torch, oracle, buf, 6)[0] != lm.expected_stream(oracle, 0, buf, 128)
    buf = put(*deep_case(300))[0]
    assert check(ctx, ffi, torch, oracle, buf, 9)[0] != check(ctx, ffi, torch, oracle, buf, 6)[0]
    # a caller's level wins over the level's own; no_compression resets it and runs no chain stage
    for fmt in (1, 2):
        got = encode(ctx, ffi, torch, fmt, MIXED[:3000], level(ffi, 6), lz77_level=1 + 3)
        assert got == vm.expected_stream(oracle, fmt, MIXED[:3000], 6, header=3)
        got = encode(ctx, ffi, torch, fmt, MIXED[:3000], level(ffi, 9), no_compression=1)
        assert got == ctx.encode_host(fmt, MIXED[:3000], ffi.make_opts(no_compression=1)) and inflate(fmt, got) == MIXED[:3000]


# ---------------------------------------------------------------------------------------------- tile seam, window instance
@pytest.mark.parametrize("at", [TILE - 1, TILE])
def test_tile_seam_window_instance(ctx, ffi, torch, oracle, at):
    """one chunk of 20 KB: each rule's deciding position at 16383 (a tile's last: the length the demotion reads next is another
    workgroup's) and at 16384"""
    assert TILE == 16384
    for case, lvl in ((nice_case(16, 16), 4), (nice_case(16, 15), 4), (nice_case(8, 8), 1), (far_case(4097, 3), 6), (far_case(4096, 3), 6),
                      (lazy_case(15, 22), 6), (lazy_case(16, 22), 6), (lazy_case(3, 9), 4), (lazy_case(4, 9), 4)):
        buf, p = put(*case, at=at, total=20000)
        assert p == at
        check(ctx, ffi, torch, oracle, buf, lvl)
    buf, _ = put(*deep_case(300), at=at, total=20000)
    check(ctx, ffi, torch, oracle, buf, 9)


# ---------------------------------------------------------------------------------------------- small instance, chunk seam, batch
def test_small_instance(ctx, ffi, torch, oracle):
    """a chunk of at most 8192 bytes"""
    for lvl in (1, 4, 6, 9):
        check(ctx, ffi, torch, oracle, (MIXED + MIXED)[:TILE_SMALL], lvl)
        check(ctx, ffi, torch, oracle, put(*far_case(4097, 3), total=TILE_SMALL - 8)[0][:TILE_SMALL], lvl)


def test_two_chunks_with_a_pair_at_the_end_of_the_first(ctx, ffi, torch, oracle):
    """window_size = 2048 and 8 KiB writes: a chunk of 16384 bytes and a remainder.  The pair at end - 2 / end - 1 of the first
    chunk: L(end - 1) is capped by the chunk's end and L(end) is 0 by contract"""
    hist, tail = lazy_case(3, 9)
    first, at = put(hist, tail[:5], at=16384 - 5, total=0)
    first = first[:16384]
    assert len(first) == 16384 and at == 16384 - 5
    L, _ = vm.level_lengths(first, 4, 2048)
    assert (L[at], L[at + 1], L[at + 2]) == (3, 4, 0)
    data = first + first[-300:] + MIXED[:3000]          # (what the second chunk repeats of the first is no candidate in it)
    for lvl in (4, 6):
        z = check(ctx, ffi, torch, oracle, data, lvl, fmts=(0, 2), window_size=2048, write_size=8192)
        assert z[0] != vm.expected_stream(oracle, 0, data, lvl, window_size=2048)        # (one write_all: one chunk)


def batch(c, ffi, torch, oracle, fmt, recs, lvl, gaps):
    n = len(recs)
    L = ffi.lib()
    opts = ffi.make_opts(lz77_kind=level(ffi, lvl))
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
    rc = L.lfx_encode_batch_device(c.handle, fmt, C.byref(opts), None, n, d_in.data_ptr(), a(offs), a([len(r) for r in recs]),
                                   d_out.data_ptr(), a(out_offs), a(caps), ol, st)
    assert rc == ffi.OK, c.last_error()
    whole = d_out.cpu().numpy().tobytes()
    assert whole[sum(caps):] == b"\xA5" * GUARD
    for i, r in enumerate(recs):
        z = whole[out_offs[i]:out_offs[i] + ol[i]]
        assert st[i] == ffi.OK and z == vm.expected_stream(oracle, fmt, r, lvl), (fmt, i, len(r), offs[i])
        assert inflate(fmt, z) == r


def test_batch_of_records(ctx, ffi, torch, oracle):
    """records of 0..5 and of 8192 bytes, off the dword and the 16-byte grid"""
    full = put(*lazy_case(15, 22), at=TILE_SMALL - 60, total=0)[0][:TILE_SMALL]
    full += MIXED[:TILE_SMALL - len(full)]
    assert len(full) == TILE_SMALL
    recs = [b"", b"a", b"ab", b"abc", b"abca", b"abcab", full, put(*nice_case(16, 16))[0], put(*far_case(4097, 3))[0],
            put(*lazy_case(16, 22))[0], put(*deep_case(300))[0], MIXED[:3000]]
    gaps = [0, 1, 0, 2, 1, 5, 3, 1, 7, 1, 1, 9]
    batch(ctx, ffi, torch, oracle, 1, recs, 6, gaps)
    batch(ctx, ffi, torch, oracle, 0, recs, 1, gaps)
    batch(ctx, ffi, torch, oracle, 2, recs[5:], 9, gaps[5:])
    batch(ctx, ffi, torch, oracle, 0, [full + b"abc"] + recs[7:10], 4, [1, 1, 1, 1])     # one record over 8192: the window instance


# ---------------------------------------------------------------------------------------------- a chain dictionary
def test_chain_dictionary(lfx, ctx, ffi, oracle):
    zdict = MIXED[3000:8000]
    data = MIXED[2000:9000]
    zd = lfx.Dictionary(zdict, ctx, chain=True)
    try:
        for fmt in (ffi.ZLIB, ffi.DEFLATE):
            got = ctx.encode_dict_host(fmt, zd, data, ffi.make_opts(lz77_kind=level(ffi, 6)))
            assert got == vm.expected_dict_stream(oracle, FMT_NAMES[fmt], zdict, data, 6)
        # the rules through the dictionary's tail: the nearest candidate, in the tail, is nice; a 3-byte match 4097 back is dropped
        for (hist, tail), lvl in ((nice_case(16, 16), 4), (nice_case(128, 128), 6), (far_case(4097, 3), 6), (far_case(4096, 3), 6), (deep_case(300), 9),
                                  (deep_case(300), 6), (nice_case(8, 8), 1)):
            d = lfx.Dictionary(hist, ctx, chain=True)
            try:
                got = ctx.encode_dict_host(ffi.DEFLATE, d, tail + MIXED[:500], ffi.make_opts(lz77_kind=level(ffi, lvl)))
                assert got == vm.expected_dict_stream(oracle, "deflate", hist, tail + MIXED[:500], lvl), (lvl, len(hist))
            finally:
                d.close()
    finally:
        zd.close()
    z = lfx.zlib.compress(data, zdict=zdict, level=6, context=ctx)          # bytes: the chain dictionary is made here
    assert z == vm.expected_dict_stream(oracle, "zlib", zdict, data, 6)
    dec = zlib.decompressobj(zdict=zdict)
    assert dec.decompress(z) + dec.flush() == data


# ---------------------------------------------------------------------------------------------- entry points
def test_host_call_and_module_helpers(lfx, ctx, ffi, oracle):
    data = MIXED
    for fmt in (0, 1, 2):
        assert ctx.encode_host(fmt, data, ffi.make_opts(lz77_kind=level(ffi, 6))) == vm.expected_stream(oracle, fmt, data, 6)
    enc = lfx.lz77.LevelLz77Encoder(6)
    assert enc.compression_level() == lfx.lz77.CompressionLevel.BALANCE and enc.window_size() == 32768
    assert lfx.deflate.compress(data, lz77=enc, context=ctx) == vm.expected_stream(oracle, 0, data, 6)
    assert lfx.deflate.compress(data, level=3, context=ctx) == vm.expected_stream(oracle, 0, data, 3)
    assert lfx.zlib.compress(data, level=9, context=ctx) == vm.expected_stream(oracle, 1, data, 9)
    assert lfx.gzip.compress(data, level=1, context=ctx) == vm.expected_stream(oracle, 2, data, 1)
    small = lfx.lz77.LevelLz77Encoder(4, window_size=1024, max_length=12)
    z = lfx.zlib.compress(data, lz77=small, context=ctx)
    assert z == vm.expected_stream(oracle, 1, data, 4, window_size=1024, max_length=12) and zlib.decompress(z) == data
    with pytest.raises(ValueError):
        lfx.gzip.compress(data, lz77=enc, level=6, context=ctx)


def test_stream_encoder_with_flushes(lfx, ctx, ffi, oracle):
    data = MIXED + MIXED[:6000]
    writes = [4096] * 2 + [None] + [4096]
    for mod, fmt in ((lfx.deflate, 0), (lfx.zlib, 1), (lfx.gzip, 2)):
        sink = io.BytesIO()
        e = mod.Encoder(sink, mod.EncodeOptions(lz77=lfx.lz77.LevelLz77Encoder(6)), ctx)
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
        assert got == vm.expected_stream(oracle, fmt, data, 6, writes=writes + [len(data) - at]), fmt
        assert inflate(fmt, got) == data


@pytest.mark.parametrize("bgzf", [False, True], ids=["plain", "bgzf"])
def test_members_of_4096_bytes(lfx, ctx, ffi, oracle, bgzf):
    data = MIXED + put(*lazy_case(16, 22))[0] + MIXED[:2500]
    out, members = lfx.gzip.encode_members(data, 4096, bgzf=bgzf, lz77=lfx.lz77.LevelLz77Encoder(6), context=ctx)
    assert pygzip.decompress(out) == data and len(members) == -(-len(data) // 4096)
    for in_off, in_len, out_off, out_len in members:
        piece = data[in_off:in_off + in_len]
        kw = {"extra": bytes([0x42, 0x43, 2, 0]) + (out_len - 1).to_bytes(2, "little")} if bgzf else {}
        assert out[out_off:out_off + out_len] == vm.expected_stream(oracle, 2, piece, 6, **kw), (in_off, bgzf)


def test_index_encode(lfx, ctx, ffi, torch, oracle):
    data = MIXED + MIXED[:7000]
    z, idx = lfx.Index.encode(data, "gzip", spacing=4 * KIB, options=lfx.gzip.EncodeOptions().block_size(4096),
                              schedule=ffi.make_schedule(2048), ctx=ctx, lz77=lfx.lz77.LevelLz77Encoder(6))
    zb = z.cpu().numpy().tobytes()
    assert zb == vm.expected_stream(oracle, 2, data, 6, write_size=2048, block_size=4096)
    assert pygzip.decompress(zb) == data
    assert idx.read(z, 9000, 3000).cpu().numpy().tobytes() == data[9000:12000]
    idx.close()


def test_auto_huffman_with_level_6(ctx, ffi, torch, oracle):
    data = MIXED[:6000] + _rand(3000, 71) + b"\x00" * 2000
    for fmt in (0, 1):
        want = abm.expected(oracle, FMT_NAMES[fmt], data, block_size=2048, write_size=1024,
                            encode=lambda f, d, write_size=0, **kw: vm.expected_stream(oracle, fmt, d, 6, write_size, **kw))[0]
        got = encode(ctx, ffi, torch, fmt, data, level(ffi, 6), write_size=1024, dynamic_huffman=2, block_size=2048)
        assert got == want and inflate(fmt, got) == data
        assert got != encode(ctx, ffi, torch, fmt, data, level(ffi, 6), write_size=1024, block_size=2048)


# ---------------------------------------------------------------------------------------------- stale state
def test_other_kinds_behind_a_level_call(lfx, ctx, ffi, torch, oracle):
    """a kind-3 and a kind-0 call directly behind a level call on one context: the bytes of a fresh context"""
    data = put(*lazy_case(16, 22), at=9000, total=12000)[0]
    fresh = lfx.Context(0)
    want3 = encode(fresh, ffi, torch, 1, data, ffi.LZ77_LAZY | 8 << 8)
    want0 = fresh.encode_host(ffi.ZLIB, data)
    assert want3 == lm.expected_stream(oracle, 1, data, 8) and want0 == oracle.encode(oracle.ZLIB, data)
    check(ctx, ffi, torch, oracle, b"a" * 14000, 9)                     # lengths of 258 all over the scratch
    check(ctx, ffi, torch, oracle, data, 6)
    assert encode(ctx, ffi, torch, 1, data, ffi.LZ77_LAZY | 8 << 8) == want3
    check(ctx, ffi, torch, oracle, data, 6)
    assert ctx.encode_host(ffi.ZLIB, data) == want0
    check(ctx, ffi, torch, oracle, data, 1)
    assert encode(ctx, ffi, torch, 1, data, ffi.LZ77_CHAIN | 8 << 8) == cm.expected_stream(oracle, 1, data, 8)
    check(ctx, ffi, torch, oracle, data[:5000], 4)                      # a level call behind them, on a shorter input


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals(lfx, ctx, ffi, torch):
    data = MIXED[:5000]
    for bad in (level(ffi, 0), level(ffi, 10), level(ffi, 255), level(ffi, 6) | 1 << 16, level(ffi, 6) | 1 << 30):
        with pytest.raises(ffi.LfxError) as e:
            ctx.encode_host(ffi.ZLIB, data, ffi.make_opts(lz77_kind=bad))
        assert e.value.status == ffi.E_ARG
    with pytest.raises(ffi.LfxError) as e:
        lfx.zlib.compress(data, level=10, context=ctx)
    assert e.value.status == ffi.E_ARG
    zd = lfx.Dictionary(MIXED[5000:9000], ctx)
    try:
        with pytest.raises(ffi.LfxError) as e:
            ctx.encode_dict_host(ffi.ZLIB, zd, data, ffi.make_opts(lz77_kind=level(ffi, 6)))
        assert e.value.status == ffi.E_UNSUPPORTED and "dictionary" in e.value.message and "LFX_LZ77_LEVEL" in e.value.message
    finally:
        zd.close()
    info = ffi.ShardInfo()
    d_in = _dev(torch, data)
    opts = ffi.make_opts(lz77_kind=level(ffi, 6))
    rc = ffi.lib().lfx_encode_shard_prepare(ctx.handle, ffi.ZLIB, C.byref(opts), None, d_in.data_ptr(), len(data), 1, 1, C.byref(info))
    assert rc == ffi.E_UNSUPPORTED and "LFX_LZ77_LEVEL" in ctx.last_error()
