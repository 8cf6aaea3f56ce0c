"""GPU: ChainLz77Encoder (LFX_LZ77_CHAIN, include/lfx.h) through every entry point that serves it.  Every case
compares bytes with the stream the contract implies (tests/chain_model.py: the oracle's generic encoder over the model's code
words; test_chain_model.py proves the model on the CPU).  Integer work: every comparison is exact.  Inputs are small — one case
needs two chunks (270 KiB), all others stay under 72 KiB — so that the Python model answers within seconds."""
import ctypes as C
import gzip as pygzip
import io
import os
import random
import re
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import chain_model as cm
from test_chain_model import OLDER_LONGER, TIE
from test_dict_encode_model import _rand, _text
from test_gpu_encode_stages import context_with
from test_gpu_parity import ctx, ffi, lfx  # noqa: F401  (fixtures)

KIB = 1 << 10
GUARD = 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tile(name):
    """a tile size of the chain kernel, from the header that exports it"""
    src = open(os.path.join(ROOT, "libflate_amd", "csrc", "lfx_chain.h")).read()
    return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, src).group(1))


TILE, TILE_SMALL = _tile("CHAIN_TILE"), _tile("CHAIN_TILE_SMALL")
TEXT = _text(48 * KIB, 51)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def _dev(torch, data):
    a = np.frombuffer(bytes(data), dtype=np.uint8).copy() if len(data) else np.zeros(4, dtype=np.uint8)
    return torch.from_numpy(a).to("cuda")


def kind(ffi, depth):
    return ffi.LZ77_CHAIN | depth << 8          # LFX_LZ77_CHAIN_DEPTH(depth)


def encode(c, ffi, torch, fmt, data, depth, write_size=0, writes=None, **kw):
    """lfx_encode_device with LFX_LZ77_CHAIN_DEPTH(depth) on device buffers, a guard behind the capacity → the stream"""
    opts, sched = ffi.make_opts(lz77_kind=kind(ffi, depth), **kw), ffi.make_schedule(write_size, writes)
    cap = (ffi.lib().lfx_encode_bound(len(data), C.byref(opts), C.byref(sched)) + 3) & ~3
    assert cap
    d_in = _dev(torch, data)
    d_out = torch.full((cap + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    n = c.encode_device(fmt, d_in.data_ptr(), len(data), d_out.data_ptr(), cap, opts, sched)
    whole = d_out.cpu().numpy().tobytes()
    assert whole[cap:] == b"\xA5" * GUARD, "bytes behind cap were written"
    return whole[:n]


def _okw(kw):
    """the library's option names → the model's / the oracle's"""
    o = dict(kw)
    if "lz77_level" in o:
        o["level"] = o.pop("lz77_level") - 1
    return o


def inflate(fmt, z):
    return zlib.decompress(z, {0: -15, 1: 15, 2: 31}[fmt])


def check(c, ffi, torch, oracle, data, depth, fmts=(0, 1, 2), write_size=0, **kw):
    """bytes equal to the expected stream in every format (the library's and the oracle's format numbers agree); python-zlib
    reads them back"""
    out = {}
    for fmt in fmts:
        got = encode(c, ffi, torch, fmt, data, depth, write_size, **kw)
        want = cm.expected_stream(oracle, fmt, data, depth, write_size, **_okw(kw))
        assert got == want, (fmt, len(data), depth, kw, len(got), len(want))
        assert inflate(fmt, got) == data
        out[fmt] = got
    return out


def roundtrip(c, ffi, torch, fmt, z, data):
    d_in = _dev(torch, z)
    d_out = torch.full((max(len(data), 4),), 0x5A, dtype=torch.uint8, device="cuda")
    rc, ol, used, msg = c.decode_device(fmt, d_in.data_ptr(), len(z), d_out.data_ptr(), len(data))
    assert (rc, ol, used) == (ffi.OK, len(data), len(z)), (rc, ol, used, msg)
    assert d_out.cpu().numpy().tobytes()[:ol] == data


# ---------------------------------------------------------------------------------------------- formats, depths, levels
@pytest.mark.parametrize("depth", [1, 2, 8, 255])
def test_formats_and_depths(ctx, ffi, torch, oracle, depth):
    z = check(ctx, ffi, torch, oracle, TEXT, depth)
    if depth == 1:
        assert z[0] == oracle.encode(oracle.DEFLATE, TEXT)          # the reference's code words
    if depth == 8:
        assert len(z[0]) < len(oracle.encode(oracle.DEFLATE, TEXT))
        roundtrip(ctx, ffi, torch, ffi.GZIP, z[2], TEXT)


def test_levels(ctx, ffi, torch, oracle):
    data = TEXT[:6000]
    z = check(ctx, ffi, torch, oracle, data, 4, fmts=(1, 2))
    assert z[1][1] >> 6 == 3 and z[2][8] == 2                       # FLEVEL 3, XFL 2: compression_level() is Best
    z = check(ctx, ffi, torch, oracle, data, 4, fmts=(1, 2), lz77_level=1 + 1)      # the caller's level wins: Fast
    assert z[1][1] >> 6 == 1 and z[2][8] == 4
    z = check(ctx, ffi, torch, oracle, data, 4, fmts=(1, 2), lz77_level=1 + 2)      # Balance
    assert z[1][1] >> 6 == 2 and z[2][8] == 0


# ---------------------------------------------------------------------------------------------- chunks, window, cap
def test_two_chunks(ctx, ffi, torch, oracle):
    """one write_all of 270 KiB: DefaultLz77Encoder's buffer holds it all — ONE chunk of 17 tiles, chains that run through 32 KiB
    of window at every tile edge; 8 KiB writes flush at 262144: two chunks, and no chain leaves its chunk"""
    data = _text(270 * KIB, 52)
    z = check(ctx, ffi, torch, oracle, data, 8, fmts=(0,))
    roundtrip(ctx, ffi, torch, ffi.DEFLATE, z[0], data)
    z8 = check(ctx, ffi, torch, oracle, data, 8, fmts=(0,), write_size=8192)
    assert z8[0] != z[0]
    # the first KiB again right behind the chunk boundary: nothing in front of 262144 is a candidate there
    rep = data[:262144] + data[:1024] + data[262144 + 1024:]
    check(ctx, ffi, torch, oracle, rep, 4, fmts=(0,), write_size=8192)
    codes = cm.chain_codes(rep[262144:], 4)
    assert all(not (w & 0xFFFF) for w in codes[:3])                 # (the model: the chunk starts with literals)


def test_window_cut_off_and_chain_end(ctx, ffi, torch, oracle):
    """window_size = 1024.  P occurs 900, 1100 and 2000 bytes back from X: the chain of X is cut off in its middle (1100 > W),
    though that occurrence is the longer one.  Q occurs 500 and 2000 back from Y: cd of the nearer one is 0 (1500 > W from
    it) and ends the chain"""
    buf = bytearray(_rand(9000, 31))
    P, Q = _rand(60, 32), _rand(40, 33)
    X, Y = 5000, 8000
    buf[X:X + 60] = P
    buf[X - 900:X - 900 + 10] = P[:10]
    buf[X - 1100:X - 1100 + 60] = P
    buf[X - 2000:X - 2000 + 60] = P
    buf[Y:Y + 40] = Q
    buf[Y - 500:Y - 500 + 40] = Q
    buf[Y - 2000:Y - 2000 + 40] = Q
    data = bytes(buf)
    codes = cm.chain_codes(data, 8, 1024)
    assert (10 << 16) | 900 in codes and (40 << 16) | 500 in codes and not any((w & 0xFFFF) > 1024 for w in codes)
    assert (60 << 16) | 1100 in cm.chain_codes(data, 8, 32768)     # (with the whole window the older, longer one is taken)
    check(ctx, ffi, torch, oracle, data, 8, window_size=1024)
    check(ctx, ffi, torch, oracle, data, 8, fmts=(0,))
    check(ctx, ffi, torch, oracle, TEXT[:20000], 8, fmts=(1,), window_size=1024)     # (CINFO follows the window)
    check(ctx, ffi, torch, oracle, TEXT[:20000], 255, fmts=(0,), window_size=300)


def test_max_length_16(ctx, ffi, torch, oracle):
    check(ctx, ffi, torch, oracle, TEXT[:20000] + b"a" * 300, 8, fmts=(0, 1), max_length=16)
    check(ctx, ffi, torch, oracle, TEXT[:5000], 8, fmts=(0,), max_length=3)


# ---------------------------------------------------------------------------------------------- runs, periods, crafted
def test_runs_and_periods(ctx, ffi, torch, oracle):
    z = check(ctx, ffi, torch, oracle, b"a" * 70000, 8, fmts=(0,))          # distance-1 chains, the early exit at the cap
    roundtrip(ctx, ffi, torch, ffi.DEFLATE, z[0], b"a" * 70000)
    per = b"abcdefg" * 3000
    assert all((w & 0xFFFF) in (0, 7) for w in cm.chain_codes(per, 8))      # ties go to the nearest: one period back
    check(ctx, ffi, torch, oracle, per, 8, fmts=(0,))
    check(ctx, ffi, torch, oracle, per, 255, fmts=(0,))
    for buf in (OLDER_LONGER, TIE):
        for depth in (1, 2, 8):
            check(ctx, ffi, torch, oracle, buf, depth, fmts=(0,))


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5])
def test_tiny_inputs(ctx, ffi, torch, oracle, n):
    check(ctx, ffi, torch, oracle, b"aaaaa"[:n], 8)
    check(ctx, ffi, torch, oracle, b"abcab"[:n], 2, fmts=(0,))


def test_match_bounded_by_the_buffer_end(ctx, ffi, torch, oracle):
    for cut in (0, 1, 2, 3, 4, 7):
        data = TEXT[:5000] + b"#" + TEXT[100:400] + TEXT[1000:1300 - cut]
        codes = cm.chain_codes(data, 8)
        assert codes[-1] & 0xFFFF or codes[-4] & 0xFFFF               # a match ends at, or three literals in front of, the end
        check(ctx, ffi, torch, oracle, data, 8, fmts=(0,))


# ---------------------------------------------------------------------------------------------- tile edges
def _edge_data(tile, n):
    """random bytes with a phrase P that straddles `tile` — its older copy the longer one — and, just behind the edge, 50 bytes
    of P's middle, whose nearest copy is the part of P that straddles the edge: a match and a chain cross it"""
    buf = bytearray(_rand(tile + 700, 40 + (tile >> 13)))
    P = _rand(300, 41)
    buf[tile - 150:tile + 150] = P
    buf[5000:5100] = P[:100]
    buf[1000:1300] = P
    buf[tile + 200:tile + 250] = P[120:170]
    return bytes(buf[:n])


@pytest.mark.parametrize("tile", [TILE, TILE_SMALL], ids=["window", "small"])
def test_tile_edges(ctx, ffi, torch, oracle, tile):
    """lengths around a tile: tile + 4 is the first with a position (one) in a second tile, end = n - 3; TILE_SMALL is also
    where the call changes from the small instance of the kernel to the window instance"""
    full = _edge_data(tile, tile + 700)
    codes = cm.chain_codes(full, 8)
    assert (258 << 16) | (tile - 150 - 1000) in codes and (50 << 16) | 230 in codes
    for n in (tile - 1, tile, tile + 1, tile + 3, tile + 4, tile + 5, tile + 700):
        check(ctx, ffi, torch, oracle, full[:n], 8, fmts=(0,))
    check(ctx, ffi, torch, oracle, full, 1, fmts=(0,))
    check(ctx, ffi, torch, oracle, b"a" * (tile + 4), 8, fmts=(0,))
    # input that does not start on a dword: the staging grid's byte phase
    opts = ffi.make_opts(lz77_kind=kind(ffi, 8))
    cap = (ffi.lib().lfx_encode_bound(len(full), C.byref(opts), None) + 3) & ~3
    for phase in (1, 2, 3):
        d_in = _dev(torch, b"\xEE" * phase + full)
        d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        n = ctx.encode_device(ffi.DEFLATE, d_in.data_ptr() + phase, len(full), d_out.data_ptr(), cap, opts, None)
        assert d_out.cpu().numpy().tobytes()[:n] == cm.expected_stream(oracle, 0, full, 8), phase


# ---------------------------------------------------------------------------------------------- other options
def test_other_options(ctx, ffi, torch, oracle):
    data = TEXT[:20000]
    check(ctx, ffi, torch, oracle, data, 8, dynamic_huffman=0)
    check(ctx, ffi, torch, oracle, data, 8, fmts=(0, 2), block_size=4096, write_size=1000)
    # 8 KiB writes with a flush event in the schedule
    writes = [8192, 8192, None, 8192, 100, None, 8192]
    for fmt in (0, 1):
        got = encode(ctx, ffi, torch, fmt, TEXT, 8, writes=writes)
        assert got == cm.expected_scheduled(oracle, fmt, TEXT, 8, writes) and inflate(fmt, got) == TEXT
    # stored blocks: no Lz77Encode runs, and no_compression resets the header's level — the default kind's bytes
    for fmt in (0, 1, 2):
        got = encode(ctx, ffi, torch, fmt, data, 8, no_compression=1)
        assert got == cm.expected_stream(oracle, fmt, data, 8, no_compression=1)
        opts = ffi.make_opts(no_compression=1)
        assert got == ctx.encode_host(fmt, data, opts)


# ---------------------------------------------------------------------------------------------- entry points
def test_host_call_and_module_helpers(lfx, ctx, ffi, oracle):
    data = TEXT[:30000]
    for fmt in (0, 1, 2):
        assert ctx.encode_host(fmt, data, ffi.make_opts(lz77_kind=kind(ffi, 8))) == cm.expected_stream(oracle, fmt, data, 8)
    enc = lfx.lz77.ChainLz77Encoder(8)
    assert enc.compression_level() == lfx.lz77.CompressionLevel.BEST and enc.window_size() == 32768
    assert lfx.deflate.compress(data, lz77=enc, context=ctx) == cm.expected_stream(oracle, 0, data, 8)
    assert lfx.zlib.compress(data, options=lfx.zlib.EncodeOptions(lz77=enc), context=ctx) == cm.expected_stream(oracle, 1, data, 8)
    assert lfx.gzip.compress(data, lz77=enc, context=ctx) == cm.expected_stream(oracle, 2, data, 8)
    small = lfx.lz77.ChainLz77Encoder(4, window_size=1024, max_length=16)
    assert lfx.zlib.compress(data, lz77=small, context=ctx) == cm.expected_stream(oracle, 1, data, 4, window_size=1024, max_length=16)


def test_batch_of_64_streams(ctx, ffi, torch, oracle):
    rng = random.Random(5)
    lens = [0, 3000, 1, 2, 3, 4, 5, 0] + [rng.randrange(6, 3000) for _ in range(56)]
    recs = [(TEXT[a:a + n // 2] + _text(n, 70 + i))[:n] for i, (n, a) in enumerate((n, rng.randrange(0, 30000)) for n in lens)]
    assert len(recs) == 64 and recs[0] == b"" and len(recs[1]) == 3000
    L = ffi.lib()
    opts = ffi.make_opts(lz77_kind=kind(ffi, 8))
    for fmt in (1, 2):
        caps = [(L.lfx_encode_bound(len(r), C.byref(opts), None) + 3) & ~3 for r in recs]
        offs = [sum(len(r) for r in recs[:i]) for i in range(64)]
        out_offs = [sum(caps[:i]) for i in range(64)]
        d_in = _dev(torch, b"".join(recs))
        d_out = torch.full((sum(caps) + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        a = lambda v: (C.c_uint64 * 64)(*v)
        ol, st = (C.c_uint64 * 64)(), (C.c_int32 * 64)()
        rc = L.lfx_encode_batch_device(ctx.handle, fmt, C.byref(opts), None, 64, d_in.data_ptr(), a(offs), a([len(r) for r in recs]),
                                       d_out.data_ptr(), a(out_offs), a(caps), ol, st)
        assert rc == ffi.OK, ctx.last_error()
        whole = d_out.cpu().numpy().tobytes()
        assert whole[sum(caps):] == b"\xA5" * GUARD
        for i, r in enumerate(recs):
            z = whole[out_offs[i]:out_offs[i] + ol[i]]
            assert st[i] == ffi.OK and z == cm.expected_stream(oracle, fmt, r, 8), (fmt, i, len(r))
            if i < 8 or i % 16 == 0:
                assert z == encode(ctx, ffi, torch, fmt, r, 8), (fmt, i)          # each equals its one-shot call


def test_stream_encoder(lfx, ctx, ffi, oracle):
    """8 KiB writes and a flush: equal to the one-shot call with that schedule"""
    data = TEXT + TEXT[:20000]
    writes = [8192] * 3 + [None] + [8192] * 5
    for mod, fmt in ((lfx.deflate, 0), (lfx.zlib, 1), (lfx.gzip, 2)):
        sink = io.BytesIO()
        e = mod.Encoder(sink, mod.EncodeOptions(lz77=lfx.lz77.ChainLz77Encoder(8)), ctx)
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
        assert got == cm.expected_scheduled(oracle, fmt, data, 8, writes + [len(data) - at]), fmt
        opts, sched = ffi.make_opts(lz77_kind=kind(ffi, 8)), ffi.make_schedule(writes=writes + [len(data) - at])
        assert got == ctx.encode_host(fmt, data, opts, sched)


@pytest.mark.parametrize("bgzf", [False, True], ids=["plain", "bgzf"])
def test_encode_members(lfx, ctx, ffi, oracle, bgzf):
    data = TEXT + _rand(9000, 44) + TEXT[:30000]
    size = 20000
    out, members = lfx.gzip.encode_members(data, size, bgzf=bgzf, lz77=lfx.lz77.ChainLz77Encoder(8), context=ctx)
    assert pygzip.decompress(out) == data
    assert len(members) == -(-len(data) // size)
    for in_off, in_len, out_off, out_len in members:
        piece = data[in_off:in_off + in_len]
        kw = {"extra": bytes([0x42, 0x43, 2, 0]) + (out_len - 1).to_bytes(2, "little")} if bgzf else {}
        assert out[out_off:out_off + out_len] == cm.expected_stream(oracle, 2, piece, 8, **kw), (in_off, bgzf)
        opts = ffi.make_opts(lz77_kind=kind(ffi, 8), **kw)
        assert out[out_off:out_off + out_len] == ctx.encode_host(ffi.GZIP, piece, opts)


def test_index_encode(lfx, ctx, ffi, torch, oracle):
    data = TEXT + TEXT[:22000]
    z, idx = lfx.Index.encode(data, "gzip", spacing=16 * KIB, options=lfx.gzip.EncodeOptions().block_size(8192),
                              schedule=ffi.make_schedule(4096), ctx=ctx, lz77=lfx.lz77.ChainLz77Encoder(8))
    zb = z.cpu().numpy().tobytes()
    assert zb == cm.expected_stream(oracle, 2, data, 8, write_size=4096, block_size=8192)
    assert zb == encode(ctx, ffi, torch, ffi.GZIP, data, 8, write_size=4096, block_size=8192)
    assert idx.read(z, 40000, 3000).cpu().numpy().tobytes() == data[40000:43000]
    idx.close()


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_and_no_state_left(lfx, ctx, ffi, torch, oracle):
    data = TEXT[:9000]
    for bad in (kind(ffi, 0), kind(ffi, 256), ffi.LZ77_CHAIN | 8 << 8 | 1 << 20):
        with pytest.raises(ffi.LfxError) as e:
            ctx.encode_host(ffi.ZLIB, data, ffi.make_opts(lz77_kind=bad))
        assert e.value.status == ffi.E_ARG
    with pytest.raises(ffi.LfxError) as e:
        ctx.encode_host(ffi.ZLIB, data, lfx.zlib.EncodeOptions(lz77=lfx.lz77.ChainLz77Encoder(256))._to_c())
    assert e.value.status == ffi.E_ARG
    zd = lfx.Dictionary(TEXT[20000:30000], ctx)
    try:
        with pytest.raises(ffi.LfxError) as e:
            ctx.encode_dict_host(ffi.ZLIB, zd, data, ffi.make_opts(lz77_kind=kind(ffi, 8)))
        assert e.value.status == ffi.E_UNSUPPORTED and "dictionary" in e.value.message
    finally:
        zd.close()
    info = ffi.ShardInfo()
    d_in = _dev(torch, data)
    opts = ffi.make_opts(lz77_kind=kind(ffi, 8))
    rc = ffi.lib().lfx_encode_shard_prepare(ctx.handle, ffi.ZLIB, C.byref(opts), None, d_in.data_ptr(), len(data), 1, 1, C.byref(info))
    assert rc == ffi.E_UNSUPPORTED
    # a chain call, then the default kind on the same context: the default bytes (and the other way round)
    check(ctx, ffi, torch, oracle, data, 8, fmts=(1,))
    assert ctx.encode_host(ffi.ZLIB, data) == oracle.encode(oracle.ZLIB, data)
    assert ctx.encode_host(ffi.ZLIB, data, ffi.make_opts(lz77_kind=ffi.LZ77_NOCOMPRESSION)) == \
        oracle.encode(oracle.ZLIB, data, lz77_kind=oracle.LZ77_NOCOMPRESSION)
    check(ctx, ffi, torch, oracle, data, 2, fmts=(1,))


def test_first_generation_match_kernel(lfx, ffi, torch, oracle):
    """the chain stage runs behind the match stage whichever generation ran (LFX_MATCH_V1 is read when a context is made)"""
    c = context_with(lfx, LFX_MATCH_V1="1")
    check(c, ffi, torch, oracle, TEXT, 8, fmts=(0,))
    check(c, ffi, torch, oracle, _edge_data(TILE, TILE + 700), 8, fmts=(0,))
