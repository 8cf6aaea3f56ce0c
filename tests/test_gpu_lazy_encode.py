"""GPU: LazyLz77Encoder (LFX_LZ77_LAZY, include/lfx.h) through every entry point that serves it.  Every case
compares bytes with the stream the contract implies (tests/lazy_model.py: the oracle's generic encoder over the model's code
words; test_lazy_model.py proves the model on the CPU), and python-zlib inflates it.  Integer work: every comparison is exact.
Inputs stay under 72 KiB so that the Python model, which measures every position, answers within seconds.

The seams the demote kernel has (lfx_chain.hip): a tile's last position reads the length of the next tile's first (16384 in the
window instance); a chunk's position end - 1 never looks at what lies behind it; an item's positions are cut on the grid of 16
positions of the call's arrays, so chunk offsets off that grid (a batch with odd record offsets) take the by-hand edges."""
import ctypes as C
import gzip as pygzip
import io
import zlib

import pytest

pytestmark = pytest.mark.gpu

import chain_model as cm
import lazy_model as lm
from test_dict_encode_model import _rand, _text
from test_gpu_chain_encode import TILE, TILE_SMALL, _dev, _okw, inflate
from test_gpu_encode_stages import context_with
from test_gpu_parity import ctx, ffi, lfx  # noqa: F401  (fixtures)
from test_lazy_model import HIST, NEXT_LONGER, RISE_HIST, RISING, long_pair, place

KIB = 1 << 10
GUARD = 64
TEXT = _text(48 * KIB, 61)
MIXED = _text(19000, 62) + b"a" * 700 + _rand(500, 63)          # about 20 KB: text, a run, random bytes


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def lazy(ffi, depth):
    return ffi.LZ77_LAZY | depth << 8           # LFX_LZ77_LAZY_DEPTH(depth)


def chain(ffi, depth):
    return ffi.LZ77_CHAIN | depth << 8


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


def check(c, ffi, torch, oracle, data, depth, fmts=(0, 1, 2), write_size=0, **kw):
    """bytes equal to the expected stream in every format (the library's and the oracle's format numbers agree); python-zlib
    reads them back"""
    out = {}
    for fmt in fmts:
        got = encode(c, ffi, torch, fmt, data, lazy(ffi, depth), write_size, **kw)
        want = lm.expected_stream(oracle, fmt, data, depth, write_size, **_okw(kw))
        assert got == want, (fmt, len(data), depth, kw, len(got), len(want))
        assert inflate(fmt, got) == data
        out[fmt] = got
    return out


def batch(c, ffi, torch, oracle, fmt, recs, depth, gaps=None):
    """lfx_encode_batch_device: every record's bytes are the model's; gaps[i] bytes lie in front of record i in the input"""
    n = len(recs)
    gaps = gaps or [0] * n
    L = ffi.lib()
    opts = ffi.make_opts(lz77_kind=lazy(ffi, depth))
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
        assert st[i] == ffi.OK and z == lm.expected_stream(oracle, fmt, r, depth), (fmt, i, len(r), offs[i])
        assert inflate(fmt, z) == r
    return offs


# ---------------------------------------------------------------------------------------------- formats, depths, levels
@pytest.mark.parametrize("depth", [1, 8, 255])
def test_formats_and_depths(ctx, ffi, torch, oracle, depth):
    z = check(ctx, ffi, torch, oracle, MIXED, depth)
    assert z[1][1] >> 6 == 3 and z[2][8] == 2                       # FLEVEL 3, XFL 2: compression_level() is Best
    assert len(z[0]) < len(cm.expected_stream(oracle, 0, MIXED, depth))     # smaller than the chain at that depth
    if depth == 8:
        z = check(ctx, ffi, torch, oracle, MIXED[:6000], 8, fmts=(1, 2), lz77_level=1 + 1)      # the caller's level wins: Fast
        assert z[1][1] >> 6 == 1 and z[2][8] == 4


# ---------------------------------------------------------------------------------------------- crafted pairs
def test_crafted_pairs(ctx, ffi, torch, oracle):
    for buf in (NEXT_LONGER, RISING):
        for depth in (1, 8):
            z = check(ctx, ffi, torch, oracle, buf, depth, fmts=(0,))
            assert z[0] != cm.expected_stream(oracle, 0, buf, depth)          # (the chain takes the short match)
    # 257 then 258: the byte of the length array keeps them apart; 258 twice: not strictly longer, no demotion
    for first, second in ((257, 258), (258, 258), (256, 257), (258, 257)):
        buf, at = long_pair(first, second)
        L, _ = lm.lengths(buf, 8)
        assert (L[at], L[at + 1]) == (first, second)
        check(ctx, ffi, torch, oracle, buf, 8, fmts=(0,))
    check(ctx, ffi, torch, oracle, MIXED, 8, fmts=(0, 1), max_length=16)
    z = check(ctx, ffi, torch, oracle, MIXED[:5000], 8, fmts=(0,), max_length=3)
    assert z[0] == cm.expected_stream(oracle, 0, MIXED[:5000], 8, max_length=3)      # nothing can be longer: the chain's bytes


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5])
def test_tiny_inputs(ctx, ffi, torch, oracle, n):
    check(ctx, ffi, torch, oracle, b"aaaaa"[:n], 8)
    check(ctx, ffi, torch, oracle, b"abcab"[:n], 2, fmts=(0,))


# ---------------------------------------------------------------------------------------------- tile seam, window instance
@pytest.mark.parametrize("at", [TILE - 2, TILE - 1, TILE])
def test_tile_seam_window_instance(ctx, ffi, torch, oracle, at):
    """one chunk of 40 KB (one write_all): the deferred pair at 16383 / 16384 — the length the demotion of the tile's last
    position reads is another workgroup's — and one position to either side"""
    buf = place(40 * KIB, at)
    L, _ = lm.lengths(buf, 8)
    assert (L[at], L[at + 1]) == (3, 9) and TILE == 16384
    check(ctx, ffi, torch, oracle, buf, 8, fmts=(0,))


def test_rising_run_across_the_tile_seam(ctx, ffi, torch, oracle):
    for at in (TILE - 2, TILE - 1):                                     # L = 3, 5, 9 at at, at + 1, at + 2
        fill = bytes(128 + (v & 127) for v in _rand(40 * KIB, 91))
        buf = fill[:at - len(RISE_HIST)] + RISE_HIST + b"abcdefghijk"
        buf += fill[len(buf):]
        L, _ = lm.lengths(buf, 8)
        assert L[at:at + 3] == (3, 5, 9)
        check(ctx, ffi, torch, oracle, buf, 8, fmts=(0,))
    # the input off the dword and the 16-byte grid: the kernels' byte phase
    buf = place(40 * KIB, TILE - 1)
    opts = ffi.make_opts(lz77_kind=lazy(ffi, 8))
    cap = (ffi.lib().lfx_encode_bound(len(buf), C.byref(opts), None) + 3) & ~3
    for phase in (1, 2, 3, 7):
        d_in = _dev(torch, b"\xEE" * phase + buf)
        d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        n = ctx.encode_device(ffi.DEFLATE, d_in.data_ptr() + phase, len(buf), d_out.data_ptr(), cap, opts, None)
        assert d_out.cpu().numpy().tobytes()[:n] == lm.expected_stream(oracle, 0, buf, 8), phase


# ---------------------------------------------------------------------------------------------- chunk seam
def test_chunk_seam(ctx, ffi, torch, oracle):
    """window_size = 2048 and 8 KiB writes: chunks of 16384 bytes and a remainder.  The pair at end - 2 / end - 1 of the first
    chunk (its last visited positions: L(end - 1) is capped by the chunk's end, L(end) is 0 by contract) and a long match as
    early in the second chunk as one can be — after an encode that left long lengths all over the scratch"""
    first = place(0, 16384 - 5, tail=b"abcde")
    assert len(first) == 16384
    L, _ = lm.lengths(first, 8, 2048)
    assert (L[16384 - 5], L[16384 - 4], L[16384 - 3]) == (3, 4, 0)
    second = b"0123456789" * 2 + b"0123456789" * 30 + bytes(128 + (v & 127) for v in _rand(3000, 92))
    data = first + second
    check(ctx, ffi, torch, oracle, b"a" * 20000, 8, fmts=(0,), window_size=2048, write_size=8192)     # lengths of 258 everywhere
    z = check(ctx, ffi, torch, oracle, data, 8, fmts=(0, 2), window_size=2048, write_size=8192)
    assert z[0] != lm.expected_stream(oracle, 0, data, 8, window_size=2048)     # (one write_all: one chunk, another parse)
    # a candidate at end - 1 whose successor, were it read, would be longer: the run goes on through the chunk's end
    run = bytes(128 + (v & 127) for v in _rand(16384 - 40, 93)) + b"xy" + b"q" * 38 + b"q" * 600
    check(ctx, ffi, torch, oracle, b"a" * 20000, 8, fmts=(0,), window_size=2048, write_size=8192)
    check(ctx, ffi, torch, oracle, run, 8, fmts=(0,), window_size=2048, write_size=8192)


# ---------------------------------------------------------------------------------------------- small instance
def test_batch_small_instance(ctx, ffi, torch, oracle):
    """records of at most 8192 bytes: the small instance.  Records of 0..5 bytes, one of exactly 8192, the pair as early and as
    late in a record as it can be made, and odd gaps so that records start off the dword and the 16-byte grid"""
    early = place(0, len(HIST))                                         # the pair right behind its history
    late = place(0, 3000, tail=b"abcde")                                # at end - 2 / end - 1
    full = place(TILE_SMALL, TILE_SMALL - 5, tail=b"abcde")
    assert len(full) == TILE_SMALL == 8192 and len(late) == 3005
    recs = [b"", b"a", b"ab", b"abc", b"abca", b"abcab", early, late, full, NEXT_LONGER, RISING, MIXED[:3000], MIXED[18000:],
            long_pair(257, 258)[0], b"a" * 1000, _text(1100, 64)]
    gaps = [0, 1, 0, 2, 1, 5, 3, 1, 7, 1, 1, 9, 1, 3, 1, 11]
    offs = batch(ctx, ffi, torch, oracle, 1, recs, 8, gaps)
    assert any(o % 2 for o in offs) and any(o % 4 == 2 for o in offs) and any(o % 16 not in (0, 8) for o in offs)
    batch(ctx, ffi, torch, oracle, 2, recs, 1)
    batch(ctx, ffi, torch, oracle, 0, recs[6:], 32, gaps[6:])
    # one record over 8192 turns the call to the window instance
    batch(ctx, ffi, torch, oracle, 0, [full + b"abc", early, late], 8, [1, 1, 1])


# ---------------------------------------------------------------------------------------------- stale state
def test_stale_state(ctx, ffi, torch, oracle):
    data = MIXED[:9000]
    check(ctx, ffi, torch, oracle, TEXT, 8, fmts=(1,))
    # a kind-2 call and a kind-0 call behind a lazy call
    assert encode(ctx, ffi, torch, 1, data, chain(ffi, 8)) == cm.expected_stream(oracle, 1, data, 8)
    assert ctx.encode_host(ffi.ZLIB, data) == oracle.encode(oracle.ZLIB, data)
    assert ctx.encode_host(ffi.ZLIB, data, ffi.make_opts(lz77_kind=ffi.LZ77_NOCOMPRESSION)) == \
        oracle.encode(oracle.ZLIB, data, lz77_kind=oracle.LZ77_NOCOMPRESSION)
    # a lazy call behind a chain call
    assert encode(ctx, ffi, torch, 1, TEXT, chain(ffi, 8)) == cm.expected_stream(oracle, 1, TEXT, 8)
    check(ctx, ffi, torch, oracle, data, 8, fmts=(1,))
    # a second lazy call on a shorter input: old lengths (258 everywhere) and candidates lie beyond it
    check(ctx, ffi, torch, oracle, b"a" * 30000, 8, fmts=(0,))
    check(ctx, ffi, torch, oracle, place(0, 2000, tail=b"abcde"), 8, fmts=(0,))
    check(ctx, ffi, torch, oracle, data[:4000], 2, fmts=(0,))


# ---------------------------------------------------------------------------------------------- other options
def test_other_options(ctx, ffi, torch, oracle):
    data = MIXED
    check(ctx, ffi, torch, oracle, data, 8, dynamic_huffman=0)
    check(ctx, ffi, torch, oracle, data, 8, fmts=(0, 2), block_size=4096, write_size=1000)
    writes = [8192, 8192, None, 8192, 100, None, 8192]
    for fmt in (0, 1):
        got = encode(ctx, ffi, torch, fmt, TEXT, lazy(ffi, 8), writes=writes)
        assert got == lm.expected_scheduled(oracle, fmt, TEXT, 8, writes) and inflate(fmt, got) == TEXT
    # stored blocks: no Lz77Encode runs, no chain stage, and no_compression resets the header's level — the default kind's bytes
    for fmt in (0, 1, 2):
        got = encode(ctx, ffi, torch, fmt, data, lazy(ffi, 8), no_compression=1)
        assert got == lm.expected_stream(oracle, fmt, data, 8, no_compression=1)
        assert got == ctx.encode_host(fmt, data, ffi.make_opts(no_compression=1)) and inflate(fmt, got) == data


# ---------------------------------------------------------------------------------------------- entry points
def test_host_call_and_module_helpers(lfx, ctx, ffi, oracle):
    data = TEXT[:30000]
    for fmt in (0, 1, 2):
        assert ctx.encode_host(fmt, data, ffi.make_opts(lz77_kind=lazy(ffi, 8))) == lm.expected_stream(oracle, fmt, data, 8)
    enc = lfx.lz77.LazyLz77Encoder(8)
    assert enc.compression_level() == lfx.lz77.CompressionLevel.BEST and enc.window_size() == 32768
    assert lfx.deflate.compress(data, lz77=enc, context=ctx) == lm.expected_stream(oracle, 0, data, 8)
    assert lfx.zlib.compress(data, options=lfx.zlib.EncodeOptions(lz77=enc), context=ctx) == lm.expected_stream(oracle, 1, data, 8)
    assert lfx.gzip.compress(data, lz77=enc, context=ctx) == lm.expected_stream(oracle, 2, data, 8)
    small = lfx.lz77.LazyLz77Encoder(4, window_size=1024, max_length=16)
    z = lfx.zlib.compress(data, lz77=small, context=ctx)
    assert z == lm.expected_stream(oracle, 1, data, 4, window_size=1024, max_length=16) and zlib.decompress(z) == data


def test_stream_encoder(lfx, ctx, ffi, oracle):
    """8 KiB writes and a flush: equal to the one-shot call with that schedule"""
    data = TEXT + TEXT[:20000]
    writes = [8192] * 3 + [None] + [8192] * 5
    for mod, fmt in ((lfx.deflate, 0), (lfx.zlib, 1), (lfx.gzip, 2)):
        sink = io.BytesIO()
        e = mod.Encoder(sink, mod.EncodeOptions(lz77=lfx.lz77.LazyLz77Encoder(8)), ctx)
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
        assert got == lm.expected_scheduled(oracle, fmt, data, 8, writes + [len(data) - at]), fmt
        assert inflate(fmt, got) == data
        opts, sched = ffi.make_opts(lz77_kind=lazy(ffi, 8)), ffi.make_schedule(writes=writes + [len(data) - at])
        assert got == ctx.encode_host(fmt, data, opts, sched)


@pytest.mark.parametrize("bgzf", [False, True], ids=["plain", "bgzf"])
def test_encode_members(lfx, ctx, ffi, oracle, bgzf):
    data = TEXT + _rand(9000, 44) + TEXT[:30000]
    size = 20000
    out, members = lfx.gzip.encode_members(data, size, bgzf=bgzf, lz77=lfx.lz77.LazyLz77Encoder(8), context=ctx)
    assert pygzip.decompress(out) == data
    assert len(members) == -(-len(data) // size)
    for in_off, in_len, out_off, out_len in members:
        piece = data[in_off:in_off + in_len]
        kw = {"extra": bytes([0x42, 0x43, 2, 0]) + (out_len - 1).to_bytes(2, "little")} if bgzf else {}
        assert out[out_off:out_off + out_len] == lm.expected_stream(oracle, 2, piece, 8, **kw), (in_off, bgzf)


def test_index_encode(lfx, ctx, ffi, torch, oracle):
    data = TEXT + TEXT[:22000]
    z, idx = lfx.Index.encode(data, "gzip", spacing=16 * KIB, options=lfx.gzip.EncodeOptions().block_size(8192),
                              schedule=ffi.make_schedule(4096), ctx=ctx, lz77=lfx.lz77.LazyLz77Encoder(8))
    zb = z.cpu().numpy().tobytes()
    assert zb == lm.expected_stream(oracle, 2, data, 8, write_size=4096, block_size=8192)
    assert pygzip.decompress(zb) == data
    assert idx.read(z, 40000, 3000).cpu().numpy().tobytes() == data[40000:43000]
    idx.close()


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals(lfx, ctx, ffi, torch):
    data = TEXT[:9000]
    for bad in (lazy(ffi, 0), lazy(ffi, 256), lazy(ffi, 8) | 1 << 20):
        with pytest.raises(ffi.LfxError) as e:
            ctx.encode_host(ffi.ZLIB, data, ffi.make_opts(lz77_kind=bad))
        assert e.value.status == ffi.E_ARG
    with pytest.raises(ffi.LfxError) as e:
        ctx.encode_host(ffi.ZLIB, data, lfx.zlib.EncodeOptions(lz77=lfx.lz77.LazyLz77Encoder(256))._to_c())
    assert e.value.status == ffi.E_ARG
    zd = lfx.Dictionary(TEXT[20000:30000], ctx)
    try:
        with pytest.raises(ffi.LfxError) as e:
            ctx.encode_dict_host(ffi.ZLIB, zd, data, ffi.make_opts(lz77_kind=lazy(ffi, 8)))
        assert e.value.status == ffi.E_UNSUPPORTED and "dictionary" in e.value.message and "LAZY" in e.value.message
    finally:
        zd.close()
    info = ffi.ShardInfo()
    d_in = _dev(torch, data)
    opts = ffi.make_opts(lz77_kind=lazy(ffi, 8))
    rc = ffi.lib().lfx_encode_shard_prepare(ctx.handle, ffi.ZLIB, C.byref(opts), None, d_in.data_ptr(), len(data), 1, 1, C.byref(info))
    assert rc == ffi.E_UNSUPPORTED and "LAZY" in ctx.last_error()


# ---------------------------------------------------------------------------------------------- match generations
def test_other_match_generations(lfx, ffi, torch, oracle):
    """the chain stage and the demotion run behind the match stage whichever generation ran (LFX_MATCH_V1 is read when a
    context is made)"""
    c = context_with(lfx, LFX_MATCH_V1="1")
    check(c, ffi, torch, oracle, MIXED, 8, fmts=(0,))
    check(c, ffi, torch, oracle, place(40 * KIB, TILE - 1), 8, fmts=(0,))
