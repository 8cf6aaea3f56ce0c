"""GPU: lfx_encode_batch_packed_device (include/lfx.h) — the batch call's streams packed back to back at offsets
scanned on the device.  The yardstick is always the existing batch call (lfx_encode_batch_device / _dict_device, outputs at bound
spacing) plus Python's zlib and gzip: every packed stream equals the batch call's byte for byte, the offsets follow out_off[0] =
0, out_off[i + 1] = round_up(out_off[i] + out_len[i], align), total = the last stream's end, gap bytes are zero, and nothing at
or behind cap changes.  Integer work: every comparison is exact."""
import ctypes as C
import gzip as pygzip
import random
import time
import zlib as pyzlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_dict_encode_model import _rand, _text
from test_gpu_parity import ctx, ffi, lfx  # noqa: F401  (fixtures)

KIB = 1 << 10
GUARD = 64
TEXT = _text(260 * KIB, 81)
RAND = _rand(210 * KIB, 82)
D32 = _text(32768, 83)
LENGTHS = (0, 1, 2, 3, 5, 63, 64, 65, 4095, 4096, 4097, 65535, 65536, 65537, 200000)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def _dev(torch, data):
    a = np.frombuffer(bytes(data), dtype=np.uint8).copy() if len(data) else np.zeros(4, dtype=np.uint8)
    return torch.from_numpy(a).to("cuda")


def _offsets(recs):
    offs, pos = [], 0
    for r in recs:
        offs.append(pos)
        pos += len(r)
    return offs


def _arr(v):
    return (C.c_uint64 * max(len(v), 1))(*v)


def batch_streams(c, ffi, torch, fmt, recs, opts=None, sched=None, zd=None, d_in=None):
    """the yardstick: lfx_encode_batch_device / _dict_device with the outputs at bound spacing → the streams"""
    L = ffi.lib()
    op, sp = C.byref(opts) if opts is not None else None, C.byref(sched) if sched is not None else None
    bound = L.lfx_encode_dict_bound if zd is not None else L.lfx_encode_bound
    known = {}
    for r in recs:
        if len(r) not in known:
            known[len(r)] = (bound(len(r), op, sp) + 3) & ~3
    caps = [known[len(r)] for r in recs]
    out_offs, pos = [], 0
    for cap in caps:
        out_offs.append(pos)
        pos += cap
    d_in = d_in if d_in is not None else _dev(torch, b"".join(recs))
    d_out = torch.empty(sum(caps), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    if zd is not None:
        rc, res = c.encode_batch_dict_device(fmt, zd, d_in.data_ptr(), _offsets(recs), [len(r) for r in recs], d_out.data_ptr(),
                                             out_offs, caps, opts, sched)
    else:
        ol, st = (C.c_uint64 * len(recs))(), (C.c_int32 * len(recs))()
        rc = L.lfx_encode_batch_device(c.handle, fmt, op, sp, len(recs), d_in.data_ptr(), _arr(_offsets(recs)), _arr([len(r) for r in recs]),
                                       d_out.data_ptr(), _arr(out_offs), _arr(caps), ol, st)
        res = list(zip(st, ol))
    assert rc == ffi.OK and all(st == ffi.OK for st, _ in res)
    whole = d_out.cpu().numpy().tobytes()
    return [whole[o:o + n] for o, (_, n) in zip(out_offs, res)]


def check_layout(layout, total, align):
    at = 0
    for off, n in layout:
        at = -(-at // align) * align
        assert off == at and off % align == 0, (off, at, align)
        at += n
    assert total == at                                   # (the tail is not rounded)


def packed(c, ffi, torch, fmt, recs, opts=None, sched=None, zd=None, align=1, cap=None, d_in=None, table=False):
    """lfx_encode_batch_packed_device into a buffer with a 0xA5 canary from cap on → (rc, total, layout, the bytes in front of
    cap, the table read back or None); asserts the canary, the layout rule and — on success — zero gaps"""
    d_in = d_in if d_in is not None else _dev(torch, b"".join(recs))
    if cap is None:
        rc, cap, _ = c.encode_batch_packed_device(fmt, d_in.data_ptr(), _offsets(recs), [len(r) for r in recs], None, 0, zdict=zd,
                                                  opts=opts, schedule=sched, align=align)
        assert rc == ffi.E_NOSPACE
    d_out = torch.full((cap + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    d_table = torch.full((2 * max(len(recs), 1),), -1, dtype=torch.int64, device="cuda") if table else None
    torch.cuda.synchronize()
    rc, total, layout = c.encode_batch_packed_device(fmt, d_in.data_ptr(), _offsets(recs), [len(r) for r in recs], d_out.data_ptr(), cap,
                                                     zdict=zd, opts=opts, schedule=sched, align=align,
                                                     d_table=d_table.data_ptr() if table else None)
    whole = d_out.cpu().numpy().tobytes()
    assert whole[cap:] == b"\xA5" * GUARD, "bytes at or behind cap changed"
    check_layout(layout, total, align)
    assert rc == (ffi.OK if total <= cap else ffi.E_NOSPACE)
    if rc == ffi.OK:
        at = 0
        for off, n in layout:
            assert whole[at:off] == bytes(off - at), "gap bytes are zero"
            at = off + n
    return rc, total, layout, whole[:cap], (d_table.cpu().numpy().astype(np.uint64).reshape(-1, 2) if table else None)


def check_equal(c, ffi, torch, fmt, recs, opts=None, sched=None, zd=None, align=1):
    d_in = _dev(torch, b"".join(recs))
    want = batch_streams(c, ffi, torch, fmt, recs, opts, sched, zd, d_in)
    rc, total, layout, whole, _ = packed(c, ffi, torch, fmt, recs, opts, sched, zd, align, None, d_in)
    assert rc == ffi.OK and [n for _, n in layout] == [len(w) for w in want]
    for i, ((off, n), w) in enumerate(zip(layout, want)):
        assert whole[off:off + n] == w, (i, len(recs[i]))
    return want, layout, total


def inflate(ffi, fmt, z, zdict=None):
    if fmt == ffi.GZIP:
        return pygzip.decompress(z)
    d = pyzlib.decompressobj(-15 if fmt == ffi.DEFLATE else 15, **({"zdict": zdict} if zdict is not None else {}))
    out = d.decompress(z) + d.flush()
    assert d.eof and not d.unused_data
    return out


def mixed_records(seed=1):
    """every length as text, as random bytes and as zeros, shuffled"""
    recs = []
    for i, n in enumerate(LENGTHS):
        recs += [TEXT[i * 977:i * 977 + n], RAND[i * 331:i * 331 + n], bytes(n)]
    random.Random(seed).shuffle(recs)
    return recs


@pytest.mark.parametrize("fmt_name", ["deflate", "zlib", "gzip"])
def test_streams_equal_the_batch_call(ctx, ffi, torch, fmt_name):
    fmt = {"deflate": ffi.DEFLATE, "zlib": ffi.ZLIB, "gzip": ffi.GZIP}[fmt_name]
    recs = mixed_records()
    assert sorted(set(map(len, recs))) == sorted(LENGTHS) and len(recs) == 45
    want, layout, total = check_equal(ctx, ffi, torch, fmt, recs)
    for r, w in zip(recs, want):
        assert inflate(ffi, fmt, w) == r


@pytest.mark.parametrize("count", [1, 2, 255, 256, 257, 1025, 65537])
def test_counts(ctx, ffi, torch, count):
    """records of 0..7 bytes, raw DEFLATE with fixed codes: a stream is a few bytes, the layout is all there is"""
    rng = random.Random(count)
    recs = [TEXT[a:a + rng.randrange(0, 8)] for a in (rng.randrange(0, 1000) for _ in range(count))]
    opts = ffi.make_opts(dynamic_huffman=0)
    d_in = _dev(torch, b"".join(recs))
    want = batch_streams(ctx, ffi, torch, ffi.DEFLATE, recs, opts, None, None, d_in)
    cap = sum(len(w) for w in want)
    t0 = time.perf_counter()
    rc, total, layout, whole, _ = packed(ctx, ffi, torch, ffi.DEFLATE, recs, opts, None, None, 1, cap, d_in)
    print("packed call and checks, %d records: %.3f s" % (count, time.perf_counter() - t0))
    assert rc == ffi.OK and total == cap and whole == b"".join(want)        # align = 1: the streams back to back are the output
    assert [n for _, n in layout] == [len(w) for w in want]


@pytest.mark.parametrize("align", [1, 4, 64, 4096])
def test_align(ctx, ffi, torch, align):
    recs = [TEXT[:300], b"", RAND[:4097], TEXT[5000:5003], bytes(70000), TEXT[9000:9063], RAND[7:8]]
    base = batch_streams(ctx, ffi, torch, ffi.ZLIB, recs)
    want, layout, total = check_equal(ctx, ffi, torch, ffi.ZLIB, recs, align=align)
    assert want == base and all(off % align == 0 for off, _ in layout)
    assert total == layout[-1][0] + layout[-1][1]                      # (the tail is not rounded)


@pytest.mark.parametrize("fmt_name", ["deflate", "zlib", "gzip"])
def test_capacity_and_reach(ctx, ffi, torch, fmt_name):
    """cap == total with total % 4 in {1, 2, 3}: the last dword of the output reaches behind cap, and for raw DEFLATE the
    pack kernel's last OR is the last write — the canary behind cap stays; one byte less is LFX_E_NOSPACE with the layout"""
    fmt = {"deflate": ffi.DEFLATE, "zlib": ffi.ZLIB, "gzip": ffi.GZIP}[fmt_name]
    pool = [TEXT[100 * k:100 * k + 40 + 3 * k] for k in range(48)]
    lens = [len(w) for w in batch_streams(ctx, ffi, torch, fmt, pool)]
    base = [TEXT[:700], RAND[:33], b""]
    base_want = batch_streams(ctx, ffi, torch, fmt, base)
    seen = set()
    for k, n in enumerate(lens):
        r = (sum(map(len, base_want)) + n) % 4
        if r == 0 or r in seen:
            continue
        seen.add(r)
        recs = base + [pool[k]]
        d_in = _dev(torch, b"".join(recs))
        want = batch_streams(ctx, ffi, torch, fmt, recs, d_in=d_in)
        total = sum(map(len, want))
        assert total % 4 == r
        rc, got_total, layout, whole, _ = packed(ctx, ffi, torch, fmt, recs, cap=total, d_in=d_in)
        assert (rc, got_total) == (ffi.OK, total) and whole == b"".join(want)
        # one byte less: void, the layout reported, nothing at or behind cap written (packed() holds the canary)
        rc, short_total, short_layout, _, _ = packed(ctx, ffi, torch, fmt, recs, cap=total - 1, d_in=d_in)
        assert (rc, short_total, short_layout) == (ffi.E_NOSPACE, total, layout)
        # the context goes on: the same call with room succeeds
        rc, again_total, again_layout, whole, _ = packed(ctx, ffi, torch, fmt, recs, cap=total, d_in=d_in)
        assert (rc, again_total, again_layout) == (ffi.OK, total, layout) and whole == b"".join(want)
        # the size query
        rc, q_total, q_layout = ctx.encode_batch_packed_device(fmt, d_in.data_ptr(), _offsets(recs), [len(x) for x in recs], None, 0)
        assert (rc, q_total, q_layout) == (ffi.E_NOSPACE, total, layout)
    assert seen == {1, 2, 3}, seen


def _kib_records(n, seed):
    rng = random.Random(seed)
    recs = []
    for i in range(n):
        a = rng.randrange(0, 30000)
        m = rng.randrange(700, 1400)
        recs.append((D32[a:a + m // 2] + TEXT[i * 200:i * 200 + m])[:m])
    return recs


def test_dictionary(lfx, ctx, ffi, torch):
    recs = _kib_records(1000, 7)
    zd = lfx.Dictionary(D32, ctx)
    try:
        want, _, _ = check_equal(ctx, ffi, torch, ffi.ZLIB, recs, zd=zd)
        for r, w in list(zip(recs, want))[::97]:
            assert int.from_bytes(w[2:6], "big") == zd.id and inflate(ffi, ffi.ZLIB, w, D32) == r
    finally:
        zd.close()


def test_chain_dictionary_lazy(lfx, ctx, ffi, torch):
    recs = _kib_records(1000, 8)
    zd = lfx.Dictionary(D32, ctx, chain=True)
    try:
        opts = ffi.make_opts(lz77_kind=ffi.LZ77_LAZY | 8 << 8)           # LazyLz77Encoder(8)
        want, _, _ = check_equal(ctx, ffi, torch, ffi.ZLIB, recs, opts=opts, zd=zd)
        plain = batch_streams(ctx, ffi, torch, ffi.ZLIB, recs[:50], zd=zd)
        assert want[:50] != plain                                        # (the option reached the parse)
        for r, w in list(zip(recs, want))[::97]:
            assert inflate(ffi, ffi.ZLIB, w, D32) == r
    finally:
        zd.close()


OPTION_CASES = {
    # name: (opts, schedule, records)
    "huffman_auto": (dict(dynamic_huffman=2), None, lambda: [RAND[:5001], RAND[20:5022], RAND[50:5053], RAND[9:70000], TEXT[3:4], TEXT[:3000], RAND[100:133], TEXT[:90000]]),
    "block_merge": (dict(block_merge=1, block_size=64 * KIB), None, lambda: [TEXT[:250 * KIB], TEXT[1000:1000 + 70 * KIB], TEXT[:100], b""]),
    "level6": (dict(lz77_kind=4 | 6 << 8), None, lambda: [TEXT[:100000], TEXT[500:1500], RAND[:2000], b"ab" * 3000]),
    "no_compression": (dict(no_compression=1), None, lambda: [TEXT[:70000], RAND[:3], b"", TEXT[:65535]]),
    "sched_fixed_8192": (dict(), ("fixed", 8192), lambda: [TEXT[:100000], TEXT[:8192], TEXT[:8193], b"", RAND[:20000]]),
    "sched_list_flush": (dict(), ("list", [100, None, 200, 5000]), lambda: [TEXT[:5300], TEXT[:300], RAND[:5300], TEXT[7:5307]]),
}


@pytest.mark.parametrize("name", list(OPTION_CASES))
def test_options(ctx, ffi, torch, name):
    kw, sch, make = OPTION_CASES[name]
    opts = ffi.make_opts(**kw)
    sched = None if sch is None else ffi.make_schedule(sch[1]) if sch[0] == "fixed" else ffi.make_schedule(writes=sch[1])
    recs = make()
    for fmt in (ffi.DEFLATE, ffi.GZIP):
        want, layout, _ = check_equal(ctx, ffi, torch, fmt, recs, opts=opts, sched=sched)
        for r, w in zip(recs, want):
            assert inflate(ffi, fmt, w) == r
        if name == "huffman_auto" and fmt == ffi.DEFLATE:
            # an incompressible record is one stored block (BTYPE 00); one of them starts at an odd byte offset
            # (5001 and 5002 random bytes are 5006 and 5007 bytes stored: the third record's stored blocks start at byte 10013)
            assert want[0][0] & 6 == 0 and len(want[0]) == 5001 + 5 and len(want[1]) == 5002 + 5
            assert want[2][0] & 6 == 0 and layout[2][0] == 10013


def test_device_table(ctx, ffi, torch):
    recs = mixed_records(2)[:20]
    for align in (1, 64):
        rc, total, layout, _, table = packed(ctx, ffi, torch, ffi.GZIP, recs, align=align, table=True)
        assert rc == ffi.OK and [tuple(int(x) for x in row) for row in table] == layout
        # a void call fills it too
        rc, short_total, short_layout, _, table = packed(ctx, ffi, torch, ffi.GZIP, recs, align=align, cap=total - 1, table=True)
        assert (rc, short_total, short_layout) == (ffi.E_NOSPACE, total, layout)
        assert [tuple(int(x) for x in row) for row in table] == layout


def test_round_trip_through_the_batch_decoder(ctx, ffi, torch):
    """lfx_decode_batch_device documents no alignment for its input: align = 1, and the device table as its in_off / in_len"""
    recs = mixed_records(3)
    L = ffi.lib()
    for fmt in (ffi.DEFLATE, ffi.ZLIB, ffi.GZIP):
        d_in = _dev(torch, b"".join(recs))
        rc, total, _ = ctx.encode_batch_packed_device(fmt, d_in.data_ptr(), _offsets(recs), [len(r) for r in recs], None, 0)
        d_z = torch.zeros(total + 4, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rc, total, layout = ctx.encode_batch_packed_device(fmt, d_in.data_ptr(), _offsets(recs), [len(r) for r in recs], d_z.data_ptr(), total)
        assert rc == ffi.OK
        k = len(recs)
        d_back = torch.full((max(d_in.numel(), 4),), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        out_len, st = (C.c_uint64 * k)(), (C.c_int32 * k)()
        assert L.lfx_decode_batch_device(ctx.handle, fmt, k, d_z.data_ptr(), _arr([o for o, _ in layout]), _arr([n for _, n in layout]),
                                         d_back.data_ptr(), _arr(_offsets(recs)), _arr([len(r) for r in recs]), out_len, st) == ffi.OK
        assert list(st) == [ffi.OK] * k and list(out_len) == [len(r) for r in recs]
        assert d_back.cpu().numpy().tobytes()[:sum(map(len, recs))] == b"".join(recs)


def test_refusals_and_argument_errors(lfx, ctx, ffi, torch):
    recs = [TEXT[:500], TEXT[600:900]]
    d_in = _dev(torch, b"".join(recs))
    d_out = torch.full((8192,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    call = lambda fmt=ffi.ZLIB, out=None, **kw: ctx.encode_batch_packed_device(
        fmt, d_in.data_ptr(), _offsets(recs), [len(r) for r in recs], d_out.data_ptr() if out is None else out, 4096, **kw)
    plain, other = lfx.Dictionary(D32, ctx), lfx.Context(0)
    foreign = lfx.Dictionary(D32, other)
    try:
        # LFX_LZ77_CHAIN with a plain dictionary: as in the batch call
        chain = ffi.make_opts(lz77_kind=ffi.LZ77_CHAIN | 8 << 8)
        with pytest.raises(ffi.LfxError) as e:
            call(zdict=plain, opts=chain)
        assert e.value.status == ffi.E_UNSUPPORTED and "LFX_LZ77_CHAIN with a preset dictionary" in e.value.message
        with pytest.raises(ffi.LfxError) as e2:
            ctx.encode_batch_dict_device(ffi.ZLIB, plain, d_in.data_ptr(), _offsets(recs), [len(r) for r in recs], d_out.data_ptr(),
                                         [0, 4096], [4096, 4096], chain)
        assert (e2.value.status, e2.value.message) == (e.value.status, e.value.message)
        assert call(opts=chain)[0] == ffi.OK                    # (without a dictionary it is served)
        for kw in (dict(align=3), dict(align=8192), dict(align=0), dict(out=d_out.data_ptr() + 1), dict(out=d_out.data_ptr() + 2),
                   dict(fmt=ffi.GZIP, zdict=plain), dict(zdict=foreign), dict(opts=ffi.make_opts(block_size=0))):
            with pytest.raises(ffi.LfxError) as e:
                call(**kw)
            assert e.value.status == ffi.E_ARG, kw
        assert d_out.cpu().numpy().tobytes()[4096:] == b"\xA5" * 4096
        # no records: LFX_OK, total 0
        assert ctx.encode_batch_packed_device(ffi.GZIP, None, [], [], d_out.data_ptr(), 4096) == (ffi.OK, 0, [])
        # NULL host outputs
        L = ffi.lib()
        assert L.lfx_encode_batch_packed_device(ctx.handle, ffi.ZLIB, None, None, None, 2, d_in.data_ptr(), _arr(_offsets(recs)),
                                                _arr([len(r) for r in recs]), 1, d_out.data_ptr(), 4096, None, None, None, None) == ffi.OK
        assert call()[0] == ffi.OK
    finally:
        plain.close()
        foreign.close()


def test_python_helpers(lfx, ctx, ffi):
    recs = [TEXT[:3000], b"", RAND[:700], TEXT[4000:4001], TEXT[:70000]]
    assert lfx.gzip.compress_batch(recs, context=ctx) == [lfx.gzip.compress(r, context=ctx) for r in recs]
    assert lfx.gzip.compress_batch(recs, context=ctx, level=6) == [lfx.gzip.compress(r, context=ctx, level=6) for r in recs]
    assert lfx.zlib.compress_batch(recs, zdict=D32, context=ctx) == [lfx.zlib.compress(r, zdict=D32, context=ctx) for r in recs]
    assert lfx.zlib.compress_batch(recs, context=ctx, merge_blocks=True) == [lfx.zlib.compress(r, context=ctx, merge_blocks=True) for r in recs]
    assert lfx.deflate.compress_batch(recs, zdict=D32, context=ctx, lz77=lfx.lz77.LazyLz77Encoder(8)) == \
        [lfx.deflate.compress(r, zdict=D32, context=ctx, lz77=lfx.lz77.LazyLz77Encoder(8)) for r in recs]
    assert lfx.gzip.compress_batch([], context=ctx) == []
    for r, z in zip(recs, lfx.gzip.compress_batch(recs, context=ctx)):
        assert pygzip.decompress(z) == r


def test_context_method_returns_the_c_layout(ctx, ffi, torch):
    recs = mixed_records(4)[:12]
    d_in = _dev(torch, b"".join(recs))
    rc, total, layout = ctx.encode_batch_packed_device(ffi.ZLIB, d_in.data_ptr(), _offsets(recs), [len(r) for r in recs], None, 0, align=64)
    k = len(recs)
    oo, ol, tt = (C.c_uint64 * k)(), (C.c_uint64 * k)(), C.c_uint64(0)
    assert ffi.lib().lfx_encode_batch_packed_device(ctx.handle, ffi.ZLIB, None, None, None, k, d_in.data_ptr(), _arr(_offsets(recs)),
                                                    _arr([len(r) for r in recs]), 64, None, 0, oo, ol, C.byref(tt), None) == ffi.E_NOSPACE
    assert rc == ffi.E_NOSPACE and (total, layout) == (tt.value, list(zip(oo, ol)))
    check_layout(layout, total, 64)
