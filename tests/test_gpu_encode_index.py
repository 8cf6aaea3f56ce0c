"""GPU: the seek index built while encoding (lfx_encode_index_device, Index.encode).  Status, length and bytes must equal
lfx_encode_device's; where no compressed block produces more than the spacing, the index must equal, byte for byte, the one
lfx_decode_index_device builds from the encoded stream; inside large blocks the points must be real code boundaries
(proved by reads through every segment) and keep max_gap within the spacing."""
import ctypes as C
import gzip as pygzip
import random
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_parity import ctx, ffi, lfx, synth  # noqa: F401  (fixtures)

KIB = 1 << 10
MIB = 1 << 20


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def _dev(torch, data):
    a = np.frombuffer(bytes(data), dtype=np.uint8).copy() if len(data) else np.zeros(1, dtype=np.uint8)
    return torch.from_numpy(a).to("cuda")


def _inflate(fmt, ffi, comp):
    if fmt == ffi.GZIP:
        return pygzip.decompress(comp)
    return zlib.decompress(comp, 15 if fmt == ffi.ZLIB else -15)


def encode_both(ctx, ffi, torch, fmt, data, opts, sched, spacing=1 << 20, cap=None):
    """lfx_encode_device next to lfx_encode_index_device → (status, encoded bytes, index handle or None, message)"""
    n = len(data)
    d_in = _dev(torch, data)
    if cap is None:
        cap = (max(ffi.lib().lfx_encode_bound(n, C.byref(opts), C.byref(sched)), 64) + 3) & ~3
    d_a = torch.full((cap,), 0x5A, dtype=torch.uint8, device="cuda")
    d_b = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda")
    L = ffi.lib()
    la, lb, h = C.c_uint64(0), C.c_uint64(0), C.c_void_p(1234)
    ra = L.lfx_encode_device(ctx.handle, fmt, C.byref(opts), C.byref(sched), d_in.data_ptr(), n, d_a.data_ptr(), cap, C.byref(la))
    ma = ctx.last_error() if ra else ""
    rb = L.lfx_encode_index_device(ctx.handle, fmt, C.byref(opts), C.byref(sched), d_in.data_ptr(), n, d_b.data_ptr(), cap,
                                   C.byref(lb), spacing, C.byref(h))
    mb = ctx.last_error() if rb else ""
    torch.cuda.synchronize()
    assert (ra, la.value, ma) == (rb, lb.value, mb)
    if rb != ffi.OK:
        assert h.value is None
        return rb, b"", None, mb
    a = d_a[:la.value].cpu().numpy().tobytes()
    b = d_b[:lb.value].cpu().numpy().tobytes()
    assert a == b
    return rb, b, h.value, mb


def wrap(ctx, h):
    from libflate_amd.index import Index
    return Index(h, ctx)


# ------------------------------------------------------------------ 1. encode parity
OPTIONS = [dict(), dict(dynamic_huffman=0), dict(no_compression=1), dict(block_size=64 * KIB),
           dict(filename=b"a.txt", comment=b"made here", mtime=123456, extra=b"XY\x02\x00ab", hcrc=1)]


@pytest.mark.parametrize("fmt_name", ["DEFLATE", "ZLIB", "GZIP"])
def test_encode_parity(ctx, ffi, torch, synth, fmt_name):
    fmt = getattr(ffi, fmt_name)
    text = synth.text(4 * MIB).tobytes()
    scheds = [("S1", lambda: ffi.make_schedule(0)), ("S8K", lambda: ffi.make_schedule(8192)),
              ("list", lambda: ffi.make_schedule(writes=[1000, None, 70000, None, None, 5000, 2 * MIB, None]))]
    cases = []
    for size in (0, 1, 4095, 64 * KIB, 4 * MIB):
        for si, _s in enumerate(scheds):
            for oi, _o in enumerate(OPTIONS):
                cases.append((text[:size], si, oi))
    big_text, big_low = synth.text(32 * MIB).tobytes(), synth.lowent(32 * MIB).tobytes()
    for data in (big_text, big_low):
        for si in range(3):
            cases.append((data, si, 0))
        for oi in range(1, len(OPTIONS)):
            cases.append((data, 1, oi))
    for data, si, oi in cases:
        kw = OPTIONS[oi]
        if fmt != ffi.GZIP and "filename" in kw:
            kw = dict()
        opts, sched = ffi.make_opts(**kw), scheds[si][1]()
        rc, comp, h, msg = encode_both(ctx, ffi, torch, fmt, data, opts, sched, spacing=64 * KIB if oi == 3 else MIB)
        assert rc == ffi.OK, (len(data), scheds[si][0], kw, msg)
        assert _inflate(fmt, ffi, comp) == data
        idx = wrap(ctx, h)
        info = idx.info
        assert (info["format"], info["flags"], info["n_members"], info["in_len"], info["out_len"]) == (fmt, 0, 1, len(comp), len(data))
        idx.close()


# ------------------------------------------------------------------ 2. identity with the decode-built index
def _identity(ctx, ffi, torch, data, fmt, spacing, **opts):
    from libflate_amd.index import Index
    enc, idx = Index.encode(data, format=fmt, spacing=spacing, options=ffi.make_opts(**opts), schedule=ffi.make_schedule(8192), ctx=ctx)
    dec, idx_d = Index.build(enc, format=fmt, spacing=spacing, ctx=ctx)
    assert dec.cpu().numpy().tobytes() == data
    assert idx.to_bytes() == idx_d.to_bytes(), (idx.info, idx_d.info)
    idx.close()
    idx_d.close()


@pytest.mark.parametrize("fmt", ["deflate", "zlib", "gzip"])
def test_identity_with_decode_built_index(ctx, ffi, torch, synth, fmt):
    data = synth.text(32 * MIB).tobytes()
    for spacing in (1 * MIB, 4 * MIB):
        _identity(ctx, ffi, torch, data, fmt, spacing)
    _identity(ctx, ffi, torch, data, fmt, 64 * KIB, block_size=64 * KIB)


@pytest.mark.parametrize("fmt", ["deflate", "zlib", "gzip"])
def test_identity_cfg2(ctx, ffi, torch, synth, fmt):
    _identity(ctx, ffi, torch, synth.text(256 * MIB).tobytes(), fmt, 1 * MIB)


# ------------------------------------------------------------------ 3. points inside blocks
def _blob_windows(idx, data):
    blob = idx.to_bytes()
    at = 64 + 40 * idx.info["n_points"]
    for (_b, _h, out_off, _m, win_len, _c, _t) in idx.points:
        assert blob[at:at + win_len] == data[out_off - win_len:out_off]
        at += win_len
    assert at + 4 == len(blob)
    return blob


@pytest.mark.parametrize("kind", ["text", "lowent", "fixed"])
def test_points_inside_blocks(ctx, ffi, torch, synth, kind):
    from libflate_amd.index import Index
    data = (synth.lowent if kind == "lowent" else synth.text)(32 * MIB).tobytes()
    opts = ffi.make_opts(dynamic_huffman=0) if kind == "fixed" else None
    for spacing in (64 * KIB, 1 * MIB):
        enc, idx = Index.encode(data, format="gzip", spacing=spacing, options=opts, ctx=ctx)
        comp = enc.cpu().numpy().tobytes()
        assert pygzip.decompress(comp) == data
        info, pts = idx.info, idx.points
        assert info["max_gap"] <= spacing, (info["max_gap"], spacing)
        assert any(p[0] > p[1] for p in pts), "no point inside a block"
        for (in_bit, hdr_bit, out_off, member, win_len, _crc, btype) in pts:
            assert member == 0 and hdr_bit <= in_bit and btype == (1 if kind == "fixed" else 2)
            assert win_len == min(32768, out_off)
        _d, idx_d = Index.build(enc, format="gzip", spacing=spacing, ctx=ctx)
        starts = {p[1] for p in idx_d.points} | {p[0] for p in idx_d.points if p[0] == p[1]}
        assert {p[1] for p in pts} <= starts
        idx_d.close()
        _blob_windows(idx, data)
        # one read of everything passes every point: each segment must end exactly at the next point
        assert idx.read(enc, 0, len(data)).cpu().numpy().tobytes() == data
        rnd = random.Random(spacing)
        ranges = [(rnd.randrange(len(data)), rnd.choice([1, 100, 4096, 65536, 300000])) for _ in range(512)]
        for (o, ln), g in zip(ranges, idx.read_many(enc, ranges)):
            assert g.cpu().numpy().tobytes() == data[o:o + ln], (o, ln)
        idx.close()


@pytest.mark.parametrize("fmt", ["deflate", "gzip"])
def test_small_blocks_between_large_ones(ctx, ffi, torch, synth, fmt):
    """a write list whose blocks alternate between large ones (one write of MiBs makes one block) and small ones, an empty one
    included, at a spacing below the large blocks: the tiles of the small blocks lie between the large blocks' tiles, where the
    candidate kernels run over them and must leave them out"""
    from libflate_amd.index import Index
    data = synth.text(12 * MIB).tobytes()
    writes = [100 * KIB, None, 3 * MIB, None, 50 * KIB, None, None, 200 * KIB, None, 5 * MIB + 12345, None, 30000, None,
              700 * KIB, 900 * KIB, None]
    spacing = 256 * KIB
    enc, idx = Index.encode(data, format=fmt, spacing=spacing, schedule=ffi.make_schedule(writes=writes), ctx=ctx)
    comp = enc.cpu().numpy().tobytes()
    assert _inflate(getattr(ffi, fmt.upper()), ffi, comp) == data
    pts = idx.points
    assert idx.info["max_gap"] <= spacing
    inner = [p for p in pts if p[0] > p[1]]
    assert {p[1] for p in inner} and len({p[1] for p in inner}) >= 2, "points inside both large blocks expected"
    _blob_windows(idx, data)
    assert idx.read(enc, 0, len(data)).cpu().numpy().tobytes() == data
    rnd = random.Random(9)
    ranges = [(rnd.randrange(len(data)), rnd.choice([1, 5000, 65536, 700000])) for _ in range(512)]
    for (o, ln), g in zip(ranges, idx.read_many(enc, ranges)):
        assert g.cpu().numpy().tobytes() == data[o:o + ln], (o, ln)
    idx.close()


# ------------------------------------------------------------------ 4. persistence
def test_persistence(ctx, ffi, torch, synth):
    from libflate_amd.index import Index
    data = synth.text(16 * MIB).tobytes()
    enc, idx = Index.encode(data, format="zlib", spacing=256 * KIB, ctx=ctx)
    blob = idx.to_bytes()
    info = Index.check(blob)
    assert info == idx.info
    idx2 = Index.from_bytes(blob, ctx)
    assert idx2.to_bytes() == blob
    rnd = random.Random(3)
    ranges = [(rnd.randrange(len(data)), 70000) for _ in range(128)]
    a = [g.cpu().numpy().tobytes() for g in idx.read_many(enc, ranges)]
    b = [g.cpu().numpy().tobytes() for g in idx2.read_many(enc, ranges)]
    assert a == b == [data[o:o + ln] for o, ln in ranges]
    idx.close()
    idx2.close()


# ------------------------------------------------------------------ 5. errors
def test_errors(ctx, ffi, torch, synth):
    from libflate_amd.index import Index
    data = synth.text(1 * MIB).tobytes()
    d_in = _dev(torch, data)
    d_out = torch.zeros(2 * MIB, dtype=torch.uint8, device="cuda")
    L = ffi.lib()
    ol, h = C.c_uint64(99), C.c_void_p(1234)
    opts, sched = ffi.make_opts(), ffi.make_schedule(8192)
    assert L.lfx_encode_index_device(ctx.handle, ffi.GZIP, C.byref(opts), C.byref(sched), d_in.data_ptr(), len(data),
                                     d_out.data_ptr(), 2 * MIB, C.byref(ol), 4095, C.byref(h)) == ffi.E_ARG
    assert h.value is None
    rc, _c, h2, _m = encode_both(ctx, ffi, torch, ffi.GZIP, data, opts, sched, cap=4096)
    assert rc == ffi.E_NOSPACE and h2 is None
    rc, _c, h3, _m = encode_both(ctx, ffi, torch, ffi.GZIP, data, ffi.make_opts(max_length=2), sched)
    assert rc == ffi.E_ARG and h3 is None
    with pytest.raises(ffi.LfxError):
        Index.encode(data, spacing=4095, ctx=ctx)
    # a read through the index with damaged input
    enc, idx = Index.encode(data, format="gzip", spacing=64 * KIB, options=ffi.make_opts(block_size=64 * KIB), ctx=ctx)
    comp = bytearray(enc.cpu().numpy().tobytes())
    pts = idx.points
    mid, nxt = pts[len(pts) // 2], pts[len(pts) // 2 + 1]
    comp[(mid[0] + nxt[0]) // 16] ^= 0x04
    d_bad = _dev(torch, bytes(comp))
    seg = nxt[2] - mid[2]
    d_o = torch.zeros(seg, dtype=torch.uint8, device="cuda")
    rc, _l, st, msg = ctx.index_read_device(idx._h, d_bad.data_ptr(), 0, len(comp), [mid[2]], [seg], d_o.data_ptr(), [0])
    assert rc == ffi.E_INVALID_DATA and st == [ffi.E_INVALID_DATA], msg
    idx.close()
