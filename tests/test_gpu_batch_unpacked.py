"""GPU: lfx_decode_batch_packed_device (include/lfx.h) — a batch decoded back to back, placed by the decoded
sizes.  The yardstick is always the composition it replaces, made here from the existing calls: lfx_decode_batch_size_device,
the layout out_off[0] = 0, out_off[i + 1] = round_up(out_off[i] + size[i], align) by numpy, then lfx_decode_batch_device /
_dict_device with out_cap = size — and, where a stream is valid, Python's zlib.  Integer work: every comparison is exact."""
import ctypes as C
import zlib as pyzlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_dict_encode_model import _rand, _text
from test_gpu_parity import ctx, ffi, lfx  # noqa: F401  (fixtures)

KIB = 1 << 10
GUARD = 64
SENTINEL = 0xA5
TEXT = _text(200 * KIB, 91)
D32 = _text(32768, 92)
D_OTHER = _text(32768, 93)
WBITS = {"gzip": 31, "zlib": 15, "deflate": -15}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def _fmt(ffi, name):
    return {"gzip": ffi.GZIP, "zlib": ffi.ZLIB, "deflate": ffi.DEFLATE}[name]


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


def _z(data, wbits, level=6, strategy=pyzlib.Z_DEFAULT_STRATEGY, zdict=None, flush_every=0):
    kw = {"zdict": zdict} if zdict is not None else {}
    co = pyzlib.compressobj(level, pyzlib.DEFLATED, wbits, 8, strategy, **kw)
    if not flush_every:
        return co.compress(data) + co.flush()
    out = b""
    for at in range(0, len(data), flush_every):
        out += co.compress(data[at:at + flush_every]) + co.flush(pyzlib.Z_FULL_FLUSH)
    return out + co.flush()


_POOLS = {}


def pool(lfx, name):
    """→ [(record, stream)]: the seven kinds of the issue's mixed batch, in the format `name`"""
    if name not in _POOLS:
        w = WBITS[name]
        recs = [b"", b"hello", TEXT[5000:5000 + 7 * 700], _rand(3000, 94), TEXT[9000:11000], TEXT, TEXT[20000:20000 + KIB]]
        mod = getattr(lfx, name)
        streams = [_z(recs[0], w),                       # an empty stream: decoded size 0
                   _z(recs[1], w),                       # fewer than 64 input bytes: the serial path
                   _z(recs[2], w, flush_every=700),      # seven full flushes: more than BLOCK_ROUNDS blocks
                   _z(recs[3], w, level=0),              # stored blocks
                   _z(recs[4], w, strategy=pyzlib.Z_FIXED),   # a fixed-Huffman block
                   mod.compress(recs[5]),                # about 200 KiB of text from this library's own encoder
                   _z(recs[6], w)]                       # a 1 KiB record
        assert len(streams[1]) < 64 <= len(streams[6]) and len(streams[0]) < 64
        _POOLS[name] = list(zip(recs, streams))
    return _POOLS[name]


def mixed(lfx, name, count, turn=0):
    """count streams cycling through the pool from kind `turn` on; the large record only among the first fourteen"""
    p = pool(lfx, name)
    picks = [(i + turn) % 7 for i in range(count)]
    picks = [6 if (k == 5 and i >= 14) else k for i, k in enumerate(picks)]
    return [p[k][0] for k in picks], [p[k][1] for k in picks]


def layout_np(sizes, align):
    sizes = np.asarray(sizes, dtype=np.uint64)
    terms = (sizes + np.uint64(align - 1)) // np.uint64(align) * np.uint64(align)
    offs = np.concatenate([np.zeros(1, np.uint64), np.cumsum(terms[:-1], dtype=np.uint64)])
    return [int(x) for x in offs], int(offs[-1]) + int(sizes[-1])


def composed(c, ffi, torch, fmt, streams, align, zd=None, sizes=None, d_in=None):
    """the yardstick → (offs, total, sizes, consumed or None, [(status, out_len)], the sentinel-filled buffer's bytes, message)"""
    d_in = d_in if d_in is not None else _dev(torch, b"".join(streams))
    in_offs, in_lens = _offsets(streams), [len(s) for s in streams]
    used = None
    if sizes is None:
        sizes, used, _st = c.decode_batch_size_device(fmt, d_in.data_ptr(), in_offs, in_lens)
    offs, total = layout_np(sizes, align)
    d_out = torch.full((total + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    if zd is not None:
        res = c.decode_batch_dict_device(fmt, zd, d_in.data_ptr(), in_offs, in_lens, d_out.data_ptr(), offs, list(sizes))
    else:
        ol, st = (C.c_uint64 * len(streams))(), (C.c_int32 * len(streams))()
        rc = ffi.lib().lfx_decode_batch_device(c.handle, fmt, len(streams), d_in.data_ptr(), _arr(in_offs), _arr(in_lens), d_out.data_ptr(),
                                               _arr(offs), _arr(list(sizes)), ol, st)
        assert rc == ffi.OK
        res = list(zip(st, ol))
    msg = c.last_error() if any(s != ffi.OK for s, _ in res) else ""
    return offs, total, list(sizes), used, res, d_out.cpu().numpy().tobytes(), msg


def unpacked(c, ffi, torch, fmt, streams, align, zd=None, cap=None, d_in=None, table=False, in_table=False):
    """the call under test into a sentinel-filled buffer of cap + GUARD bytes (cap None: the size query first)
    → (rc, offs, lens, consumed, statuses, total, the buffer's bytes, d_table read back or None)"""
    d_in = d_in if d_in is not None else _dev(torch, b"".join(streams))
    in_offs, in_lens = _offsets(streams), [len(s) for s in streams]
    kw = {"zdict": zd, "align": align}
    if in_table:
        pairs = np.array([v for p in zip(in_offs, in_lens) for v in p], dtype=np.int64)
        d_pairs = torch.from_numpy(pairs).to("cuda")
        kw["d_in_table"] = d_pairs.data_ptr()
        in_offs, in_lens = len(streams), None
    if cap is None:
        rc, _o, _l, _u, _s, cap = c.decode_batch_packed_device(fmt, d_in.data_ptr(), in_offs, in_lens, None, 0, **kw)
        assert rc == (ffi.E_NOSPACE if cap else ffi.OK)
    d_out = torch.full((cap + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_table = torch.full((2 * max(len(streams), 1),), -1, dtype=torch.int64, device="cuda") if table else None
    torch.cuda.synchronize()
    rc, offs, lens, used, st, total = c.decode_batch_packed_device(fmt, d_in.data_ptr(), in_offs, in_lens, d_out.data_ptr(), cap,
                                                                  d_table=d_table.data_ptr() if table else None, **kw)
    whole = d_out.cpu().numpy().tobytes()
    assert whole[cap:] == bytes([SENTINEL]) * GUARD, "bytes at or behind cap changed"
    return rc, offs, lens, used, st, total, whole, (d_table.cpu().numpy().astype(np.uint64).reshape(-1, 2) if table else None)


def outside_slots_untouched(whole, offs, sizes, upto):
    """every byte of whole[0, upto) outside the slots [off, off + size) still holds the sentinel"""
    mask = np.ones(upto, dtype=bool)
    for o, n in zip(offs, sizes):
        mask[o:o + n] = False
    return bool(np.all(np.frombuffer(whole, dtype=np.uint8)[:upto][mask] == SENTINEL))


def check_against_composition(c, ffi, torch, fmt, streams, align, zd=None, sizes=None, want_used=None, **kw):
    d_in = _dev(torch, b"".join(streams))
    offs, total, sizes, used, res, ref, msg = composed(c, ffi, torch, fmt, streams, align, zd, sizes, d_in)
    rc, g_offs, g_lens, g_used, g_st, g_total, whole, table = unpacked(c, ffi, torch, fmt, streams, align, zd, None, d_in, **kw)
    g_msg = c.last_error() if any(s != ffi.OK for s in g_st) else ""
    assert rc == ffi.OK
    assert (g_offs, g_total) == (offs, total)
    assert g_st == [s for s, _ in res] and g_lens == [n for _, n in res]
    used = used if used is not None else want_used
    if used is not None:
        assert g_used == list(used)
    assert whole[:total] == ref[:total], "the bytes differ from the composition's"
    assert outside_slots_untouched(whole, offs, sizes, total + GUARD)
    assert g_msg == msg
    return offs, sizes, g_lens, g_st, whole, table


# ---- 1. equality with the composition -------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 2, 257, 300])
@pytest.mark.parametrize("align", [1, 8, 4096])
@pytest.mark.parametrize("name", ["gzip", "zlib", "deflate"])
def test_equals_the_composition(ctx, ffi, lfx, torch, name, align, count):
    # (count 1 and 2 start at another kind per align, so that the single stream is the large, the stored and the flushed one)
    recs, streams = mixed(lfx, name, count, turn={1: 5, 8: 3, 4096: 2}[align] if count <= 2 else 0)
    offs, sizes, lens, st, whole, _ = check_against_composition(ctx, ffi, torch, _fmt(ffi, name), streams, align)
    assert all(s == ffi.OK for s in st) and sizes == [len(r) for r in recs] == lens
    for o, r, s in zip(offs, recs, streams):
        assert whole[o:o + len(r)] == r
    for s, r in {s: r for s, r in zip(streams, recs)}.items():         # (Python's zlib on each distinct stream)
        assert pyzlib.decompressobj(WBITS[name]).decompress(s) == r


# ---- 2. preset dictionary ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def zd(lfx, ctx):
    d = lfx.Dictionary(D32, ctx)
    yield d
    d.close()


def _dict_records():
    return [TEXT[30000 + 1500 * i:30000 + 1500 * i + n] for i, n in enumerate((KIB, 40, 0, 3 * KIB, KIB, 700, 9 * KIB, 1))]


@pytest.mark.parametrize("align", [1, 8])
def test_dictionary_zlib(ctx, ffi, torch, zd, align):
    recs = _dict_records()
    streams = [_z(r, 15, zdict=D32) for r in recs]
    streams[4] = _z(recs[4], 15)                                      # a zlib record without FDICT in the same batch
    assert all(s[1] & 0x20 for i, s in enumerate(streams) if i != 4) and not streams[4][1] & 0x20
    offs, sizes, lens, st, whole, _ = check_against_composition(ctx, ffi, torch, ffi.ZLIB, streams, align, zd, [len(r) for r in recs],
                                                                want_used=[len(s) for s in streams])
    assert all(s == ffi.OK for s in st) and lens == [len(r) for r in recs]
    for o, r in zip(offs, recs):
        assert whole[o:o + len(r)] == r


@pytest.mark.parametrize("align", [1, 4096])
def test_dictionary_raw_deflate(ctx, ffi, torch, zd, align):
    recs = _dict_records()
    streams = [_z(r, -15, zdict=D32) for r in recs]
    for s, r in zip(streams, recs):
        assert pyzlib.decompressobj(-15, zdict=D32).decompress(s) == r
    offs, sizes, lens, st, whole, _ = check_against_composition(ctx, ffi, torch, ffi.DEFLATE, streams, align, zd, [len(r) for r in recs],
                                                                want_used=[len(s) for s in streams])
    assert all(s == ffi.OK for s in st) and lens == [len(r) for r in recs]
    for o, r in zip(offs, recs):
        assert whole[o:o + len(r)] == r


def test_wrong_dictionary_fails_that_stream_only(ctx, ffi, torch, zd):
    recs = _dict_records()
    streams = [_z(r, 15, zdict=D32) for r in recs]
    streams[3] = _z(recs[3], 15, zdict=D_OTHER)
    sizes = [0 if i == 3 else len(r) for i, r in enumerate(recs)]
    offs, sizes, lens, st, whole, _ = check_against_composition(ctx, ffi, torch, ffi.ZLIB, streams, 8, zd, sizes)
    assert [s == ffi.OK for s in st] == [i != 3 for i in range(len(recs))] and lens[3] == 0
    assert ctx.last_error().startswith("Dictionary mismatch")
    for i, (o, r) in enumerate(zip(offs, recs)):
        assert i == 3 or whole[o:o + len(r)] == r


# ---- 3. damaged streams -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gzip", "zlib"])
def test_damage_stays_in_its_slot(ctx, ffi, torch, name):
    recs = [TEXT[40000 + 4000 * i:40000 + 4000 * i + n] for i, n in enumerate((KIB, 3 * KIB, 500, 2 * KIB, 5 * KIB, KIB, 2 * KIB, 100))]
    streams = [_z(r, WBITS[name]) for r in recs]
    streams[1] = streams[1][:len(streams[1]) // 2]                                     # truncated inside a block
    t = bytearray(streams[4]); t[-6 if name == "gzip" else -2] ^= 0x10; streams[4] = bytes(t)   # a flipped trailer checksum
    h = bytearray(streams[6]); h[0] ^= 0xFF; streams[6] = bytes(h)                     # a bad header
    offs, sizes, lens, st, whole, _ = check_against_composition(ctx, ffi, torch, _fmt(ffi, name), streams, 8)
    assert [s == ffi.OK for s in st] == [i not in (1, 4, 6) for i in range(8)]
    for i in (0, 2, 3, 5, 7):                                                          # the five neighbours are intact
        assert whole[offs[i]:offs[i] + len(recs[i])] == recs[i] and lens[i] == len(recs[i])
    assert lens[6] == 0 and sizes[6] == 0
    assert whole[offs[1]:offs[1] + lens[1]] == recs[1][:lens[1]]                       # what the truncated stream produced


# ---- 4. capacity and arguments ------------------------------------------------------------------------------------------------
def test_capacity_protocol(ctx, ffi, lfx, torch):
    recs, streams = mixed(lfx, "gzip", 9)
    d_in = _dev(torch, b"".join(streams))
    rc, offs, lens, used, st, total, whole, _ = unpacked(ctx, ffi, torch, ffi.GZIP, streams, 8, d_in=d_in)
    assert rc == ffi.OK and lens == [len(r) for r in recs] and used == [len(s) for s in streams]
    # one byte short: the same layout, the sizes and the size call's verdicts, nothing written
    rc1, offs1, lens1, used1, st1, total1, whole1, _ = unpacked(ctx, ffi, torch, ffi.GZIP, streams, 8, cap=total - 1, d_in=d_in)
    assert rc1 == ffi.E_NOSPACE and (offs1, lens1, used1, st1, total1) == (offs, lens, used, st, total)
    assert whole1 == bytes([SENTINEL]) * (total - 1 + GUARD)
    # the context is usable: the next call succeeds
    rc2, offs2, lens2, _u, st2, total2, whole2, _ = unpacked(ctx, ffi, torch, ffi.GZIP, streams, 8, cap=total, d_in=d_in)
    assert rc2 == ffi.OK and (offs2, lens2, st2, total2) == (offs, lens, st, total) and whole2[:total] == whole[:total]
    # the size query
    in_offs, in_lens = _offsets(streams), [len(s) for s in streams]
    rcq, offsq, lensq, usedq, stq, totalq = ctx.decode_batch_packed_device(ffi.GZIP, d_in.data_ptr(), in_offs, in_lens, None, 0, align=8)
    assert rcq == ffi.E_NOSPACE and (offsq, lensq, usedq, stq, totalq) == (offs, lens, used, st, total)
    with pytest.raises(ffi.LfxError) as e:
        ctx.decode_batch_packed_device(ffi.GZIP, d_in.data_ptr(), in_offs, in_lens, None, 1, align=8)
    assert e.value.status == ffi.E_ARG
    d_out = torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda")
    for align in (3, 8192, 0):
        with pytest.raises(ffi.LfxError) as e:
            ctx.decode_batch_packed_device(ffi.GZIP, d_in.data_ptr(), in_offs, in_lens, d_out.data_ptr(), total, align=align)
        assert e.value.status == ffi.E_ARG
    # both input forms, or neither
    pairs = torch.from_numpy(np.array([v for p in zip(in_offs, in_lens) for v in p], dtype=np.int64)).to("cuda")
    torch.cuda.synchronize()
    L, n = ffi.lib(), len(streams)
    t = C.c_uint64(0)
    call = lambda io, il, tab: L.lfx_decode_batch_packed_device(ctx.handle, ffi.GZIP, None, n, d_in.data_ptr(), io, il, tab, 8, d_out.data_ptr(),
                                                                total, None, None, None, None, C.byref(t), None)
    assert call(_arr(in_offs), _arr(in_lens), pairs.data_ptr()) == ffi.E_ARG
    assert call(None, None, None) == ffi.E_ARG
    assert call(_arr(in_offs), None, None) == ffi.E_ARG
    assert d_out.cpu().numpy().tobytes() == bytes([SENTINEL]) * total
    assert call(_arr(in_offs), _arr(in_lens), None) == ffi.OK and t.value == total       # (every result pointer NULL but total)
    # a dictionary with gzip, and count == 0
    with pytest.raises(ffi.LfxError) as e:
        d = lfx.Dictionary(D32, ctx)
        try:
            ctx.decode_batch_packed_device(ffi.GZIP, d_in.data_ptr(), in_offs, in_lens, d_out.data_ptr(), total, zdict=d)
        finally:
            d.close()
    assert e.value.status == ffi.E_ARG
    assert ctx.decode_batch_packed_device(ffi.GZIP, d_in.data_ptr(), [], [], d_out.data_ptr(), total) == (ffi.OK, [], [], [], [], 0)


# ---- 5. device tables ---------------------------------------------------------------------------------------------------------
def test_device_tables(ctx, ffi, lfx, torch):
    recs, streams = mixed(lfx, "zlib", 260)
    d_in = _dev(torch, b"".join(streams))
    host = unpacked(ctx, ffi, torch, ffi.ZLIB, streams, 8, d_in=d_in, table=True)
    dev = unpacked(ctx, ffi, torch, ffi.ZLIB, streams, 8, d_in=d_in, in_table=True)
    assert host[0] == dev[0] == ffi.OK and host[1:7] == dev[1:7]
    table = host[7]
    assert [int(x) for x in table[:, 0]] == host[1] and [int(x) for x in table[:, 1]] == [len(r) for r in recs]


@pytest.mark.parametrize("name", ["gzip", "deflate"])
def test_encode_then_decode_through_the_device_table(ctx, ffi, torch, name):
    fmt = _fmt(ffi, name)
    recs = [TEXT[1000 * i:1000 * i + n] for i, n in enumerate([KIB, 0, 70000, 5, 3 * KIB] * 53)][:259]
    d_rec = _dev(torch, b"".join(recs))
    in_offs, in_lens = _offsets(recs), [len(r) for r in recs]
    rc, comp_total, _ = ctx.encode_batch_packed_device(fmt, d_rec.data_ptr(), in_offs, in_lens, None, 0, align=8)
    assert rc == ffi.E_NOSPACE
    d_comp = torch.empty(comp_total, dtype=torch.uint8, device="cuda")
    d_table = torch.full((2 * len(recs),), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rc, _total, _layout = ctx.encode_batch_packed_device(fmt, d_rec.data_ptr(), in_offs, in_lens, d_comp.data_ptr(), comp_total, align=8,
                                                         d_table=d_table.data_ptr())
    assert rc == ffi.OK
    # from here on only the count and the table's address: no offset passes through these hands
    n, tab = len(recs), d_table.data_ptr()
    rc, _o, _l, _u, _s, total = ctx.decode_batch_packed_device(fmt, d_comp.data_ptr(), n, None, None, 0, d_in_table=tab)
    assert rc == ffi.E_NOSPACE and total == sum(in_lens)
    d_out = torch.full((total + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc, offs, lens, used, st, total = ctx.decode_batch_packed_device(fmt, d_comp.data_ptr(), n, None, d_out.data_ptr(), total, d_in_table=tab)
    assert rc == ffi.OK and all(s == ffi.OK for s in st) and lens == in_lens and offs == in_offs
    whole = d_out.cpu().numpy().tobytes()
    assert whole[:total] == b"".join(recs) and whole[total:] == bytes([SENTINEL]) * GUARD


# ---- 6. the Python modules --------------------------------------------------------------------------------------------------
def test_python_round_trips(lfx, ctx):
    recs = [TEXT[2000 * i:2000 * i + n] for i, n in enumerate((KIB, 0, 1, 70000, 300, 5 * KIB))]
    for mod in (lfx.gzip, lfx.zlib, lfx.deflate):
        assert mod.decompress_batch(mod.compress_batch(recs, context=ctx), context=ctx) == recs
        assert mod.decompress_batch([], context=ctx) == []
        for r in (recs[0], recs[1], recs[3]):
            assert mod.decompress(mod.compress(r, context=ctx), context=ctx) == r
    for mod in (lfx.zlib, lfx.deflate):
        assert mod.decompress_batch(mod.compress_batch(recs, zdict=D32, context=ctx), zdict=D32, context=ctx) == recs
        d = lfx.Dictionary(D32, ctx)
        try:
            assert mod.decompress_batch(mod.compress_batch(recs, zdict=d, context=ctx), zdict=d, context=ctx) == recs
            assert mod.decompress(mod.compress(recs[3], zdict=d, context=ctx), zdict=d, context=ctx) == recs[3]
        finally:
            d.close()
        assert mod.decompress(mod.compress(recs[0], zdict=D32, context=ctx), zdict=D32, context=ctx) == recs[0]
    assert lfx.zlib.decompress(pyzlib.compress(TEXT), context=ctx) == TEXT
    assert lfx.zlib.decompress_batch([pyzlib.compress(r) for r in recs], context=ctx) == recs


def test_python_damaged_record_raises_with_its_index(lfx, ctx):
    recs = [TEXT[3000 * i:3000 * i + 2 * KIB] for i in range(5)]
    for mod in (lfx.gzip, lfx.zlib, lfx.deflate):
        streams = mod.compress_batch(recs, context=ctx)
        streams[3] = streams[3][:len(streams[3]) // 2]
        with pytest.raises(mod.StreamError) as e:
            mod.decompress_batch(streams, context=ctx)
        assert "record 3" in str(e.value) and len(e.value.message) > len("record 3: ")
        with pytest.raises(mod.StreamError):
            mod.decompress(streams[3], context=ctx)
