"""GPU: the seek index (lfx_decode_index_device, lfx_index_read_device, export / import).  The build must equal
lfx_decode_device (status, out_len, consumed, message, bytes); every window must equal the bytes in front of its point; reads
must equal slices of the full decode (Python's zlib / gzip give the expected bytes) and write nothing else; a wrong input must
give LFX_E_INVALID_DATA."""
import ctypes as C
import gzip as pygzip
import random
import struct
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


def _own(ctx, ffi, fmt, data, write_size, **opts):
    return ctx.encode_host(fmt, bytes(data), ffi.make_opts(**opts), ffi.make_schedule(write_size))


def _raw(data, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def _bgzf(data, size=60000):
    out = b""
    for i in range(0, len(data), size):
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = c.compress(data[i:i + size]) + c.flush()
        hdr = b"\x1f\x8b\x08\x04" + b"\0" * 4 + b"\x00\xff" + struct.pack("<HBBHH", 6, 66, 67, 2, len(body) + 25)
        out += hdr + body + struct.pack("<II", zlib.crc32(data[i:i + size]), len(data[i:i + size]))
    return out


def build(ctx, ffi, torch, data, fmt, spacing=1 << 20, multi=False, cap=None):
    """the index build next to decode_device: the contract → (status, decoded bytes, index wrapper or None)"""
    from libflate_amd.index import Index
    n = len(data)
    cap = cap if cap is not None else max(1 << 16, 16 * n)
    d_in = _dev(torch, data)
    d_ref = torch.full((cap,), 0x5A, dtype=torch.uint8, device="cuda")
    d_idx = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda")
    flags = ffi.DEC_MULTI if multi else 0
    r = ctx.decode_device(fmt, d_in.data_ptr(), n, d_ref.data_ptr(), cap, flags=flags)
    rc, ol, used, h, msg = ctx.decode_index_device(fmt, d_in.data_ptr(), n, d_idx.data_ptr(), cap, spacing, flags)
    torch.cuda.synchronize()
    assert (rc, ol, used, msg) == r
    out = d_idx[:ol].cpu().numpy().tobytes()
    assert out == d_ref[:r[1]].cpu().numpy().tobytes()
    if rc != ffi.OK:
        assert h is None
        return rc, out, None
    return rc, out, Index(h, ctx)


def check_points(idx, out, spacing, gap_bound=True):
    info = idx.info
    pts = idx.points
    assert info["n_points"] == len(pts) and info["out_len"] == len(out)
    assert pts[0][2] == 0 and pts[0][4] == 0
    starts = {}
    for (in_bit, hdr_bit, out_off, member, win_len, _crc, btype) in pts:
        starts.setdefault(member, out_off)
        assert hdr_bit <= in_bit and btype <= 2
        assert win_len == min(32768, out_off - starts[member])
    if gap_bound:
        assert info["max_gap"] <= spacing, (info["max_gap"], spacing)
    return pts


def windows_match(ctx, idx, out):
    """every window of the exported index equals the decoded bytes in front of its point"""
    blob = idx.to_bytes()
    n = idx.info["n_points"]
    at = 64 + 40 * n
    for (_b, _h, out_off, _m, win_len, _c, _t) in idx.points:
        assert blob[at:at + win_len] == out[out_off - win_len:out_off]
        at += win_len
    assert at + 4 == len(blob)


def reads_match(ctx, ffi, torch, idx, data, out, n_reads=2000, seed=1):
    rnd = random.Random(seed)
    ol = len(out)
    pts = [p[2] for p in idx.points]
    ranges = [(0, ol), (ol, 5), (0, 0), (ol - 1 if ol else 0, 1), (max(ol - 1000, 0), 1000)]
    for p in pts[1:6]:
        ranges += [(max(p - 100, 0), 200), (p, 1)]
    while len(ranges) < n_reads:
        o = rnd.randrange(ol + 1)
        ranges.append((o, rnd.choice([0, 1, 17, 4096, 65536, 300000])))
    got = idx.read_many(data, ranges)
    for (o, ln), g in zip(ranges, got):
        assert g.cpu().numpy().tobytes() == out[o:o + ln], (o, ln)
    # a start past the end is LFX_E_ARG for that read, the others still OK
    d_in = _dev(torch, data)
    d_out = torch.full((64,), 0x33, dtype=torch.uint8, device="cuda")
    rc, lens, st, _ = ctx.index_read_device(idx._h, d_in.data_ptr(), 0, len(data), [ol + 1, 0], [4, 8], d_out.data_ptr(), [0, 8])
    assert rc == ffi.E_ARG and st == [ffi.E_ARG, ffi.OK] and lens == [0, min(8, ol)]


def partial_input_from_inside_a_block(ctx, ffi, torch, idx, comp, out):
    """reads that start at and behind a point inside a block, from an input buffer that holds exactly lfx_index_span (it must
    reach back to the block's header); a buffer one byte shorter at either end is LFX_E_ARG"""
    inner = [p for p in idx.points if p[0] != p[1]]
    assert inner
    for (in_bit, hdr_bit, out_off, *_r) in (inner[len(inner) // 2], inner[-1]):
        for o, ln in ((out_off, 5000), (out_off + 777, 70000)):
            if o >= len(out):               # (a point in the last 777 bytes of a short output)
                continue
            ln = min(ln, len(out) - o)
            lo, hi = idx.span(o, ln)
            assert lo == hdr_bit // 8 and lo < in_bit // 8
            part = comp[lo:hi]
            assert idx.read(part, o, ln, in_base=lo).cpu().numpy().tobytes() == out[o:o + ln]
            d_o = torch.zeros(max(ln, 1), dtype=torch.uint8, device="cuda")
            for base, held in ((lo + 1, part[1:]), (lo, part[:-1])):
                d_part = _dev(torch, held)
                rc, lens, st, _m = ctx.index_read_device(idx._h, d_part.data_ptr(), base, len(held), [o], [ln], d_o.data_ptr(), [0])
                assert rc == ffi.E_ARG and st == [ffi.E_ARG] and lens == [0]


def test_own_gzip_s8k(ctx, ffi, torch, synth):
    data = synth.text(64 * MIB).tobytes()
    comp = _own(ctx, ffi, ffi.GZIP, data, 8192)
    for spacing in (1 * MIB, 256 * KIB):
        rc, out, idx = build(ctx, ffi, torch, comp, ffi.GZIP, spacing)
        assert rc == ffi.OK and out == data
        check_points(idx, out, spacing)
        if spacing == MIB:
            windows_match(ctx, idx, out)
            reads_match(ctx, ffi, torch, idx, comp, out)
        idx.close()


def test_s1_one_block(ctx, ffi, torch, synth):
    data = synth.text(32 * MIB).tobytes()
    comp = _own(ctx, ffi, ffi.GZIP, data, 0)
    for spacing in (1 * MIB, 256 * KIB):
        rc, out, idx = build(ctx, ffi, torch, comp, ffi.GZIP, spacing)
        assert rc == ffi.OK and out == data
        pts = check_points(idx, out, spacing)
        assert any(p[0] != p[1] for p in pts), "no point inside the single block"
        if spacing == 256 * KIB:
            windows_match(ctx, idx, out)
            reads_match(ctx, ffi, torch, idx, comp, out)
            partial_input_from_inside_a_block(ctx, ffi, torch, idx, comp, out)
        idx.close()


@pytest.mark.parametrize("level", [1, 6, 9])
def test_python_zlib(ctx, ffi, torch, synth, level):
    data = synth.text(12 * MIB).tobytes()
    for fmt, comp in ((ffi.DEFLATE, _raw(data, level)), (ffi.ZLIB, zlib.compress(data, level))):
        rc, out, idx = build(ctx, ffi, torch, comp, fmt, 1 * MIB)
        assert rc == ffi.OK and out == data
        check_points(idx, out, 1 * MIB)
        if fmt == ffi.DEFLATE:
            rc2, _o, idx2 = build(ctx, ffi, torch, comp, fmt, 256 * KIB)
            check_points(idx2, out, 256 * KIB)
            idx2.close()
        windows_match(ctx, idx, out)
        reads_match(ctx, ffi, torch, idx, comp, out, seed=level)
        idx.close()


def test_fixed_and_stored(ctx, ffi, torch, synth):
    data = synth.text(3 * MIB).tobytes()
    for opts in (dict(dynamic_huffman=0), dict(no_compression=1)):
        comp = _own(ctx, ffi, ffi.GZIP, data, 8192, **opts)
        rc, out, idx = build(ctx, ffi, torch, comp, ffi.GZIP, 64 * KIB)
        assert rc == ffi.OK and out == data
        check_points(idx, out, 64 * KIB, gap_bound=False)
        windows_match(ctx, idx, out)
        reads_match(ctx, ffi, torch, idx, comp, out)
        idx.close()


def test_bgzf_multi(ctx, ffi, torch, synth):
    data = synth.text(8 * MIB).tobytes()
    comp = _bgzf(data)
    rc, out, idx = build(ctx, ffi, torch, comp, ffi.GZIP, 64 * KIB, multi=True)
    assert rc == ffi.OK and out == data
    pts = check_points(idx, out, 64 * KIB, gap_bound=False)
    assert idx.info["n_members"] == (len(data) + 59999) // 60000
    member_starts = {p[3]: p[2] for p in reversed(pts)}
    assert sorted(member_starts.values()) == list(range(0, len(data), 60000))
    windows_match(ctx, idx, out)
    reads_match(ctx, ffi, torch, idx, comp, out, n_reads=2000)
    idx.close()


def test_damaged_streams_give_no_index(ctx, ffi, torch, synth):
    data = synth.text(4 * MIB).tobytes()
    comp = _own(ctx, ffi, ffi.GZIP, data, 8192)
    rc, _o, idx = build(ctx, ffi, torch, comp[:len(comp) // 2], ffi.GZIP)
    assert rc != ffi.OK and idx is None
    bad = bytearray(comp)
    bad[len(bad) // 3] ^= 0x10
    rc, _o, idx = build(ctx, ffi, torch, bytes(bad), ffi.GZIP)
    assert rc != ffi.OK and idx is None


def test_many_reads_sentinel_span_persistence_wrong_input(ctx, ffi, torch, synth):
    from libflate_amd.index import Index
    data = synth.text(32 * MIB).tobytes()
    comp = _own(ctx, ffi, ffi.GZIP, data, 8192)
    rc, out, idx = build(ctx, ffi, torch, comp, ffi.GZIP, 1 * MIB)
    assert rc == ffi.OK
    rnd = random.Random(7)
    ol = len(out)
    # 4096 ranges in one call; bytes of d_out outside the requested outputs keep the sentinel
    ranges = [(rnd.randrange(ol), 4096) for _ in range(4096)]
    d_in = _dev(torch, comp)
    stride = 8192
    d_out = torch.full((4096 * stride,), 0x7E, dtype=torch.uint8, device="cuda")
    rc, lens, st, msg = ctx.index_read_device(idx._h, d_in.data_ptr(), 0, len(comp), [o for o, _ in ranges], [ln for _, ln in ranges],
                                              d_out.data_ptr(), [i * stride for i in range(4096)])
    assert rc == ffi.OK, msg
    h = d_out.cpu().numpy().tobytes()
    for i, (o, ln) in enumerate(ranges):
        assert h[i * stride:i * stride + lens[i]] == out[o:o + ln]
        assert h[i * stride + lens[i]:(i + 1) * stride] == b"\x7e" * (stride - lens[i])
    # a partial input that holds exactly the span
    o, ln = ol // 2, 100000
    lo, hi = idx.span(o, ln)
    part = comp[lo:hi]
    assert idx.read(part, o, ln, in_base=lo).cpu().numpy().tobytes() == out[o:o + ln]
    d_part = _dev(torch, part[:-1])
    d_o = torch.zeros(ln, dtype=torch.uint8, device="cuda")
    rc, _l, st, _m = ctx.index_read_device(idx._h, d_part.data_ptr(), lo, hi - lo - 1, [o], [ln], d_o.data_ptr(), [0])
    assert rc == ffi.E_ARG and st == [ffi.E_ARG]
    # persistence: deterministic export, an imported index reads the same bytes
    blob = idx.to_bytes()
    _rc, _o2, idx_b = build(ctx, ffi, torch, comp, ffi.GZIP, 1 * MIB)
    assert idx_b.to_bytes() == blob
    assert Index.check(blob)["n_points"] == idx.info["n_points"]
    idx_c = Index.from_bytes(blob, ctx)
    some = [(rnd.randrange(ol), 70000) for _ in range(64)]
    for (a, ln), g in zip(some, idx_c.read_many(comp, some)):
        assert g.cpu().numpy().tobytes() == out[a:a + ln]
    # another stream of the same length, and one flipped bit inside a segment
    other = bytearray(comp)
    other[64:len(comp) - 64] = bytes(reversed(other[64:len(comp) - 64]))
    d_other = _dev(torch, bytes(other))
    pts = idx.points
    mid = pts[len(pts) // 2]
    d_o = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    rc, _l, st, msg = ctx.index_read_device(idx._h, d_other.data_ptr(), 0, len(comp), [mid[2]], [4096], d_o.data_ptr(), [0])
    assert rc == ffi.E_INVALID_DATA and "index point" in msg
    flip = bytearray(comp)
    nxt = pts[len(pts) // 2 + 1]
    flip[(mid[0] + nxt[0]) // 16] ^= 0x04
    d_flip = _dev(torch, bytes(flip))
    seg_len = nxt[2] - mid[2]
    d_o = torch.zeros(seg_len, dtype=torch.uint8, device="cuda")
    rc, _l, st, msg = ctx.index_read_device(idx._h, d_flip.data_ptr(), 0, len(comp), [mid[2]], [seg_len], d_o.data_ptr(), [0])
    assert rc == ffi.E_INVALID_DATA and "index point" in msg
    for x in (idx, idx_b, idx_c):
        x.close()
