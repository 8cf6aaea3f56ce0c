"""GPU: lfx_decode_members_device / _host — gzip::MultiDecoder (src/gzip.rs:1052-1167) with the members found on the device and
decoded as one batch.  Every case asserts the full contract against the sequential member loop,
ctx.decode_device(GZIP, ..., flags=DEC_MULTI) — status, out_len, consumed, message and the bytes in front of out_len — and
against the oracle's MultiDecoder (status, bytes, consumed)."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_parity import ctx, ffi, lfx, synth  # noqa: F401  (fixtures)

KIB = 1 << 10
MIB = 1 << 20
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def _dev(torch, data):
    a = np.frombuffer(bytes(data), dtype=np.uint8).copy() if len(data) else np.zeros(1, dtype=np.uint8)
    return torch.from_numpy(a).to("cuda")


def check(ctx, ffi, oracle, torch, data, cap=None, want_status=None):
    """both device paths on `data`; the contract; the oracle → (status, out bytes, consumed, members)"""
    data = bytes(data)
    n = len(data)
    o_rc, o_out, o_used, _ = oracle.decode(oracle.GZIP, data, multi=True)
    if cap is None:
        cap = max(2 * len(o_out), 1 << 16)
    d_in = _dev(torch, data)
    d_seq = torch.full((max(cap, 1),), 0x5A, dtype=torch.uint8, device="cuda")
    d_mem = torch.full((max(cap, 1),), 0xA5, dtype=torch.uint8, device="cuda")
    s_rc, s_len, s_used, s_msg = ctx.decode_device(ffi.GZIP, d_in.data_ptr(), n, d_seq.data_ptr(), cap, flags=ffi.DEC_MULTI)
    m_rc, m_len, m_used, members, m_msg = ctx.decode_members_device(d_in.data_ptr(), n, d_mem.data_ptr(), cap)
    torch.cuda.synchronize()
    assert (m_rc, m_len, m_used, m_msg) == (s_rc, s_len, s_used, s_msg)
    out = d_mem[:m_len].cpu().numpy().tobytes()
    assert out == d_seq[:s_len].cpu().numpy().tobytes()
    if want_status is not None:
        assert m_rc == want_status, (m_rc, m_msg)
    # the member table: in order, contiguous from byte 0 / output byte 0, inside what was consumed and produced
    at, oat = 0, 0
    for (i_off, i_len, o_off, o_len) in members:
        assert (i_off, o_off) == (at, oat)
        at, oat = i_off + i_len, o_off + o_len
    assert at <= m_used and oat <= m_len
    if m_rc == ffi.OK:
        assert oat == m_len
    if cap >= 2 * len(o_out):      # (the oracle has no capacity limit)
        assert (m_rc, m_used) == (o_rc, o_used)
        if m_rc == ffi.OK:
            assert out == o_out
        else:                      # the verified members' bytes (a failing member's partial output is the sequential loop's)
            assert out[:oat] == o_out[:oat]
    return m_rc, out, m_used, members


def batch_encoded(ctx, ffi, torch, synth, count, size, seed):
    """`count` gzip members of `size` TEXT bytes each from ONE lfx_encode_batch_device call, concatenated"""
    L = ffi.lib()
    plain = synth.text(count * size, seed=seed)
    d_plain = torch.from_numpy(plain).to("cuda")
    opts, sched = ffi.make_opts(), ffi.make_schedule(0)
    bound = (L.lfx_encode_bound(size, C.byref(opts), C.byref(sched)) + 3) & ~3
    d_streams = torch.zeros(count * bound, dtype=torch.uint8, device="cuda")
    in_off = np.arange(count, dtype=np.uint64) * np.uint64(size)
    in_len = np.full(count, size, dtype=np.uint64)
    out_off = np.arange(count, dtype=np.uint64) * np.uint64(bound)
    out_cap = np.full(count, bound, dtype=np.uint64)
    out_len = np.zeros(count, dtype=np.uint64)
    status = np.zeros(count, dtype=np.int32)
    rc = L.lfx_encode_batch_device(ctx.handle, ffi.GZIP, C.byref(opts), C.byref(sched), count, d_plain.data_ptr(), in_off.ctypes.data,
                                   in_len.ctypes.data, d_streams.data_ptr(), out_off.ctypes.data, out_cap.ctypes.data,
                                   out_len.ctypes.data, status.ctypes.data)
    assert rc == 0 and not status.any(), ctx.last_error()
    host = d_streams.cpu().numpy()
    data = b"".join(host[i * bound:i * bound + int(out_len[i])].tobytes() for i in range(count))
    return plain.tobytes(), data, [int(x) for x in out_len]


def zmember(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, bgzf=False, flags=0, name=None, comment=None, extra=None):
    """a python-zlib gzip member; bgzf: the BGZF `BC` extra field (BSIZE = member length - 1)"""
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    body = co.compress(raw) + co.flush()
    trailer = struct.pack("<II", zlib.crc32(raw) & 0xFFFFFFFF, len(raw) & 0xFFFFFFFF)
    if bgzf:
        size = 12 + 6 + len(body) + 8
        return b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<HBBHH", 6, 66, 67, 2, size - 1) + body + trailer
    flg = flags
    hdr = b""
    if extra is not None:
        flg |= 4
        hdr += struct.pack("<H", len(extra)) + extra
    if name is not None:
        flg |= 8
        hdr += name + b"\0"
    if comment is not None:
        flg |= 16
        hdr += comment + b"\0"
    return bytes([0x1F, 0x8B, 8, flg, 0, 0, 0, 0, 0, 3]) + hdr + body + trailer


def small_members(synth, count, size, seed):
    plain = synth.text(count * size, seed=seed).tobytes()
    return plain, b"".join(zmember(plain[i * size:(i + 1) * size], bgzf=True) for i in range(count))


# ------------------------------------------------------------------------------------------------ clean inputs
def test_4096_batch_encoded_members_table(ctx, ffi, oracle, torch, synth):
    count, size = 4096, 64 * KIB
    plain, data, lens = batch_encoded(ctx, ffi, torch, synth, count, size, synth.SEED_BASE + 71)
    rc, out, used, members = check(ctx, ffi, oracle, torch, data, want_status=ffi.OK)
    assert out == plain and used == len(data)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(int)
    assert members == [(int(offs[i]), lens[i], i * size, size) for i in range(count)]


def test_bgzf_python_zlib_members_with_eof_block(ctx, ffi, oracle, torch, synth):
    plain, data = small_members(synth, 300, 60 * KIB, synth.SEED_BASE + 72)
    data += BGZF_EOF
    rc, out, used, members = check(ctx, ffi, oracle, torch, data, want_status=ffi.OK)
    assert out == plain and used == len(data) and len(members) == 301
    assert members[-1] == (len(data) - 28, 28, len(plain), 0)


def test_header_fields_fixed_and_stored_members(ctx, ffi, oracle, torch, synth):
    text = synth.text(200 * KIB, seed=synth.SEED_BASE + 73).tobytes()
    parts, want = [], b""
    for i in range(6):
        raw = text[i * 30 * KIB:(i + 1) * 30 * KIB]
        want += raw
        kw = [dict(filename=b"member-%d.txt" % i), dict(comment=b"a comment"), dict(extra=b"AB\x03\x00xyz", hcrc=1),
              dict(filename=b"n", comment=b"c", extra=b"CD\x00\x00", hcrc=1), dict(dynamic_huffman=0), dict(no_compression=1)][i]
        parts.append(ctx.encode_host(ffi.GZIP, raw, ffi.make_opts(**kw), ffi.make_schedule(0)))
    raw = text[180 * KIB:]
    want += raw + raw + raw
    parts.append(zmember(raw, strategy=zlib.Z_FIXED, name=b"fixed", comment=b"huffman"))
    parts.append(zmember(raw, level=0, extra=b"ZZ\x01\x00q"))
    parts.append(zmember(raw, flags=0, name=b"plain"))
    rc, out, used, members = check(ctx, ffi, oracle, torch, b"".join(parts), want_status=ffi.OK)
    assert out == want and len(members) == len(parts)


def test_stored_member_holding_a_gzip_file(ctx, ffi, oracle, torch, synth):
    """false candidates that parse and walk cleanly: the payload of a stored member is itself a complete gzip file"""
    inner_plain, inner = small_members(synth, 4, 8 * KIB, synth.SEED_BASE + 74)
    outer = ctx.encode_host(ffi.GZIP, inner, ffi.make_opts(no_compression=1), ffi.make_schedule(0))
    tail_plain, tail = small_members(synth, 8, 16 * KIB, synth.SEED_BASE + 75)
    rc, out, used, members = check(ctx, ffi, oracle, torch, outer + tail + outer, want_status=ffi.OK)
    assert out == inner + tail_plain + inner and len(members) == 10


def test_long_members_in_between(ctx, ffi, oracle, torch, synth):
    """a 64 MiB member of the project's encoder and an 8 MiB python-zlib member take the long path"""
    big = synth.text(64 * MIB, seed=synth.SEED_BASE + 76)
    d_big = torch.from_numpy(big).to("cuda")
    opts, sched = ffi.make_opts(), ffi.make_schedule(0)
    bound = ffi.lib().lfx_encode_bound(big.size, C.byref(opts), C.byref(sched))
    d_enc = torch.zeros(bound, dtype=torch.uint8, device="cuda")
    m = ctx.encode_device(ffi.GZIP, d_big.data_ptr(), big.size, d_enc.data_ptr(), bound, opts, sched)
    big_member = d_enc[:m].cpu().numpy().tobytes()
    mid = synth.text(8 * MIB, seed=synth.SEED_BASE + 77).tobytes()
    p1, s1 = small_members(synth, 16, 64 * KIB, synth.SEED_BASE + 78)
    p2, s2 = small_members(synth, 16, 64 * KIB, synth.SEED_BASE + 79)
    data = s1 + big_member + s2 + zmember(mid) + s1
    rc, out, used, members = check(ctx, ffi, oracle, torch, data, want_status=ffi.OK)
    assert out == p1 + big.tobytes() + p2 + mid + p1 and len(members) == 50


# ------------------------------------------------------------------------------------------------ damage and limits
@pytest.fixture(scope="module")
def plain64(synth):
    return small_members(synth, 64, 64 * KIB, synth.SEED_BASE + 80)


def _starts(data):
    m, at = [], 0
    while at < len(data):
        m.append(at)
        at += struct.unpack_from("<H", data, at + 16)[0] + 1
    return m


def test_crc_flip_in_member_k(ctx, ffi, oracle, torch, plain64):
    plain, data = plain64
    starts = _starts(data)
    for k in (0, 17, 63):
        end = starts[k + 1] if k + 1 < len(starts) else len(data)
        bad = bytearray(data)
        bad[end - 8] ^= 0x40
        rc, out, used, members = check(ctx, ffi, oracle, torch, bytes(bad), want_status=ffi.E_INVALID_DATA)
        assert len(members) == k and used == end


def test_truncated_last_member(ctx, ffi, oracle, torch, plain64):
    plain, data = plain64
    last = _starts(data)[-1]
    for cut in (len(data) - 1, len(data) - 9, (last + len(data)) // 2):
        rc, out, used, members = check(ctx, ffi, oracle, torch, data[:cut])
        assert rc != ffi.OK and len(members) == 63
    # a cut inside the last member's header: UnexpectedEof on the next header is the clean end (gzip.rs:1150-1156)
    rc, out, used, members = check(ctx, ffi, oracle, torch, data[:last + 5], want_status=ffi.OK)
    assert used == last + 5 and len(members) == 63


def test_trailing_garbage_partial_header_zero_padding(ctx, ffi, oracle, torch, plain64):
    plain, data = plain64
    check(ctx, ffi, oracle, torch, data + b"garbage after the last member", want_status=ffi.E_INVALID_DATA)
    rc, out, used, members = check(ctx, ffi, oracle, torch, data + data[:5], want_status=ffi.OK)   # UnexpectedEof on the next header
    assert used == len(data) + 5 and out == plain and len(members) == 64
    check(ctx, ffi, oracle, torch, data + bytes(4))
    check(ctx, ffi, oracle, torch, data + bytes(4096))


def test_empty_input(ctx, ffi, oracle, torch):
    rc, out, used, members = check(ctx, ffi, oracle, torch, b"", want_status=ffi.E_UNEXPECTED_EOF)
    assert out == b"" and members == []


def test_output_capacity(ctx, ffi, oracle, torch, plain64):
    plain, data = plain64
    rc, out, used, members = check(ctx, ffi, oracle, torch, data, cap=len(plain) - 1, want_status=ffi.E_NOSPACE)
    assert len(members) == 63
    k = 20
    check(ctx, ffi, oracle, torch, data, cap=k * 64 * KIB + 1000, want_status=ffi.E_NOSPACE)
    check(ctx, ffi, oracle, torch, data, cap=k * 64 * KIB)   # (the capacity ends between two members)
    rc, out, used, members = check(ctx, ffi, oracle, torch, data, cap=len(plain), want_status=ffi.OK)
    assert out == plain


def test_dense_candidates_in_a_stored_member(ctx, ffi, oracle, torch, synth):
    """1 MiB of repeated magic inside a stored member, normal members behind it: bounded work, same answer"""
    dense = (b"\x1f\x8b\x08\x00" * (MIB // 4))
    stored = ctx.encode_host(ffi.GZIP, dense, ffi.make_opts(no_compression=1), ffi.make_schedule(0))
    plain, tail = small_members(synth, 32, 64 * KIB, synth.SEED_BASE + 81)
    rc, out, used, members = check(ctx, ffi, oracle, torch, stored + tail + stored, want_status=ffi.OK)
    assert out == dense + plain + dense and len(members) == 34


# ------------------------------------------------------------------------------------------------ host variant, one member
def test_host_variant_pageable_and_page_locked(ctx, ffi, oracle, plain64, lfx):
    plain, data = plain64
    data = data + BGZF_EOF
    rc, out, used, members, msg = ctx.decode_members_host(data)
    assert (rc, out, used) == (0, plain, len(data)) and len(members) == 65
    assert ctx.decode_host(ffi.GZIP, data, flags=ffi.DEC_MULTI)[:3] == (rc, out, used)
    assert lfx.gzip.decode_members(data, context=ctx) == (plain, members)
    with pytest.raises(lfx.gzip.StreamError):
        lfx.gzip.decode_members(data + b"junk" * 4, context=ctx)   # (fewer than ten bytes would be the clean end)
    L = ffi.lib()
    h_in = L.lfx_host_alloc(len(data))
    h_out = L.lfx_host_alloc(len(plain) + 4096)
    assert h_in and h_out
    try:
        C.memmove(h_in, data, len(data))
        ol, cons, cnt = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
        table = (ffi.Member * 8)()
        rc = L.lfx_decode_members_host(ctx.handle, h_in, len(data), h_out, len(plain) + 4096, C.byref(ol), C.byref(cons), table, 8,
                                       C.byref(cnt))
        assert (rc, ol.value, cons.value, cnt.value) == (0, len(plain), len(data), 65)
        assert C.string_at(h_out, ol.value) == plain
        assert [(m.in_off, m.in_len, m.out_off, m.out_len) for m in table] == members[:8]
        # a truncated input: the sequential loop's verdict, partial bytes included
        cut = len(data) - 1000
        rc = L.lfx_decode_members_host(ctx.handle, h_in, cut, h_out, len(plain) + 4096, C.byref(ol), C.byref(cons), None, 0,
                                       C.byref(cnt))
        want = ctx.decode_host(ffi.GZIP, data[:cut], cap=len(plain) + 4096, flags=ffi.DEC_MULTI)
        assert (rc, C.string_at(h_out, ol.value), cons.value) == want[:3] and cnt.value == 63
    finally:
        L.lfx_host_free(h_in)
        L.lfx_host_free(h_out)


def test_one_member_equals_decode_device(ctx, ffi, oracle, torch, synth):
    raw = synth.text(3 * MIB, seed=synth.SEED_BASE + 82).tobytes()
    data = ctx.encode_host(ffi.GZIP, raw, ffi.make_opts(), ffi.make_schedule(8192))
    rc, out, used, members = check(ctx, ffi, oracle, torch, data, want_status=ffi.OK)
    d_in = _dev(torch, data)
    d_out = torch.zeros(len(raw), dtype=torch.uint8, device="cuda")
    assert ctx.decode_device(ffi.GZIP, d_in.data_ptr(), len(data), d_out.data_ptr(), len(raw))[:3] == (rc, len(out), used)
    assert out == raw and members == [(0, len(data), 0, len(raw))]
