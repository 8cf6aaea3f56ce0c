"""GPU: lfx_encode_members_device / _host — one buffer as back-to-back gzip members or BGZF, encoded in one pass and packed at
the members' final offsets.  The expected bytes are the model of tests/test_members_encode_abi.py (the oracle's gzip stream per
slice; BGZF: BC subfield, BSIZE, the stored form above 65536 bytes, the end-of-file marker), proved there without a GPU."""
import ctypes as C
import gzip as pygzip
import struct
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_parity import ctx, ffi, lfx, synth  # noqa: F401  (fixtures)
from test_members_encode_abi import (BGZF_CASES, BGZF_EOF, gzi_model, mixed, model_bgzf, model_plain, random_bytes, walk_bsize,
                                     words_text)

KIB = 1 << 10
MIB = 1 << 20
GUARD = 4096


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def _dev(torch, data):
    a = np.frombuffer(bytes(data), dtype=np.uint8).copy() if len(data) else np.zeros(1, dtype=np.uint8)
    return torch.from_numpy(a).to("cuda")


def bound_of(ffi, n, member_size, flags, opts, sched):
    return ffi.lib().lfx_encode_members_bound(n, member_size, flags, C.byref(opts) if opts is not None else None,
                                              C.byref(sched) if sched is not None else None)


def run_device(ctx, ffi, torch, data, member_size, flags=0, opts=None, sched=None, cap=None, max_members=None):
    """→ (status, bytes in front of out_len, n_members, members, message, whole buffer with its guard)"""
    n = len(data)
    if cap is None:
        cap = bound_of(ffi, n, member_size, flags, opts, sched)
    d_in = _dev(torch, data)
    d_out = torch.full((cap + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    assert d_out.data_ptr() % 4 == 0
    rc, out_len, count, members, msg = ctx.encode_members_device(d_in.data_ptr(), n, d_out.data_ptr(), cap, member_size, flags, opts,
                                                                 sched, max_members)
    torch.cuda.synchronize()
    whole = d_out.cpu().numpy().tobytes()
    assert whole[cap:] == b"\xA5" * GUARD, "bytes behind cap were written"
    return rc, whole[:out_len], count, members, msg, whole


def check_table(ffi, data, out, members, member_size, bgzf):
    """the member table agrees with the input's slices and with the bytes"""
    n = len(data)
    want_count = 0 if (bgzf and n == 0) else max(1, -(-n // member_size))
    assert len(members) == want_count
    at = 0
    for i, (i_off, i_len, o_off, o_len) in enumerate(members):
        assert i_off == i * member_size and i_len == min(member_size, n - i_off)
        assert o_off == at
        m = out[o_off:o_off + o_len]
        assert m[:3] == b"\x1f\x8b\x08"
        assert struct.unpack("<II", m[-8:]) == (zlib.crc32(data[i_off:i_off + i_len]), i_len)
        if bgzf:
            assert struct.unpack_from("<H", m, 16)[0] + 1 == o_len
        at += o_len
    assert at + (28 if bgzf else 0) == len(out)


def check_decodes(ctx, ffi, lfx, torch, data, out, members, bgzf):
    """Python's gzip, gzip.decode_members and lfx_decode_members_device read it back; the decoder's member table is the
    encoder's with in and out swapped (BGZF: the marker decodes as one more, empty member)"""
    assert pygzip.decompress(out) == data
    got, dec_members = lfx.gzip.decode_members(out)
    assert got == data
    want = [(o_off, o_len, i_off, i_len) for (i_off, i_len, o_off, o_len) in members]
    if bgzf:
        want.append((len(out) - 28, 28, len(data), 0))
    assert dec_members == want
    d_in = _dev(torch, out)
    cap = max(len(data), 1 << 16)
    d_out = torch.zeros((cap,), dtype=torch.uint8, device="cuda")
    rc, o_len, used, dm, msg = ctx.decode_members_device(d_in.data_ptr(), len(out), d_out.data_ptr(), cap)
    assert (rc, o_len, used) == (ffi.OK, len(data), len(out)), msg
    assert dm == want


def full_check(ctx, ffi, lfx, torch, data, want, want_table, member_size, flags, opts=None, sched=None):
    rc, out, count, members, msg, _ = run_device(ctx, ffi, torch, data, member_size, flags, opts, sched)
    assert rc == ffi.OK, msg
    assert len(out) == len(want)
    if out != want:
        at = next(i for i in range(len(want)) if out[i] != want[i])
        raise AssertionError("first difference at byte %d of %d (member table %r)" % (at, len(want), members[:3]))
    assert count == len(want_table) and members == want_table
    bgzf = bool(flags & ffi.MEMBERS_BGZF)
    check_table(ffi, data, out, members, member_size, bgzf)
    check_decodes(ctx, ffi, lfx, torch, data, out, members, bgzf)
    assert ffi.members_to_gzi(members) == gzi_model(want_table)
    return out, members


# ---------------------------------------------------------------------------------------------- plain mode
@pytest.mark.parametrize("member_size", [4096, 65536, MIB, 3 * MIB + 1, 64 * MIB])
@pytest.mark.parametrize("write_size", [0, 8192])
def test_plain_equals_concatenated_oracle_streams(ctx, ffi, lfx, torch, oracle, synth, member_size, write_size):
    data = synth.text(7 * MIB + 12345).tobytes() if member_size >= MIB else words_text(300 * 1000) + random_bytes(30000)
    want, table = model_plain(oracle, data, member_size, write_size=write_size)
    full_check(ctx, ffi, lfx, torch, data, want, table, member_size, 0, ffi.make_opts(), ffi.make_schedule(write_size))


@pytest.mark.parametrize("kw", [dict(dynamic_huffman=0), dict(no_compression=1), dict(window_size=1024), dict(max_length=16),
                                dict(filename=b"members.txt"), dict(filename=b"f" * 700, comment=b"long header", hcrc=1),
                                dict(block_size=10000)],
                         ids=["fixed", "stored", "window", "max_length", "filename", "long_header", "block_size"])
def test_plain_options(ctx, ffi, lfx, torch, oracle, kw):
    data = words_text(200 * 1000, seed=5) + random_bytes(70000, seed=5)
    for member_size in (30000, 65536):
        want, table = model_plain(oracle, data, member_size, **kw)
        full_check(ctx, ffi, lfx, torch, data, want, table, member_size, 0, ffi.make_opts(**kw), None)


@pytest.mark.parametrize("n,member_size", [(0, 4096), (1, 4096), (4095, 4096), (4096, 4096), (4097, 4096), (65537, 65536),
                                           (3, 1), (100, 7)])
def test_plain_odd_lengths(ctx, ffi, lfx, torch, oracle, n, member_size):
    data = words_text(n, seed=9) if n else b""
    want, table = model_plain(oracle, data, member_size)
    full_check(ctx, ffi, lfx, torch, data, want, table, member_size, 0)


# ---------------------------------------------------------------------------------------------- BGZF
@pytest.mark.parametrize("name,make,member_size", BGZF_CASES, ids=[c[0] for c in BGZF_CASES])
def test_bgzf_equals_model(ctx, ffi, lfx, torch, oracle, name, make, member_size):
    data = make()
    want, table, fallbacks = model_bgzf(oracle, data, member_size)
    if name == "mixed":
        assert 0 < fallbacks < len(table)
    out, members = full_check(ctx, ffi, lfx, torch, data, want, table, member_size, ffi.MEMBERS_BGZF)
    assert walk_bsize(out) == [m[3] for m in members] + [28]


def test_bgzf_options_and_small_blocks(ctx, ffi, lfx, torch, oracle):
    data = mixed(seed=11)
    for kw, member_size in ((dict(dynamic_huffman=0), 65505), (dict(no_compression=1), 65505), (dict(block_size=4096), 65500),
                            (dict(mtime=1234567, os=255, is_text=1), 65505), (dict(window_size=512, max_length=8), 40000)):
        want, table, _ = model_bgzf(oracle, data, member_size, **kw)
        full_check(ctx, ffi, lfx, torch, data, want, table, member_size, ffi.MEMBERS_BGZF, ffi.make_opts(**kw))
    for n, member_size in ((1, 65280), (65505, 65505), (65506, 65505), (10, 1)):
        d = random_bytes(n, seed=13)
        want, table, _ = model_bgzf(oracle, d, member_size)
        full_check(ctx, ffi, lfx, torch, d, want, table, member_size, ffi.MEMBERS_BGZF)


def test_bgzf_64mib_text(ctx, ffi, lfx, torch, oracle, synth):
    data = synth.text(64 * MIB).tobytes()
    want, table, fallbacks = model_bgzf(oracle, data, 65280)
    assert fallbacks == 0 and len(table) == -(-64 * MIB // 65280)
    full_check(ctx, ffi, lfx, torch, data, want, table, 65280, ffi.MEMBERS_BGZF)


def test_bgzf_option_errors_name_the_field(ctx, ffi, torch):
    data = words_text(1000)
    B = ffi.MEMBERS_BGZF
    cases = [("member_size", dict(), None, 0, B), ("member_size", dict(), None, 65506, B), ("member_size", dict(), None, 0, 0),
             ("extra", dict(extra=b"AB\x01\x00x"), None, 65280, B), ("filename", dict(filename=b"f"), None, 65280, B),
             ("comment", dict(comment=b"c"), None, 65280, B), ("hcrc", dict(hcrc=1), None, 65280, B),
             ("schedule", dict(), ffi.make_schedule(8192), 65280, B), ("schedule", dict(), ffi.make_schedule(writes=[10, None]), 65280, B),
             ("block_size", dict(block_size=4096), None, 65501, B), ("flags", dict(), None, 4096, 2)]
    d_in = _dev(torch, data)
    d_out = torch.full((1 << 16,), 0xA5, dtype=torch.uint8, device="cuda")
    for field, kw, sched, member_size, flags in cases:
        with pytest.raises(ffi.LfxError) as e:
            ctx.encode_members_device(d_in.data_ptr(), len(data), d_out.data_ptr(), 1 << 16, member_size, flags, ffi.make_opts(**kw), sched)
        assert e.value.status == ffi.E_ARG and field in e.value.message, (field, e.value.message)
        with pytest.raises(ffi.LfxError) as e:
            ctx.encode_members_host(data, member_size, flags, ffi.make_opts(**kw), sched, cap=1 << 16)
        assert e.value.status == ffi.E_ARG and field in e.value.message, (field, e.value.message)
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().tobytes() == b"\xA5" * (1 << 16)       # a refused call writes nothing


# ---------------------------------------------------------------------------------------------- capacity, table size, host path
@pytest.mark.parametrize("flags,member_size", [(0, 4096), (0, 65536), (1, 65280), (1, 65505)])
def test_capacity_exact_and_one_short(ctx, ffi, torch, oracle, flags, member_size):
    data = mixed(seed=17)
    want = model_bgzf(oracle, data, member_size)[0] if flags else model_plain(oracle, data, member_size)[0]
    rc, out, count, members, msg, _ = run_device(ctx, ffi, torch, data, member_size, flags)
    assert rc == ffi.OK and out == want
    for trim in (0, 1, 2, 3):           # (every phase of the output's end inside its last dword)
        d, w = (data[:len(data) - trim], None) if trim else (data, want)
        if w is None:
            w = model_bgzf(oracle, d, member_size)[0] if flags else model_plain(oracle, d, member_size)[0]
        rc, out, count, members, msg, whole = run_device(ctx, ffi, torch, d, member_size, flags, cap=len(w))
        assert rc == ffi.OK and out == w, (trim, msg)
        rc, out, count2, members, msg, whole = run_device(ctx, ffi, torch, d, member_size, flags, cap=len(w) - 1)
        assert rc == ffi.E_NOSPACE and out == b"" and count2 == count, (trim, rc, msg)
        assert whole[:len(w) - 1] == bytes(len(w) - 1)       # zero-filled, no member written
    # the empty BGZF file: the marker alone
    if flags:
        rc, out, count, members, msg, _ = run_device(ctx, ffi, torch, b"", member_size, flags, cap=28)
        assert (rc, out, count, members) == (ffi.OK, BGZF_EOF, 0, [])
        rc, out, count, members, msg, whole = run_device(ctx, ffi, torch, b"", member_size, flags, cap=27)
        assert rc == ffi.E_NOSPACE and out == b"" and whole[:27] == b"\xA5" * 27


def test_max_members_and_null_table(ctx, ffi, torch, oracle):
    data = words_text(100 * 1000, seed=21)
    want, table = model_plain(oracle, data, 4096)
    rc, out, count, members, msg, _ = run_device(ctx, ffi, torch, data, 4096, max_members=5)
    assert rc == ffi.OK and out == want and count == len(table) == 25 and members == table[:5]
    # a table of 8 with max_members = 5: the records behind the fifth stay untouched; a NULL table
    L = ffi.lib()
    d_in = _dev(torch, data)
    cap = bound_of(ffi, len(data), 4096, 0, None, None)
    d_out = torch.zeros((cap,), dtype=torch.uint8, device="cuda")
    tab = (ffi.Member * 8)()
    for m in tab:
        m.in_off = m.in_len = m.out_off = m.out_len = 0xA5A5A5A5
    out_len, got = C.c_uint64(0), C.c_uint32(0)
    assert L.lfx_encode_members_device(ctx._h, None, None, 4096, 0, d_in.data_ptr(), len(data), d_out.data_ptr(), cap, C.byref(out_len),
                                       tab, 5, C.byref(got)) == ffi.OK
    assert got.value == 25 and [(m.in_off, m.in_len, m.out_off, m.out_len) for m in tab[:5]] == table[:5]
    assert all(m.out_len == 0xA5A5A5A5 for m in tab[5:])
    assert L.lfx_encode_members_device(ctx._h, None, None, 4096, 0, d_in.data_ptr(), len(data), d_out.data_ptr(), cap, C.byref(out_len),
                                       None, 0, C.byref(got)) == ffi.OK
    assert got.value == 25 and out_len.value == len(want)
    assert d_out[:len(want)].cpu().numpy().tobytes() == want


def test_host_equals_device_and_python_api(ctx, ffi, lfx, torch, oracle):
    data = mixed(seed=23)
    for flags, member_size in ((0, 50000), (ffi.MEMBERS_BGZF, 65505)):
        rc, dev_out, count, dev_members, msg, _ = run_device(ctx, ffi, torch, data, member_size, flags)
        assert rc == ffi.OK, msg
        rc, host_out, hcount, host_members, msg = ctx.encode_members_host(data, member_size, flags)
        assert rc == ffi.OK and host_out == dev_out and host_members == dev_members and hcount == count
        rc, host_out, hcount, _m, msg = ctx.encode_members_host(data, member_size, flags, cap=len(dev_out) - 1)
        assert rc == ffi.E_NOSPACE and host_out == b""
        out, members = lfx.gzip.encode_members(data, member_size, bgzf=bool(flags), context=ctx)
        assert out == dev_out and members == dev_members
        assert lfx.gzip.decode_members(out, context=ctx)[0] == data
    # the defaults: 1 MiB members; an options object
    out, members = lfx.gzip.encode_members(data, context=ctx)
    assert out == oracle.encode(oracle.GZIP, data) and members == [(0, len(data), 0, len(out))]
    out, members = lfx.gzip.encode_members(data, 65536, options=lfx.gzip.EncodeOptions().fixed_huffman_codes(), context=ctx)
    assert out == model_plain(oracle, data, 65536, dynamic_huffman=0)[0]
    with pytest.raises(lfx.gzip.StreamError) as e:
        lfx.gzip.encode_members(data, 65506, bgzf=True, context=ctx)
    assert "member_size" in str(e.value)
    assert lfx.gzip.members_to_gzi(members) == gzi_model(members)


def test_same_plan_after_a_fallback_call(ctx, ffi, torch, oracle):
    """a BGZF call turns blocks of fallen-back members into stored ones in the device's block table: the next call with the
    same plan (same sizes) must not find them there"""
    rnd, txt = random_bytes(3 * 65505, seed=31), words_text(3 * 65505, seed=31)
    for data in (rnd, txt, rnd, txt):
        want = model_bgzf(oracle, data, 65505)[0]
        rc, out, *_ = run_device(ctx, ffi, torch, data, 65505, ffi.MEMBERS_BGZF)
        assert rc == ffi.OK and out == want
