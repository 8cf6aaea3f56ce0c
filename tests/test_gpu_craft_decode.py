"""GPU: legal DEFLATE that neither this library's encoder nor python-zlib writes, and rejects decided in a header or by one
symbol (deflate_craft.CASES), through three entry points: lfx_decode_device, lfx_decode_size_device, lfx_decode_batch_device,
and as the members of one gzip file through both members paths.
Every stream's verdict is fixed by the oracle on the CPU first (test_craft_streams.py holds the conditions under which these
tests mean anything).  Integer work: every comparison is exact.  A test walks all its cases and reports every one that differs."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import deflate_craft as dc
from test_gpu_parity import ctx, ffi, lfx, synth  # noqa: F401  (fixtures)
from test_gpu_members import _dev, check, torch  # noqa: F401
from deflate_craft import gzwrap, zwrap

GUARD = 256
ALL_FORMATS = ("A", "B")            # these go through all three containers, the rest as raw DEFLATE


@pytest.fixture(scope="module")
def crafted(oracle):
    """[(name, format name, stream, (status, output, consumed, message) of the oracle)]; the container streams carry the
    checksum of what the oracle delivered"""
    out = []
    for name, (z, want) in dc.built().items():
        verdict = oracle.decode(oracle.DEFLATE, z)
        assert (verdict[0] == 0) == (want is not None) and (want is None or verdict[1] == want), name      # (test_craft_streams.py)
        out.append((name, "DEFLATE", z, verdict))
        if name in ALL_FORMATS:
            for fmt_name, s in (("ZLIB", zwrap(verdict[1], z)), ("GZIP", gzwrap(verdict[1], z))):
                out.append((name, fmt_name, s, oracle.decode(getattr(oracle, fmt_name), s)))
    return out


def _decode_one(ctx, ffi, torch, fmt_name, z, verdict):
    """decode_device into exactly the oracle's length + a guard → a list of what differs"""
    orc, oout, oused, omsg = verdict
    cap = len(oout)
    d_in = _dev(torch, z)
    d_out = torch.full((cap + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    rc, ol, used, msg = ctx.decode_device(getattr(ffi, fmt_name), d_in.data_ptr(), len(z), d_out.data_ptr(), cap)
    host = d_out.cpu().numpy().tobytes()
    bad = []
    if (rc, ol, used) != (orc, len(oout), oused):
        bad.append("(status, out_len, consumed) %r, oracle %r, message %r" % ((rc, ol, used), (orc, len(oout), oused), msg))
    if msg.split(":")[0] != omsg.split(":")[0]:
        bad.append("message %r, oracle %r" % (msg, omsg))
    if host[:min(ol, cap)] != oout[:min(ol, cap)]:
        first = next(i for i in range(min(ol, cap)) if host[i] != oout[i])
        bad.append("bytes differ from %d of %d" % (first, ol))
    if host[cap:] != b"\x5a" * GUARD:
        bad.append("guard written")
    return bad


def _report(bad):
    for line in bad:
        print("DIFFERS", line)
    assert not bad, "%d case(s) differ: %s" % (len(bad), "; ".join(bad))


def test_decode_device(ctx, ffi, torch, crafted):
    bad = []
    for name, fmt_name, z, verdict in crafted:
        if name in dc.SMALL:
            continue
        bad += ["%s %s: %s" % (name, fmt_name, b) for b in _decode_one(ctx, ffi, torch, fmt_name, z, verdict)]
    _report(bad)


def test_decode_device_small_variants(ctx, ffi, torch, crafted):
    """under 4 KiB: the serial kernel, whose header parse must agree with the parallel one"""
    bad, seen = [], 0
    for name, fmt_name, z, verdict in crafted:
        if name in dc.SMALL:
            assert len(z) < 4096
            seen += 1
            bad += ["%s %s: %s" % (name, fmt_name, b) for b in _decode_one(ctx, ffi, torch, fmt_name, z, verdict)]
    assert seen == len(dc.SMALL)
    _report(bad)


def test_decode_size_device(ctx, ffi, torch, crafted):
    bad = []
    for name, fmt_name, z, (orc, oout, oused, omsg) in crafted:
        d_in = _dev(torch, z)
        rc, ol, used, msg = ctx.decode_size_device(getattr(ffi, fmt_name), d_in.data_ptr(), len(z))
        if (rc, ol, used) != (orc, len(oout), oused):
            bad.append("%s %s: (status, out_len, consumed) %r, oracle %r, message %r" % (name, fmt_name, (rc, ol, used), (orc, len(oout), oused), msg))
        if msg.split(":")[0] != omsg.split(":")[0]:
            bad.append("%s %s: message %r, oracle %r" % (name, fmt_name, msg, omsg))
    _report(bad)


def test_decode_batch_device(ctx, ffi, oracle, torch, crafted):
    """every case as a zlib stream in ONE call: valid ones, rejects and the reject under the fast path's 64-byte floor next to
    each other"""
    raw = dict((name, (z, v)) for name, fmt_name, z, v in crafted if fmt_name == "DEFLATE")
    valid, rejects = [n for n in raw if n in dc.VALID], [n for n in raw if n in dc.REJECTS]
    order = []
    while valid or rejects:            # two valid, one reject, ...
        order += valid[:2] + rejects[:1]
        valid, rejects = valid[2:], rejects[1:]
    assert sorted(order) == sorted(raw) and order.index("I1") not in (0, len(order) - 1)
    streams = [zwrap(raw[n][1][1], raw[n][0]) for n in order]
    assert len(streams[order.index("I1")]) < 64
    want = [oracle.decode(oracle.ZLIB, s) for s in streams]
    k = len(streams)
    in_len = [len(s) for s in streams]
    in_off = [sum(in_len[:i]) for i in range(k)]
    out_cap = [len(w[1]) for w in want]
    out_off = [sum((c + 259) & ~255 for c in out_cap[:i]) for i in range(k)]
    d_in = _dev(torch, b"".join(streams))
    d_out = torch.full((out_off[-1] + out_cap[-1] + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    a = lambda v: (C.c_uint64 * k)(*v)
    got_len, got_st = (C.c_uint64 * k)(), (C.c_int32 * k)()
    rc = ffi.lib().lfx_decode_batch_device(ctx.handle, ffi.ZLIB, k, d_in.data_ptr(), a(in_off), a(in_len), d_out.data_ptr(), a(out_off),
                                           a(out_cap), got_len, got_st)
    assert rc == ffi.OK
    host = d_out.cpu().numpy()
    bad = []
    for i, name in enumerate(order):
        orc, oout, oused, omsg = want[i]
        if (got_st[i], got_len[i]) != (orc, len(oout)):
            bad.append("%s: (status, out_len) %r, oracle %r %s" % (name, (got_st[i], got_len[i]), (orc, len(oout)), omsg))
        n = min(got_len[i], out_cap[i])
        if host[out_off[i]:out_off[i] + n].tobytes() != oout[:n]:
            bad.append("%s: bytes differ" % name)
        end = out_off[i + 1] if i + 1 < k else len(host)
        if not (host[out_off[i] + out_cap[i]:end] == 0x5A).all():
            bad.append("%s: the gap behind its output was written" % name)
    _report(bad)


def _gzip_file(crafted, third=None):
    """every valid case but M as a gzip member, in CASES order (`third`: a case to put in as the third member)
    → (the file, [(name, member bytes, output bytes)])"""
    raw = dict((name, (z, v)) for name, fmt_name, z, v in crafted if fmt_name == "DEFLATE")
    names = [n for n, _ in dc.CASES if n in dc.VALID and n != "M"]
    if third is not None:
        names.insert(2, third)
    parts = [(n, gzwrap(raw[n][1][1], raw[n][0]), raw[n][1][1]) for n in names]
    return b"".join(p[1] for p in parts), parts


def _table(parts):
    out, at, oat = [], 0, 0
    for _name, member, plain in parts:
        out.append((at, len(member), oat, len(plain)))
        at, oat = at + len(member), oat + len(plain)
    return out


def test_members_paths(ctx, ffi, oracle, torch, crafted):
    """one gzip file whose members are the valid cases: lfx_decode_members_device and the sequential member loop (`check` holds
    them to each other and to the oracle's MultiDecoder) give the oracle's bytes and the member table of the file as built"""
    data, parts = _gzip_file(crafted)
    assert len(parts) == len(dc.VALID) - 1 >= 20
    o_rc, o_out, o_used, o_msg = oracle.decode(oracle.GZIP, data, multi=True)
    assert (o_rc, o_used) == (0, len(data)) and o_out == b"".join(p[2] for p in parts), o_msg
    rc, out, used, members = check(ctx, ffi, oracle, torch, data, want_status=ffi.OK)
    bad = []
    if out != o_out:
        first = next((i for i in range(min(len(out), len(o_out))) if out[i] != o_out[i]), min(len(out), len(o_out)))
        at = [p[0] for p, m in zip(parts, _table(parts)) if m[2] <= first < m[2] + max(m[3], 1)]
        bad.append("bytes differ from %d (%d of %d), in %s" % (first, len(out), len(o_out), at))
    if used != len(data):
        bad.append("consumed %d of %d" % (used, len(data)))
    for (name, _m, _p), got, want in zip(parts, members, _table(parts)):
        if got != want:
            bad.append("%s: member %r, built as %r" % (name, got, want))
    if len(members) != len(parts):
        bad.append("%d members of %d" % (len(members), len(parts)))
    _report(bad)


def test_members_paths_reject_as_third_member(ctx, ffi, oracle, torch, crafted):
    """the same file with J_behind (an over-subscribed code behind 10 KB of valid blocks) as its third member: the oracle's
    status and message, the first two members in the table, the oracle's bytes up to the fault"""
    data, parts = _gzip_file(crafted, third="J_behind")
    assert parts[2][0] == "J_behind"
    o_rc, o_out, o_used, o_msg = oracle.decode(oracle.GZIP, data, multi=True)
    assert o_rc == ffi.E_INVALID_DATA and o_msg.startswith(dc.REJECT_PREFIX["J"])
    assert o_out == b"".join(p[2] for p in parts[:3]) and len(parts[2][2]) >= 20000
    rc, out, used, members = check(ctx, ffi, oracle, torch, data, want_status=ffi.E_INVALID_DATA)
    assert ctx.last_error().startswith(dc.REJECT_PREFIX["J"]), ctx.last_error()
    assert members == _table(parts)[:2]
    assert out == o_out


def test_record_shapes_that_leave_the_fast_path(ffi, lfx, torch, crafted, monkeypatch):
    """A record, not a contract: which legal shapes cost a serial walk (LFX_NO_SERIAL=1 makes the walk an error).  What does
    decode without it must still be the oracle's bytes."""
    monkeypatch.setenv("LFX_NO_SERIAL", "1")
    c2 = lfx.Context(0)                 # (diagnostic switches are read when a context is made)
    try:
        for name, fmt_name, z, (orc, oout, oused, omsg) in crafted:
            if name not in dc.VALID or fmt_name != "DEFLATE":
                continue
            d_in = _dev(torch, z)
            d_out = torch.full((len(oout) + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
            rc, ol, used, msg = c2.decode_device(ffi.DEFLATE, d_in.data_ptr(), len(z), d_out.data_ptr(), len(oout))
            print("NO_SERIAL %-16s -> %s" % (name, "decoded" if rc == ffi.OK else msg))
            if rc == ffi.OK:
                assert (ol, used) == (len(oout), oused) and d_out.cpu().numpy().tobytes() == oout + b"\x5a" * GUARD, name
    finally:
        c2.close()
