"""GPU: zlib and raw DEFLATE streams that use a preset dictionary (include/lfx.h "preset dictionaries") through
the one-shot calls, the batch call and the stream decoder.  python-zlib is the ground truth (dict_craft.py; test_dict_abi.py
proves every fixture on the CPU).  Integer work: every comparison is exact."""
import ctypes as C
import io
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import dict_craft as dk
from test_gpu_parity import ctx, ffi, lfx  # noqa: F401  (fixtures)
from test_gpu_members import _dev, torch  # noqa: F401

GUARD = 16
FILL = 0x5A


@pytest.fixture(scope="module")
def dicts(lfx, ctx):
    """one Dictionary per distinct dictionary of the fixtures, made once"""
    made = {}

    def get(zdict):
        if zdict not in made:
            made[zdict] = lfx.Dictionary(zdict, ctx)
        return made[zdict]
    yield get
    for d in made.values():
        d.close()


def _fmt(ffi, c):
    return ffi.ZLIB if c.fmt == "zlib" else ffi.DEFLATE


def _one_shot(ctx, ffi, torch, fmt, zdict, z, cap):
    d_in = _dev(torch, z)
    d_out = torch.full((cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    rc, ol, used, msg = ctx.decode_dict_device(fmt, zdict, d_in.data_ptr(), len(z), d_out.data_ptr(), cap)
    host = d_out.cpu().numpy().tobytes()
    assert host[cap:] == bytes([FILL]) * GUARD, "guard written"
    assert host[ol:cap] == bytes([FILL]) * (cap - ol), "bytes behind out_len written"
    return rc, host[:ol], used, msg


def _check(c, got, ffi):
    rc, out, used, msg = got
    if c.err is None:
        assert (rc, len(out), used) == (ffi.OK, len(c.want), len(c.stream)), (c.name, rc, len(out), used, msg)
        assert out == c.want, c.name
    else:
        assert (rc, out, msg) == (getattr(ffi, c.err[0]), b"", c.err[1]), (c.name, rc, len(out), msg)


def test_dictionary_object(lfx, ctx, ffi, torch):
    for zd in (dk.D32, dk.D40, dk.D300, dk.D1, dk.D0):
        d = lfx.Dictionary(zd, ctx)
        assert d.id == zlib.adler32(zd), len(zd)            # (all bytes, also beyond the window; an empty one: 1)
        d.close()
    users = ctx._users
    d = lfx.Dictionary(_dev(torch, dk.D40), ctx)             # device memory
    assert d.id == zlib.adler32(dk.D40) and ctx._users == users + 1
    c = dk.by_name("rec1100_raw_d40")
    _check(c, _one_shot(ctx, ffi, torch, ffi.DEFLATE, d, c.stream, len(c.want)), ffi)
    d.close()
    d.close()
    assert ctx._users == users


def test_serial_kernel_cases(ctx, ffi, torch, dicts):
    """records of 1 / 100 / 1100 bytes, dictionaries of 32768 / 1 / 0 / 40000 bytes, and the hand-written matches: every
    stream is below 4 KiB, the exact serial kernel's dictionary instance decodes it"""
    n = 0
    for c in dk.cases():
        if not c.name.startswith(("rec", "craft_")):
            continue
        _check(c, _one_shot(ctx, ffi, torch, _fmt(ffi, c), dicts(c.zdict), c.stream, max(len(c.want), 1)), ffi)
        rc, out, used, msg = ctx.decode_dict_host(_fmt(ffi, c), dicts(c.zdict), c.stream)
        _check(c, (rc, out, used, msg), ffi)
        n += 1
    assert n == 18


def test_block_rounds_and_one_shot_blocks(ctx, ffi, torch, dicts):
    """the 64 KiB record (head = the dictionary's tail) one-shot and in a batch, and the sync-flush stream whose second
    block reaches the dictionary across the first: in a batch these go through scan_round / emit_round, and the materialise
    kernel's dictionary instance preloads from the dictionary and from the output"""
    cs = [dk.by_name(n) for n in ("blk64k_raw", "sync_flush_reach", "rec1100_raw_d32", "blk64k_raw")]
    for c in cs[:2] + [dk.by_name("blk64k_zlib")]:
        _check(c, _one_shot(ctx, ffi, torch, _fmt(ffi, c), dicts(c.zdict), c.stream, len(c.want)), ffi)
    res, outs = _batch(ctx, ffi, torch, ffi.DEFLATE, dicts(dk.D32), [c.stream for c in cs], [len(c.want) for c in cs])
    for c, (st, ol), out in zip(cs, res, outs):
        assert (st, ol) == (ffi.OK, len(c.want)) and out == c.want, c.name
    ctx.enable_timing(True)
    _batch(ctx, ffi, torch, ffi.DEFLATE, dicts(dk.D32), [c.stream for c in cs], [len(c.want) for c in cs])
    names = [p[0] for p in ctx.last_timing()["phases"]]
    ctx.enable_timing(False)
    assert "blk_scan" in names and "lz77_copy" in names, names


def test_large_member(ctx, ffi, torch, dicts):
    """1.5 MiB behind 3000 bytes of the dictionary's tail, about 500 KB of zlib level 6: the finder path.  Not a serial
    decode: the phases are those of the block scan and the marker path (init_win = the dictionary window)"""
    c = dk.by_name("large_zlib")
    ctx.enable_timing(True)
    got = _one_shot(ctx, ffi, torch, ffi.ZLIB, dicts(dk.D32), c.stream, len(c.want))
    names = [p[0] for p in ctx.last_timing()["phases"]]
    print("phases of the large member:", names)
    _check(c, got, ffi)
    assert "serial" not in names and "blk_scan" in names and "lz77_sym" in names and "substitute" in names, names
    rc, out, used, msg = ctx.decode_dict_host(ffi.ZLIB, dicts(dk.D32), c.stream, cap=len(c.want))
    names = [p[0] for p in ctx.last_timing()["phases"]]
    ctx.enable_timing(False)
    _check(c, (rc, out, used, msg), ffi)
    assert "serial" not in names, names


def _batch(ctx, ffi, torch, fmt, zdict, streams, caps, exact=True):
    """streams packed back to back, outputs packed with GUARD bytes between the ranges → ([(status, out_len)], [bytes]);
    asserts that nothing outside [out_off, out_off + out_len) was written (exact=False: outside [out_off, out_off + out_cap),
    the guards — the dictionary-less batch call itself leaves bytes of a discarded fast-path attempt behind out_len, inside
    the stream's own capacity, when a damaged stream's verdict comes from the exact kernel)"""
    in_offs, out_offs, pos, opos = [], [], 0, GUARD
    for z, cap in zip(streams, caps):
        in_offs.append(pos)
        pos += len(z)
        out_offs.append(opos)
        opos += cap + GUARD
    d_in = _dev(torch, b"".join(streams))
    d_out = torch.full((opos,), FILL, dtype=torch.uint8, device="cuda")
    res = ctx.decode_batch_dict_device(fmt, zdict, d_in.data_ptr(), in_offs, [len(z) for z in streams], d_out.data_ptr(),
                                       out_offs, caps)
    host = d_out.cpu().numpy()
    written = np.ones(opos, dtype=bool)
    outs = []
    for off, (st, ol) in zip(out_offs, res):
        assert ol <= caps[len(outs)]
        written[off:off + (ol if exact else caps[len(outs)])] = False
        outs.append(host[off:off + ol].tobytes())
    assert (host[written] == FILL).all(), "bytes outside a stream's [out_off, out_off + out_len) written"
    return res, outs


def test_batch_corrupted_body(ctx, ffi, torch, dicts):
    """dictionary streams with one flipped byte in the body, among good neighbours: the batch's status, out_len and bytes are
    those of the one-shot dictionary call on the same stream (the exact kernel's), nothing is written outside the stream's own
    capacity (include/lfx.h rule 7), and the neighbours are exact"""
    recs = dk.batch_records(10)
    streams, want = [z for z, _ in recs], [r for _, r in recs]
    hit = {2: 0.3, 4: 0.5, 6: 0.7, 7: 0.9}
    for i, at in hit.items():
        b = bytearray(streams[i]); b[6 + int((len(b) - 10) * at)] ^= 0x55
        streams[i] = bytes(b)
    caps = [len(r) for r in want]
    res, outs = _batch(ctx, ffi, torch, ffi.ZLIB, dicts(dk.D32), streams, caps, exact=False)
    for i, ((st, ol), out) in enumerate(zip(res, outs)):
        if i in hit:
            rc, one, _used, _msg = _one_shot(ctx, ffi, torch, ffi.ZLIB, dicts(dk.D32), streams[i], caps[i])
            assert st != ffi.OK and (st, ol, out) == (rc, len(one), one), (i, st, ol, rc, len(one))
        else:
            assert (st, ol) == (ffi.OK, len(want[i])) and out == want[i], (i, st, ol)


@pytest.mark.parametrize("count", [1, 64, 1000])
def test_batch_records(ctx, ffi, torch, dicts, count):
    recs = dk.batch_records(count)
    res, outs = _batch(ctx, ffi, torch, ffi.ZLIB, dicts(dk.D32), [z for z, _ in recs], [len(r) for _, r in recs])
    bad = [i for i, ((st, ol), out, (_, r)) in enumerate(zip(res, outs, recs)) if (st, ol) != (ffi.OK, len(r)) or out != r]
    assert not bad, bad[:10]


def test_batch_mixed_verdicts(ctx, ffi, torch, dicts):
    recs = dk.batch_records(12)
    streams, want = [z for z, _ in recs], [r for _, r in recs]
    caps = [len(r) for r in want]
    wrong = bytearray(streams[1]); wrong[2:6] = (zlib.adler32(dk.D32) ^ 1).to_bytes(4, "big")
    streams[1] = bytes(wrong)                                   # wrong DICTID
    streams[3] = zlib.compress(want[3], 9)                      # no FDICT: decodes without the dictionary
    streams[5] = streams[5][:4]                                 # cut in its header
    streams[7] = streams[7][:len(streams[7]) // 2]              # cut in its body
    caps[9] -= 1                                                # one byte short
    res, outs = _batch(ctx, ffi, torch, ffi.ZLIB, dicts(dk.D32), streams, caps)
    # (the context's message is the first failing stream's)
    assert ctx.last_error() == "Dictionary mismatch: dictionary_id=0x%X, supplied=0x%X" % (zlib.adler32(dk.D32) ^ 1, zlib.adler32(dk.D32))
    for i, ((st, ol), out) in enumerate(zip(res, outs)):
        if i == 1:
            assert (st, ol) == (ffi.E_INVALID_DATA, 0), (i, st, ol)
        elif i == 5:
            assert (st, ol) == (ffi.E_UNEXPECTED_EOF, 0), (i, st, ol)
        elif i == 7:
            # what the dictionary-less batch call does with a stream cut at the same place: its status, a prefix as output
            plain = zlib.compress(want[7], 9)
            pres, pouts = _batch(ctx, ffi, torch, ffi.ZLIB, None, [plain[:len(plain) // 2]], [len(want[7])])
            assert st == pres[0][0] == ffi.E_UNEXPECTED_EOF and 0 < ol < len(want[7]) and out == want[7][:ol], (i, st, ol)
            assert pouts[0] == want[7][:pres[0][1]]
        elif i == 9:
            assert st == ffi.E_NOSPACE and out == want[9][:ol], (i, st, ol)
        else:
            assert (st, ol) == (ffi.OK, len(want[i])) and out == want[i], (i, st, ol)


def test_rules_3_and_5(ctx, ffi, torch, dicts):
    good = zlib.compress(dk.record(0), 9)
    fdict = dk.by_name("rec1100_zlib_d32").stream
    damaged = bytearray(good); damaged[len(good) // 2] ^= 0x55; damaged = bytes(damaged)
    cap = 4096
    for z in (good, fdict, damaged):
        # rule 3: without a dictionary each call is its twin
        d_in = _dev(torch, z)
        twin_out = torch.full((cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        twin = ctx.decode_device(ffi.ZLIB, d_in.data_ptr(), len(z), twin_out.data_ptr(), cap)
        got = _one_shot(ctx, ffi, torch, ffi.ZLIB, None, z, cap)
        assert (got[0], len(got[1]), got[2], got[3]) == twin, (got[0], got[3], twin)
        assert got[1] == twin_out.cpu().numpy().tobytes()[:twin[1]]
        assert ctx.decode_dict_host(ffi.ZLIB, None, z, cap=cap) == ctx.decode_host(ffi.ZLIB, z, cap=cap)
        res, outs = _batch(ctx, ffi, torch, ffi.ZLIB, None, [z], [cap], exact=False)
        msg = ctx.last_error() if res[0][0] else ""
        pres = (C.c_uint64 * 1)(), (C.c_int32 * 1)()
        a = lambda v: (C.c_uint64 * 1)(v)
        pout = torch.full((cap,), FILL, dtype=torch.uint8, device="cuda")
        assert ffi.lib().lfx_decode_batch_device(ctx.handle, ffi.ZLIB, 1, d_in.data_ptr(), a(0), a(len(z)), pout.data_ptr(), a(0),
                                                 a(cap), pres[0], pres[1]) == 0
        assert res[0] == (pres[1][0], pres[0][0]) and outs[0] == pout.cpu().numpy().tobytes()[:pres[0][0]]
        assert msg == (ctx.last_error() if pres[1][0] else "")
    assert twin[0] != ffi.OK
    got = _one_shot(ctx, ffi, torch, ffi.ZLIB, None, fdict, cap)
    assert got[0] == ffi.E_INVALID_DATA and got[3] == "Preset dictionaries are not supported: dictionary_id=0x%X" % zlib.adler32(dk.D32)
    # rule 5: FDICT clear, a dictionary given: lfx_decode_device's result
    d_in = _dev(torch, good)
    twin_out = torch.full((cap,), FILL, dtype=torch.uint8, device="cuda")
    twin = ctx.decode_device(ffi.ZLIB, d_in.data_ptr(), len(good), twin_out.data_ptr(), cap)
    got = _one_shot(ctx, ffi, torch, ffi.ZLIB, dicts(dk.D32), good, cap)
    assert (got[0], len(got[1]), got[2], got[3]) == twin and got[1] == dk.record(0)
    # gzip has no dictionary
    with pytest.raises(ffi.LfxError) as e:
        _one_shot(ctx, ffi, torch, ffi.GZIP, dicts(dk.D32), good, cap)
    assert e.value.status == ffi.E_ARG
    with pytest.raises(ffi.LfxError) as e:
        ctx.decode_batch_dict_device(ffi.GZIP, dicts(dk.D32), d_in.data_ptr(), [0], [len(good)], twin_out.data_ptr(), [0], [cap])
    assert e.value.status == ffi.E_ARG
    # rule 4: a wrong id, and what the FDICT rejection consumes for the same bytes; fewer than six bytes
    got = _one_shot(ctx, ffi, torch, ffi.ZLIB, dicts(dk.D300), fdict, cap)
    twin = ctx.decode_device(ffi.ZLIB, _dev(torch, fdict).data_ptr(), len(fdict), twin_out.data_ptr(), cap)
    assert got == (ffi.E_INVALID_DATA, b"", twin[2], "Dictionary mismatch: dictionary_id=0x%X, supplied=0x%X" %
                   (zlib.adler32(dk.D32), zlib.adler32(dk.D300))) and twin[2] == 6
    assert _one_shot(ctx, ffi, torch, ffi.ZLIB, dicts(dk.D32), fdict[:5], cap)[0] == ffi.E_UNEXPECTED_EOF
    # the Adler-32 trailer covers the output only; a bad one is the existing verdict
    bad = fdict[:-1] + bytes([fdict[-1] ^ 1])
    got = _one_shot(ctx, ffi, torch, ffi.ZLIB, dicts(dk.D32), bad, cap)
    want = dk.by_name("rec1100_zlib_d32").want
    assert got[0] == ffi.E_INVALID_DATA and got[3].startswith("Adler32 checksum mismatched: value=%u" % zlib.adler32(want)), got[3]


class _Slow(io.RawIOBase):
    """hands over at most `step` bytes a read; block: raises BlockingIOError before every chunk once"""

    def __init__(self, data, step, block=False):
        self.data, self.pos, self.step, self.block, self.armed = data, 0, step, block, True

    def read(self, n=-1):
        if self.block and self.armed and self.pos < len(self.data):
            self.armed = False
            raise BlockingIOError()
        self.armed = True
        k = min(n if n >= 0 else len(self.data), self.step)
        b = self.data[self.pos:self.pos + k]
        self.pos += len(b)
        return b


def _drain(dec, step):
    out = []
    while True:
        try:
            b = dec.read(step)
        except BlockingIOError:
            continue
        if not b:
            return b"".join(out)
        out.append(b)


def test_stream_decoder(lfx, ctx, ffi, dicts):
    c = dk.by_name("rec1100_zlib_d32")
    for step in (1, 7, 8192):
        assert _drain(lfx.zlib.Decoder.new(c.stream, ctx, zdict=dicts(dk.D32)), step) == c.want, step
    assert lfx.zlib.Decoder.new(_Slow(c.stream, 1), ctx, zdict=dk.D32).read_to_end() == c.want          # bytes as zdict
    r = dk.by_name("sync_flush_reach")
    assert lfx.deflate.Decoder.new(_Slow(r.stream, 1), ctx, zdict=dicts(dk.D32)).read_to_end() == r.want
    for cls, case in ((lfx.non_blocking.zlib.Decoder, c), (lfx.non_blocking.deflate.Decoder, r)):
        assert _drain(cls.new(_Slow(case.stream, 97, block=True), ctx, zdict=dicts(dk.D32)), 4096) == case.want
    # FDICT clear: the dictionary is not used; a wrong dictionary: the header's verdict, from the constructor
    plain = zlib.compress(c.want, 9)
    assert lfx.zlib.Decoder.new(plain, ctx, zdict=dicts(dk.D32)).read_to_end() == c.want
    with pytest.raises(lfx.StreamError) as e:
        lfx.zlib.Decoder.new(c.stream, ctx, zdict=dicts(dk.D300))
    assert e.value.status == ffi.E_INVALID_DATA and "Dictionary mismatch" in str(e.value)
    with pytest.raises(lfx.StreamError) as e:       # without one, today's rejection
        lfx.zlib.Decoder.new(c.stream, ctx)
    assert "Preset dictionaries are not supported" in str(e.value)
    # too late, and gzip
    d2 = lfx.zlib.Decoder.new(plain, ctx)
    with pytest.raises(lfx.StreamError) as e:
        d2.set_dict(dicts(dk.D32))                   # the constructor has read the header
    assert e.value.status == ffi.E_ARG
    d3 = lfx.deflate.Decoder.new(dk.by_name("rec100_raw_d32").stream, ctx, zdict=dicts(dk.D32))
    assert d3.read(10) == dk.by_name("rec100_raw_d32").want[:10]
    with pytest.raises(lfx.StreamError) as e:
        d3.set_dict(dicts(dk.D32))                   # after the first read
    assert e.value.status == ffi.E_ARG
    g = lfx.gzip.Decoder.new(__import__("gzip").compress(b"x"), ctx)
    with pytest.raises(lfx.StreamError) as e:
        g.set_dict(dicts(dk.D32))
    assert e.value.status == ffi.E_ARG


def test_stream_decoder_large_member(lfx, ctx, dicts):
    c = dk.by_name("large_zlib")
    assert lfx.zlib.Decoder.new(io.BytesIO(c.stream), ctx, zdict=dicts(dk.D32)).read_to_end() == c.want
