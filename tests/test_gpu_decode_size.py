"""GPU: the size calls (lfx_decode_size_*, lfx_decode_batch_size_device, lfx_decode_members_size_*).  Expected
values come from the oracle and from Python's zlib, never from this library's decode; the decode is called only for rule 3 of
the contract (a decode with cap = out_len never returns LFX_E_NOSPACE) and for the equality of the error message."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

from golden import kat

pytestmark = pytest.mark.gpu

from test_gpu_parity import ctx, ffi, lfx, synth  # noqa: F401  (fixtures)
from test_gpu_members import BGZF_EOF, batch_encoded, small_members, zmember

KIB = 1 << 10
MIB = 1 << 20


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def _dev(torch, data):
    a = np.frombuffer(bytes(data), dtype=np.uint8).copy() if len(data) else np.zeros(1, dtype=np.uint8)
    return torch.from_numpy(a).to("cuda")


def _ofmt(oracle, ffi, fmt):
    return {ffi.DEFLATE: oracle.DEFLATE, ffi.ZLIB: oracle.ZLIB, ffi.GZIP: oracle.GZIP}[fmt]


def _is_checksum(omsg):
    return omsg.startswith("CRC32 mismatched") or omsg.startswith("Adler32 checksum mismatched")


def check(ctx, ffi, oracle, torch, fmt, data, multi=False, want=None, host=True):
    """the contract of one stream against the oracle → (status, out_len, consumed, message)"""
    data = bytes(data)
    flags = ffi.DEC_MULTI if multi else 0
    orc, oout, oused, omsg = oracle.decode(_ofmt(oracle, ffi, fmt), data, multi=multi)
    if orc != ffi.OK and _is_checksum(omsg) and not multi:
        orc = ffi.OK            # rule 3: the one verdict a size call cannot reach (the bytes and the trailer are all there)
    d_in = _dev(torch, data)
    rc, ol, used, msg = ctx.decode_size_device(fmt, d_in.data_ptr(), len(data), flags)
    tag = (fmt, len(data), multi)
    print("size", tag, (rc, ol, used, msg), "oracle", (orc, len(oout), oused, omsg))
    assert (rc, ol, used) == (orc, len(oout), oused), (tag, msg, omsg)
    if host:
        assert ctx.decode_size_host(fmt, data, flags) == (rc, ol, used, msg), tag
    cap = max(ol, 1)
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    drc, dol, dused, dmsg = ctx.decode_device(fmt, d_in.data_ptr(), len(data), d_out.data_ptr(), cap, flags=flags)
    print("decode", tag, (drc, dol, dused, dmsg))
    assert drc != ffi.E_NOSPACE, tag
    if rc != ffi.OK:
        assert msg == dmsg, tag
        assert msg.split(":")[0] == omsg.split(":")[0], (tag, msg, omsg)
    if want is not None:
        assert (rc, ol) == want, tag
    return rc, ol, used, msg


FORMATS = ("DEFLATE", "ZLIB", "GZIP")


def _pyz(fmt_name, raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    wbits = {"DEFLATE": -15, "ZLIB": 15, "GZIP": 31}[fmt_name]
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    return co.compress(raw) + co.flush()


# ------------------------------------------------------------------------------------------------ 1. this library's encoder
@pytest.mark.parametrize("fmt_name", FORMATS)
def test_own_encoder_streams(ctx, ffi, oracle, torch, synth, fmt_name):
    fmt = getattr(ffi, fmt_name)
    rng = np.random.default_rng(7)
    kinds = {"text": lambda n: synth.text(n, seed=synth.SEED_BASE + 301).tobytes() if n else b"",
             "lowent": lambda n: synth.lowent(n, seed=synth.SEED_BASE + 302).tobytes() if n else b"",
             "random": lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()}
    for kind, make in kinds.items():
        for n in (0, 1, 300, 12 * KIB, 64 * KIB, 1 * MIB + 17, 32 * MIB):
            raw = make(n)
            variants = [dict(write_size=8192), dict(write_size=0)]
            if n <= MIB + 17:
                variants += [dict(write_size=8192, dynamic_huffman=0), dict(write_size=8192, no_compression=1)]
                if fmt == ffi.ZLIB:
                    variants.append(dict(writes=[n // 2, None, n - n // 2, None], zlib_flush_mode=ffi.FLUSH_SYNC))
            if n == 32 * MIB and (kind != "text" or fmt != ffi.GZIP):
                variants = variants[:1]
            for v in variants:
                v = dict(v)
                enc = ctx.encode_host(fmt, raw, ffi.make_opts(**{k: x for k, x in v.items() if k not in ("write_size", "writes")}),
                                      ffi.make_schedule(v.get("write_size", 0), v.get("writes")))
                check(ctx, ffi, oracle, torch, fmt, enc, want=(ffi.OK, n), host=n <= MIB + 17)


@pytest.mark.parametrize("fmt_name", FORMATS)
def test_around_the_4k_threshold(ctx, ffi, oracle, torch, synth, fmt_name):
    fmt = getattr(ffi, fmt_name)
    text = synth.text(64 * KIB, seed=synth.SEED_BASE + 303).tobytes()
    hit = {}
    for k in range(4000, 64 * KIB):
        z = _pyz(fmt_name, text[:k])
        if len(z) in (4095, 4096, 4097) and len(z) not in hit:
            hit[len(z)] = (k, z)
        if len(hit) == 3:
            break
    assert sorted(hit) == [4095, 4096, 4097]
    for size, (k, z) in hit.items():
        check(ctx, ffi, oracle, torch, fmt, z, want=(ffi.OK, k))
    stored = lambda raw: ctx.encode_host(fmt, raw, ffi.make_opts(no_compression=1, mtime=1), ffi.make_schedule(0))
    over = len(stored(text[:100])) - 100
    for size in (4095, 4096, 4097):           # the same sizes from this library's stored form
        raw = text[:size - over]
        enc = stored(raw)
        assert len(enc) == size
        check(ctx, ffi, oracle, torch, fmt, enc, want=(ffi.OK, len(raw)))


# ------------------------------------------------------------------------------------------------ 2. other encoders
@pytest.mark.parametrize("fmt_name", FORMATS)
def test_python_zlib_streams(ctx, ffi, oracle, torch, synth, fmt_name):
    fmt = getattr(ffi, fmt_name)
    text = synth.text(32 * MIB, seed=synth.SEED_BASE + 304).tobytes()
    for n in (64 * KIB, 256 * KIB, 2 * MIB, 32 * MIB):
        for level, strategy in ((0, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY),
                                (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED)):
            if n == 32 * MIB and level not in (0, 6):
                continue
            check(ctx, ffi, oracle, torch, fmt, _pyz(fmt_name, text[:n], level, strategy), want=(ffi.OK, n), host=n <= 2 * MIB)
    # stored and fixed blocks between dynamic ones
    co = zlib.compressobj(6, zlib.DEFLATED, {"DEFLATE": -15, "ZLIB": 15, "GZIP": 31}[fmt_name])
    z = b""
    rng = np.random.default_rng(5)
    total = 0
    for i in range(12):
        part = text[total:total + 300 * KIB] if i % 3 != 1 else rng.integers(0, 256, 90 * KIB, dtype=np.uint8).tobytes()
        if i % 3 == 2:
            part = part[:40]            # a tiny block: zlib writes it with the fixed code
        total += len(part)
        z += co.compress(part) + co.flush(zlib.Z_FULL_FLUSH if i % 2 else zlib.Z_SYNC_FLUSH)
    z += co.flush()
    check(ctx, ffi, oracle, torch, fmt, z, want=(ffi.OK, total))


# ------------------------------------------------------------------------------------------------ 3. the reference's vectors
def test_reference_vectors(ctx, ffi, oracle, torch):
    good = [(ffi.DEFLATE, kat.DEFLATE_HELLO), (ffi.DEFLATE, kat.DEFLATE_HELLO_STORED), (ffi.DEFLATE, kat.DEFLATE_HELLO_FIXED),
            (ffi.ZLIB, kat.ZLIB_HELLO), (ffi.ZLIB, kat.ZLIB_HELLO_STORED), (ffi.ZLIB, kat.ZLIB_HELLO_FIXED),
            (ffi.GZIP, kat.GZIP_HELLO_STORED), (ffi.ZLIB, kat.ISSUE27_ZLIB_NONE), (ffi.ZLIB, kat.ISSUE27_ZLIB_SYNC),
            (ffi.GZIP, kat.OFFSET_GZ), (ffi.GZIP, kat.GZIP_MEMBER_HELLO_ + kat.GZIP_MEMBER_WORLD)]
    for fmt, data in good:
        rc, _, _, _ = check(ctx, ffi, oracle, torch, fmt, data)
        assert rc == ffi.OK
    both = kat.GZIP_MEMBER_HELLO_ + kat.GZIP_MEMBER_WORLD
    assert check(ctx, ffi, oracle, torch, ffi.GZIP, both, multi=True)[:3] == (ffi.OK, 12, len(both))
    assert check(ctx, ffi, oracle, torch, ffi.GZIP, kat.OFFSET_GZ)[:2] == (ffi.OK, len(kat.OFFSET_PLAIN))
    enc52 = ctx.encode_host(ffi.DEFLATE, kat.ISSUE52, ffi.make_opts(), ffi.make_schedule(0))
    check(ctx, ffi, oracle, torch, ffi.DEFLATE, enc52, want=(ffi.OK, len(kat.ISSUE52)))
    rc, ol, _, msg = check(ctx, ffi, oracle, torch, ffi.DEFLATE, kat.TOO_LONG_BACKREF)
    assert rc == ffi.E_INVALID_DATA and msg == "Too long backword reference: buffer.len=5, distance=25520"
    rc, ol, _, _ = check(ctx, ffi, oracle, torch, ffi.ZLIB, kat.ISSUE71_IN)
    assert (rc, ol) == (ffi.E_UNEXPECTED_EOF, len(kat.ISSUE71_OUT))


REJECTS = [("DEFLATE", "TOO_LONG_BACKREF"), ("DEFLATE", "ISSUE64"), ("DEFLATE", "ISSUE3_INPUT"), ("GZIP", "ISSUE15_1"),
           ("GZIP", "ISSUE15_2"), ("GZIP", "ISSUE15_3"), ("ZLIB", "ISSUE71_IN"), ("ZLIB", "ISSUE82")]


@pytest.mark.parametrize("fmt_name,vector", REJECTS)
def test_reference_reject_vectors(ctx, ffi, oracle, torch, fmt_name, vector):
    """Status, partial length and consumed of the reference's reject vectors against the oracle."""
    rc, _, _, _ = check(ctx, ffi, oracle, torch, getattr(ffi, fmt_name), getattr(kat, vector))
    assert rc != ffi.OK


def test_reference_reject_vectors_issues_16(ctx, ffi, oracle, torch):
    for d in kat.ISSUES_16:
        rc, _, _, msg = check(ctx, ffi, oracle, torch, ffi.ZLIB, d)
        assert rc != ffi.OK and msg[:31] == "The value of HDIST is too big: max=30, actual=32"[:31]


# ------------------------------------------------------------------------------------------------ 4. damage
def test_truncation_sweep_small(ctx, ffi, oracle, torch, synth):
    text = synth.text(16 * KIB, seed=synth.SEED_BASE + 305).tobytes()
    z = _pyz("GZIP", text[:6000])
    assert 2500 < len(z) < 4000
    for cut in range(len(z) + 1):
        check(ctx, ffi, oracle, torch, ffi.GZIP, z[:cut], host=cut % 16 == 0)


def test_truncation_sweep_large(ctx, ffi, oracle, torch, synth):
    text = synth.text(12 * MIB, seed=synth.SEED_BASE + 306).tobytes()
    z = _pyz("ZLIB", text)
    assert len(z) > 3 * MIB
    rng = np.random.default_rng(11)
    for cut in sorted(int(x) for x in rng.integers(1, len(z), 64)):
        check(ctx, ffi, oracle, torch, ffi.ZLIB, z[:cut], host=False)


def test_bit_flips(ctx, ffi, oracle, torch, synth):
    text = synth.text(3 * MIB, seed=synth.SEED_BASE + 307).tobytes()
    z = bytearray(_pyz("DEFLATE", text))
    assert len(z) > MIB - 200 * KIB
    rng = np.random.default_rng(13)
    for bit in (int(x) for x in rng.integers(0, len(z) * 8, 64)):
        z[bit >> 3] ^= 1 << (bit & 7)
        check(ctx, ffi, oracle, torch, ffi.DEFLATE, z, host=False)
        z[bit >> 3] ^= 1 << (bit & 7)


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, w):                 # LSB first
        self.acc |= v << self.n
        self.n += w
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, v, w):                # a Huffman code: MSB first
        for i in range(w - 1, -1, -1):
            self.put((v >> i) & 1, 1)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)


def test_too_long_reference_inside_a_later_block(ctx, ffi, oracle, torch, synth):
    text = synth.text(2 * MIB, seed=synth.SEED_BASE + 308).tobytes()
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    head = co.compress(text[:100]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(text[100:200]) + co.flush(zlib.Z_FULL_FLUSH)
    b = _Bits()
    b.put(0, 1); b.put(1, 2)                        # a fixed-Huffman block, not final
    b.code(0x30 + 97, 8)                            # literal 'a'
    b.code(1, 7)                                    # length 3
    b.code(29, 5); b.put(0, 13)                     # distance 24577: 201 bytes exist
    b.code(0, 7)                                    # EndOfBlock
    b.put(0, 3); b.align(); b.out += b"\x00\x00\xff\xff"      # an empty stored block: byte aligned again
    tail = zlib.compressobj(6, zlib.DEFLATED, -15)
    z = head + bytes(b.out) + tail.compress(text[200:]) + tail.flush()
    assert len(z) > 500 * KIB
    rc, ol, used, msg = check(ctx, ffi, oracle, torch, ffi.DEFLATE, z)
    assert rc == ffi.E_INVALID_DATA and msg == "Too long backword reference: buffer.len=201, distance=24577"


def test_structural_damage(ctx, ffi, oracle, torch, synth):
    text = synth.text(200 * KIB, seed=synth.SEED_BASE + 309).tobytes()
    assert check(ctx, ffi, oracle, torch, ffi.DEFLATE, b"\x07" + bytes(80))[0] == ffi.E_INVALID_DATA          # BTYPE 3
    assert check(ctx, ffi, oracle, torch, ffi.DEFLATE, b"\x07")[0] == ffi.E_INVALID_DATA
    stored = bytearray(ctx.encode_host(ffi.GZIP, text[:30000], ffi.make_opts(no_compression=1), ffi.make_schedule(0)))
    stored[13] ^= 0x40                                                                                        # NLEN
    assert check(ctx, ffi, oracle, torch, ffi.GZIP, stored)[0] == ffi.E_INVALID_DATA
    for fmt_name, tl in (("ZLIB", 4), ("GZIP", 8)):
        z = _pyz(fmt_name, text)
        fmt = getattr(ffi, fmt_name)
        assert check(ctx, ffi, oracle, torch, fmt, z[:-tl])[0] == ffi.E_UNEXPECTED_EOF                        # no trailer
        assert check(ctx, ffi, oracle, torch, fmt, z[:-1])[0] == ffi.E_UNEXPECTED_EOF                         # a short one
        assert check(ctx, ffi, oracle, torch, fmt, z + b"trailing")[:3] == (ffi.OK, len(text), len(z))


# ------------------------------------------------------------------------------------------------ 5. checksum damage (rule 3)
def _rule3(ctx, ffi, torch, fmt, data, want_len, flags=0):
    d_in = _dev(torch, data)
    rc, ol, used, msg = ctx.decode_size_device(fmt, d_in.data_ptr(), len(data), flags)
    assert (rc, ol) == (ffi.OK, want_len), msg
    assert ctx.decode_size_host(fmt, bytes(data), flags) == (rc, ol, used, msg)
    d_out = torch.empty(max(ol, 1), dtype=torch.uint8, device="cuda")
    return (rc, ol, used), ctx.decode_device(fmt, d_in.data_ptr(), len(data), d_out.data_ptr(), max(ol, 1), flags=flags)


def test_checksum_damage_is_not_seen(ctx, ffi, torch, synth):
    text = synth.text(700 * KIB, seed=synth.SEED_BASE + 310).tobytes()
    for n in (0, 5, 3000, 700 * KIB):
        for fmt_name, where in (("GZIP", -8), ("GZIP", -5), ("GZIP", -4), ("GZIP", -1), ("ZLIB", -4), ("ZLIB", -1)):
            z = bytearray(_pyz(fmt_name, text[:n]))
            z[where] ^= 0x10
            fmt = getattr(ffi, fmt_name)
            (_, ol, used), (drc, dol, dused, dmsg) = _rule3(ctx, ffi, torch, fmt, z, len(zlib.decompress(_pyz("ZLIB", text[:n]))))
            assert used == len(z)
            if fmt_name == "GZIP" and where >= -4:      # ISIZE is read and never verified (gzip.rs:1035-1040)
                assert (drc, dol) == (ffi.OK, ol)
            else:
                assert (drc, dol) == (ffi.E_INVALID_DATA, ol) and "mismatched" in dmsg


def test_multi_member_with_one_bad_crc(ctx, ffi, torch, synth):
    text = synth.text(8 * 100 * KIB, seed=synth.SEED_BASE + 311).tobytes()
    parts = [bytearray(_pyz("GZIP", text[i * 100 * KIB:(i + 1) * 100 * KIB])) for i in range(8)]
    k = 3
    parts[k][-7] ^= 1
    data = b"".join(bytes(p) for p in parts)
    (rc, ol, used), (drc, dol, dused, dmsg) = _rule3(ctx, ffi, torch, ffi.GZIP, data, len(text), flags=ffi.DEC_MULTI)
    assert used == len(data)
    assert drc == ffi.E_INVALID_DATA and dol == (k + 1) * 100 * KIB and dused == sum(len(p) for p in parts[:k + 1])
    rc, ol, used, members, msg = ctx.decode_members_size_host(data)
    assert (rc, ol, used, len(members)) == (ffi.OK, len(text), len(data), 8)


# ------------------------------------------------------------------------------------------------ 6. batch
def _batch_check(ctx, ffi, oracle, torch, fmt, streams):
    """streams: list of bytes.  Every status / out_len / consumed against the oracle on that stream alone, then the batch
    decode laid out from the reported sizes returns the oracle's bytes for every intact stream."""
    offs, at = [], 0
    for s in streams:
        offs.append(at)
        at += len(s)
    blob = b"".join(streams)
    d_in = _dev(torch, blob)
    lens = [len(s) for s in streams]
    out_lens, used, st = ctx.decode_batch_size_device(fmt, d_in.data_ptr(), offs, lens)
    want = [oracle.decode(_ofmt(oracle, ffi, fmt), s) for s in streams]
    want = [(ffi.OK if orc != ffi.OK and _is_checksum(omsg) else orc, oout, oused, omsg) for (orc, oout, oused, omsg) in want]   # rule 3
    for i, (orc, oout, oused, omsg) in enumerate(want):
        assert (st[i], out_lens[i], used[i]) == (orc, len(oout), oused), (i, lens[i], omsg)
    out_offs, at = [], 0
    for ol in out_lens:
        out_offs.append(at)
        at += (ol + 3) & ~3
    d_out = torch.zeros(max(at, 4), dtype=torch.uint8, device="cuda")
    k = len(streams)
    a = lambda v: (C.c_uint64 * k)(*v)
    got_len, got_st = (C.c_uint64 * k)(), (C.c_int32 * k)()
    rc = ffi.lib().lfx_decode_batch_device(ctx.handle, fmt, k, d_in.data_ptr(), a(offs), a(lens), d_out.data_ptr(), a(out_offs),
                                           a(out_lens), got_len, got_st)
    assert rc == ffi.OK
    host = d_out.cpu().numpy()
    for i, (orc, oout, oused, omsg) in enumerate(want):
        assert got_st[i] != ffi.E_NOSPACE, i
        if orc == ffi.OK and not _is_checksum(omsg):
            assert got_st[i] == ffi.OK and host[out_offs[i]:out_offs[i] + out_lens[i]].tobytes() == oout, i
    return out_lens, used, st


def test_batch_4096_streams_of_64k(ctx, ffi, oracle, torch, synth):
    count, size = 4096, 64 * KIB
    plain, data, lens = batch_encoded(ctx, ffi, torch, synth, count, size, synth.SEED_BASE + 312)
    streams, at = [], 0
    for ln in lens:
        streams.append(data[at:at + ln])
        at += ln
    out_lens, used, st = _batch_check(ctx, ffi, oracle, torch, ffi.GZIP, streams)
    assert out_lens == [size] * count and used == lens and not any(st)


def test_batch_python_zlib_streams_with_damage(ctx, ffi, oracle, torch, synth):
    text = synth.text(24 * MIB, seed=synth.SEED_BASE + 313).tobytes()
    rng = np.random.default_rng(17)
    sizes = [int(x) for x in np.exp(rng.uniform(np.log(KIB), np.log(MIB), 512))]
    streams = []
    for i, n in enumerate(sizes):
        at = int(rng.integers(0, len(text) - n))
        streams.append(bytearray(_pyz("ZLIB", text[at:at + n])))
    for q, i in enumerate(range(7, 512, 32)):          # 16 damaged ones spread among them
        s = streams[i]
        if q % 3 == 0:
            del s[len(s) // 2:]
        elif q % 3 == 1:
            s[len(s) // 3] ^= 0x04
        else:
            s[0] ^= 0x0F
    _batch_check(ctx, ffi, oracle, torch, ffi.ZLIB, [bytes(s) for s in streams])


# ------------------------------------------------------------------------------------------------ 7. members
def _members_check(ctx, ffi, oracle, torch, data, max_members=None, crcs_ok=True):
    data = bytes(data)
    d_in = _dev(torch, data)
    rc, ol, used, members, msg = ctx.decode_members_size_device(d_in.data_ptr(), len(data), max_members)
    assert ctx.decode_members_size_host(data, max_members) == (rc, ol, used, members, msg)
    orc, oout, oused, omsg = oracle.decode(oracle.GZIP, data, multi=True)
    assert (rc, ol, used) == (orc, len(oout), oused), (msg, omsg)
    # the table from the oracle's per-member decode
    want, at, oat = [], 0, 0
    while at < len(data):
        mrc, mout, mused, _ = oracle.decode(oracle.GZIP, data[at:])
        if mrc != ffi.OK:
            break
        want.append((at, mused, oat, len(mout)))
        at += mused
        oat += len(mout)
    if max_members is not None:
        want = want[:max_members]
    assert members == want
    if crcs_ok:
        cap = max(ol, 1)
        d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
        drc, dol, dused, dmembers, dmsg = ctx.decode_members_device(d_in.data_ptr(), len(data), d_out.data_ptr(), cap, max_members)
        assert (drc, dol, dused, dmembers, dmsg) == (rc, ol, used, members, msg)
    return rc, ol, used, members


def test_members_batch_encoded(ctx, ffi, oracle, torch, synth):
    count, size = 4096, 64 * KIB
    plain, data, lens = batch_encoded(ctx, ffi, torch, synth, count, size, synth.SEED_BASE + 314)
    rc, ol, used, members = _members_check(ctx, ffi, oracle, torch, data)
    assert (rc, ol, used, len(members)) == (ffi.OK, count * size, len(data), count)
    rc, ol, used, few = _members_check(ctx, ffi, oracle, torch, data, max_members=100)
    assert few == members[:100]


def test_members_bgzf_and_mixed(ctx, ffi, oracle, torch, synth):
    plain, data = small_members(synth, 300, 60 * KIB, synth.SEED_BASE + 315)
    rc, ol, used, members = _members_check(ctx, ffi, oracle, torch, data + BGZF_EOF)
    assert rc == ffi.OK and len(members) == 301 and members[-1] == (len(data), 28, len(plain), 0)
    text = synth.text(6 * MIB, seed=synth.SEED_BASE + 316).tobytes()
    inner = zmember(text[:50 * KIB], name=b"inner.gz")
    parts = [zmember(text[:30 * KIB], strategy=zlib.Z_FIXED, name=b"fixed", comment=b"huffman"),
             zmember(text[:30 * KIB], level=0, extra=b"ZZ\x01\x00q"),
             zmember(inner, level=0),                                   # a stored member that holds a gzip file
             zmember(text[:5 * MIB]),                                   # a long member in between
             ctx.encode_host(ffi.GZIP, text[:200 * KIB], ffi.make_opts(extra=b"AB\x03\x00xyz", hcrc=1), ffi.make_schedule(0)),
             zmember(b"\x1f\x8b\x08\x00" * 2000, level=0),              # a dense candidate tile
             zmember(text[:70 * KIB])]
    whole = b"".join(parts)
    rc, ol, used, members = _members_check(ctx, ffi, oracle, torch, whole)
    assert rc == ffi.OK and len(members) == len(parts)
    _members_check(ctx, ffi, oracle, torch, whole[:-5])                 # truncated last member
    _members_check(ctx, ffi, oracle, torch, whole + b"garbage behind the last member")
    _members_check(ctx, ffi, oracle, torch, whole + bytes(4096))
    _members_check(ctx, ffi, oracle, torch, b"")


def test_members_of_encode_members_bgzf(ctx, ffi, lfx, oracle, torch, synth):
    text = synth.text(5 * MIB + 123, seed=synth.SEED_BASE + 317).tobytes()
    data, table = lfx.gzip.encode_members(text, ffi.BGZF_MEMBER_SIZE, bgzf=True, context=ctx)
    got = lfx.gzip.list_members(data, context=ctx)
    assert got[:-1] == [(o_off, o_len, i_off, i_len) for (i_off, i_len, o_off, o_len) in table]
    assert got[-1] == (len(data) - 28, 28, len(text), 0)
    src = [(i_off, i_len, o_off, o_len) for (o_off, o_len, i_off, i_len) in got[:-1]]
    assert lfx.gzip.members_to_gzi(src) == lfx.gzip.members_to_gzi(table)
    _members_check(ctx, ffi, oracle, torch, data)


# ------------------------------------------------------------------------------------------------ 8. memory
def test_size_call_reserves_less_than_the_output(lfx, ffi, torch, synth):
    n = 1 << 30
    enc_ctx = lfx.Context(0)
    d_plain = torch.from_numpy(synth.lowent(n, seed=synth.SEED_BASE + 5)).to("cuda")
    opts, sched = ffi.make_opts(), ffi.make_schedule(8192)
    bound = ffi.lib().lfx_encode_bound(n, C.byref(opts), C.byref(sched))
    d_z = torch.empty(bound, dtype=torch.uint8, device="cuda")
    zl = C.c_uint64(0)
    assert ffi.lib().lfx_encode_device(enc_ctx.handle, ffi.ZLIB, C.byref(opts), C.byref(sched), d_plain.data_ptr(), n,
                                       d_z.data_ptr(), bound, C.byref(zl)) == 0
    d_in = d_z[:zl.value].clone()
    del d_plain, d_z, enc_ctx
    import gc
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    fresh = lfx.Context(0)
    free0, _ = torch.cuda.mem_get_info()
    rc, ol, used, msg = fresh.decode_size_device(ffi.ZLIB, d_in.data_ptr(), d_in.numel())
    free1, _ = torch.cuda.mem_get_info()
    drop = free0 - free1
    print("decode_size_device of the 1 GiB LOWENT zlib stream (%d compressed bytes): device memory drop %d bytes" % (d_in.numel(), drop))
    assert (rc, ol, used) == (ffi.OK, n, d_in.numel()), msg
    assert drop < n


# ------------------------------------------------------------------------------------------------ 9. Python helpers
def test_python_helpers(lfx, ctx, ffi, torch, synth):
    text = synth.text(3 * MIB, seed=synth.SEED_BASE + 318).tobytes()
    for name in FORMATS:
        z = _pyz(name, text)
        assert lfx.decoded_size(z, format=name.lower(), context=ctx) == len(text)
        assert lfx.decoded_size(_dev(torch, z), format=name.lower(), context=ctx) == len(text)
    two = _pyz("GZIP", text) + _pyz("GZIP", text[:1000])
    assert lfx.decoded_size(two, context=ctx) == len(text)
    assert lfx.decoded_size(two, multi=True, context=ctx) == len(text) + 1000
    with pytest.raises(lfx.StreamError):
        lfx.decoded_size(two[:len(two) // 2], context=ctx)
