"""GPU: the block rounds that the batch decode, the members walk and the reads of a seek index share (scan_round / emit_round,
DESIGN.md §4.0).  A round's bookkeeping is by index — job, emit job, owner — so the inputs make streams leave a round in
DIFFERENT ways at once: done, continuing, dropped by the scan, emitted but flagged, over their capacity.  Bodies are raw
DEFLATE of python-zlib cut into exactly k blocks (Z_BLOCK after every 8 KiB, where zlib never cuts by itself; the window is
kept, so later blocks read earlier ones) — k = 1...6 (five and six are more blocks than the fast path has rounds), a stored
one, a Z_FIXED one, and one under the fast path's 64-byte floor.  Integer work: every comparison is exact."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_parity import ctx, ffi, lfx, synth  # noqa: F401  (fixtures)
from test_gpu_decode_size import _is_checksum
from test_gpu_index import build
from test_gpu_members import BGZF_EOF, _dev, check, torch  # noqa: F401

KIB = 1 << 10
CHUNK = 8 * KIB


def zblocks(raw, sizes=None, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    """raw DEFLATE of `raw`, a block per entry of `sizes` (default: per 8 KiB) → (body, cuts); cuts[i] = bytes of the body
    written when block i was closed (the block ends in the byte at or right behind that offset)"""
    sizes = sizes or [CHUNK] * (len(raw) // CHUNK) or [len(raw)]
    assert sum(sizes) == len(raw)
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    body, cuts, at = b"", [], 0
    for i, n in enumerate(sizes):
        body += co.compress(raw[at:at + n])
        body += co.flush(zlib.Z_BLOCK if i + 1 < len(sizes) else zlib.Z_FINISH)
        cuts.append(len(body))
        at += n
    assert zlib.decompress(body, -15) == raw
    return body, cuts


@pytest.fixture(scope="module")
def bodies(synth):
    """[(name, raw, body, cuts)], neighbours of different kinds"""
    text = synth.text(64 * CHUNK, seed=synth.SEED_BASE + 1201).tobytes()
    out, at = [], 0
    for name, k, kw in (("k3", 3, {}), ("stored", 2, dict(level=0)), ("k1", 1, {}), ("k5", 5, {}), ("fixed", 2, dict(strategy=zlib.Z_FIXED)),
                        ("k2", 2, {}), ("tiny", 0, {}), ("k6", 6, {}), ("k4", 4, {})):
        n = k * CHUNK if k else 40
        raw = text[at:at + n]
        at += n
        out.append((name, raw) + zblocks(raw, **kw))
    assert len(dict((b[0], b) for b in out)["tiny"][2]) + 6 < 64
    return out


def zwrap(raw, body):
    return b"\x78\x9c" + body + struct.pack(">I", zlib.adler32(raw) & 0xFFFFFFFF)


def gzwrap(raw, body, bgzf):
    trailer = struct.pack("<II", zlib.crc32(raw) & 0xFFFFFFFF, len(raw))
    if bgzf:
        return b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<HBBHH", 6, 66, 67, 2, 18 + len(body) + 8 - 1) + body + trailer
    return b"\x1f\x8b\x08\0\0\0\0\0\0\x03" + body + trailer


def test_batch_mixed_exits(ctx, ffi, oracle, torch, bodies):
    by = dict((b[0], b) for b in bodies)
    streams = [(name, raw, zwrap(raw, body), len(raw)) for name, raw, body, _ in bodies]
    _, raw3, body3, cuts3 = by["k3"]
    bad = bytearray(zwrap(raw3, body3))
    bad[2 + (cuts3[0] + cuts3[1]) // 2] ^= 0x10                         # a byte inside the second block
    streams.insert(2, ("flip3", raw3, bytes(bad), len(raw3)))
    streams.insert(5, ("cut3", raw3, zwrap(raw3, body3)[:2 + (cuts3[1] + cuts3[2]) // 2], len(raw3)))    # ends inside the third
    _, raw2, body2, _ = by["k2"]
    streams.insert(8, ("short2", raw2, zwrap(raw2, body2), len(raw2) - 1))
    k = len(streams)
    in_len = [len(s[2]) for s in streams]
    in_off = [sum(in_len[:i]) for i in range(k)]
    out_cap = [s[3] for s in streams]
    out_off = [sum((c + 259) & ~255 for c in out_cap[:i]) for i in range(k)]
    d_in = _dev(torch, b"".join(s[2] for s in streams))
    d_out = torch.full((out_off[-1] + out_cap[-1] + 256,), 0x5A, dtype=torch.uint8, device="cuda")
    a = lambda v: (C.c_uint64 * k)(*v)
    got_len, got_st = (C.c_uint64 * k)(), (C.c_int32 * k)()
    rc = ffi.lib().lfx_decode_batch_device(ctx.handle, ffi.ZLIB, k, d_in.data_ptr(), a(in_off), a(in_len), d_out.data_ptr(), a(out_off),
                                           a(out_cap), got_len, got_st)
    assert rc == ffi.OK
    host = d_out.cpu().numpy()
    want = [oracle.decode(oracle.ZLIB, s[2]) for s in streams]
    for i, (name, raw, s, cap) in enumerate(streams):
        orc, oout, oused, omsg = want[i]
        print(name, "status", got_st[i], "out_len", got_len[i], "oracle", orc, len(oout), oused, omsg)
        if name == "short2":
            assert got_st[i] == ffi.E_NOSPACE and got_len[i] <= cap
        elif name in ("flip3", "cut3"):
            assert orc != ffi.OK and (got_st[i], got_len[i]) == (orc, len(oout)), name
        else:
            assert (got_st[i], got_len[i]) == (ffi.OK, len(raw)) and orc == ffi.OK, name
            assert host[out_off[i]:out_off[i] + len(raw)].tobytes() == raw == oout == zlib.decompress(s), name
    # the size call on the same list: the oracle's verdicts (a checksum mismatch is not seen: the size calls compute none)
    out_lens, used, st = ctx.decode_batch_size_device(ffi.ZLIB, d_in.data_ptr(), in_off, in_len)
    for i, (orc, oout, oused, omsg) in enumerate(want):
        orc = ffi.OK if orc != ffi.OK and _is_checksum(omsg) else orc
        assert (st[i], out_lens[i], used[i]) == (orc, len(oout), oused), streams[i][0]


def test_members_mixed_exits(ctx, ffi, oracle, torch, bodies):
    members = [gzwrap(raw, body, bgzf=i % 2 == 1) for i, (_, raw, body, _) in enumerate(bodies)]
    starts = [sum(len(m) for m in members[:i]) for i in range(len(members))]
    data = b"".join(members) + BGZF_EOF
    plain = b"".join(b[1] for b in bodies)
    names = [b[0] for b in bodies]

    def sizes(d):
        d_in = _dev(torch, d)
        return ctx.decode_members_size_device(d_in.data_ptr(), len(d))

    # ---- as is
    rc, out, used, table = check(ctx, ffi, oracle, torch, data, want_status=ffi.OK)
    assert out == plain and used == len(data) and len(table) == len(members) + 1
    clean = (rc, len(out), used, table, "")
    assert sizes(data) == clean
    # ---- the CRC of a member in the middle: the verified members in front of it; the size call computes no checksum
    mid = names.index("fixed")
    bad = bytearray(data)
    bad[starts[mid] + len(members[mid]) - 8] ^= 0x40
    rc, out, used, table = check(ctx, ffi, oracle, torch, bytes(bad), want_status=ffi.E_INVALID_DATA)
    assert len(table) == mid and used == starts[mid] + len(members[mid])
    assert sizes(bytes(bad)) == clean
    # ---- a byte inside block 2 of the 3-block member
    m3 = names.index("k3")
    cuts = bodies[m3][3]
    hdr = 18 if m3 % 2 == 1 else 10
    bad = bytearray(data)
    bad[starts[m3] + hdr + (cuts[0] + cuts[1]) // 2] ^= 0x10
    rc, out, used, table = check(ctx, ffi, oracle, torch, bytes(bad))
    assert rc != ffi.OK and len(table) == m3
    d_in = _dev(torch, bytes(bad))
    d_out = torch.zeros(len(plain) + 4096, dtype=torch.uint8, device="cuda")
    dec = ctx.decode_members_device(d_in.data_ptr(), len(bad), d_out.data_ptr(), len(plain) + 4096)
    got = sizes(bytes(bad))
    if _is_checksum(dec[4]):       # (a flip that still decodes is a checksum mismatch, which the size call does not see)
        assert got == clean
    else:
        assert got == dec


def test_index_read_mixed_exits(ctx, ffi, torch, synth):
    sizes = [3 * KIB, 20 * KIB, 3 * KIB, 40 * KIB, 5 * KIB]
    raw = synth.text(sum(sizes), seed=synth.SEED_BASE + 1202).tobytes()
    comp, _ = zblocks(raw, sizes)
    rc, out, idx = build(ctx, ffi, torch, comp, ffi.DEFLATE, spacing=4096)
    assert rc == ffi.OK and out == raw
    pts = idx.points
    P = [p[2] for p in pts] + [len(raw)]
    big0, big1 = sum(sizes[:3]), sum(sizes[:4])
    inner = [i for i, p in enumerate(pts) if p[0] != p[1]]
    assert any(sizes[0] < pts[i][2] < sum(sizes[:2]) for i in inner) and any(big0 < pts[i][2] < big1 for i in inner)
    f = [i for i in inner if big0 < pts[i][2] < big1][1]            # the damaged segment: inside the 40 KiB block, not its first
    assert f >= 5 and f + 2 < len(pts)
    reads = [(P[1] + 7, (P[2] - P[1]) // 2),         # ends inside a segment
             (P[2], P[3] - P[2]),                    # exactly one segment
             (P[1] + 5, P[3] - P[1]),                # three segments
             (P[2], 0),                              # empty
             (len(raw) - 1, 1),                      # the last byte
             (P[f - 1] + 9, P[f + 1] - P[f - 1]),    # three segments, the damaged one in the middle
             (P[f], P[f + 1] - P[f]),                # exactly the damaged one
             (P[f] + 100, 50)]                       # ends inside it
    touches_f = [False] * 5 + [True] * 3
    got = idx.read_many(comp, reads)
    for (o, ln), g in zip(reads, got):
        assert g.cpu().numpy().tobytes() == raw[o:o + ln], (o, ln)
    # ---- a byte of the held input flipped inside the 40 KiB block, among the bytes point f vouches for: the reads that
    # touch segment f fail, and nothing else changes (every other segment decodes from its own point and window)
    d_in = _dev(torch, comp)
    d_in[pts[f][0] // 8 + 8] ^= 0x10
    lens = [ln for _, ln in reads]
    offs = [sum(lens[:i]) for i in range(len(reads))]
    d_out = torch.full((sum(lens) + 16,), 0x33, dtype=torch.uint8, device="cuda")
    rc, got_len, st, msg = ctx.index_read_device(idx._h, d_in.data_ptr(), 0, len(comp), [o for o, _ in reads], lens, d_out.data_ptr(), offs)
    host = d_out.cpu().numpy().tobytes()
    print("read statuses", st, "lens", got_len, "message", msg)
    assert rc == ffi.E_INVALID_DATA and "index point" in msg
    for i, (o, ln) in enumerate(reads):
        if touches_f[i]:
            assert st[i] == ffi.E_INVALID_DATA, i
        else:
            assert (st[i], got_len[i]) == (ffi.OK, ln) and host[offs[i]:offs[i] + ln] == raw[o:o + ln], i
    assert host[sum(lens):] == b"\x33" * 16
