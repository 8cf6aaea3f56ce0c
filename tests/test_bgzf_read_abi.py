"""CPU: the ABI of the BGZF reads by virtual offset (lfx_bgzf_read_device / _host, lfx_members_voffset) — declared, exported,
bound, no CPU fallback, the struct layouts, lfx_members_voffset against a bisect — and the MODEL of a read that the GPU tests
expect (tests/test_gpu_bgzf_read.py imports it): a walk that hops by BSIZE alone and zlib per block.  The model is pinned here,
without a GPU, to slices of the known plaintext."""
import bisect
import ctypes as C
import functools
import gzip as pygzip
import os
import random
import re
import struct
import subprocess
import zlib

import pytest

from test_members_encode_abi import BGZF_CASES, BGZF_EOF, model_bgzf, random_bytes, words_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lfx_bgzf_read_device", "lfx_bgzf_read_host", "lfx_members_voffset")
OK, E_INVALID_DATA, E_UNEXPECTED_EOF, E_ARG = 0, 1, 2, 6
VOFF_NONE = 2**64 - 1


# ---------------------------------------------------------------------------------------------- the model
def parse_block(b, p, end):
    """the block that starts at byte p of b, of which bytes [.., end) are held → (block_len, isize), or a status"""
    if end - p < 18:
        return E_UNEXPECTED_EOF
    if not (b[p:p + 4] == b"\x1f\x8b\x08\x04" and b[p + 10:p + 16] == b"\x06\x00BC\x02\x00"):
        return E_INVALID_DATA
    blen = struct.unpack_from("<H", b, p + 16)[0] + 1
    if blen < 26:
        return E_INVALID_DATA
    if p + blen > end:
        return E_UNEXPECTED_EOF
    isize = struct.unpack_from("<I", b, p + blen - 4)[0]
    if isize > 65536:
        return E_INVALID_DATA
    return blen, isize


@functools.lru_cache(maxsize=16384)
def _decode_member(m, isize):
    try:
        d = zlib.decompressobj(-15)
        out = d.decompress(m[18:-8])
        if not d.eof or d.unused_data:
            return None
    except zlib.error:
        return None
    if len(out) != isize or zlib.crc32(out) != struct.unpack_from("<I", m, len(m) - 8)[0]:
        return None
    return out


def decode_block(b, p, blen, isize):
    """the block's output, or None when it does not verify (rule 5)"""
    return _decode_member(bytes(b[p:p + blen]), isize)


def bgzf_read_model(file_bytes, in_base, n, voff, end_voff, length, decode=True, touched=None):
    """one read of include/lfx.h's contract over the held bytes [in_base, in_base + n) of file_bytes
    → (bytes, next_voff, status, n_blocks); decode=False: size mode (bytes is then the count); touched: a set that collects the
    coffsets of the blocks decoded"""
    b, hi = file_bytes, in_base + n
    co, uo = voff >> 16, voff & 0xffff
    e_co, e_uo = end_voff >> 16, end_voff & 0xffff
    out, count = [], 0
    done = lambda nv, st, nb: (b"".join(out) if decode else count, nv, st, nb)
    if co < in_base or co > hi:
        return done(voff, E_ARG, 0)
    if end_voff <= voff or co == hi:
        return done(voff, OK, 0)
    pos, start, first, nb, next_voff = co, uo, True, 0, voff
    while True:
        if pos == hi or pos > e_co or (pos == e_co and e_uo <= start):
            return done(next_voff, OK, nb)
        blk = parse_block(b, pos, hi)
        if isinstance(blk, int):
            return done(pos << 16 | start, blk, nb)
        blen, isize = blk
        if first and uo > isize:
            return done(pos << 16 | start, E_ARG, nb)
        lim = min(isize, e_uo) if pos == e_co else isize
        take = min(max(lim - start, 0), length - count)
        if take:
            if decode:
                data = decode_block(b, pos, blen, isize)
                if touched is not None:
                    touched.add(pos)
                if data is None:
                    return done(pos << 16 | start, E_INVALID_DATA, nb)
                out.append(data[start:start + take])
            nb += 1
        count += take
        at = start + take
        next_voff = (pos + blen) << 16 if at == isize else pos << 16 | at
        if at < isize or count == length or pos >= e_co:
            return done(next_voff, OK, nb)
        pos, start, first = pos + blen, 0, False


def block_table(b):
    """[(coffset, block_len, isize, uncompressed offset)] of a whole BGZF file"""
    p, u, rows = 0, 0, []
    while p < len(b):
        blen, isize = parse_block(b, p, len(b))
        rows.append((p, blen, isize, u))
        p += blen
        u += isize
    return rows


def voff_of(rows, uoff):
    """the virtual offset of uncompressed byte uoff: the last block that starts at or in front of it"""
    i = bisect.bisect_right([r[3] for r in rows], uoff) - 1
    return rows[i][0] << 16 | (uoff - rows[i][3])


def zlib_bgzf(data, sizes, seed=5, eof_at=()):
    """BGZF blocks made by python's zlib (level 6) of sizes[i] input bytes each, the end-of-file marker after the blocks
    numbered in eof_at and at the end (`cat a b`)"""
    out, at = [], 0
    for i, sz in enumerate(sizes):
        sl = data[at:at + sz]
        at += sz
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = c.compress(sl) + c.flush()
        total = 18 + len(body) + 8
        assert total <= 65536
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", total - 1) + body +
                   struct.pack("<II", zlib.crc32(sl), len(sl)))
        if i in eof_at:
            out.append(BGZF_EOF)
    assert at == len(data)
    return b"".join(out) + BGZF_EOF


@pytest.mark.parametrize("name,make,member_size", BGZF_CASES, ids=[c[0] for c in BGZF_CASES])
def test_model_reads_equal_slices_of_the_plaintext(oracle, name, make, member_size):
    data = make()
    f, table, _ = model_bgzf(oracle, data, member_size)
    assert pygzip.decompress(f) == data
    rows = block_table(f)
    assert [r[:2] for r in rows[:-1]] == [(m[2], m[3]) for m in table] and rows[-1][1:3] == (28, 0)
    rnd = random.Random(11)
    offs = [0, len(data)] + [r[3] for r in rows[:4]] + [rnd.randrange(len(data) + 1) for _ in range(40)]
    for off in offs:
        for length in (0, 1, 5000, 70000, 200000, len(data) + 5):
            v = voff_of(rows, off)
            got, nv, st, nb = bgzf_read_model(f, 0, len(f), v, VOFF_NONE, length)
            want = data[off:off + length]
            assert (got, st) == (want, OK), (name, off, length)
            # bgzf_tell: the position of the byte behind the last one delivered; at the end of the file, its end
            end = off + len(want)
            if length == 0:
                pass
            elif end == len(data) and length > len(want):
                assert nv == len(f) << 16
            else:
                i = bisect.bisect_right([r[3] for r in rows], end) - 1
                same = rows[i][0] << 16 | (end - rows[i][3])
                # (a position at a block's end is named as the start of the block behind it, empty blocks not skipped)
                assert nv == same or (end - rows[i][3] == 0 and nv >> 16 <= rows[i][0] and nv & 0xffff == 0), (name, off, length)
            touched = {r[0] for r in rows if end > off and r[3] < end and r[3] + r[2] > off}
            assert nb == len(touched)
            # size mode agrees without decoding; end_voff at the read's own end changes nothing but stops it there
            assert bgzf_read_model(f, 0, len(f), v, VOFF_NONE, length, decode=False) == (len(want), nv, OK, nb)
            if want:
                got2 = bgzf_read_model(f, 0, len(f), v, voff_of(rows, end), len(data) + 7)
                assert got2[0] == want and got2[2] == OK


def test_model_errors_and_windows():
    data = words_text(200000, seed=2)
    f = zlib_bgzf(data, [50000, 60000, 40000, 50000], eof_at=(1,))
    assert pygzip.decompress(f) == data
    rows = block_table(f)
    assert [r[2] for r in rows] == [50000, 60000, 0, 40000, 50000, 0]
    full = lambda v, ln, e=VOFF_NONE: bgzf_read_model(f, 0, len(f), v, e, ln)
    # across the marker in the middle; a start at uoffset == ISIZE; the end of the file
    assert full(rows[1][0] << 16 | 59990, 20) == (data[109990:110010], rows[3][0] << 16 | 10, OK, 2)
    assert full(rows[0][0] << 16 | 50000, 3) == (data[50000:50003], rows[1][0] << 16 | 3, OK, 1)
    assert full(rows[4][0] << 16 | 49999, 10) == (data[199999:], len(f) << 16, OK, 1)
    assert full(len(f) << 16, 10) == (b"", len(f) << 16, OK, 0)
    assert full(rows[0][0] << 16 | 50001, 3)[2] == E_ARG and full((len(f) + 1) << 16, 3)[2] == E_ARG
    assert full((rows[1][0] + 5) << 16, 3)[1:] == ((rows[1][0] + 5) << 16, E_INVALID_DATA, 0)
    # end_voff: inside the start block, at a block start, in front of voff; len first
    assert full(5, 100, 25) == (data[5:25], 25, OK, 1)
    assert full(5, 10, 25) == (data[5:15], 15, OK, 1)
    assert full(5, 10**6, rows[1][0] << 16) == (data[5:50000], rows[1][0] << 16, OK, 1)
    assert full(5, 100, 5) == (b"", 5, OK, 0) and full(5, 100, 4) == (b"", 5, OK, 0)
    # a held window that ends inside block 3: the bytes in front of it, UnexpectedEof, its start
    lo, hi = rows[1][0], rows[3][0] + 100
    got = bgzf_read_model(f, lo, hi - lo, rows[1][0] << 16 | 100, VOFF_NONE, 10**6)
    assert got == (data[50100:110000], rows[3][0] << 16, E_UNEXPECTED_EOF, 1)
    rest = full(got[1], 10**6)
    assert got[0] + rest[0] == data[50100:] and rest[2] == OK
    assert bgzf_read_model(f, lo, hi - lo, 0, VOFF_NONE, 5)[2] == E_ARG
    # a flipped payload byte: the prefix, InvalidData, the damaged block's first wanted byte; size mode does not see it
    bad = bytearray(f)
    bad[rows[1][0] + 40] ^= 0x10
    bad = bytes(bad)
    assert bgzf_read_model(bad, 0, len(bad), 49990, VOFF_NONE, 100) == (data[49990:50000], rows[1][0] << 16, E_INVALID_DATA, 1)
    assert bgzf_read_model(bad, 0, len(bad), 49990, VOFF_NONE, 100, decode=False) == (100, rows[1][0] << 16 | 90, OK, 2)
    assert bgzf_read_model(bad, 0, len(bad), 0, VOFF_NONE, 100)[2] == OK


# ---------------------------------------------------------------------------------------------- the ABI
@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as g
    g.build()
    from libflate_amd import _ffi
    return _ffi


def test_declared_exported_bound(ffi):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lfx_[a-z0-9_]+)\s*\(", hdr))
    out = subprocess.run(["nm", "-D", "--defined-only", ffi.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines()}
    for name in NAMES:
        assert name in declared, name
        assert name in exported, name
        assert name in ffi.EXPORTS, name
        assert hasattr(ffi.lib(), name), name
    assert ffi.VOFF_NONE == VOFF_NONE
    import libflate_amd
    assert libflate_amd.bgzf.voffset(5, 7) == 5 << 16 | 7 and libflate_amd.bgzf.split(5 << 16 | 7) == (5, 7)


def test_struct_layouts(ffi):
    assert C.sizeof(ffi.BgzfRead) == 32 and C.sizeof(ffi.BgzfResult) == 24
    for field, off in (("voff", 0), ("end_voff", 8), ("len", 16), ("out_off", 24)):
        assert getattr(ffi.BgzfRead, field).offset == off, field
    for field, off in (("out_len", 0), ("next_voff", 8), ("status", 16), ("n_blocks", 20)):
        assert getattr(ffi.BgzfResult, field).offset == off, field
    hdr = open(os.path.join(ROOT, "include", "lfx.h")).read()
    assert re.search(r"\}\s*lfx_bgzf_read;\s*/\* 32 bytes \*/", hdr) and re.search(r"\}\s*lfx_bgzf_result;\s*/\* 24 bytes \*/", hdr)


def test_null_context_is_a_device_error(ffi):
    L = ffi.lib()
    reads = (ffi.BgzfRead * 2)()
    reads[0].len = reads[1].len = 8
    reads[1].out_off = 8
    res = (ffi.BgzfResult * 2)()
    for r in res:
        r.out_len, r.next_voff, r.status, r.n_blocks = 7, 7, 7, 7
    decoded = C.c_uint64(7)
    buf = C.create_string_buffer(b"\xA5" * 64, 64)
    assert L.lfx_bgzf_read_device(None, None, 0, 0, 2, reads, None, res, C.byref(decoded)) == ffi.E_DEVICE
    assert L.lfx_bgzf_read_host(None, BGZF_EOF, 0, 28, 2, reads, buf, res, C.byref(decoded)) == ffi.E_DEVICE
    assert L.lfx_bgzf_read_host(None, BGZF_EOF, 0, 28, 0, None, None, None, None) == ffi.E_DEVICE
    assert decoded.value == 7 and buf.raw == b"\xA5" * 64
    assert all((r.out_len, r.next_voff, r.status, r.n_blocks) == (7, 7, 7, 7) for r in res)


def voffset_model(rows, uoff):
    """rows: (compressed offset, compressed length, uncompressed offset, uncompressed length) in file order → voff or None"""
    total = rows[-1][2] + rows[-1][3] if rows else 0
    if uoff > total:
        return None
    if uoff == total:
        return (rows[-1][0] + rows[-1][1] if rows else 0) << 16
    i = bisect.bisect_right([r[2] for r in rows], uoff) - 1
    return rows[i][0] << 16 | (uoff - rows[i][2])


def check_voffset(ffi, members, swapped):
    L = ffi.lib()
    rows = [(m[0], m[1], m[2], m[3]) if swapped else (m[2], m[3], m[0], m[1]) for m in members]
    table = (ffi.Member * max(len(members), 1))()
    for i, m in enumerate(members):
        table[i].in_off, table[i].in_len, table[i].out_off, table[i].out_len = m
    total = rows[-1][2] + rows[-1][3] if rows else 0
    rnd = random.Random(3)
    points = {0, total, total + 1, total + 12345} | {r[2] for r in rows} | {max(r[2] - 1, 0) for r in rows} | \
             {r[2] + 1 for r in rows if r[3] > 1} | {rnd.randrange(total + 1) for _ in range(200)}
    for u in sorted(points):
        v = C.c_uint64(0xA5A5)
        rc = L.lfx_members_voffset(table if members else None, len(members), 1 if swapped else 0, u, C.byref(v))
        want = voffset_model(rows, u)
        if want is None:
            assert rc == ffi.E_ARG and v.value == 0xA5A5, u
            with pytest.raises(ffi.LfxError):
                ffi.members_voffset(members, u, swapped)
        else:
            assert (rc, v.value) == (ffi.OK, want), u
            assert ffi.members_voffset(members, u, swapped) == want
    return rows


def test_members_voffset(ffi, oracle):
    data = words_text(400 * 1000) + random_bytes(70000)
    f, table, _ = model_bgzf(oracle, data, 65280)
    rows = check_voffset(ffi, table, False)
    # the table agrees with the file: every located position reads the byte it names
    blocks = block_table(f)
    assert [(r[0], r[1]) for r in rows] == [b[:2] for b in blocks[:-1]]
    for u in (0, 65279, 65280, 65281, len(data) - 1):
        v = voffset_model(rows, u)
        assert bgzf_read_model(f, 0, len(f), v, VOFF_NONE, 1)[0] == data[u:u + 1]
    assert voffset_model(rows, len(data)) == (len(f) - 28) << 16
    # a decoder-style table: the roles exchanged, the marker as one more, empty member; one in the middle too
    dec = [(m[2], m[3], m[0], m[1]) for m in table] + [(len(f) - 28, 28, len(data), 0)]
    check_voffset(ffi, dec, True)
    mid = dec[:3] + [(dec[3][0], 28, dec[3][2], 0)] + [(m[0] + 28, m[1], m[2], m[3]) for m in dec[3:]]
    rows = check_voffset(ffi, mid, True)
    assert voffset_model(rows, mid[3][2]) == mid[4][0] << 16          # a boundary: the later member, not the empty one
    check_voffset(ffi, [(0, 1000, 0, 300)], False)
    check_voffset(ffi, [(0, 300, 0, 1000)], True)
    check_voffset(ffi, [], False)
    check_voffset(ffi, [], True)
    # a position more than 65535 bytes into its member has no virtual offset
    big = (ffi.Member * 1)()
    big[0].in_off, big[0].in_len, big[0].out_off, big[0].out_len = 0, 1 << 20, 0, 5000
    v = C.c_uint64(0)
    assert ffi.lib().lfx_members_voffset(big, 1, 0, 65535, C.byref(v)) == ffi.OK and v.value == 65535
    assert ffi.lib().lfx_members_voffset(big, 1, 0, 65536, C.byref(v)) == ffi.E_ARG
    assert ffi.lib().lfx_members_voffset(big, 1, 0, 0, None) == ffi.E_ARG
