"""GPU: lfx_bgzf_read_device / _host — batched reads of a BGZF file by virtual offset.  Every expectation is
the model's of tests/test_bgzf_read_abi.py (a walk by BSIZE alone, zlib per block), pinned there to the plaintext without a
GPU.  Output buffers are pre-filled with 0xA5 and carry guard bytes around every read's range: the whole buffer is compared,
so nothing may be written outside out_off .. out_off + out_len."""
import ctypes as C
import math
import random
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_parity import ctx, ffi, lfx, synth  # noqa: F401  (fixtures)
from test_bgzf_read_abi import (E_ARG, E_INVALID_DATA, E_UNEXPECTED_EOF, OK, VOFF_NONE, bgzf_read_model, block_table, voff_of,
                                zlib_bgzf)
from test_members_encode_abi import random_bytes, words_text

GUARD = 64


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def file_a(lfx, ctx):
    """compressed and stored blocks, 40 of them"""
    data = words_text(1900 * 1000) + random_bytes(700 * 1000)
    f, members = lfx.gzip.encode_members(data, 65280, bgzf=True, context=ctx)
    rows = block_table(f)
    assert len(rows) == 41 and rows[-1][2] == 0 and max(r[1] for r in rows) > 65280
    return data, f, rows, members


@pytest.fixture(scope="module")
def file_b():
    """python-zlib blocks of 3000 .. 65280 input bytes, the end-of-file marker in the middle and at the end"""
    rnd = random.Random(21)
    sizes = [rnd.randrange(3000, 65281) for _ in range(28)] + [65280, 3000]
    data = words_text(sum(sizes), seed=4)
    f = zlib_bgzf(data, sizes, eof_at=(13,))
    rows = block_table(f)
    assert [r[2] for r in rows].count(0) == 2 and rows[14][2] == 0
    return data, f, rows


@pytest.fixture(scope="module")
def file_c():
    """5000 blocks of 256 input bytes: more than one group of 4096"""
    data = words_text(5000 * 256, seed=6)
    f = zlib_bgzf(data, [256] * 5000)
    return data, f, block_table(f)


def _dev(torch, data):
    a = np.frombuffer(bytes(data), dtype=np.uint8).copy() if len(data) else np.zeros(1, dtype=np.uint8)
    return torch.from_numpy(a).to("cuda")


def call(ffi, fn, handle, src, in_base, n, reads4, dst):
    k = len(reads4)
    arr = (ffi.BgzfRead * max(k, 1))()
    for i, (voff, length, end_voff, out_off) in enumerate(reads4):
        arr[i].voff, arr[i].len, arr[i].end_voff, arr[i].out_off = voff, length, end_voff, out_off
    res = (ffi.BgzfResult * max(k, 1))()
    decoded = C.c_uint64(0xA5)
    rc = fn(handle, src, in_base, n, k, arr, dst, res, C.byref(decoded))
    return rc, [(r.out_len, r.next_voff, r.status, r.n_blocks) for r in res[:k]], decoded.value


def check(ctx, ffi, torch, f, reads, in_base=0, n=None, host=False, size_equals_read=True, count_decoded=True):
    """reads: (voff, length[, end_voff]).  Device call, size mode and (host) the host call with pageable and page-locked input
    against the model → (results, model, blocks_decoded)"""
    L = ffi.lib()
    n = len(f) - in_base if n is None else n
    reads = [(r[0], r[1], r[2] if len(r) > 2 else VOFF_NONE) for r in reads]
    touched = set()
    want = [bgzf_read_model(f, in_base, n, v, e, ln, touched=touched) for v, ln, e in reads]
    sized = [bgzf_read_model(f, in_base, n, v, e, ln, decode=False) for v, ln, e in reads]
    offs, at = [], GUARD
    for _, ln, _ in reads:
        offs.append(at)
        at += ln + GUARD
    reads4 = [(v, ln, e, o) for (v, ln, e), o in zip(reads, offs)]
    expect = bytearray(b"\xA5" * at)
    for o, w in zip(offs, want):
        expect[o:o + len(w[0])] = w[0]
    expect = bytes(expect)
    want_res = [(len(w[0]), w[1], w[2], w[3]) for w in want]
    want_rc = next((w[2] for w in want if w[2] != OK), OK)
    held = f[in_base:in_base + n]
    d_in = _dev(torch, held)
    d_out = torch.full((at,), 0xA5, dtype=torch.uint8, device="cuda")
    rc, res, decoded = call(ffi, L.lfx_bgzf_read_device, ctx.handle, d_in.data_ptr(), in_base, n, reads4, d_out.data_ptr())
    torch.cuda.synchronize()
    whole = d_out.cpu().numpy().tobytes()
    bad = [i for i in range(len(reads)) if res[i] != want_res[i]]
    assert not bad, (bad[:5], [res[i] for i in bad[:5]], [want_res[i] for i in bad[:5]], ctx.last_error())
    assert rc == want_rc
    if rc != OK:
        assert "BGZF" in ctx.last_error()
    if whole != expect:
        i = next(i for i in range(at) if whole[i] != expect[i])
        raise AssertionError("output differs at byte %d (ranges start at %r ...)" % (i, offs[:4]))
    if count_decoded:
        assert decoded == len(touched)
    # size mode: the same walk, nothing decoded, nothing written
    rc2, res2, decoded2 = call(ffi, L.lfx_bgzf_read_device, ctx.handle, d_in.data_ptr(), in_base, n, reads4, None)
    assert res2 == sized and decoded2 == 0
    assert rc2 == next((s[2] for s in sized if s[2] != OK), OK)
    if size_equals_read:
        assert res2 == res
    if host:
        for pinned in (False, True):
            buf = C.create_string_buffer(b"\xA5" * at, at)
            ptr = None
            if pinned:
                ptr = L.lfx_host_alloc(max(n, 1))
                assert ptr
                C.memmove(ptr, held, n)
            try:
                rc3, res3, decoded3 = call(ffi, L.lfx_bgzf_read_host, ctx.handle, ptr if pinned else held, in_base, n, reads4, buf)
            finally:
                if pinned:
                    L.lfx_host_free(ptr)
            assert (rc3, res3, decoded3) == (rc, res, decoded), pinned
            assert buf.raw == expect, pinned
            rc4, res4, decoded4 = call(ffi, L.lfx_bgzf_read_host, ctx.handle, held, in_base, n, reads4, None)
            assert (rc4, res4, decoded4) == (rc2, res2, 0)
    return res, want, decoded


def v(rows, i, uo=0):
    return rows[i][0] << 16 | uo


# ---------------------------------------------------------------------------------------------- 1, 2: single reads
def test_single_reads(ctx, ffi, torch, file_a, file_b):
    data, f, rows = file_b
    reads = [
        (v(rows, 3, 1000), 500),                         # inside one block
        (v(rows, 4, 0), 1), (v(rows, 4, rows[4][2] - 1), 1),   # a block's first and last byte
        (v(rows, 5, 77), rows[5][2] + rows[6][2] + 10),  # over three blocks
        (v(rows, 13, rows[13][2] - 5), 4000),            # across the end-of-file marker in the middle
        (v(rows, 7, rows[7][2]), 300),                   # a start at uoffset == ISIZE
        (v(rows, 28, 100), 10**6),                       # to the end of the file: short
        (v(rows, 2, 5), 0), (v(rows, 2, rows[2][2]), 0),  # len == 0
        (len(f) << 16, 100),                             # voff at the end of the input
        (v(rows, 14, 0), 10),                            # a start AT the marker in the middle
    ]
    res, want, _ = check(ctx, ffi, torch, f, reads, host=True)
    assert res[3][3] == 3 and res[4][3] == 2 and res[6][1] == len(f) << 16 and res[9] == (0, len(f) << 16, OK, 0)
    assert want[4][0] == data[rows[13][3] + rows[13][2] - 5:][:4000]
    # the same on the library's own blocks (stored ones among them)
    data, f, rows, _ = file_a
    stored = next(i for i, r in enumerate(rows) if r[1] > 65280)
    check(ctx, ffi, torch, f, [(v(rows, stored - 1, 65000), 70000), (v(rows, 0, 0), 1), (v(rows, 39, 10), 10**6), (0, 3 * 65280)],
          host=True)


def test_end_voff(ctx, ffi, torch, file_b):
    data, f, rows = file_b
    e9 = rows[9][2] // 2
    reads = [
        (v(rows, 3, 100), 10**5, v(rows, 3, 900)),       # inside the start block
        (v(rows, 3, 100), 10**6, v(rows, 6)),            # at a block start
        (v(rows, 27, 100), 10**6, (len(f) + 50) << 16),  # behind the file
        (v(rows, 3, 100), 500, v(rows, 3, 100)), (v(rows, 3, 100), 500, v(rows, 2, 5000)), (v(rows, 3, 100), 500, 0),   # <= voff
        (v(rows, 8, 10), 10**6, v(rows, 9, e9)),         # reached before len
        (v(rows, 8, 10), 777, v(rows, 9, e9)),           # len reached before it
        (v(rows, 12, 0), 10**6, v(rows, 15, 1)),         # over the marker, one byte into the block behind it
        (v(rows, 12, 0), 10**6, v(rows, 14)),            # at the marker
        (v(rows, 10, 5), 10**6, (rows[11][0] + 7) << 16),  # end_voff inside a block's bytes: the walk passes it at the next start
    ]
    res, want, _ = check(ctx, ffi, torch, f, reads, host=True)
    assert res[0] == (800, v(rows, 3, 900), OK, 1) and res[1][1] == v(rows, 6) and res[1][3] == 3
    assert res[3] == res[4] == res[5] == (0, v(rows, 3, 100), OK, 0)
    assert res[6][0] == rows[8][2] - 10 + e9 and res[7][0] == 777


def test_empty_blocks_literal(ctx, ffi, torch, file_b):
    """end_voff and len around the empty blocks (the end-of-file marker in the middle, rows[14], and at the end): expectations
    written out by hand from rules 2 and 6 of include/lfx.h and taken from the plaintext, not from the model"""
    data, f, rows = file_b
    i12, i13, i15 = rows[12][2], rows[13][2], rows[15][2]
    u12, u15, end = rows[12][3], rows[15][3], len(f) << 16
    assert rows[14][1] == 28 and rows[14][2] == 0 and rows[-1][1] == 28 and rows[15][3] == rows[14][3] == u12 + i12 + i13
    reads = [
        (v(rows, 12), 10**6, v(rows, 14)),               # 0 end_voff AT the empty block: stops in front of it
        (v(rows, 12), 10**6, v(rows, 15)),               # 1 right behind it: the empty block is passed
        (v(rows, 12), 10**6, v(rows, 14, 5)),            # 2 a uoffset behind the empty block's ISIZE: the same
        (v(rows, 12), 10**6, v(rows, 15, 1)),            # 3 one byte of the block behind it
        (v(rows, 12), i12 + i13),                        # 4 len ends with block 13: next_voff is the next block's start
        (v(rows, 12), i12 + i13 + 1),                    # 5 one byte more: over the empty block
        (v(rows, 14), 10),                               # 6 a start AT the empty block
        (v(rows, 14), 10, v(rows, 14, 9)),               # 7 ... with end_voff inside it: nothing, the block is passed
        (v(rows, 14), 0),                                # 8 len == 0 there: uoffset == ISIZE, so the next block's start
        (v(rows, len(rows) - 1), 10),                    # 9 a start at the marker that ends the file
        (v(rows, 30, 2990), 10**6, v(rows, len(rows) - 1)),   # 10 end_voff at that marker
        (v(rows, 30, 2990), 10**6, end),                 # 11 end_voff at the end of the file
    ]
    res, want, _ = check(ctx, ffi, torch, f, reads, host=True)
    both = data[u12:u15]
    assert res[0] == (i12 + i13, v(rows, 14), OK, 2) and want[0][0] == both
    assert res[1] == res[2] == (i12 + i13, v(rows, 15), OK, 2) and want[1][0] == want[2][0] == both
    assert res[3] == (i12 + i13 + 1, v(rows, 15, 1), OK, 3) and want[3][0] == data[u12:u15 + 1]
    assert res[4] == (i12 + i13, v(rows, 14), OK, 2) and want[4][0] == both
    assert res[5] == res[3] and want[5][0] == want[3][0]
    assert res[6] == (10, v(rows, 15, 10), OK, 1) and want[6][0] == data[u15:u15 + 10]
    assert res[7] == (0, v(rows, 15), OK, 0) and res[8] == (0, v(rows, 15), OK, 0)
    assert res[9] == (0, end, OK, 0)
    assert len(rows) == 32 and rows[30][2] == 3000 and res[10] == (10, v(rows, len(rows) - 1), OK, 1) and res[11] == (10, end, OK, 1)
    assert want[10][0] == want[11][0] == data[-10:] and i15 > 10


def test_refused_call_leaves_res_untouched(ctx, ffi, torch, file_b):
    """rule 8: a call refused as a whole writes nothing to res (nor to the output), which is how Context._bgzf_call tells it from
    a read's own LFX_E_ARG"""
    data, f, rows = file_b
    L = ffi.lib()
    d_in = _dev(torch, f)
    d_out = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda")
    out = C.create_string_buffer(b"\xA5" * 4096, 4096)

    def reads_of(*r):
        arr = (ffi.BgzfRead * len(r))()
        for i, (voff, length, out_off) in enumerate(r):
            arr[i].voff, arr[i].len, arr[i].end_voff, arr[i].out_off = voff, length, VOFF_NONE, out_off
        return arr

    two = reads_of((0, 100, 0), (v(rows, 2), 100, 200))
    refused = [
        ("overlap", 0, len(f), reads_of((0, 100, 0), (v(rows, 2), 100, 99))),
        ("NULL reads", 0, len(f), None),
        ("2^48", 2**48 - 10, 100, reads_of(((2**48 - 10) << 16 & (2**64 - 1), 100, 0), (0, 100, 200))),
        ("in_base + n wraps", 2**64 - 10, 100, two),
    ]
    for name, in_base, n, arr in refused:
        for host in (False, True):
            res = (ffi.BgzfResult * 2)()
            C.memset(res, 0x5A, C.sizeof(res))
            decoded = C.c_uint64(7)
            if host:
                rc = L.lfx_bgzf_read_host(ctx.handle, f, in_base, n, 2, arr, out, res, C.byref(decoded))
            else:
                rc = L.lfx_bgzf_read_device(ctx.handle, d_in.data_ptr(), in_base, n, 2, arr, d_out.data_ptr(), res, C.byref(decoded))
            assert rc == E_ARG and "BGZF" in ctx.last_error(), (name, host)
            assert bytes(res) == b"\x5A" * C.sizeof(res) and decoded.value == 0, (name, host)
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().tobytes() == out.raw == b"\xA5" * 4096
    # a read's own LFX_E_ARG is a result, not a refusal: res is written, the other read served
    res = (ffi.BgzfResult * 2)()
    C.memset(res, 0x5A, C.sizeof(res))
    own = reads_of(((len(f) + 1) << 16, 100, 0), (v(rows, 2), 100, 200))
    assert L.lfx_bgzf_read_device(ctx.handle, d_in.data_ptr(), 0, len(f), 2, own, d_out.data_ptr(), res, None) == E_ARG
    assert (res[0].out_len, res[0].status, res[0].n_blocks) == (0, E_ARG, 0) and (res[1].out_len, res[1].status) == (100, OK)
    assert d_out[200:300].cpu().numpy().tobytes() == data[rows[2][3]:rows[2][3] + 100]
    # the Python wrapper: the one is returned, the other raised
    rc, r, _, _, msg = ctx.bgzf_read_device(d_in.data_ptr(), 0, len(f), [((len(f) + 1) << 16, 100, VOFF_NONE, 0), (0, 5, VOFF_NONE, 200)],
                                            d_out.data_ptr())
    assert rc == E_ARG and r[0][2] == E_ARG and r[1] == (5, 5, OK, 1) and "outside" in msg
    with pytest.raises(ffi.LfxError):
        ctx.bgzf_read_device(d_in.data_ptr(), 2**48 - 10, 100, [(0, 5, VOFF_NONE, 0)], d_out.data_ptr())
    with pytest.raises(ffi.LfxError):
        ctx.bgzf_read_host(f, [(0, 5)], in_base=2**48 - 10)


# ---------------------------------------------------------------------------------------------- 3: many reads in one call
def random_reads(rows, total, count, seed):
    rnd = random.Random(seed)
    reads = []
    for _ in range(count):
        off = rnd.randrange(total)
        length = min(200000, int(math.exp(rnd.uniform(0, math.log(200000)))) + rnd.choice((0, 0, 0, 65280)))
        reads.append((voff_of(rows, off), max(length, 1)))
    reads[0] = (reads[0][0], 1)
    reads[1] = (reads[1][0], 200000)
    return reads


@pytest.mark.parametrize("which", ["a", "b"])
def test_2000_random_reads(ctx, ffi, torch, file_a, file_b, which):
    data, f, rows = file_a[:3] if which == "a" else file_b
    reads = random_reads(rows, len(data), 2000, 5 if which == "a" else 6)
    res, want, decoded = check(ctx, ffi, torch, f, reads, host=True)
    assert all(r[2] == OK for r in res)
    # (check() has compared blocks_decoded with the distinct blocks the model touches)
    assert 0 < decoded <= sum(1 for r in rows if r[2]) and decoded < sum(r[3] for r in res)
    rnd = random.Random(9)
    for i in rnd.sample(range(2000), 50):             # the model itself against the plaintext, once more
        co, uo = reads[i][0] >> 16, reads[i][0] & 0xffff
        u = next(r[3] for r in rows if r[0] == co) + uo
        assert want[i][0] == data[u:u + reads[i][1]]


# ---------------------------------------------------------------------------------------------- 4: more than one group
def test_5000_blocks(ctx, ffi, torch, file_c):
    data, f, rows = file_c
    reads = [(0, len(data))] + [(v(rows, i, (i * 7) % 256), 1) for i in range(5000)]
    res, want, decoded = check(ctx, ffi, torch, f, reads)
    assert decoded == 5000 and res[0] == (len(data), v(rows, 5000), OK, 5000) and want[0][0] == data
    assert all(res[1 + i] == (1, v(rows, i, (i * 7) % 256 + 1) if (i * 7) % 256 < 255 else v(rows, i + 1), OK, 1) for i in range(5000))


# ---------------------------------------------------------------------------------------------- 5: a held window
def test_held_window(ctx, ffi, torch, file_a):
    data, f, rows, _ = file_a
    in_base, end = rows[5][0], rows[12][0] + 1000
    first = (v(rows, 6, 100), 10**6)
    res, want, _ = check(ctx, ffi, torch, f, [first, (v(rows, 7, 0), 50), (0, 10), ((end + 1) << 16, 10), (v(rows, 12, 0), 5),
                                           (v(rows, 11, 3), 10**6, v(rows, 12))],
                      in_base=in_base, n=end - in_base)
    got = sum(r[2] for r in rows[6:12]) - 100
    assert res[0] == (got, v(rows, 12), E_UNEXPECTED_EOF, 6)
    assert res[2][2] == res[3][2] == E_ARG and res[4] == (0, v(rows, 12), E_UNEXPECTED_EOF, 0) and res[5][2] == OK
    # fewer than 18 bytes of the next block held: the same verdict
    res2, _, _ = check(ctx, ffi, torch, f, [first], in_base=in_base, n=rows[12][0] + 7 - in_base)
    assert res2[0] == res[0]
    # the window ends at a block boundary: a short read, OK
    res3, _, _ = check(ctx, ffi, torch, f, [first], in_base=in_base, n=rows[12][0] - in_base)
    assert res3[0] == (got, v(rows, 12), OK, 6)
    # the caller goes on from next_voff on the full file: together, one uninterrupted read
    rest = 300000
    res4, want4, _ = check(ctx, ffi, torch, f, [(res[0][1], rest)])
    whole = bgzf_read_model(f, 0, len(f), first[0], VOFF_NONE, got + rest)
    assert want[0][0] + want4[0][0] == whole[0] and res4[0][1] == whole[1] and whole[2] == OK


# ---------------------------------------------------------------------------------------------- 6: damage
def test_damage(ctx, ffi, torch, lfx, file_b):
    data, f, rows = file_b
    bad = bytearray(f)
    bad[rows[9][0] + 18 + 300] ^= 0x04               # a payload byte of block 9
    bad = bytes(bad)
    reads = [
        (v(rows, 8, 100), 10**5),                        # starts in front of it: the prefix
        (v(rows, 9, 50), 10),                            # inside it: nothing
        (v(rows, 7, 0), rows[7][2] + rows[8][2]),        # ends right in front of it: untouched
        (v(rows, 10, 0), 10**5), (v(rows, 3, 9), 70000), (v(rows, 20, 1), 1),   # elsewhere
        ((rows[4][0] + 9) << 16, 10),                    # a voff into the middle of a block
        (v(rows, 5, rows[5][2] + 1), 10),                # uoffset > ISIZE
        (v(rows, 6, 0), 200000),                         # runs into it three blocks on
    ]
    res, want, _ = check(ctx, ffi, torch, bad, reads, host=True, size_equals_read=False, count_decoded=False)
    assert res[0] == (rows[8][2] - 100, v(rows, 9), E_INVALID_DATA, 1) and res[1] == (0, v(rows, 9, 50), E_INVALID_DATA, 0)
    assert [r[2] for r in res[2:6]] == [OK] * 4 and res[6][2] == E_INVALID_DATA and res[7][2] == E_ARG
    assert res[8] == (sum(r[2] for r in rows[6:9]), v(rows, 9), E_INVALID_DATA, 3)
    d_bad = _dev(torch, bad)
    d_tmp = torch.zeros((10**5,), dtype=torch.uint8, device="cuda")
    rc, _, _ = call(ffi, ffi.lib().lfx_bgzf_read_device, ctx.handle, d_bad.data_ptr(), 0, len(bad), [reads[0] + (VOFF_NONE, 0)], d_tmp.data_ptr())
    assert rc == E_INVALID_DATA and "coffset %d" % rows[9][0] in ctx.last_error()
    # size mode does not decode: the damaged payload is not seen
    sized = [bgzf_read_model(bad, 0, len(bad), r[0], VOFF_NONE, r[1], decode=False) for r in reads]
    assert [s[2] for s in sized] == [OK, OK, OK, OK, OK, OK, E_INVALID_DATA, E_ARG, OK]
    # the message of a header that is none names the coffset
    rc, r1, _ = call(ffi, ffi.lib().lfx_bgzf_read_device, ctx.handle, _dev(torch, f).data_ptr(), 0, len(f), [reads[6] + (VOFF_NONE, 0)], None)
    assert rc == E_INVALID_DATA and "coffset %d" % (rows[4][0] + 9) in ctx.last_error()
    # ISIZE patched to disagree with the decoded length, one too small and one too large
    for blk, delta in ((11, -1), (16, 1)):
        p = bytearray(f)
        at = rows[blk][0] + rows[blk][1] - 4
        p[at:at + 4] = struct.pack("<I", rows[blk][2] + delta)
        res, _, _ = check(ctx, ffi, torch, bytes(p), [(v(rows, blk - 1, 10), 10**5), (v(rows, blk + 1, 0), 100)], host=True,
                       size_equals_read=False, count_decoded=False)
        assert res[0] == (rows[blk - 1][2] - 10, v(rows, blk), E_INVALID_DATA, 1) and res[1][2] == OK
    # overlapping output ranges: LFX_E_ARG for the call, nothing written
    d_in = _dev(torch, f)
    d_out = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda")
    rc, r2, _ = call(ffi, ffi.lib().lfx_bgzf_read_device, ctx.handle, d_in.data_ptr(), 0, len(f),
                     [(0, 100, VOFF_NONE, 0), (v(rows, 2), 100, VOFF_NONE, 99)], d_out.data_ptr())
    torch.cuda.synchronize()
    assert rc == E_ARG and "overlap" in ctx.last_error() and r2 == [(0, 0, 0, 0)] * 2
    assert d_out.cpu().numpy().tobytes() == b"\xA5" * 4096
    with pytest.raises(ffi.LfxError):
        ctx.bgzf_read_device(d_in.data_ptr(), 0, len(f), [(0, 100, VOFF_NONE, 0), (0, 100, VOFF_NONE, 50)], d_out.data_ptr())
    rc, r2, _ = call(ffi, ffi.lib().lfx_bgzf_read_device, ctx.handle, d_in.data_ptr(), 0, len(f),
                     [(0, 100, VOFF_NONE, 0), (0, 0, VOFF_NONE, 50), (0, 100, VOFF_NONE, 100)], d_out.data_ptr())
    assert rc == OK                                  # (a range of no bytes overlaps nothing; adjacent ranges do not overlap)
    # degenerate arguments
    L = ffi.lib()
    assert L.lfx_bgzf_read_device(ctx.handle, d_in.data_ptr(), 0, len(f), 0, None, None, None, None) == OK
    assert L.lfx_bgzf_read_device(ctx.handle, d_in.data_ptr(), 0, len(f), 1, None, None, None, None) == E_ARG
    assert L.lfx_bgzf_read_host(ctx.handle, f, 0, len(f), 1, (ffi.BgzfRead * 1)(), None, None, None) == E_ARG


# ---------------------------------------------------------------------------------------------- 9: Python
def test_python_module(ctx, ffi, lfx, file_a, file_b):
    data, f, rows, members = file_a
    bgzf = lfx.bgzf
    got = bgzf.read(f, [(v(rows, 3, 10), 100), (v(rows, 3, 10), 10**6, v(rows, 5)), (v(rows, 39, 0), 10**6)], context=ctx)
    u3 = rows[3][3]
    assert got[0] == (data[u3 + 10:u3 + 110], v(rows, 3, 110))
    assert got[1] == (data[u3 + 10:rows[5][3]], v(rows, 5)) and got[2] == (data[rows[39][3]:], len(f) << 16)
    assert bgzf.sizes(f, [(v(rows, 3, 10), 100), (0, 10**9)], context=ctx) == [(100, v(rows, 3, 110), 1), (len(data), len(f) << 16, 40)]
    listed = lfx.gzip.list_members(f, context=ctx)
    for off, length in ((0, 10), (65279, 2), (65280, 65280), (123456, 300000), (len(data) - 5, 100), (len(data), 10)):
        if off < len(data):       # (behind the last byte the two tables name different, equally good positions)
            assert bgzf.locate(members, off) == bgzf.locate(listed, off, swapped=True)
        assert bgzf.read_range(f, members, off, length, context=ctx) == data[off:off + length]
        assert bgzf.read_range(f, listed, off, length, swapped=True, context=ctx) == data[off:off + length]
    assert bgzf.locate(members, 65280) == v(rows, 1) and bgzf.locate(members, len(data)) == v(rows, 40)
    with pytest.raises(lfx.StreamError) as e:
        bgzf.locate(members, len(data) + 1)
    assert e.value.status == E_ARG
    with pytest.raises(lfx.StreamError) as e:
        bgzf.read(f, [(0, 10), ((rows[2][0] + 1) << 16, 10)], context=ctx)
    assert e.value.status == E_INVALID_DATA and "coffset %d" % (rows[2][0] + 1) in e.value.message
    # Context.bgzf_read_host: the tuple the issue names
    rc, res, decoded, out, msg = ctx.bgzf_read_host(f, [(0, 5), (v(rows, 1), 7, v(rows, 1, 3))])
    assert (rc, res, decoded, out, msg) == (OK, [(5, 5, OK, 1), (3, v(rows, 1, 3), OK, 1)], 2, [data[:5], data[65280:65283]], "")
    rc, res, decoded, out, msg = ctx.bgzf_read_host(f, [(0, 5)], sizes_only=True)
    assert (rc, res, decoded, out) == (OK, [(5, 5, OK, 1)], 0, None)


# ---------------------------------------------------------------------------------------------- 10: the context afterwards
def test_context_stays_usable_and_phases(ctx, ffi, lfx, torch, file_a):
    data, f, rows, members = file_a
    bad = bytearray(f)
    bad[rows[2][0] + 500] ^= 0x40
    with pytest.raises(lfx.StreamError):
        lfx.bgzf.read(bytes(bad), [(0, 10**6)], context=ctx)
    assert lfx.gzip.decode_members(f, context=ctx)[0] == data
    assert lfx.gzip.encode_members(data, 65280, bgzf=True, context=ctx) == (f, members)
    d_in = _dev(torch, f)
    d_out = torch.zeros((300000,), dtype=torch.uint8, device="cuda")
    ctx.enable_timing(True)
    try:
        rc, res, decoded, _, _ = ctx.bgzf_read_device(d_in.data_ptr(), 0, len(f), [(v(rows, 1, 5), 200000, VOFF_NONE, 0)], d_out.data_ptr())
        names = [p[0] for p in ctx.last_timing()["phases"]]
    finally:
        ctx.enable_timing(False)
    assert rc == OK and res[0][0] == 200000 and decoded == 4 and names == ["hop", "plan", "batch", "gather"]
    assert d_out[:200000].cpu().numpy().tobytes() == data[65285:265285]
