"""CPU: the members encoder's ABI (lfx_encode_members_bound / _device / _host, lfx_members_gzi) — declared, exported, bound, no
CPU fallback, the bound's formula, the .gzi layout — and the MODEL of the bytes the GPU tests expect (tests/
test_gpu_members_encode.py imports it): per slice the oracle's gzip stream, for BGZF with the BC subfield, BSIZE patched in, the
stored form above 65536 bytes and the end-of-file marker.  The model is proved here without a GPU: Python's gzip reads it back,
and a walk that hops by BSIZE alone lands on its end."""
import ctypes as C
import gzip as pygzip
import os
import random
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

NAMES = ("lfx_encode_members_bound", "lfx_encode_members_device", "lfx_encode_members_host", "lfx_members_gzi")
GZIP = 2
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
BC0 = b"BC\x02\x00\x00\x00"
KIB, MIB = 1 << 10, 1 << 20


# ---------------------------------------------------------------------------------------------- inputs and the model
def words_text(n, seed=1):
    """seeded text of 2-9 letter words"""
    r = random.Random(seed)
    words = [bytes(r.choices(b"abcdefghijklmnopqrstuvwxyz", k=r.randint(2, 9))) for _ in range(2000)]
    out, size = [], 0
    while size < n:
        w = r.choice(words)
        out.append(w)
        size += len(w) + 1
    return b" ".join(out)[:n]


def random_bytes(n, seed=7):
    return np.random.RandomState(seed).randint(0, 256, size=n, dtype=np.uint8).tobytes()


def mixed(seed=3):
    """text + random + text, 250 KB: at 65505 per member one member lies wholly in the random part"""
    t = words_text(100000, seed)
    return t + random_bytes(100000, seed) + t[:50000]


def slices(data, member_size):
    if not data:
        return [b""]
    return [data[i:i + member_size] for i in range(0, len(data), member_size)]


def model_plain(oracle, data, member_size, write_size=0, **kw):
    """→ (bytes, [(in_off, in_len, out_off, out_len)])"""
    out, table, at, src = [], [], 0, 0
    for sl in slices(data, member_size):
        m = oracle.encode(GZIP, sl, write_size=write_size, **kw)
        out.append(m)
        table.append((src, len(sl), at, len(m)))
        at += len(m)
        src += len(sl)
    return b"".join(out), table


def model_bgzf(oracle, data, member_size, **kw):
    """→ (bytes, table, stored fallbacks)"""
    out, table, at, src, fallbacks = [], [], 0, 0, 0
    for sl in (slices(data, member_size) if data else []):
        m = oracle.encode(GZIP, sl, extra=BC0, **kw)
        if len(m) > 65536:
            m = oracle.encode(GZIP, sl, extra=BC0, **dict(kw, no_compression=1))
            fallbacks += 1
        assert len(m) <= 65536 and m[10:18] == b"\x06\x00" + BC0
        m = m[:16] + struct.pack("<H", len(m) - 1) + m[18:]
        out.append(m)
        table.append((src, len(sl), at, len(m)))
        at += len(m)
        src += len(sl)
    return b"".join(out) + BGZF_EOF, table, fallbacks


def walk_bsize(b):
    """hops from member to member by BSIZE alone → the members' lengths (the marker is one of them)"""
    p, lens = 0, []
    while p < len(b):
        assert b[p:p + 4] == b"\x1f\x8b\x08\x04" and b[p + 10:p + 16] == b"\x06\x00BC\x02\x00", p
        size = struct.unpack_from("<H", b, p + 16)[0] + 1
        lens.append(size)
        p += size
    assert p == len(b)
    return lens


def gzi_model(table):
    return struct.pack("<Q", max(len(table) - 1, 0)) + b"".join(struct.pack("<QQ", m[2], m[0]) for m in table[1:])


BGZF_CASES = [   # name, data, member_size
    ("text", lambda: words_text(772 * 1000), 65280),
    ("random", lambda: random_bytes(300 * 1000), 65280),
    ("random_full", lambda: random_bytes(300 * 1000), 65505),
    ("mixed", mixed, 65505),
    ("empty", lambda: b"", 65280),
]


# ---------------------------------------------------------------------------------------------- the model, on the CPU
@pytest.mark.parametrize("name,make,member_size", BGZF_CASES, ids=[c[0] for c in BGZF_CASES])
def test_model_bgzf_is_valid(oracle, name, make, member_size):
    data = make()
    want, table, fallbacks = model_bgzf(oracle, data, member_size)
    assert pygzip.decompress(want) == data
    lens = walk_bsize(want)
    n_members = -(-len(data) // member_size)
    assert len(lens) == n_members + 1 and lens[-1] == 28          # (the walk counts the marker)
    assert [m[3] for m in table] == lens[:-1] and max(lens) <= 65536
    print(name, len(data), "members walked", len(lens), "fallbacks", fallbacks, "largest", max(lens))
    if name == "text":
        assert fallbacks == 0
    if name == "random":          # 65280 random bytes cost 65385 as a dynamic block: they fit
        assert fallbacks == 0 and max(lens) > 65280
    if name == "random_full":     # every full member falls back to one stored block of exactly 65536 bytes
        assert fallbacks == len(data) // member_size and max(lens) == 65536
    if name == "mixed":           # both paths in one call
        assert 0 < fallbacks < n_members
    if name == "empty":
        assert want == BGZF_EOF and table == []


def test_model_plain_is_valid(oracle):
    data = words_text(300 * 1000) + random_bytes(5000)
    for ms in (4096, 65536, MIB):
        want, table = model_plain(oracle, data, ms)
        assert pygzip.decompress(want) == data
        assert len(table) == -(-len(data) // ms) and table[-1][2] + table[-1][3] == len(want)
    want, table = model_plain(oracle, b"", 4096)
    assert pygzip.decompress(want) == b"" and table == [(0, 0, 0, len(want))]


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
    assert re.search(r"LFX_MEMBERS_BGZF\s*=\s*1u", hdr) and ffi.MEMBERS_BGZF == 1


def test_null_context_is_a_device_error(ffi):
    L = ffi.lib()
    out_len, count = C.c_uint64(7), C.c_uint32(7)
    table = (ffi.Member * 4)()
    buf = C.create_string_buffer(b"\xA5" * 256, 256)
    for flags in (0, ffi.MEMBERS_BGZF):
        assert L.lfx_encode_members_device(None, None, None, 4096, flags, None, 0, None, 0, C.byref(out_len), table, 4,
                                           C.byref(count)) == ffi.E_DEVICE
        assert L.lfx_encode_members_host(None, None, None, 4096, flags, b"abc", 3, buf, 256, C.byref(out_len), table, 4,
                                         C.byref(count)) == ffi.E_DEVICE
    # nothing was computed on the CPU: the outputs are untouched
    assert out_len.value == 7 and count.value == 7 and buf.raw == b"\xA5" * 256 and table[0].out_len == 0


def test_bound_formula(ffi):
    L = ffi.lib()
    for kw, sched in (({}, None), ({"dynamic_huffman": 0}, None), ({"filename": b"a.txt"}, ffi.make_schedule(8192)),
                      ({"no_compression": 1}, None)):
        o = ffi.make_opts(**kw)
        sp = C.byref(sched) if sched is not None else None
        one = lambda n: L.lfx_encode_bound(n, C.byref(o), sp)
        for n, ms in ((0, 4096), (1, 4096), (4095, 4096), (4096, 4096), (4097, 4096), (10 * MIB + 17, MIB), (300000, 65536),
                      (5, 1 << 40)):
            full, last = divmod(n, ms)
            want = full * one(ms) + (one(last) if last or n == 0 else 0)
            assert L.lfx_encode_members_bound(n, ms, 0, C.byref(o), sp) == want, (kw, n, ms)
    o = ffi.make_opts()
    one = lambda n: min(L.lfx_encode_bound(n, C.byref(o), None), 65536)
    for n, ms in ((0, 65280), (1, 65280), (65280, 65280), (65281, 65280), (300000, 65505), (772000, 65280), (1000, 100)):
        full, last = divmod(n, ms)
        want = full * one(ms) + (one(last) if last else 0) + 28
        assert L.lfx_encode_members_bound(n, ms, ffi.MEMBERS_BGZF, C.byref(o), None) == want, (n, ms)
    assert L.lfx_encode_members_bound(0, 65280, ffi.MEMBERS_BGZF, None, None) == 28
    assert L.lfx_encode_members_bound(100, 10, 0, None, None) == 10 * L.lfx_encode_bound(10, None, None)


def test_bound_refuses_what_the_call_refuses(ffi):
    """arguments out of their domain need no device to be found: the bound is 0 (the messages: the GPU tests)"""
    L = ffi.lib()
    B = ffi.MEMBERS_BGZF
    ok = ffi.make_opts()
    assert L.lfx_encode_members_bound(1000, 0, 0, C.byref(ok), None) == 0
    assert L.lfx_encode_members_bound(1000, 0, B, C.byref(ok), None) == 0
    assert L.lfx_encode_members_bound(1000, 4096, 2, C.byref(ok), None) == 0
    assert L.lfx_encode_members_bound(1000, 65505, B, C.byref(ok), None) > 0
    assert L.lfx_encode_members_bound(1000, 65506, B, C.byref(ok), None) == 0
    assert L.lfx_encode_members_bound(1000, 65506, 0, C.byref(ok), None) > 0
    for kw in ({"extra": b"AB\x01\x00x"}, {"filename": b"f"}, {"comment": b"c"}, {"hcrc": 1}):
        o = ffi.make_opts(**kw)
        assert L.lfx_encode_members_bound(1000, 65280, B, C.byref(o), None) == 0, kw
        assert L.lfx_encode_members_bound(1000, 65280, 0, C.byref(o), None) > 0, kw
    for sched in (ffi.make_schedule(8192), ffi.make_schedule(writes=[100, None, 200])):
        assert L.lfx_encode_members_bound(1000, 65280, B, C.byref(ok), C.byref(sched)) == 0
        assert L.lfx_encode_members_bound(1000, 65280, 0, C.byref(ok), C.byref(sched)) > 0
    assert L.lfx_encode_members_bound(1000, 65280, B, C.byref(ok), C.byref(ffi.make_schedule())) > 0
    # two blocks per member (block_size <= member_size): the stored form is 36 + member_size bytes
    small = ffi.make_opts(block_size=4096)
    assert L.lfx_encode_members_bound(1000, 65500, B, C.byref(small), None) > 0
    assert L.lfx_encode_members_bound(1000, 65501, B, C.byref(small), None) == 0


def test_gzi_layout(ffi):
    L = ffi.lib()
    rows = [(0, 65280, 0, 20001), (65280, 65280, 20001, 65385), (130560, 100, 85386, 77)]
    table = (ffi.Member * 3)()
    for i, r in enumerate(rows):
        table[i].in_off, table[i].in_len, table[i].out_off, table[i].out_len = r
    want = struct.pack("<Q", 2) + struct.pack("<QQ", 20001, 65280) + struct.pack("<QQ", 85386, 130560)
    assert want == gzi_model(rows)
    buf = C.create_string_buffer(b"\xA5" * 64, 64)
    n = C.c_uint64(0)
    assert L.lfx_members_gzi(table, 3, buf, 64, C.byref(n)) == ffi.OK
    assert n.value == 40 and buf.raw[:40] == want and buf.raw[40:] == b"\xA5" * 24
    # a short cap: LFX_E_NOSPACE, *len set, nothing written
    buf = C.create_string_buffer(b"\xA5" * 64, 64)
    n = C.c_uint64(0)
    assert L.lfx_members_gzi(table, 3, buf, 39, C.byref(n)) == ffi.E_NOSPACE
    assert n.value == 40 and buf.raw == b"\xA5" * 64
    assert L.lfx_members_gzi(table, 3, None, 0, C.byref(n)) == ffi.E_NOSPACE and n.value == 40
    # no member, one member: the count alone
    for k in (0, 1):
        n = C.c_uint64(0)
        assert L.lfx_members_gzi(table if k else None, k, buf, 64, C.byref(n)) == ffi.OK
        assert n.value == 8 and buf.raw[:8] == bytes(8)
    assert ffi.members_to_gzi(rows) == want and ffi.members_to_gzi([]) == bytes(8)
    from libflate_amd import gzip as lgzip
    assert lgzip.members_to_gzi(rows) == want
