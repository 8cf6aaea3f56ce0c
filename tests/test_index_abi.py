"""CPU: the seek index's ABI (lfx_decode_index_device and friends, lfx_index_point, lfx_index_info) — declared, exported, bound,
no CPU fallback — the serialised format's validation (lfx_index_check), and the index kernels' loops (tools/isa_scan.py)."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess
import sys
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NAMES = ("lfx_decode_index_device", "lfx_index_read_device", "lfx_index_span", "lfx_index_get_info", "lfx_index_get_point",
         "lfx_index_export", "lfx_index_import", "lfx_index_check", "lfx_index_free")
KERNELS = ("idx_copy_kernel", "idx_lanes_kernel", "idx_probe_kernel")


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
    assert "typedef struct lfx_index_point" in hdr and "typedef struct lfx_index_info" in hdr


def test_struct_layouts(ffi):
    assert C.sizeof(ffi.IndexPoint) == 40
    for field, off in (("in_bit", 0), ("hdr_bit", 8), ("out_off", 16), ("member", 24), ("win_len", 28), ("in_crc", 32),
                       ("btype", 36)):
        assert getattr(ffi.IndexPoint, field).offset == off, field
    assert C.sizeof(ffi.IndexInfo) == 56
    for field, off in (("in_len", 0), ("out_len", 8), ("spacing", 16), ("max_gap", 24), ("export_bytes", 32), ("format", 40),
                       ("flags", 44), ("n_points", 48), ("n_members", 52)):
        assert getattr(ffi.IndexInfo, field).offset == off, field


def test_null_context_is_a_device_error(ffi):
    L = ffi.lib()
    out_len, used, h = C.c_uint64(7), C.c_uint64(7), C.c_void_p(1234)
    assert L.lfx_decode_index_device(None, 2, 0, None, 0, None, 0, C.byref(out_len), C.byref(used), 1 << 20, C.byref(h)) \
        == ffi.E_DEVICE
    assert out_len.value == 7 and used.value == 7 and h.value == 1234
    offs = (C.c_uint64 * 1)(0)
    ol, st = (C.c_uint64 * 1)(7), (C.c_int32 * 1)(7)
    assert L.lfx_index_read_device(None, None, None, 0, 0, 1, offs, offs, None, offs, ol, st) == ffi.E_DEVICE
    assert ol[0] == 7 and st[0] == 7
    n = C.c_uint64(7)
    assert L.lfx_index_export(None, None, None, 0, C.byref(n)) == ffi.E_DEVICE
    assert n.value == 7
    s = C.c_int32(0)
    blob = _blob()
    assert not L.lfx_index_import(None, blob, len(blob), C.byref(s))
    assert s.value == ffi.E_DEVICE


# ---- the serialised format, built here from its documentation in lfx.h
def _point(in_bit, hdr_bit, out_off, member, win_len, in_crc=0, btype=2, pad=b"\0\0\0"):
    return struct.pack("<QQQIIIB3s", in_bit, hdr_bit, out_off, member, win_len, in_crc, btype, pad)


def _blob(points=None, fmt=2, flags=1, in_len=100000, out_len=400000, spacing=65536, max_gap=70000, n_members=2,
          reserved=0, version=1, magic=b"LFXINDEX", windows=None, crc_fix=True):
    if points is None:
        # member 0: a start, a point inside a block, a block start; member 1: its start and one more point
        points = [(80, 80, 0, 0, 0, 0, 2), (9000, 80, 60000, 0, 32768, 0, 2), (20000, 20000, 120000, 0, 32768, 0, 1),
                  (400000, 400000, 200000, 1, 0, 0, 2), (450000, 440000, 210000, 1, 10000, 0, 2)]
    recs = b"".join(_point(*p) for p in points)
    if windows is None:
        windows = b"".join(bytes([i & 0xFF]) * p[4] for i, p in enumerate(points))
    head = magic + struct.pack("<IIIIQQQQII", version, fmt, flags, len(points), in_len, out_len, spacing, max_gap, n_members,
                               reserved)
    body = head + recs + windows
    return body + struct.pack("<I", zlib.crc32(body) if crc_fix else 0)


def _check(ffi, blob):
    info = ffi.IndexInfo()
    return ffi.lib().lfx_index_check(blob, len(blob), C.byref(info)), info


def test_check_accepts_the_documented_format(ffi):
    blob = _blob()
    rc, info = _check(ffi, blob)
    assert rc == ffi.OK
    assert (info.n_points, info.n_members, info.format, info.flags) == (5, 2, 2, 1)
    assert (info.in_len, info.out_len, info.spacing, info.max_gap, info.export_bytes) == (100000, 400000, 65536, 70000, len(blob))
    # one member without LFX_DEC_MULTI, raw DEFLATE
    pts = [(0, 0, 0, 0, 0, 0, 1), (5000, 0, 40000, 0, 32768, 0, 1)]
    assert _check(ffi, _blob(pts, fmt=0, flags=0, n_members=1))[0] == ffi.OK


BASE = [(80, 80, 0, 0, 0, 0, 2), (9000, 80, 60000, 0, 32768, 0, 2), (20000, 20000, 120000, 0, 32768, 0, 1),
        (400000, 400000, 200000, 1, 0, 0, 2), (450000, 440000, 210000, 1, 10000, 0, 2)]


def _with(i, **kw):
    pts = [list(p) for p in BASE]
    names = ("in_bit", "hdr_bit", "out_off", "member", "win_len", "in_crc", "btype")
    for k, v in kw.items():
        pts[i][names.index(k)] = v
    return [tuple(p) for p in pts]


MUTATIONS = {
    "magic": dict(magic=b"LFXINDEx"),
    "version": dict(version=2),
    "format": dict(fmt=3),
    "flag_other": dict(flags=3),
    "multi_without_gzip": dict(fmt=1),
    "reserved": dict(reserved=1),
    "n_members": dict(n_members=3),
    "bad_crc": dict(crc_fix=False),
    "in_bit_not_increasing": dict(points=_with(1, in_bit=80, hdr_bit=80)),
    "out_off_decreasing": dict(points=_with(2, out_off=50000)),
    "hdr_after_in": dict(points=_with(1, hdr_bit=9001)),
    "btype_3": dict(points=_with(1, btype=3)),
    "stored_inside_block": dict(points=_with(1, btype=0)),
    "member_skips": dict(points=_with(3, member=2), n_members=3),
    "member_goes_back": dict(points=_with(4, member=0)),
    "member_start_inside_block": dict(points=_with(3, in_bit=400001)),
    "member_start_window": dict(points=_with(3, win_len=1)),
    "win_len_rule": dict(points=_with(4, win_len=9999)),
    "win_len_cap": dict(points=_with(2, win_len=32769)),
    "out_past_end": dict(points=_with(4, out_off=500000, win_len=32768), out_len=400000),
    "in_past_end": dict(points=_with(4, in_bit=800000), in_len=100000),
    "first_not_at_zero": dict(points=_with(0, out_off=1)),
}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_check_rejects(ffi, name):
    rc, _ = _check(ffi, _blob(**MUTATIONS[name]))
    assert rc == ffi.E_INVALID_DATA, name


def test_check_rejects_empty_and_padding(ffi):
    assert _check(ffi, _blob(points=[], n_members=0))[0] == ffi.E_INVALID_DATA
    pts = [_point(*p) for p in BASE]
    pts[1] = pts[1][:37] + b"\x01\0\0"
    body = b"LFXINDEX" + struct.pack("<IIIIQQQQII", 1, 2, 1, 5, 100000, 400000, 65536, 70000, 2, 0) + b"".join(pts) + \
        b"".join(bytes([i]) * p[4] for i, p in enumerate(BASE))
    assert _check(ffi, body + struct.pack("<I", zlib.crc32(body)))[0] == ffi.E_INVALID_DATA


def test_check_rejects_truncation_and_size(ffi):
    blob = _blob()
    n = 5
    bounds = [0, 8, 63, 64, 64 + 40, 64 + 40 * n, 64 + 40 * n + 1, len(blob) - 4, len(blob) - 1]
    for cut in bounds:
        assert _check(ffi, blob[:cut])[0] == ffi.E_INVALID_DATA, cut
    # a window byte too many, with a CRC that matches
    body = blob[:-4] + b"\0"
    assert _check(ffi, body + struct.pack("<I", zlib.crc32(body)))[0] == ffi.E_INVALID_DATA


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")
def test_index_kernels_have_no_serialized_loads():
    import isa_scan
    asm = isa_scan.compile_to_asm(os.path.join(ROOT, "libflate_amd", "csrc", "lfx_index.hip"))
    syms = [line for line in asm.split("\n") if line.startswith("_Z")]
    for k in KERNELS:
        assert any(k in s for s in syms), k
    bad = [f for f in isa_scan.serialized_load_loops(asm) if any(k in f[0] for k in KERNELS)]
    assert not bad, bad
