"""CPU: the ABI of the size calls (lfx_decode_size_device / _host, lfx_decode_batch_size_device, lfx_decode_members_size_device /
_host) — declared, exported, bound, no CPU fallback — and the Python helpers built on them."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lfx_decode_size_device", "lfx_decode_size_host", "lfx_decode_batch_size_device", "lfx_decode_members_size_device",
         "lfx_decode_members_size_host")
GZ = b"\x1f\x8b\x08\x00" + b"\x00" * 16


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
    assert ffi.lib().lfx_version() == 0x000100


def test_walker_kernel_is_in_the_library(ffi):
    out = subprocess.run(["strings", "-a", ffi.SO_PATH], capture_output=True, text=True, check=True).stdout
    assert "blk_walk_size_kernel" in out


def test_null_context_is_a_device_error_and_writes_nothing(ffi):
    L = ffi.lib()
    out_len, used, count = C.c_uint64(7), C.c_uint64(7), C.c_uint32(7)
    for fmt in (ffi.DEFLATE, ffi.ZLIB, ffi.GZIP):
        assert L.lfx_decode_size_device(None, fmt, 0, None, 0, C.byref(out_len), C.byref(used)) == ffi.E_DEVICE
        assert L.lfx_decode_size_host(None, fmt, ffi.DEC_MULTI, GZ, len(GZ), C.byref(out_len), C.byref(used)) == ffi.E_DEVICE
    off, ln = (C.c_uint64 * 2)(0, 10), (C.c_uint64 * 2)(10, 10)
    ol, cons, st = (C.c_uint64 * 2)(7, 7), (C.c_uint64 * 2)(7, 7), (C.c_int32 * 2)(7, 7)
    assert L.lfx_decode_batch_size_device(None, ffi.GZIP, 2, None, off, ln, ol, cons, st) == ffi.E_DEVICE
    table = (ffi.Member * 4)()
    for m in table:
        m.in_off = m.in_len = m.out_off = m.out_len = 7
    assert L.lfx_decode_members_size_device(None, None, 0, C.byref(out_len), C.byref(used), table, 4, C.byref(count)) == ffi.E_DEVICE
    assert L.lfx_decode_members_size_host(None, GZ, len(GZ), C.byref(out_len), C.byref(used), table, 4, C.byref(count)) == ffi.E_DEVICE
    assert out_len.value == 7 and used.value == 7 and count.value == 7
    assert list(ol) == [7, 7] and list(cons) == [7, 7] and list(st) == [7, 7]
    assert all((m.in_off, m.in_len, m.out_off, m.out_len) == (7, 7, 7, 7) for m in table)


def test_python_helpers_need_a_device(ffi):
    import libflate_amd
    import torch
    if torch.cuda.is_available():      # (with a device the helpers are exercised by tests/test_gpu_decode_size.py)
        with pytest.raises(libflate_amd.StreamError):
            libflate_amd.decoded_size(GZ)
        return
    with pytest.raises(ffi.DeviceError):
        libflate_amd.decoded_size(GZ)
    with pytest.raises(ffi.DeviceError):
        libflate_amd.gzip.list_members(GZ)


def test_context_has_the_wrappers(ffi):
    import libflate_amd
    for name in ("decode_size_device", "decode_size_host", "decode_batch_size_device", "decode_members_size_device",
                 "decode_members_size_host"):
        assert callable(getattr(libflate_amd.Context, name)), name
    assert callable(libflate_amd.decoded_size) and callable(libflate_amd.gzip.list_members)
