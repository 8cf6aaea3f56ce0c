"""CPU: the multi-member batch decode's ABI (lfx_decode_members_device / _host, lfx_member) — declared, exported, bound, no CPU
fallback — and its candidate finder's loops hold no one-load-one-wait pattern (tools/isa_scan.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NAMES = ("lfx_decode_members_device", "lfx_decode_members_host")
FINDER = ("member_cand_count_kernel", "member_cand_emit_kernel")


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
    assert "typedef struct lfx_member" in hdr


def test_member_layout(ffi):
    assert C.sizeof(ffi.Member) == 32
    for field, off in (("in_off", 0), ("in_len", 8), ("out_off", 16), ("out_len", 24)):
        assert getattr(ffi.Member, field).offset == off, field


def test_null_context_is_a_device_error(ffi):
    L = ffi.lib()
    out_len, used, count = C.c_uint64(7), C.c_uint64(7), C.c_uint32(7)
    table = (ffi.Member * 4)()
    data = b"\x1f\x8b\x08\x00" + b"\x00" * 16
    assert L.lfx_decode_members_device(None, None, 0, None, 0, C.byref(out_len), C.byref(used), table, 4, C.byref(count)) \
        == ffi.E_DEVICE
    buf = C.create_string_buffer(64)
    assert L.lfx_decode_members_host(None, data, len(data), buf, 64, C.byref(out_len), C.byref(used), table, 4, C.byref(count)) \
        == ffi.E_DEVICE
    # nothing was computed on the CPU: the outputs are untouched
    assert out_len.value == 7 and used.value == 7 and count.value == 7


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")
def test_candidate_finder_has_no_serialized_loads():
    import isa_scan
    asm = isa_scan.compile_to_asm(os.path.join(ROOT, "libflate_amd", "csrc", "lfx_members.hip"))
    syms = [line for line in asm.split("\n") if line.startswith("_Z")]
    for k in FINDER:
        assert any(k in s for s in syms), k
    bad = [f for f in isa_scan.serialized_load_loops(asm) if any(k in f[0] for k in FINDER)]
    assert not bad, bad
