"""CPU: lfx_encode_index_device's ABI — declared, exported, bound, no CPU fallback — and its kernels' loops (tools/isa_scan.py)."""
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
KERNELS = ("idx_tile_bytes_kernel", "idx_chunk_scan_kernel", "idx_tile_points_kernel")


@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as g
    g.build()
    from libflate_amd import _ffi
    return _ffi


def test_declared_exported_bound(ffi):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfx.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+lfx_encode_index_device\s*\(", hdr)
    out = subprocess.run(["nm", "-D", "--defined-only", ffi.SO_PATH], capture_output=True, text=True, check=True).stdout
    assert "lfx_encode_index_device" in {l.split()[-1] for l in out.splitlines()}
    assert "lfx_encode_index_device" in ffi.EXPORTS
    assert len(ffi.lib().lfx_encode_index_device.argtypes) == 11


def test_null_context_is_a_device_error(ffi):
    L = ffi.lib()
    out_len, h = C.c_uint64(7), C.c_void_p(1234)
    opts = ffi.make_opts()
    assert L.lfx_encode_index_device(None, ffi.GZIP, C.byref(opts), None, None, 0, None, 0, C.byref(out_len), 1 << 20,
                                     C.byref(h)) == ffi.E_DEVICE
    assert out_len.value == 7 and h.value == 1234


def test_python_entry_points(ffi):
    from libflate_amd.context import Context
    from libflate_amd.index import Index
    assert callable(getattr(Context, "encode_index_device"))
    assert callable(getattr(Index, "encode"))


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")
def test_encode_index_kernels_have_no_serialized_loads():
    import isa_scan
    asm = isa_scan.compile_to_asm(os.path.join(ROOT, "libflate_amd", "csrc", "lfx_index_enc.hip"))
    syms = [line for line in asm.split("\n") if line.startswith("_Z")]
    for k in KERNELS:
        assert any(k in s for s in syms), k
    bad = [f for f in isa_scan.serialized_load_loops(asm) if any(k in f[0] for k in KERNELS)]
    assert not bad, bad
