"""CPU: the chain dictionary (include/lfx.h "a chain dictionary") — the header, the ctypes binding and the
library declare, bind and export lfx_dict_new_chain with lfx_dict_new's arguments; the Python spelling; and the host arithmetic
of the chain kernel's dictionary instance (tests/c/dict_chain_items.cpp) under the host compiler, plain and with
AddressSanitizer and UBSan, as a program of its own.  Without a device nothing runs."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import pytest

from test_dict_encode_abi import _declared, ffi  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_exported_bound(ffi):
    declared = _declared()
    out = subprocess.run(["nm", "-D", "--defined-only", ffi.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines()}
    assert declared.get("lfx_dict_new_chain") == declared["lfx_dict_new"] == 5
    assert "lfx_dict_new_chain" in exported and "lfx_dict_new_chain" in ffi.EXPORTS
    L = ffi.lib()
    assert L.lfx_dict_new_chain.argtypes == L.lfx_dict_new.argtypes and L.lfx_dict_new_chain.restype is L.lfx_dict_new.restype
    st = C.c_int(77)
    assert L.lfx_dict_new_chain(None, b"abc", 3, 0, C.byref(st)) is None and st.value == ffi.E_DEVICE


def test_python_spelling():
    import libflate_amd as lfx
    p = inspect.signature(lfx.Dictionary.__init__).parameters
    assert list(p)[1:] == ["data", "context", "chain"] and p["chain"].default is False


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_host_arithmetic_under_the_host_compiler(tmp_path, flags):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "dict_chain_items")
    subprocess.run([gxx, "-O2", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "c", "dict_chain_items.cpp")],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "dict_chain_items ok:" in out.stdout and "2000 lists" in out.stdout, (out.stdout[-400:], out.stderr[-400:])
