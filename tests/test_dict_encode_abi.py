"""CPU: the dictionary encode calls (include/lfx.h "encoding with a preset dictionary") — the header, the ctypes
binding and the library declare, bind and export the same four symbols with the same arities; without a device nothing runs."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"lfx_encode_dict_bound": 3, "lfx_encode_dict_device": 10, "lfx_encode_dict_host": 10, "lfx_encode_batch_dict_device": 14}
TWIN = {"lfx_encode_dict_bound": "lfx_encode_bound", "lfx_encode_dict_device": "lfx_encode_device",
        "lfx_encode_dict_host": "lfx_encode_host", "lfx_encode_batch_dict_device": "lfx_encode_batch_device"}


@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as g
    g.build()
    from libflate_amd import _ffi
    return _ffi


def _declared():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfx.h")).read(), flags=re.S)
    return {m.group(1): len([a for a in m.group(2).split(",") if a.strip() and a.strip() != "void"])
            for m in re.finditer(r"\b(lfx_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr)}


def test_declared_exported_bound(ffi):
    declared = _declared()
    out = subprocess.run(["nm", "-D", "--defined-only", ffi.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines()}
    for name, arity in ARITY.items():
        assert declared.get(name) == arity, (name, declared.get(name))
        assert name in exported and name in ffi.EXPORTS, name
        fn = getattr(ffi.lib(), name)
        assert fn.argtypes is not None and len(fn.argtypes) == arity, name
        # the arguments of the dictionary-less twin plus the dictionary
        twin = TWIN[name]
        assert declared[twin] == arity - (0 if name == "lfx_encode_dict_bound" else 1), twin
    assert ffi.lib().lfx_encode_dict_bound.restype is C.c_uint64


def test_bound_and_null_context(ffi):
    L = ffi.lib()
    opts = ffi.make_opts()
    for n in (0, 1, 1000, 1 << 20):
        assert L.lfx_encode_dict_bound(n, C.byref(opts), None) == L.lfx_encode_bound(n, C.byref(opts), None) + 4
    bad = ffi.make_opts(max_length=2)
    assert L.lfx_encode_bound(10, C.byref(bad), None) == 0 and L.lfx_encode_dict_bound(10, C.byref(bad), None) == 0
    out = C.create_string_buffer(b"\x5a" * 256, 256)
    ol = C.c_uint64(77)
    for fn in (L.lfx_encode_dict_device, L.lfx_encode_dict_host):
        assert fn(None, ffi.ZLIB, None, None, None, b"abc", 3, out, 256, C.byref(ol)) == ffi.E_DEVICE
    one = (C.c_uint64 * 1)
    lens, stat = one(77), (C.c_int32 * 1)(77)
    assert L.lfx_encode_batch_dict_device(None, ffi.ZLIB, None, None, None, 1, b"abc", one(0), one(3), out, one(0), one(256), lens,
                                          stat) == ffi.E_DEVICE
    assert out.raw == b"\x5a" * 256 and (ol.value, lens[0], stat[0]) == (77, 77, 77)
