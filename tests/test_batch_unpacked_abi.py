"""CPU: lfx_decode_batch_packed_device — declared, exported, bound with the prototype's own argument list, no
CPU fallback — and the Python surface over it: Context.decode_batch_packed_device / _host, decompress and decompress_batch in
the three format modules."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "lfx_decode_batch_packed_device"


@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as g
    g.build()
    from libflate_amd import _ffi
    return _ffi


def prototype():
    """→ [(type, name)] of the prototype in include/lfx.h, comments removed"""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfx.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NAME, hdr)
    assert m, "%s is not declared in include/lfx.h" % NAME
    args = []
    for a in m.group(1).split(","):
        a = " ".join(a.split())
        typ, name = re.match(r"(.*?)(\w+)$", a).groups()
        args.append((typ.replace(" ", ""), name))
    return args


def test_prototype_and_binding_agree(ffi):
    args = prototype()
    assert [n for _, n in args] == ["c", "format", "dict", "count", "d_in", "in_off", "in_len", "d_in_table", "align", "d_out", "cap",
                                    "out_off", "out_len", "consumed", "status", "total", "d_table"]
    u64, u32, vp, i32 = C.c_uint64, C.c_uint32, C.c_void_p, C.c_int
    # a pointer argument is bound as void* (arrays, raw addresses and None all pass) or as a typed pointer to the same type
    ok = {"int": (i32,), "uint32_t": (u32,), "uint64_t": (u64,), "uint64_t*": (vp, C.POINTER(u64)), "constuint64_t*": (vp, C.POINTER(u64)),
          "int32_t*": (vp, C.POINTER(C.c_int32)), "void*": (vp,), "constvoid*": (vp,), "lfx_ctx*": (vp,), "constlfx_dict*": (vp,)}
    bound = ffi.lib().lfx_decode_batch_packed_device.argtypes
    assert len(bound) == len(args) == 17
    for (typ, name), b in zip(args, bound):
        assert typ in ok and b in ok[typ], (typ, name, b)


def test_declared_exported_bound(ffi):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lfx_[a-z0-9_]+)\s*\(", hdr))
    out = subprocess.run(["nm", "-D", "--defined-only", ffi.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines()}
    assert NAME in declared and NAME in exported and NAME in ffi.EXPORTS and hasattr(ffi.lib(), NAME)
    # the Rust crate leaves it unbound (INTEGRATION.md says so)
    assert NAME not in open(os.path.join(ROOT, "rust", "libflate-amd", "src", "ffi.rs")).read()
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_null_context_is_a_device_error(ffi):
    L = ffi.lib()
    one = lambda v: (C.c_uint64 * 1)(v)
    off, ln, used, st, total = one(7), one(7), one(7), (C.c_int32 * 1)(7), C.c_uint64(7)
    out = C.create_string_buffer(b"\xA5" * 64, 64)
    for fmt in (ffi.DEFLATE, ffi.ZLIB, ffi.GZIP):
        assert L.lfx_decode_batch_packed_device(None, fmt, None, 1, b"\x03\x00", one(0), one(2), None, 1, out, 64, off, ln, used, st,
                                                C.byref(total), None) == ffi.E_DEVICE
    # nothing was computed on the CPU: the outputs are untouched
    assert off[0] == 7 and ln[0] == 7 and used[0] == 7 and st[0] == 7 and total.value == 7 and out.raw == b"\xA5" * 64


def test_python_surface(ffi):
    import libflate_amd
    from libflate_amd import deflate, gzip, zlib
    sig = inspect.signature(libflate_amd.Context.decode_batch_packed_device)
    assert list(sig.parameters)[:7] == ["self", "fmt", "d_in", "in_offs", "in_lens", "d_out", "cap"]
    for kw, default in (("zdict", None), ("align", 1), ("d_in_table", None), ("d_table", None)):
        assert sig.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[kw].default == default
    sig = inspect.signature(libflate_amd.Context.decode_batch_packed_host)
    assert list(sig.parameters) == ["self", "fmt", "records", "zdict"] and sig.parameters["zdict"].default is None
    for mod, has_dict in ((gzip, False), (zlib, True), (deflate, True)):
        one, many = inspect.signature(mod.decompress).parameters, inspect.signature(mod.decompress_batch).parameters
        assert list(one)[0] == "data" and list(many)[0] == "records" and "context" in many, mod.__name__
        assert ("zdict" in one) == ("zdict" in many) == has_dict, mod.__name__
        if has_dict:
            assert list(one)[1] == list(many)[1] == "zdict" and one["zdict"].default is None and many["zdict"].default is None
        assert many["context"].default is None
