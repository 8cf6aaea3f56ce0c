"""CPU: lfx_dict_train_device / lfx_dict_train_host — declared, exported, bound with the prototype's own argument
list, no CPU fallback — and the Python surface over them: Context.dict_train_device / _host, Dictionary.train,
libflate_amd.train_dictionary.  (The argument checks themselves run without a device in tests/test_dict_train_walk.py: they
are lfx_dict_train.h's, which tests/c/dict_train.cpp compiles.)"""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lfx_dict_train_device", "lfx_dict_train_host")


@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as g
    g.build()
    from libflate_amd import _ffi
    return _ffi


def prototype(name):
    """→ [(type, name)] of the prototype in include/lfx.h, comments removed"""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfx.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert m, "%s is not declared in include/lfx.h" % name
    args = []
    for a in m.group(1).split(","):
        a = " ".join(a.split())
        typ, arg = re.match(r"(.*?)(\w+)$", a).groups()
        args.append((typ.replace(" ", ""), arg))
    return args


def test_prototype_and_binding_agree(ffi):
    u64, u32, vp = C.c_uint64, C.c_uint32, C.c_void_p
    ok = {"uint32_t": (u32,), "uint64_t": (u64,), "uint64_t*": (vp, C.POINTER(u64)), "constuint64_t*": (vp, C.POINTER(u64)),
          "void*": (vp,), "constvoid*": (vp,), "lfx_ctx*": (vp,)}
    for name, samples, out in ((NAMES[0], "d_samples", "d_dict"), (NAMES[1], "samples", "dict")):
        args = prototype(name)
        assert [n for _, n in args] == ["c", samples, "count", "off", "len", "dict_size", "segment", out, "cap", "dict_len"]
        bound = getattr(ffi.lib(), name).argtypes
        assert len(bound) == len(args) == 10
        for (typ, arg), b in zip(args, bound):
            assert typ in ok and b in ok[typ], (name, typ, arg, b)


def test_declared_exported_bound(ffi):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lfx_[a-z0-9_]+)\s*\(", hdr))
    out = subprocess.run(["nm", "-D", "--defined-only", ffi.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines()}
    for name in NAMES:
        assert name in declared and name in exported and name in ffi.EXPORTS and hasattr(ffi.lib(), name)
        # the Rust crate leaves the calls unbound (INTEGRATION.md says so)
        for rs in ("ffi.rs", "dict.rs"):
            assert name not in open(os.path.join(ROOT, "rust", "libflate-amd", "src", rs)).read()
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_null_context_is_a_device_error(ffi):
    L = ffi.lib()
    one = lambda v: (C.c_uint64 * 1)(v)
    samples = b"0123456789abcdef" * 16
    for fn in (L.lfx_dict_train_device, L.lfx_dict_train_host):
        out = C.create_string_buffer(b"\xA5" * 64, 64)
        got = C.c_uint64(7)
        # in the domain, out of it, too small a capacity: without a context none of it is looked at
        for size, seg, cap in ((64, 16, 64), (63, 16, 64), (64, 15, 64), (64, 16, 8)):
            assert fn(None, samples, 1, one(0), one(len(samples)), size, seg, out, cap, C.byref(got)) == ffi.E_DEVICE
        # nothing was computed on the CPU: the outputs are untouched
        assert got.value == 7 and out.raw == b"\xA5" * 64


def test_python_surface(ffi):
    import libflate_amd
    sig = inspect.signature(libflate_amd.Dictionary.train)
    assert list(sig.parameters) == ["records", "size", "segment", "context", "chain"]
    assert [sig.parameters[p].default for p in ("size", "segment", "context", "chain")] == [32768, 128, None, False]
    sig = inspect.signature(libflate_amd.train_dictionary)
    assert list(sig.parameters)[:3] == ["records", "size", "segment"] and "train_dictionary" in libflate_amd.__all__
    sig = inspect.signature(libflate_amd.Context.dict_train_device)
    assert list(sig.parameters) == ["self", "d_samples", "offs", "lens", "size", "segment", "d_dict", "cap"]
    sig = inspect.signature(libflate_amd.Context.dict_train_host)
    assert list(sig.parameters)[:5] == ["self", "data", "offs", "lens", "size"]
