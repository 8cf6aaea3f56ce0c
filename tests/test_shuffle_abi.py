"""CPU: lfx_shuffle_device / lfx_shuffle_batch_device / lfx_shuffle_host (include/lfx.h "the byte-shuffle filter", DESIGN.md
§30) — declared, exported, bound with the prototype's own argument list, declared by the Rust crate type by type, no CPU
fallback — and the Python surface over them: Context.shuffle_*, libflate_amd.filters, the shuffle= keyword.  (The range check
and the tile list run without a device in tests/test_shuffle_geom.py; the refusals that need a context in
tests/test_gpu_shuffle.py.)"""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from test_dict_train_abi import ffi, prototype  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = ["c", "dir", "elem_size", "IN", "n", "OUT"]
NAMES = {"lfx_shuffle_device": [a.replace("IN", "d_in").replace("OUT", "d_out") for a in ONE],
         "lfx_shuffle_host": [a.replace("IN", "in").replace("OUT", "out") for a in ONE],
         "lfx_shuffle_batch_device": ["c", "dir", "elem_size", "count", "d_in", "in_off", "len", "d_table", "d_out", "out_off"]}


def test_prototype_and_binding_agree(ffi):
    u64, u32, vp, i32 = C.c_uint64, C.c_uint32, C.c_void_p, C.c_int
    ok = {"int": (i32,), "uint32_t": (u32,), "uint64_t": (u64,), "constuint64_t*": (vp, C.POINTER(u64)), "void*": (vp,), "constvoid*": (vp,),
          "lfx_ctx*": (vp,)}
    for name, want in NAMES.items():
        args = prototype(name)
        assert [n for _, n in args] == want
        bound = getattr(ffi.lib(), name).argtypes
        assert len(bound) == len(args)
        for (typ, arg), b in zip(args, bound):
            assert typ in ok and b in ok[typ], (name, typ, arg, b)
    assert (ffi.SHUFFLE, ffi.UNSHUFFLE) == (0, 1)
    hdr = open(os.path.join(ROOT, "include", "lfx.h")).read()
    assert re.search(r"enum\s*\{\s*LFX_SHUFFLE\s*=\s*0\s*,\s*LFX_UNSHUFFLE\s*=\s*1\s*\}", hdr)


def test_declared_exported_bound(ffi):
    out = subprocess.run(["nm", "-D", "--defined-only", ffi.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines()}
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in exported and name in ffi.EXPORTS and hasattr(ffi.lib(), name) and name in integration


def test_rust_externs_match_the_header():
    """The crate cannot be compiled here (source only): its extern lines are held against the header's prototypes, type by type.
    They live in filters.rs — ffi.rs holds the externs tests/c/shim_abi.c drives."""
    rust = {"lfx_ctx*": "*mut lfx_ctx", "int": "c_int", "uint32_t": "u32", "uint64_t": "u64", "constvoid*": "*const c_void",
            "void*": "*mut c_void", "constuint64_t*": "*const u64"}
    rs = open(os.path.join(ROOT, "rust", "libflate-amd", "src", "filters.rs")).read()
    for name in NAMES:
        m = re.search(r"pub fn %s\s*\(([^()]*)\)\s*->\s*c_int\s*;" % name, rs)
        assert m, "filters.rs declares " + name
        types = [" ".join(a.split(":", 1)[1].split()) for a in m.group(1).split(",") if a.strip()]
        assert types == [rust[t] for t, _ in prototype(name)], name
        assert name not in open(os.path.join(ROOT, "rust", "libflate-amd", "src", "ffi.rs")).read()
    assert "pub mod filters;" in open(os.path.join(ROOT, "rust", "libflate-amd", "src", "lib.rs")).read()


def test_null_context_is_a_device_error(ffi):
    L = ffi.lib()
    one = lambda v: (C.c_uint64 * 1)(v)
    data = b"0123456789abcdef" * 4
    for direction in (0, 1, 2):
        for s in (0, 1, 4, 256, 257):
            # in the domain or out of it: without a context none of it is looked at, and nothing is computed on the CPU
            out = C.create_string_buffer(b"\xA5" * 64, 64)
            assert L.lfx_shuffle_host(None, direction, s, data, 64, out) == ffi.E_DEVICE and out.raw == b"\xA5" * 64
            assert L.lfx_shuffle_device(None, direction, s, None, 64, None) == ffi.E_DEVICE
            assert L.lfx_shuffle_batch_device(None, direction, s, 1, None, one(0), one(64), None, None, None) == ffi.E_DEVICE
    assert L.lfx_shuffle_batch_device(None, 0, 4, 0, None, None, None, None, None, None) == ffi.E_DEVICE


def test_python_surface(ffi):
    import libflate_amd as lfx
    assert "filters" in lfx.__all__
    for fn in (lfx.filters.shuffle, lfx.filters.unshuffle):
        p = inspect.signature(fn).parameters
        assert list(p) == ["data", "elem_size", "context"] and p["context"].default is None
    p = inspect.signature(lfx.Context.shuffle_host).parameters
    assert list(p) == ["self", "data", "elem_size", "inverse"] and p["inverse"].default is False
    assert list(inspect.signature(lfx.Context.shuffle_device).parameters) == ["self", "d_in", "n", "d_out", "elem_size", "inverse"]
    p = inspect.signature(lfx.Context.shuffle_batch_device).parameters
    assert list(p) == ["self", "d_in", "in_offs", "lens", "d_out", "elem_size", "inverse", "out_offs", "d_table"]
    for mod in (lfx.gzip, lfx.zlib, lfx.deflate):
        for name in ("compress", "compress_batch", "decompress", "decompress_batch"):
            p = inspect.signature(getattr(mod, name)).parameters
            assert list(p)[-1] == "shuffle" and p["shuffle"].default is None, (mod.__name__, name)
    assert inspect.signature(lfx.Context.encode_batch_packed_host).parameters["shuffle"].default is None
    assert list(inspect.signature(lfx.Context.decode_batch_unshuffle_host).parameters) == ["self", "fmt", "records", "elem_size", "zdict"]
