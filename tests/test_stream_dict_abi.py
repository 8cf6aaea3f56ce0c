"""CPU: the stream encoder with a preset dictionary (include/lfx.h "the stream encoder with a preset dictionary") —
the header, the ctypes binding, the library and the Rust crate declare, bind and export lfx_encoder_new_dict with the stated
signature: lfx_encoder_new's arguments with the dictionary behind the options.  gzip is LFX_E_ARG and a NULL context
LFX_E_DEVICE; without a device nothing else runs."""
import ctypes as C
import inspect
import os
import re
import subprocess

from test_dict_encode_abi import _declared, ffi  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the signature the contract states, as C types without their names
SIGNATURE = ("lfx_encoder *", ["lfx_ctx *", "int", "const lfx_encode_opts *", "const lfx_dict *", "lfx_write_cb", "lfx_flush_cb", "void *", "int *"])
# the same in the crate's spelling (rust/libflate-amd/src/ffi.rs declares lfx_encoder_new this way)
RUST = {"lfx_encoder *": "*mut lfx_encoder", "lfx_ctx *": "*mut lfx_ctx", "int": "c_int", "const lfx_encode_opts *": "*const lfx_encode_opts",
        "const lfx_dict *": "*const lfx_dict", "lfx_write_cb": "lfx_write_cb", "lfx_flush_cb": "Option<lfx_flush_cb>", "void *": "*mut c_void",
        "int *": "*mut c_int"}


def _c_prototype(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfx.h")).read(), flags=re.S)
    m = re.search(r"([A-Za-z_][A-Za-z0-9_ ]*?\*?)\s*\b%s\s*\(([^()]*)\)\s*;" % name, hdr)
    assert m, name + " is not declared in include/lfx.h"

    def ctype(arg):          # "const lfx_dict *dict" → "const lfx_dict *"
        arg = " ".join(arg.split())
        t = re.sub(r"[A-Za-z_][A-Za-z0-9_]*$", "", arg).strip()
        return re.sub(r"\s*\*", " *", t)
    return re.sub(r"\s*\*", " *", " ".join(m.group(1).split())), [ctype(a) for a in m.group(2).split(",")]


def test_declared_with_the_stated_signature():
    assert _c_prototype("lfx_encoder_new_dict") == SIGNATURE
    ret, args = _c_prototype("lfx_encoder_new")
    assert ret == SIGNATURE[0] and args == SIGNATURE[1][:3] + SIGNATURE[1][4:]      # lfx_encoder_new itself did not change


def test_exported_and_bound(ffi):
    declared = _declared()
    assert declared.get("lfx_encoder_new_dict") == 8 and declared["lfx_encoder_new"] == 7
    out = subprocess.run(["nm", "-D", "--defined-only", ffi.SO_PATH], capture_output=True, text=True, check=True).stdout
    assert "lfx_encoder_new_dict" in {l.split()[-1] for l in out.splitlines()} and "lfx_encoder_new_dict" in ffi.EXPORTS
    L = ffi.lib()
    twin = L.lfx_encoder_new.argtypes
    assert L.lfx_encoder_new_dict.argtypes == twin[:3] + [C.c_void_p] + twin[3:] and L.lfx_encoder_new_dict.restype is L.lfx_encoder_new.restype


def test_gzip_and_null_context(ffi):
    L = ffi.lib()
    calls = []
    w = ffi.WRITE_CB(lambda user, p, n: calls.append(n) or n)
    f = ffi.FLUSH_CB(lambda user: calls.append("flush") or 0)
    opts = ffi.make_opts()
    for o in (None, C.byref(opts)):
        st = C.c_int(77)
        assert L.lfx_encoder_new_dict(None, ffi.GZIP, o, None, w, f, None, C.byref(st)) is None and st.value == ffi.E_ARG
        for fmt in (ffi.ZLIB, ffi.DEFLATE):
            st = C.c_int(77)
            assert L.lfx_encoder_new_dict(None, fmt, o, None, w, f, None, C.byref(st)) is None and st.value == ffi.E_DEVICE
            st2 = C.c_int(77)
            assert L.lfx_encoder_new(None, fmt, o, w, f, None, C.byref(st2)) is None and st2.value == st.value
    assert L.lfx_encoder_new_dict(None, ffi.ZLIB, None, None, w, f, None, None) is None      # (status may be NULL)
    assert calls == []                                                                     # nothing reached the sink


def test_rust_extern_line_matches_the_header():
    """The crate cannot be compiled here (source only): its extern line is held against the header's prototype, type by type.
    It lives in dict.rs, next to the other dictionary calls — ffi.rs holds the externs tests/c/shim_abi.c drives."""
    rs = open(os.path.join(ROOT, "rust", "libflate-amd", "src", "dict.rs")).read()
    m = re.search(r"pub fn lfx_encoder_new_dict\s*\(([^()]*)\)\s*->\s*([^;]+);", rs)
    assert m, "dict.rs declares lfx_encoder_new_dict"
    types = [" ".join(a.split(":", 1)[1].split()) for a in m.group(1).split(",")]
    ret, args = SIGNATURE
    assert types == [RUST[a] for a in args] and " ".join(m.group(2).split()) == RUST[ret]
    # ... and it spells the twin as ffi.rs does
    ffi_rs = open(os.path.join(ROOT, "rust", "libflate-amd", "src", "ffi.rs")).read()
    t = re.search(r"pub fn lfx_encoder_new\s*\(([^()]*)\)\s*->\s*([^;]+);", ffi_rs)
    twin = [" ".join(a.split(":", 1)[1].split()) for a in t.group(1).split(",")]
    assert twin == types[:3] + types[4:]
    lib_rs = open(os.path.join(ROOT, "rust", "libflate-amd", "src", "lib.rs")).read()
    assert "pub mod dict;" in lib_rs and "dict::lfx_encoder_new_dict(" in lib_rs
    for mod in ("zlib.rs", "deflate.rs"):
        src = open(os.path.join(ROOT, "rust", "libflate-amd", "src", mod)).read()
        assert "pub fn with_dictionary(" in src and "RawEncoder::new_dict(" in src, mod


def test_python_spelling():
    import libflate_amd as lfx
    for mod in (lfx.zlib, lfx.deflate):
        p = inspect.signature(mod.Encoder.new).parameters
        assert list(p) == ["inner", "context", "options", "zdict"] and p["zdict"].default is None and p["options"].default is None
        assert "zdict" in inspect.signature(mod.Encoder.with_options).parameters
    for name in ("new", "with_options"):
        assert "zdict" not in inspect.signature(getattr(lfx.gzip.Encoder, name)).parameters       # gzip has no preset dictionary
