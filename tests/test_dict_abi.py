"""CPU: the preset-dictionary calls (include/lfx.h) — every fixture of test_gpu_dict_decode.py is proved with
python-zlib before a GPU sees it; the symbols are declared, exported and bound; without a device nothing runs."""
import ctypes as C
import os
import re
import subprocess
import zlib

import pytest

import dict_craft as dk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lfx_dict_new", "lfx_dict_id", "lfx_dict_free", "lfx_decode_dict_device", "lfx_decode_dict_host",
         "lfx_decode_batch_dict_device", "lfx_decoder_set_dict")


@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as g
    g.build()
    from libflate_amd import _ffi
    return _ffi


def test_fixtures_decode_with_python_zlib():
    seen = 0
    for c in dk.cases():
        if c.err is None:
            assert dk.py_inflate(c.fmt, c.stream, c.zdict) == c.want, c.name
            if c.fmt == "zlib" and len(c.zdict):
                assert c.stream[1] & 0x20 and int.from_bytes(c.stream[2:6], "big") == zlib.adler32(c.zdict), c.name
        else:
            with pytest.raises(zlib.error):
                dk.py_inflate(c.fmt, c.stream, c.zdict)
        seen += 1
    assert seen == len(dk.cases()) >= 20
    # the shapes the GPU tests rely on
    assert len(dk.by_name("sync_flush_reach").stream) < 4096 and len(dk.by_name("large_zlib").stream) > 300000
    assert all(len(c.stream) < 4096 for c in dk.cases() if c.name.startswith(("rec", "craft_")))
    assert len(dk.by_name("blk64k_raw").stream) >= 4096
    # a dictionary is what makes these streams decodable: without it python-zlib refuses them too
    with pytest.raises(zlib.error):
        dk.py_inflate("raw", dk.by_name("craft_dist_32768").stream, b"")
    for z, rec in dk.batch_records(8):
        assert dk.py_inflate("zlib", z, dk.D32) == rec and 100 <= len(rec) <= 2000
    # the 40000-byte dictionary: only the tail is reachable, so the tail alone decodes the raw stream
    c = dk.by_name("rec1100_raw_d40")
    assert dk.py_inflate("raw", c.stream, dk.D40[-32768:]) == c.want


def test_declared_exported_bound(ffi):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lfx_[a-z0-9_]+)\s*\(", hdr))
    out = subprocess.run(["nm", "-D", "--defined-only", ffi.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines()}
    for name in NAMES:
        assert name in declared and name in exported and name in ffi.EXPORTS, name
        assert hasattr(ffi.lib(), name) and getattr(ffi.lib(), name).argtypes is not None, name
    assert ffi.DEC_LAZY_HEADER == 4 and re.search(r"#define LFX_DEC_LAZY_HEADER 4u", hdr)


def test_null_context_runs_nothing(ffi):
    L = ffi.lib()
    st = C.c_int(-1)
    assert L.lfx_dict_new(None, b"abc", 3, 0, C.byref(st)) is None and st.value == ffi.E_DEVICE
    assert L.lfx_dict_id(None) == 1
    L.lfx_dict_free(None)
    z = dk.by_name("rec100_zlib_d32").stream
    out = C.create_string_buffer(b"\x5a" * 256, 256)
    ol, used = C.c_uint64(77), C.c_uint64(77)
    for fn in (L.lfx_decode_dict_device, L.lfx_decode_dict_host):
        assert fn(None, ffi.ZLIB, None, z, len(z), out, 256, C.byref(ol), C.byref(used)) == ffi.E_DEVICE
    one = (C.c_uint64 * 1)
    lens, stat = one(77), (C.c_int32 * 1)(77)
    assert L.lfx_decode_batch_dict_device(None, ffi.ZLIB, None, 1, z, one(0), one(len(z)), out, one(0), one(256), lens,
                                          stat) == ffi.E_DEVICE
    assert out.raw == b"\x5a" * 256 and (ol.value, used.value, lens[0], stat[0]) == (77, 77, 77, 77)
    assert L.lfx_decoder_set_dict(None, None) == ffi.E_ARG


def test_stream_decoder_policy_with_a_dictionary(tmp_path):
    """The stream decoder's state machine (lfx_stream_dec.h: no HIP, a plain host compiler) with a preset dictionary over a
    window backend made of zlib's raw inflate (tests/c/stream_dec_dict.cpp): the header's FDICT verdicts, the first window's
    history, the reach bound handed to the backend, the trailer over the output only, when set_dict is still allowed, the lazy
    header of a blocking decoder, the non-blocking mode."""
    import shutil
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "stream_dec_dict")
    subprocess.run([gxx, "-O2", "-std=c++17", "-Wall", "-pthread", "-o", exe, os.path.join(ROOT, "tests", "c", "stream_dec_dict.cpp"), "-lz"],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "stream_dec_dict ok:" in out.stdout, out.stdout[-600:] + out.stderr[-400:]
