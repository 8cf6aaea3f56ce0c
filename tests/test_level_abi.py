"""CPU: the host side of LevelLz77Encoder (LFX_LZ77_LEVEL) — the constant in include/lfx.h and its Python and
Rust mirrors, the option check through lfx_encode_bound (host only: no device is touched), the container header's level, the
Python encoder's options and the level= shorthand, and tests/c/level_opts.cpp: the level table field by field, LFX_E_ARG for
the levels 0 and 10 and a bit above 15, the plan of kind 4 against the plan of kind 3, every encode_served cell of kind 4 and
the demote rule with max_lazy — built by the plain host compiler, once more as a program of its own with AddressSanitizer and
UBSan."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lfx():
    import __graft_entry__ as g
    g.build()
    import libflate_amd
    return libflate_amd


def test_constant_in_the_header_and_its_mirrors(lfx):
    from libflate_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "lfx.h")).read()
    assert re.search(r"enum \{ LFX_LZ77_LEVEL = 4 \};", hdr)
    assert "#define LFX_LZ77_LEVEL_N(n) (LFX_LZ77_LEVEL | (n) << 8)" in hdr
    assert _ffi.LZ77_LEVEL == 4 and (_ffi.LZ77_DEFAULT, _ffi.LZ77_NOCOMPRESSION, _ffi.LZ77_CHAIN, _ffi.LZ77_LAZY) == (0, 1, 2, 3)
    rs = open(os.path.join(ROOT, "rust", "libflate-amd", "src", "ffi.rs")).read()
    assert re.search(r"pub const LFX_LZ77_LEVEL: i32 = 4;", rs) and "pub const fn lfx_lz77_level_n(level: u8) -> i32" in rs
    lz = open(os.path.join(ROOT, "rust", "libflate-amd", "src", "lz77.rs")).read()
    assert "pub struct LevelLz77Encoder" in lz and "ffi::lfx_lz77_level_n(" in lz
    # the header's table, row by row, against the model's
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import level_model as vm
    rows = re.findall(r"^ \*\s+([1-9])\s+(greedy|lazy)\s+(\d+)\s+(\d+)\s+(\d+|-)\s+(\d+|-)\s*$", hdr, re.M)
    assert len(rows) == 9
    for lvl, walk, k, n, z, f in rows:
        depth, lazy, nice, max_lazy, too_far = vm.TABLE[int(lvl)]
        assert (int(k), walk == "lazy", int(n)) == (depth, lazy, nice)
        assert (z, f) == ((str(max_lazy), str(too_far)) if lazy else ("-", "-"))


def test_the_option_check_through_encode_bound(lfx):
    """lfx_encode_bound is 0 for options encode_spec refuses"""
    from libflate_amd import _ffi
    L = _ffi.lib()
    bound = lambda kind: L.lfx_encode_bound(1000, C.byref(_ffi.make_opts(lz77_kind=kind)), None)
    for n in range(1, 10):
        assert bound(_ffi.LZ77_LEVEL | n << 8) == bound(0) != 0
    assert bound(_ffi.LZ77_LEVEL) == 0                                             # level 0
    for n in (10, 11, 128, 255):
        assert bound(_ffi.LZ77_LEVEL | n << 8) == 0
    for bit in range(16, 32):
        assert bound(_ffi.LZ77_LEVEL | 6 << 8 | 1 << bit) == 0, bit
    assert bound(0 | 0x1200) and bound(1 | 0x7F00) and bound(_ffi.LZ77_LAZY | 255 << 8) and bound(_ffi.LZ77_CHAIN | 1 << 8)   # as before
    sched = _ffi.make_schedule(8192)
    for n in (0, 5, 300000, 1 << 20):
        b3 = L.lfx_encode_bound(n, C.byref(_ffi.make_opts(window_size=2048, lz77_kind=_ffi.LZ77_LAZY | 8 << 8)), C.byref(sched))
        assert b3 and b3 == L.lfx_encode_bound(n, C.byref(_ffi.make_opts(window_size=2048, lz77_kind=_ffi.LZ77_LEVEL | 6 << 8)), C.byref(sched))


def test_python_encoder_options_and_the_shorthand(lfx):
    from libflate_amd import _ffi
    lz = lfx.lz77
    e = lz.LevelLz77Encoder(6, window_size=1 << 20, max_length=1000)
    assert e._opts() == {"lz77_kind": 4 | 6 << 8, "window_size": 32768, "max_length": 258}
    assert e.window_size() == 32768 and not hasattr(e, "encode") and not hasattr(e, "flush")
    assert [lz.LevelLz77Encoder(n).compression_level() for n in range(1, 10)] == [1, 1, 1, 2, 2, 2, 3, 3, 3]
    o = lfx.gzip.EncodeOptions(lz77=lz.LevelLz77Encoder(3, 1024, 16))._to_c()
    assert (o.lz77_kind, o.window_size, o.max_length, o.lz77_level) == (4 | 3 << 8, 1024, 16, 0)
    assert lfx.deflate.EncodeOptions().with_lz77(lz.LevelLz77Encoder(9))._to_c().lz77_kind == 4 | 9 << 8
    assert lz.LazyLz77Encoder(8)._opts()["lz77_kind"] == 3 | 8 << 8 and lz.ChainLz77Encoder(8)._opts()["lz77_kind"] == 2 | 8 << 8   # as before
    L = _ffi.lib()
    for level in (0, 10, 256, -1):       # reaches encode_spec as a level it refuses, not as a silently different one
        assert L.lfx_encode_bound(10, C.byref(lfx.zlib.EncodeOptions(lz77=lz.LevelLz77Encoder(level))._to_c()), None) == 0
    for fmt in (0, 1, 2):
        assert L.lfx_container_header_len(fmt, C.byref(_ffi.make_opts(lz77_kind=4 | 6 << 8))) == L.lfx_container_header_len(fmt, None)
    # level= is lz77=LevelLz77Encoder(level), and excludes lz77=
    from libflate_amd.deflate import _with_lz77
    assert _with_lz77(None, None, lfx.zlib.EncodeOptions, 6)._to_c().lz77_kind == 4 | 6 << 8
    assert _with_lz77(lfx.gzip.EncodeOptions().block_size(4096), None, lfx.gzip.EncodeOptions, 1)._to_c().block_size == 4096
    assert _with_lz77(None, None, lfx.zlib.EncodeOptions) is None
    with pytest.raises(ValueError):
        _with_lz77(None, lz.LazyLz77Encoder(8), lfx.zlib.EncodeOptions, 6)
    import inspect
    for mod in (lfx.gzip, lfx.zlib, lfx.deflate):
        assert "level" in inspect.signature(mod.compress).parameters


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_host_arithmetic_under_the_host_compiler(tmp_path, sanitize):
    """a program of its own (nothing loaded into Python runs under a sanitizer)"""
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "level_opts")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run([gxx, "-std=c++17", "-Wall"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "c", "level_opts.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and re.search(r"level_opts ok: 2000 plans, 810 cells, \d+ pairs", out.stdout), (out.stdout[-400:], out.stderr[-400:])
