"""CPU: the host side of LazyLz77Encoder (LFX_LZ77_LAZY) — the constants in include/lfx.h and their Python and
Rust mirrors, the option check through lfx_encode_bound (host only: no device is touched), the Python encoder's options, and
tests/c/lazy_opts.cpp: the decoding of kind and depth with the kinds 0, 1 and 2 answering as before, the container headers, the
planner's buffering for kind 3 and the demote kernel's cut of its work items, built by the plain host compiler — once more as
a program of its own with AddressSanitizer and UBSan."""
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


def test_constants_in_the_header_and_their_mirrors(lfx):
    from libflate_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "lfx.h")).read()
    assert re.search(r"LFX_LZ77_DEFAULT = 0, LFX_LZ77_NOCOMPRESSION = 1, LFX_LZ77_CHAIN = 2, LFX_LZ77_LAZY = 3 \}", hdr)
    assert "#define LFX_LZ77_LAZY_DEPTH(k) (LFX_LZ77_LAZY | (k) << 8)" in hdr
    assert (_ffi.LZ77_DEFAULT, _ffi.LZ77_NOCOMPRESSION, _ffi.LZ77_CHAIN, _ffi.LZ77_LAZY) == (0, 1, 2, 3)
    rs = open(os.path.join(ROOT, "rust", "libflate-amd", "src", "ffi.rs")).read()
    assert re.search(r"pub const LFX_LZ77_LAZY: i32 = 3;", rs)
    lz = open(os.path.join(ROOT, "rust", "libflate-amd", "src", "lz77.rs")).read()
    assert "pub struct LazyLz77Encoder" in lz and "ffi::lfx_lz77_lazy_depth(c.depth)" in lz


def test_the_option_check_through_encode_bound(lfx):
    """lfx_encode_bound is 0 for options encode_spec refuses"""
    from libflate_amd import _ffi
    L = _ffi.lib()
    bound = lambda kind: L.lfx_encode_bound(1000, C.byref(_ffi.make_opts(lz77_kind=kind)), None)
    assert bound(0) and bound(1) and bound(0 | 0x1200) and bound(1 | 0x7F00)       # kinds 0, 1: the upper bits are not read
    for depth in (1, 2, 8, 255):
        assert bound(_ffi.LZ77_LAZY | depth << 8) == bound(0) == bound(_ffi.LZ77_CHAIN | depth << 8)
    assert bound(_ffi.LZ77_LAZY) == 0                                              # depth 0
    assert bound(_ffi.LZ77_LAZY | 256 << 8) == 0                                   # depth 256: bit 16
    for bit in range(16, 32):
        assert bound(_ffi.LZ77_LAZY | 8 << 8 | 1 << bit) == 0, bit
    # a schedule of 8 KiB writes: the planner cuts kind 3 as it cuts kind 0
    sched = _ffi.make_schedule(8192)
    for n in (0, 5, 300000, 1 << 20):
        b0 = L.lfx_encode_bound(n, C.byref(_ffi.make_opts(window_size=2048)), C.byref(sched))
        assert b0 and b0 == L.lfx_encode_bound(n, C.byref(_ffi.make_opts(window_size=2048, lz77_kind=_ffi.LZ77_LAZY | 8 << 8)), C.byref(sched))


def test_python_encoder_options(lfx):
    from libflate_amd import _ffi
    e = lfx.lz77.LazyLz77Encoder(8, window_size=1 << 20, max_length=1000)
    assert e._opts() == {"lz77_kind": 3 | 8 << 8, "window_size": 32768, "max_length": 258}
    assert e.compression_level() == lfx.lz77.CompressionLevel.BEST == 3 and e.window_size() == 32768
    assert not hasattr(e, "encode") and not hasattr(e, "flush")
    assert lfx.lz77.ChainLz77Encoder(8)._opts()["lz77_kind"] == 2 | 8 << 8          # as before
    o = lfx.gzip.EncodeOptions(lz77=lfx.lz77.LazyLz77Encoder(3, 1024, 16))._to_c()
    assert (o.lz77_kind, o.window_size, o.max_length, o.lz77_level) == (3 | 3 << 8, 1024, 16, 0)
    o = lfx.deflate.EncodeOptions().with_lz77(lfx.lz77.LazyLz77Encoder(32))._to_c()
    assert o.lz77_kind == 3 | 32 << 8
    L = _ffi.lib()
    for depth in (0, 256, -1):      # reaches encode_spec unchanged: refused, not a silently different depth
        assert L.lfx_encode_bound(10, C.byref(lfx.zlib.EncodeOptions(lz77=lfx.lz77.LazyLz77Encoder(depth))._to_c()), None) == 0
    for fmt in (0, 1, 2):
        assert L.lfx_container_header_len(fmt, C.byref(_ffi.make_opts(lz77_kind=3 | 8 << 8))) == L.lfx_container_header_len(fmt, None)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_host_arithmetic_under_the_host_compiler(tmp_path, sanitize):
    """a program of its own (nothing loaded into Python runs under a sanitizer)"""
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "lazy_opts")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run([gxx, "-std=c++17", "-Wall"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "c", "lazy_opts.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and re.search(r"lazy_opts ok: 2000 plans, \d+ spans", out.stdout), (out.stdout[-400:], out.stderr[-400:])
