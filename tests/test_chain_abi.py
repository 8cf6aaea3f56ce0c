"""CPU: the host side of ChainLz77Encoder (LFX_LZ77_CHAIN) — the constants in include/lfx.h and their Python
mirror, the option check through lfx_encode_bound (host only: no device is touched), the Python encoder's options, and
tests/c/chain_opts.cpp: the decoding of kind and depth, the container headers, the planner's buffering for kind 2 and the chain
kernel's work list, built by the plain host compiler."""
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


def test_constants_in_the_header_and_their_mirror(lfx):
    from libflate_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "lfx.h")).read()
    assert re.search(r"LFX_LZ77_DEFAULT = 0, LFX_LZ77_NOCOMPRESSION = 1, LFX_LZ77_CHAIN = 2", hdr)
    assert "#define LFX_LZ77_CHAIN_DEPTH(k) (LFX_LZ77_CHAIN | (k) << 8)" in hdr
    assert (_ffi.LZ77_DEFAULT, _ffi.LZ77_NOCOMPRESSION, _ffi.LZ77_CHAIN) == (0, 1, 2)
    rs = open(os.path.join(ROOT, "rust", "libflate-amd", "src", "ffi.rs")).read()
    assert re.search(r"pub const LFX_LZ77_CHAIN: i32 = 2;", rs)


def test_the_option_check_through_encode_bound(lfx):
    """lfx_encode_bound is 0 for options encode_spec refuses"""
    from libflate_amd import _ffi
    L = _ffi.lib()
    bound = lambda kind: L.lfx_encode_bound(1000, C.byref(_ffi.make_opts(lz77_kind=kind)), None)
    assert bound(0) and bound(1) and bound(0 | 0x1200) and bound(1 | 0x7F00)       # kinds 0, 1: the upper bits are not read
    for depth in (1, 2, 8, 255):
        assert bound(_ffi.LZ77_CHAIN | depth << 8) == bound(0)
    assert bound(_ffi.LZ77_CHAIN) == 0                                             # depth 0
    assert bound(_ffi.LZ77_CHAIN | 256 << 8) == 0                                  # depth 256: bit 16
    assert bound(_ffi.LZ77_CHAIN | 8 << 8 | 1 << 30) == 0


def test_python_encoder_options(lfx):
    from libflate_amd import _ffi
    e = lfx.lz77.ChainLz77Encoder(8, window_size=1 << 20, max_length=1000)
    assert e._opts() == {"lz77_kind": 2 | 8 << 8, "window_size": 32768, "max_length": 258}
    assert e.compression_level() == lfx.lz77.CompressionLevel.BEST == 3 and e.window_size() == 32768
    assert not hasattr(e, "encode") and not hasattr(e, "flush")
    o = lfx.gzip.EncodeOptions(lz77=lfx.lz77.ChainLz77Encoder(3, 1024, 16))._to_c()
    assert (o.lz77_kind, o.window_size, o.max_length, o.lz77_level) == (2 | 3 << 8, 1024, 16, 0)
    L = _ffi.lib()
    for depth in (0, 256, -1):
        assert L.lfx_encode_bound(10, C.byref(lfx.zlib.EncodeOptions(lz77=lfx.lz77.ChainLz77Encoder(depth))._to_c()), None) == 0
    # the header length is the default kind's: the level sits in bytes that are there anyway
    for fmt in (0, 1, 2):
        assert L.lfx_container_header_len(fmt, C.byref(_ffi.make_opts(lz77_kind=2 | 8 << 8))) == L.lfx_container_header_len(fmt, None)


def test_host_arithmetic_under_the_host_compiler(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "chain_opts")
    subprocess.run([gxx, "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "c", "chain_opts.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "chain_opts ok: 2000 plans, 2000 lists" in out.stdout, (out.stdout[-400:], out.stderr[-400:])
