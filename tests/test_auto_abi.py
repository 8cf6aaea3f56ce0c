"""CPU: the host side of LFX_HUFFMAN_AUTO — the constant in include/lfx.h and its Python and Rust mirrors, the
option builders, the bounds (host only: no device is touched), and tests/c/auto_blocks.cpp: the decoding of dynamic_huffman,
the plan of the value 2, and the blocks' in_off / in_len through the planner, its piecewise use and Plan::append, built by the
plain host compiler and once more under the address and undefined-behaviour sanitizers."""
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


def test_constant_and_its_mirrors(lfx):
    from libflate_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "lfx.h")).read()
    m = re.search(r"enum \{ LFX_HUFFMAN_FIXED = (\d+), LFX_HUFFMAN_DYNAMIC = (\d+), LFX_HUFFMAN_AUTO = (\d+) \}", hdr)
    assert m and [int(x) for x in m.groups()] == [0, 1, 2] == [_ffi.HUFFMAN_FIXED, _ffi.HUFFMAN_DYNAMIC, _ffi.HUFFMAN_AUTO]
    rs = open(os.path.join(ROOT, "rust", "libflate-amd", "src", "ffi.rs")).read()
    assert re.search(r"pub const LFX_HUFFMAN_AUTO: i32 = 2;", rs)
    for name in ("deflate.rs", "zlib.rs", "gzip.rs"):
        assert "pub fn auto_huffman_codes(mut self) -> Self" in open(os.path.join(ROOT, "rust", "libflate-amd", "src", name)).read(), name
    assert C.sizeof(_ffi.EncodeOpts) == 72 and _ffi.EncodeOpts.dynamic_huffman.offset == 8      # the layout is unchanged


def test_option_builders_and_bounds(lfx):
    from libflate_amd import _ffi
    for mod in (lfx.deflate, lfx.zlib, lfx.gzip):
        o = mod.EncodeOptions().auto_huffman_codes()._to_c()
        assert o.dynamic_huffman == 2 and (o.block_size, o.no_compression, o.lz77_kind) == (1 << 20, 0, 0)
        assert mod.EncodeOptions().auto_huffman_codes().fixed_huffman_codes()._to_c().dynamic_huffman == 0
    L = _ffi.lib()
    sched = _ffi.make_schedule(8192)
    for n in (0, 1, 100, 70000, 5 << 20):
        for kw in ({}, {"block_size": 4096}, {"window_size": 1024}):
            one, two = _ffi.make_opts(dynamic_huffman=1, **kw), _ffi.make_opts(dynamic_huffman=2, **kw)
            assert L.lfx_encode_bound(n, C.byref(one), C.byref(sched)) == L.lfx_encode_bound(n, C.byref(two), C.byref(sched)) != 0
            assert L.lfx_encode_dict_bound(n, C.byref(one), None) == L.lfx_encode_dict_bound(n, C.byref(two), None)
            assert L.lfx_encode_members_bound(n, 65280, 1, C.byref(one), None) == L.lfx_encode_members_bound(n, 65280, 1, C.byref(two), None)
    for fmt in (0, 1, 2):
        assert L.lfx_container_header_len(fmt, C.byref(_ffi.make_opts(dynamic_huffman=2))) == L.lfx_container_header_len(fmt, None)


def test_the_plan_of_2_is_the_plan_of_1(lfx):
    """through the library's own planner hook: types, ranges and chunks"""
    from libflate_amd import _ffi
    L = _ffi.lib()

    def plan(dh, n, sched, **kw):
        o = _ffi.make_opts(dynamic_huffman=dh, **kw)
        ch, bl = (C.c_uint64 * (4 * 4096))(), (C.c_uint64 * (6 * 4096))()
        nc, nb = C.c_size_t(0), C.c_size_t(0)
        assert L.lfx_debug_plan(1, C.byref(o), C.byref(sched), n, ch, 4096, C.byref(nc), bl, 4096, C.byref(nb)) == 0
        return list(ch[:4 * nc.value]), list(bl[:6 * nb.value])

    for n, sched, kw in ((0, _ffi.make_schedule(), {}), (100000, _ffi.make_schedule(4096), {"block_size": 4096}),
                         (70000, _ffi.make_schedule(0, [100, None, 30000, None]), {"zlib_flush_mode": 2, "window_size": 1024})):
        assert plan(2, n, sched, **kw) == plan(1, n, sched, **kw) == plan(3, n, sched, **kw) == plan(-1, n, sched, **kw)
        assert plan(2, n, sched, **kw) != plan(0, n, sched, **kw)


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_host_arithmetic_under_the_host_compiler(tmp_path, flags):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "auto_blocks")
    subprocess.run([gxx, "-O2", "-std=c++17", "-Wall", *flags, "-o", exe, os.path.join(ROOT, "tests", "c", "auto_blocks.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "auto_blocks ok: 2000 plans" in out.stdout, (out.stdout[-400:], out.stderr[-400:])
