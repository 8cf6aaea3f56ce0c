"""CPU: the host side of block_merge — the field in include/lfx.h and its Python and Rust mirrors, the option
builders and the keyword, the bounds (host only: no device is touched), the plan that never sees the option, the hook's export,
and tests/c/block_merge.cpp: the domain, every served/refused cell, the region layout over seeded plans and the merge tree of
the kernel's own source against the rule — built by the plain host compiler and once more, as its own executable, under the
address and undefined-behaviour sanitizers."""
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


def test_the_field_and_its_mirrors(lfx):
    from libflate_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "lfx.h")).read()
    assert re.search(r"uint32_t extra_len;\s*\n\s*uint32_t block_merge;", hdr) and "#define LFX_MERGE_MAX 16" in hdr
    assert C.sizeof(_ffi.EncodeOpts) == 72 and _ffi.EncodeOpts.block_merge.offset == 52      # in what was padding
    assert _ffi.EncodeOpts.extra_len.offset == 48 and _ffi.EncodeOpts.filename.offset == 56
    rs = open(os.path.join(ROOT, "rust", "libflate-amd", "src", "ffi.rs")).read()
    assert re.search(r"pub extra_len: u32,\s*\n\s*pub block_merge: u32,", rs)
    for name in ("deflate.rs", "zlib.rs", "gzip.rs"):
        assert "pub fn merge_blocks(mut self) -> Self" in open(os.path.join(ROOT, "rust", "libflate-amd", "src", name)).read(), name
    hooks = open(os.path.join(ROOT, "include", "lfx_testhooks.h")).read()
    assert "int lfx_debug_block_merges(lfx_ctx *c, uint32_t *out, size_t max_blocks, size_t *n_blocks);" in hooks
    assert hasattr(_ffi.lib(), "lfx_debug_block_merges")
    assert _ffi.make_opts().block_merge == 0


def test_option_builders_and_bounds(lfx):
    from libflate_amd import _ffi
    for mod in (lfx.deflate, lfx.zlib, lfx.gzip):
        o = mod.EncodeOptions().merge_blocks()._to_c()
        assert o.block_merge == 1 and (o.block_size, o.dynamic_huffman, o.no_compression, o.lz77_kind) == (1 << 20, 1, 0, 0)
        assert mod.EncodeOptions().merge_blocks().auto_huffman_codes()._to_c().dynamic_huffman == 2
        assert mod.EncodeOptions()._to_c().block_merge == 0
    L = _ffi.lib()
    sched = _ffi.make_schedule(4096)
    for n in (0, 1, 100, 70000, 5 << 20):
        for kw in ({}, {"block_size": 4096}, {"window_size": 1024}, {"dynamic_huffman": 2, "block_size": 4096}):
            off, on = _ffi.make_opts(**kw), _ffi.make_opts(block_merge=1, **kw)
            assert L.lfx_encode_bound(n, C.byref(off), C.byref(sched)) == L.lfx_encode_bound(n, C.byref(on), C.byref(sched)) != 0
            assert L.lfx_encode_dict_bound(n, C.byref(off), None) == L.lfx_encode_dict_bound(n, C.byref(on), None)
    for v in (2, 7, 2 ** 32 - 1):                          # outside the domain: no bound
        assert L.lfx_encode_bound(100, C.byref(_ffi.make_opts(block_merge=v)), None) == 0
    assert L.lfx_encode_members_bound(100000, 65280, 1, C.byref(_ffi.make_opts(block_merge=1)), None) == 0      # refused
    for fmt in (0, 1, 2):
        assert L.lfx_container_header_len(fmt, C.byref(_ffi.make_opts(block_merge=1))) == L.lfx_container_header_len(fmt, None)


def test_the_planner_never_sees_it(lfx):
    from libflate_amd import _ffi
    L = _ffi.lib()

    def plan(bm, n, sched, **kw):
        o = _ffi.make_opts(block_merge=bm, **kw)
        ch, bl = (C.c_uint64 * (4 * 4096))(), (C.c_uint64 * (6 * 4096))()
        nc, nb = C.c_size_t(0), C.c_size_t(0)
        assert L.lfx_debug_plan(1, C.byref(o), C.byref(sched), n, ch, 4096, C.byref(nc), bl, 4096, C.byref(nb)) == 0
        return list(ch[:4 * nc.value]), list(bl[:6 * nb.value])

    for n, sched, kw in ((0, _ffi.make_schedule(), {}), (100000, _ffi.make_schedule(4096), {"block_size": 4096}),
                         (70000, _ffi.make_schedule(0, [100, None, 30000, None]), {"zlib_flush_mode": 2, "window_size": 1024})):
        assert plan(1, n, sched, **kw) == plan(0, n, sched, **kw)


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_host_arithmetic_under_the_host_compiler(tmp_path, flags):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "block_merge")
    subprocess.run([gxx, "-O2", "-std=c++17", "-Wall", *flags, "-o", exe, os.path.join(ROOT, "tests", "c", "block_merge.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and re.search(r"block_merge ok: 270 cells, 66 refused, 2000 plans, \d+ regions, 300 trees", out.stdout), \
        (out.stdout[-400:], out.stderr[-400:])
