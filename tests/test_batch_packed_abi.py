"""CPU: lfx_encode_batch_packed_device — declared, exported, bound, no CPU fallback — and the layout arithmetic
its kernels share with the host (libflate_amd/csrc/lfx_batch_pack.h), walked by tests/c/batch_packed.cpp and held against the
model below: out_off[0] = 0, out_off[i + 1] = round_up(out_off[i] + len[i], align), total = the last stream's end."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "lfx_encode_batch_packed_device"
ALIGNS = (1, 2, 4, 64, 4096)
COUNTS = (1, 255, 256, 257, 65537, 262400)      # 262400 = 1025 workgroup sums: two rounds of the second level


def layout_model(lens, align):
    """→ (offsets, total), straight from the rule"""
    offs, at = [], 0
    for n in lens:
        at = -(-at // align) * align
        offs.append(at)
        at += int(n)
    return offs, at


def layout_model_np(lens, align):
    """the same rule without a Python loop per stream: out_off[i] = the sum of round_up(len, align) in front of i"""
    lens = np.asarray(lens, dtype=np.uint64)
    terms = (lens + np.uint64(align - 1)) // np.uint64(align) * np.uint64(align)
    offs = np.concatenate([np.zeros(1, np.uint64), np.cumsum(terms[:-1], dtype=np.uint64)])
    return offs, int(offs[-1]) + int(lens[-1])


@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as g
    g.build()
    from libflate_amd import _ffi
    return _ffi


def test_declared_exported_bound(ffi):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lfx_[a-z0-9_]+)\s*\(", hdr))
    out = subprocess.run(["nm", "-D", "--defined-only", ffi.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines()}
    assert NAME in declared and NAME in exported and NAME in ffi.EXPORTS and hasattr(ffi.lib(), NAME)
    assert len(ffi.lib().lfx_encode_batch_packed_device.argtypes) == 16
    # the Rust crate leaves it unbound (INTEGRATION.md says so)
    assert NAME not in open(os.path.join(ROOT, "rust", "libflate-amd", "src", "ffi.rs")).read()
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_null_context_is_a_device_error(ffi):
    L = ffi.lib()
    one = lambda v: (C.c_uint64 * 1)(v)
    off, ln, total = one(7), one(7), C.c_uint64(7)
    out = C.create_string_buffer(b"\xA5" * 64, 64)
    for fmt in (ffi.DEFLATE, ffi.ZLIB, ffi.GZIP):
        assert L.lfx_encode_batch_packed_device(None, fmt, None, None, None, 1, b"abc", one(0), one(3), 1, out, 64, off, ln,
                                                C.byref(total), None) == ffi.E_DEVICE
    # nothing was computed on the CPU: the outputs are untouched
    assert off[0] == 7 and ln[0] == 7 and total.value == 7 and out.raw == b"\xA5" * 64


def test_python_surface(ffi):
    import inspect
    import libflate_amd
    from libflate_amd import deflate, gzip, zlib
    sig = inspect.signature(libflate_amd.Context.encode_batch_packed_device)
    assert list(sig.parameters)[:7] == ["self", "fmt", "d_in", "in_offs", "in_lens", "d_out", "cap"]
    for kw, default in (("zdict", None), ("opts", None), ("schedule", None), ("align", 1), ("d_table", None)):
        assert sig.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[kw].default == default
    for mod, has_dict in ((gzip, False), (zlib, True), (deflate, True)):
        p = inspect.signature(mod.compress_batch).parameters
        want = set(inspect.signature(mod.compress).parameters) - {"data"}
        assert "records" in p and want <= set(p) and ("zdict" in p) == has_dict, mod.__name__


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan_ubsan"])
def program(request, tmp_path_factory):
    """a program of its own (nothing loaded into Python runs under a sanitizer)"""
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path_factory.mktemp("bpack") / "batch_packed")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param else ["-O2"]
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "c", "batch_packed.cpp")],
                   check=True)
    return exe


def test_layout_header_self_checks(program):
    out = subprocess.run([program, "self"], capture_output=True, text=True)
    assert out.returncode == 0 and "batch_packed self ok" in out.stdout, (out.stdout[-400:], out.stderr[-400:])


def test_model_np_is_the_rule():
    rng = np.random.default_rng(5)
    for align in ALIGNS:
        lens = rng.integers(0, 9000, 700)
        offs, total = layout_model(lens, align)
        offs_np, total_np = layout_model_np(lens, align)
        assert offs == [int(x) for x in offs_np] and total == total_np


@pytest.mark.parametrize("count", COUNTS)
def test_layout_against_the_model(program, tmp_path, count):
    rng = np.random.default_rng(count)
    for align in ALIGNS:
        # ragged: mostly small streams, zero lengths, a few large ones; lengths that are and are not multiples of align
        lens = rng.integers(0, 3 * align + 70, count).astype(np.uint64)
        lens[rng.integers(0, count, max(count // 50, 1))] = 0
        lens[rng.integers(0, count, max(count // 100, 1))] = rng.integers(1 << 20, 1 << 33, max(count // 100, 1)).astype(np.uint64)
        src, dst = str(tmp_path / "lens.u64"), str(tmp_path / "offs.u64")
        lens.astype("<u8").tofile(src)
        out = subprocess.run([program, "layout", str(align), src, dst], capture_output=True, text=True)
        assert out.returncode == 0, (out.stdout[-400:], out.stderr[-400:])
        nwg = -(-count // 256)
        assert "count=%d nwg=%d rounds=%d " % (count, nwg, -(-nwg // 1024)) in out.stdout, out.stdout
        got = np.fromfile(dst, dtype="<u8")
        want, total = layout_model_np(lens, align)
        assert len(got) == count + 1 and np.array_equal(got[:-1], want) and int(got[-1]) == total, (count, align)
        assert all(int(x) % align == 0 for x in got[:-1][:: max(count // 997, 1)])
        if count <= 257:
            ref, ref_total = layout_model(lens, align)
            assert [int(x) for x in got[:-1]] == ref and int(got[-1]) == ref_total


def test_layout_overflow_is_refused(program, tmp_path):
    src, dst = str(tmp_path / "lens.u64"), str(tmp_path / "offs.u64")
    for lens, align, over in (([2 ** 64 - 11, 10], 1, False), ([2 ** 64 - 11, 11], 1, True), ([2 ** 64 - 11, 10], 2, True),
                              ([2 ** 63, 2 ** 62, 2 ** 62], 4096, True), ([2 ** 48] * 70000, 1, True), ([2 ** 48] * 65535, 64, False)):
        np.array(lens, dtype="<u8").tofile(src)
        out = subprocess.run([program, "layout", str(align), src, dst], capture_output=True, text=True)
        assert (out.returncode, "overflow" in out.stdout) == ((3, True) if over else (0, False)), (lens[:3], align, out.stdout, out.stderr)
