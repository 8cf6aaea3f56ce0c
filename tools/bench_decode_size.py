"""GPU box: the size calls (lfx_decode_size_device, lfx_decode_batch_size_device, lfx_decode_members_size_device) against the
decode a caller runs today to learn a size, on the same device-resident input, in one process.
--yardstick-lib PATH: a liblfx.so built from the parent commit, loaded beside this tree's (two ctypes handles, one context
each); without it the yardstick is this tree's own decode.  Host clock around the blocking C call, 3 warm-ups, 15 rounds, the
size call and the yardstick alternating; median and min - max of each; the reported size is compared with the known length
after the clock stops; the phases of lfx_ctx_last_timing come from a second, untimed pass.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import libflate_amd  # noqa: E402
import synth  # noqa: E402
from libflate_amd import _ffi  # noqa: E402
import bench_members  # noqa: E402  (input builders: batch_encoded, bgzf_members)

MIB, KIB = 1 << 20, 1 << 10
WARM, ROUNDS = 3, 15
u64 = C.c_uint64


def dev(data):
    return torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).cuda()


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def stats(ts):
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def run_case(name, size_fn, yard_fn, this_fn, check, ctx):
    for _ in range(WARM):
        size_fn(); yard_fn(); this_fn()
    ts, ty, tt = [], [], []
    for _ in range(ROUNDS):
        t, r = clock(size_fn); ts.append(t); check(r)
        t, _ = clock(yard_fn); ty.append(t)
        t, _ = clock(this_fn); tt.append(t)
    ctx.enable_timing(True)
    size_fn()
    phases = ctx.last_timing()
    ctx.enable_timing(False)
    s, y = stats(ts), stats(ty)
    overlap = not (s["max"] < y["min"] or y["max"] < s["min"])
    return {"case": name, "size_ms": s, "decode_parent_ms": y, "decode_this_ms": stats(tt), "ratio": round(s["median"] / y["median"], 3),
            "spread": {"ranges_overlap": overlap, "faster": s["median"] < y["median"] and not overlap},
            "phases": [(n, round(ms, 4)) for n, ms in (phases or {}).get("phases", [])]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--yardstick-lib", default=None)
    ap.add_argument("--cases", default="abcdefgh")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _ffi.lib()
    ctx = libflate_amd.Context(0)
    if a.yardstick_lib:
        Y = C.CDLL(a.yardstick_lib)
        Y.lfx_ctx_new.restype = C.c_void_p
        Y.lfx_ctx_new.argtypes = [C.c_int, C.POINTER(C.c_int)]
        Y.lfx_decode_device.argtypes = L.lfx_decode_device.argtypes
        Y.lfx_decode_batch_device.argtypes = L.lfx_decode_batch_device.argtypes
        Y.lfx_decode_members_device.argtypes = L.lfx_decode_members_device.argtypes
        st = C.c_int(0)
        yh = Y.lfx_ctx_new(0, C.byref(st))
        assert yh and st.value == 0
    else:
        yctx = libflate_amd.Context(0)      # (kept: a temporary's handle would be freed with it before the first call)
        Y, yh = L, yctx.handle
    h = ctx.handle
    results = []

    def single(name, fmt, z, n):
        d_in, d_out = dev(z), torch.empty(max(n, 1), dtype=torch.uint8, device="cuda")
        ol, used = u64(0), u64(0)

        def size_fn():
            rc = L.lfx_decode_size_device(h, fmt, 0, d_in.data_ptr(), len(z), C.byref(ol), C.byref(used))
            return rc, ol.value, used.value

        def dec(lib, handle):
            a_, b_ = u64(0), u64(0)
            return lambda: lib.lfx_decode_device(handle, fmt, 0, d_in.data_ptr(), len(z), d_out.data_ptr(), n, C.byref(a_), C.byref(b_))

        def check(r):
            assert r == (0, n, len(z)), r
        results.append(run_case(name, size_fn, dec(Y, yh), dec(L, h), check, ctx))

    def batch(name, fmt, streams, sizes):
        k = len(streams)
        offs = np.concatenate([[0], np.cumsum([len(s) for s in streams])[:-1]]).astype(np.uint64)
        lens = np.array([len(s) for s in streams], dtype=np.uint64)
        d_in = dev(b"".join(streams))
        out_off = np.concatenate([[0], np.cumsum([(s + 3) & ~3 for s in sizes])[:-1]]).astype(np.uint64)
        out_cap = np.array(sizes, dtype=np.uint64)
        d_out = torch.empty(int(out_off[-1]) + sizes[-1] + 4, dtype=torch.uint8, device="cuda")
        ol, used, st = np.zeros(k, dtype=np.uint64), np.zeros(k, dtype=np.uint64), np.zeros(k, dtype=np.int32)

        def size_fn():
            rc = L.lfx_decode_batch_size_device(h, fmt, k, d_in.data_ptr(), offs.ctypes.data, lens.ctypes.data, ol.ctypes.data,
                                                used.ctypes.data, st.ctypes.data)
            return rc

        def dec(lib, handle):
            gl, gs = np.zeros(k, dtype=np.uint64), np.zeros(k, dtype=np.int32)
            return lambda: lib.lfx_decode_batch_device(handle, fmt, k, d_in.data_ptr(), offs.ctypes.data, lens.ctypes.data, d_out.data_ptr(),
                                                       out_off.ctypes.data, out_cap.ctypes.data, gl.ctypes.data, gs.ctypes.data)

        def check(rc):
            assert rc == 0 and not st.any() and ol.tolist() == list(sizes) and used.tolist() == lens.tolist()
        results.append(run_case(name, size_fn, dec(Y, yh), dec(L, h), check, ctx))

    def members(name, parts, sizes, extra=b""):
        data = b"".join(parts) + extra
        total = sum(sizes)
        d_in, d_out = dev(data), torch.empty(total, dtype=torch.uint8, device="cuda")
        cap_m = len(parts) + 2
        table = (_ffi.Member * cap_m)()
        ol, used, cnt = u64(0), u64(0), C.c_uint32(0)

        def size_fn():
            rc = L.lfx_decode_members_size_device(h, d_in.data_ptr(), len(data), C.byref(ol), C.byref(used), table, cap_m, C.byref(cnt))
            return rc, ol.value, used.value

        def dec(lib, handle):
            t2 = (_ffi.Member * cap_m)()
            a_, b_, c_ = u64(0), u64(0), C.c_uint32(0)
            return lambda: lib.lfx_decode_members_device(handle, d_in.data_ptr(), len(data), d_out.data_ptr(), total, C.byref(a_), C.byref(b_),
                                                         t2, cap_m, C.byref(c_))

        def check(r):
            assert r == (0, total, len(data)), r
        results.append(run_case(name, size_fn, dec(Y, yh), dec(L, h), check, ctx))

    text = synth.text(256 * MIB)
    enc = lambda raw, ws: ctx.encode_host(_ffi.GZIP, raw, _ffi.make_opts(), _ffi.make_schedule(ws))
    if "a" in a.cases:
        single("a: 256 MiB TEXT gzip S8K", _ffi.GZIP, enc(text.tobytes(), 8192), 256 * MIB)
    if "b" in a.cases:
        single("b: 128 MiB TEXT gzip S1", _ffi.GZIP, enc(text[:128 * MIB].tobytes(), 0), 128 * MIB)
    if "c" in a.cases:
        single("c: 128 MiB python-zlib level 6", _ffi.ZLIB, zlib.compress(text[:128 * MIB].tobytes(), 6), 128 * MIB)
    if "d" in a.cases or "f" in a.cases:
        count, size = bench_members.COUNT, bench_members.SIZE
        plain = text[:count * size]
        if "d" in a.cases:
            batch("d: 4096 x 64 KiB batch", _ffi.GZIP, bench_members.batch_encoded(ctx, torch.from_numpy(plain).cuda()), [size] * count)
        if "f" in a.cases:
            members("f: 4096 BGZF members", bench_members.bgzf_members(plain.tobytes()), [size] * count, bench_members.BGZF_EOF)
    if "e" in a.cases:
        raw = text.tobytes()
        batch("e: 512 python-zlib streams of 256 KiB", _ffi.ZLIB,
              [zlib.compress(raw[i * 256 * KIB:(i + 1) * 256 * KIB], 6) for i in range(512)], [256 * KIB] * 512)
    if "g" in a.cases:
        single("g: one 64 KiB gzip stream", _ffi.GZIP, enc(text[:64 * KIB].tobytes(), 8192), 64 * KIB)
    if "h" in a.cases:
        single("h: one 3 KiB stream", _ffi.GZIP, enc(text[:3 * KIB].tobytes(), 8192), 3 * KIB)
    line = json.dumps({"bench": "decode_size", "yardstick_lib": bool(a.yardstick_lib), "cases": results})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
