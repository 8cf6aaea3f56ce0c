"""GPU box: the members encoder (lfx_encode_members_device) against its yardsticks, on the same device bytes, in one process,
the calls of a pair interleaved repetition by repetition:
  bgzf_text      256 MiB TEXT at 65280 bytes per member, BGZF  |  lfx_encode_batch_device on the same slices, gzip, outputs at
                 lfx_encode_bound spacing (it writes no BSIZE, compacts nothing, and zero-fills the larger span)
  plain_1mib     the same text at 1 MiB per member, plain      |  lfx_encode_device, gzip, 1 MiB blocks: one member
  bgzf_random    256 MiB of random bytes at 65505 per member, BGZF: every full member falls back to a stored block | (none)
Wall clock around the blocking calls, input and output resident in HBM; GB/s of input bytes.  The bytes are checked AFTER the
timing: lfx_decode_members_device reads the output back to the input, the member table tiles the output, and a host walk hops
through the BGZF output by BSIZE alone.  Prints one JSON line.   --mib N: another input size (rehearsals)."""
import argparse
import ctypes as C
import json
import os
import statistics
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import libflate_amd  # noqa: E402
import synth  # noqa: E402
from libflate_amd import _ffi  # noqa: E402

WARMUP, REPS = 3, 15


def stats(ts, n):
    ts = sorted(ts)
    med = statistics.median(ts)
    return {"median_ms": round(med * 1e3, 4), "min_ms": round(ts[0] * 1e3, 4), "max_ms": round(ts[-1] * 1e3, 4),
            "p25_ms": round(ts[len(ts) // 4] * 1e3, 4), "p75_ms": round(ts[(3 * len(ts)) // 4] * 1e3, 4),
            "GBps_median": round(n / med / 1e9, 2)}


def interleaved(calls):
    """calls: name → callable; WARMUP rounds untimed, then REPS rounds, every call once per round → name → [seconds]"""
    out = {k: [] for k in calls}
    for r in range(WARMUP + REPS):
        for k, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if r >= WARMUP:
                out[k].append(dt)
    return out


def members_call(ctx, d_in, n, d_out, cap, member_size, flags, res):
    """the C call alone, on a table allocated once (the Python wrapper's list of tuples is read once, in verify)"""
    L = _ffi.lib()
    opts = _ffi.make_opts()
    count = -(-n // member_size)
    table = (_ffi.Member * count)()
    out_len, got = C.c_uint64(0), C.c_uint32(0)

    def call():
        rc = L.lfx_encode_members_device(ctx.handle, C.byref(opts), None, member_size, flags, d_in.data_ptr(), n, d_out.data_ptr(), cap,
                                         C.byref(out_len), table, count, C.byref(got))
        res["m"] = (rc, out_len.value, got.value, table, ctx.last_error() if rc else "")
    return call


def batch_call(ctx, d_in, n, member_size, res):
    L = _ffi.lib()
    opts, sched = _ffi.make_opts(), _ffi.make_schedule(0)
    count = -(-n // member_size)
    bound = (L.lfx_encode_bound(member_size, C.byref(opts), C.byref(sched)) + 3) & ~3
    d_streams = torch.zeros(count * bound, dtype=torch.uint8, device="cuda")
    in_off = np.arange(count, dtype=np.uint64) * np.uint64(member_size)
    in_len = np.minimum(np.uint64(n) - in_off, np.uint64(member_size)).astype(np.uint64)
    out_off = np.arange(count, dtype=np.uint64) * np.uint64(bound)
    out_cap = np.full(count, bound, dtype=np.uint64)
    out_len = np.zeros(count, dtype=np.uint64)
    status = np.zeros(count, dtype=np.int32)

    def call():
        res["b"] = L.lfx_encode_batch_device(ctx.handle, _ffi.GZIP, C.byref(opts), C.byref(sched), count, d_in.data_ptr(),
                                             in_off.ctypes.data, in_len.ctypes.data, d_streams.data_ptr(), out_off.ctypes.data,
                                             out_cap.ctypes.data, out_len.ctypes.data, status.ctypes.data)
    return call, lambda: res["b"] == 0 and not status.any(), lambda: int(out_len.sum()), d_streams


def verify(ctx, d_in, n, d_out, res, member_size, bgzf):
    rc, out_len, count, ctable, msg = res["m"]
    if rc != 0:
        return False, msg, 0
    table = [(m.in_off, m.in_len, m.out_off, m.out_len) for m in ctable[:count]]
    want_count = -(-n // member_size)
    tiles = count == want_count == len(table) and all(table[i][2] + table[i][3] == table[i + 1][2] for i in range(count - 1)) \
        and table[0][2] == 0 and table[-1][2] + table[-1][3] + (28 if bgzf else 0) == out_len
    d_back = torch.zeros(n, dtype=torch.uint8, device="cuda")
    drc, dlen, used, dtab, dmsg = ctx.decode_members_device(d_out.data_ptr(), out_len, d_back.data_ptr(), n, max_members=count + 1)
    back = drc == 0 and dlen == n and used == out_len and torch.equal(d_back, d_in[:n])
    fallbacks, walk = 0, True
    if bgzf:
        host = d_out[:out_len].cpu().numpy().tobytes()
        p, k = 0, 0
        while p < out_len:
            size = struct.unpack_from("<H", host, p + 16)[0] + 1
            walk = walk and host[p:p + 4] == b"\x1f\x8b\x08\x04" and (k == count or size == table[k][3])
            fallbacks += 1 if (k < count and (host[p + 18] & 6) == 0 and table[k][1] > 0) else 0
            p += size
            k += 1
        walk = walk and p == out_len and k == count + 1
    return bool(tiles and back and walk), "" if (tiles and back and walk) else "tiles %s back %s walk %s %s" % (tiles, back, walk, dmsg), fallbacks


def phases(ctx, call):
    ctx.enable_timing(True)
    call()
    t = ctx.last_timing() or {"phases": []}
    ctx.enable_timing(False)
    return {k: round(v, 4) for k, v in t["phases"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    a = ap.parse_args()
    n = a.mib << 20
    ctx = libflate_amd.Context(0)
    L = _ffi.lib()
    d_text = torch.from_numpy(synth.text(n)).cuda()
    runs = []

    # ---- BGZF text against the batch call on the same slices
    ms, flags = _ffi.BGZF_MEMBER_SIZE, _ffi.MEMBERS_BGZF
    cap = L.lfx_encode_members_bound(n, ms, flags, None, None)
    d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    res = {}
    mcall = members_call(ctx, d_text, n, d_out, cap, ms, flags, res)
    bcall, b_ok, b_bytes, d_streams = batch_call(ctx, d_text, n, ms, res)
    t = interleaved({"members": mcall, "batch": bcall})
    mcall()
    ok, why, fb = verify(ctx, d_text, n, d_out, res, ms, True)
    m, b = stats(t["members"], n), stats(t["batch"], n)
    runs.append({"case": "bgzf_text", "input_bytes": n, "member_size": ms, "members": res["m"][2], "stored_fallbacks": fb,
                 "output_bytes": res["m"][1], "zero_filled_bytes": {"members": cap, "batch": int(d_streams.numel())},
                 "encode_members_device": dict(m, ok=ok, why=why, phases_ms=phases(ctx, mcall)),
                 "encode_batch_device": dict(b, ok=bool(b_ok()), output_bytes=b_bytes()),
                 "members_over_batch_median": round(m["median_ms"] / b["median_ms"], 4),
                 "batch_spread_ms": round(b["max_ms"] - b["min_ms"], 4)})
    del d_streams, d_out

    # ---- plain, 1 MiB members, against the single-member encode with 1 MiB blocks
    ms = 1 << 20
    cap = L.lfx_encode_members_bound(n, ms, 0, None, None)
    d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    cap1 = L.lfx_encode_bound(n, None, None) & ~3
    d_one = torch.zeros(cap1, dtype=torch.uint8, device="cuda")
    mcall = members_call(ctx, d_text, n, d_out, cap, ms, 0, res)
    opts = _ffi.make_opts()

    def one():
        res["one"] = ctx.encode_device(_ffi.GZIP, d_text.data_ptr(), n, d_one.data_ptr(), cap1, opts)
    t = interleaved({"members": mcall, "one": one})
    mcall()
    ok, why, _ = verify(ctx, d_text, n, d_out, res, ms, False)
    m, o = stats(t["members"], n), stats(t["one"], n)
    runs.append({"case": "plain_1mib", "input_bytes": n, "member_size": ms, "members": res["m"][2], "output_bytes": res["m"][1],
                 "encode_members_device": dict(m, ok=ok, why=why, phases_ms=phases(ctx, mcall)),
                 "encode_device_1mib_blocks": dict(o, output_bytes=res["one"]),
                 "members_over_single_median": round(m["median_ms"] / o["median_ms"], 4)})
    del d_one, d_out, d_text

    # ---- BGZF random at 65505: every full member is written as one stored block
    ms = 65505
    g = torch.Generator(device="cuda")
    g.manual_seed(20260101)
    d_rnd = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
    cap = L.lfx_encode_members_bound(n, ms, flags, None, None)
    d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    mcall = members_call(ctx, d_rnd, n, d_out, cap, ms, flags, res)
    t = interleaved({"members": mcall})
    mcall()
    ok, why, fb = verify(ctx, d_rnd, n, d_out, res, ms, True)
    m = stats(t["members"], n)
    runs.append({"case": "bgzf_random", "input_bytes": n, "member_size": ms, "members": res["m"][2], "stored_fallbacks": fb,
                 "output_bytes": res["m"][1], "encode_members_device": dict(m, ok=ok, why=why, phases_ms=phases(ctx, mcall))})

    print(json.dumps({"workload": "members encode: one buffer as gzip members / BGZF in one pass, resident in HBM",
                      "unit": "ms per call (wall clock, blocking call); GB/s of input", "warmup": WARMUP, "reps": REPS,
                      "interleaved": True, "all_ok": all(r["encode_members_device"]["ok"] for r in runs), "runs": runs}))
    return 0 if all(r["encode_members_device"]["ok"] for r in runs) else 1


if __name__ == "__main__":
    sys.exit(main())
