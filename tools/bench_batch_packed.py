"""GPU box: the packed batch encode (lfx_encode_batch_packed_device) against the batch call it generalises, on the
same device bytes, in one process, the two calls alternating round by round:
  text_4096x64k    4096 records of 64 KiB text, gzip             |  lfx_encode_batch_device, outputs at lfx_encode_bound spacing
  dict_262144x1k   262144 records of 1 KiB, one dictionary, zlib |  lfx_encode_batch_dict_device, outputs at lfx_encode_dict_bound spacing
The packed call gets cap = the sum of the bounds.  Wall clock around the blocking calls, input and output resident in HBM; 3
warm-up and 15 timed rounds; median and min–max.  No ratio is fixed in advance: the yardstick is the batch call of the same
run, and its own min–max spread is the margin.  Behind the timing: the packed layout follows the rule, its total is the sum of
the batch call's lengths, and sampled streams are compared byte for byte on the device.  Also reported: the bytes each call
zero-fills and the phase timers of one more call each.  Writes profiles/batch_packed.json (--out) and prints it as one line.
--scale N: 1/N of the records (rehearsals)."""
import argparse
import ctypes as C
import json
import os
import statistics
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
            "GBps_median": round(n / med / 1e9, 2)}


def interleaved(calls):
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


def phases(ctx, call):
    ctx.enable_timing(True)
    call()
    t = ctx.last_timing() or {"phases": []}
    ctx.enable_timing(False)
    return {k: round(v, 4) for k, v in t["phases"]}


def run_case(ctx, name, fmt, d_in, count, size, zd):
    L = _ffi.lib()
    opts = _ffi.make_opts()
    handle = zd.handle if zd is not None else None
    bound = (L.lfx_encode_dict_bound if zd is not None else L.lfx_encode_bound)(size, C.byref(opts), None)
    spacing = (bound + 3) & ~3
    n = count * size
    in_off = np.arange(count, dtype=np.uint64) * np.uint64(size)
    in_len = np.full(count, size, dtype=np.uint64)
    # the batch call: outputs at bound spacing
    d_sparse = torch.empty(count * spacing, dtype=torch.uint8, device="cuda")
    b_off = np.arange(count, dtype=np.uint64) * np.uint64(spacing)
    b_cap = np.full(count, spacing, dtype=np.uint64)
    b_len, b_st = np.zeros(count, dtype=np.uint64), np.zeros(count, dtype=np.int32)
    # the packed call: cap = the sum of the bounds
    cap = count * bound
    d_dense = torch.empty(cap, dtype=torch.uint8, device="cuda")
    p_off, p_len, total = np.zeros(count, dtype=np.uint64), np.zeros(count, dtype=np.uint64), C.c_uint64(0)
    rcs = {}

    def batch():
        if zd is not None:
            rcs["batch"] = L.lfx_encode_batch_dict_device(ctx.handle, fmt, C.byref(opts), None, handle, count, d_in.data_ptr(),
                                                          in_off.ctypes.data, in_len.ctypes.data, d_sparse.data_ptr(), b_off.ctypes.data,
                                                          b_cap.ctypes.data, b_len.ctypes.data, b_st.ctypes.data)
        else:
            rcs["batch"] = L.lfx_encode_batch_device(ctx.handle, fmt, C.byref(opts), None, count, d_in.data_ptr(), in_off.ctypes.data,
                                                     in_len.ctypes.data, d_sparse.data_ptr(), b_off.ctypes.data, b_cap.ctypes.data,
                                                     b_len.ctypes.data, b_st.ctypes.data)

    def packed():
        rcs["packed"] = L.lfx_encode_batch_packed_device(ctx.handle, fmt, C.byref(opts), None, handle, count, d_in.data_ptr(),
                                                         in_off.ctypes.data, in_len.ctypes.data, 1, d_dense.data_ptr(), cap,
                                                         p_off.ctypes.data, p_len.ctypes.data, C.byref(total), None)

    t = interleaved({"batch": batch, "packed": packed})
    batch()
    packed()
    ok = rcs["batch"] == 0 and rcs["packed"] == 0 and not b_st.any() and np.array_equal(p_len, b_len) and \
        total.value == int(b_len.sum()) and p_off[0] == 0 and np.array_equal(p_off[1:], np.cumsum(b_len)[:-1])
    for i in sorted(set(int(x) for x in np.linspace(0, count - 1, 64))):
        a = d_sparse[int(b_off[i]):int(b_off[i]) + int(b_len[i])]
        b = d_dense[int(p_off[i]):int(p_off[i]) + int(p_len[i])]
        ok = ok and a.numel() == b.numel() and bool(torch.equal(a, b))
    sb, sp = stats(t["batch"], n), stats(t["packed"], n)
    spread = round(sb["max_ms"] - sb["min_ms"], 4)
    delta = round(sp["median_ms"] - sb["median_ms"], 4)
    ph_b, ph_p = phases(ctx, batch), phases(ctx, packed)
    return {"case": name, "format": {0: "deflate", 1: "zlib", 2: "gzip"}[fmt], "records": count, "record_bytes": size, "input_bytes": n,
            "dictionary": zd is not None, "output_bytes": total.value, "ok": bool(ok),
            "zero_filled_bytes": {"batch": int(count * spacing), "packed": int(min(cap, count * bound))},
            "batch": dict(sb, phases_ms=ph_b), "packed": dict(sp, phases_ms=ph_p, layout_kernels_ms=ph_p.get("batch_layout")),
            "batch_spread_ms": spread, "packed_minus_batch_median_ms": delta,
            "packed_inside_batch_spread": bool(sb["min_ms"] <= sp["median_ms"] <= sb["max_ms"]),
            "packed_over_batch_median": round(sp["median_ms"] / sb["median_ms"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_packed.json"))
    a = ap.parse_args()
    ctx = libflate_amd.Context(0)
    runs = []
    count, size = 4096 // a.scale, 64 << 10
    d_text = torch.from_numpy(synth.text(count * size)).cuda()
    runs.append(run_case(ctx, "text_4096x64k", _ffi.GZIP, d_text, count, size, None))
    count, size = 262144 // a.scale, 1 << 10
    zdict = synth.text((32 << 10) + 4096)[4096:].tobytes()          # (text of the same source, other bytes than the records' first)
    d_text = torch.from_numpy(synth.text(count * size)).cuda()
    zd = libflate_amd.Dictionary(zdict, ctx)
    try:
        runs.append(run_case(ctx, "dict_262144x1k", _ffi.ZLIB, d_text, count, size, zd))
    finally:
        zd.close()
    rec = {"workload": "batch encode with the streams packed back to back against the batch call at bound spacing, resident in HBM",
           "unit": "ms per call (wall clock, blocking call); GB/s of input", "warmup": WARMUP, "reps": REPS, "interleaved": True,
           "scale": a.scale, "all_ok": all(r["ok"] for r in runs), "runs": runs}
    line = json.dumps(rec)
    with open(a.out, "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")
    print(line)
    return 0 if rec["all_ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
