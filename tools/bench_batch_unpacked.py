"""GPU box: the packed batch decode (lfx_decode_batch_packed_device) against the composition it replaces, on the
same device bytes, in one process, the two alternating round by round:
  text_4096x64k   4096 gzip members of 64 KiB text   |  lfx_decode_batch_size_device, a prefix sum on the host (numpy),
                                                     |  lfx_decode_batch_device with out_cap = the sizes
  dict_65536x1k   65536 zlib records of 1 KiB text,  |  the size calls take no dictionary (an FDICT header is an error to them), so
                  one 32 KiB dictionary              |  this composition does not exist today: the yardstick is its decode half alone,
                                                     |  lfx_decode_batch_dict_device at places the caller already knows (1 KiB each)
The streams come from lfx_encode_batch_packed_device.  Wall clock around the blocking calls, input and output resident in HBM;
3 warm-up and 15 timed rounds; median and min–max.  No ratio is fixed in advance: the yardstick is the composition of the same
run, and its own min–max spread is the margin.  Behind the timing: the two layouts and the two outputs are compared whole, on
the device.  Also reported: the phase timers of one more call each; "layout" is the new call's upload of the sizes, its three
layout kernels and the copy-back of the layout.  Writes profiles/batch_unpacked.json (--out) and prints it as one line.
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
    out = {}
    for k, v in t["phases"]:               # (a phase name recurs per block round: summed)
        out[k] = round(out.get(k, 0.0) + v, 4)
    return out


def run_case(ctx, name, fmt, d_rec, count, size, zd):
    L = _ffi.lib()
    n = count * size
    handle = zd.handle if zd is not None else None
    rec_off = [i * size for i in range(count)]
    rc, comp_total, _ = ctx.encode_batch_packed_device(fmt, d_rec.data_ptr(), rec_off, [size] * count, None, 0, zdict=zd)
    d_comp = torch.empty(comp_total, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc, comp_total, layout = ctx.encode_batch_packed_device(fmt, d_rec.data_ptr(), rec_off, [size] * count, d_comp.data_ptr(), comp_total,
                                                            zdict=zd)
    assert rc == 0
    in_off = np.array([o for o, _ in layout], dtype=np.uint64)
    in_len = np.array([l for _, l in layout], dtype=np.uint64)
    d_a = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_b = torch.zeros(n, dtype=torch.uint8, device="cuda")
    c_size, c_used, c_sst = np.zeros(count, dtype=np.uint64), np.zeros(count, dtype=np.uint64), np.zeros(count, dtype=np.int32)
    c_off, c_len, c_st = np.zeros(count, dtype=np.uint64), np.zeros(count, dtype=np.uint64), np.zeros(count, dtype=np.int32)
    p_off, p_len, p_used, p_st, total = (np.zeros(count, dtype=np.uint64), np.zeros(count, dtype=np.uint64),
                                         np.zeros(count, dtype=np.uint64), np.zeros(count, dtype=np.int32), C.c_uint64(0))
    known = np.full(count, size, dtype=np.uint64)
    rcs = {}

    def composition():
        if zd is None:
            rcs["size"] = L.lfx_decode_batch_size_device(ctx.handle, fmt, count, d_comp.data_ptr(), in_off.ctypes.data, in_len.ctypes.data,
                                                         c_size.ctypes.data, c_used.ctypes.data, c_sst.ctypes.data)
            sizes = c_size
        else:
            rcs["size"] = 0
            sizes = known
        c_off[0] = 0
        np.cumsum(sizes[:-1], out=c_off[1:])
        if zd is None:
            rcs["decode"] = L.lfx_decode_batch_device(ctx.handle, fmt, count, d_comp.data_ptr(), in_off.ctypes.data, in_len.ctypes.data,
                                                      d_a.data_ptr(), c_off.ctypes.data, sizes.ctypes.data, c_len.ctypes.data,
                                                      c_st.ctypes.data)
        else:
            rcs["decode"] = L.lfx_decode_batch_dict_device(ctx.handle, fmt, handle, count, d_comp.data_ptr(), in_off.ctypes.data,
                                                           in_len.ctypes.data, d_a.data_ptr(), c_off.ctypes.data, sizes.ctypes.data,
                                                           c_len.ctypes.data, c_st.ctypes.data)

    def packed():
        rcs["packed"] = L.lfx_decode_batch_packed_device(ctx.handle, fmt, handle, count, d_comp.data_ptr(), in_off.ctypes.data,
                                                         in_len.ctypes.data, None, 1, d_b.data_ptr(), n, p_off.ctypes.data, p_len.ctypes.data,
                                                         p_used.ctypes.data, p_st.ctypes.data, C.byref(total), None)

    t = interleaved({"composition": composition, "packed": packed})
    composition()
    packed()
    ok = rcs["size"] == 0 and rcs["decode"] == 0 and rcs["packed"] == 0 and not c_st.any() and not p_st.any() and \
        np.array_equal(p_off, c_off) and np.array_equal(p_len, c_len) and total.value == n and np.array_equal(p_used, in_len) and \
        bool(torch.equal(d_a, d_b)) and bool(torch.equal(d_a, d_rec[:n]))
    sc, sp = stats(t["composition"], n), stats(t["packed"], n)
    ph_p = phases(ctx, packed)
    if zd is None:
        ph_c = {"size_call": phases(ctx, lambda: L.lfx_decode_batch_size_device(ctx.handle, fmt, count, d_comp.data_ptr(), in_off.ctypes.data,
                                                                                in_len.ctypes.data, c_size.ctypes.data, c_used.ctypes.data,
                                                                                c_sst.ctypes.data)),
                "decode_call": phases(ctx, lambda: L.lfx_decode_batch_device(ctx.handle, fmt, count, d_comp.data_ptr(), in_off.ctypes.data,
                                                                             in_len.ctypes.data, d_a.data_ptr(), c_off.ctypes.data,
                                                                             c_size.ctypes.data, c_len.ctypes.data, c_st.ctypes.data))}
    else:
        ph_c = {"decode_call": phases(ctx, composition)}
    return {"case": name, "format": {0: "deflate", 1: "zlib", 2: "gzip"}[fmt], "records": count, "record_bytes": size, "output_bytes": n,
            "input_bytes": int(comp_total), "dictionary": zd is not None, "ok": bool(ok),
            "yardstick": "size call + host prefix sum + batch decode" if zd is None else
                         "the dictionary batch decode at known places alone (no size call takes a dictionary)",
            "composition": dict(sc, phases_ms=ph_c), "packed": dict(sp, phases_ms=ph_p, layout_ms=ph_p.get("layout")),
            "composition_spread_ms": round(sc["max_ms"] - sc["min_ms"], 4),
            "packed_minus_composition_median_ms": round(sp["median_ms"] - sc["median_ms"], 4),
            "packed_inside_composition_spread": bool(sc["min_ms"] <= sp["median_ms"] <= sc["max_ms"]),
            "packed_over_composition_median": round(sp["median_ms"] / sc["median_ms"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_unpacked.json"))
    a = ap.parse_args()
    ctx = libflate_amd.Context(0)
    runs = []
    count, size = 4096 // a.scale, 64 << 10
    d_text = torch.from_numpy(synth.text(count * size)).cuda()
    runs.append(run_case(ctx, "text_4096x64k", _ffi.GZIP, d_text, count, size, None))
    count, size = 65536 // a.scale, 1 << 10
    zdict = synth.text((32 << 10) + 4096)[4096:].tobytes()          # (text of the same source, other bytes than the records' first)
    d_text = torch.from_numpy(synth.text(count * size)).cuda()
    zd = libflate_amd.Dictionary(zdict, ctx)
    try:
        runs.append(run_case(ctx, "dict_65536x1k", _ffi.ZLIB, d_text, count, size, zd))
    finally:
        zd.close()
    rec = {"workload": "batch decode placed back to back by the decoded sizes against the composition it replaces, resident in HBM",
           "unit": "ms per call (wall clock, blocking calls); GB/s of output", "warmup": WARMUP, "reps": REPS, "interleaved": True,
           "scale": a.scale, "all_ok": all(r["ok"] for r in runs), "runs": runs}
    line = json.dumps(rec)
    with open(a.out, "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")
    print(line)
    return 0 if rec["all_ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
