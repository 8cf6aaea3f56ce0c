"""The byte-shuffle filter on the GPU → profiles/shuffle.json.

Time: lfx_shuffle_batch_device in both directions for s = 2, 4, 8 (register path) and 3 (LDS path), on 256 MiB as one record
and on 4096 records of 64 KiB, each against a device-to-device copy of the same bytes in the same run, alternating: both read
n bytes and write n bytes, so the copy is the yardstick.  Every time is a host clock around a call that ends in a device
synchronise (the library call waits itself), the median of --reps calls after --warmup.
Ratio: zlib.compress_batch(level=6) with and without shuffle= on synthetic fp32 and bf16 tensors, every stream inflated by
Python's zlib.

    python tools/bench_shuffle.py --out profiles/shuffle.json
"""
import argparse
import json
import os
import statistics
import sys
import time
import zlib as pyzlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, sync):
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def bench_time(torch, ctx, model, reps, warmup):
    rows = []
    shapes = (("1 x 256 MiB", 1, 256 << 20), ("4096 x 64 KiB", 4096, 64 << 10))
    for label, count, size in shapes:
        n = count * size
        src = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        back = torch.empty_like(src)
        offs, lens = [i * size for i in range(count)], [size] * count
        sync = torch.cuda.synchronize
        sync()
        for s in (2, 4, 8, 3):
            fwd = lambda: ctx.shuffle_batch_device(src.data_ptr(), offs, lens, dst.data_ptr(), s)
            inv = lambda: ctx.shuffle_batch_device(dst.data_ptr(), offs, lens, back.data_ptr(), s, inverse=True)
            cpy = lambda: back.copy_(src)
            fwd(); inv(); sync()
            assert torch.equal(back, src), "unshuffle(shuffle(x)) != x"
            head = dst[:size].cpu().numpy().tobytes()
            assert head == model.shuffle(src[:size].cpu().numpy().tobytes(), s), "record 0 differs from the model"
            t = {"shuffle": [], "unshuffle": [], "copy": []}
            for i in range(warmup + reps):
                a, c1, b, c2 = timed(fwd, sync), timed(cpy, sync), timed(inv, sync), timed(cpy, sync)
                if i >= warmup:
                    t["shuffle"].append(a); t["unshuffle"].append(b); t["copy"] += [c1, c2]
            inv(); sync()      # (back holds the copy's bytes: put the inverse there again for the next size's check)
            med = {k: statistics.median(v) for k, v in t.items()}
            row = {"shape": label, "bytes": n, "elem_size": s, "path": "register" if s in (2, 4, 8, 16) else "lds"}
            for k, v in med.items():
                row[k + "_ms"] = round(v, 4)
                row[k + "_ms_min"] = round(min(t[k]), 4)
                row[k + "_GBps"] = round(n / v / 1e6, 1)             # bytes of the record per second (each is read once and written once)
            row["shuffle_vs_copy"] = round(med["copy"] / med["shuffle"], 3)
            row["unshuffle_vs_copy"] = round(med["copy"] / med["unshuffle"], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def tensors():
    rng = np.random.default_rng(5)
    n = 1 << 20
    t = np.arange(n, dtype=np.float64)
    signal = (np.sin(t / 5000) * 50 + np.sin(t / 37) + rng.normal(0, 0.01, n)).astype(np.float32)
    weights = rng.normal(0, 0.02, n).astype(np.float32)
    bf16 = lambda a: (a.view(np.uint32) >> 16).astype(np.uint16)
    return (("fp32 smooth signal plus noise", signal.tobytes(), 4), ("fp32 normal weights (sigma 0.02)", weights.tobytes(), 4),
            ("bf16 smooth signal plus noise", bf16(signal).tobytes(), 2), ("bf16 normal weights (sigma 0.02)", bf16(weights).tobytes(), 2))


def bench_ratio(lfx, ctx, model):
    rows = []
    for name, data, s in tensors():
        recs = [data[i:i + (64 << 10)] for i in range(0, len(data), 64 << 10)]
        plain = lfx.zlib.compress_batch(recs, context=ctx, level=6)
        shuf = lfx.zlib.compress_batch(recs, context=ctx, level=6, shuffle=s)
        assert [pyzlib.decompress(x) for x in plain] == recs
        assert [model.unshuffle(pyzlib.decompress(x), s) for x in shuf] == recs
        assert lfx.zlib.decompress_batch(shuf, context=ctx, shuffle=s) == recs
        py_plain = sum(len(pyzlib.compress(r, 6)) for r in recs)
        py_shuf = sum(len(pyzlib.compress(model.shuffle(r, s), 6)) for r in recs)
        a, b = sum(map(len, plain)), sum(map(len, shuf))
        row = {"input": name, "bytes": len(data), "records": len(recs), "elem_size": s, "level6_bytes": a, "level6_shuffle_bytes": b,
               "ratio_plain": round(a / len(data), 4), "ratio_shuffle": round(b / len(data), 4), "shuffle_over_plain": round(b / a, 4),
               "python_zlib6_bytes": py_plain, "python_zlib6_shuffle_bytes": py_shuf}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shuffle.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    import libflate_amd as lfx
    import shuffle_model as model
    ctx = lfx.Context(0)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
           "timing": "host clock around a call that ends in a device synchronise; median; the copy is torch's device-to-device copy_",
           "time": bench_time(torch, ctx, model, a.reps, a.warmup), "ratio": bench_ratio(lfx, ctx, model)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
