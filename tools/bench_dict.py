"""GPU box: a batch of small records that share a preset dictionary (lfx_decode_batch_dict_device) against the same records
compressed without one (lfx_decode_batch_device), in one process.  4096 text records of about 1 KiB,
python-zlib level 9, device-resident input and output.  Host clock around the blocking C call (it ends in a device
synchronise), 3 warm-ups, 15 rounds, the two calls alternating; median and min - max of each; every round's outputs are
compared with the records after the clock stops; the phases of lfx_ctx_last_timing come from a second, untimed pass.
Writes profiles/dict_batch.json and prints it as one JSON line."""
import ctypes as C
import json
import os
import random
import statistics
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import libflate_amd  # noqa: E402
from libflate_amd import _ffi  # noqa: E402

COUNT, WARM, ROUNDS = 4096, 3, 15
WORDS = ("the of and to in is that for it as was with be by on not he this are or his from at which but have an had they you "
         "were their one all we can her has there been if more when will would who so no record field value status error "
         "request response timestamp user session message level info warning host port path query result count total").split()


def text(n, seed):
    rng = random.Random(seed)
    out, size = [], 0
    while size < n:
        w = rng.choice(WORDS) if rng.random() < 0.9 else str(rng.randrange(100000))
        out.append(w)
        size += len(w) + 1
    return " ".join(out).encode()[:n]


def dev(data):
    return torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).cuda()


def main():
    ctx = libflate_amd.Context(0)
    zdict = text(32768, 1)
    d = libflate_amd.Dictionary(zdict, ctx)
    rng = random.Random(7)
    recs = [text(rng.randrange(900, 1200), 100 + i) for i in range(COUNT)]
    total_out = sum(len(r) for r in recs)

    def pack(streams):
        offs, pos = [], 0
        for z in streams:
            offs.append(pos)
            pos += len(z)
        return dev(b"".join(streams)), offs, [len(z) for z in streams]

    def comp(r, zd):
        co = zlib.compressobj(9, zlib.DEFLATED, 15, zdict=zd) if zd is not None else zlib.compressobj(9, zlib.DEFLATED, 15)
        return co.compress(r) + co.flush()
    with_d = pack([comp(r, zdict) for r in recs])
    plain = pack([comp(r, None) for r in recs])
    out_offs, pos = [], 0
    for r in recs:
        out_offs.append(pos)
        pos += len(r)
    caps = [len(r) for r in recs]
    d_out = torch.empty(total_out, dtype=torch.uint8, device="cuda")
    want = np.frombuffer(b"".join(recs), dtype=np.uint8)

    def call(zd, packed):
        d_in, offs, lens = packed
        return ctx.decode_batch_dict_device(_ffi.ZLIB, zd, d_in.data_ptr(), offs, lens, d_out.data_ptr(), out_offs, caps)

    def clock(fn):
        d_out.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        dt = time.perf_counter() - t0
        assert all(st == 0 and ol == c for (st, ol), c in zip(res, caps)) and (d_out.cpu().numpy() == want).all()
        return dt * 1e3

    runs = {"dict": lambda: call(d, with_d), "plain": lambda: call(None, plain)}
    for _ in range(WARM):
        for fn in runs.values():
            clock(fn)
    ts = {k: [] for k in runs}
    for _ in range(ROUNDS):
        for k, fn in runs.items():
            ts[k].append(clock(fn))
    ctx.enable_timing(True)
    phases = {}
    for k, fn in runs.items():
        fn()
        phases[k] = [(n, round(ms, 4)) for n, ms in ctx.last_timing()["phases"]]
    ctx.enable_timing(False)
    rec = {"tool": "tools/bench_dict.py", "records": COUNT, "record_bytes_mean": round(total_out / COUNT, 1),
           "dictionary_bytes": len(zdict), "output_bytes": total_out, "encoder": "python-zlib level 9",
           "method": "host clock around the blocking call, %d warm-ups, %d rounds, alternating; outputs checked every round" % (WARM, ROUNDS)}
    for k, packed in (("dict", with_d), ("plain", plain)):
        med = statistics.median(ts[k])
        rec[k] = {"compressed_bytes": sum(packed[2]), "ms_median": round(med, 4), "ms_min": round(min(ts[k]), 4),
                  "ms_max": round(max(ts[k]), 4), "records_per_s": round(COUNT / (med * 1e-3)),
                  "output_GBps": round(total_out / (med * 1e-3) / 1e9, 3), "phases_ms": phases[k]}
    d.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "dict_batch.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
