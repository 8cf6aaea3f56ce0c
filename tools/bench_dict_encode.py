"""GPU box: the encode leg of tools/bench_dict.py.  The same 4096 text records of about 1 KiB and the same
32 KiB dictionary: lfx_encode_batch_dict_device (zlib, FDICT) against lfx_encode_batch_device on device-resident input and
output, in one process.  Host clock around the blocking C call (it ends in a device synchronise), 3 warm-ups, 15 rounds, the
two calls alternating; median and min - max of each; every round's streams are read back with python-zlib and compared with
the records after the clock stops; the phases of lfx_ctx_last_timing come from a second, untimed pass.  Writes
profiles/dict_batch_encode.json and prints it as one JSON line."""
import json
import os
import random
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COUNT, WARM, ROUNDS = 4096, 3, 15
WORDS = ("the of and to in is that for it as was with be by on not he this are or his from at which but have an had they you "
         "were their one all we can her has there been if more when will would who so no record field value status error "
         "request response timestamp user session message level info warning host port path query result count total").split()


def text(n, seed):
    """tools/bench_dict.py's records and dictionary"""
    rng = random.Random(seed)
    out, size = [], 0
    while size < n:
        w = rng.choice(WORDS) if rng.random() < 0.9 else str(rng.randrange(100000))
        out.append(w)
        size += len(w) + 1
    return " ".join(out).encode()[:n]


def main():
    import ctypes as C

    import numpy as np
    sys.path.insert(0, ROOT)
    import torch

    import libflate_amd
    from libflate_amd import _ffi

    ctx = libflate_amd.Context(0)
    zdict = text(32768, 1)
    d = libflate_amd.Dictionary(zdict, ctx)
    rng = random.Random(7)
    recs = [text(rng.randrange(900, 1200), 100 + i) for i in range(COUNT)]
    total_in = sum(len(r) for r in recs)
    d_in = torch.from_numpy(np.frombuffer(b"".join(recs), dtype=np.uint8).copy()).cuda()
    in_offs, pos = [], 0
    for r in recs:
        in_offs.append(pos)
        pos += len(r)
    in_lens = [len(r) for r in recs]
    opts = _ffi.make_opts()
    caps = [(_ffi.lib().lfx_encode_dict_bound(n, C.byref(opts), None) + 3) & ~3 for n in in_lens]
    out_offs, pos = [], 0
    for c in caps:
        out_offs.append(pos)
        pos += c
    d_out = torch.empty(pos, dtype=torch.uint8, device="cuda")

    def call(zd):
        return ctx.encode_batch_dict_device(_ffi.ZLIB, zd, d_in.data_ptr(), in_offs, in_lens, d_out.data_ptr(), out_offs, caps, opts)

    sizes = {}

    def clock(key, zd):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc, res = call(zd)
        dt = time.perf_counter() - t0
        assert rc == 0 and all(st == 0 for st, _ in res)
        host = d_out.cpu().numpy().tobytes()
        for (st, ol), off, r in zip(res, out_offs, recs):
            z = zlib.decompressobj(zdict=zdict) if zd is not None else zlib.decompressobj()
            assert z.decompress(host[off:off + ol]) + z.flush() == r
        sizes[key] = sum(ol for _, ol in res)
        return dt * 1e3

    runs = {"dict": d, "plain": None}
    for _ in range(WARM):
        for k, zd in runs.items():
            clock(k, zd)
    ts = {k: [] for k in runs}
    for _ in range(ROUNDS):
        for k, zd in runs.items():
            ts[k].append(clock(k, zd))
    ctx.enable_timing(True)
    phases = {}
    for k, zd in runs.items():
        call(zd)
        phases[k] = [(n, round(ms, 4)) for n, ms in ctx.last_timing()["phases"]]
    ctx.enable_timing(False)
    rec = {"tool": "tools/bench_dict_encode.py", "records": COUNT, "record_bytes_mean": round(total_in / COUNT, 1),
           "dictionary_bytes": len(zdict), "input_bytes": total_in,
           "python_zlib_level9_bytes_per_record": {"dict": 373, "plain": 499},
           "method": "host clock around the blocking call, %d warm-ups, %d rounds, alternating; streams checked every round" % (WARM, ROUNDS)}
    for k in runs:
        med = statistics.median(ts[k])
        rec[k] = {"compressed_bytes": sizes[k], "compressed_bytes_per_record": round(sizes[k] / COUNT, 1), "ms_median": round(med, 4),
                  "ms_min": round(min(ts[k]), 4), "ms_max": round(max(ts[k]), 4), "records_per_s": round(COUNT / (med * 1e-3)),
                  "input_GBps": round(total_in / (med * 1e-3) / 1e9, 3), "phases_ms": phases[k]}
    d.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "dict_batch_encode.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
