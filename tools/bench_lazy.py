"""GPU box: what lazy matching costs and buys on top of a chain depth (LazyLz77Encoder, LFX_LZ77_LAZY), by
tools/bench_chain.py's method.  Two workloads in one process: the text corpus bench.py encodes (256 MiB, device-resident, gzip,
8 KiB writes) through lfx_encode_device, and tools/bench_dict.py's 4096 records of about 1 KiB through
lfx_encode_batch_device (zlib).  Kind 0, and the chain and the lazy encoder at the depths 1, 8 and 32, alternating: 3 warm-ups,
15 rounds; host clock around the blocking C call (it ends in a device synchronise); median, min and max of each, GB/s of
input, the two kernels of the chain stage (the phases lz77_chain_cand and lz77_lazy_demote) from a second, untimed pass of
lfx_ctx_last_timing, the demote kernel's GB/s over the 5 bytes a position it moves, the compressed bytes, and python-zlib's
sizes at levels 1, 6 and 9 on the same input.  `--prefix N` also records every kind's compressed size of the corpus's first N
bytes in one write_all (raw DEFLATE), for a comparison with tests/lazy_model.py on the CPU.  Every timed call runs under a watchdog of its own: a
call that does not return within CALL_LIMIT_S ends the tool with status 124 and nothing else is started.  After the
timed rounds every kind's streams are inflated by python-zlib and compared with the input.
Writes profiles/lazy_encode.json and prints it as one JSON line.  `--bytes N`: a smaller corpus (development)."""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys
import threading
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

DEPTHS = (1, 8, 32)
WARM, ROUNDS, COUNT, WRITE = 3, 15, 4096, 8192
CALL_LIMIT_S = 60
WORDS = ("the of and to in is that for it as was with be by on not he this are or his from at which but have an had they you "
         "were their one all we can her has there been if more when will would who so no record field value status error "
         "request response timestamp user session message level info warning host port path query result count total").split()


def text(n, seed):
    """tools/bench_dict.py's records"""
    rng = random.Random(seed)
    out, size = [], 0
    while size < n:
        w = rng.choice(WORDS) if rng.random() < 0.9 else str(rng.randrange(100000))
        out.append(w)
        size += len(w) + 1
    return " ".join(out).encode()[:n]


def guarded(fn):
    """fn() under a time limit of its own"""
    t = threading.Timer(CALL_LIMIT_S, lambda: (sys.stderr.write("bench_lazy: a timed call exceeded %d s\n" % CALL_LIMIT_S), os._exit(124)))
    t.daemon = True
    t.start()
    try:
        return fn()
    finally:
        t.cancel()


def measure(ctx, torch, runs, check):
    """runs: key → a callable that returns the compressed size.  → key → the record"""
    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        size = guarded(fn)
        return (time.perf_counter() - t0) * 1e3, size
    for _ in range(WARM):
        for fn in runs.values():
            clock(fn)
    ts, sizes = {k: [] for k in runs}, {}
    for _ in range(ROUNDS):
        for k, fn in runs.items():
            ms, sizes[k] = clock(fn)
            ts[k].append(ms)
    out = {}
    ctx.enable_timing(True)
    for k, fn in runs.items():
        guarded(fn)
        phases = [(n, round(ms, 4)) for n, ms in ctx.last_timing()["phases"]]
        check(k)
        out[k] = {"compressed_bytes": sizes[k], "ms_median": round(statistics.median(ts[k]), 4), "ms_min": round(min(ts[k]), 4),
                  "ms_max": round(max(ts[k]), 4), "lz77_chain_cand_ms": dict(phases).get("lz77_chain_cand", 0.0),
                  "lz77_lazy_demote_ms": dict(phases).get("lz77_lazy_demote", 0.0), "phases_ms": phases}
    ctx.enable_timing(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=256 << 20)
    ap.add_argument("--prefix", type=int, default=0, help="also the compressed sizes of the corpus's first N bytes, one write_all, raw DEFLATE")
    ap.add_argument("--no-zlib", action="store_true", help="skip python-zlib's sizes of the corpus (minutes of CPU at 256 MiB)")
    args = ap.parse_args()
    import numpy as np
    import torch

    import libflate_amd
    import synth
    from libflate_amd import _ffi
    L = _ffi.lib()
    ctx = libflate_amd.Context(0)
    keys = ["default"] + [name % k for k in DEPTHS for name in ("chain_%d", "lazy_%d")]
    kinds = dict(zip(keys, [_ffi.LZ77_DEFAULT] + [kind | k << 8 for k in DEPTHS for kind in (_ffi.LZ77_CHAIN, _ffi.LZ77_LAZY)]))
    rec = {"tool": "tools/bench_lazy.py",
           "method": "host clock around the blocking call, %d warm-ups, %d rounds, the kinds alternating; the last streams inflated "
                     "by python-zlib" % (WARM, ROUNDS)}

    # ---- the corpus
    n = args.bytes
    data = synth.text(n, seed=synth.SEED_BASE + 2)
    d_in = torch.from_numpy(data).cuda()
    sched = _ffi.make_schedule(WRITE)
    opts = {k: _ffi.make_opts(mtime=0, lz77_kind=v) for k, v in kinds.items()}
    bound = L.lfx_encode_bound(n, C.byref(opts["default"]), C.byref(sched)) & ~3
    d_out = torch.empty(bound, dtype=torch.uint8, device="cuda")
    raw = data.tobytes()

    def one(k):
        return lambda: ctx.encode_device(_ffi.GZIP, d_in.data_ptr(), n, d_out.data_ptr(), bound, opts[k], sched)
    last = {}

    def check_corpus(k):
        m = one(k)()
        z = d_out[:m].cpu().numpy().tobytes()
        assert zlib.decompress(z, 31) == raw, k
        last[k] = m
    corpus = measure(ctx, torch, {k: one(k) for k in keys}, check_corpus)
    for k in keys:
        corpus[k]["input_GBps"] = round(n / (corpus[k]["ms_median"] * 1e-3) / 1e9, 3)
        if corpus[k]["lz77_lazy_demote_ms"]:      # 1 byte of length read, 2 + 2 bytes of candidate read and written, per position
            corpus[k]["demote_GBps"] = round(5 * n / (corpus[k]["lz77_lazy_demote_ms"] * 1e-3) / 1e9, 1)
    for d in DEPTHS:
        corpus["lazy_%d" % d]["extra_ms_over_chain"] = round(corpus["lazy_%d" % d]["ms_median"] - corpus["chain_%d" % d]["ms_median"], 4)
    rec["corpus"] = {"workload": "lfx_encode_device, gzip, %d bytes of synth.text, 8 KiB writes, device-resident" % n, "input_bytes": n,
                     "runs": corpus}
    if not args.no_zlib:
        rec["corpus"]["python_zlib_bytes"] = {"level_%d" % lv: len(zlib.compress(raw, lv)) for lv in (1, 6, 9)}
    if args.prefix:
        popts = {k: _ffi.make_opts(lz77_kind=v) for k, v in kinds.items()}
        rec["corpus"]["prefix"] = {"bytes": args.prefix, "format": "raw DEFLATE, one write_all", "compressed_bytes": {
            k: ctx.encode_device(_ffi.DEFLATE, d_in.data_ptr(), args.prefix, d_out.data_ptr(), bound, popts[k], None) for k in keys}}
    del d_in, d_out

    # ---- the records
    rng = random.Random(7)
    recs = [text(rng.randrange(900, 1200), 100 + i) for i in range(COUNT)]
    total_in = sum(len(r) for r in recs)
    b_in = torch.from_numpy(np.frombuffer(b"".join(recs), dtype=np.uint8).copy()).cuda()
    in_lens = [len(r) for r in recs]
    in_offs = [0]
    for ln in in_lens[:-1]:
        in_offs.append(in_offs[-1] + ln)
    caps = [(L.lfx_encode_bound(ln, C.byref(opts["default"]), None) + 3) & ~3 for ln in in_lens]
    out_offs = [0]
    for c in caps[:-1]:
        out_offs.append(out_offs[-1] + c)
    b_out = torch.empty(sum(caps), dtype=torch.uint8, device="cuda")
    a = lambda v: (C.c_uint64 * COUNT)(*v)
    io, il, oo, oc = a(in_offs), a(in_lens), a(out_offs), a(caps)
    ol, st = (C.c_uint64 * COUNT)(), (C.c_int32 * COUNT)()
    bopts = {k: _ffi.make_opts(lz77_kind=v) for k, v in kinds.items()}

    def batch(k):
        def run():
            rc = L.lfx_encode_batch_device(ctx.handle, _ffi.ZLIB, C.byref(bopts[k]), None, COUNT, b_in.data_ptr(), io, il, b_out.data_ptr(),
                                           oo, oc, ol, st)
            assert rc == 0, ctx.last_error()
            return sum(ol)
        return run

    def check_batch(k):
        batch(k)()
        host = b_out.cpu().numpy().tobytes()
        for r, off, ln in zip(recs, out_offs, ol):
            assert zlib.decompress(host[off:off + ln]) == r, k
    records = measure(ctx, torch, {k: batch(k) for k in keys}, check_batch)
    for d in DEPTHS:
        records["lazy_%d" % d]["extra_ms_over_chain"] = round(records["lazy_%d" % d]["ms_median"] - records["chain_%d" % d]["ms_median"], 4)
    for k in keys:
        records[k]["compressed_bytes_per_record"] = round(records[k]["compressed_bytes"] / COUNT, 1)
        records[k]["records_per_s"] = round(COUNT / (records[k]["ms_median"] * 1e-3))
        records[k]["input_GBps"] = round(total_in / (records[k]["ms_median"] * 1e-3) / 1e9, 3)
    rec["records"] = {"workload": "lfx_encode_batch_device, zlib, %d records of %.1f bytes on average (tools/bench_dict.py's), one write_all "
                                  "each" % (COUNT, total_in / COUNT), "input_bytes": total_in, "runs": records,
                      "python_zlib_bytes": {"level_%d" % lv: sum(len(zlib.compress(r, lv)) for r in recs) for lv in (1, 6, 9)}}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    if n == 256 << 20:
        with open(os.path.join(ROOT, "profiles", "lazy_encode.json"), "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
