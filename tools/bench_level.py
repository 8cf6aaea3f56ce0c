"""GPU box: what each level of LevelLz77Encoder costs and buys (LFX_LZ77_LEVEL), by tools/bench_lazy.py's
method.  Two workloads in one process: the text corpus bench.py encodes (256 MiB, device-resident, gzip, 8 KiB writes) through
lfx_encode_device at the levels 1..9, with kind 0 and LazyLz77Encoder at the depths 8 and 32 beside them, alternating; and
tools/bench_dict.py's 4096 records of about 1 KiB behind its 32 KiB dictionary through lfx_encode_batch_dict_device (zlib, a
chain dictionary) at the levels 1, 6 and 9, with the default parse and lazy 8 and 32 beside them.  Host clock around the
blocking C call (it ends in a device synchronise); median, min and max of each, the two kernels of the chain stage (the phases
lz77_chain_cand and lz77_lazy_demote) from a second, untimed pass of lfx_ctx_last_timing, the compressed bytes, and
python-zlib's size of the same input at the same level.  The levels 7..9 walk up to 4096 candidates a position: they get
SLOW_WARM warm-up and SLOW_ROUNDS rounds where the others get WARM and ROUNDS.  Every timed call runs under a watchdog of its
own: a call that does not return within CALL_LIMIT_S ends the tool with status 124 and nothing else is started.  After the
timed rounds every run's streams are inflated by python-zlib and compared with the input.
Writes --out (default profiles/level_encode.json) and prints it as one JSON line.  `--bytes N`: a smaller corpus."""
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
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_lazy import text  # noqa: E402  (tools/bench_dict.py's records)

LEVELS = tuple(range(1, 10))
SLOW = (7, 8, 9)
WARM, ROUNDS, SLOW_WARM, SLOW_ROUNDS, COUNT, WRITE = 2, 9, 1, 3, 4096, 8192
CALL_LIMIT_S = 90


def guarded(fn):
    """fn() under a time limit of its own"""
    t = threading.Timer(CALL_LIMIT_S, lambda: (sys.stderr.write("bench_level: a timed call exceeded %d s\n" % CALL_LIMIT_S), os._exit(124)))
    t.daemon = True
    t.start()
    try:
        return fn()
    finally:
        t.cancel()


def measure(ctx, torch, runs, slow, check):
    """runs: key → a callable that returns the compressed size; slow: the keys that get fewer rounds.  → key → the record"""
    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        size = guarded(fn)
        return (time.perf_counter() - t0) * 1e3, size
    for r in range(WARM):
        for k, fn in runs.items():
            if k not in slow or r < SLOW_WARM:
                clock(fn)
    ts, sizes = {k: [] for k in runs}, {}
    for r in range(ROUNDS):
        for k, fn in runs.items():
            if k not in slow or r < SLOW_ROUNDS:
                ms, sizes[k] = clock(fn)
                ts[k].append(ms)
    out = {}
    ctx.enable_timing(True)
    for k, fn in runs.items():
        guarded(fn)
        phases = [(n, round(ms, 4)) for n, ms in ctx.last_timing()["phases"]]
        check(k)
        out[k] = {"compressed_bytes": sizes[k], "rounds": len(ts[k]), "ms_median": round(statistics.median(ts[k]), 4),
                  "ms_min": round(min(ts[k]), 4), "ms_max": round(max(ts[k]), 4),
                  "lz77_chain_cand_ms": dict(phases).get("lz77_chain_cand", 0.0),
                  "lz77_lazy_demote_ms": dict(phases).get("lz77_lazy_demote", 0.0), "phases_ms": phases}
    ctx.enable_timing(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=256 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "level_encode.json"))
    ap.add_argument("--no-zlib", action="store_true", help="skip python-zlib's sizes of the corpus")
    args = ap.parse_args()
    import numpy as np
    import torch

    import libflate_amd
    import synth
    from libflate_amd import _ffi
    L = _ffi.lib()
    ctx = libflate_amd.Context(0)
    kinds = {"default": _ffi.LZ77_DEFAULT, "lazy_8": _ffi.LZ77_LAZY | 8 << 8, "lazy_32": _ffi.LZ77_LAZY | 32 << 8}
    kinds.update({"level_%d" % v: _ffi.LZ77_LEVEL | v << 8 for v in LEVELS})
    keys = list(kinds)
    slow = {"level_%d" % v for v in SLOW}
    rec = {"tool": "tools/bench_level.py",
           "method": "host clock around the blocking call, the runs alternating; %d warm-ups and %d rounds, the levels %s %d and %d; "
                     "the last streams inflated by python-zlib" % (WARM, ROUNDS, "/".join(map(str, SLOW)), SLOW_WARM, SLOW_ROUNDS)}

    # ---- the corpus
    n = args.bytes
    data = synth.text(n, seed=synth.SEED_BASE + 2)
    raw = data.tobytes()
    pool = ThreadPoolExecutor(9)          # python-zlib's sizes beside the GPU work (zlib.compress releases the GIL)
    zsizes = {} if args.no_zlib else {"level_%d" % v: pool.submit(lambda v=v: len(zlib.compress(raw, v))) for v in LEVELS}
    d_in = torch.from_numpy(data).cuda()
    sched = _ffi.make_schedule(WRITE)
    opts = {k: _ffi.make_opts(mtime=0, lz77_kind=v) for k, v in kinds.items()}
    bound = L.lfx_encode_bound(n, C.byref(opts["default"]), C.byref(sched)) & ~3
    d_out = torch.empty(bound, dtype=torch.uint8, device="cuda")

    def one(k):
        return lambda: ctx.encode_device(_ffi.GZIP, d_in.data_ptr(), n, d_out.data_ptr(), bound, opts[k], sched)

    def check_corpus(k):
        m = one(k)()
        assert zlib.decompress(d_out[:m].cpu().numpy().tobytes(), 31) == raw, k
    corpus = measure(ctx, torch, {k: one(k) for k in keys}, slow, check_corpus)
    for k in keys:
        corpus[k]["input_GBps"] = round(n / (corpus[k]["ms_median"] * 1e-3) / 1e9, 3)
    rec["corpus"] = {"workload": "lfx_encode_device, gzip, %d bytes of synth.text, 8 KiB writes, device-resident" % n, "input_bytes": n,
                     "runs": corpus, "python_zlib_bytes": {k: f.result() for k, f in zsizes.items()}}
    del d_in, d_out

    # ---- the dictionary batch
    zdict = text(32768, 1)
    chain_d, plain_d = libflate_amd.Dictionary(zdict, ctx, chain=True), libflate_amd.Dictionary(zdict, ctx)
    rng = random.Random(7)
    recs = [text(rng.randrange(900, 1200), 100 + i) for i in range(COUNT)]
    total_in = sum(len(r) for r in recs)
    b_in = torch.from_numpy(np.frombuffer(b"".join(recs), dtype=np.uint8).copy()).cuda()
    in_lens = [len(r) for r in recs]
    in_offs = [sum(in_lens[:i]) for i in range(COUNT)]
    base = _ffi.make_opts()
    caps = [(L.lfx_encode_dict_bound(ln, C.byref(base), None) + 3) & ~3 for ln in in_lens]
    out_offs = [sum(caps[:i]) for i in range(COUNT)]
    b_out = torch.empty(sum(caps), dtype=torch.uint8, device="cuda")
    druns = {"dict_default": (plain_d, base)}
    for k in ("lazy_8", "lazy_32", "level_1", "level_6", "level_9"):
        druns["dict_" + k] = (chain_d, _ffi.make_opts(lz77_kind=kinds[k]))
    res = {}

    def batch(k):
        def run():
            rc, res[k] = ctx.encode_batch_dict_device(_ffi.ZLIB, druns[k][0], b_in.data_ptr(), in_offs, in_lens, b_out.data_ptr(), out_offs,
                                                      caps, druns[k][1])
            assert rc == 0 and all(st == 0 for st, _ in res[k]), ctx.last_error()
            return sum(ol for _, ol in res[k])
        return run

    def check_batch(k):
        batch(k)()
        host = b_out.cpu().numpy().tobytes()
        for r, off, (_, ol) in zip(recs, out_offs, res[k]):
            z = zlib.decompressobj(zdict=zdict)
            assert z.decompress(host[off:off + ol]) + z.flush() == r, k
    records = measure(ctx, torch, {k: batch(k) for k in druns}, {"dict_level_9"}, check_batch)
    for k in druns:
        records[k]["compressed_bytes_per_record"] = round(records[k]["compressed_bytes"] / COUNT, 1)
        records[k]["records_per_s"] = round(COUNT / (records[k]["ms_median"] * 1e-3))

    def zdict_size(r, v):
        z = zlib.compressobj(v, zdict=zdict)
        return len(z.compress(r) + z.flush())
    rec["records"] = {"workload": "lfx_encode_batch_dict_device, zlib, %d records of %.1f bytes on average behind a %d-byte chain dictionary "
                                  "(tools/bench_dict.py's), one write_all each" % (COUNT, total_in / COUNT, len(zdict)),
                      "input_bytes": total_in, "runs": records,
                      "python_zlib_bytes": {"level_%d" % v: sum(zdict_size(r, v) for r in recs) for v in (1, 6, 9)}}
    chain_d.close()
    plain_d.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
