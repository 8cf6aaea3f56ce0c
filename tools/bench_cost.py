"""What CostLz77Encoder costs and buys (LFX_LZ77_COST), by tools/bench_level.py's method: kind 4 is the yardstick,
at the same level in the same run.

On the GPU box (the default mode).  Two workloads in one process: the text corpus bench.py encodes (256 MiB, device-resident,
gzip, 8 KiB writes) through lfx_encode_device, and tools/bench_dict.py's 4096 records of about 1 KiB behind its 32 KiB chain
dictionary through lfx_encode_batch_dict_device (zlib) — each at the levels 1, 6 and 9 with LevelLz77Encoder and CostLz77Encoder
alternating, WARM warm-ups and ROUNDS rounds.  Host clock around the blocking C call (it ends in a device synchronise): median,
min and max; the phases lz77_cost_pass1 and lz77_cost_demote from a further, untimed pass of lfx_ctx_last_timing; the
compressed bytes; python-zlib's sizes at 6 and 9 alongside.  Every timed call runs under a watchdog of its own.  After the
timed rounds every run's streams are inflated by python-zlib and compared with the input.  The corpus's first 512 KiB are
encoded once more per level with the cost kind (one zlib stream, 8 KiB writes): the sizes the CPU model must give too.

`--model` (no GPU): tests/cost_model.py's sizes of those 512 KiB, level by level (`--levels`), merged into --out under
"model_512k" — the Python model measures every candidate of every position, so a level takes minutes.
Writes --out (default profiles/cost_parse.json) and prints it as one JSON line.  `--bytes N`: a smaller corpus."""
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

LEVELS = (1, 6, 9)
WARM, ROUNDS, COUNT, WRITE = 3, 15, 4096, 8192
HEAD = 512 << 10
CALL_LIMIT_S = 90


def guarded(fn):
    """fn() under a time limit of its own"""
    t = threading.Timer(CALL_LIMIT_S, lambda: (sys.stderr.write("bench_cost: a timed call exceeded %d s\n" % CALL_LIMIT_S), os._exit(124)))
    t.daemon = True
    t.start()
    try:
        return fn()
    finally:
        t.cancel()


def measure(ctx, torch, runs, check):
    """runs: key → a callable that returns the compressed size → key → the record"""
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
        out[k] = {"compressed_bytes": sizes[k], "rounds": len(ts[k]), "ms_median": round(statistics.median(ts[k]), 4),
                  "ms_min": round(min(ts[k]), 4), "ms_max": round(max(ts[k]), 4),
                  "lz77_cost_pass1_ms": dict(phases).get("lz77_cost_pass1", 0.0),
                  "lz77_cost_demote_ms": dict(phases).get("lz77_cost_demote", 0.0), "phases_ms": phases}
    ctx.enable_timing(False)
    return out


def versus(runs):
    """cost against level at every level: the size gained and the time paid, with kind 4's own spread as the margin"""
    out = {}
    for v in LEVELS:
        pre = "" if "level_%d" % v in runs else "dict_"
        a, b = runs["%slevel_%d" % (pre, v)], runs["%scost_%d" % (pre, v)]
        out["level_%d" % v] = {"bytes_saved": a["compressed_bytes"] - b["compressed_bytes"],
                               "bytes_saved_percent": round(100.0 * (a["compressed_bytes"] - b["compressed_bytes"]) / a["compressed_bytes"], 3),
                               "ms_median_ratio": round(b["ms_median"] / a["ms_median"], 3),
                               "ms_added": round(b["ms_median"] - a["ms_median"], 4),
                               "level_ms_spread": round(a["ms_max"] - a["ms_min"], 4)}
    return out


def model(args):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cost_model
    import synth
    from oracle import lfo_oracle as oracle
    head = synth.text(HEAD, seed=synth.SEED_BASE + 2).tobytes()
    got = {}
    for v in args.levels:
        t0 = time.perf_counter()
        got["cost_%d" % v] = len(cost_model.expected_stream(oracle, oracle.ZLIB, head, v, write_size=WRITE))
        sys.stderr.write("bench_cost: the model at level %d: %.0f s\n" % (v, time.perf_counter() - t0))
    rec = json.load(open(args.out)) if os.path.exists(args.out) else {"tool": "tools/bench_cost.py"}
    rec.setdefault("model_512k", {}).update(got)
    dev = rec.get("head_512k", {}).get("device_bytes", {})
    rec["model_512k_equals_device"] = {k: dev[k] == n for k, n in rec["model_512k"].items() if k in dev}
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"model_512k": rec["model_512k"], "equals_device": rec["model_512k_equals_device"]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=256 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cost_parse.json"))
    ap.add_argument("--model", action="store_true", help="the CPU model's sizes of the corpus's first 512 KiB, merged into --out")
    ap.add_argument("--levels", type=int, nargs="+", default=list(LEVELS))
    args = ap.parse_args()
    if args.model:
        return model(args)
    import numpy as np
    import torch

    import libflate_amd
    import synth
    from bench_lazy import text
    from libflate_amd import _ffi
    L = _ffi.lib()
    ctx = libflate_amd.Context(0)
    kinds = {}
    for v in LEVELS:                      # (alternating: level, cost, level, cost ...)
        kinds["level_%d" % v] = _ffi.LZ77_LEVEL | v << 8
        kinds["cost_%d" % v] = _ffi.LZ77_COST | v << 8
    rec = {"tool": "tools/bench_cost.py",
           "method": "host clock around the blocking call, kind 4 and the cost kind alternating in one process; %d warm-ups and %d rounds; "
                     "every run's last streams inflated by python-zlib" % (WARM, ROUNDS)}

    # ---- the corpus
    n = args.bytes
    data = synth.text(n, seed=synth.SEED_BASE + 2)
    raw = data.tobytes()
    pool = ThreadPoolExecutor(2)          # python-zlib's sizes beside the GPU work (zlib.compress releases the GIL)
    zsizes = {"level_%d" % v: pool.submit(lambda v=v: len(zlib.compress(raw, v))) for v in (6, 9)}
    d_in = torch.from_numpy(data).cuda()
    sched = _ffi.make_schedule(WRITE)
    opts = {k: _ffi.make_opts(mtime=0, lz77_kind=v) for k, v in kinds.items()}
    bound = L.lfx_encode_bound(n, C.byref(opts["level_1"]), C.byref(sched)) & ~3
    d_out = torch.empty(bound, dtype=torch.uint8, device="cuda")

    def one(k, fmt=_ffi.GZIP, m=n):
        return lambda: ctx.encode_device(fmt, d_in.data_ptr(), m, d_out.data_ptr(), bound, opts[k], sched)

    def check_corpus(k):
        m = one(k)()
        assert zlib.decompress(d_out[:m].cpu().numpy().tobytes(), 31) == raw, k
    corpus = measure(ctx, torch, {k: one(k) for k in kinds}, check_corpus)
    for k in kinds:
        corpus[k]["input_GBps"] = round(n / (corpus[k]["ms_median"] * 1e-3) / 1e9, 3)
    rec["corpus"] = {"workload": "lfx_encode_device, gzip, %d bytes of synth.text, 8 KiB writes, device-resident" % n, "input_bytes": n,
                     "runs": corpus, "cost_against_level": versus(corpus), "python_zlib_bytes": {k: f.result() for k, f in zsizes.items()}}
    # the first 512 KiB as a zlib stream of their own: what the CPU model is held against
    head = min(HEAD, n)
    dev = {}
    for v in LEVELS:
        m = one("cost_%d" % v, _ffi.ZLIB, head)()
        z = d_out[:m].cpu().numpy().tobytes()
        assert zlib.decompress(z) == raw[:head]
        dev["cost_%d" % v] = m
    rec["head_512k"] = {"workload": "lfx_encode_device, zlib, the corpus's first %d bytes, 8 KiB writes" % head, "device_bytes": dev}
    del d_in, d_out

    # ---- the dictionary batch
    zdict = text(32768, 1)
    chain_d = libflate_amd.Dictionary(zdict, ctx, chain=True)
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
    druns = {"dict_" + k: _ffi.make_opts(lz77_kind=v) for k, v in kinds.items()}
    res = {}

    def batch(k):
        def run():
            rc, res[k] = ctx.encode_batch_dict_device(_ffi.ZLIB, chain_d, b_in.data_ptr(), in_offs, in_lens, b_out.data_ptr(), out_offs, caps,
                                                      druns[k])
            assert rc == 0 and all(st == 0 for st, _ in res[k]), ctx.last_error()
            return sum(ol for _, ol in res[k])
        return run

    def check_batch(k):
        batch(k)()
        host = b_out.cpu().numpy().tobytes()
        for r, off, (_, ol) in zip(recs, out_offs, res[k]):
            z = zlib.decompressobj(zdict=zdict)
            assert z.decompress(host[off:off + ol]) + z.flush() == r, k
    records = measure(ctx, torch, {k: batch(k) for k in druns}, check_batch)
    for k in druns:
        records[k]["compressed_bytes_per_record"] = round(records[k]["compressed_bytes"] / COUNT, 1)
        records[k]["records_per_s"] = round(COUNT / (records[k]["ms_median"] * 1e-3))

    def zdict_size(r, v):
        z = zlib.compressobj(v, zdict=zdict)
        return len(z.compress(r) + z.flush())
    rec["records"] = {"workload": "lfx_encode_batch_dict_device, zlib, %d records of %.1f bytes on average behind a %d-byte chain dictionary "
                                  "(tools/bench_dict.py's), one write_all each" % (COUNT, total_in / COUNT, len(zdict)),
                      "input_bytes": total_in, "runs": records, "cost_against_level": versus(records),
                      "python_zlib_bytes": {"level_%d" % v: sum(zdict_size(r, v) for r in recs) for v in (6, 9)}}
    chain_d.close()
    if os.path.exists(args.out):          # (a model run made before this one stays)
        old = json.load(open(args.out))
        if "model_512k" in old:
            rec["model_512k"] = old["model_512k"]
            rec["model_512k_equals_device"] = {k: dev[k] == m for k, m in old["model_512k"].items() if k in dev}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
