"""GPU box: the stream encoder with and without a preset dictionary, next to another build of the package.

Two corpora: tools/bench_dict.py's 4096 text records of about 1 KiB with its 32 KiB dictionary, every record a zlib stream of
its own (one encoder, one write, finish), and 64 MiB of synth.text as ONE zlib stream in 8 KiB writes.  Rows: the stream encoder
without a dictionary, with one, and lfx_encode_dict_host on the same input (records: one call each; text: the 8 KiB schedule).
Host clock around the whole corpus, a device synchronise behind it; every round's output is inflated by python-zlib after the
clock stops (records: a sample of 64).

    python tools/bench_stream_dict.py [--other ROOT]

--other: the root of another checkout with a built package (the parent commit's).  Its dictionary-less rows run in processes
of their own, alternating with this build's: this, other, this, other — one session, the same machine, each process 1 warm-up
and ROUNDS rounds.  The claim to check: this build's dictionary-less rows lie inside the other build's own min - max.
Writes profiles/stream_dict_encode.json and prints it as one JSON line."""
import argparse
import io
import json
import os
import random
import statistics
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS, WARM = 5, 1
TEXT_BYTES, WRITE = 64 << 20, 8192


def worker(root, with_dict):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, root)
    import torch
    import libflate_amd as lfx                  # (of `root`, before bench_dict puts this checkout in front)
    from libflate_amd import _ffi
    import bench_dict
    import synth
    synth.build()
    ctx = lfx.Context(0)
    zdict = bench_dict.text(32768, 1)
    rng = random.Random(7)
    recs = [bench_dict.text(rng.randrange(900, 1200), 100 + i) for i in range(bench_dict.COUNT)]
    text = synth.text(TEXT_BYTES, seed=synth.SEED_BASE + 51).tobytes()
    views = [text[at:at + WRITE] for at in range(0, len(text), WRITE)]
    d = lfx.Dictionary(zdict, ctx) if with_dict else None
    sched = _ffi.make_schedule(WRITE)

    def stream_records(zd):
        out = []
        for r in recs:
            sink = io.BytesIO()
            e = lfx.zlib.Encoder.new(sink, context=ctx, zdict=zd) if zd is not None else lfx.zlib.Encoder.new(sink, context=ctx)
            e.write(r)
            e.finish()
            out.append(sink.getvalue())
        return out

    def stream_text(zd):
        sink = io.BytesIO()
        e = lfx.zlib.Encoder.new(sink, context=ctx, zdict=zd) if zd is not None else lfx.zlib.Encoder.new(sink, context=ctx)
        for v in views:
            e.write(v)
        e.finish()
        return [sink.getvalue()]
    rows = {"records_stream": (lambda: stream_records(None), recs, None), "text_stream": (lambda: stream_text(None), [text], None)}
    if with_dict:
        rows.update({
            "records_stream_dict": (lambda: stream_records(d), recs, zdict), "text_stream_dict": (lambda: stream_text(d), [text], zdict),
            "records_dict_host": (lambda: [ctx.encode_dict_host(_ffi.ZLIB, d, r) for r in recs], recs, zdict),
            "text_dict_host": (lambda: [ctx.encode_dict_host(_ffi.ZLIB, d, text, None, sched)], [text], zdict)})
    res = {}
    for name, (fn, plain, zd) in rows.items():
        ms = []
        for i in range(WARM + ROUNDS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            for k in range(0, len(out), max(1, len(out) // 64)):
                o = zlib.decompressobj(15, zdict=zd) if zd is not None else zlib.decompressobj(15)
                assert o.decompress(out[k]) + o.flush() == plain[k], (name, k)
            if i >= WARM:
                ms.append(dt)
        res[name] = {"ms": [round(x, 3) for x in ms], "out_bytes": sum(len(z) for z in out)}
    print("RESULT " + json.dumps(res), flush=True)


def spawn(root, with_dict):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", root] + (["--dict"] if with_dict else []),
                         capture_output=True, text=True, timeout=900)
    line = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
    assert out.returncode == 0 and line, (out.returncode, out.stdout[-400:], out.stderr[-800:])
    return json.loads(line[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", default=None)
    ap.add_argument("--worker", default=None)
    ap.add_argument("--dict", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.dict)
    runs = {"this": [], "other": []}
    for rep in range(2):                                 # this, other, this, other
        runs["this"].append(spawn(ROOT, rep == 0))
        if a.other:
            runs["other"].append(spawn(os.path.abspath(a.other), False))

    def fold(parts, name):
        ms = [x for p in parts if name in p for x in p[name]["ms"]]
        size = [p[name]["out_bytes"] for p in parts if name in p]
        return {"median_ms": round(statistics.median(ms), 3), "min_ms": min(ms), "max_ms": max(ms), "rounds": len(ms), "out_bytes": size[0]}
    report = {"rounds_per_process": ROUNDS, "warm_ups": WARM, "records": 4096, "text_bytes": TEXT_BYTES, "write": WRITE, "rows": {}}
    for name in runs["this"][0]:
        report["rows"][name] = fold(runs["this"], name)
    for name in ("records_stream", "text_stream"):
        if runs["other"]:
            o = report["rows"][name + "_other"] = fold(runs["other"], name)
            t = report["rows"][name]
            report["rows"][name]["inside_other_min_max"] = o["min_ms"] <= t["median_ms"] <= o["max_ms"]
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "stream_dict_encode.json"), "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
