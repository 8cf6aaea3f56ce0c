"""GPU box: block_merge = 0 against 1, in one process.  Two corpora — bench.py's text (tools/synth.py) and a
mixed one built here: text ‖ random ‖ low-entropy ‖ text sections of unequal lengths — at block_size 64 KiB, 256 KiB and 1 MiB,
with the default parse and with level=6, 8192-byte writes, gzip.  §19's method: host clock around the blocking C call (it ends
in a device synchronise), 3 warm-ups, 9 rounds, the two calls alternating; median and min - max of each; both outputs are
inflated by python-zlib afterwards; the block_merge phase of lfx_ctx_last_timing and the share of candidates absorbed
(lfx_debug_block_merges) come from a second, untimed pass.  python-zlib level 6 on the same bytes beside them (size only).
No ratio or time is promised: the table says what was measured, also where the merge does not pay.
Writes profiles/block_merge.json and prints it as one JSON line.  --mib N: the size of each corpus (default 32)."""
import argparse
import ctypes as C
import gzip
import json
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import libflate_amd  # noqa: E402
import synth  # noqa: E402
from libflate_amd import _ffi  # noqa: E402

WARM, ROUNDS = 3, 9


def mixed(n):
    """text ‖ random ‖ low-entropy ‖ text ..., sections of 100 KiB to 3 MiB (seeded), cut to n bytes"""
    rng = np.random.RandomState(24)
    parts, total, k = [], 0, 0
    while total < n:
        size = int(rng.randint(100 << 10, 3 << 20))
        kind = k % 4
        if kind == 1:
            part = rng.randint(0, 256, size=size, dtype=np.uint8)
        elif kind == 2:
            part = synth.lowent(size, seed=synth.SEED_BASE + 50 + k)
        else:
            part = synth.text(size, seed=synth.SEED_BASE + 60 + k)
        parts.append(np.asarray(part, dtype=np.uint8))
        total += size
        k += 1
    return np.concatenate(parts)[:n].tobytes()


def absorbed_share(ctx, nmax=1 << 16):
    buf, n = (C.c_uint32 * nmax)(), C.c_size_t(0)
    assert _ffi.lib().lfx_debug_block_merges(ctx.handle, buf, nmax, C.byref(n)) == 0
    heads = list(buf[:min(n.value, nmax)])
    return {"blocks": len(heads), "absorbed": sum(1 for i, h in enumerate(heads) if h != i),
            "share": round(sum(1 for i, h in enumerate(heads) if h != i) / max(len(heads), 1), 4)}


def variant(ctx, data, d_in, block_size, kind):
    sched = _ffi.make_schedule(8192)
    opts = {bm: _ffi.make_opts(block_size=block_size, lz77_kind=kind, block_merge=bm, mtime=0) for bm in (0, 1)}
    cap = (_ffi.lib().lfx_encode_bound(len(data), C.byref(opts[0]), C.byref(sched)) + 3) & ~3
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")

    def call(bm):
        return ctx.encode_device(_ffi.GZIP, d_in.data_ptr(), len(data), d_out.data_ptr(), cap, opts[bm], sched)

    ts, lens = {0: [], 1: []}, {}
    for it in range(WARM + ROUNDS):
        for bm in (0, 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lens[bm] = call(bm)
            if it >= WARM:
                ts[bm].append((time.perf_counter() - t0) * 1e3)
    out = {}
    ctx.enable_timing(True)
    for bm in (0, 1):
        n = call(bm)
        phases = [(name, round(ms, 4)) for name, ms in ctx.last_timing()["phases"]]
        assert gzip.decompress(d_out[:n].cpu().numpy().tobytes()) == data
        out["block_merge_%d" % bm] = {"bytes": n, "ms_median": round(statistics.median(ts[bm]), 4), "ms_min": round(min(ts[bm]), 4),
                                      "ms_max": round(max(ts[bm]), 4), "block_merge_ms": dict(phases).get("block_merge"),
                                      "huffman_merged_ms": dict(phases).get("huffman_merged"), "phases_ms": phases}
        if bm == 1:
            out["block_merge_1"]["candidates"] = absorbed_share(ctx)
    ctx.enable_timing(False)
    out["bytes_saved_share"] = round(1 - out["block_merge_1"]["bytes"] / out["block_merge_0"]["bytes"], 5)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=32)
    args = ap.parse_args()
    n = args.mib << 20
    ctx = libflate_amd.Context(0)
    rec = {"tool": "tools/bench_merge.py", "corpus_MiB": args.mib, "format": "gzip", "write_size": 8192,
           "method": "host clock around the blocking call, %d warm-ups, %d rounds, alternating; both outputs inflated by python-zlib" % (WARM, ROUNDS),
           "corpora": {}}
    for name, data in (("text", synth.text(n).tobytes()), ("mixed", mixed(n))):
        d_in = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda")
        co = zlib.compressobj(6, zlib.DEFLATED, 31)
        entry = {"bytes": len(data), "python_zlib_6_bytes": len(co.compress(data) + co.flush()), "parses": {}}
        for parse, kind in (("default", 0), ("level_6", _ffi.LZ77_LEVEL | 6 << 8)):
            entry["parses"][parse] = {str(bs >> 10) + "KiB": variant(ctx, data, d_in, bs, kind) for bs in (64 << 10, 256 << 10, 1 << 20)}
        rec["corpora"][name] = entry
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "block_merge.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
