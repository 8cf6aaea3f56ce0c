"""GPU box: the seek index (lfx_decode_index_device / lfx_index_read_device).  Build time against
lfx_decode_device on three streams (256 MiB TEXT gzip S8K — the bench's cfg2 stream —, 128 MiB gzip S1, 128 MiB python-zlib
level 6), the export size, 4096 random 64 KiB reads in one call (GB/s delivered and GB/s decoded), the latency of one 4 KiB
read, and a full decode plus a slice for comparison.  Input and output resident in HBM; wall clock around the blocking calls
(median of `--reps`).  Every read is compared with the decoded bytes.  Prints one JSON line.

    python tools/bench_index.py [--spacing BYTES] [--reps N] [--out FILE]"""
import argparse
import json
import os
import random
import statistics
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import libflate_amd  # noqa: E402
import synth  # noqa: E402
from libflate_amd import _ffi  # noqa: E402
from libflate_amd.index import Index  # noqa: E402

MIB = 1 << 20


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), r


def one_stream(ctx, name, fmt, comp, plain_len, spacing, reps):
    n = len(comp)
    d_in = torch.from_numpy(np.frombuffer(comp, dtype=np.uint8).copy()).cuda()
    cap = plain_len + MIB
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    t_dec, r = timed(lambda: ctx.decode_device(fmt, d_in.data_ptr(), n, d_out.data_ptr(), cap), reps)
    assert r[0] == 0 and r[1] == plain_len, r
    ref = d_out[:plain_len].clone()
    handles = []

    def build():
        rc, ol, _u, h, msg = ctx.decode_index_device(fmt, d_in.data_ptr(), n, d_out.data_ptr(), cap, spacing)
        assert rc == 0 and ol == plain_len, msg
        handles.append(Index(h, ctx))
        return handles[-1]

    t_build, idx = timed(build, reps)
    assert torch.equal(d_out[:plain_len], ref)
    info = idx.info
    res = {"stream": name, "in_bytes": n, "out_bytes": plain_len, "decode_ms": t_dec * 1e3, "build_ms": t_build * 1e3,
           "build_over_decode": t_build / t_dec, "n_points": info["n_points"], "max_gap": info["max_gap"],
           "export_bytes": info["export_bytes"]}
    # 4096 random 64 KiB reads in one call
    rnd = random.Random(5)
    K, L = 4096, 64 << 10
    offs = [rnd.randrange(plain_len - L) for _ in range(K)]
    d_r = torch.empty(K * L, dtype=torch.uint8, device="cuda")
    oo = [i * L for i in range(K)]
    t_reads, rr = timed(lambda: ctx.index_read_device(idx._h, d_in.data_ptr(), 0, n, offs, [L] * K, d_r.data_ptr(), oo), reps)
    assert rr[0] == 0, rr[3]
    for i in range(0, K, 97):
        assert torch.equal(d_r[i * L:(i + 1) * L], ref[offs[i]:offs[i] + L])
    # bytes decoded: from each touched point to the furthest end a read needs in its segment
    pts = [p[2] for p in idx.points]
    need = {}
    import bisect
    for o in offs:
        for s in range(bisect.bisect_right(pts, o) - 1, bisect.bisect_right(pts, o + L - 1)):
            need[s] = max(need.get(s, 0), min(o + L, pts[s + 1] if s + 1 < len(pts) else plain_len) - pts[s])
    decoded = sum(need.values())
    res.update({"reads_4096x64k_ms": t_reads * 1e3, "reads_gbps_delivered": K * L / t_reads / 1e9,
                "reads_gbps_decoded": decoded / t_reads / 1e9})
    # one 4 KiB read
    o1 = plain_len // 2 + 12345
    d_1 = torch.empty(4096, dtype=torch.uint8, device="cuda")
    t_one, r1 = timed(lambda: ctx.index_read_device(idx._h, d_in.data_ptr(), 0, n, [o1], [4096], d_1.data_ptr(), [0]), reps)
    assert r1[0] == 0 and torch.equal(d_1, ref[o1:o1 + 4096])
    # full decode plus a slice of the same 4 KiB
    d_full = torch.empty(cap, dtype=torch.uint8, device="cuda")

    def full():
        ctx.decode_device(fmt, d_in.data_ptr(), n, d_full.data_ptr(), cap)
        return d_full[o1:o1 + 4096].clone()

    t_full, _ = timed(full, reps)
    res.update({"read_4k_ms": t_one * 1e3, "full_decode_slice_ms": t_full * 1e3})
    for h in handles:
        h.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spacing", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = libflate_amd.Context(0)
    out = {"tool": "bench_index", "spacing": a.spacing, "reps": a.reps, "streams": []}
    opts = _ffi.make_opts()
    plain = synth.text(256 * MIB).tobytes()
    cfg2 = ctx.encode_host(_ffi.GZIP, plain, opts, _ffi.make_schedule(8192))
    out["streams"].append(one_stream(ctx, "text256_gzip_s8k", _ffi.GZIP, cfg2, len(plain), a.spacing, a.reps))
    del cfg2
    half = plain[:128 * MIB]
    s1 = ctx.encode_host(_ffi.GZIP, half, opts, _ffi.make_schedule(0))
    out["streams"].append(one_stream(ctx, "text128_gzip_s1", _ffi.GZIP, s1, len(half), a.spacing, a.reps))
    del s1
    pz = zlib.compress(half, 6)
    out["streams"].append(one_stream(ctx, "text128_pyzlib6", _ffi.ZLIB, pz, len(half), a.spacing, a.reps))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
