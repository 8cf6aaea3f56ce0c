"""GPU box: the seek index built while encoding (lfx_encode_index_device) against the encode alone
(lfx_encode_device) and against the encode followed by the decode-built index (lfx_decode_index_device on its output).
Three configurations: 256 MiB TEXT gzip S8K at a spacing of 1 MiB (the bench's cfg2 stream), the same stream at 64 KiB, and
128 MiB TEXT gzip S1 at 1 MiB.  Input and output resident in HBM; wall clock around the blocking calls, median of `--reps`
after one warm-up.  Every run's encoded bytes are compared with lfx_encode_device's after the clock has stopped, and 256
random reads through the index with the input.  A separate run with phase timers gives the phase split of the encode + index
call.  Prints one JSON line.

    python tools/bench_encode_index.py [--reps N] [--out FILE]"""
import argparse
import json
import os
import random
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
from libflate_amd.index import Index  # noqa: E402

MIB = 1 << 20


def timed(fn, reps, check=None):
    """median wall time of fn() over `reps` runs after one warm-up; check(result) runs on every run's result, warm-up included,
    after the clock has stopped"""
    r = fn()
    if check:
        check(r)
    ts, rs = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
        if check:
            check(r)
        rs.append(r)
    return statistics.median(ts), rs


def one_config(ctx, name, d_in, n, sched_write, spacing, reps):
    import ctypes as C
    opts, sched = _ffi.make_opts(), _ffi.make_schedule(sched_write)
    cap = (_ffi.lib().lfx_encode_bound(n, C.byref(opts), C.byref(sched)) + 3) & ~3
    d_ref = torch.empty(cap, dtype=torch.uint8, device="cuda")
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    d_dec = torch.empty(n + MIB, dtype=torch.uint8, device="cuda")
    t_enc, r_enc = timed(lambda: ctx.encode_device(_ffi.GZIP, d_in.data_ptr(), n, d_ref.data_ptr(), cap, opts, sched), reps)
    ol = r_enc[-1]
    ref = d_ref[:ol].clone()

    def enc_index():
        got, h = ctx.encode_index_device(_ffi.GZIP, d_in.data_ptr(), n, d_out.data_ptr(), cap, opts, sched, spacing)
        return got, Index(h, ctx)

    def same_bytes(r):          # (outside the timed region: the bytes of every run against lfx_encode_device's)
        assert r[0] == ol and torch.equal(d_out[:ol], ref), "lfx_encode_index_device wrote other bytes than lfx_encode_device"

    t_ei, r_ei = timed(enc_index, reps, same_bytes)
    idx = r_ei[-1][1]
    for _got, x in r_ei[:-1]:
        x.close()

    def enc_then_decode_index():
        got = ctx.encode_device(_ffi.GZIP, d_in.data_ptr(), n, d_ref.data_ptr(), cap, opts, sched)
        rc, dl, _u, h, msg = ctx.decode_index_device(_ffi.GZIP, d_ref.data_ptr(), got, d_dec.data_ptr(), n + MIB, spacing)
        assert rc == 0 and dl == n, msg
        return Index(h, ctx)

    t_ed, r_ed = timed(enc_then_decode_index, reps)
    info_d = r_ed[-1].info
    for x in r_ed:
        x.close()
    # 256 random reads through the index against the input
    rnd = random.Random(11)
    ranges = [(rnd.randrange(n), rnd.choice([1, 4096, 65536, 1 << 20])) for _ in range(256)]
    for (o, ln), g in zip(ranges, idx.read_many(ref, ranges)):
        assert torch.equal(g, d_in[o:o + ln]), (o, ln)
    # the phase split of one encode + index call
    ctx.enable_timing(True)
    got, h = ctx.encode_index_device(_ffi.GZIP, d_in.data_ptr(), n, d_out.data_ptr(), cap, opts, sched, spacing)
    tm = ctx.last_timing()
    ctx.enable_timing(False)
    Index(h, ctx).close()
    info = idx.info
    idx.close()
    return {"config": name, "in_bytes": n, "encoded_bytes": ol, "spacing": spacing, "encode_ms": t_enc * 1e3,
            "encode_index_ms": t_ei * 1e3, "encode_then_decode_index_ms": t_ed * 1e3, "encode_index_over_encode": t_ei / t_enc,
            "encode_then_decode_index_over_encode": t_ed / t_enc, "n_points": info["n_points"], "max_gap": info["max_gap"],
            "decode_built_n_points": info_d["n_points"], "decode_built_max_gap": info_d["max_gap"],
            "phases_ms": [(k, round(v, 4)) for k, v in (tm["phases"] if tm else [])]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_encode_index.json"))
    a = ap.parse_args()
    ctx = libflate_amd.Context(0)
    plain = synth.text(256 * MIB)
    d_in = torch.from_numpy(np.ascontiguousarray(plain)).cuda()
    del plain
    out = {"tool": "bench_encode_index", "reps": a.reps, "configs": []}
    out["configs"].append(one_config(ctx, "text256_gzip_s8k_1m", d_in, d_in.numel(), 8192, 1 * MIB, a.reps))
    out["configs"].append(one_config(ctx, "text256_gzip_s8k_64k", d_in, d_in.numel(), 8192, 64 << 10, a.reps))
    out["configs"].append(one_config(ctx, "text128_gzip_s1_1m", d_in[:128 * MIB], 128 * MIB, 0, 1 * MIB, a.reps))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
