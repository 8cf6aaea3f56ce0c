"""GPU box: the chained and the lazy parse through a chain dictionary on tools/bench_dict_encode.py's workload:
the same 4096 text records of about 1 KiB and the same 32 KiB dictionary, zlib, device-resident input and output, one
process.  lfx_encode_batch_dict_device with the default parse (§18's call), with LFX_LZ77_CHAIN and LFX_LZ77_LAZY at depths 1,
8 and 32 behind a chain dictionary, and lfx_encode_batch_device with LFX_LZ77_LAZY at depth 8 (the best a caller had without
the chain dictionary), all alternating.  Host clock around the blocking C call (it ends in a device synchronise), 3 warm-ups,
15 rounds; median and min - max of each; every round's streams are read back with python-zlib and compared with the records
after the clock stops; the phases of lfx_ctx_last_timing come from a second, untimed pass.  Writes
profiles/dict_chain_encode.json and prints it as one JSON line."""
import json
import os
import random
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_dict_encode import COUNT, ROUNDS, WARM, text  # noqa: E402

FIRST = 64          # the records the CPU model's figures are for (tests/test_dict_chain_model.py)


def main():
    import ctypes as C

    import numpy as np
    sys.path.insert(0, ROOT)
    import torch

    import libflate_amd
    from libflate_amd import _ffi

    ctx = libflate_amd.Context(0)
    zdict = text(32768, 1)
    plain_d = libflate_amd.Dictionary(zdict, ctx)
    chain_d = libflate_amd.Dictionary(zdict, ctx, chain=True)
    rng = random.Random(7)
    recs = [text(rng.randrange(900, 1200), 100 + i) for i in range(COUNT)]
    total_in = sum(len(r) for r in recs)
    d_in = torch.from_numpy(np.frombuffer(b"".join(recs), dtype=np.uint8).copy()).cuda()
    in_offs, pos = [], 0
    for r in recs:
        in_offs.append(pos)
        pos += len(r)
    in_lens = [len(r) for r in recs]
    base = _ffi.make_opts()
    caps = [(_ffi.lib().lfx_encode_dict_bound(n, C.byref(base), None) + 3) & ~3 for n in in_lens]
    out_offs, pos = [], 0
    for c in caps:
        out_offs.append(pos)
        pos += c
    d_out = torch.empty(pos, dtype=torch.uint8, device="cuda")

    # name → (dictionary, options)
    runs = {"dict_default": (plain_d, base)}
    for depth in (1, 8, 32):
        runs["dict_chain%d" % depth] = (chain_d, _ffi.make_opts(lz77_kind=_ffi.LZ77_CHAIN | depth << 8))
        runs["dict_lazy%d" % depth] = (chain_d, _ffi.make_opts(lz77_kind=_ffi.LZ77_LAZY | depth << 8))
    runs["plain_lazy8"] = (None, _ffi.make_opts(lz77_kind=_ffi.LZ77_LAZY | 8 << 8))

    def call(key):
        zd, opts = runs[key]
        return ctx.encode_batch_dict_device(_ffi.ZLIB, zd, d_in.data_ptr(), in_offs, in_lens, d_out.data_ptr(), out_offs, caps, opts)

    sizes, first = {}, {}

    def clock(key):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc, res = call(key)
        dt = time.perf_counter() - t0
        assert rc == 0 and all(st == 0 for st, _ in res)
        host = d_out.cpu().numpy().tobytes()
        for (st, ol), off, r in zip(res, out_offs, recs):
            z = zlib.decompressobj(zdict=zdict) if runs[key][0] is not None else zlib.decompressobj()
            assert z.decompress(host[off:off + ol]) + z.flush() == r
        sizes[key] = sum(ol for _, ol in res)
        first[key] = sum(ol for _, ol in res[:FIRST])
        return dt * 1e3

    for _ in range(WARM):
        for k in runs:
            clock(k)
    ts = {k: [] for k in runs}
    for _ in range(ROUNDS):
        for k in runs:
            ts[k].append(clock(k))
    ctx.enable_timing(True)
    phases = {}
    for k in runs:
        call(k)
        phases[k] = [(n, round(ms, 4)) for n, ms in ctx.last_timing()["phases"]]
    ctx.enable_timing(False)
    rec = {"tool": "tools/bench_dict_chain.py", "records": COUNT, "record_bytes_mean": round(total_in / COUNT, 1),
           "dictionary_bytes": len(zdict), "input_bytes": total_in,
           "model_bytes_per_record_first_%d" % FIRST: {"dict_default": 455.7, "dict_chain8": 432.2, "dict_lazy8": 431.4, "dict_lazy32": 411.8,
                                                        "plain_lazy8": 504.9},
           "method": "host clock around the blocking call, %d warm-ups, %d rounds, alternating; streams checked every round" % (WARM, ROUNDS)}
    for k in runs:
        med = statistics.median(ts[k])
        rec[k] = {"compressed_bytes": sizes[k], "compressed_bytes_per_record": round(sizes[k] / COUNT, 1),
                  "bytes_per_record_first_%d" % FIRST: round(first[k] / FIRST, 1), "ms_median": round(med, 4),
                  "ms_min": round(min(ts[k]), 4), "ms_max": round(max(ts[k]), 4), "records_per_s": round(COUNT / (med * 1e-3)),
                  "phase_lz77_chain_cand_ms": dict(phases[k]).get("lz77_chain_cand"), "phases_ms": phases[k]}
    plain_d.close()
    chain_d.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "dict_chain_encode.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
