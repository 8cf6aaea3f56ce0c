"""The dictionary trainer on the GPU (lfx_dict_train_device): what training costs and what the dictionary buys.

  time   lfx_dict_train_device on records resident in HBM, wall clock around the blocking call, warm-up then timed rounds
         (median, min - max): 4096 x 1 KiB and 256 MiB (262144 x 1 KiB) of log lines, at 2, 8 and 32 KiB, segment 128; beside
         it the batch encode of the same 4096 records with the trained 32 KiB dictionary (lfx_encode_batch_packed_device)
  size   1024 held-out log lines through zlib.compress_batch(zdict=...): a dictionary trained on 4096 other lines against the
         first bytes of those lines, at 2, 8 and 32 KiB, with the default parse and with level 6 over a chain dictionary; and
         the same pair through Python's zlib at level 6 (the trainer's model needs no GPU for that one)

    python tools/bench_dict_train.py [--out profiles/dict_train.json] [--rounds 11] [--skip-large]
prints the JSON it writes."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
import zlib as pyzlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def timed(fn, warmup, rounds):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "rounds": rounds}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dict_train.json"))
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--skip-large", action="store_true")
    args = ap.parse_args()

    import __graft_entry__ as g
    g.build()
    import torch
    import libflate_amd as lfx
    from libflate_amd import _ffi
    import dict_train_cases as cases
    import dict_train_model as model

    ctx = lfx.Context(0)
    L = _ffi.lib()
    res = {"device": torch.cuda.get_device_name(0), "segment": 128, "time": {}, "size": {}}

    # ---- time: 1 KiB records cut from a run of log lines
    def records_1k(count, distinct):
        text = np.frombuffer(b"".join(cases.log_lines(distinct * 4, 41)), dtype=np.uint8)[:distinct * 1024]
        reps = (count + distinct - 1) // distinct
        return np.tile(text, reps)[:count * 1024]

    def train_case(name, count, distinct, warmup, rounds):
        buf = torch.from_numpy(records_1k(count, distinct).copy()).to("cuda")
        offs = (C.c_uint64 * count)(*range(0, count * 1024, 1024))
        lens = (C.c_uint64 * count)(*([1024] * count))
        out = torch.empty(32768, dtype=torch.uint8, device="cuda")
        got = C.c_uint64(0)
        torch.cuda.synchronize()
        row = {"records": count, "bytes": count * 1024}
        for size in (2048, 8192, 32768):
            def run():
                rc = L.lfx_dict_train_device(ctx.handle, buf.data_ptr(), count, offs, lens, size, 128, out.data_ptr(), 32768, C.byref(got))
                assert rc == 0, (rc, ctx.last_error())
            row["train_%dk" % (size // 1024)] = dict(timed(run, warmup, rounds), dict_len=got.value)
        res["time"][name] = row
        return buf, out[:got.value].clone()

    buf, d32 = train_case("4096x1KiB", 4096, 4096, 2, args.rounds)
    zdict = lfx.Dictionary(d32, ctx)
    offs, lens = list(range(0, 4096 * 1024, 1024)), [1024] * 4096
    cap = 4096 * int(L.lfx_encode_dict_bound(1024, None, None))
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    enc = lambda: ctx.encode_batch_packed_device(_ffi.ZLIB, buf.data_ptr(), offs, lens, d_out.data_ptr(), cap, zdict=zdict)
    res["time"]["4096x1KiB"]["batch_encode_zlib_dict32k"] = timed(enc, 2, args.rounds)
    del buf
    if not args.skip_large:
        train_case("262144x1KiB", 262144, 65536, 1, max(3, args.rounds // 3))

    # ---- size: held-out lines
    recs = cases.log_lines(4096 + 1024, 7)
    train, held = recs[:4096], recs[4096:]
    res["size"]["held_out"] = {"records": len(held), "raw_bytes": sum(map(len, held))}

    def py6(zd):
        total = 0
        for r in held:
            c = pyzlib.compressobj(6, zdict=zd) if zd else pyzlib.compressobj(6)
            total += len(c.compress(r) + c.flush())
        return total

    total = lambda streams: sum(map(len, streams))
    res["size"]["no_dictionary"] = {"batch_default": total(lfx.zlib.compress_batch(held, context=ctx)),
                                    "batch_level6": total(lfx.zlib.compress_batch(held, context=ctx, level=6)), "python_zlib6": py6(b"")}
    joined = b"".join(train)
    for size in (2048, 8192, 32768):
        trained = lfx.train_dictionary(train, size, 128, context=ctx)
        assert trained == model.train(train, size, 128), "the device's dictionary differs from the model's"
        row = {}
        for name, zd in (("trained", trained), ("first_bytes", joined[:size])):
            plain, chain = lfx.Dictionary(zd, ctx), lfx.Dictionary(zd, ctx, chain=True)
            s_def = lfx.zlib.compress_batch(held, zdict=plain, context=ctx)
            s_l6 = lfx.zlib.compress_batch(held, zdict=chain, context=ctx, level=6)
            assert lfx.zlib.decompress_batch(s_def, zdict=plain, context=ctx) == held
            assert lfx.zlib.decompress_batch(s_l6, zdict=chain, context=ctx) == held
            row[name] = {"dict_len": len(zd), "batch_default": total(s_def), "batch_level6": total(s_l6), "python_zlib6": py6(zd)}
        for k in ("batch_default", "batch_level6", "python_zlib6"):
            row["ratio_" + k] = round(row["trained"][k] / row["first_bytes"][k], 4)
        res["size"]["%dk" % (size // 1024)] = row

    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
