"""GPU box: dynamic_huffman = 1 against LFX_HUFFMAN_AUTO on batches of small records, in one process.
tools/bench_dict.py's 4096 text records cut to about 64, 256 and 1024 bytes; zlib batch without a dictionary, with a plain one,
and with a chain dictionary plus LazyLz77Encoder(8).  §19's method: host clock around the blocking C call (it ends in a device
synchronise), 3 warm-ups, 15 rounds, the two calls alternating; median and min - max of each; every stream of both is inflated
by python-zlib afterwards; the phases of lfx_ctx_last_timing and the chosen forms come from a second, untimed pass.  python-zlib
levels 1 and 6 beside them (bytes only).  --corpus MIB: also one stream of so many MiB of the text through lfx_encode_device,
1 against 2.  Writes profiles/auto_blocks.json and prints it as one JSON line."""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import libflate_amd  # noqa: E402
from bench_dict import COUNT, ROUNDS, WARM, dev, text  # noqa: E402
from libflate_amd import _ffi  # noqa: E402


def inflate(z, zd):
    d = zlib.decompressobj(15, zdict=zd) if zd is not None else zlib.decompressobj(15)
    return d.decompress(z) + d.flush()


def pyz(recs, level, zd):
    total = 0
    for r in recs:
        co = zlib.compressobj(level, zlib.DEFLATED, 15, zdict=zd) if zd is not None else zlib.compressobj(level, zlib.DEFLATED, 15)
        total += len(co.compress(r) + co.flush())
    return total


def choices(ctx, nmax):
    buf, n = (C.c_uint8 * nmax)(), C.c_size_t(0)
    assert _ffi.lib().lfx_debug_block_choices(ctx.handle, buf, nmax, C.byref(n)) == 0
    got = list(buf[:min(n.value, nmax)])
    return {k: round(got.count(v) / max(len(got), 1), 4) for k, v in (("stored", 0), ("fixed", 1), ("dynamic", 2))}


def variant(ctx, recs, zd, zdict, kind):
    opts = {dh: _ffi.make_opts(dynamic_huffman=dh, lz77_kind=kind) for dh in (1, 2)}
    caps = [(_ffi.lib().lfx_encode_dict_bound(len(r), C.byref(opts[1]), None) + 3) & ~3 for r in recs]
    in_offs, out_offs, a, b = [], [], 0, 0
    for r, cap in zip(recs, caps):
        in_offs.append(a)
        out_offs.append(b)
        a += len(r)
        b += cap
    d_in, d_out = dev(b"".join(recs)), torch.empty(b, dtype=torch.uint8, device="cuda")
    lens = [len(r) for r in recs]

    def call(dh):
        rc, res = ctx.encode_batch_dict_device(_ffi.ZLIB, zd, d_in.data_ptr(), in_offs, lens, d_out.data_ptr(), out_offs, caps, opts[dh])
        assert rc == 0
        return res

    def clock(dh):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call(dh)
        return (time.perf_counter() - t0) * 1e3

    for _ in range(WARM):
        for dh in (1, 2):
            clock(dh)
    ts = {1: [], 2: []}
    for _ in range(ROUNDS):
        for dh in (1, 2):
            ts[dh].append(clock(dh))
    out = {}
    ctx.enable_timing(True)
    for dh in (1, 2):
        res = call(dh)
        phases = [(n, round(ms, 4)) for n, ms in ctx.last_timing()["phases"]]
        whole = d_out.cpu().numpy().tobytes()
        for r, o, (st, n) in zip(recs, out_offs, res):
            assert st == 0 and inflate(whole[o:o + n], zdict) == r
        med = statistics.median(ts[dh])
        out["dynamic_huffman_%d" % dh] = {
            "bytes_per_record": round(sum(n for _, n in res) / len(recs), 2), "ms_median": round(med, 4), "ms_min": round(min(ts[dh]), 4),
            "ms_max": round(max(ts[dh]), 4), "block_choose_ms": dict(phases).get("block_choose"), "phases_ms": phases}
        if dh == 2:
            out["dynamic_huffman_2"]["forms"] = choices(ctx, 2 * len(recs) + 16)
    ctx.enable_timing(False)
    out["python_zlib_1_bytes_per_record"] = round(pyz(recs, 1, zdict) / len(recs), 2)
    out["python_zlib_6_bytes_per_record"] = round(pyz(recs, 6, zdict) / len(recs), 2)
    return out


def corpus(ctx, mib):
    data = (text(1 << 20, 5) * mib)
    d_in = dev(data)
    cap = (_ffi.lib().lfx_encode_bound(len(data), None, None) + 3) & ~3
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    sched = _ffi.make_schedule(8192)
    out = {"MiB": mib}
    ts = {1: [], 2: []}
    lens = {}
    for it in range(WARM + ROUNDS):
        for dh in (1, 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lens[dh] = ctx.encode_device(_ffi.GZIP, d_in.data_ptr(), len(data), d_out.data_ptr(), cap, _ffi.make_opts(dynamic_huffman=dh), sched)
            if it >= WARM:
                ts[dh].append((time.perf_counter() - t0) * 1e3)
    for dh in (1, 2):
        out["dynamic_huffman_%d" % dh] = {"bytes": lens[dh], "ms_median": round(statistics.median(ts[dh]), 4),
                                          "ms_min": round(min(ts[dh]), 4), "ms_max": round(max(ts[dh]), 4)}
    out["forms"] = choices(ctx, 4096)
    import gzip
    assert gzip.decompress(d_out[:lens[2]].cpu().numpy().tobytes()) == data
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpus", type=int, default=0, help="MiB of text through lfx_encode_device as well (0: skip)")
    args = ap.parse_args()
    ctx = libflate_amd.Context(0)
    zdict = text(32768, 1)
    plain, chain = libflate_amd.Dictionary(zdict, ctx), libflate_amd.Dictionary(zdict, ctx, chain=True)
    rng = random.Random(7)
    full = [text(rng.randrange(900, 1200), 100 + i) for i in range(COUNT)]
    rec = {"tool": "tools/bench_auto.py", "records": COUNT, "dictionary_bytes": len(zdict),
           "method": "host clock around the blocking call, %d warm-ups, %d rounds, alternating; every stream inflated by python-zlib" % (WARM, ROUNDS),
           "sizes": {}}
    for size in (64, 256, 1024):
        recs = [r[:max(8, len(r) * size // 1024)] for r in full]
        rec["sizes"][str(size)] = {
            "record_bytes_mean": round(sum(len(r) for r in recs) / COUNT, 1),
            "no_dictionary": variant(ctx, recs, None, None, 0),
            "dictionary": variant(ctx, recs, plain, zdict, 0),
            "chain_dictionary_lazy_8": variant(ctx, recs, chain, zdict, _ffi.LZ77_LAZY | 8 << 8)}
    if args.corpus:
        rec["corpus"] = corpus(ctx, args.corpus)
    plain.close()
    chain.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "auto_blocks.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
