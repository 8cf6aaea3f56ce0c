"""GPU box: the multi-member gzip decode (lfx_decode_members_device) against the sequential member loop
(lfx_decode_device with LFX_DEC_MULTI) and against the batch decoder given the members' offsets (lfx_decode_batch_device, the
ceiling), on the same device bytes, in one process.  Two inputs of 4096 members x 64 KiB TEXT: the concatenated output of
one lfx_encode_batch_device call, and python-zlib members with a BGZF `BC` extra field (plus BGZF's empty EOF member).
Wall clock around the blocking calls, input and output resident in HBM; GB/s of output bytes.  Every output is compared
with the input.  Prints one JSON line."""
import ctypes as C
import json
import os
import statistics
import struct
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

COUNT, SIZE = 4096, 64 << 10
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def batch_encoded(ctx, d_plain):
    L = _ffi.lib()
    opts, sched = _ffi.make_opts(), _ffi.make_schedule(0)
    bound = (L.lfx_encode_bound(SIZE, C.byref(opts), C.byref(sched)) + 3) & ~3
    d_streams = torch.zeros(COUNT * bound, dtype=torch.uint8, device="cuda")
    in_off = np.arange(COUNT, dtype=np.uint64) * np.uint64(SIZE)
    in_len = np.full(COUNT, SIZE, dtype=np.uint64)
    out_off = np.arange(COUNT, dtype=np.uint64) * np.uint64(bound)
    out_cap = np.full(COUNT, bound, dtype=np.uint64)
    out_len = np.zeros(COUNT, dtype=np.uint64)
    status = np.zeros(COUNT, dtype=np.int32)
    rc = L.lfx_encode_batch_device(ctx.handle, _ffi.GZIP, C.byref(opts), C.byref(sched), COUNT, d_plain.data_ptr(), in_off.ctypes.data,
                                   in_len.ctypes.data, d_streams.data_ptr(), out_off.ctypes.data, out_cap.ctypes.data,
                                   out_len.ctypes.data, status.ctypes.data)
    assert rc == 0 and not status.any(), ctx.last_error()
    host = d_streams.cpu().numpy()
    return [host[i * bound:i * bound + int(out_len[i])].tobytes() for i in range(COUNT)]


def bgzf_members(plain):
    out = []
    for i in range(COUNT):
        raw = plain[i * SIZE:(i + 1) * SIZE]
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = co.compress(raw) + co.flush()
        size = 18 + len(body) + 8
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<HBBHH", 6, 66, 67, 2, size - 1) + body +
                   struct.pack("<II", zlib.crc32(raw), len(raw)))
    return out


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts), statistics.median(ts)


def measure(ctx, name, members, extra, d_plain, reps):
    L = _ffi.lib()
    data = b"".join(members) + extra
    n, total = len(data), COUNT * SIZE
    d_in = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    d_out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    res = {}

    def members_call():
        res["m"] = ctx.decode_members_device(d_in.data_ptr(), n, d_out.data_ptr(), total, max_members=COUNT + 1)
    members_call()
    rc, ol, used, table, msg = res["m"]
    ok_members = rc == 0 and ol == total and used == n and len(table) == COUNT + (1 if extra else 0) and torch.equal(d_out, d_plain)
    m_best, m_med = timed(members_call, reps)
    ctx.enable_timing(True)
    members_call()
    phases = {k: round(v, 4) for k, v in (ctx.last_timing() or {"phases": []})["phases"]}
    ctx.enable_timing(False)

    d_out.zero_()

    def multi_call():
        res["s"] = ctx.decode_device(_ffi.GZIP, d_in.data_ptr(), n, d_out.data_ptr(), total, flags=_ffi.DEC_MULTI)
    s_best, s_med = timed(multi_call, 2)
    ok_multi = res["s"][:3] == (0, total, n) and torch.equal(d_out, d_plain)

    d_out.zero_()
    in_off = np.array([m[0] for m in table[:COUNT]], dtype=np.uint64)
    in_len = np.array([m[1] for m in table[:COUNT]], dtype=np.uint64)
    out_off = np.arange(COUNT, dtype=np.uint64) * np.uint64(SIZE)
    out_cap = np.full(COUNT, SIZE, dtype=np.uint64)
    out_len = np.zeros(COUNT, dtype=np.uint64)
    status = np.zeros(COUNT, dtype=np.int32)

    def batch_call():
        res["b"] = L.lfx_decode_batch_device(ctx.handle, _ffi.GZIP, COUNT, d_in.data_ptr(), in_off.ctypes.data, in_len.ctypes.data,
                                             d_out.data_ptr(), out_off.ctypes.data, out_cap.ctypes.data, out_len.ctypes.data,
                                             status.ctypes.data)
    b_best, b_med = timed(batch_call, reps)
    ok_batch = res["b"] == 0 and not status.any() and torch.equal(d_out, d_plain)
    gbps = lambda t: round(total / t / 1e9, 3)   # noqa: E731
    return {"input": name, "compressed_bytes": n, "output_bytes": total,
            "members_device": {"GBps": gbps(m_best), "ms": round(m_best * 1e3, 3), "median_ms": round(m_med * 1e3, 3),
                               "ok": bool(ok_members), "phases_ms": phases},
            "sequential_multi": {"GBps": gbps(s_best), "ms": round(s_best * 1e3, 3), "median_ms": round(s_med * 1e3, 3),
                                 "ok": bool(ok_multi)},
            "batch_known_offsets": {"GBps": gbps(b_best), "ms": round(b_best * 1e3, 3), "median_ms": round(b_med * 1e3, 3),
                                    "ok": bool(ok_batch)},
            "members_vs_sequential": round(s_best / m_best, 1), "members_vs_batch": round(b_best / m_best, 3)}


def main():
    reps = int(os.environ.get("BENCH_MEMBERS_REPS", "5"))
    ctx = libflate_amd.Context(0)
    plain = synth.text(COUNT * SIZE, seed=synth.SEED_BASE + 7)
    d_plain = torch.from_numpy(plain).cuda()
    rows = [measure(ctx, "lfx_encode_batch_device members, concatenated", batch_encoded(ctx, d_plain), b"", d_plain, reps),
            measure(ctx, "python-zlib level 6 BGZF members + EOF member", bgzf_members(plain.tobytes()), BGZF_EOF, d_plain, reps)]
    print(json.dumps({"workload": "gzip multi-member decode: %d members x %d KiB TEXT, resident in HBM" % (COUNT, SIZE >> 10),
                      "unit": "GB/s of output", "runs": rows}), flush=True)


if __name__ == "__main__":
    main()
