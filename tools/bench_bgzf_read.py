"""GPU box: lfx_bgzf_read_device against what a caller does today for bytes at a virtual offset, on the same device-resident
BGZF file, in one process.  The file: 256 MiB of synth.text as BGZF from encode_members(65280).  Cases: (a) one
4 KiB read, (b) 4096 random 64 KiB reads, (c) one read of the whole file, (d) size mode of (b).  Yardsticks, alternating with
the new call: lfx_decode_members_device of the whole file, and lfx_index_read_device on an index built with LFX_DEC_MULTI for
the same reads.  --yardstick-lib PATH: a liblfx.so built from the parent commit runs the yardsticks (two ctypes handles, one
context each); without it this tree's own.  Host clock around the blocking C call, 3 warm-ups, 15 rounds; median and min - max
of each; results are checked after the clock stops; the phases of lfx_ctx_last_timing come from a second, untimed pass.  Prints
one JSON line and writes it to --out (default profiles/r11_bgzf_read.json)."""
import argparse
import bisect
import ctypes as C
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

MIB, KIB = 1 << 20, 1 << 10
WARM, ROUNDS = 3, 15
u64 = C.c_uint64


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def stats(ts):
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--yardstick-lib", default=None)
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_bgzf_read.json"))
    a = ap.parse_args()
    L = _ffi.lib()
    ctx = libflate_amd.Context(0)
    h = ctx.handle
    if a.yardstick_lib:
        Y = C.CDLL(a.yardstick_lib)
        Y.lfx_ctx_new.restype = C.c_void_p
        Y.lfx_ctx_new.argtypes = [C.c_int, C.POINTER(C.c_int)]
        for name in ("lfx_decode_members_device", "lfx_decode_index_device", "lfx_index_read_device", "lfx_index_free"):
            getattr(Y, name).argtypes = getattr(L, name).argtypes
        Y.lfx_index_free.restype = None
        st = C.c_int(0)
        yh = Y.lfx_ctx_new(0, C.byref(st))
        assert yh and st.value == 0
    else:
        yctx = libflate_amd.Context(0)      # (held to the end of main: its handle dies with it)
        Y, yh = L, yctx.handle

    n = a.mib * MIB
    text = synth.text(n)
    d_text = torch.from_numpy(text).cuda()
    cap = L.lfx_encode_members_bound(n, _ffi.BGZF_MEMBER_SIZE, _ffi.MEMBERS_BGZF, None, None)
    d_file = torch.empty(cap, dtype=torch.uint8, device="cuda")
    rc, flen, count, members, msg = ctx.encode_members_device(d_text.data_ptr(), n, d_file.data_ptr(), cap, _ffi.BGZF_MEMBER_SIZE,
                                                              _ffi.MEMBERS_BGZF)
    assert rc == 0 and count == len(members), msg
    u_offs = [m[0] for m in members]
    voff = lambda u: (lambda i: members[i][2] << 16 | (u - members[i][0]))(bisect.bisect_right(u_offs, u) - 1)
    d_out = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_ref = torch.empty(n, dtype=torch.uint8, device="cuda")

    # the index of the yardstick (built once, untimed) and the whole-file decode
    idx = C.c_void_p(None)
    ol, used = u64(0), u64(0)
    assert Y.lfx_decode_index_device(yh, _ffi.GZIP, _ffi.DEC_MULTI, d_file.data_ptr(), flen, d_ref.data_ptr(), n, C.byref(ol), C.byref(used),
                                     1 << 20, C.byref(idx)) == 0 and ol.value == n
    assert torch.equal(d_ref, d_text)
    table = (_ffi.Member * (count + 2))()
    cnt = C.c_uint32(0)

    def members_fn():
        return Y.lfx_decode_members_device(yh, d_file.data_ptr(), flen, d_ref.data_ptr(), n, C.byref(ol), C.byref(used), table, count + 2,
                                           C.byref(cnt))

    rnd = random.Random(17)
    cases = {
        "a: one 4 KiB read": [(rnd.randrange(n - 4 * KIB), 4 * KIB)],
        "b: 4096 random 64 KiB reads": [(rnd.randrange(n - 64 * KIB), 64 * KIB) for _ in range(4096)],
        "c: one read of the whole file": [(0, n)],
    }
    results = []
    for name, reads in list(cases.items()) + [("d: size mode of (b)", cases["b: 4096 random 64 KiB reads"])]:
        k = len(reads)
        size_mode = name.startswith("d")
        arr = (_ffi.BgzfRead * k)()
        at, offs = 0, []
        for i, (u, ln) in enumerate(reads):
            arr[i].voff, arr[i].end_voff, arr[i].len, arr[i].out_off = voff(u), _ffi.VOFF_NONE, ln, at
            offs.append(at)
            at += ln
        assert at <= n or k > 1
        d_o = d_out if at <= n else torch.empty(at, dtype=torch.uint8, device="cuda")
        d_i = d_ref if at <= n else torch.empty(at, dtype=torch.uint8, device="cuda")
        res = (_ffi.BgzfResult * k)()
        decoded = u64(0)
        i_off = np.array([r[0] for r in reads], dtype=np.uint64)
        i_len = np.array([r[1] for r in reads], dtype=np.uint64)
        i_out = np.array(offs, dtype=np.uint64)
        i_got, i_st = np.zeros(k, dtype=np.uint64), np.zeros(k, dtype=np.int32)

        def read_fn():
            return L.lfx_bgzf_read_device(h, d_file.data_ptr(), 0, flen, k, arr, None if size_mode else d_o.data_ptr(), res, C.byref(decoded))

        def index_fn():
            return Y.lfx_index_read_device(yh, idx, d_file.data_ptr(), 0, flen, k, i_off.ctypes.data, i_len.ctypes.data, d_i.data_ptr(),
                                           i_out.ctypes.data, i_got.ctypes.data, i_st.ctypes.data)

        def check():
            assert all(res[i].status == 0 and res[i].out_len == reads[i][1] for i in range(k))
            if not size_mode:
                for i in ([0, k - 1] + random.Random(3).sample(range(k), min(k, 16))):
                    u, ln = reads[i]
                    assert torch.equal(d_o[offs[i]:offs[i] + ln], d_text[u:u + ln]), (name, i)
            assert not i_st.any() and i_got.tolist() == [r[1] for r in reads]

        for _ in range(WARM):
            read_fn(); index_fn(); members_fn()
        tr, ti, tm = [], [], []
        for _ in range(ROUNDS):
            t, rc = clock(read_fn); tr.append(t); assert rc == 0
            t, rc = clock(index_fn); ti.append(t); assert rc == 0
            t, rc = clock(members_fn); tm.append(t); assert rc == 0
            check()
        ctx.enable_timing(True)
        read_fn()
        phases = ctx.last_timing()
        ctx.enable_timing(False)
        split = {}
        for pn, ms in (phases or {}).get("phases", []):
            split[pn] = round(split.get(pn, 0.0) + ms, 4)
        # the context's timer holds 17 events: start, hop, plan and two per group of 4096 blocks, so the split covers the
        # first seven groups and undercounts `batch` and `gather` behind them
        groups = -(-decoded.value // 4096)
        results.append({"case": name, "reads": k, "bytes": at, "blocks_decoded": decoded.value, "bgzf_read_ms": stats(tr),
                        "index_read_ms": stats(ti), "decode_members_ms": stats(tm), "phases": split, "groups": groups,
                        "phases_cover_all_groups": groups <= 7})
    Y.lfx_index_free(idx)
    line = json.dumps({"bench": "bgzf_read", "file_mib": a.mib, "blocks": count, "file_bytes": flen, "yardstick_lib": bool(a.yardstick_lib),
                       "cases": results})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
