"""GPU: the encode's host side in stages (libflate_amd/csrc/lfx_encode.cpp) — every kernel selection
encode_prepare can make, the shared steps (match fallback wrapper, pack, the side-stream zero fill, Plan::append, the upload
shadows) through every entry point of ONE context back to back, and the phase stamps.  Byte-exact against the oracle (BGZF: the
model of tests/test_members_encode_abi.py)."""
import ctypes as C
import io
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_parity import ctx, ffi, lfx, synth  # noqa: F401  (fixtures)
from test_members_encode_abi import model_bgzf, model_plain, words_text

KIB, MIB = 1 << 10, 1 << 20


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def _dev(torch, data):
    a = np.frombuffer(bytes(data), dtype=np.uint8).copy() if len(data) else np.zeros(4, dtype=np.uint8)
    return torch.from_numpy(a).to("cuda")


def encode_device(c, ffi, torch, fmt, data, write_size=8192, cap=None):
    """lfx_encode_device on device buffers → the stream (raises as Context.encode_device does)"""
    opts, sched = ffi.make_opts(), ffi.make_schedule(write_size)
    if cap is None:
        cap = (ffi.lib().lfx_encode_bound(len(data), C.byref(opts), C.byref(sched)) + 3) & ~3
    d_in = _dev(torch, data)
    d_out = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    n = c.encode_device(fmt, d_in.data_ptr(), len(data), d_out.data_ptr(), cap, opts, sched)
    whole = d_out.cpu().numpy().tobytes()
    assert whole[cap:] == b"\xA5" * 64, "bytes behind cap were written"
    return whole[:n]


def context_with(lfx, **env):
    """a fresh context: the LFX_* diagnostics switches are read once, when a context is created"""
    before = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return lfx.Context(0)
    finally:
        for k, v in before.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


# ---------------------------------------------------------------------------------------------- case 1
@pytest.fixture(scope="module")
def inputs_512k(synth):
    """512 KiB: 13 parse workgroups (more than 8: the XCD order with its empty slots is live), segments of 32 Ki positions"""
    text = synth.text(512 * KIB).tobytes()
    rnd = np.random.RandomState(11).randint(0, 256, size=448 * KIB, dtype=np.uint8)
    rnd[100000:228000] = 0x41                       # a long run
    rnd[300000:364000:2] = 0x42                     # half run, half noise
    return {"text": text, "mixed": synth.text(64 * KIB).tobytes() + rnd.tobytes()}


@pytest.fixture(scope="module")
def want_512k(oracle, ffi, inputs_512k):
    return {(name, fmt): oracle.encode(fmt, data, write_size=8192) for name, data in inputs_512k.items() for fmt in (ffi.GZIP, ffi.ZLIB, ffi.DEFLATE)}


@pytest.mark.parametrize("env", [{}, {"LFX_MATCH_V1": "1"}, {"LFX_HIST_SEPARATE": "1"}],
                         ids=["default", "match_v1", "hist_separate"])
def test_kernel_selections_at_512k(lfx, ffi, torch, inputs_512k, want_512k, env):
    c = context_with(lfx, **env)
    for name, data in inputs_512k.items():
        for fmt in (ffi.GZIP, ffi.ZLIB, ffi.DEFLATE):
            assert encode_device(c, ffi, torch, fmt, data) == want_512k[(name, fmt)], (env, name, fmt)
    assert c.match_fallbacks() == 0


# ---------------------------------------------------------------------------------------------- case 2
def test_1024_segments_at_32m(lfx, ffi, torch, oracle, synth):
    """32 MiB: 1024 segments of 32 Ki positions on 256 CUs, four per CU, through lfx_match7 and its resolver"""
    data = synth.text(32 * MIB).tobytes()
    want = oracle.encode(oracle.GZIP, data, write_size=8192)
    one = encode_device(lfx.Context(0), ffi, torch, ffi.GZIP, data)
    assert one == want


# ---------------------------------------------------------------------------------------------- case 3
def test_every_entry_point_in_one_context(lfx, ffi, torch, oracle, synth):
    c = lfx.Context(0)
    L = ffi.lib()
    first = synth.text(70000).tobytes()
    want_first = oracle.encode(oracle.GZIP, first, write_size=8192)
    # one-shot, device and host
    assert encode_device(c, ffi, torch, ffi.GZIP, first) == want_first
    assert c.encode_host(ffi.GZIP, first, ffi.make_opts(), ffi.make_schedule(8192)) == want_first
    # a batch of three unequal streams
    bufs = [b"", first[:1], first]
    opts, sched = ffi.make_opts(), ffi.make_schedule(8192)
    in_len = np.array([len(b) for b in bufs], dtype=np.uint64)
    in_off = np.array([0, 0, 1], dtype=np.uint64)
    d_in = _dev(torch, first[:1] + first)
    out_cap = np.array([(L.lfx_encode_bound(len(b), C.byref(opts), C.byref(sched)) + 3) & ~3 for b in bufs], dtype=np.uint64)
    out_off = np.concatenate(([0], np.cumsum(out_cap)[:-1])).astype(np.uint64)
    d_out = torch.full((int(out_cap.sum()),), 0xAA, dtype=torch.uint8, device="cuda")
    out_len, status = np.zeros(3, dtype=np.uint64), np.zeros(3, dtype=np.int32)
    rc = L.lfx_encode_batch_device(c.handle, ffi.ZLIB, C.byref(opts), C.byref(sched), 3, d_in.data_ptr(), in_off.ctypes.data,
                                   in_len.ctypes.data, d_out.data_ptr(), out_off.ctypes.data, out_cap.ctypes.data, out_len.ctypes.data,
                                   status.ctypes.data)
    assert rc == 0 and not status.any(), (rc, c.last_error())
    got = d_out.cpu().numpy()
    for i, b in enumerate(bufs):
        assert got[int(out_off[i]):int(out_off[i]) + int(out_len[i])].tobytes() == oracle.encode(oracle.ZLIB, b, write_size=8192), i
    # members, plain and BGZF, over the same bytes
    data = words_text(10000, seed=4)
    for flags, (want, table) in ((0, model_plain(oracle, data, 4096)), (ffi.MEMBERS_BGZF, model_bgzf(oracle, data, 4096)[:2])):
        cap = L.lfx_encode_members_bound(len(data), 4096, flags, None, None)
        d_m = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        rc, n, count, members, msg = c.encode_members_device(_dev(torch, data).data_ptr(), len(data), d_m.data_ptr(), cap, 4096, flags)
        assert rc == ffi.OK, msg
        assert d_m.cpu().numpy().tobytes()[:n] == want and members == table and count == len(table)
    # (the BGZF layout rewrote block types on the device: the block table's upload shadow must not be trusted after it)
    assert encode_device(c, ffi, torch, ffi.GZIP, first) == want_first
    # shard prepare / emit as a single, last shard
    info = ffi.ShardInfo()
    d_first = _dev(torch, first)
    rc = L.lfx_encode_shard_prepare(c.handle, ffi.GZIP, C.byref(opts), C.byref(sched), d_first.data_ptr(), len(first), 1, 1, C.byref(info))
    assert rc == 0, c.last_error()
    hdr_len = L.lfx_container_header_len(ffi.GZIP, C.byref(opts))
    from libflate_amd import sharded
    start_bits, check, total_n = sharded.layout([(info.total_bits, info.n_bytes, info.crc32, info.adler32)], hdr_len, ffi.GZIP)
    cap = len(first) + len(first) // 4 + 65536
    d_s = torch.empty(cap, dtype=torch.uint8, device="cuda")
    m = C.c_uint64(0)
    rc = L.lfx_encode_shard_emit(c.handle, start_bits[0], check, total_n, d_s.data_ptr(), cap, C.byref(m))
    assert rc == 0, c.last_error()
    assert sharded.assemble([d_s[:m.value].cpu().numpy().tobytes()], start_bits) == want_first
    # the stream encoder, bytes mode, a flush in the middle
    sink = io.BytesIO()
    se = lfx.zlib.Encoder.new(sink, c)
    oe = oracle.Encoder(oracle.ZLIB)
    for part in (first[:30000], None, first[30000:]):
        if part is None:
            se.flush(); oe.flush()
        else:
            se.write(part); oe.write(part)
    se.finish()
    assert sink.getvalue() == oe.finish()
    assert encode_device(c, ffi, torch, ffi.GZIP, first) == want_first


# ---------------------------------------------------------------------------------------------- case 4
def test_capacity_one_byte_short_leaves_no_fill_pending(lfx, ffi, torch, oracle, synth):
    c = lfx.Context(0)
    L = ffi.lib()
    data = synth.text(200000).tobytes()
    # one-shot: one byte less than the stream needs (capacities are used in whole dwords: at most len(want) - 1 of them count)
    want = oracle.encode(oracle.GZIP, data, write_size=8192)
    opts, sched = ffi.make_opts(), ffi.make_schedule(8192)
    full = (L.lfx_encode_bound(len(data), C.byref(opts), C.byref(sched)) + 3) & ~3
    d_in = _dev(torch, data)
    d_out = torch.full((full,), 0xA5, dtype=torch.uint8, device="cuda")
    assert c.encode_device(ffi.GZIP, d_in.data_ptr(), len(data), d_out.data_ptr(), full, opts, sched) == len(want)
    with pytest.raises(ffi.LfxError) as ei:
        c.encode_device(ffi.GZIP, d_in.data_ptr(), len(data), d_out.data_ptr(), len(want) - 1, opts, sched)
    assert ei.value.status == ffi.E_NOSPACE
    n = c.encode_device(ffi.GZIP, d_in.data_ptr(), len(data), d_out.data_ptr(), full, opts, sched)
    assert d_out.cpu().numpy().tobytes()[:n] == want
    # members
    mdata = words_text(10000, seed=4)
    mwant, table = model_plain(oracle, mdata, 4096)
    cap = L.lfx_encode_members_bound(len(mdata), 4096, 0, None, None)
    d_min = _dev(torch, mdata)
    d_m = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda")
    rc, n, count, members, msg = c.encode_members_device(d_min.data_ptr(), len(mdata), d_m.data_ptr(), cap, 4096)
    assert rc == ffi.OK and n == len(mwant), msg
    rc, n, count, members, msg = c.encode_members_device(d_min.data_ptr(), len(mdata), d_m.data_ptr(), len(mwant) - 1, 4096)
    assert rc == ffi.E_NOSPACE and n == 0
    rc, n, count, members, msg = c.encode_members_device(d_min.data_ptr(), len(mdata), d_m.data_ptr(), cap, 4096)
    assert rc == ffi.OK and d_m.cpu().numpy().tobytes()[:n] == mwant and members == table


# ---------------------------------------------------------------------------------------------- case 5
# The phase names of one-shot gzip, a batch and a members call at timing levels 1 and 6, as recorded from commit 2eacdfd (the
# commit before the encode's host side was split into stages) for exactly these calls.
PHASES_2EACDFD = {
    ("oneshot", 1): ["upload", "lz77_match", "lz77_parse", "histogram", "huffman", "checksum", "memset_out", "pack", "frame"],
    ("batch", 1): ["upload", "lz77_match", "lz77_parse", "histogram", "huffman", "checksum", "pack", "frame"],
    ("members", 1): ["upload", "lz77_match", "lz77_parse", "histogram", "huffman", "members_layout", "checksum", "pack", "frame"],
    ("oneshot", 6): ["upload", "lz77_cand", "lz77_resolve", "lz77_walk", "lz77_chain", "histogram", "huffman", "checksum", "memset_out", "pack",
                     "frame"],
    ("batch", 6): ["upload", "lz77_cand", "lz77_resolve", "lz77_walk", "lz77_chain", "histogram", "huffman", "checksum", "pack", "frame"],
    ("members", 6): ["upload", "lz77_cand", "lz77_resolve", "lz77_walk", "lz77_chain", "histogram", "huffman", "members_layout", "checksum",
                     "pack", "frame"],
}


@pytest.mark.parametrize("level", [1, 6])
def test_phase_lists_are_the_parents(lfx, ffi, torch, synth, level):
    c = lfx.Context(0)
    L = ffi.lib()
    c.enable_timing(level)
    data = synth.text(300000).tobytes()
    names = lambda: [k for k, _ in c.last_timing()["phases"]]
    encode_device(c, ffi, torch, ffi.GZIP, data)
    assert names() == PHASES_2EACDFD[("oneshot", level)]
    opts, sched = ffi.make_opts(), ffi.make_schedule(8192)
    sizes = [0, 1, 70000]
    in_len, in_off = np.array(sizes, dtype=np.uint64), np.array([0, 0, 1], dtype=np.uint64)
    out_cap = np.array([(L.lfx_encode_bound(n, C.byref(opts), C.byref(sched)) + 3) & ~3 for n in sizes], dtype=np.uint64)
    out_off = np.concatenate(([0], np.cumsum(out_cap)[:-1])).astype(np.uint64)
    d_in = _dev(torch, data)
    d_out = torch.zeros(int(out_cap.sum()), dtype=torch.uint8, device="cuda")
    out_len, status = np.zeros(3, dtype=np.uint64), np.zeros(3, dtype=np.int32)
    rc = L.lfx_encode_batch_device(c.handle, ffi.GZIP, C.byref(opts), C.byref(sched), 3, d_in.data_ptr(), in_off.ctypes.data,
                                   in_len.ctypes.data, d_out.data_ptr(), out_off.ctypes.data, out_cap.ctypes.data, out_len.ctypes.data,
                                   status.ctypes.data)
    assert rc == 0
    assert names() == PHASES_2EACDFD[("batch", level)]
    d_m = torch.zeros(MIB, dtype=torch.uint8, device="cuda")
    rc = c.encode_members_device(d_in.data_ptr(), 10000, d_m.data_ptr(), MIB, member_size=4096)[0]
    assert rc == ffi.OK
    assert names() == PHASES_2EACDFD[("members", level)]
