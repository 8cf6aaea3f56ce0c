"""GPU: the catalogue of crafted symbol counts (tests/huff_cases.py) through the kernels that run the Huffman stage (lfx_huff.h) on
320 lanes over LDS that the workgroup before left dirty: huffman_chunk_kernel and huffman_kernel (with histogram_kernel in front
for a caller's code words), block_merge_kernel and block_choose_kernel.  test_huff_cases.py has shown on the CPU that every case
is what it claims and that the one-lane build of the same source reproduces the oracle on it — a failure here with that module
green is a defect of the lane-parallel build.  Everything is byte-exact against lfo_oracle.

Bytes-driver cases (lz77_kind = 1) and parse-driver cases go through lfx_encode_device on device buffers in two contexts, one
made under LFX_PACK_BY_CHUNK=1 and one under =0, which must agree with each other and with the oracle; python-zlib reads the
result back.  The chunk path is legal for chunks of lz77_kind = 1 (encode_geometry, lfx_encode_stages.h: the fused histogram
counts CH_LITERALS chunks too, and nothing else is asked), so =1 runs huffman_chunk_kernel and pack_chunk_kernel on them; the
context's phase record names the same phases on both paths and cannot tell them apart, so the two contexts are told apart
only by how they were made.  A block of such chunks is ONE chunk row (the planner closes a chunk of a non-buffering encoder
only with its block): rows of unlike chunks (group h) come from the default parse with window_size = 1024.  The two contexts
live as long as the module: every case inherits what the cases before it left behind.

Codes-driver cases go through the stream encoder with a canned Lz77Encode, raw DEFLATE, one final block; there is no read-back,
the pointers reference no real history."""
import ctypes as C
import io
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import auto_block_model as abm
import huff_cases as hc
from test_gpu_auto_blocks import check as check_auto
from test_gpu_block_merge import check as check_merge
from test_gpu_encode_stages import _dev, context_with, torch  # noqa: F401  (torch: fixture)
from test_gpu_parity import ctx, ffi, lfx  # noqa: F401  (fixtures)
from test_host_pipeline import _CannedCodes

BYTES = [c.name for c in hc.CASES if c.driver == 'bytes']
CODES = [c.name for c in hc.CASES if c.driver == 'codes']
PARSE = [c.name for c in hc.CASES if c.driver == 'parse']
GUARD = 64


@pytest.fixture(scope="module")
def paths(lfx):
    """(a context that packs by chunk wherever it is legal, one that never does)"""
    return context_with(lfx, LFX_PACK_BY_CHUNK="1"), context_with(lfx, LFX_PACK_BY_CHUNK="0")


def encode_device(c, ffi, torch, fmt, d_in, spec):
    opts, sched = ffi.make_opts(**spec["opts"]), ffi.make_schedule(spec["write_size"], spec["writes"])
    n = len(spec["data"])
    cap = (ffi.lib().lfx_encode_bound(n, C.byref(opts), C.byref(sched)) + 3) & ~3
    d_out = torch.full((cap + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    got = c.encode_device(fmt, d_in.data_ptr(), n, d_out.data_ptr(), cap, opts, sched)
    assert bytes(d_out[cap:].cpu().numpy()) == b"\xA5" * GUARD, "bytes behind cap were written"
    return d_out[:got].cpu().numpy().tobytes()


def both_paths_and_oracle(paths, ffi, torch, oracle, name, formats):
    spec = hc.BY_NAME[name].make()
    d_in = _dev(torch, spec["data"])
    for fmt, ofmt, wbits in formats:
        want = hc.oracle_stream(oracle, ofmt, spec)
        one = encode_device(paths[0], ffi, torch, fmt, d_in, spec)
        zero = encode_device(paths[1], ffi, torch, fmt, d_in, spec)
        assert one == zero, (name, fmt, len(one), len(zero))
        assert one == want, (name, fmt, len(one), len(want))
        assert zlib.decompress(one, wbits) == spec["data"]
    assert paths[0].match_fallbacks() == 0 and paths[1].match_fallbacks() == 0


@pytest.mark.parametrize("name", BYTES)
def test_bytes_cases_on_both_pack_paths(paths, ffi, torch, oracle, name):
    both_paths_and_oracle(paths, ffi, torch, oracle, name, ((ffi.DEFLATE, oracle.DEFLATE, -15), (ffi.ZLIB, oracle.ZLIB, 15)))


@pytest.mark.parametrize("name", PARSE)
def test_rows_of_unlike_chunks_on_both_pack_paths(paths, ffi, torch, oracle, name):
    """gzip's header is 10 bytes, zlib's 2, raw DEFLATE has none: the first block starts at three word phases"""
    both_paths_and_oracle(paths, ffi, torch, oracle, name,
                          ((ffi.GZIP, oracle.GZIP, 31), (ffi.ZLIB, oracle.ZLIB, 15), (ffi.DEFLATE, oracle.DEFLATE, -15)))


@pytest.mark.parametrize("name", CODES)
def test_codes_cases_through_the_stream_encoder(ctx, lfx, oracle, name):
    codes = hc.BY_NAME[name].make()
    want = oracle.encode(oracle.DEFLATE, b"x", **oracle.custom_lz77(_CannedCodes(codes)))
    sink = io.BytesIO()
    enc = lfx.deflate.Encoder.with_options(sink, lfx.deflate.EncodeOptions().with_lz77(_CannedCodes(codes)), ctx)
    enc.write(b"x")
    enc.finish()
    assert sink.getvalue() == want, (name, len(sink.getvalue()), len(want))


# ---- group i: the 350 blocks as separate streams, merged, and chosen per block ------------------------------------------------
I_OPTS = dict(lz77_kind=1, block_size=hc.I_BS)


def test_group_i_as_a_batch_of_streams(paths, ffi, torch, oracle):
    L = ffi.lib()
    records = hc.i_blocks()
    count = len(records)
    assert count == 350 and sum(1 for r in records if not r) == 50
    opts, sched = ffi.make_opts(**I_OPTS), ffi.make_schedule(0)
    in_len = np.array([len(r) for r in records], dtype=np.uint64)
    in_off = np.concatenate(([0], np.cumsum(in_len)[:-1])).astype(np.uint64)
    out_cap = np.array([(L.lfx_encode_bound(int(n), C.byref(opts), C.byref(sched)) + 3) & ~3 for n in in_len], dtype=np.uint64)
    out_off = np.concatenate(([0], np.cumsum(out_cap)[:-1])).astype(np.uint64)
    total = int(out_cap.sum())
    d_in = _dev(torch, b"".join(records))
    want = {}
    for c in paths:
        d_out = torch.full((total + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        out_len, status = np.zeros(count, dtype=np.uint64), np.zeros(count, dtype=np.int32)
        rc = L.lfx_encode_batch_device(c.handle, ffi.ZLIB, C.byref(opts), C.byref(sched), count, d_in.data_ptr(), in_off.ctypes.data,
                                       in_len.ctypes.data, d_out.data_ptr(), out_off.ctypes.data, out_cap.ctypes.data, out_len.ctypes.data,
                                       status.ctypes.data)
        assert rc == 0 and not status.any(), (rc, c.last_error())
        whole = d_out.cpu().numpy()
        assert whole[total:].tobytes() == b"\xA5" * GUARD
        for i, r in enumerate(records):
            if r not in want:
                want[r] = oracle.encode(oracle.ZLIB, r, write_size=0, **I_OPTS)
            assert whole[int(out_off[i]):int(out_off[i]) + int(out_len[i])].tobytes() == want[r], i


@pytest.fixture(scope="module")
def i_base(oracle):
    data, writes = hc.i_schedule()
    return data, writes, abm.oracle_writes(oracle, "deflate", data, writes, **I_OPTS)


def test_group_i_with_block_merge(ctx, ffi, torch, oracle, i_base):
    """merge_tree builds node after node in one workgroup's scratch: a clamped build, then one of two symbols, then a full alphabet"""
    data, writes, base = i_base
    groups = check_merge(ctx, ffi, torch, oracle, "deflate", ffi.DEFLATE, data, base, write_size=0, writes=writes, **I_OPTS)
    assert any(n > 1 for _, n in groups) and any(n == 1 for _, n in groups)


def test_group_i_with_the_form_chosen_per_block(ctx, ffi, torch, oracle, i_base):
    data, writes, base = i_base
    want = abm.expected_writes(oracle, "deflate", data, writes, **I_OPTS)
    picked = check_auto(ctx, ffi, torch, oracle, "deflate", ffi.DEFLATE, data, want, writes=writes, **I_OPTS)
    assert set(picked) == {abm.STORED, abm.FIXED, abm.DYNAMIC}
    assert len(picked) == 351
