"""GPU: LFX_HUFFMAN_AUTO (include/lfx.h) through every entry point that serves it.  Every case compares bytes
with the stream the contract implies (tests/auto_block_model.py: the `= 1` and the `= 0` stream of the same call, cut at the
oracle's scan_blocks and spliced by the rule; test_auto_block_model.py proves the model on the CPU), reads the output back with
python-zlib, and checks it against the library's own `= 1` and `= 0` encodes: never longer than either.  Integer work: every
comparison is exact.  Inputs are a few KiB but the ones the eligibility edge (65535 / 65536 bytes in one block) needs."""
import ctypes as C
import gzip as pygzip
import io
import struct
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import auto_block_model as model
import auto_cases as cases
import chain_model
import dict_chain_model as dcm
import dict_encode_model as dm
import lazy_model
from auto_block_model import DYNAMIC, FIXED, STORED
from test_gpu_parity import ctx, ffi, lfx  # noqa: F401  (fixtures)
from test_gpu_round4 import OddChunksLiteral
from test_members_encode_abi import BC0, BGZF_EOF, random_bytes, slices, words_text

GUARD = 64
FORMATS = (("deflate", 0), ("zlib", 1), ("gzip", 2))
AUTO = 2


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def _dev(torch, data):
    a = np.frombuffer(bytes(data), dtype=np.uint8).copy() if len(data) else np.zeros(4, dtype=np.uint8)
    return torch.from_numpy(a).to("cuda")


def inflate(name, stream, zdict=None):
    if zdict is not None:
        return dm.py_inflate(name, stream, zdict)
    if name == "gzip":
        return pygzip.decompress(stream)
    return zlib.decompress(stream, -15 if name == "deflate" else 15)


def choices_of(ctx, ffi):
    """the test hook: the type every block of the context's last encode pass left block_choose_kernel with"""
    buf, n = (C.c_uint8 * 4096)(), C.c_size_t(0)
    assert ffi.lib().lfx_debug_block_choices(ctx.handle, buf, 4096, C.byref(n)) == ffi.OK
    return list(buf[:min(n.value, 4096)])


def encode(ctx, ffi, torch, fmt, data, dh, write_size=0, writes=None, zd=None, **kw):
    """lfx_encode_device (zd: lfx_encode_dict_device) on device buffers with dynamic_huffman = dh, a guard behind the capacity"""
    opts, sched = ffi.make_opts(dynamic_huffman=dh, **kw), ffi.make_schedule(write_size, writes)
    cap = (ffi.lib().lfx_encode_dict_bound(len(data), C.byref(opts), C.byref(sched)) + 3) & ~3
    d_in = _dev(torch, data)
    d_out = torch.full((cap + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    if zd is None:
        n = ctx.encode_device(fmt, d_in.data_ptr(), len(data), d_out.data_ptr(), cap, opts, sched)
    else:
        n = ctx.encode_dict_device(fmt, zd, d_in.data_ptr(), len(data), d_out.data_ptr(), cap, opts, sched)
    whole = d_out.cpu().numpy().tobytes()
    assert whole[cap:] == b"\xA5" * GUARD, "bytes behind cap were written"
    return whole[:n]


def check(ctx, ffi, torch, oracle, name, fmt, data, want, write_size=0, writes=None, zd=None, zdict=None, **kw):
    """want = (stream, choices, sizes) of the model → the AUTO encode equals it, its choices are the hook's, python-zlib reads
    it, and it is no longer than the library's own `= 1` and `= 0` encodes of the same call"""
    got = encode(ctx, ffi, torch, fmt, data, AUTO, write_size, writes, zd, **kw)
    picked = choices_of(ctx, ffi)
    assert got == want[0], (name, len(data), kw, len(got), len(want[0]), picked, want[1])
    assert picked == want[1]
    assert inflate(name, got, zdict) == data
    for dh in (1, 0):
        assert len(got) <= len(encode(ctx, ffi, torch, fmt, data, dh, write_size, writes, zd, **kw))
        assert choices_of(ctx, ffi) == []              # (nothing of an AUTO call stays behind)
    return want[1]


def okw(name, **kw):
    return dict(kw, mtime=0) if name == "gzip" else kw


# ---- single streams
@pytest.mark.parametrize("name,fmt", FORMATS)
def test_text_sizes(ctx, ffi, torch, oracle, name, fmt):
    seen = set()
    for n in cases.SIZES:
        data = cases.record(n)
        seen |= set(check(ctx, ffi, torch, oracle, name, fmt, data, model.expected(oracle, name, data, **okw(name))))
    assert seen == {FIXED, DYNAMIC}


def test_empty_stream_is_two_bytes(ctx, ffi, torch, oracle):
    assert encode(ctx, ffi, torch, ffi.DEFLATE, b"", AUTO) == b"\x03\x00"


@pytest.mark.parametrize("n,want", [(1000, STORED), (60000, STORED), (65535, STORED), (65536, DYNAMIC)])
def test_random_and_the_eligibility_edge(ctx, ffi, torch, oracle, n, want):
    data = cases.rand(n)
    assert check(ctx, ffi, torch, oracle, "zlib", ffi.ZLIB, data, model.expected(oracle, "zlib", data)) == [want]


def test_stored_block_of_several_chunks(ctx, ffi, torch, oracle):
    """window_size = 1024 and 4096-byte writes: an LZ77 flush every 8192 bytes, eight chunks in the one block"""
    data = cases.rand(60000)
    enc = lambda f, d, **kw: oracle.encode(oracle.DEFLATE, d, 4096, **kw)
    want = model.expected(oracle, "deflate", data, encode=enc, window_size=1024)
    o, sched = ffi.make_opts(window_size=1024), ffi.make_schedule(4096)
    ch, bl, nc, nb = (C.c_uint64 * 400)(), (C.c_uint64 * 60)(), C.c_size_t(0), C.c_size_t(0)
    assert ffi.lib().lfx_debug_plan(0, C.byref(o), C.byref(sched), len(data), ch, 100, C.byref(nc), bl, 10, C.byref(nb)) == 0
    assert (nc.value, nb.value) == (8, 1)
    assert check(ctx, ffi, torch, oracle, "deflate", ffi.DEFLATE, data, want, write_size=4096, window_size=1024) == [STORED]


def test_tie_and_one_bit_either_side_of_stored(ctx, ffi, torch, oracle):
    data = cases.record(*cases.TIE)
    assert check(ctx, ffi, torch, oracle, "deflate", ffi.DEFLATE, data, model.expected(oracle, "deflate", data)) == [FIXED]
    got = [check(ctx, ffi, torch, oracle, "deflate", ffi.DEFLATE, d, model.expected(oracle, "deflate", d))[0] for d, _ in cases.S_EDGE]
    assert got[0] != STORED and got[1] != STORED and got[2] == STORED


@pytest.mark.parametrize("length", cases.PHASE_PREFIX)
def test_mixed_blocks_at_every_bit_phase(ctx, ffi, torch, oracle, length):
    data, writes = cases.prefixed(length)
    for name, fmt in (FORMATS if length == cases.PHASE_PREFIX[0] else FORMATS[:1]):
        want = model.expected_writes(oracle, name, data, writes, **okw(name, block_size=4096))
        assert check(ctx, ffi, torch, oracle, name, fmt, data, want, writes=writes, block_size=4096) == [DYNAMIC, STORED, DYNAMIC, FIXED]


def test_max_length_3(ctx, ffi, torch, oracle):
    data = cases.record(3000, 5) + cases.rand(500, 2)
    check(ctx, ffi, torch, oracle, "zlib", ffi.ZLIB, data, model.expected(oracle, "zlib", data, max_length=3), max_length=3)


@pytest.mark.parametrize("kind,mdl", [(2, chain_model), (3, lazy_model)])
def test_chained_and_lazy_lz77(ctx, ffi, torch, oracle, kind, mdl):
    data, writes = cases.prefixed(5)
    enc = lambda name, d, **kw: mdl.expected_scheduled(oracle, oracle.ZLIB, d, 8, writes, **kw)
    want = model.expected(oracle, "zlib", data, encode=enc, block_size=4096)
    picked = check(ctx, ffi, torch, oracle, "zlib", ffi.ZLIB, data, want, writes=writes, block_size=4096, lz77_kind=kind | 8 << 8)
    assert set(picked) == {STORED, FIXED, DYNAMIC}


def test_encode_host(ctx, ffi, lfx, oracle):
    data, writes = cases.prefixed(7)
    for name, fmt in FORMATS:
        want = model.expected_writes(oracle, name, data, writes, **okw(name, block_size=4096))
        got = ctx.encode_host(fmt, data, ffi.make_opts(dynamic_huffman=AUTO, block_size=4096), ffi.make_schedule(0, writes))
        assert got == want[0] and choices_of(ctx, ffi) == want[1]
    # the option builders: deflate, zlib and gzip
    small = cases.record(64)
    for name, mod in (("deflate", lfx.deflate), ("zlib", lfx.zlib), ("gzip", lfx.gzip)):
        assert ffi.HUFFMAN_AUTO == AUTO
        got = mod.compress(small, options=mod.EncodeOptions().auto_huffman_codes(), context=ctx)
        assert inflate(name, got) == small
        if name != "gzip":                                   # (the module's gzip header carries the time)
            assert got == model.expected(oracle, name, small)[0]


# ---- batches, dictionaries
def batch(ctx, ffi, torch, fmt, records, dh, zd=None, **kw):
    opts = ffi.make_opts(dynamic_huffman=dh, **kw)
    caps = [(ffi.lib().lfx_encode_dict_bound(len(r), C.byref(opts), None) + 3) & ~3 for r in records]
    in_offs, out_offs, a, b = [], [], 0, 0
    for r, cap in zip(records, caps):
        in_offs.append(a)
        out_offs.append(b)
        a += len(r)
        b += cap
    d_in = _dev(torch, b"".join(records))
    d_out = torch.full((b + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    rc, res = ctx.encode_batch_dict_device(fmt, zd, d_in.data_ptr(), in_offs, [len(r) for r in records], d_out.data_ptr(), out_offs, caps, opts)
    assert rc == ffi.OK and all(st == ffi.OK for st, _ in res), ctx.last_error()
    whole = d_out.cpu().numpy().tobytes()
    assert whole[b:] == b"\xA5" * GUARD
    return [whole[o:o + n] for o, (_, n) in zip(out_offs, res)]


def check_batch(ctx, ffi, torch, oracle, name, fmt, records, enc, zd=None, zdict=None, **kw):
    want = [model.expected(oracle, name, r, encode=enc, zdict=zdict) for r in records]
    got = batch(ctx, ffi, torch, fmt, records, AUTO, zd, **kw)
    picked = choices_of(ctx, ffi)
    assert picked == [c for w in want for c in w[1]]
    dyn, fix = batch(ctx, ffi, torch, fmt, records, 1, zd, **kw), batch(ctx, ffi, torch, fmt, records, 0, zd, **kw)
    for i, r in enumerate(records):
        assert got[i] == want[i][0], (i, len(r), want[i][1:])
        assert inflate(name, got[i], zdict) == r
        assert len(got[i]) <= len(dyn[i]) and len(got[i]) <= len(fix[i])
    return set(picked)


def test_batch_of_300_records(ctx, ffi, torch, oracle):
    records = cases.batch_records()
    for name, fmt in FORMATS[:2]:
        code = oracle.ZLIB if name == "zlib" else oracle.DEFLATE
        seen = check_batch(ctx, ffi, torch, oracle, name, fmt, records, lambda f, d, **kw: oracle.encode(code, d, **kw))
        assert seen == {STORED, FIXED, DYNAMIC}


def test_batch_through_a_plain_dictionary(ctx, ffi, lfx, torch, oracle):
    records = cases.batch_records()
    zd = lfx.Dictionary(cases.DICT, ctx)
    try:
        enc = lambda f, d, **kw: dm.expected_stream(oracle, f, cases.DICT, d, **kw)
        assert FIXED in check_batch(ctx, ffi, torch, oracle, "zlib", ffi.ZLIB, records, enc, zd, cases.DICT)
        # the one-shot call; a stored block holds the record's bytes alone
        data = cases.rand(3000, 9)
        want = model.expected(oracle, "deflate", data, encode=enc, zdict=cases.DICT)
        assert check(ctx, ffi, torch, oracle, "deflate", ffi.DEFLATE, data, want, zd=zd, zdict=cases.DICT) == [STORED]
        assert want[0][5:] == data
    finally:
        zd.close()


def test_batch_through_a_chain_dictionary_lazy_8(ctx, ffi, lfx, torch, oracle):
    records = cases.batch_records()[::3]
    zd = lfx.Dictionary(cases.DICT, ctx, chain=True)
    try:
        enc = lambda f, d, **kw: dcm.expected_stream(oracle, f, cases.DICT, d, dcm.LAZY, 8, **kw)
        check_batch(ctx, ffi, torch, oracle, "zlib", ffi.ZLIB, records, enc, zd, cases.DICT, lz77_kind=3 | 8 << 8)
    finally:
        zd.close()


# ---- the stream encoder
def test_stream_encoder_bytes_mode(ctx, ffi, lfx, oracle):
    msgs = cases.messages()
    data = b"".join(msgs)
    writes = [x for m in msgs for x in (len(m), None)]
    for name, mod in (("deflate", lfx.deflate), ("zlib", lfx.zlib)):
        want = model.expected_writes(oracle, name, data, writes)
        outs = []
        for opts in (mod.EncodeOptions().auto_huffman_codes(), mod.EncodeOptions(), mod.EncodeOptions().fixed_huffman_codes()):
            enc = mod.Encoder.with_options(io.BytesIO(), opts, ctx)
            for m in msgs:
                enc.write(m)
                enc.flush()
            outs.append(enc.finish().getvalue())
        assert outs[0] == want[0] and set(want[1]) == {STORED, FIXED, DYNAMIC}
        assert inflate(name, outs[0]) == data
        assert len(outs[0]) <= len(outs[1]) and len(outs[0]) <= len(outs[2])


def test_stream_encoder_codes_mode_never_stores(ctx, ffi, lfx, oracle):
    msgs = cases.messages()
    data = b"".join(msgs)
    writes = [x for m in msgs for x in (len(m), None)]
    enc_model = lambda f, d, **kw: model.oracle_writes(oracle, f, d, writes, **dict(kw, **oracle.custom_lz77(OddChunksLiteral(oracle, 2))))
    want = model.expected(oracle, "deflate", data, stored_ok=False, encode=enc_model)
    assert STORED not in want[1] and STORED in model.expected(oracle, "deflate", data, encode=enc_model)[1]
    enc = lfx.deflate.Encoder.with_options(io.BytesIO(), lfx.deflate.EncodeOptions().with_lz77(OddChunksLiteral(oracle, 2)).auto_huffman_codes(), ctx)
    for m in msgs:
        enc.write(m)
        enc.flush()
    got = enc.finish().getvalue()
    assert got == want[0]
    assert [b[2] for b in oracle.scan_blocks(got)] == want[1]
    assert inflate("deflate", got) == data


# ---- members
def members_model(oracle, data, member_size, bgzf):
    out = []
    for sl in (slices(data, member_size) if data or not bgzf else []):
        kw = dict(extra=BC0) if bgzf else {}
        m = model.expected(oracle, "gzip", sl, **kw)[0]
        if bgzf:
            if len(m) > 65536:
                m = oracle.encode(oracle.GZIP, sl, extra=BC0, no_compression=1)
            m = m[:16] + struct.pack("<H", len(m) - 1) + m[18:]
        out.append(m)
    return b"".join(out) + (BGZF_EOF if bgzf else b"")


def run_members(ctx, ffi, data, member_size, flags, dh):
    rc, out, count, members, msg = ctx.encode_members_host(data, member_size, flags, ffi.make_opts(dynamic_huffman=dh))
    assert rc == ffi.OK, msg
    return out


@pytest.mark.parametrize("name,member_size,bgzf", [("mixed", 4096, False), ("random", 65280, True), ("text", 65280, True)])
def test_members(ctx, ffi, oracle, name, member_size, bgzf):
    data = {"mixed": cases.mixed, "random": lambda: random_bytes(150 * 1000), "text": lambda: words_text(150 * 1000)}[name]()
    flags = ffi.MEMBERS_BGZF if bgzf else 0
    got = run_members(ctx, ffi, data, member_size, flags, AUTO)
    assert got == members_model(oracle, data, member_size, bgzf)
    assert pygzip.decompress(got) == data
    for dh in (1, 0):
        assert len(got) <= len(run_members(ctx, ffi, data, member_size, flags, dh))


# ---- state
def test_no_state_is_left_between_calls(ctx, ffi, torch, oracle):
    """AUTO, then 1, then 0, then AUTO on one context with identical plans: the block table the AUTO call changed on the device
    is uploaded again, whatever the host shadow says"""
    data, writes = cases.prefixed(3)
    auto = model.expected_writes(oracle, "deflate", data, writes, block_size=4096)[0]
    dyn, fix = [model.oracle_writes(oracle, "deflate", data, writes, block_size=4096, dynamic_huffman=dh) for dh in (1, 0)]
    for dh, want in ((AUTO, auto), (1, dyn), (0, fix), (AUTO, auto), (AUTO, auto), (1, dyn), (1, dyn)):
        assert encode(ctx, ffi, torch, ffi.DEFLATE, data, dh, writes=writes, block_size=4096) == want, dh
    assert auto != dyn and auto != fix


def test_values_other_than_0_and_2_stay_dynamic(ctx, ffi, torch, oracle):
    data = cases.record(64)
    dyn = oracle.encode(oracle.DEFLATE, data)
    for dh in (1, 3, -1):
        assert encode(ctx, ffi, torch, ffi.DEFLATE, data, dh) == dyn
    assert encode(ctx, ffi, torch, ffi.DEFLATE, data, 0) == oracle.encode(oracle.DEFLATE, data, dynamic_huffman=0)


def test_refusals(ctx, ffi, torch):
    data = cases.record(5000)
    d_in = _dev(torch, data)
    d_out = torch.zeros((1 << 16,), dtype=torch.uint8, device="cuda")
    opts = ffi.make_opts(dynamic_huffman=AUTO)
    out_len, idx = C.c_uint64(0), C.c_void_p()
    rc = ffi.lib().lfx_encode_index_device(ctx.handle, ffi.GZIP, C.byref(opts), None, d_in.data_ptr(), len(data), d_out.data_ptr(), 1 << 16,
                                           C.byref(out_len), 4096, C.byref(idx))
    assert rc == ffi.E_UNSUPPORTED and not idx.value
    assert "lfx_encode_index_device does not serve LFX_HUFFMAN_AUTO" in ctx.last_error()
    info = ffi.ShardInfo()
    rc = ffi.lib().lfx_encode_shard_prepare(ctx.handle, ffi.GZIP, C.byref(opts), None, d_in.data_ptr(), len(data), 1, 1, C.byref(info))
    assert rc == ffi.E_UNSUPPORTED
    assert "the N-GPU encode does not serve LFX_HUFFMAN_AUTO" in ctx.last_error()
    # the N-GPU encode, a world of one rank (no collective is called): it prepares through lfx_encode_shard_prepare
    cm, state, part = ffi.Comm(), C.c_void_p(), ffi.ShardedPart()
    cm.rank, cm.world = 0, 1
    d_member = torch.zeros((1 << 16,), dtype=torch.uint8, device="cuda")
    rc = ffi.lib().lfx_sharded_encode_begin(ctx.handle, C.byref(cm), ffi.GZIP, C.byref(opts), None, d_in.data_ptr(), len(data),
                                            d_out.data_ptr(), 1 << 16, d_member.data_ptr(), 1 << 16, None, 0, C.byref(state), C.byref(part))
    assert rc == ffi.E_UNSUPPORTED and not state.value
    assert "the N-GPU encode does not serve LFX_HUFFMAN_AUTO" in ctx.last_error()
    # the context is as good as before
    assert ctx.encode_host(ffi.DEFLATE, b"", opts) == b"\x03\x00"
