"""GPU: block_merge (include/lfx.h) through every entry point that serves it.  Every case compares bytes with
the stream the contract implies (tests/merge_model.py: the `= 0` stream of the same call, its code words read back, the tree
rule with every size taken from the oracle; test_merge_model.py proves the model on the CPU), compares the groups
lfx_debug_block_merges reports with the model's, reads the output back with python-zlib, and checks that it is no longer than
the library's own `block_merge = 0` encode.  Integer work: every comparison is exact.  Inputs of a few dozen KiB."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

import auto_block_model as abm
import auto_cases as cases
import chain_model
import dict_chain_model as dcm
import dict_encode_model as dm
import level_model
import merge_cases as mc
import merge_model as model
from test_gpu_auto_blocks import GUARD, _dev, choices_of, encode, inflate, okw, torch  # noqa: F401  (torch: fixture)
from test_gpu_encode_stages import context_with
from test_gpu_parity import ctx, ffi, lfx  # noqa: F401  (fixtures)

FORMATS = (("deflate", 0), ("zlib", 1), ("gzip", 2))
BS = mc.BS


def merges_of(c, ffi):
    """the test hook: for every block of the context's last encode pass, the block it ended up in"""
    buf, n = (C.c_uint32 * 8192)(), C.c_size_t(0)
    assert ffi.lib().lfx_debug_block_merges(c.handle, buf, 8192, C.byref(n)) == ffi.OK
    return list(buf[:min(n.value, 8192)])


def ocode(oracle, name):
    return {"deflate": oracle.DEFLATE, "zlib": oracle.ZLIB, "gzip": oracle.GZIP}[name]


def check(c, ffi, torch, oracle, name, fmt, data, base, write_size=BS, writes=None, zd=None, zdict=None, auto=False, **kw):
    """base: the model's `block_merge = 0` stream of the call → the `= 1` encode equals the model's stream, its groups are the
    hook's, python-zlib reads it, and it is no longer than the library's own `= 0` encode (which is `base`).  → the groups"""
    dh = 2 if auto else 1
    want = model.expected(oracle, name, base, data, zdict, auto)
    got = encode(c, ffi, torch, fmt, data, dh, write_size, writes, zd, block_merge=1, **kw)
    heads = merges_of(c, ffi)
    assert got == want[0], (name, len(data), kw, len(got), len(want[0]), heads, want[1])
    assert heads == want[1]
    if auto:
        it = iter(want[3])
        assert choices_of(c, ffi) == [next(it) if h == i else 3 for i, h in enumerate(want[1])]
    assert inflate(name, got, zdict) == data
    plain = encode(c, ffi, torch, fmt, data, dh, write_size, writes, zd, **kw)
    assert merges_of(c, ffi) == []                       # (nothing of a block_merge call stays behind)
    assert len(got) <= len(plain)
    if not auto:
        assert plain == base
    return model.groups(want[1])


# ---- single streams
@pytest.mark.parametrize("name,fmt", FORMATS)
def test_64k_of_text_merges_fully(ctx, ffi, torch, oracle, name, fmt):
    data = mc.text(65536)
    base = oracle.encode(ocode(oracle, name), data, BS, **okw(name, block_size=BS))
    # (sixteen full candidates and the empty one that closes a stream whose length is a multiple of the write size)
    assert check(ctx, ffi, torch, oracle, name, fmt, data, base, **okw(name, block_size=BS)) == [(0, 16), (16, 1)]


def test_sections_keep_their_cuts(ctx, ffi, torch, oracle):
    data = mc.sections()
    base = oracle.encode(oracle.ZLIB, data, BS, block_size=BS)
    got = check(ctx, ffi, torch, oracle, "zlib", ffi.ZLIB, data, base, block_size=BS)
    assert got == [(0, 2), (2, 2), (4, 2), (6, 2), (8, 1)]


@pytest.mark.parametrize("n", mc.RUNS)
def test_run_lengths(ctx, ffi, torch, oracle, n):
    data = mc.run_of(n)
    base = oracle.encode(oracle.DEFLATE, data, BS, block_size=BS)
    assert check(ctx, ffi, torch, oracle, "deflate", ffi.DEFLATE, data, base, block_size=BS) == mc.RUN_GROUPS[n]


@pytest.mark.parametrize("seed,diff", mc.TIES)
def test_ties(ctx, ffi, torch, oracle, seed, diff):
    data = mc.tie(seed)
    base = oracle.encode(oracle.DEFLATE, data, mc.TIE_BS, block_size=mc.TIE_BS)
    got = check(ctx, ffi, torch, oracle, "deflate", ffi.DEFLATE, data, base, write_size=mc.TIE_BS, block_size=mc.TIE_BS)
    assert got == ([(0, 2)] if diff <= 0 else [(0, 1), (1, 1)])


def test_a_zlib_sync_flush_splits_a_run(ctx, ffi, torch, oracle):
    data = mc.text(6 * BS + 100, 4)
    writes = [BS, BS, BS, None, BS, BS, BS, 100]
    base = abm.oracle_writes(oracle, "zlib", data, writes, block_size=BS, zlib_sync_flush=1)
    got = check(ctx, ffi, torch, oracle, "zlib", ffi.ZLIB, data, base, write_size=0, writes=writes, block_size=BS, zlib_flush_mode=2)
    # three candidates, the flush's own (empty) candidate, the marker, four candidates
    assert got == [(0, 4), (4, 1), (5, 4)]


@pytest.mark.parametrize("n", [0, 1, 100, BS - 1])
def test_empty_and_shorter_than_one_block(ctx, ffi, torch, oracle, n):
    data = mc.text(n, 6)
    base = oracle.encode(oracle.DEFLATE, data, BS, block_size=BS)
    assert check(ctx, ffi, torch, oracle, "deflate", ffi.DEFLATE, data, base, block_size=BS) == [(0, 1)]


def test_candidates_of_several_chunks(ctx, ffi, torch, oracle):
    """window_size = 1024 and 4096-byte writes: an LZ77 flush every 8192 bytes, two chunks in every 16 KiB candidate"""
    data = mc.text(65536 + 500, 7)
    kw = dict(window_size=1024, block_size=16384)
    base = oracle.encode(oracle.ZLIB, data, BS, **kw)
    o, sched = ffi.make_opts(**kw), ffi.make_schedule(BS)
    ch, bl, nc, nb = (C.c_uint64 * 400)(), (C.c_uint64 * 60)(), C.c_size_t(0), C.c_size_t(0)
    assert ffi.lib().lfx_debug_plan(1, C.byref(o), C.byref(sched), len(data), ch, 100, C.byref(nc), bl, 10, C.byref(nb)) == 0
    assert (nc.value, nb.value) == (9, 5)
    assert check(ctx, ffi, torch, oracle, "zlib", ffi.ZLIB, data, base, **kw) == [(0, 5)]


def test_auto_on_top_stores_a_merged_random_section(ctx, ffi, torch, oracle):
    data = mc.text(8192, 8) + cases.rand(8192, 9) + mc.text(5000, 10)
    base = oracle.encode(oracle.DEFLATE, data, BS, block_size=BS)
    want = model.expected(oracle, "deflate", base, data, None, True)
    assert model.groups(want[1]) == [(0, 2), (2, 2), (4, 2)] and want[3][1] == abm.STORED
    check(ctx, ffi, torch, oracle, "deflate", ffi.DEFLATE, data, base, auto=True, block_size=BS)


def test_level_6_and_chain_depth_8(ctx, ffi, torch, oracle):
    data = mc.sections()[:3 * 8192] + mc.text(5000, 11)
    base = level_model.expected_stream(oracle, oracle.ZLIB, data, 6, BS, block_size=BS)
    check(ctx, ffi, torch, oracle, "zlib", ffi.ZLIB, data, base, block_size=BS, lz77_kind=ffi.LZ77_LEVEL | 6 << 8)
    base = chain_model.expected_stream(oracle, oracle.ZLIB, data, 8, BS, block_size=BS)
    check(ctx, ffi, torch, oracle, "zlib", ffi.ZLIB, data, base, block_size=BS, lz77_kind=ffi.LZ77_CHAIN | 8 << 8)


# ---- batches, dictionaries
def batch(c, ffi, torch, fmt, records, zd=None, **kw):
    opts, sched = ffi.make_opts(**kw), ffi.make_schedule(BS)
    caps = [(ffi.lib().lfx_encode_dict_bound(len(r), C.byref(opts), C.byref(sched)) + 3) & ~3 for r in records]
    in_offs, out_offs, a, b = [], [], 0, 0
    for r, cap in zip(records, caps):
        in_offs.append(a)
        out_offs.append(b)
        a += len(r)
        b += cap
    d_in = _dev(torch, b"".join(records))
    d_out = torch.full((b + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    rc, res = c.encode_batch_dict_device(fmt, zd, d_in.data_ptr(), in_offs, [len(r) for r in records], d_out.data_ptr(), out_offs, caps,
                                         opts, sched)
    assert rc == ffi.OK and all(st == ffi.OK for st, _ in res), c.last_error()
    whole = d_out.cpu().numpy().tobytes()
    assert whole[b:] == b"\xA5" * GUARD
    return [whole[o:o + n] for o, (_, n) in zip(out_offs, res)]


def check_batch(c, ffi, torch, oracle, name, fmt, records, bases, zd=None, zdict=None, **kw):
    want = [model.expected(oracle, name, b, r, zdict) for b, r in zip(bases, records)]
    got = batch(c, ffi, torch, fmt, records, zd, block_size=BS, block_merge=1, **kw)
    heads = merges_of(c, ffi)
    plain = batch(c, ffi, torch, fmt, records, zd, block_size=BS, **kw)
    assert merges_of(c, ffi) == []
    at, merged = 0, 0
    for i, r in enumerate(records):
        assert got[i] == want[i][0], (i, len(r), want[i][1])
        # no group crosses a record: the record's heads are its own blocks, as the model has them
        assert heads[at:at + len(want[i][1])] == [at + h for h in want[i][1]], i
        assert inflate(name, got[i], zdict) == r
        assert plain[i] == bases[i] and len(got[i]) <= len(plain[i])
        merged += sum(1 for q, h in enumerate(want[i][1]) if h != q)
        at += len(want[i][1])
    # (how many merge is the rule's affair and checked against the model above; the batch only has to hold merged groups at all)
    assert at == len(heads) and merged > 0


def test_batch_of_200_records(ctx, ffi, torch, oracle):
    records = mc.batch_records()
    bases = [oracle.encode(oracle.ZLIB, r, BS, block_size=BS) for r in records]
    check_batch(ctx, ffi, torch, oracle, "zlib", ffi.ZLIB, records, bases)


def test_batch_through_a_plain_dictionary(ctx, ffi, lfx, torch, oracle):
    records = mc.batch_records()
    zd = lfx.Dictionary(cases.DICT, ctx)
    try:
        bases = [dm.expected_stream(oracle, "zlib", cases.DICT, r, BS, block_size=BS) for r in records]
        check_batch(ctx, ffi, torch, oracle, "zlib", ffi.ZLIB, records, bases, zd, cases.DICT)
        data = records[2]                                # the one-shot call
        check(ctx, ffi, torch, oracle, "deflate", ffi.DEFLATE, data, dm.expected_stream(oracle, "deflate", cases.DICT, data, BS, block_size=BS),
              zd=zd, zdict=cases.DICT, block_size=BS)
    finally:
        zd.close()


def test_batch_through_a_chain_dictionary_lazy_8(ctx, ffi, lfx, torch, oracle):
    records = mc.batch_records()[::3]
    zd = lfx.Dictionary(cases.DICT, ctx, chain=True)
    try:
        bases = [dcm.expected_stream(oracle, "zlib", cases.DICT, r, dcm.LAZY, 8, BS, block_size=BS) for r in records]
        check_batch(ctx, ffi, torch, oracle, "zlib", ffi.ZLIB, records, bases, zd, cases.DICT, lz77_kind=3 | 8 << 8)
    finally:
        zd.close()


# ---- the host call, the module helpers
def test_encode_host_and_the_module_helpers(ctx, ffi, lfx, oracle):
    data = mc.sections()
    for name, fmt in FORMATS:
        base = oracle.encode(ocode(oracle, name), data, BS, **okw(name, block_size=BS))
        want = model.expected(oracle, name, base, data)
        got = ctx.encode_host(fmt, data, ffi.make_opts(block_size=BS, block_merge=1, **okw(name)), ffi.make_schedule(BS))
        assert got == want[0] and merges_of(ctx, ffi) == want[1]
    # the option builders and the keyword: one write_all, so one candidate — the option reaches the library and changes nothing
    small = mc.text(3000, 12)
    for name, mod in (("deflate", lfx.deflate), ("zlib", lfx.zlib), ("gzip", lfx.gzip)):
        assert mod.EncodeOptions().merge_blocks()._to_c().block_merge == 1
        one = mod.compress(small, options=mod.EncodeOptions().merge_blocks(), context=ctx)
        assert merges_of(ctx, ffi) == [0]
        two = mod.compress(small, merge_blocks=True, context=ctx)
        assert merges_of(ctx, ffi) == [0]
        assert one == two == mod.compress(small, context=ctx) and inflate(name, one) == small
        assert merges_of(ctx, ffi) == []


def test_pack_by_chunk_switch_stays_correct(lfx, ffi, torch, oracle):
    """LFX_PACK_BY_CHUNK=1 takes the chunk path wherever it is legal; a block_merge call stays off it"""
    c = context_with(lfx, LFX_PACK_BY_CHUNK="1")
    data = mc.sections()
    base = oracle.encode(oracle.ZLIB, data, BS, block_size=BS)
    check(c, ffi, torch, oracle, "zlib", ffi.ZLIB, data, base, block_size=BS)


# ---- state
def test_no_state_is_left_between_calls(ctx, ffi, torch, oracle):
    """merge → plain → merge → merge → plain on one context with identical plans: the block and chunk tables the merge changed
    on the device are uploaded again, whatever the host shadows say"""
    data = mc.sections()
    base = oracle.encode(oracle.DEFLATE, data, BS, block_size=BS)
    merged = model.expected(oracle, "deflate", base, data)[0]
    assert merged != base
    for bm, want in ((1, merged), (0, base), (1, merged), (1, merged), (0, base), (0, base)):
        assert encode(ctx, ffi, torch, ffi.DEFLATE, data, 1, BS, block_size=BS, block_merge=bm) == want, bm


def test_no_effect_under_stored_blocks_and_fixed_codes(ctx, ffi, torch, oracle):
    data = mc.text(3 * BS, 13)
    for kw in (dict(no_compression=1), dict(dynamic_huffman=0)):
        dh = kw.get("dynamic_huffman", 1)
        okw_ = {k: v for k, v in kw.items() if k != "dynamic_huffman"}
        got = encode(ctx, ffi, torch, ffi.DEFLATE, data, dh, BS, block_size=BS, block_merge=1, **okw_)
        assert got == oracle.encode(oracle.DEFLATE, data, BS, block_size=BS, **kw) and merges_of(ctx, ffi) == []


# ---- the domain, the refusals
def test_the_value_2_is_outside_the_domain(ctx, ffi, torch):
    data = mc.text(100)
    d_in, d_out = _dev(torch, data), torch.zeros((4096,), dtype=torch.uint8, device="cuda")
    out_len = C.c_uint64(0)
    for v in (2, 3, 0xFFFFFFFF):
        opts = ffi.make_opts(block_merge=v)
        rc = ffi.lib().lfx_encode_device(ctx.handle, ffi.DEFLATE, C.byref(opts), None, d_in.data_ptr(), len(data), d_out.data_ptr(), 4096,
                                         C.byref(out_len))
        assert rc == ffi.E_ARG
        assert ffi.lib().lfx_encode_bound(100, C.byref(opts), None) == 0


def test_refusals(ctx, ffi, lfx, torch):
    import io
    data = mc.text(5000)
    d_in = _dev(torch, data)
    d_out = torch.zeros((1 << 16,), dtype=torch.uint8, device="cuda")
    opts = ffi.make_opts(block_merge=1)
    # the stream encoder
    L = ffi.lib()
    with pytest.raises(lfx.deflate.StreamError) as refused:
        lfx.deflate.Encoder.with_options(io.BytesIO(), lfx.deflate.EncodeOptions().merge_blocks(), ctx)
    assert "status %d" % ffi.E_UNSUPPORTED in str(refused.value)
    assert "the stream encoder does not serve block_merge" in ctx.last_error()
    # the members encode
    with pytest.raises(ffi.LfxError) as refused:
        ctx.encode_members_host(data, 4096, 0, opts)
    assert "status %d" % ffi.E_UNSUPPORTED in str(refused.value) and "lfx_encode_members_* does not serve block_merge" in str(refused.value)
    # the encode with an index
    out_len, idx = C.c_uint64(0), C.c_void_p()
    rc = L.lfx_encode_index_device(ctx.handle, ffi.GZIP, C.byref(opts), None, d_in.data_ptr(), len(data), d_out.data_ptr(), 1 << 16,
                                   C.byref(out_len), 4096, C.byref(idx))
    assert rc == ffi.E_UNSUPPORTED and not idx.value
    assert "lfx_encode_index_device does not serve block_merge" in ctx.last_error()
    # the N-GPU encode
    info = ffi.ShardInfo()
    rc = L.lfx_encode_shard_prepare(ctx.handle, ffi.GZIP, C.byref(opts), None, d_in.data_ptr(), len(data), 1, 1, C.byref(info))
    assert rc == ffi.E_UNSUPPORTED and "the N-GPU encode does not serve block_merge" in ctx.last_error()
    cm, state, part = ffi.Comm(), C.c_void_p(), ffi.ShardedPart()
    cm.rank, cm.world = 0, 1
    d_member = torch.zeros((1 << 16,), dtype=torch.uint8, device="cuda")
    rc = L.lfx_sharded_encode_begin(ctx.handle, C.byref(cm), ffi.GZIP, C.byref(opts), None, d_in.data_ptr(), len(data),
                                    d_out.data_ptr(), 1 << 16, d_member.data_ptr(), 1 << 16, None, 0, C.byref(state), C.byref(part))
    assert rc == ffi.E_UNSUPPORTED and not state.value
    # under no_compression there is nothing to refuse; the context is as good as before
    rc, out, count, members, msg = ctx.encode_members_host(data, 4096, 0, ffi.make_opts(block_merge=1, no_compression=1))
    assert rc == ffi.OK
    assert ctx.encode_host(ffi.DEFLATE, b"", opts) == ctx.encode_host(ffi.DEFLATE, b"")
