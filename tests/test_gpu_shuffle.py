"""GPU: the byte-shuffle filter (include/lfx.h "the byte-shuffle filter") — lfx_shuffle_device, _batch_device and
_host against tests/shuffle_model.py byte for byte, both directions: every element size that takes another kernel path, the
sizes around one element and around one tile, every 16-byte residue of the input and output places on the register path,
a batch of records lying back to back (the boundary-race case) with canaries around it, the refusals, and the shuffle= keyword
of the compress / decompress calls against Python's own zlib.  Byte permutations: every comparison is exact."""
import gzip as pygzip
import zlib as pyzlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import shuffle_model as model
from test_gpu_parity import ctx, ffi, lfx  # noqa: F401  (fixtures)

SIZES = (1, 2, 3, 4, 5, 8, 16, 17, 256)
CANARY_IN, CANARY_OUT = 0x5A, 0xA5


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def place(lens, gaps=None, start=0):
    """offsets of records lying back to back from `start`; gaps: {index: bytes left free in front of that record}"""
    offs, at = [], start
    for i, n in enumerate(lens):
        at += (gaps or {}).get(i, 0)
        offs.append(at)
        at += n
    return offs, at


def run_batch(torch, ctx, recs, s, inverse, in_offs, out_offs, in_size, out_size, table=False, single=False):
    """the records at in_offs of a canary-filled input → the whole output buffer; with table=True the places come from a device
    table and out_offs must equal in_offs"""
    src = np.full(max(in_size, 16), CANARY_IN, dtype=np.uint8)
    for r, o in zip(recs, in_offs):
        src[o:o + len(r)] = np.frombuffer(r, dtype=np.uint8)
    d_in = torch.from_numpy(src).to("cuda")
    d_out = torch.full((max(out_size, 16),), CANARY_OUT, dtype=torch.uint8, device="cuda")
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    lens = [len(r) for r in recs]
    if table:
        assert out_offs == in_offs
        pairs = np.array([v for o, n in zip(in_offs, lens) for v in (o, n)], dtype=np.int64)
        d_table = torch.from_numpy(pairs).to("cuda")
        torch.cuda.synchronize()
        ctx.shuffle_batch_device(d_in.data_ptr(), len(recs), None, d_out.data_ptr(), s, inverse=inverse, d_table=d_table.data_ptr())
    elif single:
        torch.cuda.synchronize()
        ctx.shuffle_device(d_in.data_ptr() + in_offs[0], lens[0], d_out.data_ptr() + out_offs[0], s, inverse=inverse)
    else:
        torch.cuda.synchronize()
        ctx.shuffle_batch_device(d_in.data_ptr(), in_offs, lens, d_out.data_ptr(), s, inverse=inverse, out_offs=out_offs)
    assert d_in.cpu().numpy().tobytes() == src.tobytes()            # the input is only read
    return d_out.cpu().numpy()


def check(torch, ctx, recs, s, in_offs, out_offs, in_size, out_size, **kw):
    """both directions: every record equals the model, every other byte of the output keeps its canary"""
    for inverse in (False, True):
        want = [model.unshuffle(r, s) if inverse else model.shuffle(r, s) for r in recs]
        got = run_batch(torch, ctx, recs, s, inverse, in_offs, out_offs, in_size, out_size, **kw)
        expect = np.full(len(got), CANARY_OUT, dtype=np.uint8)
        for w, o in zip(want, out_offs):
            expect[o:o + len(w)] = np.frombuffer(w, dtype=np.uint8)
        bad = np.nonzero(got != expect)[0]
        assert bad.size == 0, (s, inverse, "first differing output byte", int(bad[0]), [(o, len(w)) for w, o in zip(want, out_offs)][:8])


@pytest.mark.parametrize("s", SIZES)
def test_sizes_around_one_element(torch, ctx, s):
    lens = sorted({0, 1, s - 1, s, s + 1, 2 * s - 1, 2 * s})
    recs = [model.payload(n, 100 + s + i) for i, n in enumerate(lens)]
    gaps = {i: 3 for i in range(len(lens))}
    in_offs, in_size = place(lens, gaps, 5)
    out_offs, out_size = place(lens, gaps, 7)
    check(torch, ctx, recs, s, in_offs, out_offs, in_size + 9, out_size + 9)
    for r in recs:            # the one-record call, at an odd place
        check(torch, ctx, [r], s, [3], [1], len(r) + 8, len(r) + 8, single=True)


@pytest.mark.parametrize("s", SIZES)
def test_sizes_around_one_tile(torch, ctx, s):
    t = model.tile_elems(s)
    lens = [(t - 1) * s, t * s, (t + 1) * s, (3 * t + 5) * s + s - 1]
    recs = [model.payload(n, 200 + s + i) for i, n in enumerate(lens)]
    in_offs, in_size = place(lens, {0: 1, 2: 2}, 0)
    out_offs, out_size = place(lens, {1: 5}, 3)
    check(torch, ctx, recs, s, in_offs, out_offs, in_size + 4, out_size + 4)


@pytest.mark.parametrize("s", (2, 4, 8))
def test_every_residue_of_the_places(torch, ctx, s):
    """the register path's wide loads and stores at every input and output residue 0..15, heads and ragged ends included"""
    recs, in_offs, out_offs, a_in, a_out = [], [], [], 0, 0
    for a in range(16):
        for b in range(16):
            n = (259 + a + 3 * b) * s + (a + b) % s            # full lanes, a ragged last lane, trailing bytes
            a_in = (a_in + 15) // 16 * 16 + 16 + a
            a_out = (a_out + 15) // 16 * 16 + 16 + b
            recs.append(model.payload(n, 1000 * s + 16 * a + b))
            in_offs.append(a_in)
            out_offs.append(a_out)
            a_in += n
            a_out += n
    check(torch, ctx, recs, s, in_offs, out_offs, a_in + 32, a_out + 32)


@pytest.mark.parametrize("s", (4, 3, 16, 17))
@pytest.mark.parametrize("table", (False, True), ids=("host_arrays", "device_table"))
def test_batch_back_to_back(torch, ctx, s, table):
    """about 40 mixed records with no gap between neighbours and odd lengths: a store that reaches over a record's or a plane's
    end lands in a neighbour that another workgroup writes at the same time"""
    t = model.tile_elems(s)
    rng = np.random.default_rng(7 + s)
    lens = [0, 1, s - 1, t * s + 1, (2 * t + 3) * s + s - 1, 0, s + 1]
    while len(lens) < 40:
        kind = len(lens) % 4
        k = (int(rng.integers(1, 40)), int(rng.integers(t - 9, t + 9)), int(rng.integers(2 * t, 3 * t)), int(rng.integers(0, 2)))[kind]
        lens.append(k * s + int(rng.integers(0, s)) | (s > 1))       # (odd, where s allows a remainder)
    recs = [model.payload(n, 300 + i) for i, n in enumerate(lens)]
    gaps = {0: 13, 11: 1, 23: 3}                                     # canaries in front of the first record and in two gaps
    offs, size = place(lens, gaps, 0)
    check(torch, ctx, recs, s, offs, offs, size + 11, size + 11, table=table)


def test_refusals(torch, ctx, ffi):
    import ctypes as C
    L = ffi.lib()
    d = torch.full((4096,), CANARY_OUT, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p = d.data_ptr()
    one = lambda v: (C.c_uint64 * 1)(v)
    tab = torch.tensor([0, 64], dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    h = ctx.handle
    assert L.lfx_shuffle_device(h, 0, 0, p, 64, p + 1024) == ffi.E_ARG
    assert L.lfx_shuffle_device(h, 0, 257, p, 64, p + 1024) == ffi.E_ARG
    assert L.lfx_shuffle_device(h, 2, 4, p, 64, p + 1024) == ffi.E_ARG
    assert L.lfx_shuffle_device(h, -1, 4, p, 64, p + 1024) == ffi.E_ARG
    assert L.lfx_shuffle_host(h, 0, 0, b"abcd", 4, C.create_string_buffer(4)) == ffi.E_ARG
    # the descriptor forms: both, neither, one host array alone, out_off with the table
    assert L.lfx_shuffle_batch_device(h, 0, 4, 1, p, one(0), one(64), tab.data_ptr(), p + 1024, None) == ffi.E_ARG
    assert L.lfx_shuffle_batch_device(h, 0, 4, 1, p, None, None, None, p + 1024, None) == ffi.E_ARG
    assert L.lfx_shuffle_batch_device(h, 0, 4, 1, p, one(0), None, None, p + 1024, None) == ffi.E_ARG
    assert L.lfx_shuffle_batch_device(h, 0, 4, 1, p, None, one(64), None, p + 1024, None) == ffi.E_ARG
    assert L.lfx_shuffle_batch_device(h, 0, 4, 1, p, None, None, tab.data_ptr(), p + 1024, one(0)) == ffi.E_ARG
    assert L.lfx_shuffle_batch_device(h, 0, 4, 1, p, None, None, tab.data_ptr() + 4, p + 1024, None) == ffi.E_ARG
    # overlap: in place, partly, the output of one record over the input of another, two outputs over each other
    assert L.lfx_shuffle_device(h, 0, 4, p, 64, p) == ffi.E_ARG
    assert L.lfx_shuffle_device(h, 1, 4, p, 64, p + 63) == ffi.E_ARG
    two = lambda a, b: (C.c_uint64 * 2)(a, b)
    assert L.lfx_shuffle_batch_device(h, 0, 4, 2, p, two(0, 512), two(64, 64), None, p, two(1024, 500)) == ffi.E_ARG
    assert L.lfx_shuffle_batch_device(h, 0, 4, 2, p, two(0, 64), two(64, 64), None, p + 1024, two(0, 32)) == ffi.E_ARG
    assert L.lfx_shuffle_batch_device(h, 0, 4, 1, p, None, None, tab.data_ptr(), p, None) == ffi.E_ARG        # (the table in place)
    with pytest.raises(ffi.LfxError):
        ctx.shuffle_device(p, 64, p + 32, 4)
    # nothing to do
    assert L.lfx_shuffle_device(h, 0, 4, p, 0, p) == ffi.OK
    assert L.lfx_shuffle_batch_device(h, 0, 4, 0, p, None, None, None, p, None) == ffi.OK
    assert L.lfx_shuffle_host(h, 1, 4, None, 0, None) == ffi.OK
    torch.cuda.synchronize()
    assert bool((d == CANARY_OUT).all())                              # no refused call and no empty call wrote a byte


def test_host_call_and_filters(lfx, ctx):
    for s, n in ((4, 100003), (3, 70001), (8, 8), (1, 5), (256, 1000)):
        x = model.payload(n, 40 + s)
        assert ctx.shuffle_host(x, s) == model.shuffle(x, s)
        assert lfx.filters.shuffle(x, s, context=ctx) == model.shuffle(x, s)
        assert lfx.filters.unshuffle(model.shuffle(x, s), s, context=ctx) == x
    assert lfx.filters.shuffle(b"", 4, context=ctx) == b""


@pytest.fixture(scope="module")
def tensors():
    """numeric records: a smooth fp32 signal plus noise, fp32 weights, an odd-sized tail, an empty record"""
    rng = np.random.default_rng(11)
    t = np.arange(20000, dtype=np.float32)
    sig = (np.sin(t / 300) * 100 + rng.normal(0, 0.01, t.size)).astype(np.float32).tobytes()
    w = rng.normal(0, 0.02, 12345).astype(np.float32).tobytes()
    return [sig, w, sig[:4001], b"", w[:3]]


def test_compress_batch_keyword(lfx, ctx, tensors):
    z = lfx.zlib
    plain_before = z.compress_batch(tensors, context=ctx)
    got = z.compress_batch(tensors, context=ctx, shuffle=4)
    assert got == z.compress_batch([model.shuffle(r, 4) for r in tensors], context=ctx)
    # what an HDF5 reader does with a chunk: inflate, then unshuffle
    assert [model.unshuffle(pyzlib.decompress(g), 4) for g in got] == tensors
    assert z.decompress_batch(got, context=ctx, shuffle=4) == tensors
    assert sum(map(len, got)) < sum(map(len, plain_before))           # the reason the filter exists
    # a call without the keyword behind calls with it returns what it returned before
    assert z.compress_batch(tensors, context=ctx) == plain_before
    assert z.decompress_batch(plain_before, context=ctx) == tensors
    # the keyword with the other options: a level parse
    lv = z.compress_batch(tensors, context=ctx, level=6, shuffle=4)
    assert lv == z.compress_batch([model.shuffle(r, 4) for r in tensors], context=ctx, level=6)
    assert [model.unshuffle(pyzlib.decompress(g), 4) for g in lv] == tensors


def test_gzip_deflate_and_one_shot(lfx, ctx, tensors):
    g = lfx.gzip.compress_batch(tensors, context=ctx, shuffle=2)
    assert g == lfx.gzip.compress_batch([model.shuffle(r, 2) for r in tensors], context=ctx)
    assert [model.unshuffle(pygzip.decompress(x), 2) for x in g] == tensors
    assert lfx.gzip.decompress_batch(g, context=ctx, shuffle=2) == tensors
    d = lfx.deflate.compress_batch(tensors, context=ctx, shuffle=3)
    assert d == lfx.deflate.compress_batch([model.shuffle(r, 3) for r in tensors], context=ctx)
    assert [model.unshuffle(pyzlib.decompress(x, wbits=-15), 3) for x in d] == tensors
    assert lfx.deflate.decompress_batch(d, context=ctx, shuffle=3) == tensors
    # the one-shot calls
    for mod, inflate in ((lfx.zlib, pyzlib.decompress), (lfx.gzip, pygzip.decompress)):
        before = mod.compress(tensors[0], context=ctx)
        one = mod.compress(tensors[0], context=ctx, shuffle=4)
        assert one == mod.compress(model.shuffle(tensors[0], 4), context=ctx)
        assert model.unshuffle(inflate(one), 4) == tensors[0]
        assert mod.decompress(one, context=ctx, shuffle=4) == tensors[0]
        assert mod.compress(tensors[0], context=ctx) == before and mod.decompress(before, context=ctx) == tensors[0]
    with pytest.raises(lfx._ffi.LfxError):
        lfx.zlib.compress_batch(tensors, context=ctx, shuffle=0)
