"""GPU: lfx_dict_train_device / _host (include/lfx.h) — the dictionary the device trains equals the model's
(tests/dict_train_model.py) byte for byte on every crafted case of tests/dict_train_cases.py and on the generator's records at
scale; nothing outside the dictionary is written; the host call equals the device call; and a trained dictionary round-trips
through the batch encode and decode.  Integer work: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import dict_train_cases as cases
from test_gpu_parity import ctx, ffi, lfx  # noqa: F401  (fixtures)

GUARD = 64
SENTINEL = 0xA5
CASES = cases.cases()
BIG = cases.big_cases()


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def expected():
    """the model's dictionary per case, computed once"""
    return {c[0]: cases.expect(c)[0] for c in CASES + BIG}


def _dev(torch, data):
    a = np.frombuffer(bytes(data), dtype=np.uint8).copy() if len(data) else np.zeros(4, dtype=np.uint8)
    return torch.from_numpy(a).to("cuda")


def train_device(torch, ctx, case):
    """→ the dictionary; the bytes around it must keep their values"""
    _name, buf, offs, lens, size, k = case
    d_in = _dev(torch, buf)
    d_out = torch.full((size + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n = ctx.dict_train_device(d_in.data_ptr(), offs, lens, size, k, d_out.data_ptr() + GUARD, size)
    out = d_out.cpu().numpy().tobytes()
    assert n <= size and n % k == 0
    assert out[:GUARD] == bytes([SENTINEL]) * GUARD and out[GUARD + n:] == bytes([SENTINEL]) * (size - n + GUARD)
    return out[GUARD:GUARD + n]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_crafted_case_equals_the_model(torch, ctx, expected, case):
    assert train_device(torch, ctx, case) == expected[case[0]]


@pytest.mark.parametrize("case", BIG, ids=[c[0] for c in BIG])
def test_generator_records_equal_the_model(torch, ctx, expected, case):
    got = train_device(torch, ctx, case)
    assert len(got) == case[4] and got == expected[case[0]]


def test_again_on_the_same_context(torch, ctx, expected):
    """the scratch is the context's: a small call behind a large one, and the large one again, see none of each other"""
    by_name = {c[0]: c for c in CASES + BIG}
    for name in ("gen4096_size2048", "tie_across_epochs", "gen4096_size2048", "shorter_than_a_dmer"):
        assert train_device(torch, ctx, by_name[name]) == expected[name], name


def test_host_call_equals_device_call(torch, ctx, expected):
    for case in CASES + BIG[:1]:
        name, buf, offs, lens, size, k = case
        assert ctx.dict_train_host(buf, offs, lens, size, k) == expected[name], name


def test_arguments(torch, ctx, ffi):
    L = ffi.lib()
    buf = b"".join(cases.log_lines(8, 21))
    d_in, d_out = _dev(torch, buf), torch.full((256,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    one = lambda v: (C.c_uint64 * 1)(v)
    two = lambda a, b: (C.c_uint64 * 2)(a, b)
    got = C.c_uint64(7)
    call = lambda count, off, ln, size, seg, cap: L.lfx_dict_train_device(ctx.handle, d_in.data_ptr(), count, off, ln, size, seg,
                                                                         d_out.data_ptr(), cap, C.byref(got))
    n = len(buf)
    for size, seg in ((63, 16), (32769, 128), (64, 15), (64, 65), (64, 0)):
        assert call(1, one(0), one(n), size, seg, 1 << 16) == ffi.E_ARG, (size, seg)
    assert call(1, None, one(n), 128, 128, 256) == ffi.E_ARG
    assert call(2, two(100, 50), two(10, 10), 128, 128, 256) == ffi.E_ARG           # not ascending
    assert call(2, two(0, 99), two(100, 10), 128, 128, 256) == ffi.E_ARG            # overlapping
    assert call(2, two(0, 1 << 31), two(1 << 31, 1), 128, 128, 256) == ffi.E_ARG    # more than 2^31 positions
    assert call(1, one(0), one(n), 128, 128, 127) == ffi.E_NOSPACE
    assert got.value == 7
    # no records, or only empty ones: OK and an empty dictionary
    assert call(0, None, None, 128, 128, 256) == ffi.OK and got.value == 0
    got.value = 7
    assert call(2, two(5, 5), two(0, 0), 128, 128, 256) == ffi.OK and got.value == 0
    assert d_out.cpu().numpy().tobytes() == bytes([SENTINEL]) * 256
    # segment 0 selects 128
    assert call(1, one(0), one(n), 256, 0, 256) == ffi.OK and got.value == 256


@pytest.mark.parametrize("chain,level", [(False, None), (True, 6)], ids=["plain", "chain_level6"])
def test_round_trip_through_the_batch_calls(torch, lfx, ctx, chain, level):
    recs = cases.log_lines(600, 31)
    train, held = recs[:400], recs[400:]
    zdict = lfx.Dictionary.train(train, size=2048, segment=128, context=ctx, chain=chain)
    assert zdict.trained == 2048
    kw = {"level": level} if level else {}
    streams = lfx.zlib.compress_batch(held, zdict=zdict, context=ctx, **kw)
    assert lfx.zlib.decompress_batch(streams, zdict=zdict, context=ctx) == held
    # the dictionary earns its keep, and Python's zlib reads the streams with the same bytes
    import zlib as pyzlib
    raw = lfx.train_dictionary(train, 2048, 128, context=ctx)
    assert len(raw) == 2048 and sum(map(len, streams)) < sum(len(s) for s in lfx.zlib.compress_batch(held, context=ctx, **kw))
    for s, r in zip(streams[:20], held[:20]):
        assert pyzlib.decompressobj(zdict=raw).decompress(s) == r


def test_records_in_a_tensor(torch, lfx, ctx, expected):
    """Dictionary.train from (tensor, offsets, lengths): the dictionary never leaves the device, and it is the same one"""
    name, buf, offs, lens, size, k = BIG[0]
    zdict = lfx.Dictionary.train((_dev(torch, buf), offs, lens), size=size, segment=k, context=ctx)
    want = lfx.Dictionary(expected[name], ctx)
    assert zdict.trained == len(expected[name]) and zdict.id == want.id
