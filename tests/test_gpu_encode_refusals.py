"""GPU: every refusing cell of the table of which encode entry point serves what (encode_served, libflate_amd/csrc/lfx_enc_frame.h;
DESIGN.md §3.0; the whole table on the CPU: tests/c/encode_spec.cpp) through the real entry points — status, message, outputs
untouched, and the context as good as before.  Every case is an argument refusal that returns before a launch."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import auto_cases as cases
from test_gpu_parity import ctx, ffi, lfx  # noqa: F401  (fixtures)

N = 5000
CAP = 1 << 16
CHAIN, LAZY = 2 | 8 << 8, 3 | 8 << 8
MSG = {
    "dict_chain": "lz77_kind: LFX_LZ77_CHAIN with a preset dictionary is not supported (a dictionary made by lfx_dict_new_chain serves it)",
    "dict_lazy": "lz77_kind: LFX_LZ77_LAZY with a preset dictionary is not supported (a dictionary made by lfx_dict_new_chain serves it)",
    "shard_chain": "lz77_kind: the N-GPU encode does not serve LFX_LZ77_CHAIN",
    "shard_lazy": "lz77_kind: the N-GPU encode does not serve LFX_LZ77_LAZY",
    "shard_auto": "dynamic_huffman: the N-GPU encode does not serve LFX_HUFFMAN_AUTO (a stored block's size depends on the bit phase)",
    "shard_stored": "sharded encode of stored blocks is not supported (their size depends on the bit phase)",
    "index_auto": "dynamic_huffman: lfx_encode_index_device does not serve LFX_HUFFMAN_AUTO (the candidates are laid out from the host plan's block types)",
}
# (entry point, its options, the message)
CASES = [
    ("dict_device", dict(lz77_kind=CHAIN), "dict_chain"), ("dict_device", dict(lz77_kind=LAZY), "dict_lazy"),
    ("dict_host", dict(lz77_kind=CHAIN), "dict_chain"), ("dict_host", dict(lz77_kind=LAZY), "dict_lazy"),
    ("batch_dict", dict(lz77_kind=CHAIN), "dict_chain"), ("batch_dict", dict(lz77_kind=LAZY), "dict_lazy"),
    ("shard_prepare", dict(lz77_kind=CHAIN), "shard_chain"), ("shard_prepare", dict(lz77_kind=LAZY), "shard_lazy"),
    ("shard_prepare", dict(dynamic_huffman=2), "shard_auto"), ("shard_prepare", dict(no_compression=1), "shard_stored"),
    ("sharded_begin", dict(lz77_kind=LAZY), "shard_lazy"), ("sharded_begin", dict(dynamic_huffman=2), "shard_auto"),
    ("index", dict(dynamic_huffman=2), "index_auto"),
]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def bufs(torch):
    """the 5000 input bytes, on the host and on the device, made once"""
    data = cases.record(N)
    assert len(data) == N
    return data, torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda")


@pytest.fixture(scope="module")
def plain(lfx, ctx, bufs):
    d = lfx.Dictionary(bufs[0][:2000], ctx, chain=False)
    yield d
    d.close()


@pytest.mark.parametrize("entry,kw,msg", CASES, ids=["%s-%s" % (e, m) for e, _, m in CASES])
def test_refusal_matrix(ctx, ffi, torch, bufs, plain, entry, kw, msg):
    L = ffi.lib()
    data, d_in = bufs
    opts = ffi.make_opts(**kw)
    d_out = torch.full((CAP,), 0xA5, dtype=torch.uint8, device="cuda")
    out_len = C.c_uint64(77)
    untouched = lambda: bool((d_out == 0xA5).all()) and out_len.value == 77
    if entry == "dict_device":
        rc = L.lfx_encode_dict_device(ctx.handle, ffi.ZLIB, C.byref(opts), None, plain.handle, d_in.data_ptr(), N, d_out.data_ptr(), CAP,
                                      C.byref(out_len))
        assert untouched()
    elif entry == "dict_host":
        out = C.create_string_buffer(b"\xA5" * CAP, CAP)
        rc = L.lfx_encode_dict_host(ctx.handle, ffi.ZLIB, C.byref(opts), None, plain.handle, data, N, out, CAP, C.byref(out_len))
        assert out.raw == b"\xA5" * CAP and out_len.value == 77
    elif entry == "batch_dict":
        u64 = lambda *v: np.array(v, dtype=np.uint64)
        io, il, oo, oc, ol, st = u64(0, 2500), u64(2500, 2500), u64(0, CAP // 2), u64(CAP // 2, CAP // 2), u64(77, 77), np.full(2, 77, dtype=np.int32)
        rc = L.lfx_encode_batch_dict_device(ctx.handle, ffi.DEFLATE, C.byref(opts), None, plain.handle, 2, d_in.data_ptr(), io.ctypes.data,
                                            il.ctypes.data, d_out.data_ptr(), oo.ctypes.data, oc.ctypes.data, ol.ctypes.data, st.ctypes.data)
        assert untouched() and list(ol) == [77, 77] and list(st) == [77, 77]
    elif entry == "shard_prepare":
        info = ffi.ShardInfo(77, 77, 77, 77)
        rc = L.lfx_encode_shard_prepare(ctx.handle, ffi.GZIP, C.byref(opts), None, d_in.data_ptr(), N, 1, 1, C.byref(info))
        assert (info.total_bits, info.n_bytes, info.crc32, info.adler32) == (77, 77, 77, 77)
    elif entry == "sharded_begin":
        # the N-GPU encode, a world of one rank (no collective is called): it prepares through lfx_encode_shard_prepare.  (Its
        # shard buffer is zero-filled beside the prepare call by design: not looked at here.)
        cm, state, part = ffi.Comm(), C.c_void_p(), ffi.ShardedPart()
        cm.rank, cm.world = 0, 1
        d_member = torch.full((CAP,), 0xA5, dtype=torch.uint8, device="cuda")
        rc = L.lfx_sharded_encode_begin(ctx.handle, C.byref(cm), ffi.GZIP, C.byref(opts), None, d_in.data_ptr(), N, d_out.data_ptr(), CAP,
                                        d_member.data_ptr(), CAP, None, 0, C.byref(state), C.byref(part))
        assert not state.value and bool((d_member == 0xA5).all())
    else:
        idx = C.c_void_p()
        rc = L.lfx_encode_index_device(ctx.handle, ffi.GZIP, C.byref(opts), None, d_in.data_ptr(), N, d_out.data_ptr(), CAP, C.byref(out_len),
                                       4096, C.byref(idx))
        assert not idx.value and untouched()
    assert rc == ffi.E_UNSUPPORTED
    assert ctx.last_error() == MSG[msg]
    # the context is as good as before (no bytes: LFX_HUFFMAN_AUTO picks the fixed form, an empty final block)
    assert ctx.encode_host(ffi.DEFLATE, b"", ffi.make_opts(dynamic_huffman=2)) == b"\x03\x00"
