"""GPU: pack by chunk (symbol counts per chunk, huffman_chunk_kernel, pack_chunk_kernel) against the tile-parallel
pack kernels and the oracle.  Every case is encoded by a fresh context with LFX_PACK_BY_CHUNK=1 — the chunk path wherever it is
legal, whatever the number of chunks: small inputs reach it — and by a fresh one with =0; the two must agree byte for byte, and
with lfo_oracle, for gzip, zlib and raw DEFLATE.  Inputs of at most 2 MiB, 8192-byte writes unless a case says otherwise."""
import ctypes as C
import gzip as pygzip
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_parity import ffi, lfx, synth  # noqa: F401  (fixtures)
from test_gpu_encode_stages import context_with, torch, _dev  # noqa: F401  (fixture, helpers)

KIB, MIB = 1 << 10, 1 << 20


def encode_device(c, ffi, torch, fmt, data, write_size=8192, writes=None, **okw):
    opts, sched = ffi.make_opts(**okw), ffi.make_schedule(write_size, writes)
    cap = (ffi.lib().lfx_encode_bound(len(data), C.byref(opts), C.byref(sched)) + 3) & ~3
    d_in = _dev(torch, data)
    d_out = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    n = c.encode_device(fmt, d_in.data_ptr(), len(data), d_out.data_ptr(), cap, opts, sched)
    whole = d_out.cpu().numpy().tobytes()
    assert whole[cap:] == b"\xA5" * 64, "bytes behind cap were written"
    return whole[:n]


def oracle_encode(oracle, fmt, data, write_size=8192, writes=None, **okw):
    if writes is None:
        return oracle.encode(fmt, data, write_size=write_size, **okw)
    e, at = oracle.Encoder(fmt, **okw), 0
    for w in writes:
        e.write(data[at:at + w])
        at += w
    assert at == len(data)
    return e.finish()


def literals(n):
    """n bytes in which no three bytes occur twice: the greedy parse finds no match, the chunk is n literal code words (and
    EndOfBlock): the number of code words is known exactly"""
    for seed in range(1000):
        b = np.random.RandomState(seed).randint(0, 256, size=n, dtype=np.uint8).tobytes()
        if len({b[i:i + 3] for i in range(n - 2)}) == max(n - 2, 0):
            return b
    raise AssertionError("no seed without a repeated three-byte string")


@pytest.fixture(scope="module")
def cases(synth):
    text = synth.text(2 * MIB).tobytes()
    rnd = np.random.RandomState(5).randint(0, 256, size=2 * MIB, dtype=np.uint8).tobytes()
    out = {}
    # one chunk of exactly 1, 2047, 2048, 2049, 4096 and 4097 code words (PACK_TILE = 2048): n - 1 literals and EndOfBlock
    for ncodes in (1, 2047, 2048, 2049, 4096, 4097):
        out["codes_%d" % ncodes] = (literals(ncodes - 1), {})
    # random bytes: the longest code words, the staging buffer at its fullest
    out["random_64k"] = (rnd[:64 * KIB], {})
    out["random_2m"] = (rnd, {})
    # all 258-byte matches: few code words per chunk, every chunk far short of its tiles
    out["lowent_1m"] = (synth.lowent(MIB).tobytes(), {})
    # a block of two chunks whose last holds one literal and EndOfBlock (256 KiB close the first chunk, the byte behind them
    # closes the block), then the empty final block: a chunk that holds only EndOfBlock.  (A chunk of NO bytes behind other
    # chunks of its block cannot be planned: the planner — block_flush, lfx_plan.h — makes a zero-length chunk only for a block
    # that holds nothing but EndOfBlock, and every case here ends with such a block.  One byte is the nearest reachable shape.)
    out["last_chunk_one_byte"] = (text[:256 * KIB + 1], dict(writes=[256 * KIB, 1], block_size=256 * KIB + 1))
    # 1 MiB = the block size: four chunks, then the empty final block
    out["text_1m"] = (text[:MIB], {})
    # blocks of 600000 bytes (rounded up to whole writes) over chunks of 256 KiB: blocks of unequal chunk counts
    out["blocks_600000"] = (text, dict(block_size=600000))
    # fixed codes: no header behind the three block bits
    out["fixed_1m"] = (text[:MIB], dict(dynamic_huffman=0))
    # writes of 1000 bytes: chunks of 262000 + ... bytes, blocks that end inside a tile
    out["writes_1000"] = (text[:MIB + 12345], dict(write_size=1000))
    return out


CASE_NAMES = ["codes_1", "codes_2047", "codes_2048", "codes_2049", "codes_4096", "codes_4097", "random_64k", "random_2m", "lowent_1m",
              "last_chunk_one_byte", "text_1m", "blocks_600000", "fixed_1m", "writes_1000"]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_chunk_path_equals_tile_path_and_oracle(lfx, ffi, torch, oracle, cases, name):
    data, kw = cases[name]
    by_chunk, by_tile = context_with(lfx, LFX_PACK_BY_CHUNK="1"), context_with(lfx, LFX_PACK_BY_CHUNK="0")
    # (gzip's header is 10 bytes, zlib's 2, raw DEFLATE has none: the first block starts at three different word phases)
    for fmt, ofmt in ((ffi.GZIP, oracle.GZIP), (ffi.ZLIB, oracle.ZLIB), (ffi.DEFLATE, oracle.DEFLATE)):
        one = encode_device(by_chunk, ffi, torch, fmt, data, **kw)
        zero = encode_device(by_tile, ffi, torch, fmt, data, **kw)
        assert one == zero, (name, fmt)
        assert one == oracle_encode(oracle, ofmt, data, **kw), (name, fmt)
    assert by_chunk.match_fallbacks() == 0 and by_tile.match_fallbacks() == 0


def test_all_cases_are_run(cases):
    assert sorted(cases) == sorted(CASE_NAMES)


def test_shards_at_a_bit_phase(lfx, ffi, torch, synth):
    """lfx_encode_shard_emit packs at a caller's start bit: the second of two shards starts wherever the first one's bits end,
    at any bit phase of a word.  The member the two parts assemble to is one gzip stream of the input, the same on both paths."""
    from libflate_amd import sharded
    L = ffi.lib()
    data = synth.text(MIB + 300 * KIB).tobytes()
    halves = [data[:MIB], data[MIB:]]            # (a shard that is not the last ends on a block boundary: the block size)
    opts, sched = ffi.make_opts(), ffi.make_schedule(8192)
    d_in = [_dev(torch, h) for h in halves]
    members = {}
    for switch in ("1", "0"):
        ctxs = [context_with(lfx, LFX_PACK_BY_CHUNK=switch) for _ in halves]
        infos = []
        for r, (c, h, d) in enumerate(zip(ctxs, halves, d_in)):
            info = ffi.ShardInfo()
            rc = L.lfx_encode_shard_prepare(c.handle, ffi.GZIP, C.byref(opts), C.byref(sched), d.data_ptr(), len(h), int(r == 0),
                                            int(r == 1), C.byref(info))
            assert rc == 0, c.last_error()
            infos.append((info.total_bits, info.n_bytes, info.crc32, info.adler32))
        hdr_len = L.lfx_container_header_len(ffi.GZIP, C.byref(opts))
        start_bits, check, total_n = sharded.layout(infos, hdr_len, ffi.GZIP)
        assert start_bits[1] % 32 != 0, "the case is about a start inside a word"
        parts = []
        for r, (c, h) in enumerate(zip(ctxs, halves)):
            cap = len(h) + len(h) // 4 + 65536
            d_s = torch.empty(cap, dtype=torch.uint8, device="cuda")
            m = C.c_uint64(0)
            rc = L.lfx_encode_shard_emit(c.handle, start_bits[r], check, total_n, d_s.data_ptr(), cap, C.byref(m))
            assert rc == 0, c.last_error()
            parts.append(d_s[:m.value].cpu().numpy().tobytes())
        members[switch] = sharded.assemble(parts, start_bits)
        assert pygzip.decompress(members[switch]) == data, switch
    assert members["1"] == members["0"]


def test_stored_blocks_stay_on_the_tile_path(lfx, ffi, torch, oracle, cases):
    """no_compression: every block is stored — nothing to pack by chunk; =1 changes nothing"""
    data = cases["text_1m"][0][:300000]
    c = context_with(lfx, LFX_PACK_BY_CHUNK="1")
    for fmt, ofmt in ((ffi.GZIP, oracle.GZIP), (ffi.ZLIB, oracle.ZLIB), (ffi.DEFLATE, oracle.DEFLATE)):
        assert encode_device(c, ffi, torch, fmt, data, no_compression=1) == oracle.encode(ofmt, data, write_size=8192, no_compression=1)


def test_callers_code_words_stay_on_the_tile_path(lfx, oracle, cases):
    """a caller's own Lz77Encode (the stream encoder's codes mode): no parse has counted the chunks' symbols; =1 changes nothing"""

    class EveryByteALiteral:
        def encode(self, buf, sink):
            sink.extend(("Literal", b) for b in buf)

        def flush(self, sink):
            pass

        def compression_level(self):
            return 0

        def window_size(self):
            return 32768

    data = cases["text_1m"][0][:200000]
    want = oracle.encode(oracle.GZIP, data, write_size=70000, mtime=0, block_size=60000, **oracle.custom_lz77(EveryByteALiteral()))
    sink = io.BytesIO()
    c = context_with(lfx, LFX_PACK_BY_CHUNK="1")
    enc = lfx.gzip.Encoder.with_options(sink, lfx.gzip.EncodeOptions().with_lz77(EveryByteALiteral()).block_size(60000), c)
    for a in range(0, len(data), 70000):
        enc.write(data[a:a + 70000])
    enc.finish()
    assert sink.getvalue() == want


def test_more_chunks_than_workgroups(lfx, ffi, torch, oracle, cases):
    """A batch of 2304 short streams is 2304 chunks: more than the eight workgroups per CU the chunk kernel launches, so
    workgroups take several chunks one after the other — of different blocks, with the code tables reloaded in between."""
    L = ffi.lib()
    text = cases["blocks_600000"][0]                         # (the 2 MiB text)
    sizes = [0, 1, 37, 300, 2100]                            # (0 bytes: a chunk that holds only EndOfBlock)
    count = 2304
    in_len = np.array([sizes[i % len(sizes)] for i in range(count)], dtype=np.uint64)
    in_off = np.concatenate(([0], np.cumsum(in_len)[:-1])).astype(np.uint64)
    assert int(in_len.sum()) <= len(text)
    data = text[:int(in_len.sum())]
    opts, sched = ffi.make_opts(), ffi.make_schedule(8192)
    out_cap = np.array([(L.lfx_encode_bound(int(n), C.byref(opts), C.byref(sched)) + 3) & ~3 for n in in_len], dtype=np.uint64)
    out_off = np.concatenate(([0], np.cumsum(out_cap)[:-1])).astype(np.uint64)
    d_in = _dev(torch, data)
    got = {}
    for switch in ("1", "0"):
        c = context_with(lfx, LFX_PACK_BY_CHUNK=switch)
        d_out = torch.full((int(out_cap.sum()),), 0xAA, dtype=torch.uint8, device="cuda")
        out_len, status = np.zeros(count, dtype=np.uint64), np.zeros(count, dtype=np.int32)
        rc = L.lfx_encode_batch_device(c.handle, ffi.ZLIB, C.byref(opts), C.byref(sched), count, d_in.data_ptr(), in_off.ctypes.data,
                                       in_len.ctypes.data, d_out.data_ptr(), out_off.ctypes.data, out_cap.ctypes.data, out_len.ctypes.data,
                                       status.ctypes.data)
        assert rc == 0 and not status.any(), (rc, c.last_error())
        whole = d_out.cpu().numpy()
        got[switch] = [whole[int(out_off[i]):int(out_off[i]) + int(out_len[i])].tobytes() for i in range(count)]
    assert got["1"] == got["0"]
    for i in list(range(0, count, 97)) + [count - 1]:
        a = int(in_off[i])
        assert got["1"][i] == oracle.encode(oracle.ZLIB, data[a:a + int(in_len[i])], write_size=8192), i
