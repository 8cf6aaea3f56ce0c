"""GPU: the stream decoder's state machine (lfx_stream_dec.h) over its real window backend (lfx_stream_dec.cpp), on small
inputs.  A reader that hands over short reads makes the decoder attempt a window per read, so a few hundred KB of compressed
bytes give many windows: decode ahead by the worker thread, damage and truncation in a later window, MultiDecoder with
junk behind the last member, a non-blocking reader.  (The 40 MiB ... 2 GiB cases: test_gpu_round3.py, test_gpu_round6.py.)"""
import io

import pytest

pytestmark = pytest.mark.gpu

from test_gpu_parity import ctx, enc, ffi, lfx, synth  # noqa: F401  (fixtures)


class Chunky(io.RawIOBase):
    """hands over at most `step` bytes a call; every second call WouldBlock when `blocky`"""

    def __init__(self, data, step, blocky=False):
        self.data, self.pos, self.step, self.blocky, self.calls = data, 0, step, blocky, 0

    def read(self, n=-1):
        self.calls += 1
        if self.blocky and self.calls % 2 == 0:
            return None
        k = min(self.step, n if n >= 0 else self.step)
        piece = self.data[self.pos:self.pos + k]
        self.pos += len(piece)
        return piece


def drain(lfx, d, read_size, each=None):
    """→ (status, bytes delivered in front of it)"""
    out = bytearray()
    while True:
        try:
            piece = d.read(read_size)
        except BlockingIOError:
            continue
        except lfx.deflate.StreamError as err:
            return err.status, bytes(out)
        if not piece:
            return 0, bytes(out)
        out += piece
        if each:
            each()


@pytest.fixture(scope="module")
def member(oracle, synth):
    """3 MiB of text as one gzip member of 64 KiB blocks, from the oracle"""
    plain = synth.text(3 << 20, seed=synth.SEED_BASE + 21).tobytes()
    return plain, oracle.encode(oracle.GZIP, plain, block_size=65536, write_size=4096, mtime=0)


def test_decode_ahead_on_a_chunked_reader(ctx, lfx, ffi, synth):
    """24 MiB of LOWENT as zlib (schedule S8K, under 1 MiB compressed) through a reader of 200 000 bytes a call, read 8192
    bytes at a time.  The first window is the header pull plus the first hand-over, 265 534 bytes, and yields 7 MiB, above the
    4 MiB decode-ahead threshold; three more windows of 6, 6 and 5 MiB follow.  Seen once with LFX_DEBUG=1: those four
    `[lfx] window:` lines, equal to the parent commit's, and one more thread in the process right after a read than before
    the decoder was made — the worker with a later window."""
    plain = synth.lowent(24 << 20).tobytes()
    z = enc(ctx, ffi, ffi.ZLIB, plain, 8192)
    assert len(z) < (1 << 20)
    d = lfx.zlib.Decoder.new(Chunky(z, 200000), context=ctx)
    peak = [0]

    def watch():
        peak[0] = max(peak[0], ffi.lib().lfx_decoder_buffered(d._h))
    status, out = drain(lfx, d, 8192, watch)
    assert status == 0 and out == plain
    assert d.consumed() == len(z)
    assert peak[0] <= (256 << 20)


def test_damage_in_a_later_window(ctx, lfx, oracle, member):
    plain, z = member
    status, out = drain(lfx, lfx.gzip.Decoder.new(Chunky(z, 100000), context=ctx), 1 << 20)
    assert status == 0 and out == plain
    at = len(z) * 6 // 10
    for kind in ("flip", "cut"):
        bad = bytearray(z)
        if kind == "flip":
            bad[at] ^= 0x10
        else:
            del bad[at:]
        orc, oout, _used, _msg = oracle.decode(oracle.GZIP, bytes(bad))
        assert orc != 0
        status, out = drain(lfx, lfx.gzip.Decoder.new(Chunky(bytes(bad), 100000), context=ctx), 1 << 20)
        assert status == orc, (kind, status, orc)
        assert out == oout[:len(out)], kind
        assert len(oout) - len(out) <= 65536 + 4096, (kind, len(out), len(oout))   # at most the damaged block's own bytes


def test_multidecoder_with_junk_behind_the_members(ctx, lfx, ffi, member):
    plain, z = member
    data = z + z + bytes(range(100, 200))
    rc, want, _used, _msg = ctx.decode_host(ffi.GZIP, data, flags=ffi.DEC_MULTI)
    status, out = drain(lfx, lfx.gzip.MultiDecoder.new(Chunky(data, 100000), context=ctx), 1 << 20)
    assert status == rc
    assert out == plain + plain and want[:len(out)] == out


def test_non_blocking_reader(ctx, lfx, member):
    plain, z = member
    d = lfx.non_blocking.gzip.Decoder.new(Chunky(z, 100000, blocky=True), context=ctx)
    while True:
        try:
            h = d.header()
            break
        except BlockingIOError:
            pass
    assert h["modification_time"] == 0 and h["filename"] is None
    status, out = drain(lfx, d, 1 << 20)
    assert status == 0 and out == plain
