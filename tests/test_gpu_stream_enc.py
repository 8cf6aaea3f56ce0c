"""GPU: the stream encoder's batch backend (libflate_amd/csrc/lfx_stream_enc.cpp) at the smallest shapes at which it can go
wrong; the state machine above it is checked on the CPU (tests/c/stream_enc.cpp).  Everything byte-exact against the oracle."""
import io

import pytest

pytestmark = pytest.mark.gpu

from test_gpu_parity import ctx, ffi, lfx, synth  # noqa: F401  (fixtures)


class RunsLz77:
    """A caller's own Lz77Encode: buffers, and on flush emits literals and distance-1 runs."""

    def __init__(self):
        self.buf = bytearray()

    def encode(self, buf, sink):
        self.buf += buf

    def flush(self, sink):
        b, i = bytes(self.buf), 0
        self.buf.clear()
        while i < len(b):
            run = 0
            if i:
                while i + run < len(b) and run < 258 and b[i + run] == b[i - 1]:
                    run += 1
            if run >= 3:
                sink.append(("Pointer", run, 1))
                i += run
            else:
                sink.append(("Literal", b[i]))
                i += 1

    def compression_level(self):
        return 2

    def window_size(self):
        return 32768


class CountingSink(io.BytesIO):
    writes = 0

    def write(self, b):
        self.writes += 1
        return super().write(b)


@pytest.fixture()
def small_batches(lfx, monkeypatch):
    """a context whose stream encoders cut a batch at 1 MiB of closed blocks"""
    monkeypatch.setenv("LFX_ENC_BATCH_MB", "1")
    c = lfx.Context(0)                      # (diagnostic switches are read when a context is made)
    yield c
    c.close()


def test_three_batches_unaligned_ends_flush_and_empty_final_batch(small_batches, lfx, oracle, synth):
    """3 MiB of text in 8192-byte writes, 64 KiB blocks, 1 MiB batches: at least three batches (both staging buffers are
    reused), batch ends that are not byte-aligned (the carried byte), a flush in the middle (a drained batch), and finish
    straight after a flush: a final batch of n == 0 that holds the empty final block alone."""
    data = synth.text(3 << 20, seed=synth.SEED_BASE + 21).tobytes()
    for mod, ofmt, okw in ((lfx.gzip, oracle.GZIP, {"mtime": 0}), (lfx.zlib, oracle.ZLIB, {}), (lfx.deflate, oracle.DEFLATE, {})):
        ref = oracle.Encoder(ofmt, block_size=65536, **okw)
        sink = CountingSink()
        enc = mod.Encoder.with_options(sink, mod.EncodeOptions().block_size(65536), context=small_batches)
        header_writes = sink.writes
        for at in range(0, len(data), 8192):
            ref.write(data[at:at + 8192])
            enc.write(data[at:at + 8192])
            if at == 320 * 8192:
                # (2.5 MiB written: with 1 MiB batches the first has been collected and handed over — by the write that started
                #  the second, which is in flight; with the default 8 MiB — the switch ignored — nothing would have reached the
                #  sink yet, and the flush would hand over one batch, not two)
                assert sink.writes - header_writes == 1, sink.writes
                ref.flush()
                enc.flush()
                assert sink.writes - header_writes == 3, sink.writes   # the batch in flight, and the drained one
        ref.flush()
        enc.flush()
        want = ref.finish()
        enc.finish()
        assert sink.getvalue() == want, (ofmt, len(sink.getvalue()), len(want))
        assert sink.writes - header_writes >= 5      # (three 1 MiB batches and the two drained ones)


def test_stored_blocks_no_chunks_checksum_fork(ctx, lfx, oracle, synth):
    """300 KiB of gzip and zlib with no_compression: a plan without chunks — the parse launches nothing, and the side
    stream's checksum must still wait for the batch's H2D copy (the fork event is recorded by the parse stage itself)."""
    data = synth.text(300 << 10, seed=synth.SEED_BASE + 22).tobytes()
    for mod, ofmt, okw in ((lfx.gzip, oracle.GZIP, {"mtime": 0}), (lfx.zlib, oracle.ZLIB, {})):
        want = oracle.encode(ofmt, data, write_size=8192, no_compression=1, **okw)
        sink = io.BytesIO()
        enc = mod.Encoder.with_options(sink, mod.EncodeOptions().no_compression(), context=ctx)
        for at in range(0, len(data), 8192):
            enc.write(data[at:at + 8192])
        enc.finish()
        assert sink.getvalue() == want, (ofmt, len(sink.getvalue()), len(want))


def test_codes_mode_a_few_blocks(ctx, lfx, oracle, synth):
    """A caller's Lz77Encode through launch + immediate drain: a few blocks, a flush, zlib's sync marker."""
    data = synth.text(100000, seed=synth.SEED_BASE + 23).tobytes() + b"a" * 30000
    for mod, ofmt, okw, sync in ((lfx.gzip, oracle.GZIP, {"mtime": 0}, False), (lfx.zlib, oracle.ZLIB, {}, True)):
        okw = dict(okw, block_size=40000, **oracle.custom_lz77(RunsLz77()))
        opts = mod.EncodeOptions().with_lz77(RunsLz77()).block_size(40000)
        if sync:
            okw["zlib_sync_flush"] = 1
            opts = opts.flush_mode(lfx.zlib.FlushMode.SYNC)
        ref = oracle.Encoder(ofmt, **okw)
        sink = io.BytesIO()
        enc = mod.Encoder.with_options(sink, opts, context=ctx)
        for at in range(0, len(data), 7000):
            ref.write(data[at:at + 7000])
            enc.write(data[at:at + 7000])
            if at == 7000 * 9:
                ref.flush()
                enc.flush()
        want = ref.finish()
        enc.finish()
        assert sink.getvalue() == want, (ofmt, len(sink.getvalue()), len(want))
