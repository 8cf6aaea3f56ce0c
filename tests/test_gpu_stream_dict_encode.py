"""GPU: the stream encoder with a preset dictionary (include/lfx.h "the stream encoder with a preset dictionary").
The expected bytes come from the models over the oracle — dict_encode_model (default parse), dict_chain_model (chain, lazy),
level_model (levels) as Lz77Encodes of the oracle's generic encoder, driven with the same writes and flushes — never from the
library.  Every stream is also compared byte for byte with lfx_encode_dict_host under the same schedule, and read back by
zlib.decompressobj(zdict=...) and by this package's stream decoder.  Integer work: every comparison is exact.  Small shapes:
a few KiB, but for the cases that need a second chunk (600 KiB) or a second batch (1 MiB batches)."""
import ctypes as C
import io
import zlib

import pytest

pytestmark = pytest.mark.gpu

import dict_chain_model as dcm
import dict_encode_model as dm
import level_model as lvm
from test_dict_encode_model import _rand, _text
from test_gpu_encode_stages import context_with
from test_gpu_parity import ctx, ffi, lfx, synth  # noqa: F401  (fixtures)

KIB = 1 << 10
TEXT = _text(48 * KIB, 81)
D32 = TEXT[:32768]
REC = D32[-400:] + TEXT[40000:42000] + D32[9000:9400] + D32[:200] + b"a" * 300
FMTS = ("zlib", "deflate")
FLUSH = None


@pytest.fixture(scope="module")
def dicts(lfx, ctx):
    """one Dictionary per distinct dictionary, kind of object and context, made once"""
    made = {}

    def get(zdict, c=ctx, chain=False):
        key = (zdict, id(c), chain)
        if key not in made:
            made[key] = lfx.Dictionary(zdict, c, chain=chain)
        return made[key]
    yield get
    for d in made.values():
        d.close()


# ---- the parse of a case: the package's options, and the model's Lz77Encode for the oracle
def default_parse(lfx, oracle, zdict, **okw):
    return (lambda mod: mod.EncodeOptions(),
            lambda: dm.PrimedLz77(oracle, zdict, okw.get("window_size", 32768), okw.get("max_length", 258)), False)


def chained_parse(lfx, zdict, kind, depth):
    cls = lfx.lz77.LazyLz77Encoder if kind == dcm.LAZY else lfx.lz77.ChainLz77Encoder
    return (lambda mod: mod.EncodeOptions(cls(depth)), lambda: dcm.PrimedChainLz77(zdict, kind, depth), True)


def level_parse(lfx, zdict, level):
    return (lambda mod: mod.EncodeOptions(lfx.lz77.LevelLz77Encoder(level)), lambda: lvm.LevelLz77(level, T=bytes(zdict)), True)


def expected(oracle, name, zdict, events, model, **okw):
    """the oracle's encoder over the model's Lz77Encode, driven with the events (bytes: a write; FLUSH) → the stream with the
    FDICT header.  model None: the oracle's own body (options that do no matching)."""
    if model is not None:
        okw = dict(okw, **oracle.custom_lz77(model()))
    e = oracle.Encoder(oracle.ZLIB if name == "zlib" else oracle.DEFLATE, **okw)
    for ev in events:
        if ev is FLUSH:
            e.flush()
        else:
            e.write(ev)
    z = e.finish()
    if name == "deflate":
        return z
    cmf, flg = z[0], (z[1] & 0xC0) | 0x20
    if ((cmf << 8) + flg) % 31:
        flg += 31 - ((cmf << 8) + flg) % 31
    return bytes([cmf, flg]) + zlib.adler32(bytes(zdict)).to_bytes(4, "big") + z[2:]


def run_stream(lfx, c, name, zd, events, options):
    mod = lfx.zlib if name == "zlib" else lfx.deflate
    sink = io.BytesIO()
    enc = mod.Encoder.new(sink, context=c, options=options, zdict=zd)
    assert len(sink.getvalue()) == (6 if name == "zlib" else 0)          # the header goes out in the constructor
    for ev in events:
        if ev is FLUSH:
            enc.flush()
        else:
            assert enc.write(ev) == len(ev)
    enc.finish()
    return sink.getvalue()


def check(lfx, ffi, c, oracle, dicts, zdict, events, parse=None, names=FMTS, one_shot=True, tweak=None, **okw):
    """both formats: the stream encoder's bytes are the model's, lfx_encode_dict_host's under the same schedule, and python-zlib
    and the stream decoder read them back.  tweak(options): further builder calls; okw: the same options for the oracle."""
    mk_opts, model, chain = parse if parse is not None else default_parse(lfx, oracle, zdict, **okw)
    zd = dicts(zdict, c, chain)
    data = b"".join(ev for ev in events if ev is not FLUSH)
    streams = []
    for name in names:
        mod, fmt = (lfx.zlib, ffi.ZLIB) if name == "zlib" else (lfx.deflate, ffi.DEFLATE)
        options = mk_opts(mod)
        if tweak:
            tweak(options)
        got = run_stream(lfx, c, name, zd, events, options)
        want = expected(oracle, name, zdict, events, model, **okw)
        assert got == want, (name, len(zdict), [len(ev) if ev is not FLUSH else "flush" for ev in events][:8], len(got), len(want))
        if one_shot:
            sched = ffi.make_schedule(writes=[None if ev is FLUSH else len(ev) for ev in events])
            assert c.encode_dict_host(fmt, zd, data, options._to_c(), sched) == got, (name, "lfx_encode_dict_host")
        assert dm.py_inflate(name, got, zdict) == data
        assert mod.Decoder.new(got, context=c, zdict=zd).read_to_end() == data
        streams.append(got)
    return streams[0]             # (of names[0]: zlib unless the case says otherwise)


# ---- formats and parses
def test_default_parse_plain_dictionary(lfx, ffi, ctx, oracle, dicts):
    got = check(lfx, ffi, ctx, oracle, dicts, D32, [REC])
    assert len(got) < len(lfx.deflate.compress(REC, context=ctx))        # (the dictionary is used: the record's head is its tail)


@pytest.mark.parametrize("which", ["chain8", "lazy8", "level6"])
def test_chained_parses_chain_dictionary(lfx, ffi, ctx, oracle, dicts, which):
    parse = {"chain8": lambda: chained_parse(lfx, D32, dcm.CHAIN, 8), "lazy8": lambda: chained_parse(lfx, D32, dcm.LAZY, 8),
             "level6": lambda: level_parse(lfx, D32, 6)}[which]()
    check(lfx, ffi, ctx, oracle, dicts, D32, [REC], parse)
    check(lfx, ffi, ctx, oracle, dicts, D32, [REC[:1500], FLUSH, REC[1500:]], parse)      # the second chunk is not primed


@pytest.mark.parametrize("m", [0, 1, 2, 3, 32768, 40000])
def test_dictionary_lengths(lfx, ffi, ctx, oracle, dicts, m):
    """32768: the whole window; 40000: the tail primes and the id covers all bytes; 0: an empty dictionary primes nothing and
    the header still carries FDICT and the id 1"""
    zdict = TEXT[:m]
    rec = zdict[-300:] + TEXT[41000:41300] + zdict[:200] + zdict[-32768:][:64] + TEXT[41000:41100]
    got = check(lfx, ffi, ctx, oracle, dicts, zdict, [rec], names=("zlib",))
    assert got[1] & 0x20 and got[2:6] == zlib.adler32(zdict).to_bytes(4, "big")
    check(lfx, ffi, ctx, oracle, dicts, zdict, [zdict[-2:] + zdict[-5:] * 3 + b"xyz"])


@pytest.mark.parametrize("n", [0, 1, 2, 3, 5])
def test_record_lengths(lfx, ffi, ctx, oracle, dicts, n):
    check(lfx, ffi, ctx, oracle, dicts, D32, [D32[-5:][:n]])
    check(lfx, ffi, ctx, oracle, dicts, D32, [D32[-5:][:n]], chained_parse(lfx, D32, dcm.LAZY, 8))


def test_straddling_prefix_and_match_from_the_dictionary(lfx, ffi, ctx, oracle, dicts):
    # T ends "ab", the chunk begins "cabcabc": its first two bytes complete the prefix at |T|-2
    assert dm.primed_codes(b"..xyzab", b"cabcabc..")[1] == (6 << 16) | 3
    check(lfx, ffi, ctx, oracle, dicts, b"..xyzab", [b"cabcabc.."])
    check(lfx, ffi, ctx, oracle, dicts, b"..xyza", [b"bcQabcR.."])
    check(lfx, ffi, ctx, oracle, dicts, b"..xyzab", [b"c", b"abcabc.."])          # (two writes, one chunk)
    # a match that starts in the dictionary and runs on into the data
    assert dm.primed_codes(b"a" * 100, b"a" * 600)[0] == (258 << 16) | 1
    check(lfx, ffi, ctx, oracle, dicts, b"a" * 100, [b"a" * 600])
    assert dm.primed_codes(b"..hello", b"hellohello!")[0] >> 16 == 10
    check(lfx, ffi, ctx, oracle, dicts, b"..hello", [b"hellohello!"])


# ---- schedules
def test_8k_writes_over_600k_three_chunks_first_primed(lfx, ffi, ctx, oracle, dicts, synth):
    """600 KiB in 8 KiB writes: chunks of 256, 256 and 88 KiB in one block; the first alone is primed — the second and the third
    begin with the dictionary's tail too, and the model parses them cold"""
    body = synth.text(600 * KIB, seed=synth.SEED_BASE + 41).tobytes()
    data = bytearray(body)
    for at in (0, 256 * KIB, 512 * KIB):
        data[at:at + 600] = D32[-600:]
    data = bytes(data)
    check(lfx, ffi, ctx, oracle, dicts, D32, [data[at:at + 8192] for at in range(0, len(data), 8192)], names=("zlib",))


def test_flushes(lfx, ffi, ctx, oracle, dicts):
    """a flush before the first byte (the empty block's empty chunk is the stream's first chunk, as in the one-shot call and the
    model: nothing behind it is primed), after one byte, and in mid-stream with zlib's sync marker"""
    sync = lambda o: o.flush_mode(lfx.zlib.FlushMode.SYNC)
    for events in ([FLUSH, REC], [REC[:1], FLUSH, REC[1:]], [REC[:1700], FLUSH, REC[1700:]], [b"", b"", b"", REC], [FLUSH, FLUSH, REC, FLUSH]):
        check(lfx, ffi, ctx, oracle, dicts, D32, events)
        check(lfx, ffi, ctx, oracle, dicts, D32, events, names=("zlib",), tweak=sync, zlib_sync_flush=1)
    got = check(lfx, ffi, ctx, oracle, dicts, D32, [REC[:1700], FLUSH, REC[1700:]], names=("zlib",), tweak=sync, zlib_sync_flush=1)
    assert b"\x00\x00\xff\xff" in got
    check(lfx, ffi, ctx, oracle, dicts, D32, [])                                   # finish with nothing written


@pytest.fixture(scope="module")
def small_batches(lfx):
    """a context whose stream encoders cut a batch at 1 MiB of closed blocks (tests/test_gpu_stream_enc.py's means)"""
    c = context_with(lfx, LFX_ENC_BATCH_MB="1")
    yield c
    c.close()


@pytest.mark.parametrize("empty_flush_first", [False, True])
def test_more_than_one_batch(lfx, ffi, small_batches, oracle, dicts, synth, empty_flush_first):
    """2.5 MiB in 8 KiB writes, 64 KiB blocks, 1 MiB batches: the primed chunk is in batch 0 of three; with a flush first, the
    first batch holds the empty block alone, whose empty chunk takes the priming"""
    data = bytearray(synth.text(2560 * KIB, seed=synth.SEED_BASE + 42).tobytes())
    for at in (0, 64 * KIB, 1024 * KIB, 2048 * KIB):                               # (later chunks and batches begin with the tail too)
        data[at:at + 600] = D32[-600:]
    data = bytes(data)
    events = ([FLUSH] if empty_flush_first else []) + [data[at:at + 8192] for at in range(0, len(data), 8192)]

    class Counting(io.BytesIO):
        writes = 0

        def write(self, b):
            self.writes += 1
            return super().write(b)
    sink = Counting()
    enc = lfx.zlib.Encoder.new(sink, context=small_batches, options=lfx.zlib.EncodeOptions().block_size(65536), zdict=dicts(D32, small_batches))
    for ev in events:
        enc.flush() if ev is FLUSH else enc.write(ev)
    enc.finish()
    assert sink.writes >= 4 + empty_flush_first                                    # header, three batches or more, trailer
    got = sink.getvalue()
    assert got == expected(oracle, "zlib", D32, events, default_parse(lfx, oracle, D32)[1], block_size=65536)
    assert dm.py_inflate("zlib", got, D32) == data
    sched = ffi.make_schedule(writes=[None if ev is FLUSH else len(ev) for ev in events])
    opts = lfx.zlib.EncodeOptions().block_size(65536)._to_c()
    assert small_batches.encode_dict_host(ffi.ZLIB, dicts(D32, small_batches), data, opts, sched) == got


# ---- options
def test_no_compression_fixed_codes_auto(lfx, ffi, ctx, oracle, dicts):
    events = [REC[:1700], FLUSH, REC[1700:]]
    got = check(lfx, ffi, ctx, oracle, dicts, D32, events, (lambda mod: mod.EncodeOptions().no_compression(), None, False), no_compression=1)
    assert got[:2] == b"\x78\x20" and got[2:6] == zlib.adler32(D32).to_bytes(4, "big")       # FLEVEL 0, FDICT; the code words unchanged
    check(lfx, ffi, ctx, oracle, dicts, D32, events,
          (lambda mod: mod.EncodeOptions(lfx.lz77.NoCompressionLz77Encoder()), None, False), lz77_kind=oracle.LZ77_NOCOMPRESSION)
    check(lfx, ffi, ctx, oracle, dicts, D32, events, tweak=lambda o: o.fixed_huffman_codes(), dynamic_huffman=0)
    # AUTO has no oracle option: its bytes are the one-shot call's, which test_gpu_auto_blocks.py holds against its model
    for name, mod, fmt in (("zlib", lfx.zlib, ffi.ZLIB), ("deflate", lfx.deflate, ffi.DEFLATE)):
        options = mod.EncodeOptions().auto_huffman_codes()
        got = run_stream(lfx, ctx, name, dicts(D32), events, options)
        sched = ffi.make_schedule(writes=[None if ev is FLUSH else len(ev) for ev in events])
        assert got == ctx.encode_dict_host(fmt, dicts(D32), REC, options._to_c(), sched)
        assert len(got) <= len(run_stream(lfx, ctx, name, dicts(D32), events, mod.EncodeOptions()))
        assert dm.py_inflate(name, got, D32) == REC


def test_codes_mode_fed_with_the_models_code_words(lfx, ffi, ctx, oracle, dicts):
    """a caller's own Lz77Encode — the model — on an encoder made with a dictionary: the header carries FDICT and DICTID, the
    code words (Pointers in front of byte 0 among them) are Huffman-coded as they come: the bytes-mode stream's bytes"""
    events = [REC[:1700], FLUSH, REC[1700:]]
    assert dm.primed_codes(D32, REC[:1700])[0] & 0xFFFF                # the first code word is a Pointer in front of byte 0
    for name in FMTS:
        mod = lfx.zlib if name == "zlib" else lfx.deflate
        bytes_mode = run_stream(lfx, ctx, name, dicts(D32), events, mod.EncodeOptions())
        codes_mode = run_stream(lfx, ctx, name, dicts(D32), events, mod.EncodeOptions().with_lz77(dm.PrimedLz77(oracle, D32)))
        assert codes_mode == bytes_mode == expected(oracle, name, D32, events, lambda: dm.PrimedLz77(oracle, D32))


def test_dictionary_less_encoder_before_and_after(lfx, ffi, ctx, oracle, dicts):
    """nothing of a dictionary encoder stays in the context: the dictionary-less encoder writes the oracle's bytes"""
    events = [REC[:1700], FLUSH, REC[1700:]]

    def plain(mod, ofmt, **kw):
        sink = io.BytesIO()
        enc = mod.Encoder.new(sink, context=ctx, **kw)
        ref = oracle.Encoder(ofmt)
        for ev in events:
            if ev is FLUSH:
                enc.flush(), ref.flush()
            else:
                enc.write(ev), ref.write(ev)
        enc.finish()
        assert sink.getvalue() == ref.finish()
    for _ in range(2):
        plain(lfx.zlib, oracle.ZLIB)
        check(lfx, ffi, ctx, oracle, dicts, D32, events, one_shot=False)
        plain(lfx.deflate, oracle.DEFLATE)
        check(lfx, ffi, ctx, oracle, dicts, D32, events, chained_parse(lfx, D32, dcm.LAZY, 8), one_shot=False)
        plain(lfx.zlib, oracle.ZLIB, zdict=None)                                   # (dict == NULL: lfx_encoder_new's bytes)
    # the C call itself with dict == NULL
    got = []
    w = ffi.WRITE_CB(lambda user, p, n: got.append(C.string_at(p, n)) or n)
    f = ffi.FLUSH_CB(lambda user: 0)
    st = C.c_int(77)
    L = ffi.lib()
    h = L.lfx_encoder_new_dict(ctx.handle, ffi.ZLIB, None, None, w, f, None, C.byref(st))
    assert h and st.value == ffi.OK and got == [b"\x78\x9c"]
    assert L.lfx_encoder_write(h, REC, len(REC)) == len(REC) and L.lfx_encoder_finish(h) == ffi.OK
    L.lfx_encoder_free(h)
    assert b"".join(got) == oracle.encode(oracle.ZLIB, REC)


# ---- refusals
def test_refusals(lfx, ffi, ctx, dicts):
    plain, chain = dicts(D32), dicts(D32, chain=True)
    for enc, word in ((lfx.lz77.ChainLz77Encoder(8), "LFX_LZ77_CHAIN"), (lfx.lz77.LazyLz77Encoder(8), "LFX_LZ77_LAZY"),
                      (lfx.lz77.LevelLz77Encoder(6), "LFX_LZ77_LEVEL")):
        for mod in (lfx.zlib, lfx.deflate):
            sink = io.BytesIO()
            with pytest.raises(lfx.zlib.StreamError) as e:
                mod.Encoder.new(sink, context=ctx, options=mod.EncodeOptions(enc), zdict=plain)
            assert e.value.status == ffi.E_UNSUPPORTED and sink.getvalue() == b""
            assert "lz77_kind: %s with a preset dictionary is not supported (a dictionary made by lfx_dict_new_chain serves it)" % word in e.value.message
    for zd in (plain, chain):                              # block_merge: the stream encoder's own reason, in front of the dictionary's
        with pytest.raises(lfx.zlib.StreamError) as e:
            lfx.zlib.Encoder.new(io.BytesIO(), context=ctx, options=lfx.zlib.EncodeOptions(lfx.lz77.ChainLz77Encoder(8)).merge_blocks(), zdict=zd)
        assert e.value.status == ffi.E_UNSUPPORTED and "block_merge: the stream encoder does not serve block_merge" in e.value.message
    # gzip, whatever the dictionary; a foreign context's dictionary
    got = []
    w = ffi.WRITE_CB(lambda user, p, n: got.append(n) or n)
    f = ffi.FLUSH_CB(lambda user: 0)
    L = ffi.lib()
    for handle in (None, plain.handle):
        st = C.c_int(77)
        assert L.lfx_encoder_new_dict(ctx.handle, ffi.GZIP, None, handle, w, f, None, C.byref(st)) is None and st.value == ffi.E_ARG
    with pytest.raises(TypeError):
        lfx.gzip.Encoder.new(io.BytesIO(), context=ctx, zdict=D32)
    other = lfx.Context(0)
    try:
        for fmt in (ffi.ZLIB, ffi.DEFLATE):
            st = C.c_int(77)
            assert L.lfx_encoder_new_dict(other.handle, fmt, None, plain.handle, w, f, None, C.byref(st)) is None and st.value == ffi.E_ARG
        with pytest.raises(lfx.zlib.StreamError) as e:
            lfx.zlib.Encoder.new(io.BytesIO(), context=other, zdict=plain)
        assert e.value.status == ffi.E_ARG and "a dictionary of another context" in e.value.message
    finally:
        other.close()
    assert got == []                                       # no refused call reached the sink


# ---- the Python classes
def test_python_classes(lfx, ffi, ctx, oracle, dicts):
    for name, mod in (("zlib", lfx.zlib), ("deflate", lfx.deflate)):
        want = dm.expected_stream(oracle, name, D32, REC)
        for zd in (D32, dicts(D32)):                       # bytes, and a Dictionary
            sink = io.BytesIO()
            enc = mod.Encoder.new(sink, context=ctx, zdict=zd)
            enc.write_all(REC)
            assert enc.finish() is sink and sink.getvalue() == want
            sink = io.BytesIO()
            enc = mod.Encoder.with_options(sink, mod.EncodeOptions(), context=ctx, zdict=zd)
            enc.write(REC)
            enc.finish()
            assert sink.getvalue() == want
        # a level with bytes: the class makes the chain dictionary itself, as compress(data, zdict=bytes, level=6) does
        sink = io.BytesIO()
        enc = mod.Encoder.new(sink, context=ctx, options=mod.EncodeOptions(lfx.lz77.LevelLz77Encoder(6)), zdict=D32)
        assert enc._zdict.chain
        enc.write(REC)
        enc.finish()
        assert sink.getvalue() == lvm.expected_dict_stream(oracle, name, D32, REC, 6) == mod.compress(REC, zdict=D32, level=6, context=ctx)
        assert enc._zdict is None                          # (the encoder's own dictionary went with it)
