"""GPU: the crafted streams of deflate_craft.CASES and lz77_craft.CASES through the stream decoders ({deflate,zlib,gzip}::Decoder
and the non-blocking ones), whose windows start at a bit inside a byte with the last 32 KiB of earlier output as history and
decode only the blocks that are complete in the bytes held.  A reader of short reads (test_gpu_stream_dec.Chunky) cuts the
input at every byte position: blocks that open with a match into the block in front, a window relayed through forty blocks,
distance 32768 into the history, stored blocks at every bit phase as a window's first block, hundreds of empty blocks over
several windows, a reject in a later window.  Whether a case MUST take several windows is decided from the oracle's block list
alone (deflate_craft.takes_windows; the CPU tests hold that the named cases qualify), and the reader's position is recorded
at every delivery: bytes must arrive before the reader has ended, and at three positions or more where five blocks or more
produce bytes.  Every verdict is the oracle's; integer work: every comparison is exact.  A test walks all its cases and
reports every one that differs."""
import pytest

pytestmark = pytest.mark.gpu

import deflate_craft as dc
import lz77_craft as lc
import test_gpu_craft_decode as craft_decode
import test_gpu_lz77_craft_decode as lz77_decode
from deflate_craft import gzwrap, zwrap
from test_gpu_craft_decode import _report
from test_gpu_parity import ctx, ffi, lfx, synth  # noqa: F401  (fixtures)
from test_gpu_stream_dec import Chunky, drain

STEPS = (997, 4096)          # 997: a prime below every multi-block case's block size, the window cuts drift over all byte positions
WHOLE = 0                    # the whole stream in one read
M_STEP = 65536
ALL_FORMATS = craft_decode.ALL_FORMATS + lz77_decode.ALL_FORMATS + ("N_chain",)          # these also go through as zlib and gzip
HEAD = {"DEFLATE": 0, "ZLIB": 2, "GZIP": 10}
# (name, format, step) that must take several windows — the least the CPU tests promise; seen at the end of each test
MUST = [("N_chain", "DEFLATE", 997), ("G", "DEFLATE", 997), ("H", "DEFLATE", 997), ("M", "DEFLATE", M_STEP),
        ("X_relay40", "DEFLATE", 997), ("X_over_stored", "DEFLATE", 997), ("U_anchor_big", "DEFLATE", 997)]


@pytest.fixture(scope="module")
def crafted(oracle):
    """{name: [(format name, stream, the oracle's (status, output, consumed, message), the block list that decides the windows,
    the most bytes a reject may fall short by)]}.  The block list is the stream's own for a valid case and that of the
    valid blocks in front of the fault for a reject, whose last window may withhold the faulty block's output."""
    out = {}
    for corpus in (dc, lc):
        for name, (z, want) in corpus.built().items():
            verdict = oracle.decode(oracle.DEFLATE, z)
            assert (verdict[0] == 0) == (want is not None) and (want is None or verdict[1] == want), name
            if verdict[0] == 0:
                blocks, slack = oracle.scan_blocks(z), 0
            else:
                blocks = oracle.scan_blocks(corpus.valid_prefix(name))
                slack = len(verdict[1]) - sum(b[4] for b in blocks)
                assert slack >= 0
            rows = [("DEFLATE", z, verdict, blocks, slack)]
            if name in ALL_FORMATS:
                for fmt_name, s in (("ZLIB", zwrap(verdict[1], z)), ("GZIP", gzwrap(verdict[1], z))):
                    rows.append((fmt_name, s, oracle.decode(getattr(oracle, fmt_name), s), blocks, slack))
            out[name] = rows
    return out


def _decoder(lfx, fmt_name, blocky):
    return getattr(lfx.non_blocking if blocky else lfx, fmt_name.lower()).Decoder


def _stream_case(lfx, ctx, name, row, step, blocky=False, seen_windows=None):
    """one stream through one decoder → a list of what differs"""
    fmt_name, s, (orc, oout, oused, omsg), blocks, slack = row
    reader = Chunky(s, step or len(s), blocky)
    d = _decoder(lfx, fmt_name, blocky).new(reader, context=ctx)
    at = []
    status, out = drain(lfx, d, 1 << 20, lambda: at.append(reader.pos))
    label = "%s %s step %d%s" % (name, fmt_name, step, " non-blocking" if blocky else "")
    print("STREAM %-44s %4d reads, delivered at %3d reader positions, %3d of them in front of the end" %
          (label, reader.calls, len(set(at)), len(set(p for p in at if p < len(s)))))
    bad = []
    if status != orc:
        bad.append("status %d, oracle %d (%s)" % (status, orc, d._err()))
    if orc == 0:
        if out != oout:
            first = next((i for i in range(min(len(out), len(oout))) if out[i] != oout[i]), min(len(out), len(oout)))
            bad.append("bytes differ from %d (%d of %d delivered)" % (first, len(out), len(oout)))
        if d.consumed() != oused:
            bad.append("consumed %d, oracle %d" % (d.consumed(), oused))
    else:
        if d._err().split(":")[0] != omsg.split(":")[0]:
            bad.append("message %r, oracle %r" % (d._err(), omsg))
        if out != oout[:len(out)]:
            bad.append("the delivered bytes are no prefix of the oracle's")
        if len(oout) - len(out) > slack:
            bad.append("%d bytes short of the oracle's %d, the faulty block holds %d" % (len(oout) - len(out), len(oout), slack))
    # ---- not on one window
    if step and len(blocks) > 1 and dc.takes_windows(blocks, len(s), step, HEAD[fmt_name]):
        if seen_windows is not None:
            seen_windows.add((name, fmt_name, step))
        if not any(p < len(s) for p in at):
            bad.append("nothing was delivered before the reader had ended (positions %r)" % sorted(set(at))[:5])
        # (bytes are delivered where a block that produces some has ended: G's 303 blocks are two of those)
        if sum(1 for b in blocks if b[4]) >= 5 and len(set(at)) < 3:
            bad.append("delivered at %d reader positions only" % len(set(at)))
    return ["%s: %s" % (label, b) for b in bad]


def _walk(lfx, ctx, crafted, names, steps, seen):
    bad = []
    for name in names:
        for row in crafted[name]:
            for step in steps:
                bad += _stream_case(lfx, ctx, name, row, step, seen_windows=seen)
    return bad


def _groups(names, size):
    return [names[i:i + size] for i in range(0, len(names), size)]


DC_VALID = [n for n in dc.VALID if n != "M"]


@pytest.mark.parametrize("names", _groups(DC_VALID, 5) + _groups(lc.VALID, 5), ids=lambda g: g[0])
def test_valid_cases(ctx, lfx, crafted, names):
    seen = set()
    bad = _walk(lfx, ctx, crafted, names, STEPS + (WHOLE,), seen)
    for must in MUST:
        if must[0] in names and must not in seen:
            bad.append("%s %s step %d does not have to take several windows" % must)
    _report(bad)


def test_M(ctx, lfx, crafted):
    """1.5 MiB of another encoder's blocks in front of the crafted ones: at its own step only"""
    seen = set()
    bad = _walk(lfx, ctx, crafted, ["M"], (M_STEP,), seen)
    assert ("M", "DEFLATE", M_STEP) in seen
    _report(bad)


@pytest.mark.parametrize("corpus", [dc, lc], ids=["deflate_craft", "lz77_craft"])
def test_rejects(ctx, lfx, crafted, corpus):
    """the oracle's status and message; what is delivered in front of it is a prefix of the oracle's bytes that lacks at most
    the output of the block that holds the fault"""
    assert sorted(corpus.REJECTS) == sorted(n for n, _ in corpus.CASES if crafted[n][0][2][0] != 0)
    _report(_walk(lfx, ctx, crafted, corpus.REJECTS, STEPS + (WHOLE,), set()))


def test_non_blocking(ctx, lfx, crafted):
    """a reader that would block at every second call"""
    bad, seen = [], set()
    for name in ("N_chain", "X_relay40"):
        for row in crafted[name]:
            bad += _stream_case(lfx, ctx, name, row, 4096, blocky=True, seen_windows=seen)
    assert ("N_chain", "DEFLATE", 4096) in seen
    _report(bad)


def test_case_lists(crafted):
    assert sorted(crafted) == sorted([n for n, _ in dc.CASES] + [n for n, _ in lc.CASES])
    assert all(len(crafted[n]) == (3 if n in ALL_FORMATS else 1) for n in crafted)
    assert all(n in DC_VALID + lc.VALID + ["M"] for n, _f, _s in MUST)
