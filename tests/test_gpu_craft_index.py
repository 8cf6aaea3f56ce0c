"""GPU: the crafted streams of deflate_craft.CASES and lz77_craft.CASES through the seek index: lfx_decode_index_device (the
build must equal lfx_decode_device AND the oracle), the points and their windows, and lfx_index_read_device, whose segments
start at symbol boundaries inside such blocks, seed a 32 KiB window that the first match behind a point reads to its first
byte (W_32768), and meet codes that produce more output than one candidate bucket (C1, T_all258 at the ABI's least spacing).
Every stream's verdict is fixed by the oracle on the CPU first (test_craft_streams.py, test_lz77_craft_streams.py).  Integer
work: every comparison is exact.  A test walks all its cases and reports every one that differs."""
import pytest

pytestmark = pytest.mark.gpu

import deflate_craft as dc
import lz77_craft as lc
import test_gpu_craft_decode as craft_decode
import test_gpu_lz77_craft_decode as lz77_decode
from deflate_craft import MIB, gzwrap, zwrap
from test_gpu_craft_decode import GUARD, _report
from test_gpu_index import build, check_points, partial_input_from_inside_a_block, reads_match, windows_match
from test_gpu_members import _dev, torch  # noqa: F401
from test_gpu_parity import ctx, ffi, lfx, synth  # noqa: F401  (fixtures)

SPACING_MIN, SPACING_WIDE = 4096, 65536
# The least spacing wherever the windows of one index (32 KiB a point) stay under 50 MB.  The outputs of C1, E1 (1.16 MB) and
# X_relay40 (1.34 MB) are 10 MB of windows at 4096: they stay at the least spacing, where a candidate bucket (256 bytes) is
# shorter than one code (258).  M's 5.9 MB would be 47 MB: the wide spacing.
WIDE_FROM = 2 * MIB
ALL_FORMATS = craft_decode.ALL_FORMATS + lz77_decode.ALL_FORMATS          # these also go through as zlib and gzip
SENTINEL = 0x6B

# The cases the serial kernel decodes keep only their start point, by design: every stream under 4 KiB, and ...
SERIAL = {"G": "300 empty blocks in a row cost the serial walk (DESIGN §4)", "G_small": "under 4 KiB"}
# max_gap above the spacing, with the bound that holds instead and why.  (test_gpu_index.py passes gap_bound=False for its
# stored streams for the first reason.)
OVER_SPACING = {
    "H": (65535, "a stored block has no symbol boundary inside: max_gap is the longest stored block"),
    "X_over_stored": (20000, "likewise: its stored block of 20000 bytes"),
    # The candidates inside a block are the scan's proved LANE starts (lfx_index.hip, idx_finish: one per lane of a BlkLanes
    # slot, thinned to the first in each spacing / 16 bytes), not code boundaries, so candidates lie up to one lane's output
    # apart.  This block is 295 Kbit in a stream of five blocks: one workgroup of the 256-lane instance, 1153 bits a lane; a
    # match at distance 32766 .. 32768 is at least 8 + 4 + 13 bits for up to 258 bytes: 46 codes, 11.9 KB a lane at the most.
    # Measured on the MI355X: 7926 and 8217.
    "W_32768_lits": (256 + 47 * 258, "one lane of the 256-lane scan decodes up to 47 matches"),
    "W_near_ring_lits": (256 + 47 * 258, "likewise"),
}
# The cases that must have points inside blocks: one or a few blocks of more than 4096 bytes on the block-parallel path.
INNER = ["A", "B", "C1", "C2", "D", "E1", "E2", "E2_span", "E3", "E4_hclen5", "E4_hclen_field4", "E4_hclen19", "E4_wide_step", "M",
         "N_chain"] + lc.DIRECT
# Two consecutive in-block points of these should fall less than a bucket (spacing / 16) and two codes of 258 bytes short of
# the spacing: the selection takes the last candidate within the spacing, so a larger shortfall is a gap between candidates.
ONE_CODE = ("C1", "T_all258")
# Cases that do not meet their INNER / ONE_CODE assertion on the MI355X, with the reason read from the code.  Both keep the
# assertions that points inside blocks exist, that two of them are consecutive, and max_gap <= spacing.
OTHER = {
    "C1": "ONE_CODE: falls 2543 bytes short, not under 772.  The candidates of lfx_decode_index_device are the block scan's "
          "proved lane starts (idx_finish reads one (bit, output offset) per lane of a BlkLanes slot), not the first code "
          "boundary of each bucket, which is lfx_encode_index_device's rule.  Its block of 98 Kbit is 96 bits a lane, and 96 "
          "bits hold up to nineteen (258, 1) of 5 bits: a lane can produce 4.9 KB",
    "T_all258": "ONE_CODE: falls 2290 bytes short.  Likewise: 84 Kbit, 82 bits a lane, a match of 258 bytes is 13 to 21 bits: up "
                "to six of them, 1.5 KB, a lane, and a lane whose start the scan did not prove is left out",
}
assert len(OTHER) <= 3


def spacing_of(out):
    return SPACING_MIN if len(out) < WIDE_FROM else SPACING_WIDE


@pytest.fixture(scope="module")
def crafted(oracle):
    """{name: (raw DEFLATE, (status, output, consumed, message) of the oracle)} of both corpora"""
    out = {}
    for corpus in (dc, lc):
        for name, (z, want) in corpus.built().items():
            verdict = oracle.decode(oracle.DEFLATE, z)
            assert (verdict[0] == 0) == (want is not None) and (want is None or verdict[1] == want), name
            assert name not in out
            out[name] = (z, verdict)
    return out


def _containers(oracle, name, z, verdict):
    yield "DEFLATE", z, verdict
    if name in ALL_FORMATS:
        for fmt_name, s in (("ZLIB", zwrap(verdict[1], z)), ("GZIP", gzwrap(verdict[1], z))):
            yield fmt_name, s, oracle.decode(getattr(oracle, fmt_name), s)


def _built(ctx, ffi, torch, fmt_name, s, verdict, spacing):
    """test_gpu_index.build (build == decode_device), then both against the oracle → the index, or None for a reject"""
    orc, oout, oused, omsg = verdict
    rc, out, idx = build(ctx, ffi, torch, s, getattr(ffi, fmt_name), spacing, cap=len(oout) + GUARD)
    assert (rc, len(out)) == (orc, len(oout)), "(status, out_len) %r, oracle %r" % ((rc, len(out)), (orc, len(oout)))
    assert out == oout, "bytes differ from %d" % next(i for i in range(len(out)) if out[i] != oout[i])
    assert (idx is None) == (orc != 0)
    if orc != 0:
        assert ctx.last_error().split(":")[0] == omsg.split(":")[0], (ctx.last_error(), omsg)
    return idx


def point_reads(pts, ol):
    """around up to forty points inside blocks and forty block starts: the point's byte, the byte in front, 600 bytes from
    the point and 600 around it, clamped to the output"""
    inner = [p for p in pts if p[0] != p[1]][:40]
    starts = [p for p in pts if p[0] == p[1]][:40]
    ranges = []
    for p in inner + starts:
        o = p[2]
        for a, b in ((o, o + 1), (o - 1, o + 1), (o, o + 600), (o - 300, o + 300)):
            a, b = max(a, 0), min(b, ol)
            ranges.append((a, max(b - a, 0)))
    return ranges


def guarded_reads(ctx, ffi, torch, idx, s, out, ranges):
    """ONE lfx_index_read_device call, the outputs at byte phases 0 .. 3 with sentinel bytes between them: the bytes are the
    oracle's and nothing outside [out_off, out_off + len) changes"""
    offs, at = [], 16
    for i, (o, ln) in enumerate(ranges):
        at = ((at + 3) & ~3) + i % 4
        offs.append(at)
        at += ln + 16
    d_in = _dev(torch, s)
    d_out = torch.full((at + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    rc, lens, st, msg = ctx.index_read_device(idx._h, d_in.data_ptr(), 0, len(s), [o for o, _ in ranges], [ln for _, ln in ranges],
                                              d_out.data_ptr(), offs)
    assert rc == ffi.OK and st == [ffi.OK] * len(ranges), (rc, st, msg)
    host = d_out.cpu().numpy().tobytes()
    want = bytearray([SENTINEL]) * len(host)
    for (o, ln), at, got in zip(ranges, offs, lens):
        assert got == len(out[o:o + ln]), (o, ln, got)
        want[at:at + got] = out[o:o + ln]
    if host != bytes(want):
        first = next(i for i in range(len(host)) if host[i] != want[i])
        k = max(i for i, at in enumerate(offs) if at <= first) if first >= offs[0] else -1
        inside = k >= 0 and first < offs[k] + lens[k]
        raise AssertionError("%s at byte %d (read %d: %r at %d)" % ("bytes differ" if inside else "written outside a read's output", first, k,
                                                                 ranges[k] if k >= 0 else None, offs[max(k, 0)]))


def inner_points(name, pts, spacing):
    """points inside blocks exist where they must; for ONE_CODE the candidates are as dense as the rule says: the selection
    takes the LAST candidate within `spacing` of a point, so the next candidate lies behind point + spacing, and a point
    that falls more than a bucket and two codes short of point + spacing has no candidate that near behind it"""
    inner = [p for p in pts if p[0] != p[1]]
    short = 0
    for a, b, c in zip(pts, pts[1:], pts[2:]):
        if a[0] != a[1] and b[0] != b[1] and a[1] == b[1] == c[1]:
            short = max(short, a[2] + spacing - b[2])
    print("INNER %-16s spacing %5d: %4d points, %4d inside blocks, falls short of the spacing by at most %d" % (name, spacing, len(pts), len(inner), short))
    if name in INNER and name not in OTHER:
        assert inner, "no point inside a block"
    if name in ONE_CODE:
        assert sum(1 for a, b in zip(pts, pts[1:]) if a[0] != a[1] and b[0] != b[1]) >= 1, "no two consecutive points inside a block"
    if name in ONE_CODE and name not in OTHER:
        assert short < spacing // 16 + 2 * 258, "consecutive in-block points fall %d short of the spacing" % short


def _valid_case(ctx, ffi, oracle, torch, name, z, verdict):
    bad = []
    for fmt_name, s, v in _containers(oracle, name, z, verdict):
        label = "%s %s" % (name, fmt_name)
        idx = None
        try:
            out = v[1]
            spacing = spacing_of(out)
            idx = _built(ctx, ffi, torch, fmt_name, s, v, spacing)
            start_only = len(z) < 4096 or name in SERIAL
            loose = start_only or name in OVER_SPACING
            pts = check_points(idx, out, spacing, gap_bound=not loose)
            info = idx.info
            print("INDEX %-24s spacing %5d: out %8d, %4d points, max_gap %d" % (label, spacing, len(out), info["n_points"], info["max_gap"]))
            if start_only:
                assert info["n_points"] == info["n_members"] == 1 and info["max_gap"] == len(out), (info["n_points"], info["max_gap"])
            elif name in OVER_SPACING:
                assert spacing < info["max_gap"] <= OVER_SPACING[name][0], (info["max_gap"], OVER_SPACING[name])
            windows_match(ctx, idx, out)
            inner_points(name, pts, spacing)
            reads_match(ctx, ffi, torch, idx, s, out, n_reads=300)
            ranges = point_reads(pts, len(out)) + [(0, len(out))]
            for (o, ln), got in zip(ranges, idx.read_many(s, ranges)):
                assert got.cpu().numpy().tobytes() == out[o:o + ln], "read (%d, %d) differs" % (o, ln)
            guarded_reads(ctx, ffi, torch, idx, s, out, ranges[:64])
        except AssertionError as e:
            bad.append("%s: %s" % (label, str(e).split("\n")[0] or repr(e)))
        finally:
            if idx is not None:
                idx.close()
    return bad


def _groups(names, size):
    return [names[i:i + size] for i in range(0, len(names), size)]


DC_VALID = [n for n in dc.VALID if n != "M"]


@pytest.mark.parametrize("names", _groups(DC_VALID, 5), ids=lambda g: g[0])
def test_deflate_craft_valid(ctx, ffi, oracle, torch, crafted, names):
    bad = []
    for name in names:
        bad += _valid_case(ctx, ffi, oracle, torch, name, *crafted[name])
    _report(bad)


def test_deflate_craft_M(ctx, ffi, oracle, torch, crafted):
    _report(_valid_case(ctx, ffi, oracle, torch, "M", *crafted["M"]))


@pytest.mark.parametrize("names", _groups(lc.VALID, 5), ids=lambda g: g[0])
def test_lz77_craft_valid(ctx, ffi, oracle, torch, crafted, names):
    bad = []
    for name in names:
        bad += _valid_case(ctx, ffi, oracle, torch, name, *crafted[name])
    _report(bad)


def test_case_lists(crafted):
    assert sorted(DC_VALID + ["M"] + dc.REJECTS + lc.VALID + lc.REJECTS) == sorted(crafted)
    assert set(INNER) <= set(dc.VALID + lc.VALID) and set(ONE_CODE) <= set(INNER) and set(OTHER) <= set(INNER)
    assert not set(INNER) & set(SERIAL) and not any(len(crafted[n][0]) < 4096 for n in INNER)
    assert [n for n in crafted if crafted[n][1][0] == 0 and len(crafted[n][1][1]) >= WIDE_FROM] == ["M"]


def test_rejects_give_no_index(ctx, ffi, oracle, torch, crafted):
    """the build's status, message and bytes are the oracle's, and no handle comes back"""
    bad = []
    for name in dc.REJECTS + lc.REJECTS:
        z, verdict = crafted[name]
        for fmt_name, s, v in _containers(oracle, name, z, verdict):
            try:
                assert v[0] != 0
                assert _built(ctx, ffi, torch, fmt_name, s, v, SPACING_MIN) is None
            except AssertionError as e:
                bad.append("%s %s: %s" % (name, fmt_name, str(e).split("\n")[0] or repr(e)))
    _report(bad)


@pytest.mark.parametrize("name", ["A", "C1", "W_32768", "N_chain"])
def test_span_from_inside_a_block(ctx, ffi, torch, crafted, name):
    """reads from exactly lfx_index_span, which reaches back to the block's header; one byte less at either end is LFX_E_ARG"""
    z, verdict = crafted[name]
    idx = _built(ctx, ffi, torch, "DEFLATE", z, verdict, SPACING_MIN)
    try:
        partial_input_from_inside_a_block(ctx, ffi, torch, idx, z, verdict[1])
    finally:
        idx.close()


@pytest.mark.parametrize("name", ["N_chain", "W_32768_lits", "X_relay40"])
def test_persistence(ctx, ffi, torch, crafted, name):
    from libflate_amd.index import Index
    z, verdict = crafted[name]
    out = verdict[1]
    idx = _built(ctx, ffi, torch, "DEFLATE", z, verdict, SPACING_MIN)
    other = None
    try:
        blob = idx.to_bytes()
        other = Index.from_bytes(blob, ctx)
        assert other.to_bytes() == blob and other.points == idx.points
        ranges = point_reads(idx.points, len(out))[:64]
        assert len(ranges) == 64
        got = [g.cpu().numpy().tobytes() for g in other.read_many(z, ranges)]
        assert got == [g.cpu().numpy().tobytes() for g in idx.read_many(z, ranges)] == [out[o:o + ln] for o, ln in ranges]
        guarded_reads(ctx, ffi, torch, other, z, out, ranges)
    finally:
        idx.close()
        if other is not None:
            other.close()
