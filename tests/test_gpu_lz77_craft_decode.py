"""GPU: the crafted LZ77 token streams of lz77_craft.CASES through the decode entry points: lfx_decode_device (every output
phase, every path, both widths of the materialise kernel), lfx_decode_batch_device, lfx_decode_members_device.  Every
stream's verdict is fixed by the oracle on the CPU first, and test_lz77_craft_streams.py proves there which edge of the
materialisation each case sits on.  Integer work: every comparison is exact.  A test walks all its cases and reports every one
that differs."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

import lz77_craft as lc
from deflate_craft import gzwrap, zwrap
from test_gpu_craft_decode import GUARD, _report
from test_gpu_members import _dev, check, torch  # noqa: F401
from test_gpu_parity import ctx, ffi, lfx, synth  # noqa: F401  (fixtures)

ALL_FORMATS = ("W_32768", "W_32768_lits", "X_first_token", "R_second_block")          # these also go through as zlib and gzip
PHASED = ("T_sweep", "P_all_periods", "X_first_token", "W_near_ring")
# Cases of DIRECT that do not decode without the marker phases, with the reason read from the code.
OTHER_PATH = {
    "V_second_block": "its one match opens the second block and reads the first: a block that reads in front of itself raises "
                      "the emit step's flag 2, and the stream is materialised through markers",
}
assert len(OTHER_PATH) <= 2 and not any(n[0] in "TPW" for n in OTHER_PATH)


@pytest.fixture(scope="module")
def crafted(oracle):
    """{name: (raw DEFLATE, (status, output, consumed, message) of the oracle)}"""
    out = {}
    for name, (z, want) in lc.built().items():
        verdict = oracle.decode(oracle.DEFLATE, z)
        assert (verdict[0] == 0) == (want is not None) and (want is None or verdict[1] == want), name      # (test_lz77_craft_streams.py)
        out[name] = (z, verdict)
    return out


def _decode_at(c, ffi, torch, fmt_name, z, verdict, k=0):
    """decode_device to d_out + k, into exactly the oracle's length, guards on both sides → (what differs, phase names)"""
    orc, oout, oused, omsg = verdict
    cap = len(oout)
    d_in = _dev(torch, z)
    d_buf = torch.full((GUARD + k + cap + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    at = GUARD + k
    rc, ol, used, msg = c.decode_device(getattr(ffi, fmt_name), d_in.data_ptr(), len(z), d_buf.data_ptr() + at, cap)
    timing = c.last_timing()
    host = d_buf.cpu().numpy().tobytes()
    bad = []
    if (rc, ol, used) != (orc, len(oout), oused):
        bad.append("(status, out_len, consumed) %r, oracle %r, message %r" % ((rc, ol, used), (orc, len(oout), oused), msg))
    if msg.split(":")[0] != omsg.split(":")[0]:
        bad.append("message %r, oracle %r" % (msg, omsg))
    n = min(ol, cap)
    if host[at:at + n] != oout[:n]:
        first = next(i for i in range(n) if host[at + i] != oout[i])
        bad.append("bytes differ from %d of %d" % (first, ol))
    if host[:at] != b"\x5a" * at:
        bad.append("written in front of the output")
    if host[at + cap:] != b"\x5a" * GUARD:
        bad.append("guard written")
    return bad, [p[0] for p in (timing or {"phases": []})["phases"]]


def _containers(oracle, name, z, verdict):
    yield "DEFLATE", z, verdict
    if name in ALL_FORMATS:
        for fmt_name, s in (("ZLIB", zwrap(verdict[1], z)), ("GZIP", gzwrap(verdict[1], z))):
            yield fmt_name, s, oracle.decode(getattr(oracle, fmt_name), s)


def test_decode_device(ctx, ffi, oracle, torch, crafted):
    bad = []
    for name, (z, verdict) in crafted.items():
        for fmt_name, s, v in _containers(oracle, name, z, verdict):
            bad += ["%s %s: %s" % (name, fmt_name, b) for b in _decode_at(ctx, ffi, torch, fmt_name, s, v)[0]]
    _report(bad)


def test_decode_device_output_phases(ctx, ffi, torch, crafted):
    """d_out + 1, 2, 3: the head and the tail of the materialise kernel's dword flush"""
    bad = []
    for name in PHASED:
        z, verdict = crafted[name]
        for k in (1, 2, 3):
            bad += ["%s +%d: %s" % (name, k, b) for b in _decode_at(ctx, ffi, torch, "DEFLATE", z, verdict, k)[0]]
    _report(bad)


def test_paths_taken(ffi, lfx, torch, crafted, monkeypatch):
    """A contract, not a record: without the serial walk (LFX_NO_SERIAL=1 makes it an error) every valid case decodes, the
    DIRECT ones by the byte materialisation alone (lz77_copy and no marker phase, OTHER_PATH excepted), the MARKER ones
    through lz77_sym, win_chain and substitute."""
    monkeypatch.setenv("LFX_NO_SERIAL", "1")
    c2 = lfx.Context(0)                 # (diagnostic switches are read when a context is made)
    bad = []
    try:
        c2.enable_timing(True)
        for name in lc.DIRECT + lc.MARKER:
            z, verdict = crafted[name]
            differs, names = _decode_at(c2, ffi, torch, "DEFLATE", z, verdict)
            print("PATH %-16s %s" % (name, " ".join(names)))
            bad += ["%s: %s" % (name, b) for b in differs]
            if "serial" in names:
                bad.append("%s: the serial walk ran" % name)
            if name in lc.MARKER:
                missing = [p for p in ("lz77_sym", "win_chain", "substitute") if p not in names]
                if missing:
                    bad.append("%s: no %s among %s" % (name, missing, names))
            else:
                if "lz77_copy" not in names:
                    bad.append("%s: no lz77_copy among %s" % (name, names))
                if ("lz77_sym" in names) != (name in OTHER_PATH):
                    bad.append("%s: marker phases %s among %s" % (name, "missing" if name in OTHER_PATH else "present", names))
    finally:
        c2.close()
    _report(bad)


def test_narrow_and_wide_instances(ctx, ffi, oracle, torch):
    """Up to four emit jobs run the 1024-lane materialise kernel (the one- and two-block cases in the tests above), more run
    the 256-lane one: the self-contained blocks of six cases as one stream.  W_32768_lits' block goes first, its distances
    need 32768 bytes of its own in front.  (Which instance ran is not visible from outside: it follows from the number of
    emit jobs, lfx_inflate_fast.hip, launch_blk_materialize; what is asserted is the direct path and the bytes.)"""
    blocks = []
    for name in ("W_32768_lits", "T_all258", "T_sweep", "T_avg8", "P_short_runs", "P_all_periods"):
        blocks += [b for b in lc.blocks_of(name) if b[1]]
    assert len(blocks) == 7
    z = lc.write(blocks + [("fixed", [])])
    want = b"".join(lc.model([b])[0] for b in blocks)
    verdict = oracle.decode(oracle.DEFLATE, z)
    assert verdict[:3] == (0, want, len(z))
    ctx.enable_timing(True)
    try:
        bad, names = _decode_at(ctx, ffi, torch, "DEFLATE", z, verdict)
    finally:
        ctx.enable_timing(False)
    print("PATH narrow: %s" % " ".join(names))
    if "lz77_copy" not in names or "lz77_sym" in names or "serial" in names:
        bad.append("not the direct path: %s" % names)
    _report(bad)


def test_decode_batch_device(ctx, ffi, oracle, torch, crafted):
    """Every case as a zlib stream in ONE call, the outputs packed without a gap at three byte phases: a reject's output lies
    directly behind a valid stream's, which its bad match must not read, and nothing may be written outside a stream's own
    capacity."""
    valid, rejects = list(lc.VALID), list(lc.REJECTS)
    order = []
    while valid or rejects:            # two valid, one reject, ...
        order += valid[:2] + rejects[:1]
        valid, rejects = valid[2:], rejects[1:]
    assert sorted(order) == sorted(crafted)
    assert all(order[i - 1] in lc.VALID for i, n in enumerate(order) if n in lc.REJECTS) and order[0] in lc.VALID
    streams = [zwrap(crafted[n][1][1], crafted[n][0]) for n in order]
    want = [oracle.decode(oracle.ZLIB, s) for s in streams]
    k = len(streams)
    in_len = [len(s) for s in streams]
    in_off = [sum(in_len[:i]) for i in range(k)]
    out_cap = [len(w[1]) for w in want]
    d_in = _dev(torch, b"".join(streams))
    a = lambda v: (C.c_uint64 * k)(*v)
    bad = []
    for phase in (0, 1, 3):
        out_off = [phase + sum(out_cap[:i]) for i in range(k)]
        d_out = torch.full((out_off[-1] + out_cap[-1] + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        got_len, got_st = (C.c_uint64 * k)(), (C.c_int32 * k)()
        rc = ffi.lib().lfx_decode_batch_device(ctx.handle, ffi.ZLIB, k, d_in.data_ptr(), a(in_off), a(in_len), d_out.data_ptr(), a(out_off),
                                               a(out_cap), got_len, got_st)
        assert rc == ffi.OK
        host = d_out.cpu().numpy()
        for i, name in enumerate(order):
            orc, oout, oused, omsg = want[i]
            if (got_st[i], got_len[i]) != (orc, len(oout)):
                bad.append("+%d %s: (status, out_len) %r, oracle %r %s" % (phase, name, (got_st[i], got_len[i]), (orc, len(oout)), omsg))
            n = min(got_len[i], out_cap[i])
            if host[out_off[i]:out_off[i] + n].tobytes() != oout[:n]:      # (a valid stream's whole region; a reject's up to out_len)
                bad.append("+%d %s: bytes differ" % (phase, name))
        if not (host[:phase] == 0x5A).all():
            bad.append("+%d: written in front of the first stream" % phase)
        if not (host[out_off[-1] + out_cap[-1]:] == 0x5A).all():
            bad.append("+%d: guard written" % phase)
    _report(bad)


@pytest.mark.parametrize("middle", ["R_have0_small", "R_second_block"])
def test_members_neighbour_reject(ctx, ffi, oracle, torch, crafted, middle):
    """a gzip file of three members whose second starts with (or holds) a match that reaches in front of the member's first
    byte, where the first member's output lies: both device paths give the oracle's verdict and deliver the first member only"""
    zv, (_, v_out, _, _) = crafted["V_first_block"]
    zr, (_, r_out, _, _) = crafted[middle]
    good = gzwrap(v_out, zv)
    data = good + gzwrap(r_out, zr) + good
    o_rc, o_out, o_used, o_msg = oracle.decode(oracle.GZIP, data, multi=True)
    assert o_rc == ffi.E_INVALID_DATA and o_msg.startswith(lc.REJECT_PREFIX) and o_out[:len(v_out)] == v_out
    rc, out, used, members = check(ctx, ffi, oracle, torch, data, want_status=ffi.E_INVALID_DATA)
    assert members == [(0, len(good), 0, len(v_out))]
    assert out == v_out + r_out           # the bytes in front of the bad match, none of them copied from the neighbour
    assert ctx.last_error().startswith(lc.REJECT_PREFIX)


def test_storing_scan_and_two_pass_agree(ctx, ffi, lfx, torch, crafted, monkeypatch):
    """Blocks over 1 Mbit are for the storing scan and blk_place, under LFX_TWO_PASS=1 for blk_emit: `reach` and the cut
    candidates are tracked in both.  Held here: both settings give the oracle's bytes.  Not held: that the default context
    did place the blocks — that also depends on the finder's candidate count and on plan_store, and no phase tells."""
    monkeypatch.setenv("LFX_TWO_PASS", "1")
    c3 = lfx.Context(0)
    bad = []
    try:
        for name in ("U_anchor_big", "U_anchor_big_m1", "X_first_token"):
            z, verdict = crafted[name]
            for label, c in (("default", ctx), ("two-pass", c3)):
                bad += ["%s %s: %s" % (name, label, b) for b in _decode_at(c, ffi, torch, "DEFLATE", z, verdict)[0]]
    finally:
        c3.close()
    _report(bad)
