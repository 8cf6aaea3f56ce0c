"""No GPU: every crafted stream of deflate_craft.CASES gets its verdict from the oracle here, before a GPU sees it
(test_gpu_craft_decode.py).  A valid case the oracle and the plain model `expand` disagree on is a bug in the writer, not a
finding.  python-zlib must agree on the cases listed as such and must REFUSE B and D: the two legal shapes (for the reference)
that no zlib-made input can stand in for."""
import time
import zlib

import pytest

import deflate_craft as dc
from deflate_craft import gzwrap, zwrap

OK, INVALID_DATA, UNEXPECTED_EOF = 0, 1, 2


@pytest.fixture(scope="module")
def verdicts(oracle):
    """{name: (z, expected, (status, output, consumed, message))}"""
    return dict((name, (z, want, oracle.decode(oracle.DEFLATE, z))) for name, (z, want) in dc.built().items())


def test_case_list_is_whole():
    names = [n for n, _ in dc.CASES]
    assert len(set(names)) == len(names)
    assert sorted(names) == sorted(dc.VALID + dc.REJECTS)
    assert sorted(dc.REJECTS) == sorted([k for k in dc.REJECT_PREFIX] + [k + "_behind" for k in dc.REJECT_PREFIX])


@pytest.mark.parametrize("name", dc.VALID)
def test_valid_cases(verdicts, name):
    z, want, (rc, out, used, msg) = verdicts[name]
    assert want is not None
    assert rc == OK, msg
    assert out == want
    assert used == len(z)
    if name in dc.VALID_ZLIB_AGREES or name in dc.SMALL and name != "B_small":
        assert zlib.decompress(z, -15) == want
    elif name != "M":
        with pytest.raises(zlib.error) as e:
            zlib.decompress(z, -15)
        print(name, "zlib:", e.value)
        assert ("invalid literal/lengths set" if name.startswith("B") else "too many length or distance symbols") in str(e.value)


def test_sizes_pick_the_entry_paths(verdicts):
    """between 4 KiB and 1.5 MiB compressed a member starts with the piece walk from the known first block; M's head is past
    that; the small variants and the rejects that stand alone are for the serial kernel; a reject under 64 bytes exists (the batch
    path's floor, as a zlib stream: 6 bytes more)"""
    for name in dc.VALID_ZLIB_AGREES + dc.VALID_ZLIB_REFUSES:
        assert 4 * dc.KIB <= len(verdicts[name][0]) < 3 * dc.MIB // 2, (name, len(verdicts[name][0]))
    assert len(verdicts["M"][0]) > 3 * dc.MIB // 2
    for name in dc.SMALL + list(dc.REJECT_PREFIX):
        assert len(verdicts[name][0]) < 4 * dc.KIB, (name, len(verdicts[name][0]))
    for name in dc.REJECT_PREFIX:
        assert len(verdicts[name + "_behind"][0]) >= 8 * dc.KIB, name
    assert len(verdicts["I1"][0]) + 6 < 64


@pytest.mark.parametrize("name", dc.REJECTS)
def test_reject_cases(verdicts, name):
    z, want, (rc, out, used, msg) = verdicts[name]
    print(name, rc, len(out), used, msg)
    assert want is None
    assert msg.startswith(dc.REJECT_PREFIX[name.split("_")[0]]), msg
    assert rc == (UNEXPECTED_EOF if name.startswith("K") else INVALID_DATA)
    if name.endswith("_behind"):          # the bytes of the valid blocks in front are delivered
        assert len(out) >= 20000 and set(out[:20000]) <= set(range(65, 75))
    with pytest.raises(zlib.error):
        zlib.decompress(z, -15)


def test_stored_headers_at_every_bit_phase():
    phases = []
    dc.build_H(phases)
    assert sorted(phases) == list(range(8))


N_CODED = ["D", "C1", "A", "B", "C2", "E2", "E3", "E4", "A", "A"]


def test_N_chain_blocks(oracle, verdicts):
    """one stream of every shape: at least twelve non-final blocks, the coded ones of 8 to 40 KiB, four stored ones of 1000 to
    3000 bytes whose headers sit at four bit phases, unlike neighbours, an empty final fixed block"""
    phases, kinds = [], []
    z, want = dc.build_N_chain(phases, kinds)
    assert (z, want) == verdicts["N_chain"][:2]
    assert phases == list(dc.N_PHASES) and len(set(phases)) == 4
    blocks = oracle.scan_blocks(z)
    assert len(blocks) == len(kinds) + 1 >= 13 and [b[3] for b in blocks] == [0] * len(kinds) + [1]
    assert blocks[-1][2:] == (1, 1, 0) and blocks[-1][1] - blocks[-1][0] == 10
    assert [k for k in kinds if k != "stored"] == N_CODED and all(a != b for a, b in zip(kinds, kinds[1:-1]))
    at, got_phases = 0, []
    for kind, (start, end, btype, bfinal, out_len) in zip(kinds, blocks):
        size = (end - start) / 8
        print("N_chain %-6s btype %d  %7.0f bytes -> %6d" % (kind, btype, size, out_len))
        if kind == "stored":
            assert btype == 0 and 1000 <= out_len <= 3000
            got_phases.append(start % 8)
        else:
            assert btype == 2 and 8 * dc.KIB <= size <= 40 * dc.KIB, (kind, size)
        at += out_len
    assert got_phases == phases and at == len(want) < dc.MIB
    # the matches that open the A blocks read the blocks in front, the first of them through a stored block
    for i, kind in enumerate(kinds):
        if kind == "A":
            assert sum(b[4] for b in blocks[:i]) >= 32768
    assert kinds[kinds.index("A") - 1] == "stored" and kinds[len(kinds) - 2:] == ["A", "A"] and kinds[len(kinds) - 3] == "stored"


STREAM_STEP = 997           # (test_gpu_craft_stream.py: a prime below every multi-block case's block size)


def test_cases_that_must_take_several_windows(oracle, verdicts):
    """the stream decoder's tests mean something only where a case cannot be decoded in one window (deflate_craft.takes_windows)"""
    for name, step in (("N_chain", STREAM_STEP), ("G", STREAM_STEP), ("H", STREAM_STEP), ("M", 65536)):
        z = verdicts[name][0]
        blocks = oracle.scan_blocks(z)
        assert len(blocks) >= 5 and dc.takes_windows(blocks, len(z), step), name
    for name in ("N_chain", "H"):         # ... also as zlib and gzip streams
        z = verdicts[name][0]
        assert dc.takes_windows(oracle.scan_blocks(z), len(z) + 18, STREAM_STEP, head=10), name
    coded = [b for b in oracle.scan_blocks(verdicts["N_chain"][0]) if b[2] == 2]
    assert min(b[1] - b[0] for b in coded) // 8 > STREAM_STEP


@pytest.mark.parametrize("name", dc.REJECTS)
def test_reject_prefixes(oracle, verdicts, name):
    """valid_prefix(name) is the reject's own bits up to the block that holds the fault, and the oracle delivers its bytes"""
    z, _want, (rc, out, used, msg) = verdicts[name]
    prefix = dc.valid_prefix(name)
    prc, pout, pused, _ = oracle.decode(oracle.DEFLATE, prefix)
    blocks = oracle.scan_blocks(prefix)
    assert prc == OK and pused == len(prefix) and blocks[-1][2:] == (1, 1, 0)
    assert dc.same_bits(z, prefix, blocks[-1][0])
    assert out[:len(pout)] == pout and len(pout) == sum(b[4] for b in blocks)


def test_the_shapes_the_cases_are_about(oracle, verdicts):
    # A: both codes reach 15 bits and the distances 24577...32768 are used
    assert max(dc.A_LIT) == 15 and max(dc.A_DIST) == 15 and dc.dist_symbol(32768) == (29, 13, 8191)
    # E1: 258 as symbol 284 with extra 31; the same bytes as C1 from a different stream, and a longer header
    assert dc.len_symbol(258, True) == (284, 5, 31) and dc.len_symbol(258) == (285, 0, 0) and dc.len_symbol(257) == (284, 5, 30)
    assert verdicts["E1"][1] == verdicts["C1"][1] and verdicts["E1"][0] != verdicts["C1"][0]
    assert any(t == (258, 1) for t in dc.c1_tokens(20000))
    # G: 300 empty blocks in a row, of three kinds, each producing nothing
    blocks = oracle.scan_blocks(verdicts["G"][0])
    assert len(blocks) == 303 and [b[4] for b in blocks[1:301]] == [0] * 300
    assert [b[2] for b in blocks[1:7]] == [1, 0, 2, 1, 0, 2]
    # M: the crafted blocks sit behind ≥ 1.5 MiB of another encoder's blocks and their first long matches read its bytes
    z, want, _ = verdicts["M"]
    blocks = oracle.scan_blocks(z)
    crafted = [i for i, b in enumerate(blocks) if b[2] == 2 and b[4] == 60000]
    assert len(crafted) == 1 and blocks[crafted[0] - 1][0] // 8 >= 3 * dc.MIB // 2


@pytest.mark.parametrize("name", [n for n, _ in dc.CASES])
def test_containers(oracle, verdicts, name):
    """the same bodies as zlib and gzip streams: the verdict of the body, the bytes, and the container's own bytes consumed"""
    z, want, (rc, out, used, msg) = verdicts[name]
    for fmt, wrapped, head, tail in ((oracle.ZLIB, zwrap(out, z), 2, 4), (oracle.GZIP, gzwrap(out, z), 10, 8)):
        wrc, wout, wused, wmsg = oracle.decode(fmt, wrapped)
        if name.startswith("K"):          # its data runs to the end of the input: the trailer's bytes are data too
            assert (wrc, wmsg) == (rc, msg) and wout[:len(out)] == out and wused == len(wrapped), (name, fmt, wmsg)
            continue
        assert (wrc, wout, wmsg.split(":")[0]) == (rc, out, msg.split(":")[0]), (name, fmt, wmsg)
        assert wused == head + used + (tail if rc == OK else 0), (name, fmt)


def test_writer_is_quick():
    """a 60 000-token block in well under a second (about 0.05 s): the best of three runs, so that a loaded machine's one
    slow run does not decide"""
    best = 1e9
    for _ in range(3):
        t0 = time.perf_counter()
        dc.build_B(60000)
        best = min(best, time.perf_counter() - t0)
    print("build_B(60000): %.3f s" % best)
    assert best < 0.5
