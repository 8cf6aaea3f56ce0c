"""CPU: the model of block_merge (tests/merge_model.py; the contract: include/lfx.h) against python-zlib and the
oracle, never against the library — test_gpu_block_merge.py then holds the library to the model.  Every model stream inflates
to the input, none is longer than the oracle's unmerged one, and the rule gives the groups the contract spells out: a full
merge of homogeneous text, kept cuts between sections of different statistics, partial right children, the region seam, and a
node one bit either side of its children."""
import gzip as pygzip
import zlib

import pytest

import auto_block_model as abm
import auto_cases as cases
import merge_cases as mc
import merge_model as model

BS = mc.BS


def inflate(name, stream):
    if name == "gzip":
        return pygzip.decompress(stream)
    return zlib.decompress(stream, -15 if name == "deflate" else 15)


def run(oracle, name, data, write_size=BS, **kw):
    code = {"deflate": oracle.DEFLATE, "zlib": oracle.ZLIB, "gzip": oracle.GZIP}[name]
    base = oracle.encode(code, data, write_size, **kw)
    out = model.expected(oracle, name, base, data)
    assert inflate(name, out[0]) == data and len(out[0]) <= len(base)
    return base, out


@pytest.mark.parametrize("name", ["deflate", "zlib", "gzip"])
def test_homogeneous_text_merges_fully(oracle, name):
    data = mc.text(65536)
    base, (stream, head, nodes) = run(oracle, name, data, block_size=BS)
    assert model.groups(head) == [(0, 16), (16, 1)]      # (the 17th: the empty candidate behind a multiple of the write size)
    assert len(stream) < len(base)
    # the container is the base stream's
    h, t = abm.header_len(name, base), abm.TRAILER[name]
    assert stream[:h] == base[:h] and (t == 0 or stream[-t:] == base[-t:])
    # 16 leaves + the empty one, and the 15 inner nodes of a full tree
    assert len(nodes) == 17 + 15


def test_sections_keep_their_cuts(oracle):
    data = mc.sections()
    _, (stream, head, nodes) = run(oracle, "zlib", data, block_size=BS)
    assert model.groups(head) == [(0, 2), (2, 2), (4, 2), (6, 2), (8, 1)]
    sizes = {(lo, hi): d for lo, hi, d in nodes}
    for lo in (0, 4):                                     # text ‖ random, zeros ‖ text: one code for both is longer
        assert sizes[(lo, lo + 4)] > sizes[(lo, lo + 2)] + sizes[(lo + 2, lo + 4)]
    assert (0, 8) not in sizes                            # a node that is not whole ends its ancestors: never evaluated


@pytest.mark.parametrize("n", mc.RUNS)
def test_run_lengths(oracle, n):
    data = mc.run_of(n)
    _, (stream, head, nodes) = run(oracle, "deflate", data, block_size=BS)
    assert len(head) == n and model.groups(head) == mc.RUN_GROUPS[n]
    assert all(hi - lo <= model.MERGE_MAX and lo // 16 == (hi - 1) // 16 for lo, hi, _ in nodes)


def test_tree_shapes_by_hand():
    """the rule alone, over made-up sizes: a partial right child, an empty one, a node that is not whole, the seam"""
    always = lambda lo, hi: hi - lo                       # D(node) = D(left) + D(right): always whole
    assert model.tree(3, always) == [0, 0, 0]
    assert model.tree(5, always) == [0] * 5               # [0,4) + the leaf 4, whose own right children are empty up to level 3
    assert model.tree(17, always) == [0] * 16 + [16]
    assert model.tree(33, always) == [0] * 16 + [16] * 16 + [32]
    never = lambda lo, hi: 1 if hi - lo == 1 else 10 ** 9
    assert model.tree(7, never) == list(range(7))
    # [2,4) fails: [0,2) stays a group, [0,4) and [0,8) are dead, [4,7) is whole
    pair23 = lambda lo, hi: 10 ** 9 if (lo, hi) == (2, 4) else hi - lo
    assert model.tree(7, pair23) == [0, 0, 2, 3, 4, 4, 4]
    # one bit: D(node) = D(l) + D(r) + 1 is not whole, D(l) + D(r) and D(l) + D(r) - 1 are
    for extra, want in ((-1, [0, 0]), (0, [0, 0]), (1, [0, 1])):
        assert model.tree(2, lambda lo, hi, extra=extra: 100 if hi - lo == 1 else 200 + extra) == want


@pytest.mark.parametrize("seed,diff", mc.TIES)
def test_ties(oracle, seed, diff):
    data = mc.tie(seed)
    _, (stream, head, nodes) = run(oracle, "deflate", data, mc.TIE_BS, block_size=mc.TIE_BS)
    sizes = {(lo, hi): d for lo, hi, d in nodes}
    assert sizes[(0, 2)] - sizes[(0, 1)] - sizes[(1, 2)] == diff
    assert head == ([0, 0] if diff <= 0 else [0, 1])


def test_a_zlib_sync_flush_splits_a_run(oracle):
    data = mc.text(6 * BS + 100, 4)
    writes = [BS, BS, BS, None, BS, BS, BS, 100]
    base = abm.oracle_writes(oracle, "zlib", data, writes, block_size=BS, zlib_sync_flush=1)
    stream, head, nodes = model.expected(oracle, "zlib", base, data)
    assert zlib.decompress(stream) == data and len(stream) <= len(base)
    assert model.groups(head) == [(0, 4), (4, 1), (5, 4)]
    assert [b[2] for b in oracle.scan_blocks(stream[2:-4])] == [2, 0, 2]


@pytest.mark.parametrize("n", [0, 1, 100, BS - 1])
def test_empty_and_shorter_than_one_block(oracle, n):
    data = mc.text(n, 6)
    base, (stream, head, nodes) = run(oracle, "deflate", data, block_size=BS)
    assert stream == base and head == [0]


def test_candidates_of_several_chunks(oracle):
    data = mc.text(65536 + 500, 7)
    _, (stream, head, nodes) = run(oracle, "zlib", data, window_size=1024, block_size=16384)
    assert model.groups(head) == [(0, 5)]


def test_auto_on_top(oracle):
    data = mc.text(8192, 8) + cases.rand(8192, 9) + mc.text(5000, 10)
    base = oracle.encode(oracle.DEFLATE, data, BS, block_size=BS)
    merged = model.expected(oracle, "deflate", base, data)
    stream, head, nodes, choices = model.expected(oracle, "deflate", base, data, None, True)
    assert zlib.decompress(stream, -15) == data
    assert model.groups(head) == [(0, 2), (2, 2), (4, 2)] and choices == [abm.DYNAMIC, abm.STORED, abm.DYNAMIC]
    assert len(stream) <= len(merged[0]) <= len(base)
    # the 8192 random bytes are ONE stored block now: 5 bytes of framing, not 10
    assert [b[4] for b in oracle.scan_blocks(stream)] == [8192, 8192, 5000]


def test_batch_records_never_grow(oracle):
    for r in mc.batch_records()[:40]:
        run(oracle, "zlib", r, block_size=BS)
