"""CPU: the catalogue of crafted symbol counts (tests/huff_cases.py).  First, with the oracle alone: every case is what it claims
— the limit is active, the alphabets have the sizes named, the depth queue meets a run of equal weights long enough to leave the
register window, the counts cross (or stay below) 2^23, the header has the runs named, the plan has the blocks and chunks.
Then every case's histograms go through lfx_debug_huff_block — lfx_huff.h as lane 0 of 1 — against the oracle's widths, codes
and header bytes.  test_gpu_huff_crafted.py runs the same catalogue through the kernels: a case that passes here and fails
there is a defect of the 320-lane build (a barrier, a stride, a field read before it is written, a lost atomic)."""
import heapq

import numpy as np
import pytest

import huff_cases as hc
import merge_model
from test_host_pipeline import _CannedCodes, _one_final_block, ffi, huff_block, plan  # noqa: F401  (ffi: fixture)


# ---- what a case's blocks count: from the plan and the oracle alone ------------------------------------------------------
def block_hists(ffi, oracle, case, spec=None):
    """→ (histograms (320 counters) of the case's blocks in order, rows: the counters of block 0's chunks one by one)"""
    spec = case.make() if spec is None else spec
    if case.driver == "codes":
        h = hc.hist_of_codes(spec)
        return [h], [h]
    data, o = spec["data"], spec["opts"]
    chunks, blocks = plan(ffi, ffi.DEFLATE, len(data), spec["write_size"], spec["writes"], **o)
    hists, rows = [], []
    for bi, (btype, final, first, nch, in_off, in_len) in enumerate(blocks):
        h = np.zeros(320, np.int64)
        for c in chunks[int(first):int(first) + int(nch)]:
            off, ln, flags = int(c[0]), int(c[1]), int(c[3])
            seg = data[off:off + ln]
            r = np.zeros(320, np.int64)
            if ln == 0:
                pass                                 # (a block that holds EndOfBlock alone: a chunk of no bytes)
            elif flags & 2:
                r[:256] = np.bincount(np.frombuffer(seg, np.uint8), minlength=256)
            else:
                assert case.driver == "parse"
                for w in oracle.lz77_chunk(seg, o.get("window_size", 32768), o.get("max_length", 258)):
                    val, dist = int(w) >> 16, int(w) & 0xFFFF
                    if dist == 0:
                        r[val] += 1
                    else:
                        r[hc.len_symbol(val)] += 1
                        r[288 + hc.dist_symbol(dist)] += 1
            if flags & 1:
                r[256] += 1
            h += r
            if bi == 0:
                rows.append(r)
        assert h[256] == 1
        hists.append(h)
    return hists, rows


def dist_counts(h):
    d = h[288:318].copy()
    if d.sum() == 0:
        d[0] = 1                                     # symbol.rs:332-337: the dist[0] dummy
    return d


# ---- restatements from src/huffman.rs, for the claims only ----------------------------------------------------------------
def depth_queue_runs(freqs):
    """calc_optimal_max_bitwidth (huffman.rs:261-274): a heap of (weight, width) that pops the smallest weight and, among equal
    weights, the largest width.  Internal nodes are made in non-decreasing weight, so those waiting form a queue; whenever
    one is popped, the nodes of its weight waiting with it are a run at the queue's head.  → (the depth, the longest such run,
    whether some run held unequal widths)"""
    heap = [(int(f), 0, i) for i, f in enumerate(freqs) if f > 0]
    heapq.heapify(heap)
    waiting, tick, longest, unequal = {}, len(heap), 0, False            # waiting: weight → widths of the internal nodes
    while len(heap) > 1:
        got = []
        for _ in range(2):
            w, negd, _ = heapq.heappop(heap)
            if negd < 0:
                run = waiting[w]
                longest = max(longest, len(run))
                unequal |= len(set(run)) > 1
                run.remove(-negd)
            got.append((w, -negd))
        w, d = got[0][0] + got[1][0], 1 + max(got[0][1], got[1][1])
        waiting.setdefault(w, []).append(d)
        heapq.heappush(heap, (w, -d, tick))
        tick += 1
    return (max(1, -heap[0][1]) if heap else 0), longest, unequal


def package_merge_events(freqs, limit):
    """length_limited_huffman_codes::calc (huffman.rs:307-362) over the weights alone → (some merge met a package and a leaf of
    equal weight, some package() dropped an odd tail)"""
    src = sorted(int(f) for f in freqs if f > 0)
    depth = depth_queue_runs(freqs)[0]
    tie = odd = False
    cur = list(src)
    for _ in range(min(limit, depth) - 1):
        odd |= len(cur) % 2 == 1 and len(cur) >= 2
        pk = [cur[2 * i] + cur[2 * i + 1] for i in range(len(cur) // 2)] if len(cur) >= 2 else cur
        tie |= bool(set(pk) & set(src))
        cur = sorted(pk + src)                   # (weights alone: the order inside a tie does not show)
    odd |= len(cur) % 2 == 1 and len(cur) >= 2
    return tie, odd


def runs_of(widths):
    out = []
    for w in widths:
        if out and out[-1][0] == w:
            out[-1][1] += 1
        else:
            out.append([int(w), 1])
    return out


# ---- 1: every case is what it claims ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", hc.NAMES)
def test_case_is_what_it_claims(ffi, oracle, name):
    case = hc.BY_NAME[name]
    claim = dict(case.claim)
    spec = case.make()
    hists, rows = block_hists(ffi, oracle, case, spec)
    if case.driver == "codes":
        assert len(spec) <= hc.MAX_CODES
    else:
        chunks, blocks = plan(ffi, ffi.DEFLATE, len(spec["data"]), spec["write_size"], spec["writes"], **spec["opts"])
        if "blocks" in claim:
            assert len(blocks) == claim.pop("blocks")
        if "chunks" in claim:
            assert len(chunks) == claim.pop("chunks")
        if "rows" in claim:
            assert int(blocks[0][3]) == claim.pop("rows") == len(rows)
        if claim.pop("disjoint_rows", False):
            used = [set(np.nonzero(r[:256])[0]) for r in rows]
            assert all(not (used[i] & used[j]) for i in range(4) for j in range(i)) and len(used[1]) == 1
            assert int(rows[4][:256].sum()) == 1 and len(spec["data"]) - int(blocks[0][5]) == 0 and int(blocks[1][5]) == 0
    h = hists[claim.pop("block", 0)]
    lit, dist = h[:286], dist_counts(h)
    lw, dw = oracle.huff_widths(lit, 15), oracle.huff_widths(dist, 15)
    nl = max(257, int(np.nonzero(lw)[0].max()) + 1)
    nd = max(1, int(np.nonzero(dw)[0].max()) + 1)
    widths = list(lw[:nl]) + [-1] + list(dw[:nd])                # (-1: a run never crosses into the distance table)
    clen = np.bincount(hc.header_entries(lw[:nl], dw[:nd]), minlength=19)
    for key, want in claim.items():
        if want is None:
            continue
        if key == "lit_n":
            assert int((lit > 0).sum()) == want
        elif key == "dist_n":
            assert int((h[288:318] > 0).sum()) == want
        elif key == "lit_clamp":
            assert (int(max(oracle.huff_widths(lit, 60))) > 15) == want
        elif key == "dist_clamp":
            assert (int(max(oracle.huff_widths(dist, 60))) > 15) == want
        elif key == "clen_clamp":
            assert (int(max(oracle.huff_widths(clen, 60))) > 7) == want
        elif key == "tie_run":
            depth, longest, unequal = depth_queue_runs(dist if claim.get("tie_alpha") == "dist" else lit)
            assert longest >= want and longest > 3                # (the register window holds three entries)
            assert unequal == claim.get("tie_unequal", True)
        elif key in ("tie_alpha", "tie_unequal"):
            pass
        elif key == "pm_tie":
            assert package_merge_events(dist if claim.get("tie_alpha") == "dist" else lit, 15)[0] == want
        elif key == "pm_odd":
            assert package_merge_events(lit, 15)[1] == want
        elif key == "big":
            assert (int(h.max()) >= 1 << 23) == want
        elif key == "tied":
            for count, nsym in want.items():
                assert int((h == count).sum()) == nsym
            if claim.get("big"):
                assert int((h == h.max()).sum()) == 2 and int(h.max()) == 1 << 23     # the symbol decides between the two
        elif key == "max_count":
            assert int(h.max()) == want
        elif key == "nl":
            assert nl == want
        elif key == "nd":
            assert nd == want
        elif key == "zero_run":
            assert [0, want] in runs_of(widths)
        elif key == "width_run":
            assert any(v > 0 and n == want for v, n in runs_of(widths))
        else:
            raise AssertionError("unknown claim " + key)


def test_the_restated_depth_bounds_the_oracles_widths(oracle):
    """package-merge never goes deeper than the depth the queue merge finds (it is given that depth as its limit), so the
    catalogue's criterion — the oracle's widths at a limit of 60 exceed 15 — implies that the build's clamp is in force"""
    rng = np.random.default_rng(3)
    for trial in range(200):
        n = int(rng.integers(2, 60))
        f = rng.integers(1, 5, n) if trial % 2 else np.array(hc.fib(n))
        assert depth_queue_runs(f)[0] >= int(max(oracle.huff_widths(f, 60)))
        if trial % 2 == 0:
            assert depth_queue_runs(f)[0] == n - 1 == int(max(oracle.huff_widths(f, 60)))


def test_group_i_alternates_its_shapes(ffi, oracle):
    """group i: every seventh block is the clamped full alphabet; the blocks between have 1, 2, 3, 257, 257 and 10 symbols"""
    case = hc.BY_NAME["i_350_unlike_blocks"]
    hists, _ = block_hists(ffi, oracle, case)
    assert len(hists) == 351
    ns = [int((h[:286] > 0).sum()) for h in hists]
    assert ns[:7] == [257, 1, 2, 3, 257, 257, 10] and ns[:350] == ns[:7] * 50 and ns[350] == 1
    for h in hists[0:350:7]:
        assert int(max(oracle.huff_widths(h[:286], 60))) > 15
    for h in hists[5:350:7]:
        assert int(max(oracle.huff_widths(h[:286], 60))) == 9


# ---- 2: the one-lane build over the whole catalogue ------------------------------------------------------------------------
def header_bytes(hdr, hbits):
    v = 0
    for i, w in enumerate(hdr):
        v |= int(w) << (32 * i)
    return v & ((1 << hbits) - 1)


def oracle_header_symbols(raw):
    """the code-length symbols (0..18) that the header of the first block of a raw DEFLATE stream is written with, read back
    from the stream (RFC 1951 3.2.7) — what header_entries() restates"""
    v = int.from_bytes(raw[:700], "little")                      # (a header is at most 17 + 57 + 316 * 14 bits)
    assert (v >> 1) & 3 == 2
    nl, nd, nc = 257 + ((v >> 3) & 31), 1 + ((v >> 8) & 31), 4 + ((v >> 13) & 15)
    at, cl = 17, [0] * 19
    for k in range(nc):
        cl[merge_model.CLEN_ORDER[k]] = (v >> at) & 7
        at += 3
    table, syms, n = merge_model._decoder(cl), [], 0
    while n < nl + nd:
        s, at = merge_model._symbol(v, at, table)
        syms.append(s)
        if s < 16:
            n += 1
        else:
            bits, base = {16: (2, 3), 17: (3, 3), 18: (7, 11)}[s]
            n += base + ((v >> at) & ((1 << bits) - 1))
            at += bits
    assert n == nl + nd
    return syms, nl, nd


@pytest.mark.parametrize("name", hc.NAMES)
def test_one_lane_build_equals_oracle(ffi, oracle, name):
    case = hc.BY_NAME[name]
    spec = case.make()
    hists, _ = block_hists(ffi, oracle, case, spec)
    seen = set()
    for h in hists:
        key = h.tobytes()
        if key in seen:                                          # (group i repeats its shapes)
            continue
        seen.add(key)
        lit, dst, hdr, hbits, body = huff_block(ffi, h, 2)
        lw, dw = oracle.huff_widths(h[:286], 15), oracle.huff_widths(dist_counts(h), 15)
        assert list(lit[:286] >> 16) == list(lw)
        assert list(dst[:30] >> 16) == list(dw)
        assert list(lit[:286] & 0xFFFF) == list(oracle.huff_codes(lw))
        assert list(dst[:30] & 0xFFFF) == list(oracle.huff_codes(dw))
        # the header: the oracle's encoder writes the same block (BFINAL, BTYPE, the header, the code words) from a code list
        # with this histogram — every histogram of the catalogue but the 16 MiB ones is small enough to go through as one
        if int(h.sum()) <= 70000:
            codes = spec if case.driver == "codes" else hc.codes_of_hist(h, 70000)
            want = oracle.encode(oracle.DEFLATE, b"x", **oracle.custom_lz77(_CannedCodes(codes)))
            assert _one_final_block(ffi, codes) == want
            assert header_bytes(hdr, hbits) == (int.from_bytes(want, "little") >> 3) & ((1 << hbits) - 1)
        else:
            # (too many code words for a list: the widths and codes above, and the header's bits against the oracle's encode of
            #  the case's own data, whose one block this is)
            assert len(hists) == 1
            want = hc.oracle_stream(oracle, oracle.DEFLATE, spec)
            assert header_bytes(hdr, hbits) == (int.from_bytes(want[:512], "little") >> 3) & ((1 << hbits) - 1)
            assert 8 * len(want) - 7 <= body <= 8 * len(want)
        # the restatement the claims of group d rest on writes the header with the very symbols the oracle's stream holds
        syms, nl, nd = oracle_header_symbols(want)
        assert syms == hc.header_entries(lw[:nl], dw[:nd])
        assert nl == max(257, int(np.nonzero(lw)[0].max()) + 1) and nd == max(1, int(np.nonzero(dw)[0].max()) + 1)


# ---- 3: LFX_PACK_BY_CHUNK=1 takes the chunk path for every byte input of the catalogue ------------------------------------------
def test_chunk_path_is_legal_for_every_byte_case(tmp_path):
    """encode_geometry (lfx_encode_stages.h, host code) over the real Planner's plan of every bytes / parse case, by
    tests/c/huff_geom.cpp: with the switch on the chunk path is taken — chunks of lz77_kind = 1 included —, with it off never.
    (The context's phase record names the same phases on both paths, so the GPU test cannot see this for itself.)"""
    import os
    import shutil
    import subprocess
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "huff_geom")
    subprocess.run([gxx, "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(root, "tests", "c", "huff_geom.cpp")], check=True)
    literal = 0
    for case in hc.CASES:
        if case.driver == "codes":
            continue
        spec = case.make()
        n, ws, writes, o = len(spec["data"]), spec["write_size"], spec["writes"], spec["opts"]
        if writes is None:
            writes = [n] if ws == 0 else [ws] * (n // ws) + ([n % ws] if n % ws else [])
        args = [str(o.get("lz77_kind", 0)), str(o.get("window_size", 32768)), str(o["block_size"])] + ["f" if w is None else str(w) for w in writes]
        out = subprocess.run([exe] + args, capture_output=True, text=True, check=True).stdout
        got = dict(kv.split("=") for kv in out.split())
        assert got["on"] == "1" and got["off"] == "0" and got["fused_hist"] == "1" and got["err"] == "0", (case.name, out)
        if "chunks" in case.claim:
            assert int(got["chunks"]) == case.claim["chunks"] and int(got["blocks"]) == case.claim["blocks"], (case.name, out)
        literal += int(got["literal_chunks"]) > 0
    assert literal > 25


# ---- 4: the GPU module runs exactly the catalogue ---------------------------------------------------------------------------
def test_all_cases_are_run():
    import ast
    import os
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_huff_crafted.py")).read()
    tree = ast.parse(src)
    assert "skip" not in src and "xfail" not in src
    # the GPU module parametrises over these three lists and nothing else; together they are the catalogue
    names = {}
    for node in tree.body:
        if isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Name) and node.targets[0].id in ("BYTES", "CODES", "PARSE"):
            names[node.targets[0].id] = ast.unparse(node.value)
    assert names == {"BYTES": "[c.name for c in hc.CASES if c.driver == 'bytes']", "CODES": "[c.name for c in hc.CASES if c.driver == 'codes']",
                     "PARSE": "[c.name for c in hc.CASES if c.driver == 'parse']"}
    used = [ast.unparse(d) for f in tree.body if isinstance(f, ast.FunctionDef) for d in f.decorator_list]
    for lst in ("BYTES", "CODES", "PARSE"):
        assert "pytest.mark.parametrize('name', %s)" % lst in used
    assert sorted(hc.NAMES) == sorted(c.name for c in hc.CASES if c.driver in ("bytes", "codes", "parse"))
    assert {c.group for c in hc.CASES} == set("abcdefghi")
    assert len(hc.header_code_lists()) == hc.N_HEADER_LISTS
