"""The contract of block_merge (include/lfx.h) restated in plain Python, and the stream it implies.  Test
infrastructure: checked against the oracle and python-zlib (test_merge_model.py), never against the library.

The plan and the LZ77 code words are those of block_merge = 0, so the model starts from the `= 0` stream of the call (the
oracle's, or that of another model: a dictionary, an opt-in LZ77 kind), cuts it at the oracle's scan_blocks and reads every
dynamic block's code words back.  Every size D(node) is the ORACLE's: the node's code words go through it as one block
(oracle custom Lz77Encode, one write, a block_size beyond it) and scan_blocks measures what came out — there is no second
Huffman builder here.  The final stream is written the same way: a group's block is the oracle's block over its code words.
"""
import ctypes as C

import numpy as np

import auto_block_model as abm

STORED, FIXED, DYNAMIC = 0, 1, 2
MERGE_MAX = 16
CLEN_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


# ---- reading a dynamic block's code words back (RFC 1951 3.2.7)
def _decoder(lengths):
    """canonical code → {(width, code read MSB-first): symbol}"""
    code, table = 0, {}
    for w in range(1, 16):
        for s, l in enumerate(lengths):
            if l == w:
                table[(w, code)] = s
                code += 1
        code <<= 1
    return table


def _symbol(v, at, table):
    code = 0
    for w in range(1, 16):
        code = (code << 1) | ((v >> at) & 1)
        at += 1
        s = table.get((w, code))
        if s is not None:
            return s, at
    raise ValueError("no such code")


def block_words(v, start):
    """v: the raw DEFLATE data as one little-endian integer; start: the first bit of a dynamic block → (its code words
    (value << 16 | distance, the oracle's own form) without the EndOfBlock, the bit behind the block)"""
    assert (v >> (start + 1)) & 3 == DYNAMIC
    at = start + 3
    nl, nd, nc = 257 + ((v >> at) & 31), 1 + ((v >> (at + 5)) & 31), 4 + ((v >> (at + 10)) & 15)
    at += 14
    cl = [0] * 19
    for k in range(nc):
        cl[CLEN_ORDER[k]] = (v >> at) & 7
        at += 3
    tcl, lens = _decoder(cl), []
    while len(lens) < nl + nd:
        s, at = _symbol(v, at, tcl)
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + ((v >> at) & 3))
            at += 2
        elif s == 17:
            lens += [0] * (3 + ((v >> at) & 7))
            at += 3
        else:
            lens += [0] * (11 + ((v >> at) & 127))
            at += 7
    assert len(lens) == nl + nd
    tl, td = _decoder(lens[:nl]), _decoder(lens[nl:])
    # a 9-bit first-level table for the literal/length code: most symbols are one lookup
    fast = {}
    for (w, code), s in tl.items():
        if w <= 9:
            rev = int(format(code, "0%db" % w)[::-1], 2)
            for hi in range(1 << (9 - w)):
                fast[rev | hi << w] = (s, w)
    words = []
    while True:
        hit = fast.get((v >> at) & 511)
        if hit:
            s, at = hit[0], at + hit[1]
        else:
            s, at = _symbol(v, at, tl)
        if s < 256:
            words.append(s << 16)
        elif s == 256:
            return words, at
        else:
            e = LEN_EXTRA[s - 257]
            length = LEN_BASE[s - 257] + ((v >> at) & ((1 << e) - 1))
            at += e
            d, at = _symbol(v, at, td)
            e = DIST_EXTRA[d]
            words.append(length << 16 | (DIST_BASE[d] + ((v >> at) & ((1 << e) - 1))))
            at += e


# ---- one block over given code words, by the oracle
def oracle_block(oracle, words, n_bytes, dynamic_huffman=1):
    """the oracle's DEFLATE block over `words` (an EndOfBlock behind them), for n_bytes of input behind it → (its bits
    as an integer — bit 0 is BFINAL, set —, their number)"""
    arr = np.asarray(words if len(words) else [0], dtype=np.uint32)
    state = {"left": len(words)}

    def cb(_user, p, n, out):
        if p:                                   # Lz77Encode::encode: buffers, emits nothing
            return 0
        k, state["left"] = state["left"], 0     # Lz77Encode::flush: everything, once
        out[0] = C.cast(arr.ctypes.data, C.POINTER(C.c_uint32))
        return k

    fn = oracle.CUSTOM_CB(cb)
    raw = oracle.encode(oracle.DEFLATE, b"\0" * n_bytes, lz77_kind=oracle.LZ77_CUSTOM, custom_cb=C.cast(fn, C.c_void_p).value,
                        custom_level=2, block_size=n_bytes + 1, dynamic_huffman=dynamic_huffman)
    # (scan_blocks inflates: the code words reach back into candidates in front of the node, or into a dictionary — 32 KiB of
    #  history go in front as a stored block, which ends on a byte boundary, and are taken off the answer again)
    pre = b"\x00\x00\x80\xff\x7f" + bytes(32768)
    blocks = [(s - 8 * len(pre), e - 8 * len(pre), t, f) for s, e, t, f, _ in oracle.scan_blocks(pre + raw)[1:]]
    assert len(blocks) == 1 and blocks[0][0] == 0 and blocks[0][3] == 1, blocks
    nbits = blocks[0][1]
    return int.from_bytes(raw, "little") & ((1 << nbits) - 1), nbits


# ---- the rule
def tree(n, D):
    """n candidates of one run, D(lo, hi) = the exact size of one block over the candidates [lo, hi) → head[i] for every
    candidate: the first candidate of its group.  Regions of MERGE_MAX; in each the fixed binary tree, bottom-up."""
    head = list(range(n))
    for r0 in range(0, n, MERGE_MAX):
        m = min(MERGE_MAX, n - r0)

        def node(lo, span):
            """→ (whole, size) of the node [lo, min(lo + span, m)) of the region, lo < m"""
            if span == 1:
                return True, D(r0 + lo, r0 + lo + 1)
            half = span // 2
            left = node(lo, half)
            if lo + half >= m:                  # an empty right child: the node is its left child
                return left
            right = node(lo + half, half)
            hi = min(lo + span, m)
            if left[0] and right[0]:
                d = D(r0 + lo, r0 + hi)
                if d <= left[1] + right[1]:
                    for i in range(lo, hi):
                        head[r0 + i] = r0 + lo
                    return True, d
            return False, None

        node(0, MERGE_MAX)
    return head


def merge(oracle, raw, data, zdict=None, dynamic_huffman=1):
    """raw: the raw DEFLATE data of the block_merge = 0 encode of `data` → (the raw DEFLATE data of the block_merge = 1
    encode, head[b] for every block b of `raw` in order: the block it ends up in, [(lo, hi, D) per node evaluated]).
    dynamic_huffman = 0: the same groups, every group's block in its fixed form (what LFX_HUFFMAN_AUTO chooses from)."""
    blocks = abm.scan(oracle, raw, zdict)
    v = int.from_bytes(raw, "little")
    words, lens, at = [], [], 0
    for s, e, btype, bfinal, n in blocks:
        if btype == DYNAMIC:
            w, end = block_words((v >> s) & ((1 << (e - s)) - 1), 0)
            assert end == e - s
            words.append(w)
        else:
            assert btype == STORED
            words.append(None)
        lens.append(n)
        at += n
    assert at == len(data)
    head, nodes, cache = list(range(len(blocks))), [], {}
    b = 0
    while b < len(blocks):
        if words[b] is None:
            b += 1
            continue
        e = b
        while e < len(blocks) and words[e] is not None:
            e += 1
            if blocks[e - 1][3]:
                break

        def D(lo, hi, b=b):
            key = (b + lo, b + hi)
            if key not in cache:
                w = [x for q in range(*key) for x in words[q]]
                cache[key] = (w, sum(lens[key[0]:key[1]]), oracle_block(oracle, w, sum(lens[key[0]:key[1]])))
                nodes.append((key[0], key[1], cache[key][2][1]))
                if hi == lo + 1:                # a leaf: the oracle writes the very block the base stream holds
                    assert cache[key][2][1] == blocks[key[0]][1] - blocks[key[0]][0]
            return cache[key][2][1]

        for i, h in enumerate(tree(e - b, D)):
            head[b + i] = b + h
        b = e
    out, pos = abm._Bits(), 0
    for i, (s, e, btype, bfinal, n) in enumerate(blocks):
        if btype == STORED:                     # RawBuf::flush encode.rs:364-382
            out.put(bfinal, 3)
            out.align()
            out.put(n | ((n ^ 0xFFFF) << 16), 32)
            out.put(int.from_bytes(data[pos:pos + n], "little"), 8 * n)
        elif head[i] == i:
            j = i + 1
            while j < len(blocks) and head[j] == i:
                j += 1
            w, nb, (bits, nbits) = cache[(i, j)]
            if dynamic_huffman == 0:
                bits, nbits = oracle_block(oracle, w, nb, 0)
            out.put((bits & ~1) | blocks[j - 1][3], nbits)
        pos += n
    return out.bytes(), head, nodes


def expected(oracle, fmt, base, data, zdict=None, auto=False):
    """fmt: "deflate", "zlib" or "gzip"; base: the whole block_merge = 0, dynamic_huffman = 1 stream of one call over `data` →
    (the bytes the block_merge = 1 call must write, head per block of the plan, nodes).  The container header and the trailer
    are the base stream's.  auto: dynamic_huffman = LFX_HUFFMAN_AUTO — the form is chosen per merged block behind the merge
    (auto_block_model's rule over the merged stream and its fixed twin)."""
    data = bytes(data)
    h, t = abm.header_len(fmt, base), abm.TRAILER[fmt]
    raw, head, nodes = merge(oracle, base[h:len(base) - t], data, zdict)
    tail = base[len(base) - t:] if t else b""
    if not auto:
        return base[:h] + raw + tail, head, nodes
    fix = merge(oracle, base[h:len(base) - t], data, zdict, dynamic_huffman=0)[0]
    stream, choices, _ = abm.expected_stream(oracle, fmt, base[:h] + raw + tail, base[:h] + fix + tail, data, True, zdict)
    return stream, head, nodes, choices


def groups(head):
    """head per block → the groups as (first, count), heads in order"""
    out = []
    for i, h in enumerate(head):
        if h == i:
            out.append([i, 1])
        else:
            assert out and out[-1][0] == h
            out[-1][1] += 1
    return [tuple(g) for g in out]
