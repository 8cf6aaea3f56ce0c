"""Inputs shared by test_auto_block_model.py (CPU) and test_gpu_auto_blocks.py (GPU): seeded, small, and chosen so that the
LFX_HUFFMAN_AUTO rule (auto_block_model.py) meets each of its three answers and its edges."""
import random

import numpy as np


def record(n, seed=0):
    """a JSON-like record cut to n bytes"""
    r = random.Random(1000 + seed)
    keys = ["id", "user", "ts", "level", "msg", "host", "path", "status", "bytes", "tags"]
    words = ["alpha", "beta", "gamma", "delta", "error", "warn", "info", "GET", "POST", "/api/v1/items", "/index.html", "node-7"]
    out = []
    while sum(len(x) for x in out) < n + 1:
        k = r.choice(keys)
        v = r.choice(words) if r.random() < 0.5 else str(r.randint(0, 99999))
        out.append('{"%s": "%s", "%s": %d}\n' % (k, v, r.choice(keys), r.randint(0, 999)))
    return "".join(out).encode()[:n]


def rand(n, seed=7):
    return np.random.RandomState(seed).randint(0, 256, size=n, dtype=np.uint8).tobytes()


def literals(n_low, n_high):
    """distinct bytes without a 3-byte repeat: n_low of them below 144 (8-bit fixed codes), n_high from 144 on (9-bit).  Its one
    block is all literals and the end of block: F = 3 + 8 * n_low + 9 * n_high + 7, S = 8 * n + 42, D whatever the dynamic header
    of so many equally frequent symbols costs."""
    assert n_low <= 144 and n_high <= 112
    low, high = list(range(n_low)), list(range(144, 144 + n_high))
    out = []
    while low or high:                       # interleaved: no run, no repeat
        if low:
            out.append(low.pop())
        if high:
            out.append(high.pop())
    return bytes(out)


# one block each, around S == min(D, F): (data, min(D, F) - S) — found by a search over literals(); the sizes are asserted in
# test_auto_block_model.py.  S must be SMALLER to win: -1 and 0 stay compressed, +1 is stored.
S_EDGE = [(literals(0, 93), -1), (literals(0, 35), 0), (literals(0, 105), 1)]
# F == D (both 1 block of 94 text bytes): the tie goes to the fixed form
TIE = (94, 14)                               # record(94, 14)

SIZES = (0, 1, 16, 64, 128, 256, 1024)


def mixed():
    """text ‖ random ‖ zeros ‖ 16 bytes, 4096 each: with 4096-byte writes and block_size = 4096 a dynamic, a stored, a
    dynamic and a fixed block"""
    return record(4096, 3) + rand(4096, 5) + bytes(4096) + record(16, 4)


# text prefixes in front of `mixed`, written as a write of their own: the first block grows by them, and the stored block behind
# it starts at bit phase 0, 1, ... 7 of a byte (asserted in test_auto_block_model.py)
PHASE_PREFIX = (1, 14, 7, 5, 25, 2, 8, 3)


def prefixed(length):
    """→ (data, writes): record(length, 77) ‖ mixed(), written as `length` bytes and then 4096 at a time"""
    return record(length, 77) + mixed(), [length, 4096, 4096, 4096, 16]


def messages(seed=11, count=12):
    """the stream encoder's messages: 10..2000 bytes, text and random ones"""
    r = random.Random(seed)
    out = []
    for i in range(count):
        n = r.randint(10, 2000)
        out.append(rand(n, 100 + i) if i % 4 == 2 else record(n, 50 + i))
    return out


def batch_records(count=300):
    """record i has i bytes; every seventh is random bytes"""
    return [rand(i, i) if i % 7 == 6 else record(i, i) for i in range(count)]


DICT = b"".join(record(200, 900 + i) for i in range(40))       # 8000 bytes of the records' vocabulary
