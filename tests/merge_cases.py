"""Inputs shared by test_merge_model.py (CPU) and test_gpu_block_merge.py (GPU): seeded, small, and chosen so that the
block_merge rule (merge_model.py) meets a full merge, kept cuts, partial right children, the region seam and its ties."""
import random

import auto_cases as cases

BS = 4096                                    # block_size and write size of most cases: a candidate per 4096 bytes


def text(n, seed=0):
    return cases.record(n, seed)


def sections():
    """text ‖ random ‖ zeros ‖ text, 8 KiB each: two candidates per section, and one statistics per section"""
    return text(8192, 1) + cases.rand(8192, 2) + bytes(8192) + text(8192, 3)


def run_of(n):
    """homogeneous text that plans into exactly n candidates at BS-byte writes: the last one is short (a length that is a
    multiple of BS would end with one more, empty, candidate)"""
    return text((n - 1) * BS + 1000, 10 + n)


RUNS = (1, 2, 3, 15, 16, 17, 33)
# what homogeneous text must give: everything merges, up to the region seam (groups as (first, count))
RUN_GROUPS = {1: [(0, 1)], 2: [(0, 2)], 3: [(0, 3)], 15: [(0, 15)], 16: [(0, 16)], 17: [(0, 16), (16, 1)], 33: [(0, 16), (16, 16), (32, 1)]}

# two candidates — 512 bytes of text, then 40 random bytes, block_size = 512 — whose one node has D(node) - D(left) - D(right) =
# -1, 0, +1: whole, whole, not whole.  Found by a search over the seed on the CPU (merge_model.merge's nodes); the differences
# are asserted in test_merge_model.py.
TIE_BS = 512
TIES = ((39, -1), (1, 0), (137, 1))


def tie(seed):
    return cases.record(TIE_BS, seed) + cases.rand(40, seed)


def batch_records(count=200, seed=5):
    """records of 0..20 000 bytes: text, every seventh random bytes; the first three 0, 1 and 20 000 bytes"""
    r = random.Random(seed)
    sizes = [0, 1, 20000] + [r.randint(0, 20000) for _ in range(count - 3)]
    return [cases.rand(n, i) if i % 7 == 6 else text(n, i) for i, n in enumerate(sizes)]
