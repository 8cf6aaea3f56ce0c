"""The dictionary trainer's definition (include/lfx.h "training a preset dictionary") in numpy: a simplified
FASTCOVER.  lfx_dict_train_device / _host must return these bytes.

  - The records, in the order given, concatenated, are the position space [0, N).
  - h(p) = (le64(bytes at p) * 0x9E3779B185EBCA87 mod 2^64) >> (64 - F), defined where p + D does not pass the end of p's record.
  - freq[x]: the number of defined positions with h(p) == x.
  - E = dict_size // k epochs; epoch e owns the positions [e * N // E, (e + 1) * N // E).
  - A position is a candidate when p + k stays inside its record.  Its score is the sum of freq[h(q)] over q in [p, p + k - D],
    read as the counters stand when its epoch is decided, and held in 32 bits: a sum above 2^32 - 1 counts as 2^32 - 1.
  - Epochs are decided in order: the highest score, among equal scores the lowest position; a best score of 0 picks nothing.
    After a pick freq[h(q)] = 0 for every q of the picked segment.
  - The dictionary is the picked segments sorted by score ascending, among equal scores the earlier epoch later.
"""
import numpy as np

D = 8
F = 20
PRIME = np.uint64(0x9E3779B185EBCA87)
SCORE_MAX = (1 << 32) - 1


def hashes(cat):
    """h(p) for every p with p + D <= len(cat) (record ends are the caller's business) → uint32 array"""
    n = len(cat)
    if n < D:
        return np.zeros(0, dtype=np.uint32)
    v = np.zeros(n - D + 1, dtype=np.uint64)
    for b in range(D):
        v |= cat[b:n - D + 1 + b].astype(np.uint64) << np.uint64(8 * b)
    with np.errstate(over="ignore"):
        v = v * PRIME
    return (v >> np.uint64(64 - F)).astype(np.uint32)


def train_flat(buf, offs, lens, dict_size, k=128):
    """buf: bytes-like; record i is buf[offs[i], offs[i] + lens[i]) → (dictionary bytes, picks) with picks =
    [(epoch, position, score)] in epoch order"""
    assert 64 <= dict_size <= 32768 and 16 <= k <= dict_size
    buf = np.frombuffer(bytes(buf), dtype=np.uint8)
    recs = [buf[o:o + n] for o, n in zip(offs, lens) if n]
    if not recs:
        return b"", []
    cat = np.concatenate(recs)
    n = len(cat)
    assert n <= 1 << 31
    rl = np.array([len(r) for r in recs], dtype=np.int64)
    ends = np.cumsum(rl)
    rec_end = np.repeat(ends, rl)                         # the end of p's record, in positions
    pos = np.arange(n, dtype=np.int64)
    defined = pos + D <= rec_end
    h = np.zeros(n, dtype=np.int64)
    hh = hashes(cat)
    h[:len(hh)] = hh
    freq = np.bincount(h[defined], minlength=1 << F).astype(np.uint32)
    cand = pos + k <= rec_end
    epochs = dict_size // k
    picks = []
    for e in range(epochs):
        lo, hi = e * n // epochs, (e + 1) * n // epochs
        if hi <= lo:
            continue
        s1 = min(hi + k - D, n)                           # the d-mers a candidate of [lo, hi) can read
        f = np.where(defined[lo:s1], freq[h[lo:s1]], 0).astype(np.uint64)
        x = np.concatenate([[0], np.cumsum(f, dtype=np.uint64)]).astype(np.uint64)
        p = np.arange(lo, hi)
        c = cand[lo:hi]
        score = np.zeros(hi - lo, dtype=np.uint64)
        pc = p[c] - lo
        score[c] = np.minimum(x[pc + k - D + 1] - x[pc], np.uint64(SCORE_MAX))
        best = int(np.argmax(score))                      # the first of the highest: the lowest position
        if score[best] == 0:
            continue
        at = lo + best
        picks.append((e, at, int(score[best])))
        freq[h[at:at + k - D + 1]] = 0
    order = sorted(picks, key=lambda t: (t[2], -t[0]))
    out = b"".join(cat[at:at + k].tobytes() for _e, at, _s in order)
    return out, picks


def train(records, dict_size, k=128):
    """records: a list of bytes → the dictionary"""
    records = [bytes(r) for r in records]
    offs, at = [], 0
    for r in records:
        offs.append(at)
        at += len(r)
    return train_flat(b"".join(records), offs, [len(r) for r in records], dict_size, k)[0]
