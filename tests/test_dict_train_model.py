"""CPU: the dictionary trainer's definition (tests/dict_train_model.py) — properties of the model, the crafted
cases' intent, and what a trained dictionary is worth against Python's zlib at level 6 on held-out records."""
import zlib

import pytest

import dict_train_cases as cases
import dict_train_model as model


@pytest.fixture(scope="module")
def corpus():
    recs = cases.log_lines(4096 + 1024, 7)
    return recs[:4096], recs[4096:]


def test_length_substrings_determinism():
    recs = cases.log_lines(300, 3)
    for size, k in ((2048, 128), (1000, 128), (64, 16), (777, 100), (256, 256)):
        d = model.train(recs, size, k)
        assert len(d) % k == 0 and 0 < len(d) <= size
        for i in range(0, len(d), k):
            assert any(d[i:i + k] in r for r in recs), (size, k, i)      # every segment lies inside ONE record
        assert d == model.train(list(recs), size, k)


def test_identical_records_one_pick_per_content():
    a, b = cases.log_lines(2, 5)
    a, b = a[:128], b[10:138]
    # one content: the first epoch takes it and clears its counters, every later epoch finds only zeros
    assert model.train([a] * 50, 2048, 128) == a
    # two contents: one pick each, whatever their order and number
    d = model.train([a] * 30 + [b] * 20 + [a] * 5, 2048, 128)
    assert len(d) == 256 and sorted([d[:128], d[128:]]) == sorted([a, b])
    # the more frequent one scores higher and lies last
    assert d[128:] == a


def test_crafted_cases_mean_what_they_say():
    by_name = {c[0]: c for c in cases.cases()}
    exp = lambda n: cases.expect(by_name[n])
    rec = lambda n, i: by_name[n][1][by_name[n][2][i]:by_name[n][2][i] + by_name[n][3][i]]
    assert exp("shorter_than_a_dmer") == (b"", []) and exp("k_minus_1") == (b"", [])
    d, picks = exp("exactly_k")
    assert d == rec("exactly_k", 0) and picks == [(0, 0, 121)]
    # two candidates of equal score in one epoch: the lower position
    d, picks = exp("tie_in_one_epoch")
    assert picks == [(0, 0, 121)] and d == rec("tie_in_one_epoch", 0)
    # ... and in two epochs: both picked with the same score, the earlier epoch later
    d, picks = exp("tie_across_epochs")
    assert picks == [(0, 0, 121), (1, 128, 121)] and d == rec("tie_across_epochs", 1) + rec("tie_across_epochs", 0)
    # the seam: the 128 hot bytes lie across two records; the pick is a whole record, not the hot bytes
    name, buf, offs, lens, _size, _k = by_name["seam"]
    hot = buf[offs[0] + 64:offs[0] + 128] + buf[offs[1]:offs[1] + 64]
    assert buf[offs[0] + 64:offs[1] + 64] == hot              # ... which a trainer blind to seams would see, and score highest
    d, picks = exp("seam")
    assert len(picks) == 1 and d != hot and d in (rec("seam", 0), rec("seam", 1))
    # N < E: most epochs own no position at all
    _d, picks = exp("n_below_epochs")
    assert 0 < len(picks) < 300
    # identical records: the zeroing starves the later epochs
    d, picks = exp("identical_records")
    assert len(picks) < 16


def test_trained_2k_beats_the_first_2k(corpus):
    """The issue's measurement: held-out records through zlib.compressobj(6, zdict=...); the trained 2 KiB dictionary at segment
    128 against the first 2 KiB of the samples.  The prototype measured a ratio of 0.75; below 0.85 is asserted."""
    train, held = corpus

    def size(zdict):
        total = 0
        for r in held:
            c = zlib.compressobj(6, zdict=zdict) if zdict else zlib.compressobj(6)
            total += len(c.compress(r) + c.flush())
        return total

    trained = model.train(train, 2048, 128)
    first = b"".join(train)[:2048]
    s_trained, s_first, s_none = size(trained), size(first), size(b"")
    ratio = s_trained / s_first
    print("held-out %d records, %d bytes raw: no dictionary %d, trained 2 KiB %d, first 2 KiB %d, ratio %.4f"
          % (len(held), sum(map(len, held)), s_none, s_trained, s_first, ratio))
    assert len(trained) == 2048
    assert s_trained < s_first and ratio < 0.85, (s_trained, s_first, ratio)
