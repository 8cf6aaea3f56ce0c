"""CPU: the model of LevelLz77Encoder (tests/level_model.py) against the models of ChainLz77Encoder and
LazyLz77Encoder, which their own tests prove, and against python-zlib — never against the library.  With the three new rules
switched off (nice = 258, max_lazy above 258, too_far beyond the window) the model is lazy_model's, and its greedy form
chain_model's; crafted buffers pin each rule on both sides of its threshold; the stream the model implies is read by
python-zlib at every level and in every format, and its header bytes say Fast, Balance or Best.

The builders below are the GPU cases' too (test_gpu_level_encode.py): each returns (hist, tail), and put() lays `tail` at a
chosen position with `hist` right in front of it, inside filler of bytes 128..255 that shares no 3-byte prefix with them."""
import gzip
import zlib

import pytest

import chain_model as cm
import lazy_model as lm
import level_model as vm
from test_chain_model import BUFS
from test_dict_encode_model import _rand, _text

NEVER = vm.NEVER
MIXED = _text(9000, 62) + b"a" * 700 + _rand(500, 63)


def _fill(n, seed):
    return bytes(128 + (v & 127) for v in _rand(n, seed))


def _phrase(n, seed):
    """n bytes of 1..100 whose first three occur nowhere else in them"""
    while True:
        p = bytes(1 + v for v in _rand(n, seed, alphabet=100))
        if p.find(p[:3], 1) < 0:
            return p
        seed += 1000


def put(hist, tail, at=None, total=0, seed=90):
    """→ (buf, at): `tail` at position `at` (default: right behind hist), hist in front of it, filler around"""
    at = len(hist) if at is None else at
    assert at >= len(hist)
    total = max(total, at + len(tail) + 8)
    fill = _fill(total, seed)
    buf = fill[:at - len(hist)] + hist + tail
    return buf + fill[len(buf):], at


def nice_case(nice, reach):
    """at `tail`: the nearest candidate matches `reach` bytes (nice or nice - 1), an older one nice + 8"""
    p = _phrase(nice + 8, 7)
    hist = b"\x7e\x7e" + p + b"\x7d\x7d" + p[:reach] + b"\x7c\x7c"
    return hist, p + b"\x7b\x7b"


def far_case(dist, length):
    """at `tail`: one candidate, `length` (3 or 4) bytes long and `dist` back"""
    word = b"xyzw"[:length]
    hist = word + b"A" + _fill(dist - length - 1, 17)
    assert len(hist) == dist
    return hist, word + b"B"


def lazy_case(first, second):
    """L(at) = first and L(at + 1) = second > first (test_lazy_model.long_pair for any lengths)"""
    B = _phrase(second + 12, 80)
    x = b"\x6f"
    hist = b"\x7e\x7e" + x + B[:first - 1] + b"\x7d\x7d" + B[:second] + b"\x7c\x7c"
    return hist, x + B + b"\x7b\x7b\x7b"


def deep_case(links=300):
    """at `tail`: `links` candidates of 3 bytes, and behind them, beyond the 255th link, one of 36"""
    long = b"abcdefghijklmnopqrstuvwxyz0123456789"
    noise = b"".join(b"abc" + bytes([128 + i % 100, 230 + i // 100]) for i in range(links))
    return long + b"\x7e\x7e" + noise, long + b"!!!!"


# ---------------------------------------------------------------------------------------------- the rules switched off
@pytest.mark.parametrize("depth", [1, 2, 8, 40])
@pytest.mark.parametrize("window,max_len", [(32768, 258), (1024, 258), (32768, 16)])
def test_without_the_new_rules_it_is_the_lazy_and_the_chain_model(depth, window, max_len):
    for buf in BUFS + [MIXED[:4000]]:
        assert vm.tuned_codes(buf, depth, True, 258, 259, NEVER, window, max_len) == lm.lazy_codes(buf, depth, window, max_len)
        assert vm.tuned_codes(buf, depth, False, 258, NEVER, NEVER, window, max_len) == cm.chain_codes(buf, depth, window, max_len)
        assert vm.lengths(buf, depth, 258, NEVER, window, max_len) == lm.lengths(buf, depth, window, max_len)


def test_the_table():
    assert sorted(vm.TABLE) == list(range(1, 10))
    assert [vm.TABLE[v][0] for v in range(1, 10)] == [4, 8, 32, 16, 32, 128, 256, 1024, 4096]
    assert [vm.TABLE[v][1] for v in range(1, 10)] == [False] * 3 + [True] * 6
    assert [vm.TABLE[v][2] for v in range(1, 10)] == [8, 16, 32, 16, 32, 128, 128, 258, 258]
    assert [vm.TABLE[v][3] for v in range(4, 10)] == [4, 16, 16, 32, 128, 258]
    assert all(vm.TABLE[v][4] == 4096 for v in range(4, 10)) and all(vm.TABLE[v][3:] == (NEVER, NEVER) for v in (1, 2, 3))


@pytest.mark.parametrize("level", range(1, 10))
def test_code_words_replay_inside_window_and_cap(level):
    for buf, window, max_len in [(b, 32768, 258) for b in BUFS] + [(MIXED, 1024, 258), (MIXED, 32768, 16), (MIXED[:3000], 300, 5)]:
        codes = vm.level_codes(buf, level, window, max_len)
        assert vm.replay(codes) == buf
        assert all((c & 0xFFFF) <= window for c in codes) and all((c >> 16) <= max_len for c in codes if c & 0xFFFF)
        L, _ = vm.level_lengths(buf, level, window, max_len)
        assert all(L[p] == 0 for p in range(max(3, len(buf)) - 3, len(buf) + 1))


# ---------------------------------------------------------------------------------------------- nice
@pytest.mark.parametrize("level", [1, 3, 4, 6])
def test_a_nice_match_ends_the_walk(level):
    depth, lazy, nice = vm.TABLE[level][:3]
    buf, at = put(*nice_case(nice, nice))
    L, D = vm.level_lengths(buf, level)
    assert L[at] == nice and D[at] == nice + 2                       # the nearest: it reaches nice, the older one is not tried
    assert lm.lengths(buf, depth)[0][at] == nice + 8                 # (without the cut the older one wins)
    assert (nice << 16) | (nice + 2) in vm.level_codes(buf, level)
    buf, at = put(*nice_case(nice, nice - 1))
    L, D = vm.level_lengths(buf, level)
    assert L[at] == nice + 8 and D[at] == (nice - 1) + 2 + (nice + 8) + 2      # one byte short of nice: the walk goes on
    assert vm.replay(vm.level_codes(buf, level)) == buf


def test_nice_is_capped_by_max_length_and_by_the_end():
    """max_length below nice: a candidate of max_length bytes ends the walk (nothing can be longer), and the parse is the
    untuned one's at that cap"""
    for level, max_len in ((3, 6), (6, 16), (1, 3)):
        depth, lazy = vm.TABLE[level][:2]
        assert vm.level_lengths(MIXED, level, 32768, max_len) == vm.lengths(MIXED, depth, 258, vm.TABLE[level][4] if lazy else NEVER, 32768, max_len)
    buf, at = put(*nice_case(32, 32))
    assert vm.level_lengths(buf, 3, 32768, 20)[0][at] == 20
    # the end of the buffer caps lim below nice: the nearest candidate of lim bytes ends the walk
    hist, tail = nice_case(32, 32)
    buf = _fill(50, 5) + hist + tail[:10]
    L, D = vm.level_lengths(buf, 3)
    assert (L[len(buf) - 10], D[len(buf) - 10]) == (10, 34)


# ---------------------------------------------------------------------------------------------- too far
@pytest.mark.parametrize("level", [4, 6, 9])
def test_a_far_match_of_three_is_dropped(level):
    buf, at = put(*far_case(4096, 3))
    L, D = vm.level_lengths(buf, level)
    assert (L[at], D[at]) == (3, 4096) and (3 << 16) | 4096 in vm.level_codes(buf, level)
    buf, at = put(*far_case(4097, 3))
    L, D = vm.level_lengths(buf, level)
    assert (L[at], D[at]) == (0, 0) and lm.lengths(buf, 8)[0][at] == 3
    codes = vm.level_codes(buf, level)
    assert (3 << 16) | 4097 not in codes and vm.replay(codes) == buf
    buf, at = put(*far_case(4097, 4))
    L, D = vm.level_lengths(buf, level)
    assert (L[at], D[at]) == (4, 4097) and (4 << 16) | 4097 in vm.level_codes(buf, level)


@pytest.mark.parametrize("level", [1, 3])
def test_the_greedy_levels_keep_it(level):
    buf, at = put(*far_case(4097, 3))
    assert vm.level_lengths(buf, level)[0][at] == 3 and (3 << 16) | 4097 in vm.level_codes(buf, level)


# ---------------------------------------------------------------------------------------------- max_lazy
@pytest.mark.parametrize("level", [4, 6, 9])
def test_max_lazy(level):
    Z = vm.TABLE[level][3]
    second = min(Z + 6, 258)
    buf, at = put(*lazy_case(Z - 1, second))
    L, D = vm.level_lengths(buf, level)
    assert (L[at], L[at + 1]) == (Z - 1, second)
    codes = vm.level_codes(buf, level)
    assert (second << 16) | D[at + 1] in codes and ((Z - 1) << 16) | D[at] not in codes      # below max_lazy: deferred
    assert vm.replay(codes) == buf
    if Z < 258:                                                      # (a length of 258 has no longer successor)
        buf, at = put(*lazy_case(Z, second))
        L, D = vm.level_lengths(buf, level)
        assert (L[at], L[at + 1]) == (Z, second)
        codes = vm.level_codes(buf, level)
        assert (Z << 16) | D[at] in codes and (second << 16) | D[at + 1] not in codes        # max_lazy reached: taken
        assert codes != lm.lazy_codes(buf, vm.TABLE[level][0]) and vm.replay(codes) == buf


# ---------------------------------------------------------------------------------------------- depth beyond 255
def test_a_match_beyond_the_255th_link():
    buf, at = put(*deep_case(300))
    for level, want in ((6, 3), (7, 3), (8, 36), (9, 36)):
        L, D = vm.level_lengths(buf, level)
        assert L[at] == want, level
    L, D = vm.level_lengths(buf, 9)
    assert D[at] == 300 * 5 + 2 + 36
    c6, c9 = vm.level_codes(buf, 6), vm.level_codes(buf, 9)
    assert (36 << 16) | D[at] in c9 and (36 << 16) | D[at] not in c6
    assert vm.replay(c6) == buf and vm.replay(c9) == buf and c6 != c9


# ---------------------------------------------------------------------------------------------- placed cases, a dictionary
def test_placed_cases_sit_where_they_are_asked_for():
    for at in (16383, 16384):
        buf, p = put(*nice_case(16, 16), at=at, total=20000)
        assert p == at and vm.level_lengths(buf, 4)[0][at] == 16 and lm.lengths(buf, 16)[0][at] == 24
        buf, p = put(*far_case(4097, 3), at=at, total=20000)
        assert vm.level_lengths(buf, 6)[0][at] == 0 and lm.lengths(buf, 8)[0][at] == 3
        buf, p = put(*lazy_case(16, 22), at=at, total=20000)
        assert vm.level_lengths(buf, 6)[0][at:at + 2] == (16, 22)


def test_behind_a_dictionary():
    """the candidates run on into the dictionary's tail under the same rules"""
    import dict_chain_model as dcm
    hist, tail = nice_case(16, 16)
    codes = vm.primed_codes(hist, tail, 4)
    assert codes[0] == (16 << 16) | 18 and dcm.primed_codes(hist, tail, dcm.LAZY, 16)[0] == (24 << 16) | 44
    hist, tail = far_case(4097, 3)
    assert vm.primed_codes(hist, tail, 6)[0] == ord("x") << 16 and vm.primed_codes(hist, tail, 3)[0] == (3 << 16) | 4097
    T, buf = MIXED[:5000], MIXED[4000:7000]
    for level in (1, 6):
        codes = vm.primed_codes(T, buf, level)
        assert cm.replay([x << 16 for x in T] + codes) == T + buf


# ---------------------------------------------------------------------------------------------- streams
@pytest.mark.parametrize("level", range(1, 10))
def test_python_zlib_reads_every_stream_and_the_header_names_the_level(oracle, level):
    data = MIXED
    want_flevel, want_xfl = {1: (1, 4), 2: (2, 0), 3: (3, 2)}[vm.header_level(level)]
    assert vm.header_level(level) == (1, 1, 1, 2, 2, 2, 3, 3, 3)[level - 1]
    z = vm.expected_stream(oracle, oracle.ZLIB, data, level)
    assert zlib.decompress(z) == data and z[1] >> 6 == want_flevel and ((z[0] << 8) + z[1]) % 31 == 0
    g = vm.expected_stream(oracle, oracle.GZIP, data, level, mtime=0)
    assert gzip.decompress(g) == data and g[8] == want_xfl
    r = vm.expected_stream(oracle, oracle.DEFLATE, data, level, write_size=4096)
    assert zlib.decompress(r, -15) == data
    assert r == vm.expected_stream(oracle, oracle.DEFLATE, data, level, writes=[4096, 4096])
    # a caller's level is the one written; no_compression resets it
    assert vm.expected_stream(oracle, oracle.ZLIB, data, level, header=3)[1] >> 6 == 3
    for buf in (put(*deep_case(300))[0], put(*far_case(4097, 3))[0], put(*lazy_case(15, 21))[0], put(*nice_case(16, 16))[0]):
        assert zlib.decompress(vm.expected_stream(oracle, oracle.DEFLATE, buf, level), -15) == buf
    zd = MIXED[2000:6000]
    s = vm.expected_dict_stream(oracle, "zlib", zd, data[:5000], level)
    d = zlib.decompressobj(zdict=zd)
    assert d.decompress(s) + d.flush() == data[:5000]


def test_levels_grow_smaller_on_text(oracle):
    data = _text(20000, 21)
    sizes = [len(vm.expected_stream(oracle, oracle.DEFLATE, data, level)) for level in (1, 3, 6, 9)]
    assert sizes[0] > sizes[1] > sizes[2] >= sizes[3], sizes
