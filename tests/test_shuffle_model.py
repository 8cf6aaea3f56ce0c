"""CPU: tests/shuffle_model.py, the numpy restatement of the byte-shuffle filter (include/lfx.h), against a
byte-by-byte loop of the formula, against its own inverse, and — where the machine happens to have them — against numcodecs'
Shuffle and h5py's shuffle filter, which it claims to be."""
import numpy as np
import pytest

import shuffle_model as model

SIZES = (1, 2, 3, 4, 5, 8, 16, 17, 256)


def lengths(s):
    t = model.tile_elems(s)
    return sorted({0, 1, s - 1, s, s + 1, 2 * s - 1, 2 * s, 7 * s + s // 2, (t + 1) * s + s - 1})


@pytest.mark.parametrize("s", SIZES)
def test_model_equals_the_formula(s):
    for n in lengths(s):
        x = model.payload(n, 17 * s + n)
        y = model.shuffle(x, s)
        assert y == model.shuffle_loop(x, s), (s, n)
        assert len(y) == n and model.unshuffle(y, s) == x
        assert sorted(y) == sorted(x)                      # a permutation
        k = n // s
        assert y[k * s:] == x[k * s:]                      # the trailing bytes stay where they are
        if s == 1 or k <= 1:
            assert y == x                                  # the identity cases follow from the formula


def test_planes_are_what_the_filter_is_for():
    x = np.arange(1000, dtype="<u4").tobytes()
    y = model.shuffle(x, 4)
    assert y[2000:] == bytes(2000)                         # the two high bytes of every small number, together
    assert y[:1000] == bytes(i & 255 for i in range(1000))


def test_tile_elems_matches_the_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "libflate_amd", "csrc", "lfx_shuffle.h")).read()
    assert re.search(r"SHUF_TILE_BYTES = 16384;", hdr) and "SHUF_TILE_BYTES / s / 64 * 64" in hdr
    assert model.tile_elems(4) == 4096 and model.tile_elems(3) == 5440 and model.tile_elems(256) == 64 and model.tile_elems(200) == 64


def test_against_numcodecs():
    numcodecs = pytest.importorskip("numcodecs")
    for s in (2, 4, 8, 3):
        x = model.payload(40 * s, s)                       # (numcodecs takes whole elements)
        assert bytes(numcodecs.Shuffle(elementsize=s).encode(np.frombuffer(x, dtype=np.uint8))) == model.shuffle(x, s)


def test_against_h5py(tmp_path):
    h5py = pytest.importorskip("h5py")
    import zlib
    a = np.frombuffer(model.payload(4 * 1000, 5), dtype="<f4")
    with h5py.File(tmp_path / "a.h5", "w") as f:
        d = f.create_dataset("a", data=a, chunks=(1000,), shuffle=True, compression="gzip")
        _mask, chunk = d.id.read_direct_chunk((0,))
    assert zlib.decompress(chunk) == model.shuffle(a.tobytes(), 4)
