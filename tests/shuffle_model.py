"""The byte-shuffle filter's definition in numpy (include/lfx.h "the byte-shuffle filter"): HDF5's
H5Z_FILTER_SHUFFLE, numcodecs' Shuffle.  For n bytes and element size s: k = n // s, r = n % s;
shuffle: out[j*k + i] = in[i*s + j]; the r trailing bytes are copied; unshuffle is the inverse."""
import numpy as np


def shuffle(data, s):
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    k = len(a) // s
    return a[:k * s].reshape(k, s).T.tobytes() + a[k * s:].tobytes()


def unshuffle(data, s):
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    k = len(a) // s
    return a[:k * s].reshape(s, k).T.tobytes() + a[k * s:].tobytes()


def shuffle_loop(data, s):
    """the formula, byte by byte"""
    data = bytes(data)
    n = len(data)
    k, out = n // s, bytearray(n)
    for i in range(k):
        for j in range(s):
            out[j * k + i] = data[i * s + j]
    out[k * s:] = data[k * s:]
    return bytes(out)


def tile_elems(s):
    """the elements one workgroup takes (libflate_amd/csrc/lfx_shuffle.h: shuf_tile_elems)"""
    if s in (2, 4, 8, 16):
        return 16384 // s
    return max(64, 16384 // s // 64 * 64)


def payload(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()
