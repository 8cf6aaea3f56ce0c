"""CPU: the arithmetic of pack by chunk — a block's histogram as the sum of its chunks' rows, a chunk's packed size
from its row and the block's code widths, the chunks' first bits, and which calls take the path (tests/c/chunk_bits.cpp over
lfx_huff.h and lfx_encode_stages.h) — under the host compiler, plain and with AddressSanitizer and UBSan, as a program of its
own.  Without a device nothing runs."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_chunk_bits_under_the_host_compiler(tmp_path, flags):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "chunk_bits")
    subprocess.run([gxx, "-O2", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "c", "chunk_bits.cpp")],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "chunk_bits ok: 186 blocks of 1, 4 and 129 chunks" in out.stdout, (out.stdout[-400:], out.stderr[-400:])
