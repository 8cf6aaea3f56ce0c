"""CPU: the host arithmetic of the byte-shuffle filter (libflate_amd/csrc/lfx_shuffle.h) by
tests/c/shuffle_geom.cpp — a program of its own, built plain and once more with AddressSanitizer and UBSan (nothing loaded
into Python runs under a sanitizer): the tile list covers every element of every record exactly once, for every element size."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_tile_list_and_range_check(sanitize, tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "shuffle_geom")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "c", "shuffle_geom.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "shuffle geom ok" in out.stdout, (out.stdout[-400:], out.stderr[-2000:])
