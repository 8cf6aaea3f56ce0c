"""CPU: the layout of lfx_decode_batch_packed_device — the host walk of its three kernels
(libflate_amd/csrc/lfx_batch_unpack.h) against the rule, by tests/c/batch_unpacked.cpp: a program of its own, built plain and
once more with AddressSanitizer and UBSan (nothing loaded into Python runs under a sanitizer)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan_ubsan"])
def program(request, tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path_factory.mktemp("bunpack") / "batch_unpacked")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param else ["-O2"]
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "c", "batch_unpacked.cpp")],
                   check=True)
    return exe


def test_layout_walk_against_the_rule(program):
    out = subprocess.run([program, "self"], capture_output=True, text=True)
    assert out.returncode == 0 and "batch_unpacked self ok" in out.stdout, (out.stdout[-400:], out.stderr[-400:])
    # every count of the list ran, 262145 with two rounds of the second scan level
    for line in ("count=1 nwg=1 rounds=1 ok", "count=256 nwg=1 rounds=1 ok", "count=257 nwg=2 rounds=1 ok",
                 "count=262145 nwg=1025 rounds=2 ok"):
        assert line in out.stdout, out.stdout
