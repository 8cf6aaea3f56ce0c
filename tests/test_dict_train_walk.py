"""CPU: the host side of lfx_dict_train_device (libflate_amd/csrc/lfx_dict_train.h) by tests/c/dict_train.cpp — a
program of its own, built plain and once more with AddressSanitizer and UBSan (nothing loaded into Python runs under a
sanitizer): the argument checks and the scratch's places, and the kernels' steps walked on the host with the kernels' own
cursor and lane walk, against tests/dict_train_model.py."""
import os
import shutil
import struct
import subprocess

import pytest

import dict_train_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan_ubsan"])
def program(request, tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path_factory.mktemp("dtrain") / "dict_train")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param else ["-O2"]
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "c", "dict_train.cpp")], check=True)
    return exe


def test_checks_and_layout(program):
    out = subprocess.run([program, "self"], capture_output=True, text=True)
    assert out.returncode == 0 and "dict_train self ok" in out.stdout, (out.stdout[-400:], out.stderr[-400:])


def walk(program, tmp_path, case):
    name, buf, offs, lens, size, k = case
    path = str(tmp_path / (name + ".bin"))
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(offs)))
        for o, n in zip(offs, lens):
            f.write(struct.pack("<QQ", o, n))
        f.write(buf)
    out = subprocess.run([program, "walk", path, str(size), str(k)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("dict "), (name, out.stdout[-200:], out.stderr[-2000:])
    return bytes.fromhex(out.stdout.split(" ", 1)[1].strip())


def test_walk_equals_the_model(program, tmp_path):
    for case in cases.cases() + cases.big_cases():
        assert walk(program, tmp_path, case) == cases.expect(case)[0], case[0]
