"""CPU: the stream encoder's state machine with a preset dictionary (libflate_amd/csrc/lfx_stream_enc.h: no HIP, no context,
DESIGN.md §25) over a stand-in batch backend with kilobyte batches — tests/c/stream_enc_dict.cpp, a program of its own, built by
the host compiler plain and with AddressSanitizer and UBSan.  The header bytes (FDICT, FCHECK, DICTID) for every FLEVEL; exactly
one batch of a stream carries the primed chunk (first write larger than a batch, flush before the first byte, three empty
writes and then data, finish with nothing written, 600 KiB in 8 KiB writes, zlib sync markers), none with stored blocks,
literal-only chunks or an empty dictionary; a batch that is run again still carries it; without a dictionary the call sequence
and the batches are those of an encoder that was never given one; the codes mode writes the FDICT header and primes nothing."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_state_machine_with_a_dictionary_over_a_stand_in_backend(tmp_path, flags):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "stream_enc_dict")
    subprocess.run([gxx, "-O2", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "c", "stream_enc_dict.cpp")],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "stream_enc_dict ok: 37 cases" in out.stdout, (out.stdout[-400:], out.stderr[-400:])
