"""GPU: a plain `bench.py` run — the result line's headline keys and nothing measured beside them, and what
--dump-outputs writes (the last timed step's compressed member and decoded bytes)."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    import bench
    import synth
    n = 16 << 20
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--bytes", str(n),
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0
    assert not {"roofline", "cpu_baseline", "other_configs", "phases_ms"} & set(line)
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64 << 20
    enc, dec, lengths = (np.load(out / (f + ".npy")) for f in ("encoded", "decoded", "lengths"))
    assert enc.dtype == dec.dtype == np.float32 and lengths.dtype == np.float64
    assert lengths[0] == line["config"]["compressed_bytes"] and lengths[1] == n
    data = synth.text(n, seed=synth.SEED_BASE + 2)
    assert np.array_equal(dec, data[bench.sample_positions(n, 2)].astype(np.float32))
    assert np.array_equal(enc, enc.astype(np.uint8).astype(np.float32))
    trailer = enc[-8:].astype(np.uint8).tobytes()           # the gzip member's CRC-32 and ISIZE
    assert enc[0] == 0x1f and enc[1] == 0x8b and trailer == zlib.crc32(data.tobytes()).to_bytes(4, "little") + n.to_bytes(4, "little")
