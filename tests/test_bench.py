"""GPU (-m gpu): bench.py's plain run -- the result line, and what --dump-outputs writes -- against the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _block_sums(a, block):
    a = a.astype(np.int64)
    w = np.arange(1, block + 1, dtype=np.int64)
    sums = [int(a[q : q + block].sum()) for q in range(0, a.size, block)]
    wsums = [int((a[q : q + block] * w[: a[q : q + block].size]).sum()) for q in range(0, a.size, block)]
    return np.array(sums, dtype=np.float64), np.array(wsums, dtype=np.float64)


@pytest.mark.gpu
def test_plain_run_and_dumped_outputs_match_the_oracle(tmp_path):
    """a plain run prints the headline fields and none of --full's; the dump of its last timed step is the oracle's
    .crs2 of that step's input, and the decoded bytes are the input"""
    import bench
    import datagen as dg
    from oracle import oracle as orc

    steps, mib = 5, 16
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--mib", str(mib),
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["metric"] == "encode+decode GB/s (input bytes)" and d["unit"] == "GB/s" and d["higher_is_better"] is True
    assert d["dtype"] == "u8" and d["steps"] == steps and d["value"] > 0 and d["ms_per_step"] > 0
    assert not d["full"] and not any(k in d for k in ("cpu_baseline", "configs", "roofline", "stage_ms_alone", "single_buffer_ms"))

    files = {f: np.load(out / f) for f in os.listdir(out)}
    assert all(f.endswith(".npy") for f in files) and all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(os.path.getsize(out / f) for f in files) <= 64 << 20

    n = mib << 20
    data = dg.make("uniform", n, offset=((steps - 1) % d["config"]["buffer_sets"]) * n)  # the last step's buffer set
    ref = orc.compress(data)
    code = orc.build_code(orc.histogram(data))
    assert files["code_length.npy"].tolist() == list(code.length)
    assert files["code_codeword.npy"].tolist() == list(code.codeword)
    for name, want in (("compressed", ref), ("decoded", data)):
        assert int(files[name + "_nbytes.npy"][0]) == want.size, name
        assert np.array_equal(files[name + "_head.npy"], want[: bench.DUMP_HEAD].astype(np.float32)), name
        pos = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, want.size, size=min(want.size, bench.DUMP_SAMPLE)))
        assert np.array_equal(files[name + "_sample.npy"], want[pos].astype(np.float32)), name
        s, ws = _block_sums(want, bench.DUMP_BLOCK)
        assert np.array_equal(files[name + "_block_sums.npy"], s) and np.array_equal(files[name + "_block_wsums.npy"], ws), name
