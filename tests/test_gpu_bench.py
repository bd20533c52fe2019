"""bench.py's plain run on the GPU: one small `--gpus 1 --steps K --warmup W --dump-outputs DIR` run
in a child process (the form every later measurement uses).  The line carries the headline fields
and none of the --full legs, and the dumped outputs of the last timed step are a consistent RS
result: statuses all "corrected", and the written-back codewords are the oracle's encode of the
restored payloads, for the fixed sample of blocks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB = 20000  # more blocks than the dump's sample (2^14), not a multiple of any tile


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path, oracle):
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--blocks", str(NB), "--prewarm-s", "0", "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["metric"] == bench.METRIC and line["unit"] == "GiB/s" and line["higher_is_better"] is True
    assert line["dtype"] == "u8" and line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["ms_per_step"] > 0
    n, k, _ = oracle.rs_sizes(512, 3)
    # value and ms_per_step describe the same timed region (both rounded in the line)
    assert line["value"] == pytest.approx(2 * (n + k) * NB / (line["ms_per_step"] * 1e-3) / 2**30, rel=2e-2)
    for leg in ("roofline", "cpu_baseline", "configs", "cfg1", "standalone", "host_inclusive", "kernels_ms",
                "repeat_ms_per_step"):
        assert leg not in line, leg
    got = {name: np.load(d / f"{name}.npy") for name in ("sample_blocks", "codewords", "payload", "status")}
    assert sorted(os.listdir(d)) == sorted(f"{name}.npy" for name in got)
    assert sum(a.nbytes for a in got.values()) <= 64 * 10**6
    idx = got["sample_blocks"]
    assert idx.dtype == np.float64 and np.array_equal(idx, bench.dump_sample(NB))
    m = len(idx)
    assert m == bench.DUMP_SAMPLE_BLOCKS
    for name, shape in (("codewords", (m, n)), ("payload", (m, k)), ("status", (NB,))):
        assert got[name].dtype == np.float32 and got[name].shape == shape, name
    assert np.all(got["status"] == 1)  # one injected byte error per block, every one corrected
    pay = got["payload"].astype(np.uint8)
    assert np.array_equal(pay, got["payload"])  # whole bytes
    assert len(np.unique(pay)) == 256  # uniform synthetic payloads, not a blank buffer
    assert np.array_equal(got["codewords"], oracle.rs_encode(512, 3, pay.reshape(-1)).reshape(m, n))
