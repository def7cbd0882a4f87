"""-m gpu: bench.py's plain run (the timed steps only) and --dump-outputs: the files hold the factorization of the seeded input that
the last timed step computed, identical from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, *args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--dump-outputs", str(out_dir), *args]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_plain_run_dumps_the_last_step(tmp_path):
    n, steps = 1024, 3
    d = _bench(tmp_path / "a", "--size", str(n), "--steps", str(steps), "--warmup", "1")
    assert d["steps"] == steps and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "GFLOP/s" and d["dtype"] == "f64"
    # nothing but the timed steps: the extras of --full are absent
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["check"] == {} and d["kernel_ms"] == {}

    files = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert set(files) == {"factors_sample", "factors_sample_index", "ipiv", "info"}
    assert all(v.dtype in (np.float32, np.float64) for v in files.values())
    assert sum(v.nbytes for v in files.values()) <= 64 << 20
    # n*n is below the sample size: every entry, column-major order
    assert np.array_equal(files["factors_sample_index"], np.arange(n * n, dtype=np.float64))
    F = files["factors_sample"].reshape(n, n).T
    ipiv = files["ipiv"].astype(np.int64)
    A = O.np_uniform(n, n, 12)   # bench.py's input: the library's generator, seed 12
    _, ipo, infoo = O.lu(A)
    assert files["info"][0] == infoo == 0
    assert np.array_equal(ipiv, ipo)
    assert O.residual(A, F, ipiv)[1] < 1e-12

    e = _bench(tmp_path / "b", "--size", str(n), "--steps", "2", "--warmup", "0")
    assert e["steps"] == 2
    for name, v in files.items():
        assert np.array_equal(np.load(tmp_path / "b" / f"{name}.npy"), v), name
