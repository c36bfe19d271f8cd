"""bench.py's plain line and --dump-outputs: a plain run prints the headline keys only, the number of timed steps is the one
asked for, and the dumped arrays are what the timed path returned (checked against the CPU oracle, identical from run to
run, up to rounding)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from lambda_lanczos_amd import generators as G
from util import overlap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE, WINDOW = 100, 20


def _bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "c2",
           "--size", str(SIDE), "--window", str(WINDOW), "--dump-outputs", str(out_dir)] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.strip()][-1])


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path, oracle):
    d = _bench(tmp_path / "a")
    assert d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False
    assert d["unit"] == "Lanczos iterations/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - d["config"]["iterations_per_step"]) <= 1e-6 * d["config"]["iterations_per_step"]
    for key in ("cpu_baseline", "roofline", "phases", "other_configs", "value_host_io"):
        assert key not in d, key
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["eigenvalues.npy", "eigenvector.npy", "iteration_counts.npy"], files
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert all(a.dtype == np.float64 for a in got.values())
    n = SIDE * SIDE
    ora = oracle.lanczos(G.laplace2d_np(SIDE), G.start_vector(n, 1), False, max_iteration=WINDOW, offset=-8.0)
    assert abs(got["iteration_counts"][0] - ora["iter_counts"][0]) <= 2
    lam = ora["eigenvalues"][0]
    assert abs(got["eigenvalues"][0] - lam) <= 1e-10 * max(1.0, abs(lam))
    assert got["eigenvector"].shape == (n,) and 1 - overlap(got["eigenvector"], ora["eigenvectors"][0]) <= 1e-8
    # the same arguments give the same inputs, hence the same outputs (up to the SpMV kernel the operator picks by timing)
    _bench(tmp_path / "b")
    for f in files:
        again = np.load(tmp_path / "b" / f)
        assert again.shape == got[f[:-4]].shape and np.max(np.abs(again - got[f[:-4]])) <= 1e-9 * np.max(np.abs(got[f[:-4]])), f
