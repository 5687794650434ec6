"""bench.py at one GPU, small job: a plain run prints the headline line only, and --dump-outputs writes the same
(dist, idx) sample from run to run (seeded inputs, deterministic path)."""

from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--rows", "1000000", "--refs", "20000", *extra]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_bench_run_and_output_dump(tmp_path):
    runs = [_bench("--dump-outputs", str(tmp_path / name)) for name in ("a", "b")]
    for res in runs:
        assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0
        assert res["unit"] == "Mqueries/s" and res["higher_is_better"] is True and res["value"] > 0
        assert res["roofline"]["timed_calls"] == 3 and 0 < res["roofline"]["frac"] <= 1.0
        for moved in ("cpu_baseline", "parity_vs_cpu_reference", "configs", "laws", "host_to_host_Mq_s"):
            assert moved not in res
    n = (48 << 20) // (16 * 5)  # the sample the dump takes of 1M rows x k = 5
    d_a, i_a = np.load(tmp_path / "a" / "dist.npy"), np.load(tmp_path / "a" / "idx.npy")
    assert d_a.shape == i_a.shape == (n, 5) and d_a.dtype == i_a.dtype == np.float64
    assert (i_a == np.round(i_a)).all() and i_a.min() >= 0 and i_a.max() < 20_000
    assert np.isfinite(d_a).all() and (d_a >= 0).all()
    np.testing.assert_array_equal(np.load(tmp_path / "b" / "dist.npy"), d_a)
    np.testing.assert_array_equal(np.load(tmp_path / "b" / "idx.npy"), i_a)
