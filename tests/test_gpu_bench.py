"""bench.py as it is run for every change: a plain run prints the one result line and does nothing that needs runs of
its own; --dump-outputs writes what the last timed step returned, which must equal the oracle's sort of that step's
input; --full adds the verification of every timed step and the roofline of one profiled sort."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def run_bench(*args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-3000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step_u32(tmp_path):
    logn, K, W = 20, 3, 2
    d = run_bench("--logn", str(logn), "--steps", str(K), "--warmup", str(W), "--dump-outputs", str(tmp_path))
    assert all(f in d for f in CONTRACT) and d["steps"] == K and d["ms_per_step"] > 0
    assert d["unit"] == "Gkeys/s" and d["dtype"] == "u32" and d["higher_is_better"] is True
    assert d["roofline"] is None and d["cpu_baseline"] is None and "other_configs" not in d and d["config"]["verified"] is None
    n = 1 << logn
    last = W + K - 1
    want = O.sort_u32(O.gen_uniform_u32(n, seed=0x5EED0001 + 1000003 * last))
    assert sorted(os.listdir(tmp_path)) == ["keys.npy", "sample_index.npy"]
    idx = np.load(tmp_path / "sample_index.npy")
    keys = np.load(tmp_path / "keys.npy")
    assert keys.dtype == np.float64 and idx.tolist() == list(range(n))     # 2^20 keys: the whole output
    assert (keys == want.astype(np.float64)).all()


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step_pairs(tmp_path):
    logn, K, W = 21, 2, 1
    run_bench("--config", "c5a", "--logn", str(logn), "--steps", str(K), "--warmup", str(W), "--dump-outputs", str(tmp_path))
    n = 1 << logn
    want = O.sort_u64(O.gen_uniform_u64(n, seed=0x5EED0005 + 1000003 * (W + K - 1)))
    idx = np.load(tmp_path / "sample_index.npy").astype(np.int64)
    assert idx[0] == 0 and idx[-1] == n - 1 and (np.diff(idx) > 0).all() and idx.size <= 1 << 20
    total = idx.nbytes
    for name in ("keys", "rids"):                                   # rid = key
        hi, lo = np.load(tmp_path / f"{name}_hi32.npy"), np.load(tmp_path / f"{name}_lo32.npy")
        assert hi.dtype == lo.dtype == np.float64
        total += hi.nbytes + lo.nbytes
        got = (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)
        assert (got == want[idx]).all()
    assert total <= 64 << 20


@pytest.mark.gpu
def test_full_run_verifies_and_profiles():
    d = run_bench("--logn", "20", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline")
    assert all(f in d for f in CONTRACT) and d["steps"] == 2
    assert d["config"]["verified"] is True and d["config"]["steps_verified"] == 2
    assert d["roofline"] is not None and d["roofline"]["achieved"] > 0
    assert d["whole_sort"]["device_copy_GBps_same_run"] > 0


def test_options(monkeypatch):
    """The options every run relies on: --full and --dump-outputs are off unless asked for; --steps sets the step count."""
    monkeypatch.syspath_prepend(ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 3)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "out"
