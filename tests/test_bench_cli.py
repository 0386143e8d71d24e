"""bench.py command line: the result line, --dump-outputs and --full.

Runs the smallest model at a tiny batch so each invocation is a second or
two; the flagship configuration is measured by the benchmark itself.
"""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--model", "mnist_cnn", "--batch-per-gpu", "8"]


def _bench(*extra, cpu=True):
    env = dict(os.environ)
    if cpu:  # pin the CPU fp32 path wherever the suite runs
        env["HIP_VISIBLE_DEVICES"] = env["CUDA_VISIBLE_DEVICES"] = ""
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"),
                        *SMALL, *extra],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def _load(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def _check_dump(d):
    arrays = _load(d)
    assert "loss.npy" in arrays
    for k, a in arrays.items():
        assert k.endswith(".npy")
        assert a.dtype in (np.float32, np.float64), (k, a.dtype)
        assert np.isfinite(a).all(), k
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 1000 * 1000
    return arrays


def test_result_line_and_steps(tmp_path):
    res = _bench("--steps", "3", "--warmup", "1")
    for key in ("metric", "value", "unit", "higher_is_better", "dtype",
                "ms_per_step"):
        assert key in res
    assert res["steps"] == 3 and res["warmup"] == 1
    assert res["ms_per_step"] > 0
    # value is images/sec over exactly the timed steps
    img_s = res["config"]["global_batch"] / (res["ms_per_step"] * 1e-3)
    assert res["value"] == pytest.approx(img_s, rel=1e-2)


def test_dump_outputs_repeatable(tmp_path):
    a_dir, b_dir = str(tmp_path / "a"), str(tmp_path / "b")
    _bench("--steps", "2", "--warmup", "1", "--dump-outputs", a_dir)
    _bench("--steps", "2", "--warmup", "1", "--full", "--dump-outputs", b_dir)
    a, b = _check_dump(a_dir), _check_dump(b_dir)
    assert a.keys() == b.keys()
    for k in a:  # CPU fp32 path is deterministic: identical inputs => bitwise
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    # a different number of steps trains further: the dump tracks the last step
    c_dir = str(tmp_path / "c")
    _bench("--steps", "3", "--warmup", "1", "--dump-outputs", c_dir)
    c = _load(c_dir)
    assert any(not np.array_equal(a[k], c[k]) for k in a)


@pytest.mark.gpu
def test_dump_outputs_graphed_step(tmp_path):
    d = str(tmp_path / "g")
    res = _bench("--steps", "2", "--warmup", "1", "--dump-outputs", d,
                 cpu=False)
    assert res["config"]["graphed_step"] is True
    assert res["dtype"] == "bf16"
    arrays = _check_dump(d)
    assert arrays["loss.npy"].shape == (1,)
