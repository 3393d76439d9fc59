"""bench.py's command line on the GPU (the tiny config): a plain run times its steps and leaves
out what takes runs of its own, --full adds those, and --dump-outputs writes the same arrays in
both (the same inputs with the same arguments, captured before any further step)."""

from __future__ import annotations

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
TINY = ["--gpus", "1", "--config", "tiny", "--steps", "3", "--warmup", "1"]


def _bench(dump: Path, *extra: str) -> tuple[dict, Path]:
    cmd = [sys.executable, str(ROOT / "bench.py"), *TINY, "--dump-outputs", str(dump), *extra]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    line = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(line) == 1
    return json.loads(line[0]), dump


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _bench(tmp_path_factory.mktemp("plain"))


@pytest.fixture(scope="module")
def full(tmp_path_factory):
    return _bench(tmp_path_factory.mktemp("full"), "--full", "--cpu-steps", "2", "--cpu-warmup", "1")


def test_plain_run_times_the_steps_only(plain):
    out, _ = plain
    assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["value"] > 0 and out["ms_per_step"] > 0 and out["higher_is_better"] is True
    assert out["unit"] == "interactions/s" and out["dtype"] == "fp32"
    # interactions/s and ms_per_step describe the same timed region (B = 1024; both rounded)
    assert out["value"] == pytest.approx(1024 / (out["ms_per_step"] * 1e-3), rel=1e-3)
    assert out["cpu_baseline"] is None and "exact_table_math" not in out


def test_full_run_adds_the_sub_lines(full):
    out, _ = full
    assert out["value"] > 0 and out["steps"] == 3
    assert out["exact_table_math"]["value"] > 0 and out["exact_table_math"]["steps"] == 3
    assert out["cpu_baseline"]["value"] > 0, out["cpu_baseline"]


def test_dumped_outputs_are_the_same_from_run_to_run(plain, full):
    a, b = plain[1], full[1]
    names = sorted(p.name for p in a.glob("*.npy"))
    assert names == sorted(p.name for p in b.glob("*.npy"))
    # the tiny config has a table written whole (2,000 users) and one sampled by rows (20,000 items)
    assert {"losses.npy", "user_encoder.embedding.weight.npy", "item_encoder.embedding.weight.rows_sampled.npy",
            "item_encoder.embedding.weight.rows_last_batch.npy"} <= set(names)
    total = 0
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all(), n
        assert x.shape == y.shape, n
        total += x.nbytes
        if n.startswith("batch_"):  # the inputs: identical
            assert np.array_equal(x, y), n
        else:  # the project's fp32 tolerance (sums by atomics may differ in order between runs)
            scale = float(np.abs(x).max())
            assert float(np.abs(x.astype(np.float64) - y).max()) <= 1e-5 * scale, n
    assert total <= 64 << 20
    assert np.load(a / "losses.npy").shape == (5,)
    assert np.load(a / "item_encoder.embedding.weight.rows_sampled.npy").shape == (4096, 96)
