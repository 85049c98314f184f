"""bench.py: a plain run prints the headline line only; --full adds the rest; --dump-outputs writes what the last timed
step computed (the whole output, or a fixed seeded sample of a large one)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _size(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_outputs_small_outputs_whole(tmp_path):
    bm = torch.arange(8 * 40, dtype=torch.int32).to(torch.uint8).reshape(8, 40)[:, :37]  # rows with padding cut off
    hits = torch.tensor([7, 1 << 40], dtype=torch.int64)
    bench.dump_outputs(str(tmp_path), [("bitmap", bm), ("hits", hits)])
    assert sorted(os.listdir(tmp_path)) == ["bitmap.npy", "hits.npy"]
    a, h = np.load(tmp_path / "bitmap.npy"), np.load(tmp_path / "hits.npy")
    assert a.dtype == np.float32 and a.shape == (8, 37) and np.array_equal(a, bm.numpy())
    assert h.dtype == np.float64 and h.tolist() == [7, 1 << 40]


def test_dump_outputs_large_output_fixed_sample(tmp_path):
    n = 3 * bench.DUMP_MAX_VALUES + 5
    g = torch.Generator().manual_seed(3)
    out = torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), [("bitmap", out)], prefix="rank0_")
    for f in ("rank0_bitmap.npy", "rank0_bitmap_index.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f  # same positions every run
    vals, idx = np.load(tmp_path / "a" / "rank0_bitmap.npy"), np.load(tmp_path / "a" / "rank0_bitmap_index.npy")
    assert vals.dtype == np.float32 and idx.dtype == np.float64 and len(vals) == len(idx) <= bench.DUMP_MAX_VALUES
    pos = idx.astype(np.int64)
    assert np.all(np.diff(pos) > 0) and pos[0] == 0 and pos[-1] == n - 1
    assert np.array_equal(vals, out.numpy()[pos])
    # the budget: two outputs of the largest element type stay under 64 MB
    assert 2 * bench.DUMP_MAX_VALUES * (8 + 8) <= 64 * 2 ** 20 and _size(tmp_path / "a") < 32 * 2 ** 20


def test_options_default_to_a_plain_run(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


def _run(*args, timeout=600):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], cwd=ROOT,
                         capture_output=True, text=True, timeout=timeout)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path, O):
    """BASELINE config 1's column (1e7 x 9 bit, v = i % 5, key 3): the plain line, and the dumped bitmap and hit count
    equal the oracle's"""
    n, c = 10_000_000, 9
    line = _run("--rows", str(n), "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0 and line["unit"] == "values/s"
    assert "cpu_baseline" not in line and line["hits"] == 2_000_000
    assert sorted(os.listdir(tmp_path)) == ["bitmap.npy", "hits.npy"]
    obm, ohits = O.scan_eq(O.pack(O.gen_values("mod", n, c, 5), c), n, c, 3)
    assert np.load(tmp_path / "hits.npy").tolist() == [ohits] == [2_000_000]
    assert np.array_equal(np.load(tmp_path / "bitmap.npy"), obm.astype(np.float32))


@pytest.mark.gpu
def test_full_run_keeps_the_cpu_baseline():
    line = _run("--rows", "10000000", "--steps", "3", "--warmup", "1", "--full", "--cpu-reps", "1")
    assert line["cpu_baseline"]["bitmap_equals_gpu"] and line["cpu_baseline"]["value"] > 0
