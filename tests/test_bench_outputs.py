"""bench.py's output dump (--dump-outputs) and the plain / --full split of a
run: the dumped field is the timed path's final state (bitwise the CPU
oracle's), larger fields are sampled by a fixed row subset, a plain run skips
the verification and --full runs it."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from parallel_heat_amd import HeatConfig, HeatSolver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("heat_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Field:
    def __init__(self, grid):
        self.grid = grid

    def gather(self):
        return self.grid


def test_dump_small_field_is_written_whole(tmp_path):
    bench = _bench_module()
    g = np.arange(37 * 53, dtype=np.float32).reshape(37, 53)
    bench.dump_outputs(_Field(g), str(tmp_path / "d"), 0)
    assert sorted(os.listdir(tmp_path / "d")) == ["grid.npy"]
    out = np.load(tmp_path / "d" / "grid.npy")
    assert out.dtype == np.float32 and np.array_equal(out, g)


def test_dump_large_field_is_a_fixed_row_sample(tmp_path):
    bench = _bench_module()
    nx, ny = 2048, 8192  # 64 MiB of float32: above the 48 MB a dump may hold
    g = np.random.default_rng(5).random((nx, ny), dtype=np.float32)
    for d in ("a", "b"):
        bench.dump_outputs(_Field(g), str(tmp_path / d), 0)
    rows = np.load(tmp_path / "a" / "grid_rows.npy")
    out = np.load(tmp_path / "a" / "grid.npy")
    assert rows.dtype == np.float64 and out.dtype == np.float32
    assert len(rows) == bench.DUMP_BYTES // (ny * 4) == 1464
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < nx
    assert np.array_equal(out, g[rows.astype(np.int64)])
    assert out.nbytes + rows.nbytes <= 64 * 10**6
    assert np.array_equal(rows, np.load(tmp_path / "b" / "grid_rows.npy"))
    assert np.array_equal(out, np.load(tmp_path / "b" / "grid.npy"))


def test_dump_other_ranks_write_nothing(tmp_path):
    bench = _bench_module()
    bench.dump_outputs(_Field(None), str(tmp_path / "d"), 1)
    assert not (tmp_path / "d").exists()


def _bench(*args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--nx", "150",
                        "--ny", "333", "--iters-per-step", "15", "--steps", "3", "--warmup", "2",
                        *args], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.splitlines()
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_final_field(gpu, tmp_path):
    d = _bench("--dump-outputs", str(tmp_path / "out"))
    assert d["verified"] is None and "verification" not in d
    assert d["steps"] == 3 and d["warmup"] == 2 and d["ms_per_step"] > 0
    assert d["unit"] == "Mcells/s" and d["higher_is_better"] is True and d["dtype"] == "fp32"
    # value and ms_per_step are the same measurement (3 steps of 15
    # iterations), up to the 4 decimals ms_per_step is printed with.
    assert d["value"] == pytest.approx(150 * 333 * 15 / (d["ms_per_step"] * 1e-3) / 1e6,
                                       rel=1e-4 / d["ms_per_step"] + 1e-6)
    assert sorted(os.listdir(tmp_path / "out")) == ["grid.npy"]
    got = np.load(tmp_path / "out" / "grid.npy")
    cfg = HeatConfig(nx=150, ny=333, steps=(2 + 3) * 15, init="random", seed=1234, backend="cpu")
    with HeatSolver(cfg) as cpu:
        cpu.run()
        want = cpu.gather()
    assert got.dtype == np.float32 and np.array_equal(got, want)


@pytest.mark.gpu
def test_bench_full_run_verifies(gpu):
    d = _bench("--full")
    assert d["verified"] is True
    assert d["verification"]["steps"] == (2 + 3) * 15
    assert d["verification"]["hash"] == d["verification"]["reference_hash"]
