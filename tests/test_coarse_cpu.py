"""The coarse view (block sum / min / max of the field) without a GPU: the
host twin heat::coarse_block against the NumPy oracle reference.coarse_np,
the CPU backend's Solver::coarse alone and across gloo ranks, both CLIs, the
limit of heat_coarse_dims, and the zero-scratch guardrail of the device
kernels (read from the built library's code objects)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from parallel_heat_amd import _native, ops
from parallel_heat_amd.models import reference as R
from parallel_heat_amd.utils import io as hio

from . import coarse_cases as C
from .coarse_worker import run_world

ROOT = str(_native.REPO_DIR)
HEAT = str(_native.CLI_PATH)
PY = [sys.executable, "-m", "parallel_heat_amd"]


@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_twin_matches_oracle(shape):
    C.check_shape_against_oracle("cpu", shape)


@pytest.mark.parametrize("factors", C.MERGE_FACTORS, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("cut", C.MERGE_GRIDS, ids=lambda c: f"{c[0]}x{c[1]}")
def test_blocks_add_up(cut, factors):
    C.check_blocks_add_up("cpu", cut, factors)


@pytest.mark.parametrize("name", C.GENERAL_SETS)
def test_general_values_within_fp64_bound(name):
    C.check_general_values("cpu", name)


def test_nonfinite_cells():
    C.check_nonfinite("cpu")


def test_oracle_is_independent_of_reduceat_order():
    # The oracle against plain slicing per cell (pad-free), on one odd shape.
    g = C.int_grid(33, 257)
    want = R.coarse_np(g, 7, 3)
    for i in range(want["sum"].shape[0]):
        for j in range(want["sum"].shape[1]):
            c = g[i * 7:(i + 1) * 7, j * 3:(j + 1) * 3]
            assert want["sum"][i, j] == c.astype(np.float64).sum()
            assert want["min"][i, j] == c.min() and want["max"][i, j] == c.max()
            assert want["count"][i, j] == c.size


@pytest.mark.parametrize("edges", C.EDGES, ids=["dirichlet", "insulated", "periodic"])
def test_cpu_solver_coarse_and_continuation(edges):
    C.check_solver("cpu", edges)


@pytest.mark.parametrize("world,kw", [(4, dict(px=2, py=2)), (3, dict(px=3, py=1))],
                         ids=["2x2", "3x1"])
def test_gloo_ranks_agree_with_one_rank(tmp_path, world, kw):
    nx, ny = C.SOLVER_SHAPE
    fx, fy = C.SOLVER_FACTORS
    grid = C.int_grid(nx, ny)
    cfg = dict(nx=nx, ny=ny, steps=0, init="zero", backend="cpu", **kw)
    res = run_world(world, cfg, grid, fx, fy, C.SOLVER_STEPS, tmp_path)
    assert (int(res[0]["px"]), int(res[0]["py"])) == (kw["px"], kw["py"])
    # Scattered integer data, 0 steps: every rank's planes are the one-rank
    # result (the oracle's) bit for bit.
    from parallel_heat_amd import HeatConfig, HeatSolver
    with HeatSolver(HeatConfig(nx=nx, ny=ny, steps=0, init="zero", backend="cpu")) as s:
        s.scatter(grid)
        one = s.coarse(fx, fy)
    C.assert_exact(one, grid, fx, fy, "one rank")
    for r, d in enumerate(res):
        for k in ("sum", "min", "max", "mean", "count"):
            assert np.array_equal(d[k + "0"], one[k], equal_nan=True), (r, k)
        assert d["sum0"].tobytes() == one["sum"].tobytes(), r
    # After 24 steps: identical on every rank, min / max exact, sum within the bound.
    after = res[0]["grid"]
    for r, d in enumerate(res):
        for k in ("sum", "min", "max"):
            assert d[k + "1"].tobytes() == res[0][k + "1"].tobytes(), (r, k)
    C.assert_within_bound({k: res[0][k + "1"] for k in ("sum", "min", "max")}, after, fx, fy,
                          f"{world} ranks, 24 steps")


def _run(cmd, cwd, check=True):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=300, check=check,
                          env=dict(os.environ, PYTHONPATH=ROOT))


CLI_ARGS = ["--backend", "cpu", "--nx", "70", "--ny", "519", "--steps", "24", "--init", "random",
            "--seed", "5", "--coarse", "4x8", "--json"]


@pytest.mark.parametrize("fmt", ["dat", "bin"])
def test_both_clis_write_the_oracles_view(tmp_path, fmt):
    outs = {}
    for name, cmd in (("native", [HEAT]), ("python", PY)):
        d = tmp_path / name
        d.mkdir()
        for stat in ("mean", "min", "max"):
            p = _run(cmd + CLI_ARGS + ["--out-format", fmt, "--out", f"full.{fmt}",
                                       "--coarse-out", f"view_{stat}.{fmt}", "--coarse-stat", stat],
                     d)
            m = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
            assert m["coarse"] == {"fx": 4, "fy": 8, "rows": 18, "cols": 65, "stat": stat,
                                   "path": f"view_{stat}.{fmt}"}
        outs[name] = {f.name: f.read_bytes() for f in sorted(d.iterdir())}
    assert outs["native"].keys() == outs["python"].keys()
    for k, v in outs["native"].items():
        assert v == outs["python"][k], k
    d = tmp_path / "native"
    if fmt == "bin":
        full, h = hio.read_bin(str(d / "full.bin"), mmap=False)
        want = R.coarse_np(full, 4, 8)
        for stat in ("mean", "min", "max"):
            g, hv = hio.read_bin(str(d / f"view_{stat}.bin"), mmap=False)
            assert (hv["nx"], hv["ny"], hv["step"]) == (18, 65, 24) and h["step"] == 24
            if stat == "mean":
                # Rounded once from fp64: the engine's fp64 sum may differ from
                # the oracle's in its last bits, so at most one fp32 ulp here.
                m32 = (want["sum"] / want["count"]).astype(np.float32)
                assert np.all(np.abs(g - m32) <= np.spacing(np.abs(m32)))
            else:
                assert np.array_equal(g, want[stat])
    else:
        # The text holds "%6.1f" values: the view of the run's state, printed.
        from parallel_heat_amd import HeatConfig, HeatSolver
        with HeatSolver(HeatConfig(nx=70, ny=519, steps=24, init="random", seed=5,
                                   backend="cpu")) as s:
            s.run()
            want = R.coarse_np(s.gather(), 4, 8)
        want["mean"] = (want["sum"] / want["count"]).astype(np.float32)
        for stat in ("mean", "min", "max"):
            g = hio.read_dat(str(d / f"view_{stat}.dat"))
            assert g.shape == (18, 65)
            assert np.abs(g - want[stat]).max() <= 0.05 + 1e-4


@pytest.mark.parametrize("cmd", [[HEAT], PY], ids=["native", "python"])
def test_cli_refuses_bad_coarse_flags(tmp_path, cmd):
    base = ["--backend", "cpu", "--nx", "20", "--ny", "20", "--steps", "1"]
    p = _run(cmd + base + ["--coarse", "0x3", "--coarse-out", "v.dat"], tmp_path, check=False)
    assert p.returncode != 0 and "factor must be >= 1" in p.stderr, p.stderr
    p = _run(cmd + base + ["--coarse", "4"], tmp_path, check=False)
    assert p.returncode != 0 and "--coarse-out" in p.stderr and "go together" in p.stderr
    p = _run(cmd + base + ["--coarse-out", "v.dat"], tmp_path, check=False)
    assert p.returncode != 0 and "--coarse FX[xFY]" in p.stderr and "go together" in p.stderr
    p = _run(cmd + ["--backend", "cpu", "--nx", "4096", "--ny", "4096", "--steps", "1",
                    "--coarse", "1x1", "--coarse-out", "v.bin"], tmp_path, check=False)
    assert p.returncode != 0 and "2^22" in p.stderr and "1x1" in p.stderr, p.stderr
    assert not list(tmp_path.glob("v.*"))


def test_coarse_dims_limit():
    assert ops.coarse_dims(2048, 2048, 1, 1) == (2048, 2048)          # 2^22: the limit
    assert ops.coarse_dims(131072, 131072, 64, 64) == (2048, 2048)
    assert ops.coarse_dims(37, 53, 4, 6) == (10, 9)
    with pytest.raises(_native.NativeError, match=r"2\^22.*|limit"):
        ops.coarse_dims(2048, 2049, 1, 1)                              # one above
    with pytest.raises(_native.NativeError, match=r"1x1"):
        ops.coarse_dims(2049, 2048, 1, 1)
    with pytest.raises(_native.NativeError, match=">= 1"):
        ops.coarse_dims(10, 10, 0, 1)
    assert _native.lib().heat_abi_version() == 9 == _native.ABI_VERSION


def test_coarse_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    lib = os.path.join(ROOT, "parallel_heat_amd", "_lib", "libheat.so")
    if not os.path.exists(lib):
        pytest.skip("libheat.so not built")
    from kernel_resources import kernels
    try:
        ks = kernels(lib)
    except (OSError, Exception) as e:  # noqa: BLE001 - toolchain missing
        pytest.skip(f"cannot read code objects: {e}")
    ks = [k for k in ks if re.search(r"coarse", k["name"])]
    # Both reductions of the block kernel, and reset / encode / decode.
    assert len(ks) >= 5, [k["name"] for k in ks]
    bad = [(k["name"], k["scratch"]) for k in ks if k["scratch"] > 0 or k.get("spill", 0) > 0]
    assert not bad, "coarse kernels use scratch: %r" % bad
