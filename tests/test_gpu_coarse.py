"""The coarse view on the MI355X: the coarse_block kernel through ops.coarse
against the NumPy oracle (every reduction path: lanes holding several cells,
cells across lanes, cells wider than a strip, taller than a chunk, cut by the
block's edge), Solver::coarse on one GPU (graphs on and off, resident tiles,
insulated and periodic edges) and across loopback ranks, and the `heat` CLI."""
import json
import subprocess

import numpy as np
import pytest

from parallel_heat_amd import HeatConfig, HeatSolver, _native, ops
from parallel_heat_amd.models import reference as R
from parallel_heat_amd.parallel.group import run_group
from parallel_heat_amd.utils import io as hio

from . import coarse_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_matches_oracle(gpu, shape):
    # Ghost ring (depth 2) and pitch padding are NaN: one cell read outside
    # the owned block would turn a plane NaN.
    C.check_shape_against_oracle(gpu, shape)


@pytest.mark.parametrize("factors", C.MERGE_FACTORS, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("cut", C.MERGE_GRIDS, ids=lambda c: f"{c[0]}x{c[1]}")
def test_blocks_add_up(gpu, cut, factors):
    C.check_blocks_add_up(gpu, cut, factors)


@pytest.mark.parametrize("name", C.GENERAL_SETS)
def test_general_values_within_fp64_bound(gpu, name):
    C.check_general_values(gpu, name)


def test_nonfinite_cells(gpu):
    C.check_nonfinite(gpu)


@pytest.mark.parametrize("factors", ["2x2", "8x8", "wide"])
def test_every_loop_runs_twice(gpu, factors):
    # A shape from the planner's own constants: with the launch capped at
    # kWaves waves, the plate has more than two strips of strip_cols columns
    # and more than two chunks of max_chunk_rows rows per wave, so the
    # grid-stride loop, the row loop over chunks and the strips of a wave all
    # run at least twice, at cells narrower than a lane's float4 (2x2), cells
    # across lanes (8x8) and cells wider than a strip and taller than a chunk.
    probe = ops.coarse_plan(ops.Field(8, 8, halo=2, device=gpu), 1, 1)
    strip_cols, max_rows, min_rows = (probe["strip_cols"], probe["max_chunk_rows"],
                                      probe["min_chunk_rows"])
    assert (strip_cols, max_rows, min_rows, probe["waves_per_cu"]) == (256, 64, 8, 32)
    kWaves = 4
    nx, ny = 5 * max_rows + 3, 2 * strip_cols + 37
    fx, fy = {"2x2": (2, 2), "8x8": (8, 8),
              "wide": (max_rows + 36, strip_cols + 44)}[factors]
    grid = C.int_grid(nx, ny)
    f = C.field_of(grid, gpu)
    ops.set_coarse_max_waves(kWaves)
    try:
        plan = ops.coarse_plan(f, fx, fy)
        got = ops.coarse(f, fx, fy)
        C.assert_exact(got, grid, fx, fy, (factors, plan))
    finally:
        ops.set_coarse_max_waves(0)
    assert plan["waves"] == kWaves and plan["units"] >= 2 * kWaves, plan
    assert plan["strips"] >= 2 and plan["chunks"] >= 2, plan
    assert plan["vector_rows"] == 1, plan
    if factors == "wide":
        assert plan["owned"] == 0 and plan["cells_per_chunk"] == 0 and plan["pieces"] >= 2, plan
    else:
        assert plan["owned"] == 1 and plan["cells_per_strip"] * fy > strip_cols - 4 - fy, plan
        assert plan["cells_per_chunk"] * fx == plan["chunk_rows"] <= max_rows, plan
    # The default launch (no cap) gives the same planes.
    C.assert_exact(ops.coarse(f, fx, fy), grid, fx, fy, (factors, "default launch"))


@pytest.mark.parametrize("pitch", [263, 264])
def test_unaligned_origin(gpu, pitch):
    # An origin that is not 16-byte aligned.  Pitch 263 (no multiple of 4): rows
    # are read cell by cell; pitch 264: float4 rows whose strips start 1 column
    # before the block.  Same planes.
    import ctypes

    import torch
    nx, ny = 33, 257
    grid = C.int_grid(nx, ny)
    buf = torch.full((nx + 2, pitch), float("nan"), dtype=torch.float32, device=gpu)
    buf[1:nx + 1, 3:3 + ny] = torch.from_numpy(np.array(grid)).to(gpu)
    for fx, fy in [(2, 2), (3, 5), (8, 64), (5, 300)]:
        cr, cc = ops.coarse_dims(nx, ny, fx, fy)
        out = {"sum": torch.zeros((cr, cc), dtype=torch.float64, device=gpu),
               "min": torch.full((cr, cc), float("inf"), dtype=torch.float32, device=gpu),
               "max": torch.full((cr, cc), float("-inf"), dtype=torch.float32, device=gpu)}
        _native.call("heat_op_coarse", ctypes.c_void_p(buf.data_ptr() + 4 * (pitch + 3)), pitch,
                     nx, ny, 0, 0, nx, ny, fx, fy, ctypes.c_void_p(out["sum"].data_ptr()),
                     ctypes.c_void_p(out["min"].data_ptr()),
                     ctypes.c_void_p(out["max"].data_ptr()),
                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        C.assert_exact(out, grid, fx, fy, ("unaligned origin", pitch, fx, fy))


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("edges", C.EDGES, ids=["dirichlet", "insulated", "periodic"])
def test_solver_coarse_and_continuation(gpu, edges, graph):
    C.check_solver("hip", edges, use_graph=graph, device=0)


@pytest.mark.parametrize("edges", C.EDGES, ids=["dirichlet", "insulated", "periodic"])
def test_solver_resident_tiles(gpu, edges):
    r = C.check_solver("hip", edges, shape=(1024, 520), device=0)
    assert r.resident_passes > 0, r


@pytest.mark.parametrize("world,kw", [(2, dict(decomp="rows")), (3, dict(decomp="rows")),
                                      (4, dict(decomp="auto"))], ids=["2", "3", "4"])
def test_loopback_ranks_agree_with_one_rank(gpu, world, kw):
    nx, ny = 150, 300   # test_gpu_loopback's plate, TB passes of depth 8
    fx, fy = C.SOLVER_FACTORS
    grid = C.int_grid(nx, ny)
    cfg = HeatConfig(nx=nx, ny=ny, steps=0, init="zero", backend="hip", tb_depth=8, **kw)

    def fn(s):
        s.scatter(grid if s.rank == 0 else None)
        v0 = s.coarse(fx, fy)
        s.run(C.SOLVER_STEPS)
        return v0, s.coarse(fx, fy), s.gather()

    res = run_group(cfg, world, fn, transport="loopback")
    with HeatSolver(cfg.replace(decomp="auto")) as s:
        one = fn(s)
    C.assert_exact(one[0], grid, fx, fy, "one rank")
    for r, (v0, v1, _) in enumerate(res):
        for k in ("sum", "min", "max"):
            # Scattered integers: bit for bit the one-rank result on every rank.
            assert v0[k].tobytes() == one[0][k].tobytes(), (r, k)
            assert v1[k].tobytes() == res[0][1][k].tobytes(), (r, k)
        for k in ("min", "max"):
            assert np.array_equal(v1[k], one[1][k]), (r, k)
    after = next(g for _, _, g in res if g is not None)
    assert np.array_equal(after, one[2])
    C.assert_within_bound(res[0][1], after, fx, fy, f"{world} loopback ranks")


@pytest.mark.parametrize("mode", [["--backend", "hip"],
                                  ["--backend", "hip", "--gpus", "2", "--transport", "loopback"]],
                         ids=["hip", "gpus2-loopback"])
def test_heat_cli_writes_the_oracles_view(gpu, tmp_path, mode):
    for stat in ("mean", "min", "max"):
        p = subprocess.run([str(_native.CLI_PATH)] + mode +
                           ["--nx", "70", "--ny", "519", "--steps", "24", "--init", "random",
                            "--seed", "5", "--out-format", "bin", "--out", "full.bin", "--coarse",
                            "4x8", "--coarse-out", f"view_{stat}.bin", "--coarse-stat", stat,
                            "--json"], cwd=tmp_path, capture_output=True, text=True, timeout=300,
                           check=True)
        m = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
        assert m["coarse"] == {"fx": 4, "fy": 8, "rows": 18, "cols": 65, "stat": stat,
                               "path": f"view_{stat}.bin"}
        full, _ = hio.read_bin(str(tmp_path / "full.bin"), mmap=False)
        want = R.coarse_np(full, 4, 8)
        g, h = hio.read_bin(str(tmp_path / f"view_{stat}.bin"), mmap=False)
        assert (h["nx"], h["ny"], h["step"]) == (18, 65, 24)
        if stat == "mean":
            m32 = (want["sum"] / want["count"]).astype(np.float32)
            assert np.all(np.abs(g - m32) <= np.spacing(np.abs(m32)))
        else:
            assert np.array_equal(g, want[stat])
