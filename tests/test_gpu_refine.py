"""Starting from a coarse grid on the MI355X: the refine_block kernel through
ops.refine against the NumPy oracle (whole and ragged lanes, aligned and
unaligned origins and pitches, every loop of the kernel more than once, blocks
at their offsets), Solver::refine on one GPU (graphs on and off, TB and naive
kernels, every edge mode, resident tiles) and across loopback ranks, and the
`heat` CLI.  Equality is bitwise throughout."""
import json
import subprocess
import sys

import numpy as np
import pytest

from parallel_heat_amd import HeatConfig, HeatSolver, _native, ops
from parallel_heat_amd.models import reference as R
from parallel_heat_amd.parallel.group import run_group
from parallel_heat_amd.utils import io as hio

from . import refine_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", C.GPU_CASES, ids=C.case_id)
def test_kernel_matches_oracle(gpu, case):
    # Ghost ring (depth 2) and pitch padding are NaN before and must be after.
    C.check_case(gpu, case, halo=2)


class RawField:
    """An lx x ly block at column `off` of row 1 of a NaN buffer of `pitch`
    floats per row: what ops.refine needs of a Field, at any alignment."""

    def __init__(self, lx, ly, pitch, off, device):
        import torch
        self.lx, self.ly, self.pitch, self.off = lx, ly, pitch, off
        self.data = torch.full((lx + 2, pitch), float("nan"), dtype=torch.float32, device=device)
        self.device = self.data.device

    def ptr(self):
        return self.data.data_ptr() + 4 * (self.pitch + self.off)

    def owned(self):
        return self.data[1:1 + self.lx, self.off:self.off + self.ly]

    def assert_frame_intact(self, what):
        import torch
        d = self.data.clone()
        d[1:1 + self.lx, self.off:self.off + self.ly] = float("nan")
        assert bool(torch.isnan(d).all()), (what, "a cell outside the block was written")


@pytest.mark.parametrize("pitch,off", [(527, 1), (528, 1), (528, 2), (528, 3)],
                         ids=lambda v: str(v))
@pytest.mark.parametrize("ly", [516, 517, 518, 519])
def test_unaligned_origin_and_ragged_last_lane(gpu, ly, pitch, off):
    # Ghost depth 1: the origin sits `off` floats past a 16-byte boundary.  Pitch
    # 527 (no multiple of 4): every lane stores dword by dword; pitch 528:
    # float4 rows whose first lane starts before the block.  Widths 516..519
    # leave the last lane 4, 1, 2 and 3 of its cells (with the origin's shift).
    case = (21, ly, 4, 3)
    nx, _, fx, fy = case
    S = C.source("signed", *C.dims(case))
    for order in C.ORDERS:
        for wrap in ("", "xy"):
            f = RawField(nx, ly, pitch, off, gpu)
            plan = ops.refine_plan(f)
            assert plan["vector_rows"] == int(pitch % 4 == 0), plan
            assert plan["align"] == (off if pitch % 4 == 0 else 0), plan
            ops.refine(f, S, fx, fy, order=order, wrap=wrap)
            what = (ly, pitch, off, order, wrap)
            C.assert_bitwise(f.owned().cpu().numpy(), C.expected("signed", case, order, wrap), what)
            f.assert_frame_intact(what)


@pytest.mark.parametrize("order", C.ORDERS)
def test_every_loop_runs_twice(gpu, order):
    # A shape from the planner's own constants: with the launch capped at
    # kWaves waves the plate has three strips and six chunks of max_chunk_rows
    # rows, so the grid-stride loop, the row loop of a chunk and the strips of
    # a wave all run at least twice.
    probe = ops.refine_plan(ops.Field(8, 8, halo=2, device=gpu))
    strip_cols, max_rows, min_rows = (probe["strip_cols"], probe["max_chunk_rows"],
                                      probe["min_chunk_rows"])
    assert (strip_cols, max_rows, min_rows, probe["waves_per_cu"]) == (256, 64, 8, 32)
    kWaves = 4
    case = (5 * max_rows + 3, 2 * strip_cols + 37, 8, 16)
    nx, ny, fx, fy = case
    S = C.source("signed", *C.dims(case))
    f = C.nan_field(nx, ny, gpu)
    ops.set_refine_max_waves(kWaves)
    try:
        plan = ops.refine_plan(f)
        ops.refine(f, S, fx, fy, order=order, wrap="x")
    finally:
        ops.set_refine_max_waves(0)
    C.assert_bitwise(f.owned().cpu().numpy(), C.expected("signed", case, order, "x"), plan)
    C.assert_frame_intact(f, plan)
    assert plan["waves"] == kWaves and plan["units"] >= 2 * kWaves, plan          # grid stride
    assert plan["strips"] >= 2 and plan["chunks"] >= 2, plan                      # strips of a wave
    assert plan["strips"] % kWaves != 0, plan          # so a wave meets more than one strip
    assert 2 <= plan["chunk_rows"] <= max_rows and nx >= 2 * plan["chunk_rows"], plan  # row loop
    assert plan["vector_rows"] == 1 and plan["align"] == 0, plan
    # The default launch (no cap) gives the same plate.
    g = C.nan_field(nx, ny, gpu)
    ops.refine(g, S, fx, fy, order=order, wrap="x")
    C.assert_bitwise(g.owned().cpu().numpy(), C.expected("signed", case, order, "x"), "default")
    assert ops.refine_plan(g)["waves"] > kWaves


@pytest.mark.parametrize("cut", C.BLOCK_CUTS, ids=lambda c: f"{c[0]}x{c[1]}")
def test_blocks_make_the_plate(gpu, cut):
    C.check_blocks(gpu, cut)


def test_special_values(gpu):
    # Order 0 copies NaN payloads and infinities bit for bit; under order 1 a
    # NaN source cell makes NaN exactly its footprint.
    case = (37, 53, 4, 8)
    nx, ny, fx, fy = case
    S = np.array(C.source("signed", *C.dims(case)))
    u = S.view(np.uint32)
    u[0, 0], u[3, 2], u[9, 6] = 0x7FC12345, 0xFFA00001, 0x7F800001
    S[1, 1], S[2, 5] = np.inf, -np.inf
    f = C.nan_field(nx, ny, gpu)
    ops.refine(f, S, fx, fy, order=0)
    C.assert_bitwise(f.owned().cpu().numpy(),
                     S[np.arange(nx)[:, None] // fx, np.arange(ny)[None, :] // fy], "order 0")
    for wrap in C.WRAPS:
        for spot in [(0, 0), (4, 3), (9, 6)]:
            S = np.array(C.source("int", *C.dims(case)))
            S[spot] = np.nan
            want = C.nan_footprint(case, wrap, spot)
            f = C.nan_field(nx, ny, gpu)
            ops.refine(f, S, fx, fy, order=1, wrap=wrap)
            g = f.owned().cpu().numpy()
            assert np.array_equal(np.isnan(g), want), (spot, wrap)
            clean = C.expected("int", case, 1, wrap)
            assert np.array_equal(C.bits(g)[~want], C.bits(clean)[~want]), (spot, wrap)


@pytest.mark.parametrize("kernel", ["tb", "naive"])
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("edges", C.EDGES, ids=C.EDGE_IDS)
def test_solver_refine_then_steps(gpu, edges, graph, kernel):
    # tb: ghost depth of the pass; naive: ghost depth 1.
    C.check_solver("hip", edges, use_graph=graph, kernel=kernel, device=0)
    # The CPU backend gives the same plate (it is held to the oracle without a GPU).
    nx, ny, fx, fy = C.SOLVER_CASE
    S = C.source("signed", *C.dims(C.SOLVER_CASE))
    out = []
    for backend, kw in (("hip", dict(use_graph=graph, kernel=kernel, device=0)), ("cpu", {})):
        with HeatSolver(HeatConfig(nx=nx, ny=ny, steps=0, backend=backend, **edges, **kw)) as s:
            s.refine(S, order=0)
            s.run(25)
            out.append(s.gather())
    C.assert_bitwise(out[0], out[1], (edges, graph, kernel, "hip vs cpu"))


@pytest.mark.parametrize("edges", C.EDGES, ids=C.EDGE_IDS)
def test_solver_resident_tiles(gpu, edges):
    nx, ny, fx, fy = 1024, 520, 16, 8
    S = C.source("signed", 64, 65)
    out = []
    for backend, kw in (("hip", dict(device=0)), ("cpu", {})):
        with HeatSolver(HeatConfig(nx=nx, ny=ny, steps=0, backend=backend, **edges, **kw)) as s:
            s.run(24)                       # graphs captured before the refine
            s.refine(S, fx, fy)
            first = s.gather()
            r = s.run(24)
            out.append((first, s.gather()))
            if backend == "hip":
                assert r.resident_passes > 0, r
    periodic = edges.get("periodic", "")
    C.assert_bitwise(out[0][0], R.refine_np(S, nx, ny, fx, fy, 1, periodic), "refined")
    C.assert_bitwise(out[0][0], out[1][0], "refined, hip vs cpu")
    C.assert_bitwise(out[0][1], out[1][1], "24 steps, hip vs cpu")


@pytest.mark.parametrize("world,kw", [(2, dict(px=2, py=1)), (4, dict(px=2, py=2))],
                         ids=["2x1", "2x2"])
@pytest.mark.parametrize("edges", [dict(), dict(periodic="xy")], ids=["dirichlet", "periodic"])
def test_loopback_ranks_fill_their_own_blocks(gpu, edges, world, kw):
    case = (150, 300, 8, 16)   # test_gpu_loopback's plate, TB passes of depth 8
    nx, ny, fx, fy = case
    S = C.source("signed", *C.dims(case))
    cfg = HeatConfig(nx=nx, ny=ny, steps=0, init="zero", backend="hip", tb_depth=8, **edges, **kw)

    def fn(s):
        s.refine(S, fx, fy)
        g0 = s.gather()
        s.run(25)
        return g0, s.gather(), (s.info.px, s.info.py)

    res = run_group(cfg, world, fn, transport="loopback")
    assert res[0][2] == (kw["px"], kw["py"])
    lv = C.solver_levels(case, 1, "", edges.get("periodic", ""))
    C.assert_bitwise(res[0][0], lv[0], (world, "refined"))
    C.assert_bitwise(res[0][1], lv[25], (world, "25 steps"))


def test_heat_cli_agrees_with_the_python_cli(gpu, tmp_path):
    run = dict(cwd=tmp_path, capture_output=True, text=True, timeout=300, check=True)
    heat = str(_native.CLI_PATH)
    plate = ["--nx", "70", "--ny", "519"]
    subprocess.run([heat, "--backend", "hip"] + plate +
                   ["--steps", "24", "--init", "random", "--seed", "5", "--out", "none",
                    "--out-format", "bin", "--coarse", "4x8", "--coarse-out", "v.bin"], **run)
    common = plate + ["--steps", "5", "--init-from", "v.bin", "--out-format", "bin", "--json"]
    outs = []
    for cmd in ([heat, "--backend", "hip"],
                [heat, "--backend", "hip", "--gpus", "2", "--transport", "loopback"],
                [sys.executable, "-m", "parallel_heat_amd", "--backend", "cpu"]):
        import os
        p = subprocess.run(cmd + common + ["--out", f"final{len(outs)}.bin"],
                           env=dict(os.environ, PYTHONPATH=str(_native.REPO_DIR)), **run)
        m = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
        assert m["init_from"] == {"path": "v.bin", "rows": 18, "cols": 65, "fx": 4, "fy": 8,
                                  "order": 1}
        outs.append((tmp_path / f"final{len(outs)}.bin").read_bytes())
    assert outs[0] == outs[2] and outs[1] == outs[2]
    S, _ = hio.read_bin(str(tmp_path / "v.bin"), mmap=False)
    g = R.refine_np(S, 70, 519, 4, 8, 1)
    for _ in range(5):
        g = R.step_np_fma(g)
    last, h = hio.read_bin(str(tmp_path / "final0.bin"), mmap=False)
    assert h["step"] == 5
    C.assert_bitwise(last, g, "heat --init-from, 5 steps")
