"""HeatConfig(cx=0.05, cy=0.2) through the GPU solver, against the independent
exact oracle (`reference.step_np_fma` / `run_np(numerics="fma")`): the
plumbing HeatConfig -> capi -> Solver -> StencilGeom on every kernel, graphs,
resident tiles, device-judged convergence, multi-rank loopback groups, the
`heat --gpus` CLI and the checkpoint header.  The product library only (no
experiment kernels).  Needs an MI355X."""
import json
import subprocess

import numpy as np
import pytest

from parallel_heat_amd import HeatConfig, HeatSolver, _native, ops
from parallel_heat_amd.models import reference as R
from parallel_heat_amd.parallel.group import run_group
from parallel_heat_amd.utils import io as hio

from . import oracle_cases as O
from .oracle_cases import assert_bitwise

pytestmark = pytest.mark.gpu

CX, CY = O.ANISO
F = np.float32


def _run(cfg, steps=None):
    with HeatSolver(cfg) as s:
        r = s.run(steps)
        return s.gather(), r


@pytest.mark.parametrize("kernel,depth", [("tb", 8), ("tb", 5), ("lds", 4), ("naive", 3)])
@pytest.mark.parametrize("graph", [True, False])
def test_solver_anisotropic_bitwise(gpu, kernel, depth, graph):
    cfg = HeatConfig(nx=150, ny=333, steps=45, cx=CX, cy=CY, init="random", seed=9,
                     backend="hip", kernel=kernel, tb_depth=depth, use_graph=graph)
    g, r = _run(cfg)
    assert r.steps_done == 45
    assert_bitwise(g, O.levels_of_init(150, 333, CX, CY, 45, "random", 9)[45])


def test_solver_mfma_anisotropic_within_bound(gpu):
    steps = 45
    cfg = HeatConfig(nx=150, ny=333, steps=steps, cx=CX, cy=CY, init="random", seed=9,
                     backend="hip", kernel="mfma", tb_depth=4)
    g, _ = _run(cfg)
    ref = O.levels_of_init(150, 333, CX, CY, steps, "random", 9)[steps]
    dev = float(np.abs(g.astype(np.float64) - ref.astype(np.float64)).max())
    print(f"mfma solver, {steps} steps: max |got - oracle| = {dev:.3e} (bound {steps * 2e-5:.1e})")
    # One mfma step is within 2e-5 of the oracle's on [0, 100) data
    # (test_mfma_step_close_to_oracle).  The exact step is a convex
    # combination of five cells (1 - 2cx - 2cy = 0.5 >= 0): it keeps the data
    # in [0, 100) and does not amplify an error in max norm, so the errors of
    # n steps add up to at most n * 2e-5.  (Swapped coefficients: ~10.)
    assert dev <= steps * 2e-5
    for sl in (np.s_[0, :], np.s_[-1, :], np.s_[:, 0], np.s_[:, -1]):
        assert_bitwise(g[sl], ref[sl], "ring")


@pytest.fixture
def res_shape():
    """Force the resident planner's tile shape (rows per wave, waves)."""
    saved = ops.tb_tuning()

    def set_(rows, waves):
        t = ops.tb_tuning()
        t.tile_rows, t.tile_waves = rows, waves
        ops.set_tb_tuning(t)
    try:
        yield set_
    finally:
        ops.set_tb_tuning(saved)


@pytest.mark.parametrize("shape", [(12, 16), (20, 16)])
def test_resident_anisotropic_bitwise(gpu, monkeypatch, res_shape, shape):
    # Resident tiles (tb_resident_kern.hpp over tb_tile_core.hpp): 12-row
    # waves take the packed update, 20-row waves the scalar one.
    res_shape(*shape)
    monkeypatch.setenv("HEAT_TB_RESIDENT", "1")
    cfg = HeatConfig(nx=203, ny=517, steps=97, cx=CX, cy=CY, init="random", seed=11,
                     backend="hip")
    g, r = _run(cfg)
    assert r.resident_passes > 0, r
    assert_bitwise(g, O.levels_of_init(203, 517, CX, CY, 97, "random", 11)[97])


def test_gpu_convergence_predicted_exactly(gpu):
    kw = dict(nx=24, ny=30, steps=20000, converge=True, check_interval=20, eps=1e-3)
    g, r = _run(HeatConfig(**kw, cx=CX, cy=CY, init="ref-wrap", backend="hip"))
    ref, done, conv_at = R.run_np(**kw, cx=CX, cy=CY, numerics="fma")
    assert conv_at > 0 and r.converged
    assert (r.steps_done, r.converged_at) == (done, conv_at)
    assert_bitwise(g, ref)


def test_gated_replay_inside_depth12_pass(gpu):
    # Checks every 20 steps at depth 12: most fall inside a pass, the
    # converging one is replayed up to its level
    # (test_gated_convergence_bitwise's plate).
    kw = dict(nx=26, ny=37, steps=40000, converge=True, check_interval=20, eps=1e-3)
    g, r = _run(HeatConfig(**kw, cx=CX, cy=CY, init="ref-wrap", backend="hip", tb_depth=12))
    ref, done, conv_at = R.run_np(**kw, cx=CX, cy=CY, numerics="fma")
    assert conv_at > 0 and conv_at % 12 != 0, conv_at   # the check is not at a pass end
    assert r.converged and (r.steps_done, r.converged_at) == (done, conv_at)
    assert r.checks == conv_at // 20
    assert_bitwise(g, ref)


@pytest.mark.parametrize("world,kw", [(2, dict(decomp="rows")), (2, dict(px=1, py=2)),
                                      (4, dict(decomp="auto"))])
def test_loopback_anisotropic_bitwise(gpu, world, kw):
    # Row split, column split, 2 x 2: a decomposition that confuses the axes
    # or a rank with default coefficients shows against the one-plate oracle.
    cfg = HeatConfig(nx=150, ny=300, steps=0, cx=CX, cy=CY, init="random", seed=2,
                     backend="hip", tb_depth=8, **kw)

    def fn(s):
        s.run(45)
        return s.gather()

    got = next(g for g in run_group(cfg, world, fn) if g is not None)
    assert_bitwise(got, O.levels_of_init(150, 300, CX, CY, 45, "random", 2)[45])


def test_cli_gpus_anisotropic(gpu, tmp_path):
    p = subprocess.run([str(_native.CLI_PATH), "--backend", "hip", "--gpus", "2", "--nx", "130",
                        "--ny", "90", "--steps", "37", "--init", "random", "--seed", "6",
                        "--cx", str(CX), "--cy", str(CY), "--out", "g.bin", "--out-format", "bin",
                        "--json"], cwd=tmp_path, capture_output=True, text=True, timeout=300,
                       check=True)
    assert json.loads(p.stdout.splitlines()[-1])["ranks"] == 2
    g, h = hio.read_bin(str(tmp_path / "g.bin"))
    assert h["step"] == 37 and (F(h["cx"]), F(h["cy"])) == (F(CX), F(CY))
    assert_bitwise(np.asarray(g), O.levels_of_init(130, 90, CX, CY, 37, "random", 6)[37])


def test_gpu_checkpoint_round_trip_anisotropic(gpu, tmp_path, capfd):
    cfg = HeatConfig(nx=100, ny=120, steps=60, cx=CX, cy=CY, init="random", seed=3,
                     backend="hip")
    lv = O.levels_of_init(100, 120, CX, CY, 60, "random", 3)
    with HeatSolver(cfg) as s:
        s.run(25)
        s.save(str(tmp_path / "ck.bin"))
    g25, h = hio.read_bin(str(tmp_path / "ck.bin"))
    assert (F(h["cx"]), F(h["cy"]), h["step"]) == (F(CX), F(CY), 25)
    assert_bitwise(np.asarray(g25), lv[25])
    capfd.readouterr()
    with HeatSolver(cfg) as s:
        s.load(str(tmp_path / "ck.bin"))
        assert s.step == 25
        s.run(35)
        g = s.gather()
    assert "warning" not in capfd.readouterr().err
    assert_bitwise(g, lv[60])
