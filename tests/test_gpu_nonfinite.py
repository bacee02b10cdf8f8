"""The convergence decision end to end on the GPU: a residual exactly at the
threshold on the device-judged gate (graph and eager) and the host-judged
path, and a non-finite residual -- gate reason 2, the state restored at the
check, the error raised after the run -- on one rank and on one rank of
several (host-staged torch transport, loopback threads, RCCL processes).  In
the multi-rank runs eps = 1e30 makes any finite residual converge at the first
check, so a NaN that the cross-rank max drops shows as a false "converged".
tests/test_nonfinite_cpu.py holds the CPU side.  Needs an MI355X."""
import functools
import re

import numpy as np
import pytest

from parallel_heat_amd import HeatConfig, HeatSolver, _native
from parallel_heat_amd.parallel.group import run_group

from . import service_cases as SC
from .dist_worker import run_outcome, run_outcomes

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------
# the threshold
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["graph", "eager", "host"])
def test_threshold_gpu(gpu, monkeypatch, mode):
    if mode == "host":
        monkeypatch.setenv("HEAT_HOST_CHECKS", "1")

    def solve(kw):
        with HeatSolver(HeatConfig(backend="hip", use_graph=mode != "eager", **kw)) as s:
            r = s.run()
            return r, s.gather()
    SC.check_threshold(solve)


# ---------------------------------------------------------------------------
# non-finite, one rank
# ---------------------------------------------------------------------------
# mode -> (plate, check interval, config, environment)
ONE_RANK = {
    "graph": ((64, 48), 5, dict(use_graph=True), {}),
    "eager": ((64, 48), 5, dict(use_graph=False), {}),
    "host": ((64, 48), 5, {}, {"HEAT_HOST_CHECKS": "1"}),
    "inside-depth-12": ((64, 48), 7, dict(tb_depth=12), {}),   # check at level 7 of a pass
    "resident": ((48, 96), 20, {}, {"HEAT_TB_RESIDENT": "1"}),  # test_gpu_resident's checked plate
}
BAD = {"nan": np.nan, "inf": np.inf}


def _config(shape, interval, **kw):
    return HeatConfig(nx=shape[0], ny=shape[1], steps=200, init="random", seed=13, converge=True,
                      check_interval=interval, eps=1e-3, **kw)


def _raise_and_gather(cfg, grid):
    with HeatSolver(cfg) as s:
        s.load_local(grid)
        with pytest.raises(_native.NativeError) as e:
            s.run()
        return str(e.value), s.gather()


@functools.lru_cache(maxsize=None)
def _cpu_after_raise(shape, interval, bad):
    grid = SC.bad_grid(*shape, (shape[0] // 2, shape[1] // 2), BAD[bad])
    msg, g = _raise_and_gather(_config(shape, interval, backend="cpu", tb_depth=1), grid)
    g.setflags(write=False)
    return msg, g


@pytest.mark.parametrize("bad", sorted(BAD))
@pytest.mark.parametrize("mode", sorted(ONE_RANK))
def test_nonfinite_one_rank(gpu, monkeypatch, mode, bad):
    shape, interval, kw, env = ONE_RANK[mode]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg = _config(shape, interval, backend="hip", **kw)
    if mode == "resident":  # the path under test is the resident one
        with HeatSolver(cfg.replace(eps=0.0)) as s:
            assert s.run(60).resident_passes > 0
    grid = SC.bad_grid(*shape, (shape[0] // 2, shape[1] // 2), BAD[bad])
    msg, g = _raise_and_gather(cfg, grid)
    assert "non-finite" in msg and re.search(rf"at step {interval}\b", msg), msg
    cpu_msg, want = _cpu_after_raise(shape, interval, bad)
    assert "non-finite" in cpu_msg and re.search(rf"at step {interval}\b", cpu_msg), cpu_msg
    assert np.isnan(want).any()
    SC.assert_same_bits(g, want, f"{mode} {bad}: state after the raise, GPU vs CPU backend")


# ---------------------------------------------------------------------------
# non-finite, several ranks
# ---------------------------------------------------------------------------
NX, NY, C = 24, 40, 5
SMALL = dict(nx=NX, ny=NY, steps=C, init="zero", converge=True, check_interval=C, eps=1e30,
             backend="hip")
WATCHDOG = {"HEAT_WATCHDOG_S": "30"}


@pytest.mark.parametrize("world,nan_rank", [(2, 0), (2, 1), (3, 0), (3, 1), (3, 2)])
def test_nonfinite_staged_torch_ranks(gpu, tmp_path, world, nan_rank):
    # GPU ranks of separate processes on one device, halos and the residual
    # max staged through the host and torch.distributed (gloo).
    at = SC.block_centres(NX, NY, world, 1)[nan_rank]
    texts = run_outcomes(world, dict(SMALL, decomp="rows"), C, SC.bad_grid(NX, NY, at, np.nan),
                         tmp_path, transport="torch", env=WATCHDOG)
    SC.assert_all_nonfinite(texts, C)


@pytest.mark.parametrize("world,kw,blocks", [
    (2, dict(decomp="rows"), (2, 1)),
    (3, dict(decomp="rows"), (3, 1)),
    (4, dict(px=2, py=2), (2, 2)),
])
def test_nonfinite_loopback_ranks(gpu, monkeypatch, world, kw, blocks):
    monkeypatch.setenv("HEAT_WATCHDOG_S", "30")
    for at in SC.block_centres(NX, NY, *blocks):
        grid = SC.bad_grid(NX, NY, at, np.nan)
        texts = run_group(HeatConfig(**{**SMALL, **kw}), world, lambda s: run_outcome(s, grid, C))
        SC.assert_all_nonfinite(texts, C)


# The plate of test_gpu_rccl_multirank.py; 20 steps, one check at the end.
RCCL = dict(nx=150, ny=300, steps=20, init="zero", converge=True, check_interval=20, eps=1e30,
            backend="hip", tb_depth=8, decomp="rows")


@pytest.mark.parametrize("nan_rank", [0, 1])
@pytest.mark.parametrize("kw,env", [
    (dict(use_graph=True), {"HEAT_TB_RESIDENT": "2"}),   # 2: resident spans on a shared device
    (dict(use_graph=False), {"HEAT_TB_RESIDENT": "2"}),
    (dict(use_graph=True), {"HEAT_TB_RESIDENT": "0"}),
], ids=["graph", "eager", "graph-no-resident"])
def test_nonfinite_rccl_ranks(gpu, tmp_path, kw, env, nan_rank):
    # Two RCCL processes on one device: the residual word goes through
    # ncclAllReduce(max) before each rank's own judge launch.
    at = SC.block_centres(150, 300, 2, 1)[nan_rank]
    texts = run_outcomes(2, {**RCCL, **kw}, 20, SC.bad_grid(150, 300, at, np.nan), tmp_path,
                         transport="rccl", env={**WATCHDOG, **env})
    SC.assert_all_nonfinite(texts, 20)
