"""Degenerate plates through the GPU solver, bitwise against the exact NumPy
oracle (`reference.step_np_fma`): plates with no interior, one interior cell,
row or column, fewer rows than a pass is deep, a width just past a strip
boundary, and the reference's own default run (20 x 20, 10000 steps), with
every kernel choice, graph and eager, resident tiles on and off; and loopback
rank groups whose block extent EQUALS the halo depth (the smallest the solver
accepts).  The same plates run on the CPU backend in
tests/test_small_plates_cpu.py.  Product library only.  Needs an MI355X."""
import functools

import pytest

from parallel_heat_amd import HeatConfig, HeatSolver
from parallel_heat_amd.models import reference as R
from parallel_heat_amd.parallel.group import run_group

from . import oracle_cases as O
from .oracle_cases import assert_bitwise
from .test_small_plates_cpu import CHUNKS, PLATES, SEED, oracle, plate_id, run_chunked, small_cfg

pytestmark = pytest.mark.gpu

# name -> (HeatConfig fields, HEAT_TB_RESIDENT or None)
SETTINGS = {
    "auto": (dict(), None),
    "auto_resident0": (dict(), "0"),
    "auto_resident1": (dict(), "1"),
    "tb8": (dict(kernel="tb", tb_depth=8), None),
    "tb12": (dict(kernel="tb", tb_depth=12), None),
    "lds": (dict(kernel="lds"), None),
    "naive": (dict(kernel="naive"), None),
}


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_small_plates_gpu_bitwise(gpu, monkeypatch, setting, use_graph):
    kw, resident = SETTINGS[setting]
    if resident is not None:
        monkeypatch.setenv("HEAT_TB_RESIDENT", resident)
    bad = []
    for plate in PLATES:
        lv = oracle(*plate)
        states, results = run_chunked(small_cfg(*plate, backend="hip", use_graph=use_graph, **kw))
        done = 0
        for n, got, r in zip(CHUNKS, states, results):
            done += n
            if r.steps_done != n:
                bad.append(f"{plate_id(plate)}: chunk of {n} ran {r.steps_done} steps")
            diff = O.bits(got) != O.bits(lv[done])
            if got.shape != lv[done].shape or diff.any():
                bad.append(f"{plate_id(plate)} after {done} steps: {int(diff.sum())} of "
                           f"{diff.size} cells differ")
    assert not bad, "\n".join(bad)


# -- the reference's default run ---------------------------------------------------

DEFAULT = dict(nx=20, ny=20, steps=10000, cx=0.1, cy=0.1, init="ref-wrap")


@functools.lru_cache(maxsize=None)
def _default_oracle(converge):
    g, done, at = R.run_np(**DEFAULT, converge=converge, check_interval=20, eps=1e-3,
                           numerics="fma")
    g.setflags(write=False)
    return g, done, at


def test_reference_default_run_gpu(gpu):
    with HeatSolver(HeatConfig(**DEFAULT, backend="hip")) as s:
        r = s.run()
        got = s.gather()
    want, done, _ = _default_oracle(False)
    assert r.steps_done == done == 10000
    assert_bitwise(got, want)


def test_reference_default_run_converging_gpu(gpu):
    cfg = HeatConfig(**DEFAULT, backend="hip", converge=True, check_interval=20, eps=1e-3)
    with HeatSolver(cfg) as s:
        r = s.run()
        got = s.gather()
    want, done, at = _default_oracle(True)
    assert (r.steps_done, r.converged_at) == (done, at)
    assert r.converged == (at > 0)
    assert_bitwise(got, want)


# -- rank groups whose blocks are exactly as thick as the halo ------------------------

@pytest.mark.parametrize("world,kw", [
    (2, dict(nx=16, ny=13, decomp="rows")),      # two 8-row blocks
    (2, dict(nx=13, ny=16, px=1, py=2)),         # two 8-column blocks
    (4, dict(nx=16, ny=16, px=2, py=2)),         # four 8 x 8 blocks, ghost corners
], ids=["rows_16x13", "cols_13x16", "grid_16x16"])
def test_loopback_block_extent_equals_halo(gpu, world, kw):
    steps = 45
    cfg = HeatConfig(steps=0, cx=O.ANISO[0], cy=O.ANISO[1], init="random", seed=SEED,
                     backend="hip", tb_depth=8, halo_passes=1, **kw)

    def fn(s):
        s.run(steps)
        return s.gather(), s.info.halo

    res = run_group(cfg, world, fn)
    assert {h for _, h in res} == {8}            # the blocks' extent: the edge of lx >= H
    got = next(g for g, _ in res if g is not None)
    want = O.levels_of_init(cfg.nx, cfg.ny, *O.ANISO, steps, "random", SEED)[steps]
    assert_bitwise(got, want)
