"""Degenerate plates on the CPU backend against the exact NumPy oracle
(`reference.step_np_fma`): plates without an interior (1 x 1, 1 x N, N x 1,
2 x 2), one interior cell, one interior row or column, and the reference's own
20 x 20.  tests/test_gpu_small_plates.py runs the same plates on the GPU
against the same oracle states; this file pins that oracle (and the CPU
backend on these shapes) where there is no GPU."""
import pytest

from parallel_heat_amd import HeatConfig, HeatSolver

from . import oracle_cases as O
from .oracle_cases import assert_bitwise

# (nx, ny).  13 x 519: two float4 strips at depth 12 (W = 232), the plate's
# last column in lane element 2, fewer rows than two passes are deep.
PLATES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (3, 9), (4, 4), (20, 20), (5, 300), (300, 5),
          (13, 519)]
CHUNKS = (5, 1, 17, 14)
STEPS = sum(CHUNKS)
SEED = 4


def plate_id(p):
    return f"{p[0]}x{p[1]}"


def oracle(nx, ny):
    """States 0..STEPS of the plate from init="random", anisotropic."""
    return O.levels_of_init(nx, ny, *O.ANISO, STEPS, "random", SEED)


def run_chunked(cfg):
    """The state after each chunk of CHUNKS and the run results."""
    states, results = [], []
    with HeatSolver(cfg) as s:
        for n in CHUNKS:
            results.append(s.run(n))
            states.append(s.gather())
    return states, results


def check_chunked(cfg):
    lv = oracle(cfg.nx, cfg.ny)
    states, results = run_chunked(cfg)
    done = 0
    for n, got, r in zip(CHUNKS, states, results):
        done += n
        assert r.steps_done == n
        assert_bitwise(got, lv[done], f"after {done} steps")


def small_cfg(nx, ny, **kw):
    return HeatConfig(nx=nx, ny=ny, steps=0, cx=O.ANISO[0], cy=O.ANISO[1], init="random",
                      seed=SEED, **kw)


@pytest.mark.parametrize("depth", [1, 8])
@pytest.mark.parametrize("plate", PLATES, ids=plate_id)
def test_small_plate_cpu_bitwise(plate, depth):
    check_chunked(small_cfg(*plate, backend="cpu", tb_depth=depth))


@pytest.mark.parametrize("plate", [(1, 1), (1, 7), (7, 1), (2, 2)], ids=plate_id)
def test_no_interior_plate_never_changes(plate):
    # The oracle itself on a plate that is all ring: every state is the first.
    lv = oracle(*plate)
    for s in lv[1:]:
        assert_bitwise(s, lv[0])
