"""Inputs and exact references shared by the oracle tests (CPU and GPU).

Value sets beyond the engine's own `init="random"` ([0, 100), all positive,
all normal), written into fields through `Field.set_owned` /
`HeatSolver.scatter`, and their step-by-step states under the independent
NumPy oracle `reference.step_np_fma` (or `step_np_mpi`), cached per
(set, shape, coefficients, numerics) so that every test of a module shares
one computation and nobody modifies it (the arrays are read-only)."""
import functools

import numpy as np

from parallel_heat_amd.models import reference as R

# Anisotropic pairs first: a kernel that swaps cx and cy, or uses one of them
# twice, differs from the oracle by ~10 on [0, 100) data after a few steps.
ANISO = (0.05, 0.2)
COEFFS = [(0.1, 0.1), (0.05, 0.2), (0.2, 0.05), (0.125, 0.25), (0.25, 0.0), (0.0, 0.25)]
SHAPES = [(3, 9), (37, 53), (203, 517)]
SETS = ["pos", "signed", "wide", "tiny"]
# Seed 8: the tiny set keeps >= half of its interior non-zero subnormal for
# every shape, coefficient pair and step count used (the 3 x 9 plate has only
# 7 interior cells; most seeds leave it mostly normal after 48 steps).
SEED = 8


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def assert_bitwise(got, want, what=""):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape
    same = bits(got) == bits(want)
    assert same.all(), (f"{what}: {int((~same).sum())} of {same.size} cells differ, max |diff| "
                        f"{np.nanmax(np.abs(got.astype(np.float64) - want.astype(np.float64)))}")


def values(name: str, nx: int, ny: int, seed: int = SEED) -> np.ndarray:
    """pos: [0, 100); signed: [-100, 100); wide: +-2^[-140, 100) (subnormals to
    huge, neighbours of very different magnitude); tiny: +-2^[-149, -120)
    (mostly subnormal: a flush-to-zero anywhere changes every cell)."""
    rng = np.random.default_rng(seed)
    if name == "pos":
        v = rng.random((nx, ny)) * 100
    elif name == "signed":
        v = rng.random((nx, ny)) * 200 - 100
    elif name == "wide":
        v = rng.choice([-1.0, 1.0], (nx, ny)) * 2.0 ** rng.uniform(-140, 100, (nx, ny))
    elif name == "tiny":
        v = rng.choice([-1.0, 1.0], (nx, ny)) * 2.0 ** rng.uniform(-149, -120, (nx, ny))
    else:
        raise ValueError(name)
    v = v.astype(np.float32)
    v.setflags(write=False)
    return v


def _frozen(a: np.ndarray) -> np.ndarray:
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def levels(name: str, nx: int, ny: int, cx: float, cy: float, steps: int,
           numerics: str = "fma", seed: int = SEED):
    """Tuple of the states after 0..steps oracle steps from values(name, ...)."""
    step = {"fma": R.step_np_fma, "mpi": R.step_np_mpi}[numerics]
    out = [values(name, nx, ny, seed)]
    for _ in range(steps):
        out.append(_frozen(step(out[-1], cx, cy)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def levels_of_init(nx: int, ny: int, cx: float, cy: float, steps: int, init: str = "random",
                   seed: int = 0, numerics: str = "fma"):
    """The same from the engine's own initial condition (R.init_grid)."""
    step = {"fma": R.step_np_fma, "mpi": R.step_np_mpi}[numerics]
    out = [_frozen(R.init_grid(nx, ny, init, seed))]
    for _ in range(steps):
        out.append(_frozen(step(out[-1], cx, cy)))
    return tuple(out)


def resid(lv, k: int) -> float:
    """max |state k - state k-1| as the engine reports it (fp32 differences)."""
    return float(np.abs(lv[k] - lv[k - 1]).max())


def subnormal_share(u: np.ndarray) -> float:
    """Share of the interior cells that are non-zero subnormals."""
    a = np.abs(u[1:-1, 1:-1])
    return float(((a > 0) & (a < np.finfo(np.float32).tiny)).mean())


def check_preconditions(name: str, lv) -> None:
    """Conditions on the REFERENCE alone that make a set worth running: the
    wide set never overflows, at least half of the tiny set's interior stays
    non-zero subnormal (flush-to-zero would be loud)."""
    if name == "wide":
        assert all(np.isfinite(s).all() for s in lv)
    if name == "tiny":
        share = subnormal_share(lv[-1])
        assert share >= 0.5, share
