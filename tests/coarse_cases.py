"""Inputs, references and checks shared by the coarse-view tests (CPU and GPU).

The reference is `reference.coarse_np` (NumPy reduceat, no code shared with
the engine) and, for sums of general values, `math.fsum` per coarse cell.
Inputs are cached per shape and read-only, so every test of a module shares
one computation and nobody modifies it."""
import functools
import math

import numpy as np

from parallel_heat_amd.models import reference as R

from .oracle_cases import values

SHAPES = [(1, 1), (5, 3), (37, 53), (64, 256), (33, 255), (33, 257), (70, 519), (9, 1030)]
FACTORS = [(1, 1), (2, 2), (3, 5), (4, 4), (7, 3), (8, 64), (16, 256), (5, 300), (64, 1),
           (1, 64), (1000, 1000)]
# Blocks of a 37 x 53 plate whose edges fall inside coarse cells.
MERGE_SHAPE = (37, 53)
MERGE_GRIDS = [(2, 2), (3, 1)]
MERGE_FACTORS = [(4, 6), (5, 5)]
# General values (oracle_cases.values): signed, +-2^[-140, 100), mostly subnormal.
GENERAL_SETS = ["signed", "wide", "tiny"]
GENERAL_SHAPE = (37, 53)
GENERAL_FACTORS = [(4, 6), (1, 1), (37, 53), (5, 300)]
U = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def int_grid(nx: int, ny: int, seed: int = 11) -> np.ndarray:
    """Integers in [-2^15, 2^15] as float32: every partial sum of a coarse
    cell is exact in fp64, so sums are equal bit for bit in any order."""
    g = np.random.default_rng(seed).integers(-2 ** 15, 2 ** 15 + 1, size=(nx, ny))
    g = g.astype(np.float32)
    g.setflags(write=False)
    return g


def planes(d) -> dict:
    """sum / min / max of a result (torch tensors or arrays) as NumPy arrays."""
    out = {}
    for k in ("sum", "min", "max"):
        v = d[k]
        out[k] = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
    return out


def assert_minmax_exact(got, want, what=""):
    for k in ("min", "max"):
        assert got[k].dtype == np.float32 and got[k].shape == want[k].shape, (what, k)
        # As numbers: NaN equals NaN, the sign of a zero is unspecified.
        assert np.array_equal(got[k], want[k], equal_nan=True), (
            what, k, np.argwhere(~((got[k] == want[k]) | (np.isnan(got[k]) & np.isnan(want[k])))))


def assert_exact(got, grid, fx, fy, what=""):
    """All three planes equal to the oracle's (sums bit for bit)."""
    got, want = planes(got), R.coarse_np(grid, fx, fy)
    assert_minmax_exact(got, want, what)
    assert got["sum"].dtype == np.float64 and got["sum"].shape == want["sum"].shape, what
    same = (got["sum"] == want["sum"]) | (np.isnan(got["sum"]) & np.isnan(want["sum"]))
    assert same.all(), (what, "sum", np.argwhere(~same)[:8])


def assert_within_bound(got, grid, fx, fy, what=""):
    """min / max exact; |sum - exact| <= g * S per coarse cell, g = (n-1)u /
    (1 - (n-1)u), u = 2^-53, n the cell count, exact and S = sum |v| from
    math.fsum: the bound of ANY fp64 summation order (derived, not measured)."""
    got, want = planes(got), R.coarse_np(grid, fx, fy)
    assert_minmax_exact(got, want, what)
    g64 = np.asarray(grid, np.float32).astype(np.float64)
    nx, ny = g64.shape
    worst = 0.0
    for i in range(want["sum"].shape[0]):
        for j in range(want["sum"].shape[1]):
            cell = g64[i * fx:(i + 1) * fx, j * fy:(j + 1) * fy].ravel().tolist()
            n = len(cell)
            assert n == want["count"][i, j]
            exact, s_abs = math.fsum(cell), math.fsum(abs(v) for v in cell)
            gam = (n - 1) * U / (1 - (n - 1) * U)
            err = abs(float(got["sum"][i, j]) - exact)
            assert err <= gam * s_abs, (what, i, j, err, gam * s_abs)
            if s_abs > 0:
                worst = max(worst, err / s_abs)
    return worst


def general_grid(name: str) -> np.ndarray:
    return values(name, *GENERAL_SHAPE)


# One NaN at a time: the four corners of coarse cell (2, 3) of the 37 x 53 plate
# at factors 4 x 6 (rows 8..11, columns 18..23) and the last, partial cell
# (row 36, columns 48..52).
NAN_SHAPE, NAN_FACTORS = (37, 53), (4, 6)
NAN_SPOTS = [((8, 18), (2, 3)), ((8, 23), (2, 3)), ((11, 18), (2, 3)), ((11, 23), (2, 3)),
             ((36, 52), (9, 8))]


def nan_grid(spot) -> np.ndarray:
    g = int_grid(*NAN_SHAPE).copy()
    g[spot] = np.nan
    return g


def assert_one_nan_cell(got, spot, cell):
    """Exactly `cell` is NaN, in all three planes; every other coarse cell is
    what the plate without the NaN gives."""
    got, clean = planes(got), R.coarse_np(int_grid(*NAN_SHAPE), *NAN_FACTORS)
    for k in ("sum", "min", "max"):
        isn = np.isnan(got[k])
        assert isn[cell] and isn.sum() == 1, (spot, k, np.argwhere(isn))
        rest = ~isn
        assert np.array_equal(got[k][rest], clean[k][rest]), (spot, k)


def inf_grid() -> np.ndarray:
    """+inf and -inf inside coarse cell (2, 3), +inf alone in cell (0, 0)."""
    g = int_grid(*NAN_SHAPE).copy()
    g[9, 19] = np.inf
    g[10, 22] = -np.inf
    g[1, 2] = np.inf
    return g


def assert_inf_cells(got):
    got = planes(got)
    assert np.isnan(got["sum"][2, 3]) and got["min"][2, 3] == -np.inf and got["max"][2, 3] == np.inf
    assert got["sum"][0, 0] == np.inf and got["max"][0, 0] == np.inf
    assert np.isfinite(got["min"][0, 0])
    want = R.coarse_np(inf_grid(), *NAN_FACTORS)
    assert_minmax_exact(got, want, "inf")
    assert np.isnan(got["sum"]).sum() == 1 and np.isinf(got["sum"]).sum() == 1


def block_spans(n: int, parts: int):
    """(offset, size) of every part of n, as the engine cuts it (heat_block_span)."""
    import ctypes

    from parallel_heat_amd import _native
    out = []
    for i in range(parts):
        o, z = ctypes.c_int64(0), ctypes.c_int64(0)
        _native.call("heat_block_span", n, parts, i, ctypes.byref(o), ctypes.byref(z))
        out.append((int(o.value), int(z.value)))
    return out


# -- the cases themselves, on any device ("cpu": the host twin) ----------------------------

def field_of(grid: np.ndarray, device, halo: int = 2):
    """A Field holding `grid` whose ghost ring (depth `halo`) and pitch padding
    are NaN: nothing outside the owned block may reach a plane."""
    import torch

    from parallel_heat_amd import ops
    f = ops.Field(grid.shape[0], grid.shape[1], halo=halo, device=device, fill=float("nan"))
    f.set_owned(torch.from_numpy(np.array(grid, np.float32)).to(device))
    return f


def coarse_of(grid: np.ndarray, fx: int, fy: int, device):
    from parallel_heat_amd import ops
    return ops.coarse(field_of(grid, device), fx, fy)


def check_shape_against_oracle(device, shape):
    from parallel_heat_amd import ops
    grid = int_grid(*shape)
    f = field_of(grid, device)
    for fx, fy in FACTORS:
        got = ops.coarse(f, fx, fy)
        assert_exact(got, grid, fx, fy, (shape, fx, fy))
        assert np.array_equal(got["count"].numpy(), R.coarse_np(grid, fx, fy)["count"])


def check_blocks_add_up(device, cut, factors):
    """The plate cut px x py (heat_block_span), merged block by block."""
    from parallel_heat_amd import ops
    grid = int_grid(*MERGE_SHAPE)
    nx, ny = grid.shape
    fx, fy = factors
    out = None
    for ox, lx in block_spans(nx, cut[0]):
        for oy, ly in block_spans(ny, cut[1]):
            f = field_of(grid[ox:ox + lx, oy:oy + ly], device)
            out = ops.coarse(f, fx, fy, ox=ox, oy=oy, nx=nx, ny=ny, out=out)
    assert_exact(out, grid, fx, fy, (cut, factors))


def check_general_values(device, name):
    grid = general_grid(name)
    for fx, fy in GENERAL_FACTORS:
        assert_within_bound(coarse_of(grid, fx, fy, device), grid, fx, fy, (name, fx, fy))


def check_nonfinite(device):
    for spot, cell in NAN_SPOTS:
        assert_one_nan_cell(coarse_of(nan_grid(spot), *NAN_FACTORS, device), spot, cell)
    assert_inf_cells(coarse_of(inf_grid(), *NAN_FACTORS, device))


SOLVER_SHAPE, SOLVER_FACTORS, SOLVER_STEPS = (70, 519), (4, 8), 24
EDGES = [dict(), dict(insulated="all"), dict(periodic="xy")]


def check_solver(backend: str, edges: dict, shape=SOLVER_SHAPE, **kw):
    """coarse() after 24 steps against the oracle on gather(); then 24 more
    steps equal an uninterrupted 48-step run bit for bit.  Returns the last
    run's result (resident_passes, ...)."""
    from parallel_heat_amd import HeatConfig, HeatSolver
    cfg = HeatConfig(nx=shape[0], ny=shape[1], steps=0, init="random", seed=5, backend=backend,
                     **edges, **kw)
    fx, fy = SOLVER_FACTORS
    with HeatSolver(cfg) as s:
        s.run(SOLVER_STEPS)
        v = s.coarse(fx, fy)
        grid = s.gather()
        assert_within_bound(v, grid, fx, fy, (backend, edges))
        want = R.coarse_np(grid, fx, fy)
        assert np.array_equal(v["count"], want["count"])
        assert v["mean"].dtype == np.float64 and np.array_equal(v["mean"], v["sum"] / v["count"])
        assert s.step == SOLVER_STEPS
        r = s.run(SOLVER_STEPS)
        after = s.gather()
    with HeatSolver(cfg) as s:
        s.run(2 * SOLVER_STEPS)
        straight = s.gather()
    assert np.array_equal(after.view(np.uint32), straight.view(np.uint32)), (backend, edges)
    return r
