"""Inputs, references and checks shared by the refinement tests (CPU and GPU).

The reference is `reference.refine_np` (NumPy gathers and the oracle's fma32,
no code shared with the engine).  Equality is bitwise throughout: nothing here
has a tolerance.  Sources and references are cached per case and read-only, so
every test of a module shares one computation and nobody modifies it."""
import functools
import os

import numpy as np

from parallel_heat_amd.models import reference as R

from .coarse_cases import block_spans
from .dist_worker import free_port
from .oracle_cases import values

# (nx, ny, fx, fy): partial last cells; factor 1; CC == 1; a factor larger
# than the plate; whole cells.
CASES = [(37, 53, 4, 8), (9, 519, 1, 3), (130, 70, 64, 300), (5, 5, 7, 2), (64, 256, 8, 8)]
GPU_CASES = CASES + [(70, 777, 8, 16)]   # more than three strips of 256 columns
ORDERS = [0, 1]
WRAPS = ["", "x", "y", "xy"]
KINDS = ["int", "signed", "wide"]        # wide: +-2^[-140, 100), subnormals to huge
BLOCK_PLATE = (37, 53, 4, 8)
BLOCK_CUTS = [(2, 2), (3, 1)]


def case_id(c):
    return "x".join(str(v) for v in c[:2]) + "-f" + "x".join(str(v) for v in c[2:])


def dims(case):
    nx, ny, fx, fy = case
    return -(-nx // fx), -(-ny // fy)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def source(kind: str, cr: int, cc: int) -> np.ndarray:
    if kind == "int":
        g = np.random.default_rng(23).integers(-2 ** 15, 2 ** 15 + 1, size=(cr, cc))
        g = g.astype(np.float32)
    else:
        g = np.array(values(kind, cr, cc), np.float32)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def expected(kind: str, case, order: int, wrap: str) -> np.ndarray:
    nx, ny, fx, fy = case
    g = R.refine_np(source(kind, *dims(case)), nx, ny, fx, fy, order, wrap)
    g.setflags(write=False)
    return g


def assert_bitwise(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape)
    same = bits(got) == bits(want)
    assert same.all(), (what, np.argwhere(~same)[:8])


def nan_field(lx: int, ly: int, device, halo: int = 2):
    """A Field that is NaN everywhere: owned block, ghost ring, pitch padding."""
    from parallel_heat_amd import ops
    return ops.Field(lx, ly, halo=halo, device=device, fill=float("nan"))


def assert_frame_intact(f, what=""):
    """Everything but the owned block is still NaN: nothing was written there."""
    import torch
    d = f.data.clone()
    d[f.hx:f.hx + f.lx, f.hy:f.hy + f.ly] = float("nan")
    assert bool(torch.isnan(d).all()), (what, "a ghost or padding cell was written")


def check_case(device, case, halo: int = 2, kinds=KINDS):
    """ops.refine of the whole plate, every order, wrap and kind of data, into a
    NaN-framed field: the oracle bit for bit, the frame untouched."""
    from parallel_heat_amd import ops
    nx, ny, fx, fy = case
    for kind in kinds:
        S = source(kind, *dims(case))
        for order in ORDERS:
            for wrap in WRAPS:
                f = nan_field(nx, ny, device, halo)
                ops.refine(f, S, fx, fy, order=order, wrap=wrap)
                what = (case, kind, order, wrap, halo)
                assert_bitwise(f.owned().cpu().numpy(), expected(kind, case, order, wrap), what)
                assert_frame_intact(f, what)


def check_blocks(device, cut, halo: int = 2):
    """The plate cut px x py (heat_block_span), every block refined on its own
    at its offset: together the whole plate."""
    from parallel_heat_amd import ops
    nx, ny, fx, fy = BLOCK_PLATE
    S = source("signed", *dims(BLOCK_PLATE))
    for order in ORDERS:
        for wrap in WRAPS:
            got = np.full((nx, ny), np.nan, np.float32)
            for ox, lx in block_spans(nx, cut[0]):
                for oy, ly in block_spans(ny, cut[1]):
                    f = nan_field(lx, ly, device, halo)
                    ops.refine(f, S, fx, fy, order=order, wrap=wrap, ox=ox, oy=oy, nx=nx, ny=ny)
                    assert_frame_intact(f, (cut, ox, oy))
                    got[ox:ox + lx, oy:oy + ly] = f.owned().cpu().numpy()
            assert_bitwise(got, expected("signed", BLOCK_PLATE, order, wrap), (cut, order, wrap))


# -- properties of the definition (checked on the oracle AND on a device's result) ---------

def check_order0_inverts_coarse(refined, S, fx, fy):
    c = R.coarse_np(refined, fx, fy)
    assert np.array_equal(c["min"], S) and np.array_equal(c["max"], S)
    assert np.array_equal((c["sum"] / c["count"]).astype(np.float32), S)


def linear_source(nx, ny, fx, fy):
    """S[I, J] = 3 * c2_I + 5 * c2_J: a plane in plate coordinates."""
    def c2(n, f):
        i = np.arange(-(-n // f), dtype=np.int64)
        return i * f + np.minimum((i + 1) * f, n) - 1
    return (3 * c2(nx, fx)[:, None] + 5 * c2(ny, fy)[None, :]).astype(np.float32)


def check_linear_exact(refined, nx, ny, fx, fy):
    """Between the first and the last centres the plane 3 * 2i + 5 * 2j comes
    back exactly (power-of-two factors dividing the plate: every weight and
    every product is exact)."""
    i = np.arange(nx)[:, None]
    j = np.arange(ny)[None, :]
    want = (3 * 2 * i + 5 * 2 * j).astype(np.float32)
    inner = ((2 * i >= fx - 1) & (2 * i <= 2 * nx - fx - 1)
             & (2 * j >= fy - 1) & (2 * j <= 2 * ny - fy - 1))
    assert inner.sum() > 0
    assert np.array_equal(np.asarray(refined)[inner], want[inner])


def nan_footprint(case, wrap, spot):
    """The plate cells whose four taps include source cell `spot` with a
    non-zero weight, from the oracle's tables."""
    nx, ny, fx, fy = case
    i0, i1, wx = R.refine_axis_np(nx, fx, 1, "x" in wrap)
    j0, j1, wy = R.refine_axis_np(ny, fy, 1, "y" in wrap)
    rows = (i0 == spot[0]) | ((i1 == spot[0]) & (wx != 0))
    cols = (j0 == spot[1]) | ((j1 == spot[1]) & (wy != 0))
    return rows[:, None] & cols[None, :]


# -- solver ----------------------------------------------------------------------------------

SOLVER_CASE = (37, 53, 4, 8)
SOLVER_STEPS = (0, 1, 25)
EDGES = [dict(), dict(insulated="all"), dict(periodic="xy")]
EDGE_IDS = ["dirichlet", "insulated", "periodic"]


@functools.lru_cache(maxsize=None)
def solver_levels(case, order: int, insulated: str, periodic: str, steps: int = 25):
    """States 0..steps of the oracle (step_np_fma) from refine_np of the case's
    signed source, wrapping where the run is periodic."""
    lv = [np.array(expected("signed", case, order, periodic))]
    for _ in range(steps):
        lv.append(R.step_np_fma(lv[-1], 0.1, 0.1, insulated, periodic))
    for g in lv:
        g.setflags(write=False)
    return tuple(lv)


def check_solver(backend: str, edges: dict, case=SOLVER_CASE, order: int = 1, infer=False, **kw):
    """refine, then 0, 1 and 25 steps, against the oracle; then a run, refine
    and a run again (graphs captured before the refine are replayed after)."""
    from parallel_heat_amd import HeatConfig, HeatSolver
    nx, ny, fx, fy = case
    S = source("signed", *dims(case))
    lv = solver_levels(case, order, edges.get("insulated", ""), edges.get("periodic", ""))
    cfg = HeatConfig(nx=nx, ny=ny, steps=0, init="random", seed=3, backend=backend, **edges, **kw)
    with HeatSolver(cfg) as s:
        for steps in SOLVER_STEPS:
            s.refine(S, None if infer else fx, None if infer else fy, order=order)
            assert s.step == 0
            if steps:
                s.run(steps)
            assert s.step == steps
            assert_bitwise(s.gather(), lv[steps], (backend, edges, order, steps))
        s.refine(S, fx, fy, order=order, step=7)
        assert s.step == 7
        r = s.run(25)
        assert_bitwise(s.gather(), lv[25], (backend, edges, order, "again"))
        s.reset()   # still the formula initial condition, not S
        assert s.step == 0
        assert_bitwise(s.gather(), R.init_grid(nx, ny, "random", 3), "reset")
    return r


def worker(rank, world, port, cfg_kwargs, src_path, fx, fy, order, steps, out_dir):
    """A gloo rank on the CPU backend: refine (not collective: every rank passes
    the same S), gather, run, gather."""
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from parallel_heat_amd import HeatConfig, HeatSolver
    from parallel_heat_amd.parallel.comm import DistInfo

    s = HeatSolver(HeatConfig(**cfg_kwargs), transport="torch",
                   dist_info=DistInfo(rank, world, rank))
    s.refine(np.load(src_path), fx, fy, order=order)
    g0 = s.gather()
    s.run(steps)
    g1 = s.gather()
    if rank == 0:
        np.savez(os.path.join(out_dir, "refine_0.npz"), px=s.info.px, py=s.info.py, g0=g0, g1=g1)
    s.close()
    dist.barrier()
    dist.destroy_process_group()


def run_world(world, cfg_kwargs, S, fx, fy, order, steps, tmp_path):
    import torch.multiprocessing as mp

    src_path = str(tmp_path / "source.npy")
    np.save(src_path, S)
    mp.spawn(worker, args=(world, free_port(), cfg_kwargs, src_path, fx, fy, order, steps,
                           str(tmp_path)), nprocs=world, join=True)
    return dict(np.load(tmp_path / "refine_0.npz"))
