"""Insulated (zero-flux) plate edges on the GPU: the ghost-fill kernel alone,
then every kernel family, the resident spans, loopback ranks and the
device-judged convergence path, bitwise against the CPU backend (which
tests/test_insulated_cpu.py ties to the exact NumPy oracle).  The stencil
kernels never learn about the option: they see a plate extended into the
ghost ring, which csrc/kernels/ghost_fill.hip keeps equal to the plate's mirror
image.  Needs an MI355X."""
import functools

import numpy as np
import pytest
import torch

from parallel_heat_amd import HeatConfig, HeatSolver, ops
from parallel_heat_amd.parallel.group import run_group

pytestmark = pytest.mark.gpu

CHUNKS = (5, 1, 17, 22, 8)  # 53 steps


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# --------------------------------------------------------------------------
# the fill kernel alone
# --------------------------------------------------------------------------
def fill_expected(full, hx, hy, lx, ly, sides, d):
    """The field array after the fill: every cell of the frame
    [-d, lx+d) x [-d, ly+d) takes its per-axis reflection across the insulated
    sides it lies beyond (np.pad's "reflect"); a cell beyond none of them maps
    to itself, as does everything outside the frame."""
    n, s, w, e = (c in sides for c in "nswe")
    r = np.arange(-d, lx + d)
    c = np.arange(-d, ly + d)
    sr = np.where(n & (r < 0), -r, np.where(s & (r >= lx), 2 * (lx - 1) - r, r))
    sc = np.where(w & (c < 0), -c, np.where(e & (c >= ly), 2 * (ly - 1) - c, c))
    want = full.copy()
    want[(hx + r)[:, None], (hy + c)[None, :]] = full[(hx + sr)[:, None], (hy + sc)[None, :]]
    return want


@pytest.mark.parametrize("lx,ly,halo,d", [
    (37, 70, 12, 12),      # the frame as deep as the ring; ly % 4 == 2: a scalar row tail
    (37, 70, 12, 1),
    (37, 72, 12, 12),      # whole float4 rows
    (40, 67, 12, 5),       # a frame shallower than the ring: cells beyond it stay
    (300, 1100, 96, 96),   # the deepest halo: several workgroups per side, long rows
])
def test_fill_kernel_all_side_subsets(gpu, lx, ly, halo, d):
    rng = np.random.default_rng(lx + ly + d)
    f = ops.Field(lx, ly, halo, gpu)
    start = rng.random(tuple(f.data.shape), np.float32)
    # Every ghost and padding cell NaN, each with its own payload, so that a
    # cell written from the wrong NaN source shows.
    nan = (np.uint32(0x7FC00000) + np.arange(start.size, dtype=np.uint32).reshape(start.shape)
           % np.uint32(1 << 20)).view(np.float32)
    own = np.zeros(start.shape, bool)
    own[f.hx:f.hx + lx, f.hy:f.hy + ly] = True
    start = np.where(own, start, nan)
    masks = range(1, 16) if lx < 100 else (15, 9, 6)
    for mask in masks:
        sides = "".join(c for k, c in enumerate("nswe") if mask >> k & 1)
        f.data.copy_(torch.from_numpy(start))
        ops.fill_insulated_ghosts(f, sides, d)
        torch.cuda.synchronize()
        got = f.data.cpu().numpy()
        want = fill_expected(start, f.hx, f.hy, lx, ly, sides, d)
        # Targets hold their reflection; every other cell (the owned block,
        # cells beyond Dirichlet sides only, the padding) is bit-unchanged.
        assert np.array_equal(bits(got), bits(want)), sides
        pad = ((d * ("n" in sides), d * ("s" in sides)), (d * ("w" in sides), d * ("e" in sides)))
        frame = got[f.hx - pad[0][0]:f.hx + lx + pad[0][1], f.hy - pad[1][0]:f.hy + ly + pad[1][1]]
        assert np.array_equal(frame, np.pad(start[f.hx:f.hx + lx, f.hy:f.hy + ly], pad,
                                            mode="reflect")), sides


def test_fill_kernel_rejects_bad_arguments(gpu):
    f = ops.Field(10, 20, 4, gpu)
    with pytest.raises(ValueError):
        ops.fill_insulated_ghosts(f, "n", 5)      # deeper than the ring
    with pytest.raises(ValueError):
        ops.fill_insulated_ghosts(f, "x", 1)
    with pytest.raises(ValueError):
        ops.fill_insulated_ghosts(ops.Field(4, 20, 4, gpu), "s", 4)  # no rows 1..4 to mirror


# --------------------------------------------------------------------------
# every kernel family, one rank
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cpu_reference(nx, ny, sides, steps, seed=3):
    cfg = HeatConfig(nx=nx, ny=ny, steps=steps, init="random", seed=seed, backend="cpu",
                     insulated=sides, tb_depth=1)
    with HeatSolver(cfg) as s:
        s.run()
        return s.gather(), s.checksum()


def gpu_run(cfg, chunks=CHUNKS):
    with HeatSolver(cfg) as s:
        rs = [s.run(n) for n in chunks]
        return s.gather(), rs, s.info


KERNELS = {
    "naive": dict(kernel="naive"),
    "lds3": dict(kernel="lds", tb_depth=3),
    "tb8": dict(kernel="tb", tb_depth=8),
    "tb12": dict(kernel="tb", tb_depth=12),
    "tile": dict(kernel="tb", tb_depth=8),   # with the workgroup-tile variant forced
    "auto": dict(),
}


@pytest.mark.parametrize("sides", ["nswe", "n", "e", "nw", "ns"])
@pytest.mark.parametrize("nx,ny", [(203, 517), (150, 300)])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_kernel_families_bitwise(gpu, kernel, nx, ny, sides):
    cfg = HeatConfig(nx=nx, ny=ny, steps=0, init="random", seed=3, backend="hip", device=0,
                     insulated=sides, **KERNELS[kernel])
    saved = ops.tb_tuning()
    if kernel == "tile":
        t = ops.tb_tuning()
        t.variant = int(ops.TbVariant.TILE | ops.TbVariant.XCD_GROUPS)
        ops.set_tb_tuning(t)
    try:
        got, rs, info = gpu_run(cfg)
    finally:
        ops.set_tb_tuning(saved)
    want, _ = cpu_reference(nx, ny, sides, sum(CHUNKS))
    assert sum(r.steps_done for r in rs) == sum(CHUNKS) and info.insulated == sides
    assert info.schedule == "sync" and info.halo >= info.tb_depth
    assert np.array_equal(bits(got), bits(want)), np.abs(got - want).max()


@pytest.mark.parametrize("kernel", ["tb12", "lds3", "auto"])
def test_kernel_families_eager(gpu, kernel):
    cfg = HeatConfig(nx=203, ny=517, steps=0, init="random", seed=3, backend="hip", device=0,
                     insulated="nswe", use_graph=False, **KERNELS[kernel])
    got, _, _ = gpu_run(cfg)
    want, _ = cpu_reference(203, 517, "nswe", sum(CHUNKS))
    assert np.array_equal(bits(got), bits(want))


def test_halo_passes_set_the_ghost_depth(gpu, monkeypatch):
    # One rank with an insulated side takes the multi-rank halo rule: m passes
    # per ghost fill, from the parameter or HEAT_HALO_PASSES, clamped so that
    # the block still holds the mirror sources (rows 1..H).
    base = HeatConfig(nx=150, ny=300, steps=0, init="random", seed=3, backend="hip", device=0,
                      insulated="nswe", kernel="tb", tb_depth=8)
    want, _ = cpu_reference(150, 300, "nswe", sum(CHUNKS))
    for m, halo in ((1, 8), (3, 24), (40, 144)):  # (150 - 1) // 8 = 18 passes at most
        got, rs, info = gpu_run(base.replace(halo_passes=m))
        assert info.halo == halo
        assert np.array_equal(bits(got), bits(want)), m
    monkeypatch.setenv("HEAT_HALO_PASSES", "2")
    got, rs, info = gpu_run(base)
    assert info.halo == 16 and sum(r.exchanges for r in rs) >= sum(CHUNKS) // 16
    assert np.array_equal(bits(got), bits(want))
    # Dirichlet edges only: no ghosts, no fill, whatever is asked.
    with HeatSolver(base.replace(insulated="", halo_passes=3)) as s:
        assert s.info.halo == 8 and s.run(24).exchanges == 0


def test_mpi_numerics_insulated(gpu):
    want = None
    for kernel in ("lds", "naive"):
        cfg = HeatConfig(nx=150, ny=300, steps=0, init="random", seed=3, backend="hip", device=0,
                         insulated="nswe", numerics="mpi", kernel=kernel, tb_depth=2)
        got, _, _ = gpu_run(cfg)
        if want is None:
            with HeatSolver(cfg.replace(backend="cpu", tb_depth=1)) as c:
                c.run(sum(CHUNKS))
                want = c.gather()
        assert np.array_equal(bits(got), bits(want)), kernel


def test_mfma_insulated_within_bound(gpu):
    steps = sum(CHUNKS)
    cfg = HeatConfig(nx=150, ny=300, steps=0, init="random", seed=3, backend="hip", device=0,
                     insulated="nswe", kernel="mfma", tb_depth=4)
    got, _, _ = gpu_run(cfg)
    want, _ = cpu_reference(150, 300, "nswe", steps)
    dev = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    print(f"mfma, insulated, {steps} steps: max |got - oracle| = {dev:.3e} "
          f"(bound {steps * 2e-5:.1e})")
    # The bound of tests/test_gpu_coefficients_solver.py: one mfma step is
    # within 2e-5 of the exact one on [0, 100) data, and the insulated step is
    # a convex combination too (the mirror doubles a weight), so the errors of
    # n steps add up to at most n * 2e-5.
    assert dev <= steps * 2e-5


# --------------------------------------------------------------------------
# resident spans
# --------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny,sides", [(700, 300, "nswe"), (203, 517, "nswe"), (700, 300, "ns")])
def test_resident_spans_bitwise(gpu, monkeypatch, nx, ny, sides):
    cfg = HeatConfig(nx=nx, ny=ny, steps=0, init="random", seed=3, backend="hip", device=0,
                     insulated=sides)
    want, _ = cpu_reference(nx, ny, sides, 96)
    monkeypatch.setenv("HEAT_TB_RESIDENT", "1")
    got, rs, info = gpu_run(cfg, chunks=(96,))
    assert rs[0].resident_passes > 0, (rs[0], info)
    assert np.array_equal(bits(got), bits(want)), np.abs(got - want).max()
    monkeypatch.setenv("HEAT_TB_RESIDENT", "0")
    got0, rs0, _ = gpu_run(cfg, chunks=(96,))
    assert rs0[0].resident_passes == 0
    assert np.array_equal(bits(got0), bits(want))


# --------------------------------------------------------------------------
# loopback ranks (threads of this process sharing the GPU)
# --------------------------------------------------------------------------
WORLDS = {
    "2rows": (2, dict(decomp="rows")),
    "1x2": (2, dict(px=1, py=2)),
    "3rows": (3, dict(decomp="rows")),
    "4auto": (4, dict(decomp="auto")),
}


def group_run(cfg, world):
    def fn(s):
        for n in CHUNKS:
            s.run(n)
        return s.gather(), s.checksum(), s.info
    out = run_group(cfg, world, fn)
    grid = next(g for g, _, _ in out if g is not None)
    return grid, [c for _, c, _ in out], [i for _, _, i in out]


@pytest.mark.parametrize("sides", ["nswe", "nw"])
@pytest.mark.parametrize("halo_passes", [0, 1, 2, 3])
@pytest.mark.parametrize("world", list(WORLDS))
def test_loopback_ranks_bitwise(gpu, world, halo_passes, sides):
    n, kw = WORLDS[world]
    cfg = HeatConfig(nx=150, ny=300, steps=0, init="random", seed=3, backend="hip", device=0,
                     insulated=sides, tb_depth=8, halo_passes=halo_passes, **kw)
    grid, sums, infos = group_run(cfg, n)
    want, cs = cpu_reference(150, 300, sides, sum(CHUNKS))
    assert np.array_equal(bits(grid), bits(want)), np.abs(grid - want).max()
    assert all(c["hash"] == cs["hash"] and c["count"] == cs["count"] for c in sums)
    assert len({i.halo for i in infos}) == 1  # every rank took the same ghost depth
    if halo_passes:
        assert infos[0].halo == 8 * halo_passes


def test_loopback_overlap_falls_back_to_sync(gpu):
    cfg = HeatConfig(nx=150, ny=300, steps=0, init="random", seed=3, backend="hip", device=0,
                     insulated="nswe", tb_depth=8, schedule="overlap", decomp="rows")
    grid, sums, infos = group_run(cfg, 2)
    assert all(i.schedule == "sync" for i in infos)
    want, cs = cpu_reference(150, 300, "nswe", sum(CHUNKS))
    assert np.array_equal(bits(grid), bits(want))
    assert all(c["hash"] == cs["hash"] for c in sums)
    # Without insulated sides the schedule is kept.
    out = run_group(cfg.replace(insulated=""), 2, lambda s: s.info.schedule)
    assert out == ["overlap", "overlap"]


# --------------------------------------------------------------------------
# device-judged convergence
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cpu_converged(interval):
    cfg = HeatConfig(nx=48, ny=96, steps=40000, converge=True, check_interval=interval,
                     init="random", seed=3, backend="cpu", insulated="nswe", tb_depth=1)
    with HeatSolver(cfg) as s:
        r = s.run()
        return s.gather(), r


@pytest.mark.parametrize("resident", ["1", "0"])
@pytest.mark.parametrize("interval", [20, 50])
def test_device_judged_convergence(gpu, monkeypatch, interval, resident):
    # The residual covers the insulated edge cells.  At 48 x 96 the passes
    # between two ghost fills are one resident span (depth 8), so the checks,
    # the converging one included, sit at even levels inside a span, whose
    # state is replayed from the span's source buffer.
    want, rc = cpu_converged(interval)
    assert rc.converged and rc.converged_at % interval == 0
    monkeypatch.setenv("HEAT_TB_RESIDENT", resident)
    cfg = HeatConfig(nx=48, ny=96, steps=40000, converge=True, check_interval=interval,
                     init="random", seed=3, backend="hip", device=0, insulated="nswe")
    with HeatSolver(cfg) as s:
        r = s.run()
        got = s.gather()
    assert r.converged and r.converged_at == rc.converged_at and r.steps_done == rc.steps_done
    assert np.float32(r.last_resid) == np.float32(rc.last_resid)
    assert (r.resident_passes > 0) == (resident == "1"), r
    assert np.array_equal(bits(got), bits(want)), np.abs(got - want).max()
