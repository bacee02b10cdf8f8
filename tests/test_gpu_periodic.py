"""Periodic (wrap-around) plate edges on the GPU: the ghost-fill kernel's wrap
mode alone, then every kernel family, the resident spans, loopback and RCCL
ranks and the device-judged convergence path, bitwise against the CPU backend
(which tests/test_periodic_cpu.py ties to the exact NumPy oracle).  The stencil
kernels never learn about the option: they see a plate extended into the ghost
ring, which holds the opposite edge of the plate -- a neighbour rank's halo, or
csrc/kernels/ghost_fill.hip's wrap of the rank's own block.  Needs an MI355X."""
import functools

import numpy as np
import pytest
import torch

from parallel_heat_amd import HeatConfig, HeatSolver, ops
from parallel_heat_amd.parallel.group import run_group

from .dist_worker import run_world

pytestmark = pytest.mark.gpu

CHUNKS = (5, 1, 17, 22, 8)  # 53 steps


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# --------------------------------------------------------------------------
# the fill kernel alone
# --------------------------------------------------------------------------
def source(i, n, lo, hi, wrap):
    """Per-axis source of the indices i of an axis of extent n."""
    if wrap:
        return np.where(i < 0, i + n, np.where(i >= n, i - n, i))
    return np.where(lo & (i < 0), -i, np.where(hi & (i >= n), 2 * (n - 1) - i, i))


def fill_expected(full, hx, hy, lx, ly, ins, per, d):
    """The field array after the fill: every cell of the frame
    [-d, lx+d) x [-d, ly+d) takes its per-axis source (wrapped along the axes
    in `per`, reflected across the sides in `ins`); a cell beyond no filled
    side maps to itself, as does everything outside the frame."""
    r = np.arange(-d, lx + d)
    c = np.arange(-d, ly + d)
    sr = source(r, lx, "n" in ins, "s" in ins, "x" in per)
    sc = source(c, ly, "w" in ins, "e" in ins, "y" in per)
    want = full.copy()
    want[(hx + r)[:, None], (hy + c)[None, :]] = full[(hx + sr)[:, None], (hy + sc)[None, :]]
    return want


FILL_MODES = [("x", ""), ("y", ""), ("xy", ""), ("x", "we"), ("y", "n"), ("y", "ns")]


@pytest.mark.parametrize("lx,ly,halo,d", [
    (37, 70, 12, 12),      # the frame as deep as the ring; ly % 4 == 2: unaligned wrap columns
    (37, 70, 12, 1),
    (37, 72, 12, 12),      # whole float4 rows
    (40, 67, 12, 5),       # a frame shallower than the ring: cells beyond it stay
    (300, 1100, 96, 96),   # the deepest halo: several workgroups per side, long rows
])
def test_fill_kernel_wrap_modes(gpu, lx, ly, halo, d):
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
    modes = FILL_MODES if lx < 100 else [("xy", ""), ("x", "e")]
    for per, ins in modes:
        f.data.copy_(torch.from_numpy(start))
        ops.fill_edge_ghosts(f, ins, per, d)
        torch.cuda.synchronize()
        got = f.data.cpu().numpy()
        want = fill_expected(start, f.hx, f.hy, lx, ly, ins, per, d)
        # Targets hold their source; every other cell (the owned block, cells
        # beyond Dirichlet sides only, the padding) is bit-unchanged.
        assert np.array_equal(bits(got), bits(want)), (per, ins)
        # The frame is np.pad's, axis by axis.
        px, py = "x" in per, "y" in per
        n0, n1 = d * (px or "n" in ins), d * (px or "s" in ins)
        w0, w1 = d * (py or "w" in ins), d * (py or "e" in ins)
        pad = np.pad(start[f.hx:f.hx + lx, f.hy:f.hy + ly], ((n0, n1), (0, 0)),
                     mode="wrap" if px else "reflect")
        pad = np.pad(pad, ((0, 0), (w0, w1)), mode="wrap" if py else "reflect")
        frame = got[f.hx - n0:f.hx + lx + n1, f.hy - w0:f.hy + ly + w1]
        assert np.array_equal(bits(frame), bits(pad)), (per, ins)
        # The host twin writes the same bits.
        h = ops.Field(lx, ly, halo, "cpu")
        h.data.copy_(torch.from_numpy(start))
        ops.fill_edge_ghosts(h, ins, per, d)
        assert np.array_equal(bits(h.data.numpy()), bits(got)), (per, ins)


def test_fill_kernel_rejects_bad_arguments(gpu):
    f = ops.Field(10, 20, 4, gpu)
    with pytest.raises(ValueError):
        ops.fill_edge_ghosts(f, "", "x", 5)       # deeper than the ring
    with pytest.raises(ValueError):
        ops.fill_edge_ghosts(f, "", "z", 1)
    with pytest.raises(ValueError, match="wrap"):
        ops.fill_edge_ghosts(ops.Field(3, 20, 4, gpu), "", "x", 4)  # 3 rows cannot lend 4
    with pytest.raises(ValueError, match="axis x"):
        ops.fill_edge_ghosts(f, "s", "x", 1)      # wrapped and mirrored
    with pytest.raises(ValueError, match="axis y"):
        ops.fill_edge_ghosts(f, "w", "xy", 1)
    # A wrapped axis lends its whole extent: 4 rows, depth 4.
    g = ops.Field(4, 20, 4, gpu)
    g.data.copy_(torch.rand(tuple(g.data.shape)))
    before = g.data.cpu().numpy()
    ops.fill_edge_ghosts(g, "", "x", 4)
    torch.cuda.synchronize()
    want = fill_expected(before, g.hx, g.hy, 4, 20, "", "x", 4)
    assert np.array_equal(bits(g.data.cpu().numpy()), bits(want))


# --------------------------------------------------------------------------
# every kernel family, one rank
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cpu_reference(nx, ny, per, ins, steps, seed=3):
    cfg = HeatConfig(nx=nx, ny=ny, steps=steps, init="random", seed=seed, backend="cpu",
                     periodic=per, insulated=ins, tb_depth=1)
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
MODES = [("xy", ""), ("x", ""), ("y", ""), ("y", "n")]


@pytest.mark.parametrize("per,ins", MODES)
@pytest.mark.parametrize("nx,ny", [(203, 517), (150, 300)])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_kernel_families_bitwise(gpu, kernel, nx, ny, per, ins):
    cfg = HeatConfig(nx=nx, ny=ny, steps=0, init="random", seed=3, backend="hip", device=0,
                     periodic=per, insulated=ins, **KERNELS[kernel])
    saved = ops.tb_tuning()
    if kernel == "tile":
        t = ops.tb_tuning()
        t.variant = int(ops.TbVariant.TILE | ops.TbVariant.XCD_GROUPS)
        ops.set_tb_tuning(t)
    try:
        got, rs, info = gpu_run(cfg)
    finally:
        ops.set_tb_tuning(saved)
    want, _ = cpu_reference(nx, ny, per, ins, sum(CHUNKS))
    assert sum(r.steps_done for r in rs) == sum(CHUNKS)
    assert info.periodic == per and info.insulated == ins
    assert info.schedule == "sync" and info.halo >= info.tb_depth
    assert np.array_equal(bits(got), bits(want)), np.abs(got - want).max()


@pytest.mark.parametrize("kernel", ["tb12", "lds3", "auto"])
def test_kernel_families_eager(gpu, kernel):
    cfg = HeatConfig(nx=203, ny=517, steps=0, init="random", seed=3, backend="hip", device=0,
                     periodic="xy", use_graph=False, **KERNELS[kernel])
    got, _, _ = gpu_run(cfg)
    want, _ = cpu_reference(203, 517, "xy", "", sum(CHUNKS))
    assert np.array_equal(bits(got), bits(want))


def test_halo_passes_set_the_ghost_depth(gpu, monkeypatch):
    # One rank with a periodic axis takes the multi-rank halo rule: m passes
    # per ghost fill, from the parameter or HEAT_HALO_PASSES, clamped so that
    # the block holds the wrap sources (its last and first H rows).
    base = HeatConfig(nx=150, ny=300, steps=0, init="random", seed=3, backend="hip", device=0,
                      periodic="xy", kernel="tb", tb_depth=8)
    want, _ = cpu_reference(150, 300, "xy", "", sum(CHUNKS))
    for m, halo in ((1, 8), (3, 24), (40, 144)):  # 150 // 8 = 18 passes at most
        got, rs, info = gpu_run(base.replace(halo_passes=m))
        assert info.halo == halo
        assert np.array_equal(bits(got), bits(want)), m
    monkeypatch.setenv("HEAT_HALO_PASSES", "2")
    got, rs, info = gpu_run(base)
    assert info.halo == 16 and sum(r.exchanges for r in rs) >= sum(CHUNKS) // 16
    assert np.array_equal(bits(got), bits(want))
    # No periodic axis: no ghosts, no fill, whatever is asked.
    with HeatSolver(base.replace(periodic="", halo_passes=3)) as s:
        assert s.info.halo == 8 and s.run(24).exchanges == 0


def test_mpi_numerics_periodic(gpu):
    want = None
    for kernel in ("lds", "naive"):
        cfg = HeatConfig(nx=150, ny=300, steps=0, init="random", seed=3, backend="hip", device=0,
                         periodic="xy", numerics="mpi", kernel=kernel, tb_depth=2)
        got, _, _ = gpu_run(cfg)
        if want is None:
            with HeatSolver(cfg.replace(backend="cpu", tb_depth=1)) as c:
                c.run(sum(CHUNKS))
                want = c.gather()
        assert np.array_equal(bits(got), bits(want)), kernel


def test_mfma_periodic_within_bound(gpu):
    steps = sum(CHUNKS)
    cfg = HeatConfig(nx=150, ny=300, steps=0, init="random", seed=3, backend="hip", device=0,
                     periodic="xy", kernel="mfma", tb_depth=4)
    got, _, _ = gpu_run(cfg)
    want, _ = cpu_reference(150, 300, "xy", "", steps)
    dev = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    print(f"mfma, periodic, {steps} steps: max |got - oracle| = {dev:.3e} "
          f"(bound {steps * 2e-5:.1e})")
    # The bound of tests/test_gpu_coefficients_solver.py: one mfma step is
    # within 2e-5 of the exact one on [0, 100) data, and the periodic step is
    # a convex combination too, so the errors of n steps add up to at most
    # n * 2e-5.
    assert dev <= steps * 2e-5


# --------------------------------------------------------------------------
# resident spans
# --------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny,per", [(700, 300, "xy"), (203, 517, "xy"), (700, 300, "x")])
def test_resident_spans_bitwise(gpu, monkeypatch, nx, ny, per):
    cfg = HeatConfig(nx=nx, ny=ny, steps=0, init="random", seed=3, backend="hip", device=0,
                     periodic=per)
    want, _ = cpu_reference(nx, ny, per, "", 96)
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
    "2rows": (2, dict(decomp="rows")),   # periodic x: north and south are one peer
    "1x2": (2, dict(px=1, py=2)),
    "3rows": (3, dict(decomp="rows")),
    "4auto": (4, dict(decomp="auto")),   # 2 x 2: periodic xy makes all four diagonals one peer
}


def group_run(cfg, world):
    def fn(s):
        for n in CHUNKS:
            s.run(n)
        return s.gather(), s.checksum(), s.info
    out = run_group(cfg, world, fn)
    grid = next(g for g, _, _ in out if g is not None)
    return grid, [c for _, c, _ in out], [i for _, _, i in out]


@pytest.mark.parametrize("per,ins", [("xy", ""), ("x", "w")])
@pytest.mark.parametrize("halo_passes", [0, 1, 2, 3])
@pytest.mark.parametrize("world", list(WORLDS))
def test_loopback_ranks_bitwise(gpu, world, halo_passes, per, ins):
    n, kw = WORLDS[world]
    cfg = HeatConfig(nx=150, ny=300, steps=0, init="random", seed=3, backend="hip", device=0,
                     periodic=per, insulated=ins, tb_depth=8, halo_passes=halo_passes, **kw)
    grid, sums, infos = group_run(cfg, n)
    want, cs = cpu_reference(150, 300, per, ins, sum(CHUNKS))
    assert np.array_equal(bits(grid), bits(want)), np.abs(grid - want).max()
    assert all(c["hash"] == cs["hash"] and c["count"] == cs["count"] for c in sums)
    assert len({i.halo for i in infos}) == 1  # every rank took the same ghost depth
    if halo_passes:
        assert infos[0].halo == 8 * halo_passes


def test_loopback_overlap_falls_back_to_sync(gpu):
    cfg = HeatConfig(nx=150, ny=300, steps=0, init="random", seed=3, backend="hip", device=0,
                     periodic="xy", tb_depth=8, schedule="overlap", decomp="rows")
    grid, sums, infos = group_run(cfg, 2)
    assert all(i.schedule == "sync" for i in infos)
    want, cs = cpu_reference(150, 300, "xy", "", sum(CHUNKS))
    assert np.array_equal(bits(grid), bits(want))
    assert all(c["hash"] == cs["hash"] for c in sums)
    # Without a periodic axis the schedule is kept.
    out = run_group(cfg.replace(periodic=""), 2, lambda s: s.info.schedule)
    assert out == ["overlap", "overlap"]


# --------------------------------------------------------------------------
# device-judged convergence
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cpu_converged(interval):
    cfg = HeatConfig(nx=48, ny=96, steps=40000, converge=True, check_interval=interval,
                     init="random", seed=3, backend="cpu", periodic="x", tb_depth=1)
    with HeatSolver(cfg) as s:
        r = s.run()
        return s.gather(), r


@pytest.mark.parametrize("resident", ["1", "0"])
@pytest.mark.parametrize("interval", [20, 50])
def test_device_judged_convergence(gpu, monkeypatch, interval, resident):
    # The residual covers the edge rows of the periodic axis.
    want, rc = cpu_converged(interval)
    assert rc.converged and rc.converged_at % interval == 0
    monkeypatch.setenv("HEAT_TB_RESIDENT", resident)
    cfg = HeatConfig(nx=48, ny=96, steps=40000, converge=True, check_interval=interval,
                     init="random", seed=3, backend="hip", device=0, periodic="x")
    with HeatSolver(cfg) as s:
        r = s.run()
        got = s.gather()
    assert r.converged and r.converged_at == rc.converged_at and r.steps_done == rc.steps_done
    assert np.float32(r.last_resid) == np.float32(rc.last_resid)
    assert (r.resident_passes > 0) == (resident == "1"), r
    assert np.array_equal(bits(got), bits(want)), np.abs(got - want).max()


# --------------------------------------------------------------------------
# RCCL, two processes on the one GPU
# --------------------------------------------------------------------------
def test_rccl_two_ranks_same_peer(gpu, tmp_path):
    # Rows on a periodic x axis: both messages of a rank go to the one peer,
    # inside one grouped send / receive.
    base = dict(nx=150, ny=300, steps=0, init="random", seed=3, backend="hip", tb_depth=8,
                periodic="x", decomp="rows")
    res = run_world(2, base, 0, tmp_path, transport="rccl", chunks=list(CHUNKS))
    with HeatSolver(HeatConfig(**{**base, "decomp": "auto"})) as s:
        s.run(sum(CHUNKS))
        want, h = s.gather(), s.checksum()["hash"]
    assert int(res["done"]) == sum(CHUNKS)
    assert np.array_equal(bits(res["grid"]), bits(want))
    assert str(res["hash"]) == h
    ref, _ = cpu_reference(150, 300, "x", "", sum(CHUNKS))
    assert np.array_equal(bits(want), bits(ref))
