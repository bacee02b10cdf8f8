"""Coverage of the residual the SOLVER reports (`last_resid`): the hot cell
of tests/hot_cell.py in the first and last owned rows and columns, at the
tile-wave boundaries of forced resident shapes, on both sides of the ranks'
seams and on updated plate edges; after run(interval), after a second
run(interval) and, from a fresh plate, after one run(2 * interval) whose
passes form a resident span.  Exact against the oracle and the CPU backend;
in a group every rank must report the same word (the maximum lives in one
rank and has to survive the all-reduce).  Needs an MI355X."""
import functools

import numpy as np
import pytest

from parallel_heat_amd import HeatConfig, HeatSolver, ops
from parallel_heat_amd.parallel.group import run_group

from . import hot_cell as Hc
from .test_residual_coverage_cpu import edge_positions

pytestmark = pytest.mark.gpu

INTERVALS = [5, 7, 10, 12, 20]
N = 40   # steps of the oracle's tables: 2 x the longest interval


def _cfg(nx, ny, interval, backend="hip", **kw):
    kw.setdefault("tb_depth", 12 if backend == "hip" else 1)
    return HeatConfig(nx=nx, ny=ny, steps=0, converge=True, eps=0.0, check_interval=interval,
                      init="zero", backend=backend, cx=Hc.COEF[0], cy=Hc.COEF[1], **kw)


@functools.lru_cache(maxsize=None)
def _oracle(nx, ny, positions, ins="", per="", n=N):
    t = Hc.resid_table((nx, ny), positions, (0, nx, 0, ny), n, insulated=ins, periodic=per)
    t.setflags(write=False)
    return t


def _phases(s, nx, ny, positions, interval):
    """Per position: last_resid after run(interval), after a second one, and
    after one run(2 * interval) from a fresh plate; the resident passes of
    the last."""
    got, res = np.zeros((len(positions), 3), np.float32), 0
    root = s.rank == 0
    for i, q in enumerate(positions):
        s.scatter(Hc.plate(nx, ny, q) if root else None)
        got[i, 0] = s.run(interval).last_resid
        got[i, 1] = s.run(interval).last_resid
        s.scatter(Hc.plate(nx, ny, q) if root else None)
        r = s.run(2 * interval)
        got[i, 2], res = r.last_resid, res + r.resident_passes
    return got, res


@functools.lru_cache(maxsize=None)
def _cpu(nx, ny, positions, interval, ins="", per=""):
    with HeatSolver(_cfg(nx, ny, interval, "cpu", threads=4, insulated=ins, periodic=per)) as s:
        return _phases(s, nx, ny, positions, interval)[0]


def _compare(got, nx, ny, positions, interval, what, ins="", per="", cpu=True):
    lv = _oracle(nx, ny, positions, ins, per, max(N, 2 * interval))
    want = np.stack([lv[:, interval - 1], lv[:, 2 * interval - 1], lv[:, 2 * interval - 1]], 1)
    for k, name in enumerate(("run 1", "run 2", "one run of both")):
        Hc.assert_words(got[:, k], want[:, k], positions, f"{what}, every {interval}, {name}")
    if cpu:
        ref = _cpu(nx, ny, positions, interval, ins, per)
        for k in range(3):
            Hc.assert_words(got[:, k], ref[:, k], positions, f"{what} vs cpu, every {interval}")


def _plate_positions(nx, ny):
    """First and last owned rows and columns (the ring and the first updated
    cells), both sides of the wave and tile boundaries of 12- and 20-row
    waves (12 x 8: 96-row tiles; 20 x 16: 320-row), in the first and in the
    second strip."""
    rows = [0, 1, 11, 12, 19, 20, 95, 96, 191, 192, 199, 200, nx - 2, nx - 1]
    rows = sorted({r for r in rows if r < nx})
    cols = [c for c in (100, 300) if c < ny - 1] or [ny // 2]
    pos = [(r, c) for r in rows for c in cols]
    pos += [(nx // 2, c) for c in (0, 1, 2, 3, 4, ny - 5, ny - 4, ny - 3, ny - 2, ny - 1)]
    return tuple(dict.fromkeys(pos))


@pytest.fixture
def res_shape():
    saved = ops.tb_tuning()

    def set_(rows, waves):
        t = ops.tb_tuning()
        t.tile_rows, t.tile_waves = rows, waves
        ops.set_tb_tuning(t)
    yield set_
    ops.set_tb_tuning(saved)


@pytest.mark.parametrize("nx,ny,resident,graph,tile", [
    (203, 517, 1, True, None), (203, 517, 1, False, None),
    (203, 517, 0, True, None), (203, 517, 0, False, None),
    (203, 517, 1, True, (12, 8)), (203, 517, 1, False, (12, 8)), (203, 517, 1, True, (20, 16)),
    (40, 70, 1, True, None), (40, 70, 1, False, None),
    (40, 70, 0, True, None), (40, 70, 0, False, None),
])
def test_single_rank(gpu, monkeypatch, res_shape, nx, ny, resident, graph, tile):
    # Depth 12: every 5 / 7 / 10 steps inner levels, every 12 pass ends,
    # every 20 a second pass.  Resident spans are two or more passes of one
    # even depth whose checks sit at even levels (Solver::resident_span), and
    # only the one run of 2 x interval steps has more than one pass:
    #   every 12: 24 = 12 + 12, checks at level 12 of both: a span;
    #   every 20: 40 = 12 + 12 + 8 + 8, checks at level 8 of the 2nd and of
    #             the 4th pass: two spans, the reported check inside the 2nd;
    #   every 10: 20 = 12 + 8 (checks at levels 10 and 8): two passes of
    #             different depths, no span can form;
    #   every 5, 7: checks at odd levels cut the passes, no span.
    monkeypatch.setenv("HEAT_TB_RESIDENT", str(resident))
    if tile:
        res_shape(*tile)
    pos = _plate_positions(nx, ny)
    for interval in INTERVALS:
        with HeatSolver(_cfg(nx, ny, interval, use_graph=graph)) as s:
            assert s.info.tb_depth == 12
            got, res = _phases(s, nx, ny, pos, interval)
        assert (res > 0) == (bool(resident) and interval in (12, 20)), (interval, res)
        _compare(got, nx, ny, pos, interval, f"{nx} x {ny} resident {resident} graph {graph}")


@pytest.mark.parametrize("ins,per", [("all", ""), ("", "xy"), ("ns", "y")])
@pytest.mark.parametrize("resident", [1, 0])
def test_insulated_and_periodic_edges(gpu, monkeypatch, ins, per, resident):
    # The residual covers updated edge cells: q on each edge row, edge column
    # and corner, next to them, and one cell inside.  Every 12 steps the run
    # of 24 is two depth-12 passes behind one fill of the (at least 24 deep)
    # ghost frame: a resident span; every 7 the checks cut the passes.
    monkeypatch.setenv("HEAT_TB_RESIDENT", str(resident))
    nx, ny = 203, 517
    pos = tuple(edge_positions(nx, ny))
    for interval in (7, 12):
        with HeatSolver(_cfg(nx, ny, interval, insulated=ins, periodic=per)) as s:
            got, res = _phases(s, nx, ny, pos, interval)
        assert (res > 0) == (bool(resident) and interval == 12), (interval, res)
        _compare(got, nx, ny, pos, interval, f"insulated {ins!r} periodic {per!r}", ins, per)


def _group_phases(s, nx, ny, positions, interval):
    """As _phases, the one run 6 x interval steps long."""
    got, res = np.zeros((len(positions), 3), np.float32), 0
    for i, q in enumerate(positions):
        s.scatter(Hc.plate(nx, ny, q) if s.rank == 0 else None)
        got[i, 0] = s.run(interval).last_resid
        got[i, 1] = s.run(interval).last_resid
        s.scatter(Hc.plate(nx, ny, q) if s.rank == 0 else None)
        r = s.run(6 * interval)
        got[i, 2], res = r.last_resid, res + r.resident_passes
    return got, res


@functools.lru_cache(maxsize=None)
def _cpu_group(nx, ny, positions, interval):
    with HeatSolver(_cfg(nx, ny, interval, "cpu", threads=8)) as s:
        return _group_phases(s, nx, ny, positions, interval)[0]


@pytest.mark.parametrize("schedule", ["sync", "overlap"])
@pytest.mark.parametrize("world,kw", [
    (2, dict(decomp="rows")),
    (4, dict(px=2, py=2)),
])
def test_loopback_groups(gpu, monkeypatch, world, kw, schedule):
    # 1024 x 1024 (the plate test_resident_span_converges_inside's groups go
    # resident on), the default depth of its 512-row blocks, checks every 8
    # steps.  q in the last owned row of rank 0, the first of rank 1, the
    # four cells around the 2 x 2 corner, the rows next to them, and both sides of the
    # seams between the overlap schedule's boundary bands (8 deep) and its
    # interior.  The sync schedule's passes between two exchanges must form
    # resident spans (the overlap schedule plans none).  Also against the CPU
    # backend on one rank.
    monkeypatch.setenv("HEAT_TB_RESIDENT", "2")
    nx = ny = 1024
    interval = 8
    pos = tuple((r, c) for r in (510, 511, 512, 513) for c in (300, 511, 512))
    pos += tuple((r, c) for r in (503, 504, 519, 520) for c in (300, 504, 519))
    cfg = _cfg(nx, ny, interval, tb_depth=0, schedule=schedule, **kw)

    out = run_group(cfg, world, lambda s: _group_phases(s, nx, ny, pos, interval))
    if schedule == "sync":
        assert all(res > 0 for _, res in out), [res for _, res in out]
    lv = _oracle(nx, ny, pos, n=6 * interval)
    want = np.stack([lv[:, interval - 1], lv[:, 2 * interval - 1], lv[:, 6 * interval - 1]], 1)
    for rank, (got, _) in enumerate(out):
        for k in range(3):
            Hc.assert_words(got[:, k], want[:, k], pos, f"rank {rank} of {world}, phase {k}")
    ref = _cpu_group(nx, ny, pos, interval)
    for k in range(3):
        Hc.assert_words(out[0][0][:, k], ref[:, k], pos, f"{world} ranks vs cpu, phase {k}")
