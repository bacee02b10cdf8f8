"""Coverage of the residual (`max |new - old|`) without a GPU: the hot-cell
oracle of tests/hot_cell.py on its own, then the CPU backend swept with it.

The rest of the suite checks the residual's VALUE on random data, where the
maximum sits in one arbitrary cell per seed; a residual that leaves out one
row per thread, or reads one cell past its box, passes.  Here one hot cell q
visits every cell in turn and holds the maximum wherever it is (unique, the
runner-up at most 2/3 of it), so a dropped or an extra cell changes the fp32
word the comparison is made on.  Every comparison is exact."""
import numpy as np
import pytest
import torch

from parallel_heat_amd import HeatConfig, HeatSolver, ops

from . import hot_cell as Hc

EDGES = [("", ""), ("all", ""), ("", "xy"), ("ns", "y")]   # (insulated, periodic)


def _updated(shape, q, ins, per):
    """Is q an updated cell (not on a fixed side of the plate)?"""
    ins = "nswe" if ins == "all" else ins
    fixed_r = (q[0] == 0 and "n" not in ins and "x" not in per) or \
              (q[0] == shape[0] - 1 and "s" not in ins and "x" not in per)
    fixed_c = (q[1] == 0 and "w" not in ins and "y" not in per) or \
              (q[1] == shape[1] - 1 and "e" not in ins and "y" not in per)
    return not (fixed_r or fixed_c)


# --------------------------------------------------------------------------
# the oracle alone
# --------------------------------------------------------------------------
NEAR = [0, 1, 2, 20, 37, 38, 39]   # at, next to and two from each edge; far inside


@pytest.mark.parametrize("ins,per", EDGES)
@pytest.mark.parametrize("coef", [Hc.COEF, Hc.SWAPPED])
def test_window_equals_full_plate(ins, per, coef):
    # All four corners, the cells next to them, edge cells and a far interior
    # cell; on a plate larger than the window (cut sides) and one it covers.
    n = 12
    for shape in [(40, 40), (61, 47), (25, 61)]:
        nx, ny = shape
        pos = [(r, c) for r in (0, 1, nx // 2, nx - 2, nx - 1)
               for c in (0, 1, ny // 2, ny - 2, ny - 1)] + [(nx // 2 + 3, 14)]
        for q in pos:
            full = Hc.full_deltas(nx, ny, q, n, coef, ins, per)
            ri, ci, win, _ = Hc.window(shape, q, n, coef, ins, per)
            for k in range(n):
                assert np.array_equal(Hc.bits(win[k]), Hc.bits(full[k][np.ix_(ri, ci)])), (q, k)
                rest = np.array(full[k])
                rest[np.ix_(ri, ci)] = 0
                assert not rest.any(), (q, k)      # nothing moved outside the window
            box = (3, nx - 5, 2, ny - 1)
            want = [np.float32(d[box[0]:box[1], box[2]:box[3]].max()) for d in full]
            assert np.array_equal(Hc.bits(Hc.resid_levels(shape, q, box, n, coef, ins, per)),
                                  Hc.bits(want)), q


def test_window_mpi_numerics_equals_full_plate():
    for q in [(1, 1), (20, 20), (38, 1)]:
        full = Hc.full_deltas(40, 40, q, 1, numerics="mpi")
        got = Hc.resid_levels((40, 40), q, (0, 40, 0, 40), 1, numerics="mpi")
        assert Hc.bits(got)[0] == Hc.bits(full[0].max())


@pytest.mark.parametrize("ins,per", EDGES)
@pytest.mark.parametrize("coef", [Hc.COEF, Hc.SWAPPED])
def test_preconditions_hold_on_the_reference(ins, per, coef):
    # Every position class the sweeps use (q at, next to and away from every
    # edge and corner), 40 steps: the solver sweeps check steps up to 2 x 20.
    # The argmax is q, alone; the runner-up stays below (at most 1/3 of the
    # max with fixed or periodic edges, 2/3 with q on an insulated edge); the
    # levels are pairwise distinct.  A fixed side's cells are never updated:
    # q there is no residual cell (the sweeps still compare its neighbours'
    # values with the oracle, as they do for q outside the box).
    shape, worst = (40, 40), 0.0
    for q in [(r, c) for r in NEAR for c in NEAR]:
        if _updated(shape, q, ins, per):
            worst = max(worst, Hc.preconditions(shape, q, (0, 40, 0, 40), 40, coef=coef,
                                                insulated=ins, periodic=per))
    print(f"worst runner-up / max, insulated={ins!r} periodic={per!r} coef={coef}: {worst:.4f}")
    assert worst <= (2 / 3 if ins else 1 / 3) + 1e-6


def test_levels_of_a_pass_are_the_measured_ones():
    got = Hc.resid_levels((40, 40), (20, 20), (0, 40, 0, 40), 12)
    assert [f"{v:.6f}" for v in got[:3]] == ["0.867188", "0.841217", "0.816124"]
    assert len(set(got.tolist())) == 12 and np.all(np.diff(got) < 0)


def test_q_outside_the_box_gives_the_neighbours_value():
    # One cell outside the box: the box's max is the neighbour's cx*h or cy*h
    # at step 1, far below what a residual that looks one cell too far sees.
    box = (10, 30, 10, 30)
    inside = Hc.resid_levels((40, 40), (10, 20), box, 1)[0]
    above = Hc.resid_levels((40, 40), (9, 20), box, 1)[0]
    left = Hc.resid_levels((40, 40), (20, 9), box, 1)[0]
    assert above == np.float32(37.0 / 256) and left == np.float32(37.0 / 128)
    assert inside == 3 * left == 6 * above      # 1 - 2 cx - 2 cy = 3 cy = 6 cx
    assert Hc.resid_levels((40, 40), (8, 20), box, 1)[0] == 0


# --------------------------------------------------------------------------
# the CPU backend, single step
# --------------------------------------------------------------------------
def _cpu_sweep(shape, block, positions, box=None):
    """ops.naive_step on CPU fields for the hot cell at each of `positions`
    (plate coordinates): the residual words."""
    nx, ny = shape
    ox, oy, lx, ly = block
    g = ops.Geom(nx=nx, ny=ny, gx0=ox, gy0=oy, cx=Hc.COEF[0], cy=Hc.COEF[1])
    a, b = ops.Field(lx, ly, 2, "cpu", fill=float(Hc.C)), ops.Field(lx, ly, 2, "cpu")
    got = np.zeros(len(positions), np.float32)
    for i, (r, c) in enumerate(positions):
        cell = a.view(r - ox, r - ox + 1, c - oy, c - oy + 1)
        cell.fill_(float(Hc.C + Hc.H))
        resid = torch.zeros(1, dtype=torch.int32)
        ops.naive_step(a, b, g, box, resid=resid)
        got[i] = ops.resid_value(resid)
        cell.fill_(float(Hc.C))
    return got


def test_cpu_step_every_cell_of_a_plate():
    shape = (37, 53)
    pos = [(r, c) for r in range(37) for c in range(53)]
    want = Hc.resid_table(shape, pos, (0, 37, 0, 53), 1)[:, 0]
    Hc.assert_words(_cpu_sweep(shape, (0, 0, 37, 53), pos), want, pos, "cpu naive_step, plate")


def test_cpu_step_every_cell_of_a_block_and_its_ghosts():
    # A block inside a larger plate, q also in the two ghost rows and columns
    # around it (valid cells the residual must not count), and a sub-box.
    shape, block = (40, 60), (5, 8, 20, 30)
    ox, oy, lx, ly = block
    pos = [(r, c) for r in range(ox - 2, ox + lx + 2) for c in range(oy - 2, oy + ly + 2)]
    want = Hc.resid_table(shape, pos, (ox, ox + lx, oy, oy + ly), 1)[:, 0]
    Hc.assert_words(_cpu_sweep(shape, block, pos), want, pos, "cpu naive_step, block")
    sub = (3, 11, 4, 17)
    want = Hc.resid_table(shape, pos, (ox + 3, ox + 11, oy + 4, oy + 17), 1)[:, 0]
    Hc.assert_words(_cpu_sweep(shape, block, pos, sub), want, pos, "cpu naive_step, sub-box")


# --------------------------------------------------------------------------
# the CPU solver
# --------------------------------------------------------------------------
def solver_sweep(cfg, positions, interval, runs=2, make=HeatSolver):
    """last_resid after each of `runs` run(interval) calls, per position: one
    solver, the hot-cell plate scattered anew for every position."""
    got = np.zeros((len(positions), runs), np.float32)
    with make(cfg.replace(check_interval=interval)) as s:
        for i, q in enumerate(positions):
            s.scatter(Hc.plate(cfg.nx, cfg.ny, q))
            for k in range(runs):
                got[i, k] = s.run(interval).last_resid
    return got


def solver_want(cfg, positions, interval, runs=2):
    lv = Hc.resid_table((cfg.nx, cfg.ny), positions, (0, cfg.nx, 0, cfg.ny), runs * interval,
                        coef=(cfg.cx, cfg.cy), insulated=cfg.insulated, periodic=cfg.periodic)
    return lv[:, interval - 1::interval]


def edge_positions(nx, ny):
    """Each edge row and column, each corner, the cells next to them, one
    cell inside."""
    rr, cc = (0, 1, nx // 2, nx - 2, nx - 1), (0, 1, ny // 2, ny - 2, ny - 1)
    return [(r, c) for r in rr for c in cc]


def _cfg(nx, ny, **kw):
    return HeatConfig(nx=nx, ny=ny, steps=0, converge=True, eps=0.0, init="zero", backend="cpu",
                      threads=4, tb_depth=1, cx=Hc.COEF[0], cy=Hc.COEF[1], **kw)


@pytest.mark.parametrize("interval", [1, 5])
def test_cpu_solver_every_row_holds_the_max(interval):
    # q down one column through every row (every OpenMP thread's first and
    # last row holds the max once), and along one row through every column.
    cfg = _cfg(37, 53)
    pos = [(r, 7) for r in range(37)] + [(18, c) for c in range(53)]
    got, want = solver_sweep(cfg, pos, interval), solver_want(cfg, pos, interval)
    for k in range(2):
        Hc.assert_words(got[:, k], want[:, k], pos, f"cpu solver, check {k + 1}")


@pytest.mark.parametrize("ins,per", EDGES[1:])
def test_cpu_solver_edges(ins, per):
    # The residual covers updated edge cells: q on the edge rows, edge
    # columns and corners of insulated and periodic plates.
    cfg = _cfg(37, 53, insulated=ins, periodic=per)
    pos = edge_positions(37, 53) + [(r, 0) for r in range(37)] + [(0, c) for c in range(53)]
    got, want = solver_sweep(cfg, pos, 3), solver_want(cfg, pos, 3)
    for k in range(2):
        Hc.assert_words(got[:, k], want[:, k], pos, f"cpu solver {ins!r} {per!r}, check {k + 1}")
