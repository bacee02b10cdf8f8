"""Scenarios, oracle and precondition checks shared by the lifecycle tests (CPU
and GPU): replace or inspect the state of a solver that has ALREADY RUN, then
continue, and compare with the NumPy oracle.

A solver that has stepped carries state no kernel test sees: the buffer
parity, the valid ghost depth per axis (GhostState, plan.hpp), cached segment
graphs keyed by both, a device gate a converging check closed, a pending
enqueued run.  `load`, `scatter`, `load_local`, `refine` and `reset` must leave
it as a fresh solver holding the new state at the new step: the next run
re-exchanges and refills every ghost (neighbours' halos, the mirror frame of
insulated edges, the wrap frame of periodic ones) and places its checks at the
new absolute steps.

The oracle is `reference.step_np_fma` / `step_np_mpi` only (never the CPU
backend, which shares solver.cpp with the code under test).  Equality is
bitwise; the only tolerance is the fp64 summation-order bound of the checksum
and coarse sums (coarse_cases.assert_within_bound: derived, not measured).

Two unrelated data sets, so that a stale ghost or cell cannot go unnoticed:
state A is the engine's own `init="random"` advanced n1 steps (what the solver
holds before the replacement), state B (and C, the third state of a second
replacement) is `oracle_cases.values("signed", ...)` in [-100, 100); the
coefficients are anisotropic.  `check_preconditions` asserts on the oracle
alone that A and B differ in every cell a ghost could come from and that a
stale ghost at any seam or filled edge changes the next step."""
import functools
import math
from typing import NamedTuple, Optional

import numpy as np

from parallel_heat_amd.models import reference as R

from . import coarse_cases as CC
from .oracle_cases import ANISO, assert_bitwise, bits, values

SEED_A, SEED_B, SEED_C, SEED_R = 21, 8, 13, 31   # unrelated streams: no cell in common
REFINE_F = (4, 8)       # refine(): factors of the coarse source grid
COARSE_F = (64, 128)    # coarse(): few coarse cells, partial last ones on every plate here
S0, S0_ALT = 25, 33     # steps given to a replacement: multiples of no depth or interval used


class Plate(NamedTuple):
    nx: int
    ny: int
    insulated: str = ""
    periodic: str = ""
    numerics: str = "fma"   # the oracle's: "fma" (engine default) or "mpi"
    cx: float = ANISO[0]
    cy: float = ANISO[1]
    seed: int = SEED_A


def _frozen(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a, np.float32)
    a.setflags(write=False)
    return a


def step_fn(plate: Plate):
    f = {"fma": R.step_np_fma, "mpi": R.step_np_mpi}[plate.numerics]
    return lambda u: f(u, plate.cx, plate.cy, plate.insulated, plate.periodic)


def refine_source(plate: Plate) -> np.ndarray:
    fx, fy = REFINE_F
    return values("signed", -(-plate.nx // fx), -(-plate.ny // fy), SEED_R)


def start_state(plate: Plate, kind: str) -> np.ndarray:
    """A: the engine's random initial condition; B, C: unrelated signed sets;
    R0, R1: refine_np of the signed source (order 0 / 1); U: all 1.0."""
    nx, ny = plate.nx, plate.ny
    if kind == "A":
        return _frozen(R.init_grid(nx, ny, "random", plate.seed))
    if kind in ("B", "C"):
        return values("signed", nx, ny, SEED_B if kind == "B" else SEED_C)
    if kind in ("R0", "R1"):
        return _frozen(R.refine_np(refine_source(plate), nx, ny, *REFINE_F, int(kind[1]),
                                   plate.periodic))
    if kind == "U":
        return _frozen(np.ones((nx, ny), np.float32))
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def _trajectory(plate: Plate, kind: str) -> list:
    """The (growing) list of oracle states from start_state(plate, kind): one
    per (plate, data, coefficients, edges), shared by every test of a session.
    Extended by state() on the main thread only."""
    return [start_state(plate, kind)]


def state(plate: Plate, kind: str, k: int) -> np.ndarray:
    lv = _trajectory(plate, kind)
    step = step_fn(plate)
    while len(lv) <= k:
        lv.append(_frozen(step(lv[-1])))
    return lv[k]


def is_check_step(k: int, interval: int, compat: str) -> bool:
    """Solver::is_check_point: a check follows completed step k."""
    return k >= 1 and ((k - 1) % interval == 0 if compat == "cuda" else k % interval == 0)


class Continued(NamedTuple):
    grid: np.ndarray
    steps_done: int
    converged_at: int
    checks: int
    last_resid: float


def continue_full(u, step0: int, n: int, *, cx: float = 0.1, cy: float = 0.1,
                  converge: bool = False, check_interval: int = 20, eps: float = 1e-3,
                  compat: str = "none", insulated: str = "", periodic: str = "",
                  numerics: str = "fma") -> Continued:
    """n more steps of a run that stands at the ABSOLUTE step `step0`, checks
    at the absolute steps Solver::is_check_point uses (k % C == 0, compat cuda:
    (k - 1) % C == 0), the residual max |u' - u| in float32 over the plate (a
    fixed cell contributes 0), converged when r < float32(eps) (compat mpi:
    r <= eps in double).  reference.run_np always starts at step 0 and cannot
    predict a resumed run."""
    step = {"fma": R.step_np_fma, "mpi": R.step_np_mpi}[numerics]
    u = np.array(u, np.float32)
    checks, last = 0, 0.0
    for k in range(step0 + 1, step0 + n + 1):
        v = step(u, cx, cy, insulated, periodic)
        if converge and is_check_step(k, check_interval, compat):
            r = np.float32(np.max(np.abs(v - u))) if v.size else np.float32(0)
            checks += 1
            last = float(r)
            if (float(r) <= eps) if compat == "mpi" else (r < np.float32(eps)):
                return Continued(v, k - step0, k, checks, last)
        u = v
    return Continued(u, n, -1, checks, last)


def continue_np(u, step0: int, n: int, **kw):
    """(grid, steps_done, converged_at or -1) of continue_full."""
    c = continue_full(u, step0, n, **kw)
    return c.grid, c.steps_done, c.converged_at


def check_steps_between(lo: int, hi: int, interval: int, compat: str) -> list:
    """The check steps k with lo < k <= hi."""
    return [k for k in range(lo + 1, hi + 1) if is_check_step(k, interval, compat)]


# -- decomposition, bands, preconditions ----------------------------------------------------

def blocks(plate: Plate, px: int, py: int):
    """[(ox, lx, oy, ly)] in rank order (row-major process grid)."""
    return [(ox, lx, oy, ly) for ox, lx in CC.block_spans(plate.nx, px)
            for oy, ly in CC.block_spans(plate.ny, py)]


def _filled(plate: Plate) -> str:
    """The plate sides whose ghost frame the solver fills: letters of "nswe"."""
    ins = R.insulated_sides(plate.insulated)
    per = R.periodic_axes(plate.periodic)
    return "".join(c for c, ax in zip("nswe", "xxyy") if c in ins or ax in per)


def ghosted(plate: Plate, px: int, py: int) -> bool:
    return px * py > 1 or bool(_filled(plate))


def active_axes(plate: Plate, px: int, py: int):
    """(ns, ew): the axis has ghosts to keep valid (plan.hpp Sides)."""
    f = _filled(plate)
    return px > 1 or "n" in f or "s" in f, py > 1 or "w" in f or "e" in f


def ghost_band(plate: Plate, px: int, py: int, H: int) -> np.ndarray:
    """Cells within H of a block seam or of a filled plate edge: every cell a
    ghost of depth H is a copy of."""
    nx, ny = plate.nx, plate.ny
    m = np.zeros((nx, ny), bool)
    for ox, _ in CC.block_spans(nx, px)[1:]:
        m[max(0, ox - H):ox + H, :] = True
    for oy, _ in CC.block_spans(ny, py)[1:]:
        m[:, max(0, oy - H):oy + H] = True
    f = _filled(plate)
    if "n" in f:
        m[:H + 1, :] = True
    if "s" in f:
        m[nx - H - 1:, :] = True
    if "w" in f:
        m[:, :H + 1] = True
    if "e" in f:
        m[:, ny - H - 1:] = True
    return m


def _fixed_cells(plate: Plate) -> np.ndarray:
    """Cells no step changes: the ring along the Dirichlet sides."""
    f = _filled(plate)
    m = np.zeros((plate.nx, plate.ny), bool)
    if "n" not in f:
        m[0, :] = True
    if "s" not in f:
        m[-1, :] = True
    if "w" not in f:
        m[:, 0] = True
    if "e" not in f:
        m[:, -1] = True
    return m


def _pad(u, plate: Plate):
    """u with a one-cell frame beyond every filled side (mirror across an
    insulated edge row, the other end of a periodic axis), built here from
    slices (not from the oracle's own padding), and the frame widths."""
    ins, per = R.insulated_sides(plate.insulated), R.periodic_axes(plate.periodic)
    n0 = int("n" in ins or "x" in per)
    n1 = int("s" in ins or "x" in per)
    w0 = int("w" in ins or "y" in per)
    w1 = int("e" in ins or "y" in per)
    rows = ([u[-1:] if "x" in per else u[1:2]] if n0 else []) + [u] + \
           ([u[:1] if "x" in per else u[-2:-1]] if n1 else [])
    p = np.concatenate(rows, 0)
    cols = ([p[:, -1:] if "y" in per else p[:, 1:2]] if w0 else []) + [p] + \
           ([p[:, :1] if "y" in per else p[:, -2:-1]] if w1 else [])
    return np.concatenate(cols, 1), (n0, n1, w0, w1)


_CHECKED = {}


def check_preconditions(plate: Plate, px: int, py: int, H: int, old: np.ndarray,
                        new: np.ndarray, shared_ring: bool = False) -> None:
    """_preconditions, once per pair of oracle states and decomposition (a
    failure is not remembered: it fails every case that meets it)."""
    key = (plate, px, py, H, id(old), id(new), shared_ring)
    hit = _CHECKED.get(key)
    if hit is None or hit[0] is not old or hit[1] is not new:
        _preconditions(plate, px, py, H, old, new, shared_ring)
        _CHECKED[key] = (old, new)


def _preconditions(plate: Plate, px: int, py: int, H: int, old: np.ndarray,
                   new: np.ndarray, shared_ring: bool = False) -> None:
    """On the oracle alone: `old` (what the solver held) and `new` (what it is
    given) differ bitwise in every cell a ghost can be a copy of, and for each
    seam and each filled edge one oracle step of `new` differs from one step
    of `new` with that seam's or edge's neighbour cells taken from `old`: a
    stale ghost moves a result.  shared_ring: reset() returns to the state the
    run started from, whose Dirichlet ring no step ever changed; those fixed
    cells are equal by construction and leave the comparison."""
    band = ghost_band(plate, px, py, H)
    if shared_ring:
        band &= ~_fixed_cells(plate)
    if ghosted(plate, px, py):
        assert band.any()
    same = (bits(old) == bits(new)) & band
    assert not same.any(), ("old and new state share cells near a seam or edge",
                            np.argwhere(same)[:8])
    plain = Plate(plate.nx, plate.ny, numerics=plate.numerics, cx=plate.cx, cy=plate.cy)
    want = step_fn(plate)(new)
    # Seams: the block on either side computes its edge row / column from the
    # other block's first row / column, its ghost.
    for axis, parts in ((0, px), (1, py)):
        n = new.shape[axis]
        for o, _ in CC.block_spans(n, parts)[1:]:
            for lo, hi, owner in ((o, min(n, o + H), o - 1), (max(0, o - H), o, o)):
                stale = np.array(new)
                idx = [slice(None)] * 2
                idx[axis] = slice(lo, hi)
                stale[tuple(idx)] = old[tuple(idx)]
                got = step_fn(plate)(stale)
                idx[axis] = owner
                assert (bits(got[tuple(idx)]) != bits(want[tuple(idx)])).any(), (
                    "a stale halo would go unnoticed", axis, o, owner)
    # Filled edges: the frame cell is a copy of an owned cell of the same rank.
    pn, (n0, n1, w0, w1) = _pad(new, plate)
    po, _ = _pad(old, plate)
    if n0 or n1 or w0 or w1:
        crop = (slice(n0, pn.shape[0] - n1), slice(w0, pn.shape[1] - w1))
        assert_bitwise(step_fn(plain)(pn)[crop], want, "the frame rule of this file")
        frames = [(n0, (slice(0, 1), slice(None)), (0, slice(None))),
                  (n1, (slice(-1, None), slice(None)), (-1, slice(None))),
                  (w0, (slice(None), slice(0, 1)), (slice(None), 0)),
                  (w1, (slice(None), slice(-1, None)), (slice(None), -1))]
        for on, frame, edge in frames:
            if not on:
                continue
            stale = np.array(pn)
            stale[frame] = po[frame]
            got = step_fn(plain)(stale)[crop]
            assert (bits(got[edge]) != bits(want[edge])).any(), (
                "a stale edge frame would go unnoticed", frame)


def ghost_model(calls, K: int, m: int, ns: bool, ew: bool, tb: bool, gr: int = 0, gc: int = 0):
    """GhostState's bookkeeping (plan.hpp) for run calls of the given lengths
    on the sync schedule at pass depth K <= 8 (passes of K steps and one
    shorter remainder pass): ([(passes, exchanges)] per call, gr, gc)."""
    out = []
    for n in calls:
        p = e = 0
        while n > 0:
            k = min(K, n)
            if (ns and gr < k) or (ew and gc < k):
                gr = gc = m * K
                e += 1
            gr = gr - k if ns else 0
            gc = ((gc - k) // 4 * 4 if tb else gc - k) if ew else 0
            p += 1
            n -= k
        out.append((p, e))
    return out, gr, gc


# -- the scenario ---------------------------------------------------------------------------

READS = ("gather", "local", "checksum", "coarse", "save", "run0", "time_exchange")
OPS = ("load", "scatter", "load_local", "refine0", "refine1", "reset")
_TARGET = {"refine0": "R0", "refine1": "R1", "reset": "A"}


class Case(NamedTuple):
    """One life of a solver.  pre: run calls from the initial state A; the
    read-only operations `reads` follow, in this order; mid: more run calls
    (what the reads must not have changed); then the replacement `op` at step
    s0 (reset: 0), the run calls `post` with two reads in between, and
    optionally a second replacement `op2` to the third state and `post2`."""
    pre: tuple
    mid: tuple
    reads: tuple
    op: str
    post: tuple
    s0: int = S0
    op2: Optional[str] = None
    post2: tuple = ()
    s02: int = S0_ALT
    enqueue: bool = False   # pre and mid through run(wait=False), no run(0) before `op`


def target(op: str, second: bool = False):
    return _TARGET.get(op, "C" if second else "B")


def rotate(seq, k: int) -> tuple:
    """A different order per case: seq rotated by k, every other one reversed."""
    seq = list(seq)
    k %= len(seq)
    seq = seq[k:] + seq[:k]
    return tuple(seq[::-1] if k % 2 else seq)


class Plan(NamedTuple):
    """Everything a rank needs, computed on the main thread before any solver
    exists: the oracle states after each phase and the checkpoint paths."""
    plate: Plate
    case: Case
    px: int
    py: int
    H: int
    a_pre: np.ndarray
    a_mid: np.ndarray
    new1: np.ndarray
    end1: np.ndarray
    post_reads: tuple      # ((index into post after which to read, state there), ...)
    new2: Optional[np.ndarray]
    end2: Optional[np.ndarray]
    paths: dict            # {"load1": ..., "load2": ..., "save": ...}


def make_plan(plate: Plate, case: Case, px: int, py: int, H: int, paths: dict) -> Plan:
    """The oracle side of a case, with its preconditions asserted."""
    n_pre, n1 = sum(case.pre), sum(case.pre) + sum(case.mid)
    a_pre, a_mid = state(plate, "A", n_pre), state(plate, "A", n1)
    k1 = target(case.op)
    new1, end1 = state(plate, k1, 0), state(plate, k1, sum(case.post))
    check_preconditions(plate, px, py, H, a_mid, new1, shared_ring=case.op == "reset")
    if ghosted(plate, px, py):
        # The continuation crosses a full exchange interval and a remainder pass.
        assert sum(case.post) > H and any(n % 2 for n in case.post), case.post
    cut = max(1, len(case.post) // 2)
    post_reads = ((cut, state(plate, k1, sum(case.post[:cut]))),)
    new2 = end2 = None
    if case.op2:
        k2 = target(case.op2, second=True)
        assert k2 != k1
        new2, end2 = state(plate, k2, 0), state(plate, k2, sum(case.post2))
        check_preconditions(plate, px, py, H, end1, new2, shared_ring=case.op2 == "reset")
    return Plan(plate, case, px, py, H, a_pre, a_mid, new1, end1, post_reads, new2, end2, paths)


_BY_STATE = {}


def _of_state(grid: np.ndarray, what: str, make):
    """make(grid), computed once per oracle state and purpose: the states are
    the frozen arrays of the trajectory cache (kept alive here, so the id
    stays theirs), and every case and rank reads the same few of them."""
    key = (id(grid), what)
    hit = _BY_STATE.get(key)
    if hit is None or hit[0] is not grid:
        hit = _BY_STATE[key] = (grid, make(grid))
    return hit[1]


def _checksum_oracle(grid):
    want = R.checksum_np(grid)
    s_abs = math.fsum(abs(v) for v in np.asarray(grid, np.float64).ravel().tolist())
    return want, s_abs


def assert_checksum(got: dict, want_grid: np.ndarray, what="") -> None:
    """hash, count, min and max exact; the sum within the bound of any fp64
    summation order of the exactly rounded one (README: (n-1)u / (1-(n-1)u)
    times sum |v|, u = 2^-53)."""
    want, s_abs = _of_state(want_grid, "checksum", _checksum_oracle)
    assert got["hash"] == f"{want['hash']:016x}", (what, got, want)
    assert got["count"] == want["count"], what
    assert got["min"] == want["min"] and got["max"] == want["max"], (what, got, want)
    n = want["count"]
    gam = (n - 1) * CC.U / (1 - (n - 1) * CC.U)
    assert abs(got["sum"] - want["sum"]) <= gam * s_abs, (what, got["sum"], want["sum"])


def hash_of(grid: np.ndarray) -> str:
    return f"{_of_state(grid, 'checksum', _checksum_oracle)[0]['hash']:016x}"


def _coarse_oracle(grid):
    """coarse_np's planes and, per coarse cell, the exactly rounded sum and
    the bound of coarse_cases.assert_within_bound: (n-1)u / (1-(n-1)u) times
    sum |v| (math.fsum), for any fp64 summation order."""
    fx, fy = COARSE_F
    want = R.coarse_np(grid, fx, fy)
    g64 = np.asarray(grid, np.float32).astype(np.float64)
    exact, bound = np.empty(want["sum"].shape), np.empty(want["sum"].shape)
    for i in range(exact.shape[0]):
        for j in range(exact.shape[1]):
            cell = g64[i * fx:(i + 1) * fx, j * fy:(j + 1) * fy].ravel().tolist()
            n = len(cell)
            assert n == want["count"][i, j]
            exact[i, j] = math.fsum(cell)
            bound[i, j] = (n - 1) * CC.U / (1 - (n - 1) * CC.U) * math.fsum(abs(v) for v in cell)
    return want, exact, bound


def assert_coarse(got: dict, want_grid: np.ndarray, what="") -> None:
    """min, max and count exact, every sum within its fp64-order bound."""
    want, exact, bound = _of_state(want_grid, "coarse", _coarse_oracle)
    CC.assert_minmax_exact(CC.planes(got), want, what)
    assert np.array_equal(got["count"], want["count"]), what
    assert got["sum"].dtype == np.float64 and got["sum"].shape == exact.shape, what
    err = np.abs(got["sum"] - exact)
    assert (err <= bound).all(), (what, np.argwhere(~(err <= bound))[:8])


def do_read(s, name: str, want: np.ndarray, step: int, plan: Plan, what) -> None:
    """One operation that only reads the state, checked against the oracle."""
    info = s.info
    blk = want[info.ox:info.ox + info.lx, info.oy:info.oy + info.ly]
    if name == "gather":
        g = s.gather()
        assert (g is None) == (s.rank != 0)
        if g is not None:
            assert_bitwise(g, want, (what, "gather"))
    elif name == "local":
        assert_bitwise(s.local(), blk, (what, "local", s.rank))
    elif name == "checksum":
        assert_checksum(s.checksum(), want, (what, "checksum", s.rank))
    elif name == "coarse":
        assert_coarse(s.coarse(*COARSE_F), want, (what, "coarse", s.rank))
    elif name == "save":
        s.save(plan.paths["save"])
        s.barrier()
        if s.rank == 0:
            from parallel_heat_amd.utils import io as hio
            g, h = hio.read_bin(plan.paths["save"], mmap=False)
            assert h["step"] == step, (what, h)
            assert_bitwise(g, want, (what, "save"))
        s.barrier()
    elif name == "run0":
        r = s.run(0)
        assert r.steps_done == 0 and r.passes == 0 and not r.converged, (what, r)
    elif name == "time_exchange":
        if s.world > 1 and s.config.backend == "hip":
            depth = max(1, plan.H - 3)
            assert depth < plan.H
            t, nbytes = s.time_exchange(depth, iters=2)
            assert t >= 0 and nbytes > 0
    else:
        raise ValueError(name)
    assert s.step == step, (what, name, s.step, step)


def do_replace(s, op: str, new: np.ndarray, s0: int, path: Optional[str], plate: Plate) -> int:
    """Apply one replacement; returns the step the run now stands at."""
    info = s.info
    if op == "load":
        s.load(path)
    elif op == "scatter":
        s.scatter(new if s.rank == 0 else None, step=s0)
    elif op == "load_local":
        s.load_local(new[info.ox:info.ox + info.lx, info.oy:info.oy + info.ly], step=s0)
    elif op in ("refine0", "refine1"):
        s.refine(refine_source(plate), *REFINE_F, order=int(op[-1]), step=s0)
    elif op == "reset":
        s.reset()
        return 0
    else:
        raise ValueError(op)
    return s0


def _assert_state(s, want: np.ndarray, step: int, what) -> None:
    info = s.info
    assert s.step == step, (what, s.step, step)
    assert_bitwise(s.local(), want[info.ox:info.ox + info.lx, info.oy:info.oy + info.ly],
                   (what, "local", s.rank))
    g = s.gather()
    if g is not None:
        assert_bitwise(g, want, (what, "gather"))
    assert s.checksum()["hash"] == hash_of(want), what


def play(s, plan: Plan) -> dict:
    """The scenario on one rank (every rank of a group runs it: the collective
    calls match).  Returns the RunResults of each phase."""
    plate, case = plan.plate, plan.case
    info = s.info
    assert (info.px, info.py) == (plan.px, plan.py), info
    assert (info.ox, info.lx, info.oy, info.ly) == blocks(plate, plan.px, plan.py)[s.rank], info
    if ghosted(plate, plan.px, plan.py):
        assert info.halo == plan.H, (info.halo, plan.H)
    what = (case.op, case.op2, s.rank)
    out = {"pre": [], "mid": [], "post": [], "post2": []}
    wait = not case.enqueue
    # 1. a solver that has run
    for n in case.pre:
        out["pre"].append(s.run(n, wait=wait))
    step = sum(case.pre)
    # 2. operations that only read the state
    if not case.enqueue:
        for name in case.reads:
            do_read(s, name, plan.a_pre, step, plan, what)
    for n in case.mid:
        out["mid"].append(s.run(n, wait=wait))
    step += sum(case.mid)
    if not case.enqueue:
        # what the reads must not have changed
        assert_bitwise(s.local(), plan.a_mid[info.ox:info.ox + info.lx, info.oy:info.oy + info.ly],
                       (what, "after the reads"))
        assert s.step == step
    # 3. the replacement, 4. its state
    step = do_replace(s, case.op, plan.new1, case.s0, plan.paths.get("load1"), plate)
    _assert_state(s, plan.new1, step, (what, "replaced"))
    # 5. continue in uneven calls, reading in between
    reads_at = dict(plan.post_reads)
    for i, n in enumerate(case.post):
        out["post"].append(s.run(n))
        step += n
        if i + 1 in reads_at and i + 1 < len(case.post):
            for name in case.reads[:2]:
                do_read(s, name, reads_at[i + 1], step, plan, (what, "between"))
    # 6. the continued state
    _assert_state(s, plan.end1, step, (what, "continued"))
    if ghosted(plate, plan.px, plan.py):
        assert out["post"][0].exchanges >= 1, (what, out["post"][0])
    # 7. once more, another operation, a third state
    if case.op2:
        step = do_replace(s, case.op2, plan.new2, case.s02, plan.paths.get("load2"), plate)
        _assert_state(s, plan.new2, step, (what, "replaced again"))
        for n in case.post2:
            out["post2"].append(s.run(n))
            step += n
        _assert_state(s, plan.end2, step, (what, "continued again"))
        if ghosted(plate, plan.px, plan.py):
            assert out["post2"][0].exchanges >= 1, (what, out["post2"][0])
    return out


def assert_sync_counts(out: dict, case: Case, plate: Plate, px: int, py: int, K: int, m: int,
                       tb: bool) -> tuple:
    """passes and exchanges of every run call against ghost_model (sync
    schedule, K <= 8): the replacement dropped the ghosts' validity, no more
    and no less.  Returns the valid ghost depth (gr, gc) the solver had at the
    first replacement."""
    ns, ew = active_axes(plate, px, py)
    want, gr, gc = ghost_model(case.pre + case.mid, K, m, ns, ew, tb)
    got = [(r.passes, r.exchanges) for r in out["pre"] + out["mid"]]
    assert got == want, ("before the replacement", got, want)
    for phase, calls in (("post", case.post), ("post2", case.post2)):
        want = ghost_model(calls, K, m, ns, ew, tb)[0]
        got = [(r.passes, r.exchanges) for r in out[phase]]
        assert got == want, (phase, got, want)
    return gr, gc


def write_checkpoint(s, grid: np.ndarray, step: int, path: str) -> None:
    """A checkpoint of `grid` at `step`, written by the solver `s` (collective)."""
    s.scatter(grid if s.rank == 0 else None, step=step)
    s.save(path)
    s.barrier()


# -- convergence across a replacement --------------------------------------------------------

CONV = dict(nx=40, ny=70, cx=0.1, cy=0.1, eps=0.02, seed=3)
CONV_RUN = 400     # steps asked of every run: more than any case needs to converge


@functools.lru_cache(maxsize=None)
def conv_start(kind: str = "A", nx: int = CONV["nx"], ny: int = CONV["ny"]) -> np.ndarray:
    if kind == "U":
        return _frozen(np.ones((nx, ny), np.float32))
    return _frozen(R.init_grid(nx, ny, "random", CONV["seed"]))


@functools.lru_cache(maxsize=None)
def conv_oracle(step0: int, interval: int, compat: str = "none", periodic: str = "",
                kind: str = "A", n: int = CONV_RUN, pre: int = 0) -> Continued:
    """continue_full of the convergence plate from conv_start(kind) advanced
    `pre` unchecked steps, standing at absolute step `step0`."""
    u = conv_start(kind)
    for _ in range(pre):
        u = R.step_np_fma(u, CONV["cx"], CONV["cy"], "", periodic)
    c = continue_full(u, step0, n, cx=CONV["cx"], cy=CONV["cy"], converge=True,
                      check_interval=interval, eps=CONV["eps"], compat=compat,
                      periodic=periodic)
    return c._replace(grid=_frozen(c.grid))


def assert_converges_inside(c: Continued, step0: int, interval: int, compat: str,
                            n: int = CONV_RUN) -> None:
    """The oracle converges at a check that is neither the first after step0
    nor the last the run could reach."""
    ks = check_steps_between(step0, step0 + n, interval, compat)
    assert c.converged_at in ks[1:-1], (c.converged_at, ks[:3], ks[-2:])
    assert c.checks == ks.index(c.converged_at) + 1


def assert_run_result(r, c: Continued, what="") -> None:
    assert r.converged == (c.converged_at >= 0), (what, r, c[1:])
    if c.converged_at >= 0:
        assert r.converged_at == c.converged_at, (what, r, c[1:])
    assert r.steps_done == c.steps_done, (what, r, c[1:])
    assert r.checks == c.checks, (what, r, c[1:])
    assert np.float32(r.last_resid) == np.float32(c.last_resid), (what, r, c[1:])
