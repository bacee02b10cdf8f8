"""Shared cases of the heat-source tests (tests/test_source_cpu.py on the host
twin and the CPU backend, tests/test_gpu_source.py on the MI355X): the one-step
source kernel alone against reference.step_np_fma(source=), the solver against
reference.run_np(source=), the exact conservation case and the ghost rule.
Equality is bitwise throughout."""
import numpy as np
import torch

from parallel_heat_amd import HeatConfig, HeatSolver, ops
from parallel_heat_amd.models import reference as R

COEFS = [(0.05, 0.2), (0.1, 0.1)]
KINDS = ["signed", "wide", "subnormal"]
SENTINEL = -777.25  # what dst holds where the step must not write

# Plates whose one block is the whole plate and whose box is the block.
# No or one interior cell; plate column ny-1 in each lane element; widths
# around the 256-column strip; 70 rows (more than a chunk of 64).
PLATES = [(1, 1), (1, 9), (9, 1), (2, 2), (3, 3), (13, 516), (13, 517), (13, 518), (13, 519),
          (5, 255), (5, 256), (5, 257), (5, 513), (70, 300)]

EDGES = [dict(), dict(insulated="ns"), dict(periodic="y"), dict(insulated="we", periodic="x"),
         dict(periodic="xy")]
EDGE_IDS = ["dirichlet", "ins-ns", "per-y", "ins-we+per-x", "per-xy"]
# (nx, ny, fx, fy, order): both factors leave partial last cells.
SOLVER_CASES = [(37, 53, 4, 8, 0), (37, 53, 5, 3, 1), (64, 300, 4, 8, 1), (64, 300, 5, 3, 0)]
STEPS = 30


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def word_of(x):
    """The float32 bits of a scalar as an int (what a residual word holds)."""
    return int(np.array(x, np.float32).reshape(1).view(np.uint32)[0])


def assert_bitwise(got, want, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, (what, f"{len(bad)} cells differ, first {tuple(bad[0])}: "
                           f"{got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}")


def values(kind, shape, seed):
    """signed: N(0, 100); wide: +-2^e, e uniform in [-140, 100]; subnormal:
    nine in ten cells subnormal (random mantissa, exponent field 0), the rest
    of the order of 2^-120, signs mixed."""
    rng = np.random.default_rng(seed)
    if kind == "signed":
        return (rng.standard_normal(shape) * 100).astype(np.float32)
    sign = np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    if kind == "wide":
        return (sign * np.exp2(rng.uniform(-140, 100, shape))).astype(np.float32)
    if kind == "subnormal":
        sub = rng.integers(1, 1 << 23, shape, dtype=np.uint32).view(np.float32)
        small = np.exp2(rng.uniform(-126, -118, shape)).astype(np.float32)
        return (sign * np.where(rng.random(shape) < 0.9, sub, small)).astype(np.float32)
    raise ValueError(kind)


class RawField:
    """An lx x ly block at column `off` of row 1 of a buffer of `pitch` floats
    per row, one frame row above and below: what ops.source_step needs of a
    Field, at any alignment."""

    def __init__(self, lx, ly, pitch, off, device, fill):
        assert off >= 1 and pitch >= off + ly + 1
        self.lx, self.ly, self.pitch, self.off = lx, ly, pitch, off
        self.hx, self.hy = 1, off
        self.data = torch.full((lx + 2, pitch), fill, dtype=torch.float32, device=device)
        self.device = self.data.device

    def ptr(self):
        return self.data.data_ptr() + 4 * (self.pitch + self.off)


def _fields(device, lx, ly, raw):
    if raw is None:
        mk = lambda fill: ops.Field(lx, ly, halo=1, device=device, fill=fill)  # noqa: E731
    else:
        mk = lambda fill: RawField(lx, ly, raw[0], raw[1], device, fill)  # noqa: E731
    return mk(float("nan")), mk(SENTINEL), mk(float("nan"))


def run_step(device, plate, coef, kind, block=None, box=None, raw=None, seed=0, q_plate=None,
             resid0=None, gate=None):
    """One source step of the block (gx0, gy0, lx, ly) of a plate (default: the
    whole plate) over `box` (local; default: the block).  src holds the plate's
    values wherever a cell of the field, its frame included, lies on the plate
    and NaN elsewhere; q holds its values in the box alone, NaN elsewhere; dst
    is SENTINEL.  Returns (dst as a NumPy array of the whole buffer, the index
    arrays of the box in it, the expected box, u's box, the residual word or
    None)."""
    nx, ny = plate
    gx0, gy0, lx, ly = block or (0, 0, nx, ny)
    r0, r1, c0, c1 = box or (0, lx, 0, ly)
    u = values(kind, plate, seed)
    # A source of the field's own magnitude, so that the add rounds.
    q = values(kind, plate, seed + 1000) if q_plate is None else np.asarray(q_plate, np.float32)
    src, dst, qf = _fields(device, lx, ly, raw)
    rows, cols = src.data.shape
    # Buffer cell (i, j) is local (i - hx, j - hy), plate (gx0 + i - hx, gy0 + j - hy).
    pi = np.arange(rows) - src.hx + gx0
    pj = np.arange(cols) - src.hy + gy0
    on = ((pi >= 0) & (pi < nx))[:, None] & ((pj >= 0) & (pj < ny))[None, :]
    host = np.full((rows, cols), np.nan, np.float32)
    host[on] = u[np.clip(pi, 0, nx - 1)[:, None], np.clip(pj, 0, ny - 1)[None, :]][on]
    src.data.copy_(torch.from_numpy(host))
    bi = slice(src.hx + r0, src.hx + r1)
    bj = slice(src.hy + c0, src.hy + c1)
    pr, pc = slice(gx0 + r0, gx0 + r1), slice(gy0 + c0, gy0 + c1)
    hq = np.full((rows, cols), np.nan, np.float32)
    hq[bi, bj] = q[pr, pc]
    qf.data.copy_(torch.from_numpy(hq))
    word = None
    if resid0 is not None:
        word = torch.tensor([resid0], dtype=torch.int64).to(torch.int32).to(src.device)
    geom = ops.Geom(nx, ny, gx0, gy0, coef[0], coef[1])
    ops.source_step(src, dst, qf, geom, (r0, r1, c0, c1), resid=word, gate=gate)
    want = R.step_np_fma(u, coef[0], coef[1], source=q)
    return (dst.data.cpu().numpy(), (bi, bj), want[pr, pc], u[pr, pc],
            None if word is None else int(word.cpu()[0]) & 0xFFFFFFFF)


def check_step(device, plate, coef, kind, what=None, **kw):
    """The box holds the oracle's step bit for bit, every other cell of dst
    still SENTINEL, and the residual word NumPy's max |new - old|."""
    what = what or (plate, coef, kind, kw)
    got, (bi, bj), want, old, word = run_step(device, plate, coef, kind, resid0=0, **kw)
    assert_bitwise(got[bi, bj], want, what)
    rest = got.copy()
    rest[bi, bj] = SENTINEL
    assert np.all(rest == np.float32(SENTINEL)), (what, "a cell outside the box was written")
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.max(np.abs(want - old)) if want.size else np.float32(0)
    assert word == word_of(m), (what, "residual", hex(word), float(m))


def source_map(cr, cc, seed=11):
    """A random, asymmetric source map of small integers' halves (exact in the
    bilinear weights' products more often than not; the comparison is bitwise
    either way)."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-40, 41, (cr, cc)) * 0.5).astype(np.float32)


def dims(nx, ny, fx, fy):
    return -(-nx // fx), -(-ny // fy)


def solver_want(case, edges, steps=STEPS, u0=None, S=None, **kw):
    """(S, the oracle's levels run_np gives after `steps`)."""
    nx, ny, fx, fy, order = case
    S = source_map(*dims(nx, ny, fx, fy)) if S is None else S
    q = R.refine_np(S, nx, ny, fx, fy, order, edges.get("periodic", ""))
    u0 = R.init_grid(nx, ny, "random", 3) if u0 is None else u0
    return S, R.run_np(nx, ny, steps, u0=u0, numerics="fma", source=q,
                       insulated=edges.get("insulated", ""), periodic=edges.get("periodic", ""),
                       **kw)


def solver_cfg(case, edges, backend, steps=STEPS, **kw):
    nx, ny = case[:2]
    return HeatConfig(nx=nx, ny=ny, steps=steps, init="random", seed=3, backend=backend,
                      source=True, **edges, **kw)


def check_solver(backend, case, edges, **kw):
    nx, ny, fx, fy, order = case
    S, (want, _, _) = solver_want(case, edges)
    with HeatSolver(solver_cfg(case, edges, backend, **kw)) as s:
        s.set_source(S, fx, fy, order)
        r = s.run()
        assert r.steps_done == STEPS
        got = s.gather()
    assert_bitwise(got, want, (backend, case, edges, kw))
    return got


# Conservation on a torus: with cx = cy = 1/4 and integer data every value is
# a multiple of 4^-n after n steps and below 2^24 in units of it (64 + 4n
# bounds the field; 6 steps: 88 * 4^6 < 2^19), so every fp32 operation of the
# update is exact: the field equals the fp64 recurrence and its sum grows by
# sum(q) per step, exactly.
CONSERVATION_PLATES = [(37, 53), (13, 519), (1, 9)]
CONSERVATION_STEPS = 6


def conservation_case(plate, seed=5):
    nx, ny = plate
    rng = np.random.default_rng(seed)
    u0 = rng.integers(0, 64, plate).astype(np.float32)
    S = rng.integers(0, 4, plate).astype(np.float32)  # order 0, factors 1: q = S
    u = u0.astype(np.float64)
    for _ in range(CONSERVATION_STEPS):
        n, s = np.roll(u, 1, 0), np.roll(u, -1, 0)
        w, e = np.roll(u, 1, 1), np.roll(u, -1, 1)
        u = u + 0.25 * ((s + n) - 2 * u) + 0.25 * ((e + w) - 2 * u) + S
    total = float(u0.astype(np.float64).sum() + CONSERVATION_STEPS * S.astype(np.float64).sum())
    return u0, S, u, total


def check_conservation(make_solver, plate):
    """make_solver(cfg, fn) -> what fn(solver) returned on rank 0."""
    u0, S, want, total = conservation_case(plate)
    cfg = HeatConfig(nx=plate[0], ny=plate[1], steps=CONSERVATION_STEPS, cx=0.25, cy=0.25,
                     init="zero", periodic="xy", source=True)

    def fn(s):
        s.scatter(u0 if s.rank == 0 else None)
        s.set_source(S, 1, 1, 0)
        s.run()
        return s.checksum(), s.gather()

    ck, got = make_solver(cfg, fn)
    assert ck["sum"] == total, (plate, ck["sum"], total)
    assert np.array_equal(got.astype(np.float64), want), plate
    assert float(want.sum()) == total


def ghost_map(i, n, wrap, lo, hi):
    """The plate index a cell at index i of an axis stands for (the issue's
    `map`): identity on the plate, i mod n on a periodic axis, the mirror
    beyond an insulated end, clamped beyond a fixed one."""
    i = np.asarray(i)
    if wrap:
        return np.mod(i, n)
    m = np.where(i < 0, -i if lo else 0, np.where(i >= n, 2 * (n - 1) - i if hi else n - 1, i))
    return np.clip(m, 0, n - 1)


def check_source_block(s, S, case, edges):
    """A rank's extended source block equals refine_np of the plate indexed
    through the map, ghost ring and corners included."""
    nx, ny, fx, fy, order = case
    per, ins = edges.get("periodic", ""), edges.get("insulated", "")
    q = R.refine_np(S, nx, ny, fx, fy, order, per)
    i, H = s.info, s.info.halo
    rows = ghost_map(np.arange(i.ox - H, i.ox + i.lx + H), nx, "x" in per, "n" in ins, "s" in ins)
    cols = ghost_map(np.arange(i.oy - H, i.oy + i.ly + H), ny, "y" in per, "w" in ins, "e" in ins)
    assert_bitwise(s.source_block(H), q[rows[:, None], cols[None, :]],
                   (case, edges, "rank", s.rank, "halo", H))
