"""The hot-cell plate and its exact residual oracle (CPU and GPU coverage
tests of the residual, `max |new - old|`).

The plate is one constant C with a single cell q raised by H, stepped with
cx = 1/256, cy = 1/128 (exact in fp32, anisotropic).  A cell whose five
inputs are all C stays exactly C under `heat::stencil` (fma(-2, C, C + C) is
exactly 0), so after n steps only cells within Manhattan distance n of q have
moved, |delta| has its unique maximum at q at every step (while q is an
updated cell), the runner-up is at most 2/3 of it, and the residuals of the
steps of one pass are pairwise distinct.  A residual that drops q's row,
column, lane, wave or stage, takes another level, or looks one cell past its
box therefore reports another fp32 word than the oracle.

The oracle steps `reference.step_np_fma` on a window around q: the plate
cropped to q +- (n + 1) rows and columns, clipped at the plate's edges.  The
crop's rim is the plate's own ring or cells that provably stay C, so the
window is exact, not an approximation; test_residual_coverage_cpu.py proves
it bit for bit against the full plate.  Windows are memoised by what they
depend on (the distances to the plate's edges, clipped at n + 1, and the
edge kinds met), the residual over a box is a masked max of the window."""
import functools

import numpy as np

from parallel_heat_amd.models import reference as R

C, H = np.float32(50.0), np.float32(37.0)
COEF = (1.0 / 256, 1.0 / 128)
SWAPPED = COEF[::-1]
_STEP = {"fma": R.step_np_fma, "mpi": R.step_np_mpi}


def plate(nx, ny, q=None):
    """The nx x ny plate of C, cell q (row, column) raised by H."""
    u = np.full((nx, ny), C, np.float32)
    if q is not None:
        u[q] += H
    return u


def full_deltas(nx, ny, q, n, coef=COEF, insulated="", periodic="", numerics="fma"):
    """|state k - state k-1| for k = 1..n of the FULL plate (the slow twin of
    the window; the oracle's own tests compare the two)."""
    step, u, out = _STEP[numerics], plate(nx, ny, q), []
    for _ in range(n):
        v = step(u, coef[0], coef[1], insulated, periodic)
        out.append(np.abs(v - u))
        u = v
    return out


def _axis(size, q, n, wraps, ins_lo, ins_hi):
    """One axis of the window: the plate indices of its rows (or columns),
    q's index in it, and the edge treatment it keeps: "p" the whole periodic
    axis, else the insulated plate sides it touches as (lo, hi) flags.  Sides
    cut inside the plate lie n + 1 cells from q and stay C: fixed."""
    w = n + 1
    if wraps:
        if size <= 2 * w + 1:
            return np.arange(size), q, "p"
        return (q + np.arange(-w, w + 1)) % size, w, (False, False)
    lo, hi = max(0, q - w), min(size, q + w + 1)
    return np.arange(lo, hi), q - lo, (ins_lo and lo == 0, ins_hi and hi == size)


@functools.lru_cache(maxsize=None)
def _window(rows, cols, qi, qj, ex, ey, n, coef, numerics):
    """|delta| of steps 1..n on a rows x cols window with the hot cell at
    (qi, qj) and the edge treatment (ex, ey) of _axis; read-only arrays."""
    ins = "".join(s for s, on in zip("ns", ex if ex != "p" else ()) if on) + \
          "".join(s for s, on in zip("we", ey if ey != "p" else ()) if on)
    per = ("x" if ex == "p" else "") + ("y" if ey == "p" else "")
    out = full_deltas(rows, cols, (qi, qj), n, coef, ins, per, numerics)
    for d in out:
        d.setflags(write=False)
    return tuple(out)


def window(shape, q, n, coef=COEF, insulated="", periodic="", numerics="fma"):
    """(plate rows of the window, plate columns, |delta| of steps 1..n on it,
    q's position in it)."""
    ins, per = R.insulated_sides(insulated), R.periodic_axes(periodic)
    ri, qi, ex = _axis(shape[0], q[0], n, "x" in per, "n" in ins, "s" in ins)
    ci, qj, ey = _axis(shape[1], q[1], n, "y" in per, "w" in ins, "e" in ins)
    return ri, ci, _window(len(ri), len(ci), qi, qj, ex, ey, n, tuple(coef), numerics), (qi, qj)


def resid_levels(shape, q, box, n, coef=COEF, insulated="", periodic="", numerics="fma"):
    """The residuals of steps 1..n over box (r0, r1, c0, c1; plate
    coordinates) of the hot-cell plate, as an fp32 vector.  q anywhere on the
    plate, inside the box or not; cells outside the window did not move."""
    ri, ci, deltas, _ = window(shape, q, n, coef, insulated, periodic, numerics)
    rin = np.flatnonzero((ri >= box[0]) & (ri < box[1]))
    cin = np.flatnonzero((ci >= box[2]) & (ci < box[3]))
    out = np.zeros(n, np.float32)
    if rin.size and cin.size:
        for k, d in enumerate(deltas):
            out[k] = d[np.ix_(rin, cin)].max()
    return out


def resid_table(shape, positions, box, n, **kw):
    """resid_levels for each of `positions`: an (len(positions), n) array."""
    return np.stack([resid_levels(shape, q, box, n, **kw) for q in positions]) \
        if len(positions) else np.zeros((0, n), np.float32)


def preconditions(shape, q, box, n, **kw):
    """What makes the comparison sharp, on the reference alone, for an
    UPDATED cell q inside the box: at every step 1..n the maximum of |delta|
    over the box is at q and nowhere else, and the n residuals are pairwise
    distinct.  Returns the worst runner-up / max ratio over the steps."""
    ri, ci, deltas, (qi, qj) = window(shape, q, n, **kw)
    rin = np.flatnonzero((ri >= box[0]) & (ri < box[1]))
    cin = np.flatnonzero((ci >= box[2]) & (ci < box[3]))
    assert qi in rin and qj in cin, (q, box)
    worst, seen = 0.0, set()
    for k, d in enumerate(deltas, 1):
        m = np.array(d[np.ix_(rin, cin)])
        top = m.max()
        at = np.argwhere(m == top)
        assert top > 0 and len(at) == 1 and (rin[at[0][0]], cin[at[0][1]]) == (qi, qj), \
            (q, k, float(top), at.tolist())
        m[at[0][0], at[0][1]] = 0
        assert m.max() < top, (q, k)
        worst = max(worst, float(m.max()) / float(top))
        seen.add(top.tobytes())
    assert len(seen) == n, (q, "levels not distinct")
    return worst


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def assert_words(got, want, positions, what=""):
    """Exact equality of the fp32 words; on failure every failing position
    (the pattern names the broken mask: every 4th column, one row per chunk,
    one band)."""
    got, want = np.asarray(got, np.float32).ravel(), np.asarray(want, np.float32).ravel()
    assert got.shape == want.shape == (len(positions),)
    bad = np.flatnonzero(bits(got) != bits(want))
    if bad.size:
        rows = sorted({positions[i][0] for i in bad})
        cols = sorted({positions[i][1] for i in bad})
        lines = [f"  q=({positions[i][0]}, {positions[i][1]}): got {got[i]!r} want {want[i]!r}"
                 for i in bad[:40]]
        raise AssertionError(
            f"{what}: {bad.size} of {len(positions)} positions differ\n  rows {rows}\n"
            f"  cols {cols}\n" + "\n".join(lines) + ("\n  ..." if bad.size > 40 else ""))


def cross(lx, ly, cols, rows, r0=0, c0=0):
    """The sweep positions of an lx x ly block at (r0, c0): every row along
    the columns `cols`, every column along the rows `rows` (block-local), so
    that every row and every column holds the maximum at least once."""
    out = [(r0 + r, c0 + c) for c in cols for r in range(lx)]
    out += [(r0 + r, c0 + c) for r in rows for c in range(ly)]
    return list(dict.fromkeys(out))


def frame(lx, ly, r0=0, c0=0, above=2, below=2, left=2, right=4):
    """The exclusion frame of the block: the rows -above..-1 and lx..lx +
    below - 1 and the columns -left..-1 and ly..ly + right - 1 along their
    full length (the corners included)."""
    rr = list(range(-above, 0)) + list(range(lx, lx + below))
    cc = list(range(-left, 0)) + list(range(ly, ly + right))
    out = [(r0 + r, c0 + c) for r in rr for c in range(-left, ly + right)]
    out += [(r0 + r, c0 + c) for c in cc for r in range(lx)]
    return list(dict.fromkeys(out))
