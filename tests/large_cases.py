"""Helpers of the large-offset tests (CPU and GPU): where in a field the byte
offset from the tensor's base passes 2^31, 2^32, 2^33 and 2^34, row bands
around those cells, a windowed NumPy oracle that never holds more than a band,
and the poisoning that turns a stray read into a NaN and a stray store into a
broken sentinel.  Plain functions on ops.Field; nothing here needs a GPU."""
import numpy as np
import torch

from parallel_heat_amd.models import reference as R

# Signed / unsigned 32-bit byte offsets, signed / unsigned 32-bit float indices.
MARKS = (1 << 31, 1 << 32, 1 << 33, 1 << 34)
SENTINEL = -12345.5   # finite, negative: no heat value of a random plate (0..100)
CHUNK_CELLS = 1 << 26  # cells per device reduction: temporaries stay far below a field

# The plates (nx, ny) of the GPU tests, all with a 12-deep ghost ring; DEEP has
# a 4352-float pitch and 18 depth-12 strips.  test_large_cases_cpu.py checks,
# from the layout alone, which marks each one reaches.
HALO = 12
SETS = {"DEEP": (1_000_000, 4072), "MID3": (500_000, 4072), "SQUARE": (34_000, 34_000),
        "WIDE": (1_200, 1_000_000), "CELLS": (46_400, 46_400)}


def marks(field, marks=MARKS):
    """[(mark, r, c)]: the local row and column of the cell whose byte offset
    from the tensor's first element (ghost rows and columns included) is
    `mark`, for every mark that falls inside the tensor.  c may lie in the
    ghost columns or the row padding (c < 0 or c >= ly)."""
    out = []
    for m in marks:
        e = int(m) // 4
        if e >= field.rows * field.pitch:
            continue
        out.append((int(m), e // field.pitch - field.hx, e % field.pitch - field.hy))
    return out


def _cols(field, c, width):
    """The column window of a band: every column (cut to a multiple of 4), or
    `width` columns around column c, starting at a multiple of 4."""
    c1 = field.ly - field.ly % 4
    if width is None or width >= c1:
        return 0, c1
    c0 = min(max(0, (c - width // 2) // 4 * 4), c1 - width // 4 * 4)
    return c0, c0 + width // 4 * 4


def bands(field, mark_list=None, half=32, width=None, edge=64):
    """Boxes (r0, r1, c0, c1): rows [R - half, R + half) around every mark row
    R, the plate's first and last `edge` rows (the last hold the bottom
    Dirichlet edge and the largest offsets), clipped to the owned block, bands
    that overlap merged.  Columns: all of them, cut to a multiple of 4 (TB
    boxes need c0 % 4 == 0); with `width`, that many columns around the mark's
    column (the first rows at the first columns, the last rows at the last)."""
    mark_list = marks(field) if mark_list is None else mark_list
    raw = [(0, edge, 0), (field.lx - edge, field.lx, field.ly - 1)]
    raw += [(r - half, r + half, c) for _, r, c in mark_list]
    out = []
    for r0, r1, c in sorted(raw):
        r0, r1 = max(0, r0), min(field.lx, r1)
        if r1 <= r0:
            continue
        c0, c1 = _cols(field, min(max(c, 0), field.ly - 1), width)
        if out and out[-1][2:] == (c0, c1) and r0 <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], r1), c0, c1)
        else:
            out.append((r0, r1, c0, c1))
    return out


def grow(box, k, nx, ny):
    """`box` grown by k cells on every side, clipped to the nx x ny plate."""
    r0, r1, c0, c1 = box
    return max(0, r0 - k), min(nx, r1 + k), max(0, c0 - k), min(ny, c1 + k)


def init_window(nx, ny, seed, box):
    """The random initial condition of the plate on `box` alone."""
    r0, r1, c0, c1 = box
    return R.init_grid(nx, ny, "random", seed, r0, c0, r1 - r0, c1 - c0)


def source_window(nx, ny, seed, box):
    """A per-cell heat source of both signs, a function of the plate cell:
    the random initial condition of another seed, shifted and scaled."""
    v = init_window(nx, ny, seed ^ 0x5EED, box)
    return ((v - np.float32(50.0)) * np.float32(0.03125)).astype(np.float32)


def window_levels(nx, ny, seed, box, k, cx=0.1, cy=0.1, q=None, step=R.step_np_fma):
    """States 0..k of `box` (plate coordinates, the field being the whole
    plate): the initial condition on the box grown by k and clipped to the
    plate, k steps on that window, every state cropped back to the box.  The
    window's own ring stays fixed, which is wrong k cells away from the box at
    most (and right where the window ends at the plate's edge), so the crop is
    the full-plate result bit for bit.  q: a source seed (source_window)."""
    r0, r1, c0, c1 = box
    g = grow(box, k, nx, ny)
    u = init_window(nx, ny, seed, g)
    src = None if q is None else source_window(nx, ny, q, g)
    crop = (slice(r0 - g[0], r1 - g[0]), slice(c0 - g[2], c1 - g[2]))
    out = [u[crop].copy()]
    for _ in range(k):
        u = step(u, cx, cy) if src is None else step(u, cx, cy, source=src)
        out.append(u[crop].copy())
    return out


def step_np_mfma(u, cx=0.1, cy=0.1):
    """One step in the association of the MFMA kernel (csrc/kernels/mfma.hip):
    the banded products accumulate the four neighbours, the centre joins last,
        fma(k0, c, fma(cy, e, fma(cy, w, fma(cx, s, cx * n)))),
        k0 = fma(-2, cy, fma(-2, cx, 1)),
    every operation a correctly rounded fp32 one (zero terms are exact
    no-ops); the ring stays fixed.  On values in [0, 100) with cx = cy = 0.1
    the partial sums stay below 10, 20, 30, 40 and 100, so the chain is
    within 0.48 + 0.95 + 0.95 + 1.9 + 3.8 = 8.1e-6 of the exact step, and
    step_np_fma within 1.5 + 1.5 + 3.8 + 3.8 = 10.6e-6 of it: at most 1.87e-5
    apart, inside the 2e-5 the mfma tests hold the kernel to."""
    u = np.asarray(u, np.float32)
    out = u.copy()
    if u.shape[0] < 3 or u.shape[1] < 3:
        return out
    fcx, fcy = np.float32(cx), np.float32(cy)
    k0 = R.fma32(np.float32(-2.0), fcy, R.fma32(np.float32(-2.0), fcx, np.float32(1.0)))
    d = (fcx * u[:-2, 1:-1]).astype(np.float32)
    d = R.fma32(fcx, u[2:, 1:-1], d)
    d = R.fma32(fcy, u[1:-1, :-2], d)
    d = R.fma32(fcy, u[1:-1, 2:], d)
    out[1:-1, 1:-1] = R.fma32(k0, u[1:-1, 1:-1], d)
    return out


def window_oracle(nx, ny, seed, box, k, cx=0.1, cy=0.1, q=None):
    """The plate's state after k steps on `box`, from a window (window_levels)."""
    return window_levels(nx, ny, seed, box, k, cx, cy, q)[k]


def refine_rows(S, nx, ny, fx, fy, order, r0, r1, wrap=""):
    """Rows [r0, r1) of reference.refine_np(S, nx, ny, fx, fy, order, wrap): its
    definition with the row table sliced, so that no host array is larger
    than those rows."""
    S = np.ascontiguousarray(S, np.float32)
    i0, i1, wx = (t[r0:r1] for t in R.refine_axis_np(nx, fx, order, "x" in wrap))
    j0, j1, wy = R.refine_axis_np(ny, fy, order, "y" in wrap)
    top = R._lerp32(S[i0][:, j0], S[i0][:, j1], wy[None, :])
    bot = R._lerp32(S[i1][:, j0], S[i1][:, j1], wy[None, :])
    return np.ascontiguousarray(R._lerp32(top, bot, wx[:, None]))


def coarse_banded(values, nx, ny, fx, fy):
    """The coarse view (reference.coarse_np) of an nx x ny plate that is 0.0
    everywhere but on the full-width row bands `values` ([(r0, array)], no
    two overlapping), from the bands alone: {coarse row I: (sum, min, max,
    bound)} for every coarse row that meets a band, each an array over the
    coarse columns.  bound: the worst case of any fp64 summation order,
    cells * 2^-53 * sum |v|; the zeros add exactly and join min and max where
    a coarse cell is not all band."""
    out = {}
    for r0, v in values:
        assert v.shape[1] == ny
        for I in range(r0 // fx, -(-(r0 + v.shape[0]) // fx)):
            lo, hi = max(r0, I * fx), min(r0 + v.shape[0], (I + 1) * fx)
            c = R.coarse_np(v[lo - r0:hi - r0], hi - lo, fy)
            s, mn, mx = c["sum"][0], c["min"][0], c["max"][0]
            a = R.coarse_np(np.abs(v[lo - r0:hi - r0]), hi - lo, fy)["sum"][0]
            n = c["count"][0].astype(np.float64)
            rows = np.zeros_like(n)
            if I in out:
                s0, mn0, mx0, a0, n0, rows0 = out[I]
                s, mn, mx = s + s0, np.minimum(mn, mn0), np.maximum(mx, mx0)
                a, n, rows = a + a0, n + n0, rows0
            out[I] = (s, mn, mx, a, n, rows + (hi - lo))
    res = {}
    for I, (s, mn, mx, a, n, rows) in out.items():
        full = rows == min((I + 1) * fx, nx) - I * fx  # the coarse row is all band
        zero = np.float32(0.0)
        res[I] = (s, np.where(full, mn, np.minimum(mn, zero)),
                  np.where(full, mx, np.maximum(mx, zero)), n * 2.0 ** -53 * a)
    return res


def _put(field, box, values):
    r0, r1, c0, c1 = box
    field.view(r0, r1, c0, c1).copy_(torch.from_numpy(np.ascontiguousarray(values)))


def poison(src, dst, boxes, k, seed, q=None, qseed=None, grow_q=None):
    """src: NaN in every cell of the tensor but the boxes grown by k (clipped
    to the plate), which hold the initial condition; dst: SENTINEL everywhere.
    A read outside a box's light cone then drags a NaN into the result, a
    store outside the boxes breaks the sentinel count (`untouched`).  q (a
    third field) is poisoned like src with source_window(qseed), grown by
    grow_q (default k)."""
    nx, ny = src.lx, src.ly
    src.data.fill_(float("nan"))
    if dst is not None:
        dst.data.fill_(SENTINEL)
    for b in boxes:
        g = grow(b, k, nx, ny)
        _put(src, g, init_window(nx, ny, seed, g))
    if q is not None:
        q.data.fill_(float("nan"))
        for b in boxes:
            g = grow(b, k if grow_q is None else grow_q, nx, ny)
            _put(q, g, source_window(nx, ny, qseed, g))


def chunks(t):
    """The 2-D tensor t in runs of whole rows of at most CHUNK_CELLS cells."""
    rows = max(1, CHUNK_CELLS // max(1, t.shape[1]))
    return [t[r:r + rows] for r in range(0, t.shape[0], rows)]


def count_ne(t, value):
    """Cells of the 2-D tensor t that differ from `value` (a NaN differs), by
    row chunks on the tensor's device."""
    return sum(int((c != value).sum()) for c in chunks(t))


def untouched(dst, boxes, sentinel=SENTINEL):
    """Cells of dst's whole tensor (ghosts and padding included) outside the
    (disjoint) boxes that no longer hold the sentinel."""
    inside = sum(count_ne(dst.view(*b), sentinel) for b in boxes)
    return count_ne(dst.data, sentinel) - inside


def same_values(a, b):
    """torch.equal of two 2-D tensors of one shape, by row chunks."""
    assert a.shape == b.shape
    return all(torch.equal(x, y) for x, y in zip(chunks(a), chunks(b)))
