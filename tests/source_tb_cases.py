"""Shared cases of the fused source-pass tests (tests/test_gpu_source_tb.py on
the MI355X, tests/test_source_tb_cpu.py for the planner): ops.source_tb_step
against k applications of reference.step_np_fma(source=) over the shrinking
boxes, with NaN wherever the contract forbids a read.  Equality is bitwise
throughout."""
import numpy as np
import torch

from parallel_heat_amd import ops
from parallel_heat_amd.models import reference as R

from .source_cases import (COEFS, KINDS, SENTINEL, assert_bitwise, bits, values,  # noqa: F401
                           word_of)

DEPTHS = [2, 3, 4, 5, 6, 7, 8]
EDGE_DEPTHS = [2, 3, 8]     # the shallowest, an odd one (overlap 4 > k), the deepest
STRIP_COLS = 256


def overlap(k):
    return -(-k // 4) * 4


def stride(k):
    """Columns a strip stores: W of the issue."""
    return STRIP_COLS - 2 * overlap(k)


class FramedField:
    """An lx x ly block at column `off` of row `frame` of a buffer of `pitch`
    floats per row, `frame` rows above and below: what ops.source_tb_step needs
    of a Field, at any alignment."""

    def __init__(self, lx, ly, frame, pitch, off, device, fill):
        assert off >= frame and pitch >= off + ly + frame
        self.lx, self.ly, self.pitch = lx, ly, pitch
        self.hx, self.hy = frame, off
        self.data = torch.full((lx + 2 * frame, pitch), fill, dtype=torch.float32, device=device)
        self.device = self.data.device

    def ptr(self):
        return self.data.data_ptr() + 4 * (self.hx * self.pitch + self.hy)


def fields(device, lx, ly, k, raw=None, q_off=None):
    """(src, dst, q): NaN, SENTINEL and NaN filled.  raw = (pitch, off): a
    FramedField, q at column q_off if given (out of phase with src)."""
    if raw is None:
        mk = lambda fill, _: ops.Field(lx, ly, halo=k, device=device, fill=fill)  # noqa: E731
    else:
        mk = lambda fill, off: FramedField(lx, ly, k, raw[0], off or raw[1], device,  # noqa: E731
                                           fill)
    return mk(float("nan"), None), mk(SENTINEL, None), mk(float("nan"), q_off)


def grown(box, e, plate):
    """Plate-coordinate box grown by e on every side, clipped to the plate."""
    r0, r1, c0, c1 = box
    return max(r0 - e, 0), min(r1 + e, plate[0]), max(c0 - e, 0), min(c1 + e, plate[1])


def framed(a, box):
    """a with NaN outside `box` (plate coordinates)."""
    out = np.full(a.shape, np.nan, np.float32)
    r0, r1, c0, c1 = box
    out[r0:r1, c0:c1] = a[r0:r1, c0:c1]
    return out


def oracle(u, q, coef, box, k):
    """(level k on the box, level k-1 on the box): k steps of step_np_fma, step
    j over the box grown by k-1-j and clipped to the plate, every other cell
    kept.  u and q may hold NaN outside what the contract lets the kernel read."""
    r0, r1, c0, c1 = box
    prev, cur = None, np.asarray(u, np.float32)
    for j in range(k):
        b = grown(box, k - 1 - j, u.shape)
        full = R.step_np_fma(cur, coef[0], coef[1], source=q)
        prev, cur = cur, cur.copy()
        cur[b[0]:b[1], b[2]:b[3]] = full[b[0]:b[1], b[2]:b[3]]
    return cur[r0:r1, c0:c1], prev[r0:r1, c0:c1]


def to_buffer(f, a, gx0, gy0):
    """The field's whole buffer as a NumPy array: plate array a wherever a cell
    lies on the plate, NaN elsewhere."""
    rows, cols = f.data.shape
    nx, ny = a.shape
    pi = np.arange(rows) - f.hx + gx0
    pj = np.arange(cols) - f.hy + gy0
    on = ((pi >= 0) & (pi < nx))[:, None] & ((pj >= 0) & (pj < ny))[None, :]
    host = np.full((rows, cols), np.nan, np.float32)
    host[on] = a[np.clip(pi, 0, nx - 1)[:, None], np.clip(pj, 0, ny - 1)[None, :]][on]
    return host


def run_tb(device, plate, coef, kind, k, block=None, box=None, raw=None, q_off=None, seed=0,
           q_plate=None, resid0=None, gate=None):
    """k fused steps of the block (gx0, gy0, lx, ly) of a plate (default: the
    whole plate) over `box` (local; default: the block).  src holds the plate's
    values in the box grown by k (clipped to the plate) and NaN everywhere
    else, q its values in the box grown by k-1 and NaN everywhere else, dst is
    SENTINEL.  Returns (dst's whole buffer, the box's index slices in it, the
    oracle's level k and level k-1 on the box, the residual word or None)."""
    nx, ny = plate
    gx0, gy0, lx, ly = block or (0, 0, nx, ny)
    r0, r1, c0, c1 = box or (0, lx, 0, ly)
    pbox = (gx0 + r0, gx0 + r1, gy0 + c0, gy0 + c1)
    u = framed(values(kind, plate, seed), grown(pbox, k, plate))
    # A source of the field's own magnitude, so that the add rounds.
    q = values(kind, plate, seed + 1000) if q_plate is None else np.asarray(q_plate, np.float32)
    q = framed(q, grown(pbox, k - 1, plate))
    src, dst, qf = fields(device, lx, ly, k, raw, q_off)
    host = to_buffer(src, u, gx0, gy0)
    src.data.copy_(torch.from_numpy(host))
    qf.data.copy_(torch.from_numpy(to_buffer(qf, q, gx0, gy0)))
    word = None
    if resid0 is not None:
        word = torch.tensor([resid0], dtype=torch.int64).to(torch.int32).to(src.device)
    geom = ops.Geom(nx, ny, gx0, gy0, coef[0], coef[1])
    ops.source_tb_step(src, dst, qf, geom, (r0, r1, c0, c1), k, resid=word, gate=gate)
    want, old = oracle(u, q, coef, pbox, k)
    after = src.data.cpu().numpy()
    assert np.array_equal(bits(after), bits(host)), "src was written"
    bi = slice(dst.hx + r0, dst.hx + r1)
    bj = slice(dst.hy + c0, dst.hy + c1)
    return (dst.data.cpu().numpy(), (bi, bj), want, old,
            None if word is None else int(word.cpu()[0]) & 0xFFFFFFFF)


def expected_word(want, old):
    with np.errstate(invalid="ignore", over="ignore"):
        return word_of(np.max(np.abs(want - old)) if want.size else np.float32(0))


def check_tb(device, plate, coef, kind, k, what=None, **kw):
    """The box holds the oracle's level k bit for bit, every other cell of dst
    is still SENTINEL, src is untouched, and the residual word is NumPy's
    max |u_k - u_(k-1)| over the box."""
    what = what or (plate, coef, kind, k, kw)
    got, (bi, bj), want, old, word = run_tb(device, plate, coef, kind, k, resid0=0, **kw)
    assert_bitwise(got[bi, bj], want, what)
    rest = got.copy()
    rest[bi, bj] = SENTINEL
    assert np.all(rest == np.float32(SENTINEL)), (what, "a cell outside the box was written")
    assert word == expected_word(want, old), (what, "residual", hex(word))
    return got


# (rows, columns, c0, c1, k) of boxes for the planner's invariants: narrow and
# wide, aligned and not, a strip's width and one more, tall and flat.
PLAN_SHAPES = [(1, 1, 0, 1, 2), (37, 53, 0, 53, 2), (37, 53, 3, 50, 3), (13, 519, 0, 519, 8),
               (513, 517, 0, 517, 8), (70, 248, 1, 249, 2), (70, 249, 2, 251, 4),
               (300, 240, 5, 245, 8), (300, 241, 7, 248, 7), (8192, 8192, 0, 8192, 8),
               (1024, 8192, 8, 8200, 4), (33, 1000, 9, 1009, 5)]


class FakeField:
    """Addresses only: what the planner looks at (no memory behind them)."""

    def __init__(self, lx, ly, pitch, addr):
        self.lx, self.ly, self.pitch, self.addr = lx, ly, pitch, addr

    def ptr(self):
        return self.addr


def check_plan(rows, cols, c0, c1, k, cap, phase=0, pitch=None):
    """The invariants of source_tb_plan under a cap of `cap` waves: the strips'
    stored columns tile [c0 - align, ...) past c1, the chunks tile the rows,
    every strip keeps at least k unstored columns per side, and the launch has
    at most `cap` waves."""
    pitch = pitch or -(-(c1 + 16) // 64) * 64
    base = 1 << 20
    f = FakeField(rows, cols, pitch, base + 4 * phase)
    ops.set_source_tb_max_waves(cap)
    try:
        p = ops.source_tb_plan(f, f, f, (0, rows, c0, c1), k)
    finally:
        ops.set_source_tb_max_waves(0)
    what = ((rows, cols, c0, c1, k, cap, phase, pitch), p)
    assert p["strip_cols"] == STRIP_COLS and p["max_depth"] == 8, what
    assert p["overlap"] == overlap(k) >= k and p["strip_stride"] == stride(k), what
    assert p["vector_rows"] == int(pitch % 4 == 0), what
    assert p["align"] == ((phase + c0) % 4 if pitch % 4 == 0 else 0), what
    # Strip s stores columns [c0 - align + s W, c0 - align + (s + 1) W).
    W = p["strip_stride"]
    assert (p["strips"] - 1) * W < c1 - c0 + p["align"] <= p["strips"] * W, what
    # It loads `overlap` more on each side: a whole 256-column strip.
    assert W + 2 * p["overlap"] == STRIP_COLS, what
    assert (p["chunks"] - 1) * p["chunk_rows"] < rows <= p["chunks"] * p["chunk_rows"], what
    assert p["chunk_rows"] <= p["max_chunk_rows"], what
    assert p["units"] == p["strips"] * p["chunks"], what
    assert p["waves"] == min(p["units"], cap), what
    # Chunks shorter than min_chunk_rows would spend most rows on the 2k-row ramp.
    assert p["chunk_rows"] >= min(rows, p["min_chunk_rows"]), what
    return p
