"""Pure NumPy / PyTorch reference of the heat model (the test oracle).

Mirrors the reference programs' semantics:
  * ``inidat``  (``cuda/cuda_heat.cu:274-280``): u = ix*(nx-ix-1)*iy*(ny-iy-1) in int32
  * the 5-point update with fixed boundary (``cuda/cuda_heat.cu:57-65``,
    ``mpi/mpi_heat_improved_persistent_stat.c:166-174``)
  * the convergence test every C steps (``cuda/cuda_heat.cu:219-236``,
    ``mpi/...c:235-262``) with the canonical / mpi / cuda schedules.

Three evaluations of the update:
  * ``step_np`` / ``step_torch``: plain float32, every operation rounded on
    its own.  The native engine contracts the expression into FMAs, so these
    agree with it to within a few float32 ulps per step, not bitwise.
  * ``step_np_fma``: the engine's default numerics (``heat::stencil``,
    csrc/include/heat/init_fn.hpp) bit for bit.  NumPy has no fused
    multiply-add; ``fma32`` emulates a correctly rounded fp32 one in float64
    (exact product, TwoSum error term, round-to-odd, one rounding to fp32).
    It shares no code with the engine, so it is the independent exact oracle
    of every kernel and backend (``run_np(numerics="fma")``).
  * ``step_np_mpi``: the reference MPI program's double arithmetic
    (``numerics="mpi"``), exact as well.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

_U64 = np.uint64


def _mix64(z: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        z = z + _U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U64(27))) * _U64(0x94D049BB133111EB)
        return z ^ (z >> _U64(31))


def init_grid(nx: int, ny: int, mode: str = "ref-wrap", seed: int = 0,
              ox: int = 0, oy: int = 0, lx: Optional[int] = None,
              ly: Optional[int] = None) -> np.ndarray:
    """Initial condition for the block [ox, ox+lx) x [oy, oy+ly) of an nx x ny plate."""
    lx = nx - ox if lx is None else lx
    ly = ny - oy if ly is None else ly
    ix = np.arange(ox, ox + lx, dtype=np.int64)[:, None]
    iy = np.arange(oy, oy + ly, dtype=np.int64)[None, :]
    if mode == "ref-wrap":
        with np.errstate(over="ignore"):
            a = (ix.astype(np.uint32) * (nx - ix - 1).astype(np.uint32))
            a = a * iy.astype(np.uint32)
            a = a * (ny - iy - 1).astype(np.uint32)
        return a.astype(np.uint32).view(np.int32).astype(np.float32)
    if mode in ("exact", "ref64"):
        return (ix.astype(np.float64) * (nx - ix - 1) * iy * (ny - iy - 1)).astype(np.float32)
    if mode == "random":
        s = _U64(seed)
        with np.errstate(over="ignore"):
            inner = _mix64(ix.astype(np.uint64) * _U64(0x9E3779B97F4A7C15) ^ iy.astype(np.uint64))
            h = _mix64(s * _U64(0xD1B54A32D192ED03) ^ inner)
        v = (h >> _U64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0) * np.float32(100.0)
        return v.astype(np.float32)
    if mode == "zero":
        return np.zeros((lx, ly), np.float32)
    raise ValueError(mode)


def checksum_np(block: np.ndarray, ox: int = 0, oy: int = 0, ny: Optional[int] = None) -> dict:
    """The engine's checksum of a block whose cell (0, 0) is cell (ox, oy) of a
    plate with `ny` columns (default: the block's own), computed independently:
    hash = sum of mix64(global index * 0x100000001B3 ^ float bits) mod 2^64
    over uint64 arrays, count / min / max from the float values (NaN as NumPy
    orders it: it wins both), sum from math.fsum (exactly rounded, so any
    summation order of the engine lies within the fp64 worst-case bound of
    it).  Same keys as ops.checksum."""
    import math

    b = np.ascontiguousarray(block, np.float32)
    lx, ly = b.shape
    ny = ly if ny is None else int(ny)
    with np.errstate(over="ignore"):
        gidx = ((_U64(ox) + np.arange(lx, dtype=np.uint64))[:, None] * _U64(ny)
                + (_U64(oy) + np.arange(ly, dtype=np.uint64))[None, :])
        h = _mix64(gidx * _U64(0x100000001B3) ^ b.view(np.uint32).astype(np.uint64))
        total = int(np.add.reduce(h.ravel(), dtype=np.uint64)) if h.size else 0
    vals = b.astype(np.float64).ravel().tolist()
    with np.errstate(invalid="ignore"):
        mn = float(b.min()) if b.size else float("inf")
        mx = float(b.max()) if b.size else float("-inf")
    try:
        s = math.fsum(vals)
    except (OverflowError, ValueError):  # +inf and -inf both present, or overflow
        with np.errstate(invalid="ignore", over="ignore"):
            s = float(np.sum(b.astype(np.float64)))
    return {"hash": total, "sum": s, "min": mn, "max": mx, "count": int(b.size)}


def coarse_np(grid: np.ndarray, fx: int, fy: int) -> dict:
    """Coarse view of a full grid, NumPy only: coarse cell (I, J) covers rows
    [I*fx, (I+1)*fx) and columns [J*fy, (J+1)*fy), cut at the grid's edge.
    {"sum": float64 (np.add.reduceat over float64 copies), "min", "max":
    float32 (np.minimum / np.maximum.reduceat: a NaN wins, as in np.min),
    "count": int64 cells per coarse cell}, each (ceil(nx/fx), ceil(ny/fy)).
    Shares no code with the engine."""
    g = np.ascontiguousarray(grid, np.float32)
    nx, ny = g.shape
    fx, fy = int(fx), int(fy)
    if fx < 1 or fy < 1:
        raise ValueError(f"coarse factors {fx}x{fy}: a factor must be >= 1")
    r0 = np.arange(0, nx, fx)
    c0 = np.arange(0, ny, fy)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.add.reduceat(np.add.reduceat(g.astype(np.float64), r0, axis=0), c0, axis=1)
        mn = np.minimum.reduceat(np.minimum.reduceat(g, r0, axis=0), c0, axis=1)
        mx = np.maximum.reduceat(np.maximum.reduceat(g, r0, axis=0), c0, axis=1)
    rows = np.minimum(r0 + fx, nx) - r0
    cols = np.minimum(c0 + fy, ny) - c0
    return {"sum": s, "min": mn, "max": mx,
            "count": (rows[:, None] * cols[None, :]).astype(np.int64)}


_SIDES = "nswe"  # north = row 0, south = last row, west = column 0, east = last column


def insulated_sides(insulated: str) -> str:
    """"" | any subset of "nswe" | "all" -> the letters, validated."""
    if insulated == "all":
        return _SIDES
    if any(c not in _SIDES for c in insulated):
        raise ValueError(f"insulated={insulated!r}; expected 'all' or any of the letters {_SIDES!r}")
    return insulated


_AXES = "xy"  # x: rows (north and south edges joined), y: columns (west and east joined)


def periodic_axes(periodic: str) -> str:
    """"" | "x" | "y" | "xy" -> the letters, validated."""
    if any(c not in _AXES for c in periodic):
        raise ValueError(f"periodic={periodic!r}; expected any of the letters {_AXES!r}")
    return periodic


def _edge_pads(insulated: str, periodic: str):
    """Per axis (rows, columns): (cells padded before, after, np.pad mode)."""
    ins, per = insulated_sides(insulated), periodic_axes(periodic)
    pads = []
    for axis, (lo, hi) in zip(_AXES, ("ns", "we")):
        if axis in per:
            if lo in ins or hi in ins:
                raise ValueError(f"axis {axis} is periodic and has an insulated side")
            pads.append((1, 1, "wrap"))
        else:
            pads.append((int(lo in ins), int(hi in ins), "reflect"))
    return pads


def _edge_step(step, u, cx, cy, insulated, periodic="", source=None):
    """One step with insulated (zero-flux) sides, the second-order mirror
    scheme, and periodic axes: the grid is padded by one cell beyond every
    insulated side with its reflection across the edge row / column
    (u[-1, j] := u[1, j], the edge cell not repeated; a corner between two
    insulated sides takes both) and beyond both ends of every periodic axis
    with the cell at the other end (u[-1, j] := u[nx-1, j], u[nx, j] :=
    u[0, j]; an axis of extent 1 pads with itself), axis by axis, the
    Dirichlet step runs on the padded grid, whose ring it leaves fixed, and
    the padding is cropped.  Edge cells of such a side are thereby updated
    like interior cells; a corner shared with a Dirichlet side lies on the
    padded grid's ring and stays fixed."""
    (n0, n1, mx), (w0, w1, my) = _edge_pads(insulated, periodic)
    u = np.asarray(u, np.float32)
    p = np.pad(u, ((n0, n1), (0, 0)), mode=mx)
    p = np.pad(p, ((0, 0), (w0, w1)), mode=my)
    pad = ((n0, n1), (w0, w1))
    if source is None:
        v = step(p, cx, cy)
    else:  # the padding cells' source: that of the plate cells they stand for
        q = np.pad(np.asarray(source, np.float32), ((n0, n1), (0, 0)), mode=mx)
        v = step(p, cx, cy, source=np.pad(q, ((0, 0), (w0, w1)), mode=my))
    return np.ascontiguousarray(v[pad[0][0]:v.shape[0] - pad[0][1], pad[1][0]:v.shape[1] - pad[1][1]])


def step_np(u: np.ndarray, cx: float = 0.1, cy: float = 0.1, insulated: str = "",
            periodic: str = "") -> np.ndarray:
    """One Jacobi step in float32; boundary ring unchanged, except along the
    `insulated` sides (letters of "nswe", or "all") and the `periodic` axes
    (letters of "xy"); see _edge_step."""
    if insulated or periodic:
        return _edge_step(step_np, u, cx, cy, insulated, periodic)
    u = np.asarray(u, np.float32)
    out = u.copy()
    if u.shape[0] < 3 or u.shape[1] < 3:
        return out
    c = u[1:-1, 1:-1]
    n, s = u[:-2, 1:-1], u[2:, 1:-1]
    w, e = u[1:-1, :-2], u[1:-1, 2:]
    two = np.float32(2.0)
    tx = (s + n) - two * c
    ty = (e + w) - two * c
    out[1:-1, 1:-1] = (c + np.float32(cx) * tx) + np.float32(cy) * ty
    return out


def fma32(a, b, c) -> np.ndarray:
    """Correctly rounded float32 fused multiply-add ``a * b + c`` on arrays
    (what C's ``fmaf`` and the GPU's ``v_fma_f32`` compute, subnormals kept).

    The float64 product of two float32 values is exact (48 significant bits,
    exponents within range).  Adding ``c`` in float64 rounds once; rounding
    that sum to float32 would round twice and go wrong near float32 ties.  So
    the sum is first forced to round-to-odd: TwoSum gives the exact error of
    the float64 addition, and an inexact sum with an even last mantissa bit is
    moved to its odd neighbour on the side of the error.  A round-to-odd value
    with >= 2 bits more than the target format rounds to the target exactly as
    the infinitely precise sum would (float64 has 29 more than float32, and
    still more where the float32 result is subnormal)."""
    a = np.asarray(a, np.float32).astype(np.float64)
    b = np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        bb = s - p                       # TwoSum (Knuth): s + err == p + c exactly
        err = (p - (s - bb)) + (c - bb)
        s, err = np.broadcast_arrays(s, err)
        even = (s.view(np.int64) & 1) == 0
        fix = (err != 0) & np.isfinite(s) & even   # inf / NaN sums pass through
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
        return s.astype(np.float32)


def refine_axis_np(n: int, f: int, order: int = 1, wrap: bool = False):
    """The refinement table of an axis of n cells refined by the factor f,
    NumPy only: (i0, i1) int32 source indices and w float32 for every index.
    Source cell I covers [I*f, min((I+1)*f, n)); twice its centre is
    c2_I = lo + hi - 1.  Order 0: i0 = i1 = i // f, w = 0.  Order 1: with
    t = 2i and k the largest I with c2_I <= t (-1 if none), an index between
    two centres gets (k, k+1, (t - c2_k) / (c2_{k+1} - c2_k)); one outside them
    clamps to the nearest cell with w = 0, or with `wrap` (and more than one
    cell) gets (C-1, 0, (t - c2_{C-1} [+ 2n if k < 0]) / (c2_0 + 2n - c2_{C-1})).
    The quotient is taken in float64 and rounded once to float32."""
    n, f, order = int(n), int(f), int(order)
    if n < 1 or f < 1 or order not in (0, 1):
        raise ValueError(f"refine axis: n {n}, factor {f}, order {order}")
    i = np.arange(n, dtype=np.int64)
    if order == 0:
        k = (i // f).astype(np.int32)
        return k, k.copy(), np.zeros(n, np.float32)
    C = -(-n // f)
    I = np.arange(C, dtype=np.int64)
    c2 = I * f + np.minimum((I + 1) * f, n) - 1
    t = 2 * i
    k = np.searchsorted(c2, t, side="right") - 1
    i0 = np.clip(k, 0, C - 1)
    i1 = i0.copy()
    w = np.zeros(n, np.float64)
    inner = (k >= 0) & (k < C - 1)
    ki = k[inner]
    i1[inner] = ki + 1
    w[inner] = (t[inner] - c2[ki]).astype(np.float64) / (c2[ki + 1] - c2[ki]).astype(np.float64)
    if wrap and C > 1:
        outer = ~inner
        i0[outer] = C - 1
        i1[outer] = 0
        num = t[outer] - c2[C - 1] + np.where(k[outer] < 0, 2 * n, 0)
        w[outer] = num.astype(np.float64) / np.float64(c2[0] + 2 * n - c2[C - 1])
    return i0.astype(np.int32), i1.astype(np.int32), w.astype(np.float32)


def _lerp32(a, b, w) -> np.ndarray:
    """(w == 0) ? a : fmaf(w, b - a, a) in float32; the select keeps a's bits."""
    a, b, w = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32),
                                  np.asarray(w, np.float32))
    with np.errstate(invalid="ignore", over="ignore"):
        d = b - a
        return np.where(w == 0, a, fma32(w, d, a))


def refine_np(S: np.ndarray, nx: int, ny: int, fx: int, fy: int, order: int = 1,
              periodic: str = "") -> np.ndarray:
    """The nx x ny plate refined from the (ceil(nx/fx), ceil(ny/fy)) source grid
    S, NumPy only, bit for bit what the engine's refine gives: piecewise
    constant (order 0) or cell-centred bilinear (order 1), an axis in
    `periodic` wrapping, the others clamping.  With the tables of
    refine_axis_np, in float32, columns first:
        top = lerp(S[i0, j0], S[i0, j1], wy);  bot = lerp(S[i1, j0], S[i1, j1], wy)
        u = lerp(top, bot, wx),   lerp(a, b, w) = a if w == 0 else fma(w, b - a, a)"""
    S = np.ascontiguousarray(S, np.float32)
    nx, ny, fx, fy = int(nx), int(ny), int(fx), int(fy)
    per = periodic_axes(periodic)
    if fx < 1 or fy < 1 or S.ndim != 2 or S.shape != (-(-nx // fx), -(-ny // fy)):
        raise ValueError(f"refine: a {S.shape} source grid does not fit factors {fx}x{fy} on a "
                         f"{nx}x{ny} plate")
    i0, i1, wx = refine_axis_np(nx, fx, order, "x" in per)
    j0, j1, wy = refine_axis_np(ny, fy, order, "y" in per)
    top = _lerp32(S[i0][:, j0], S[i0][:, j1], wy[None, :])
    bot = _lerp32(S[i1][:, j0], S[i1][:, j1], wy[None, :])
    return np.ascontiguousarray(_lerp32(top, bot, wx[:, None]))


def step_np_fma(u: np.ndarray, cx: float = 0.1, cy: float = 0.1,
                insulated: str = "", periodic: str = "", *,
                source: Optional[np.ndarray] = None) -> np.ndarray:
    """One step with the engine's default numerics, bit for bit: the
    expression of ``heat::stencil`` with the same operands in the same order,
        tx = fma(-2, c, s + n);  ty = fma(-2, c, e + w)
        u' = fma(cy, ty, fma(cx, tx, c))
    (n / s: rows above / below, w / e: columns left / right; cx and cy rounded
    to float32 first, as HeatParams carries them); boundary ring unchanged,
    except along the `insulated` sides (mirror scheme, _edge_step: the same
    expression, the missing neighbour being the cell's mirror image) and the
    `periodic` axes (the missing neighbour: the cell at the other end).
    `source`: a per-cell heat source q of u's shape; every cell the step
    updates becomes (u' + q) rounded to float32, one more rounded add after the
    expression, and a fixed cell ignores it."""
    if insulated or periodic:
        return _edge_step(step_np_fma, u, cx, cy, insulated, periodic, source)
    u = np.asarray(u, np.float32)
    out = u.copy()
    if source is not None and np.shape(source) != u.shape:
        raise ValueError(f"source shape {np.shape(source)} != grid shape {u.shape}")
    if u.shape[0] < 3 or u.shape[1] < 3:
        return out
    c = u[1:-1, 1:-1]
    with np.errstate(over="ignore", invalid="ignore"):
        ns = u[2:, 1:-1] + u[:-2, 1:-1]     # s + n, float32
        ew = u[1:-1, 2:] + u[1:-1, :-2]     # e + w, float32
    m2 = np.float32(-2.0)
    tx = fma32(m2, c, ns)
    ty = fma32(m2, c, ew)
    out[1:-1, 1:-1] = fma32(np.float32(cy), ty, fma32(np.float32(cx), tx, c))
    if source is not None:
        with np.errstate(over="ignore", invalid="ignore"):
            out[1:-1, 1:-1] = (out[1:-1, 1:-1]
                               + np.asarray(source, np.float32)[1:-1, 1:-1]).astype(np.float32)
    return out


def step_np_mpi(u: np.ndarray, cx: float = 0.1, cy: float = 0.1,
                insulated: str = "", periodic: str = "") -> np.ndarray:
    """One step with the reference MPI program's arithmetic
    (mpi/mpi_heat_improved_persistent_stat.c:168-174): the two neighbour sums
    in float32 (float + float in C), the rest in float64 because of the 2.0
    literal, evaluated left to right, rounded to float32 once.  NumPy float64
    ops are IEEE and never fused, so this is the exact oracle of
    `numerics="mpi"`.  `insulated`, `periodic`: as step_np."""
    if insulated or periodic:
        return _edge_step(step_np_mpi, u, cx, cy, insulated, periodic)
    u = np.asarray(u, np.float32)
    out = u.copy()
    if u.shape[0] < 3 or u.shape[1] < 3:
        return out
    c = u[1:-1, 1:-1].astype(np.float64)
    ns = (u[2:, 1:-1] + u[:-2, 1:-1]).astype(np.float64)   # float32 add, then widen
    ew = (u[1:-1, 2:] + u[1:-1, :-2]).astype(np.float64)
    fcx, fcy = float(np.float32(cx)), float(np.float32(cy))  # parms are float
    a = c + fcx * (ns - 2.0 * c)
    out[1:-1, 1:-1] = (a + fcy * (ew - 2.0 * c)).astype(np.float32)
    return out


def step_torch(u: torch.Tensor, cx: float = 0.1, cy: float = 0.1,
               insulated: str = "", periodic: str = "") -> torch.Tensor:
    """The same step as plain PyTorch fp32 ops (any device).  `insulated`,
    `periodic`: as step_np."""
    if insulated or periodic:
        (n0, n1, mx), (w0, w1, my) = _edge_pads(insulated, periodic)
        p = u
        if mx == "wrap":
            p = torch.cat([p[-1:], p, p[:1]], 0)
        else:
            if n0:
                p = torch.cat([p[1:2], p], 0)
            if n1:
                p = torch.cat([p, p[-2:-1]], 0)
        if my == "wrap":
            p = torch.cat([p[:, -1:], p, p[:, :1]], 1)
        else:
            if w0:
                p = torch.cat([p[:, 1:2], p], 1)
            if w1:
                p = torch.cat([p, p[:, -2:-1]], 1)
        v = step_torch(p, cx, cy)
        return v[n0:v.shape[0] - n1, w0:v.shape[1] - w1].clone()
    out = u.clone()
    if u.shape[0] < 3 or u.shape[1] < 3:
        return out
    c = u[1:-1, 1:-1]
    tx = (u[2:, 1:-1] + u[:-2, 1:-1]) - 2.0 * c
    ty = (u[1:-1, 2:] + u[1:-1, :-2]) - 2.0 * c
    out[1:-1, 1:-1] = (c + cx * tx) + cy * ty
    return out


def check_points(total: int, interval: int, compat: str = "none"):
    """Completed-step counts after which a convergence check happens."""
    if compat == "cuda":
        return [c for c in range(1, total + 1) if (c - 1) % interval == 0]
    return [c for c in range(1, total + 1) if c % interval == 0]


def run_np(nx: int, ny: int, steps: int, cx: float = 0.1, cy: float = 0.1,
           converge: bool = False, check_interval: int = 20, eps: float = 1e-3,
           compat: str = "none", init: str = "ref-wrap", seed: int = 0,
           u0: Optional[np.ndarray] = None,
           numerics: str = "fp32", insulated: str = "",
           periodic: str = "", *,
           source: Optional[np.ndarray] = None) -> Tuple[np.ndarray, int, int]:
    """Run the model; returns (grid, steps_done, converged_at or -1).
    numerics: "fp32" (plain float32, a few ulps from the engine), "fma" (the
    engine's default numerics, exact) or "mpi" (its numerics="mpi", exact).
    insulated: the plate's insulated (zero-flux) sides, letters of "nswe" or
    "all"; periodic: its periodic axes, letters of "xy"; the residual then
    covers their edge cells too.  source: a full-plate per-cell heat source
    (step_np_fma's; from refine_np for a source map), numerics "fma" only."""
    step = {"fp32": step_np, "fma": step_np_fma, "mpi": step_np_mpi}[numerics]
    if source is not None:
        if numerics != "fma":
            raise ValueError("a source needs numerics='fma'")
        q = np.ascontiguousarray(source, np.float32)

        def step(u, cx, cy, insulated="", periodic=""):  # noqa: F811
            return step_np_fma(u, cx, cy, insulated, periodic, source=q)
    u = init_grid(nx, ny, init, seed) if u0 is None else np.array(u0, np.float32)
    total = steps + 1 if compat == "mpi" else steps
    checks = set(check_points(total, check_interval, compat)) if converge else set()
    for k in range(1, total + 1):
        v = step(u, cx, cy, insulated, periodic) if insulated or periodic else step(u, cx, cy)
        if k in checks:
            r = float(np.max(np.abs(v - u))) if v.size else 0.0
            ok = r <= eps if compat == "mpi" else r < np.float32(eps)
            if ok:
                return v, k, k
        u = v
    return u, total, -1
