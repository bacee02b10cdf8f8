"""Coverage of the fused residual of every HIP kernel family: the hot cell
of tests/hot_cell.py visits every row and every column of the launch's box,
and the cells just outside it, and the kernel's residual word must equal the
exact oracle's at every position.

The other GPU tests compare the word on random data, where the maximum sits
in one arbitrary cell per seed: a kernel that leaves out the last row of each
chunk, one element of the last partial lane, one wave of a workgroup or one
stage's levels, or that counts a spill column or a ghost row holding valid
data, passes them.  Here the hot cell holds the maximum wherever it is (the
runner-up at most 2/3 of it), the levels of a pass are pairwise distinct, and
with q one cell outside the box the box's maximum is 1/3 to 1/6 of what a
residual looking one cell too far reports.

A sweep allocates its fields once and is stream-ordered per position (write
C + H into q, launch with that position's residual word, write C back); one
synchronisation at the end, one exact comparison of the whole vector, every
failing position reported.  Needs an MI355X."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from parallel_heat_amd import ops

from . import hot_cell as Hc
from .test_gpu_coefficients import (DEEP, STREAM, TILE, TILE_DPP, TILES, K, V, _field, _p, tb)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("exp_kernels")]

N = 12            # levels of the oracle's tables (the deepest pass)
HALO = 4          # thinnest ghost ring swept: the frame reaches 2 rows, 4 columns out

RESID = _p("residual", K("residual"))
NAIVE, LDS, MFMA = _p("naive", K("naive")), _p("lds", K("lds")), _p("mfma", K("mfma"))
LDS_MPI = _p("lds_mpi", K("lds_mpi"))
SINGLE = [NAIVE, LDS, LDS_MPI, RESID, MFMA]
DEEP12 = [_p("DEEP@12", tb(DEEP, 12)), _p("DEEP_nt1@12", tb(DEEP, 12, nt=1))]
DEEP_PLANS = [_p("DEEP_LINEAR@12", tb(DEEP | V.LINEAR, 12)),
              _p("DEEP_ALT@12", tb(DEEP | V.ALT_DIRECTION, 12)),
              _p("DEEP_AGE_PAIRS@12", tb(DEEP | V.FORCE_AGE_PAIRS, 12))]
TILES12 = [_p(f"{n}_{r}x{w}", tb(v, 12, tile_rows=r, tile_waves=w))
           for n, v in (("TILE", TILE), ("TILE_DPP", TILE_DPP))
           for r, w in ((12, 8), (20, 8), (12, 16))]


def _seam(k):
    """Last column of the first strip of k's launches (the streaming kernels'
    strips: 64 lanes less two ghost zones; the tiles' and the single-step
    kernels' blocks end elsewhere, every column is swept anyway)."""
    if k.kind != "tb":
        return 231
    lane = 2 if k.variant & V.FLOAT2 else 4
    return 64 * lane - 2 * (-(-k.depth // lane) * lane) - 1


class Geo:
    """A block (ox, oy, lx, ly) of an nx x ny hot-cell plate."""

    def __init__(self, name, shape, block=None):
        self.name, self.shape = name, shape
        self.block = block or (0, 0) + shape

    def fields(self, k, dev):
        halo = max(k.depth, HALO)
        full = Hc.plate(*self.shape)
        return _field(full, dev, halo, self.block), _field(full, dev, halo, self.block)

    def plate_box(self, box=None):
        ox, oy, lx, ly = self.block
        r0, r1, c0, c1 = box or (0, lx, 0, ly)
        return (ox + r0, ox + r1, oy + c0, oy + c1)

    def cross(self, k):
        ox, oy, lx, ly = self.block
        return Hc.cross(lx, ly, (1, _seam(k), ly - 2), (1, lx // 2, lx - 2), ox, oy)

    def frame(self):
        ox, oy, lx, ly = self.block
        return Hc.frame(lx, ly, ox, oy)


PLATE = Geo("plate", (203, 517))                          # (a) masked paths, partial last lane
BLOCK = Geo("block", (120, 700), (30, 256, 50, 301))     # (b) unmasked; ly % 4 == 1
SEAMS = Geo("seams", (120, 700), (30, 256, 50, 300))     # (c) the solver's five boxes


@functools.lru_cache(maxsize=None)
def _table(geo, positions, box, numerics="fma", coef=Hc.COEF):
    t = Hc.resid_table(geo.shape, positions, box, N, coef=coef, numerics=numerics)
    t.setflags(write=False)
    return t


@contextlib.contextmanager
def _tuned(k):
    saved = ops.tb_tuning()
    try:
        if k.tune:
            t = ops.tb_tuning()
            for name, v in k.tune.items():
                setattr(t, name, v)
            ops.set_tb_tuning(t)
        yield
    finally:
        ops.set_tb_tuning(saved)


def _launch(k, a, b, g, resid, boxes, res_level, waves):
    """One residual of k over `boxes` (local; None: the owned block) into the
    one-word tensor `resid`.  No synchronisation."""
    if k.kind == "tb":
        ops.tb_step(a, b, g, k.depth, boxes=boxes, resid=resid, waves_target=waves,
                    variant=k.variant, res_level=res_level)
        return
    for box in boxes or [None]:
        if k.kind == "naive":
            ops.naive_step(a, b, g, box, resid=resid)
        elif k.kind == "lds":
            ops.lds_step(a, b, g, box, resid=resid)
        elif k.kind == "lds_mpi":
            ops.lds_step(a, b, g, box, resid=resid, numerics="mpi")
        elif k.kind == "mfma":
            ops.mfma_step(a, b, g, box, resid=resid)
        else:
            ops.residual(a, b, box, resid=resid)


def _sweep(k, geo, dev, positions, boxes=None, box=None, res_level=0, waves=0, coef=Hc.COEF,
           what=""):
    """The hot cell at each of `positions` (plate coordinates): k's residual
    over `boxes` must be the oracle's over `box` (local; default: the block)
    at level res_level (default: the launch's last)."""
    positions = tuple(positions)
    ox, oy, lx, ly = geo.block
    g = ops.Geom(nx=geo.shape[0], ny=geo.shape[1], gx0=ox, gy0=oy, cx=coef[0], cy=coef[1])
    a, b = geo.fields(k, dev)
    for r, c in positions:   # inside the allocation, on the plate
        assert -a.hx <= r - ox < lx + a.hx and -a.hy <= c - oy < ly + a.hy, (r, c)
        assert 0 <= r < geo.shape[0] and 0 <= c < geo.shape[1], (r, c)
    words = torch.zeros(len(positions), dtype=torch.int32, device=dev)
    own = torch.zeros(len(positions), dtype=torch.float32, device=dev)
    hot, cold = float(Hc.C + Hc.H), float(Hc.C)
    views = boxes or [box or (0, lx, 0, ly)]
    with _tuned(k):
        for i, (r, c) in enumerate(positions):
            cell = a.view(r - ox, r - ox + 1, c - oy, c - oy + 1)
            cell.fill_(hot)
            _launch(k, a, b, g, words[i:i + 1], boxes or ([box] if box else None), res_level,
                    waves)
            if k.kind == "mfma":
                # Defined against its own output (another association than
                # heat::stencil): max |its output - its input| over the box.
                own[i] = torch.stack([(b.view(*v) - a.view(*v)).abs().max() for v in views]).max()
            cell.fill_(cold)
        torch.cuda.synchronize()
    got = words.cpu().view(torch.float32).numpy()
    if k.kind == "mfma":
        want = own.cpu().numpy()
        # Its own output stays within the mfma tests' bound of the oracle's.
        ref = _table(geo, positions, geo.plate_box(box))[:, 0]
        assert np.allclose(want, ref, rtol=0, atol=2e-5), float(np.abs(want - ref).max())
    elif k.kind == "residual":
        pb = geo.plate_box(box)
        want = np.array([Hc.H if pb[0] <= r < pb[1] and pb[2] <= c < pb[3] else 0
                         for r, c in positions], np.float32)
    else:
        numerics = "mpi" if k.kind == "lds_mpi" else "fma"
        level = res_level or max(k.depth, 1)
        want = _table(geo, positions, geo.plate_box(box), numerics, coef)[:, level - 1]
    Hc.assert_words(got, want, positions, f"{what or geo.name} level {res_level or k.depth}")


# -- (a) the full plate, (b) a block with valid ghosts all around -------------------

@pytest.mark.parametrize("k", SINGLE + STREAM + TILES)
def test_plate_every_row_and_column(gpu, k):
    _sweep(k, PLATE, gpu, PLATE.cross(k))


@pytest.mark.parametrize("k", SINGLE + STREAM + TILES)
def test_block_every_row_and_column_and_frame(gpu, k):
    # The unmasked paths; three spill elements of the last lane and the rows
    # above and below the block are valid cells the residual must not count.
    _sweep(k, BLOCK, gpu, BLOCK.cross(k) + BLOCK.frame())


@pytest.mark.parametrize("k", [NAIVE, LDS, _p("DEF@8", tb(V.DEFAULT, 8)), _p("DEEP@12", tb(DEEP, 12)),
                               _p("TILE_12x8@12", tb(TILE, 12, tile_rows=12, tile_waves=8))])
def test_plate_swapped_coefficients(gpu, k):
    _sweep(k, PLATE, gpu, PLATE.cross(k), coef=Hc.SWAPPED)


@pytest.mark.parametrize("waves", [6, 20])
@pytest.mark.parametrize("k", STREAM)
def test_plate_forced_chunks(gpu, k, waves):
    # Several chunks per strip, ending at rows the default plan does not
    # produce.  The plate is 3 strips of 203 rows (609 strip-rows; 5 strips,
    # 1015, with float2 lanes).  tb_step starts at ceil(609 / waves) rows per
    # chunk and lengthens it until strips x chunks <= waves:
    #   waves 6:  102 rows, 2 chunks per strip, the first ending with row 101
    #             (float2: 170 -> 284, one chunk per strip);
    #   waves 20: 31 -> 33 -> 35 rows, 6 chunks, ending with rows 34, 69, 104,
    #             139, 174 (float2: 51 rows, 4 chunks: 50, 101, 152).
    # The default plan cuts chunks of the minimum length (8 or 12 rows: last
    # rows 8 i + 7 or 12 i + 11) and the split kernels' age-group units of two
    # such chunks (depth 12: last rows 24 i + 14 and 24 i + 23): none of the
    # rows above.
    _sweep(k, PLATE, gpu, PLATE.cross(k), waves=waves)


# -- (c) the solver's five boxes, and one of them alone --------------------------

def _five(d, lx=50, ly=300):
    return [(0, d, 0, ly), (lx - d, lx, 0, ly), (d, lx - d, 0, 8), (d, lx - d, 296, ly),
            (d, lx - d, 8, 296)]


def _five_sweep(k, dev, **kw):
    # Top and bottom bands, left and right bands, interior (as in
    # test_interior_subdomain_anisotropic): one residual over their union, q
    # on both sides of every seam and in the frame around the block.
    ox, oy, lx, ly = SEAMS.block
    d = max(k.depth, 8)
    pos = [(ox + r, oy + c) for r in (0, d - 1, d, lx - d - 1, lx - d, lx - 1) for c in range(ly)]
    pos += [(ox + r, oy + c) for c in (0, 7, 8, 295, 296, ly - 1) for r in range(lx)]
    _sweep(k, SEAMS, dev, list(dict.fromkeys(pos)) + SEAMS.frame(), boxes=_five(d),
           what="five boxes", **kw)


def _sub_sweep(k, dev, **kw):
    # A box inside the block launched alone: q in owned cells just outside
    # it (285 columns: three spill elements of its last lane are owned cells).
    ox, oy, lx, ly = SEAMS.block
    d = max(k.depth, 8)
    sub = Geo("sub", SEAMS.shape, (ox + d, oy + 8, lx - 2 * d, 285))
    _sweep(k, SEAMS, dev, sub.cross(k) + sub.frame(), box=(d, lx - d, 8, 293), what="sub-box",
           **kw)


@pytest.mark.parametrize("k", SINGLE + STREAM + TILES)
def test_five_boxes_both_sides_of_every_seam(gpu, k):
    _five_sweep(k, gpu)


@pytest.mark.parametrize("k", SINGLE + STREAM + TILES)
def test_sub_box_alone_excludes_owned_cells_around_it(gpu, k):
    _sub_sweep(k, gpu)


# -- inner levels -------------------------------------------------------------------

@pytest.mark.parametrize("rl", range(1, 12))
@pytest.mark.parametrize("geo", [PLATE, BLOCK], ids=lambda g: g.name)
@pytest.mark.parametrize("k", DEEP12)
def test_split_inner_levels(gpu, k, geo, rl):
    # tb_split_rl{a,b,c}: levels 1..6 come from stage 0, 7..11 from stage 1.
    _sweep(k, geo, gpu, geo.cross(k) + (geo.frame() if geo is BLOCK else []), res_level=rl)


@pytest.mark.parametrize("rl", [3, 6, 7, 11])
@pytest.mark.parametrize("geo", [PLATE, BLOCK], ids=lambda g: g.name)
@pytest.mark.parametrize("k", DEEP_PLANS)
def test_split_plans_inner_levels(gpu, k, geo, rl):
    _sweep(k, geo, gpu, geo.cross(k) + (geo.frame() if geo is BLOCK else []), res_level=rl)


@pytest.mark.parametrize("rl", range(1, 12))
@pytest.mark.parametrize("k", DEEP12)
def test_split_inner_levels_five_boxes_and_sub_box(gpu, k, rl):
    # The solver's launches (solver.cpp compute: the four band boxes, the
    # interior box) carry the check's level: the row window of acc_mid and
    # the contributor count of the block's max run over several boxes, each
    # with its own first wave and chunk plan.
    _five_sweep(k, gpu, res_level=rl)
    _sub_sweep(k, gpu, res_level=rl)


@pytest.mark.parametrize("rl", [3, 6, 7, 11])
@pytest.mark.parametrize("k", DEEP_PLANS)
def test_split_plans_inner_levels_five_boxes_and_sub_box(gpu, k, rl):
    # Both stages' first, last and middle levels, as on the plate and block.
    _five_sweep(k, gpu, res_level=rl)
    _sub_sweep(k, gpu, res_level=rl)


@pytest.mark.parametrize("rl", [3, 7])
@pytest.mark.parametrize("k", DEEP12 + DEEP_PLANS[:1])
def test_split_inner_levels_forced_chunks(gpu, k, rl):
    # One level of each stage; chunk ends as in test_plate_forced_chunks, and
    # the boxes of the block cut by the same forced plan.
    _sweep(k, PLATE, gpu, PLATE.cross(k), res_level=rl, waves=20)
    _sweep(k, BLOCK, gpu, BLOCK.cross(k) + BLOCK.frame(), res_level=rl, waves=20)
    _five_sweep(k, gpu, res_level=rl, waves=20)
    _sub_sweep(k, gpu, res_level=rl, waves=20)


@pytest.mark.parametrize("rl", range(1, 12))
@pytest.mark.parametrize("k", TILES12)
def test_tile_inner_levels(gpu, k, rl):
    # Level 12 is TILES' own entry above.  The plate, then the block's
    # exclusion frame.
    _sweep(k, PLATE, gpu, PLATE.cross(k), res_level=rl)
    _sweep(k, BLOCK, gpu, BLOCK.frame(), res_level=rl)
