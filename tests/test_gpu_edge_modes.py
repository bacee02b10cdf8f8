"""Geometry of the HIP kernels against the independent exact oracle
(`reference.step_np_fma`): every Dirichlet edge mode, blocks next to a plate
edge, degenerate plates, and what a launch may write.

The value tests (test_gpu_coefficients.py) run six plate shapes.  Whole code
paths never ran on them:

* the right-edge modes keep ONE register element per row fixed, the element
  holding plate column ny-1: `mode = 2 + ((ny-1-gy0) & 3)` in tb_segment
  (tb_stream.inl), `kTileRight + ((ny-1-gy0) & 3)` in tile_mode
  (tb_tile_core.hpp).  The old widths give elements 0 and 3 only;
* a strip whose overlap columns reach past a plate edge that its block does
  not touch: on the left the generic path (gy0 != 0), on the right a fixed
  column held by a lane that stores nothing;
* plates narrower than a strip, shorter than the depth, without an interior,
  and widths at a strip boundary (W+1: the last strip owns only the ring);
* the tile_xl = 1 build of the tile kernel;
* the cells a launch writes: the boxes, plus at most the 3 columns up to the
  next multiple of 4 after a box's c1 (whole float4 lanes), and nothing else.

Data: the "signed" value set, cx != cy, and NaN in every cell outside the
plate, so a ring column that is updated, or a mask written as a multiply, is
NaN or off by ~10 within a step.  Every comparison is bitwise, the fused
residual included.  The one exception is the MFMA kernel: another
association of exact fp32 products (bound 2e-5 of _mfma_check, ring bitwise),
and zero ghost cells, since its banded products multiply ghost rows and
columns by zero coefficients (0 * NaN).  Needs an MI355X."""
import functools

import numpy as np
import pytest
import torch

from parallel_heat_amd import ops
from parallel_heat_amd.models import reference as R

from . import oracle_cases as O
from .oracle_cases import assert_bitwise
from .test_gpu_coefficients import (DEEP, DEF, RAMP_S, TILE, TILE_DPP, K, V, _check, _field,
                                    _mfma_check, tb)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("exp_kernels")]

CX, CY = O.ANISO
NAN = float("nan")
STEPS = 12          # the deepest pass; shallower kernels use the first states
SENTINEL = 12345.0  # no result: the data are convex combinations of [-100, 100)


def _kc(name, k, res_level=0):
    return pytest.param((k, res_level), id=name)


PRODUCT = [
    _kc("naive", K("naive")), _kc("lds", K("lds")),
    _kc("RAMP_S@3", tb(RAMP_S, 3)), _kc("RAMP_S@8", tb(RAMP_S, 8)),
    _kc("DEF@8", tb(DEF, 8)), _kc("DEF@12", tb(DEF, 12)),
    _kc("DEEP@8", tb(DEEP, 8)), _kc("DEEP@12", tb(DEEP, 12)),
    _kc("DEEP_nt1@12", tb(DEEP, 12, nt=1)),
    _kc("DEEP_LINEAR@12", tb(DEEP | V.LINEAR, 12)),
    _kc("DEEP_ALT@12", tb(DEEP | V.ALT_DIRECTION, 12)),
    _kc("DEEP@12_res5", tb(DEEP, 12), 5),
    _kc("TILE_12x8@8", tb(TILE, 8, tile_rows=12, tile_waves=8)),
    _kc("TILE_12x8@12", tb(TILE, 12, tile_rows=12, tile_waves=8)),
    _kc("TILE_20x8@8", tb(TILE, 8, tile_rows=20, tile_waves=8)),
    _kc("TILE_20x8@12", tb(TILE, 12, tile_rows=20, tile_waves=8)),
    _kc("TILE_xl1@12", tb(TILE, 12, tile_xl=1)),       # both shifts ds_bpermute (tb_tile_xl1.hip)
    _kc("TILE_DPP@12", tb(TILE_DPP, 12)),
]
EXPERIMENT = [
    _kc("RING3@8", tb(V.RING3, 8)),
    _kc("DEF_FLOAT2@8", tb(DEF | V.FLOAT2, 8)),         # mode index (ny-1-gy0) & 1
    _kc("DEEP_MIXED@12", tb(DEEP | V.SHIFT_MIXED, 12)),
]
KERNELS = PRODUCT + EXPERIMENT
# Odd and short pipelines have a ramp of their own: the degenerate plates only.
SHORT = [_kc(f"RAMP_S@{d}", tb(RAMP_S, d)) for d in (1, 2, 5)]


def _lv(nx, ny):
    """States 0..STEPS of the nx x ny plate, shared by every test (read-only)."""
    return O.levels("signed", nx, ny, CX, CY, STEPS)


@functools.lru_cache(maxsize=None)
def _edge_column_is_live(nx, ny, side):
    """On the reference alone: the plate's left / right ring column would move
    in every interior row, at every state a pass starts from or passes
    through, if a kernel updated it.  One oracle step on the plate padded by
    a zero column beyond that edge, where the former ring column is interior."""
    zero = np.zeros((nx, 1), np.float32)
    for u in _lv(nx, ny)[:STEPS]:
        padded = np.concatenate([u, zero] if side == "right" else [zero, u], axis=1)
        col = ny - 1 if side == "right" else 1
        moved = O.bits(R.step_np_fma(padded, CX, CY)[1:-1, col]) != O.bits(padded[1:-1, col])
        assert moved.all(), (nx, ny, side)
    return True


def _each(cases, fn):
    """fn(case) for every case; one assertion naming every case that failed."""
    bad = []
    for c in cases:
        try:
            fn(c)
        except AssertionError as e:
            bad.append(f"{c}: {e}")
    assert not bad, f"{len(bad)} of {len(cases)} cases failed:\n" + "\n".join(bad)


# -- a. every right-edge element on a full plate ---------------------------------------

# (ly - 1) & 3 = 3, 0, 1, 2.  With 203 rows the default plans have chunks
# clear of rows 0 and nx-1 (the pure edge modes) between a top and a bottom
# chunk on the generic path over the same column.
FULL_NX, FULL_LY = 203, (516, 517, 518, 519)


@pytest.mark.parametrize("kc", KERNELS)
def test_right_edge_elements_full_plate(gpu, kc):
    k, rl = kc

    def run(ly):
        _edge_column_is_live(FULL_NX, ly, "right")
        g = ops.Geom(nx=FULL_NX, ny=ly, cx=CX, cy=CY)
        _check(k, _lv(FULL_NX, ly), g, gpu, fill=NAN, res_level=rl)

    _each(FULL_LY, run)


def test_right_edge_elements_full_plate_mfma(gpu):
    _each(FULL_LY, lambda ly: _mfma_check("signed", O.ANISO, gpu, shape=(FULL_NX, ly)))


# -- b, c. blocks with valid ghosts: on an edge, and next to one --------------------------

# Rows 30..179 of 240: no chunk's K-window reaches a plate row for K <= 12, so
# every wave of an edge strip takes the non-generic mode it is entitled to.
NXB, OXB, LXB = 240, 30, 150


def _block(k, rl, dev, oy, ly, ny, side):
    _edge_column_is_live(NXB, ny, side)
    g = ops.Geom(nx=NXB, ny=ny, gx0=OXB, gy0=oy, cx=CX, cy=CY)
    _check(k, _lv(NXB, ny), g, dev, block=(OXB, oy, LXB, ly), fill=NAN, res_level=rl)


@pytest.mark.parametrize("kc", KERNELS)
def test_block_on_right_edge_every_element(gpu, kc):
    k, rl = kc
    _each((300, 301, 302, 303), lambda ly: _block(k, rl, gpu, 256, ly, 256 + ly, "right"))


@pytest.mark.parametrize("kc", KERNELS)
def test_block_on_left_edge(gpu, kc):
    k, rl = kc
    _block(k, rl, gpu, 0, 300, 700, "left")


@pytest.mark.parametrize("kc", KERNELS)
def test_block_d_columns_after_left_edge(gpu, kc):
    # Plate column 0 lies in the ghost ring (beyond it: NaN); gy0 = d is no
    # multiple of 4 for d = 1, 2, 3, 5: deliberately the generic path.
    k, rl = kc
    _each((1, 2, 3, 5), lambda d: _block(k, rl, gpu, d, 300, 700, "left"))


@pytest.mark.parametrize("kc", KERNELS)
def test_block_d_columns_before_right_edge(gpu, kc):
    # Plate column ny-1 is held by a lane that stores nothing; it must stay
    # fixed all the same: its value flows inward for K steps.
    k, rl = kc
    _each((1, 2, 3, 5), lambda d: _block(k, rl, gpu, 256, 300, 556 + d, "right"))


# -- d. degenerate and strip-boundary plates ------------------------------------------------

def _depth(k):
    return max(k.depth, 1)


def _strip_width(k):
    d = _depth(k)
    if k.kind == "tb" and k.variant & V.FLOAT2:
        return 128 - 2 * ((d + 1) // 2 * 2)
    return 256 - 2 * ((d + 3) // 4 * 4)


def _plates(k, rl, dev, shapes):
    def run(shape):
        g = ops.Geom(nx=shape[0], ny=shape[1], cx=CX, cy=CY)
        _check(k, _lv(*shape), g, dev, fill=NAN, res_level=rl)

    _each(sorted(set(shapes)), run)


@pytest.mark.parametrize("kc", KERNELS + SHORT)
def test_plates_of_few_rows(gpu, kc):
    k, rl = kc
    d, w = _depth(k), _strip_width(k)
    rows = [lx for lx in (1, 2, 3, 4, d - 1, d, d + 1, 2 * d, 2 * d + 1) if lx >= 1]
    _plates(k, rl, gpu, [(lx, ly) for lx in rows for ly in (37, w + 5)])


@pytest.mark.parametrize("kc", KERNELS + SHORT)
def test_plates_of_few_columns(gpu, kc):
    k, rl = kc
    _plates(k, rl, gpu, [(37, ly) for ly in (1, 2, 3, 4, 5, 7, 8, 9)] +
            [(1, 1), (2, 2), (3, 3), (3, 9), (20, 20)])


@pytest.mark.parametrize("kc", KERNELS + SHORT)
def test_plate_widths_at_strip_boundaries(gpu, kc):
    # W+1: the last strip owns only the fixed ring column; W+2: one interior
    # column and the ring.
    k, rl = kc
    w = _strip_width(k)
    _plates(k, rl, gpu, [(37, ly) for ly in (w - 1, w, w + 1, w + 2, w + 3, w + 4, w + 5, 2 * w,
                                            2 * w + 1)])


# -- e. the cells a launch writes --------------------------------------------------------------

def _launch(k, a, b, g, boxes, resid, rl):
    if k.kind in ("naive", "lds"):
        step = ops.naive_step if k.kind == "naive" else ops.lds_step
        for box in boxes:
            step(a, b, g, box=box, resid=resid)
        torch.cuda.synchronize()
    else:
        k.run(a, b, g, resid=resid, res_level=rl, boxes=boxes)


def _write_set(k, rl, dev, plate, block, boxes):
    """dst pre-filled with SENTINEL: after the launch the boxes hold the
    oracle's state, box rows x [c1, round_up(c1, 4)) anything (TB kernels
    store whole float4 lanes; naive and lds write the boxes alone), and every
    other cell of the allocation, ghost ring and pitch padding included, still
    the sentinel."""
    lv = _lv(*plate)
    d = _depth(k)
    ox, oy, lx, ly = block
    sl = np.s_[ox:ox + lx, oy:oy + ly]
    g = ops.Geom(nx=plate[0], ny=plate[1], gx0=ox, gy0=oy, cx=CX, cy=CY)
    a = _field(lv[0], dev, d, block, NAN)
    inbox = np.zeros(tuple(a.data.shape), bool)
    spill = np.zeros_like(inbox)
    for r0, r1, c0, c1 in boxes:
        inbox[a.hx + r0:a.hx + r1, a.hy + c0:a.hy + c1] = True
        if k.kind == "tb":
            spill[a.hx + r0:a.hx + r1, a.hy + c1:a.hy + (c1 + 3) // 4 * 4] = True
    assert inbox[a.hx:a.hx + lx, a.hy:a.hy + ly].all() and int(inbox.sum()) == lx * ly
    untouched = ~(inbox | spill)
    for with_resid in ((True,) if rl else (False, True)):
        b = ops.Field(lx, ly, d, dev, fill=SENTINEL)
        resid = torch.zeros(4, dtype=torch.int32, device=dev) if with_resid else None
        _launch(k, a, b, g, boxes, resid, rl)
        out = b.data.cpu().numpy()
        what = "with residual" if with_resid else "no residual"
        assert_bitwise(out[a.hx:a.hx + lx, a.hy:a.hy + ly], lv[d][sl], what)
        stray = untouched & (O.bits(out) != O.bits(np.float32(SENTINEL)))
        assert not stray.any(), (f"{what}: {int(stray.sum())} cells written outside the boxes and "
                                 f"their lane spill, first at (row, column) "
                                 f"{tuple(np.argwhere(stray)[0] - (a.hx, a.hy))} of the block")
        if with_resid:
            want = float(np.abs(lv[rl or d][sl] - lv[(rl or d) - 1][sl]).max())
            got = ops.resid_value(resid)
            assert np.isfinite(got) and got == want, (got, want)


@pytest.mark.parametrize("plate", [(37, 70), (203, 519)], ids=["37x70", "203x519"])
@pytest.mark.parametrize("kc", KERNELS)
def test_write_set_full_plate(gpu, kc, plate):
    # 70 % 4 == 2, 519 % 4 == 3: two and one spill columns.
    k, rl = kc
    _write_set(k, rl, gpu, plate, (0, 0) + plate, [(0, plate[0], 0, plate[1])])


@pytest.mark.parametrize("kc", KERNELS)
def test_write_set_five_box_frame(gpu, kc):
    # The frame of test_tb_subdomain_offsets_and_boxes: K-row bands above and
    # below, 8 / 4-column bands left and right, the interior; in a block with
    # valid ghosts all around.
    k, rl = kc
    d = _depth(k)
    lx, ly = 50, 300
    boxes = [(0, d, 0, ly), (lx - d, lx, 0, ly), (d, lx - d, 0, 8), (d, lx - d, 296, ly),
             (d, lx - d, 8, 296)]
    _write_set(k, rl, gpu, (120, 700), (30, 256, lx, ly), boxes)
