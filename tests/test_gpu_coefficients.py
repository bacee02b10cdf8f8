"""Every HIP kernel family against the independent exact oracle
(`reference.step_np_fma`, NumPy only) with ANISOTROPIC coefficients, on
negative / subnormal / widely mixed values, and with NaN in every cell the
kernels call don't-care.

The rest of the suite runs cx == cy == 0.1 on positive normal data against
the CPU backend (which shares `heat::stencil` with the kernels): a kernel
that swaps cx and cy or loads one of them twice, a packed build that flushes
subnormals or re-associates a sum, a Dirichlet mask written as a multiply, or
a residual that reads a spill column passes all of that.  Here each of those
is off by ~10 (swap), in every cell (flush) or NaN (masks).  Needs an MI355X."""
import numpy as np
import pytest
import torch

from parallel_heat_amd import ops

from . import oracle_cases as O
from .oracle_cases import assert_bitwise

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("exp_kernels")]

V = ops.TbVariant
RAMP_S = V.RAMP | V.SCALAR
DEF = V.DEFAULT
DEEP = V.DEFAULT_DEEP
TILE = V.TILE | V.XCD_GROUPS
TILE_DPP = TILE | V.TILE_DPP

LX, LY = 203, 517   # partial strips, chunks and tiles; all four plate edges
SWAPPED = O.ANISO[::-1]


class K:
    """One kernel launch shape: kind naive / lds / mfma / tb, and for tb the
    variant, depth and tuning knobs (restored after the launch)."""

    def __init__(self, kind, variant=-1, depth=1, **tune):
        self.kind, self.variant, self.depth, self.tune = kind, variant, depth, tune

    def run(self, a, b, g, resid=None, res_level=0, boxes=None, numerics="fp32"):
        saved = ops.tb_tuning()
        try:
            if self.tune:
                t = ops.tb_tuning()
                for k, v in self.tune.items():
                    setattr(t, k, v)
                ops.set_tb_tuning(t)
            if self.kind == "naive":
                ops.naive_step(a, b, g, resid=resid)
            elif self.kind == "lds":
                ops.lds_step(a, b, g, resid=resid, numerics=numerics)
            elif self.kind == "mfma":
                ops.mfma_step(a, b, g, resid=resid)
            else:
                ops.tb_step(a, b, g, self.depth, boxes=boxes, resid=resid, variant=self.variant,
                            res_level=res_level)
            torch.cuda.synchronize()
        finally:
            ops.set_tb_tuning(saved)


def tb(variant, depth, **tune):
    return K("tb", variant, depth, **tune)


def _p(name, k):
    return pytest.param(k, id=name)


NAIVE, LDS = _p("naive", K("naive")), _p("lds", K("lds"))
STREAM = [
    _p("RAMP_S@8", tb(RAMP_S, 8)), _p("RAMP_S@12", tb(RAMP_S, 12)),
    _p("DEF@8", tb(DEF, 8)), _p("DEF@12", tb(DEF, 12)),
    _p("DEEP@8", tb(DEEP, 8)), _p("DEEP@12", tb(DEEP, 12)),
    _p("DEEP_LINEAR@12", tb(DEEP | V.LINEAR, 12)),
    _p("DEEP_ALT@12", tb(DEEP | V.ALT_DIRECTION, 12)),
    _p("DEEP_nt1@12", tb(DEEP, 12, nt=1)),              # tb_split_nt.hip
    _p("RING3@8", tb(V.RING3, 8)),                      # packed pair code (tb_packed.hip)
    _p("DEF_FLOAT2@8", tb(DEF | V.FLOAT2, 8)),
    _p("DEEP_MIXED@12", tb(DEEP | V.SHIFT_MIXED, 12)),
]
# 12-row waves take the packed update (tb_tile_core.hpp Upd::apply PK), 20-row
# waves the scalar one; 16 waves: the other workgroup shape.
TILES = [_p(f"{n}_{r}x{w}@{d}", tb(v, d, tile_rows=r, tile_waves=w))
         for n, v in (("TILE", TILE), ("TILE_DPP", TILE_DPP))
         for r, w in ((12, 8), (20, 8), (12, 16)) for d in (8, 12)]
HARD = [NAIVE, LDS, _p("DEF@8", tb(DEF, 8)), _p("DEEP@12", tb(DEEP, 12)),
        _p("DEEP_nt1@12", tb(DEEP, 12, nt=1)), _p("RING3@8", tb(V.RING3, 8)),
        _p("TILE_12x8@12", tb(TILE, 12, tile_rows=12, tile_waves=8)),
        _p("TILE_DPP@12", tb(TILE_DPP, 12))]
POISON = [NAIVE, LDS, _p("DEF@8", tb(DEF, 8)), _p("DEEP@12", tb(DEEP, 12)),
          _p("DEEP_LINEAR@12", tb(DEEP | V.LINEAR, 12)), _p("TILE@12", tb(TILE, 12)),
          _p("TILE_DPP@12", tb(TILE_DPP, 12))]


def _field(full, dev, halo, block=None, fill=0.0):
    """A field holding block (ox, oy, lx, ly) of the plate `full` (default: all
    of it): the owned cells and the ghost ring's cells that lie inside the
    plate; every other cell (outside the plate, pitch padding) is `fill`."""
    nx, ny = full.shape
    ox, oy, lx, ly = block or (0, 0, nx, ny)
    f = ops.Field(lx, ly, halo, dev, fill=fill)
    r0, r1 = max(0, ox - f.hx), min(nx, ox + lx + f.hx)
    c0, c1 = max(0, oy - f.hy), min(ny, oy + ly + f.hy)
    f.data[r0 - ox + f.hx:r1 - ox + f.hx, c0 - oy + f.hy:c1 - oy + f.hy] = \
        torch.from_numpy(full[r0:r1, c0:c1].copy()).to(dev)
    return f


def _check(k, lv, g, dev, block=None, fill=0.0, res_level=0, boxes=None, numerics="fp32",
           start=0):
    """Launch k on the state lv[start]; the owned block must be
    lv[start + k.depth] bit for bit and the fused residual that of step
    res_level of the launch (default: its last)."""
    nx, ny = lv[0].shape
    ox, oy, lx, ly = block or (0, 0, nx, ny)
    sl = np.s_[ox:ox + lx, oy:oy + ly]
    a = _field(lv[start], dev, max(k.depth, 1), block, fill)
    if not res_level:
        # Without a residual first: its own instantiation of most kernels (the
        # 12-row tile waves take the packed update only there unless their
        # lane shifts are DPP).
        b = _field(lv[start], dev, max(k.depth, 1), block, fill)
        k.run(a, b, g, boxes=boxes, numerics=numerics)
        assert_bitwise(b.owned().cpu().numpy(), lv[start + k.depth][sl], "no residual")
    b = _field(lv[start], dev, max(k.depth, 1), block, fill)
    resid = torch.zeros(4, dtype=torch.int32, device=dev)
    k.run(a, b, g, resid=resid, res_level=res_level, boxes=boxes, numerics=numerics)
    assert_bitwise(b.owned().cpu().numpy(), lv[start + k.depth][sl], "with residual")
    rl = start + (res_level or k.depth)
    want = float(np.abs(lv[rl][sl] - lv[rl - 1][sl]).max())
    got = ops.resid_value(resid)
    assert np.isfinite(got) and got == want, (got, want)


def _plate(name, coef, steps=12, numerics="fma", shape=(LX, LY)):
    g = ops.Geom(nx=shape[0], ny=shape[1], cx=coef[0], cy=coef[1])
    return g, O.levels(name, shape[0], shape[1], coef[0], coef[1], steps, numerics)


# -- 1. every kernel family, anisotropic, [0, 100) data ------------------------

@pytest.mark.parametrize("coef", [O.ANISO, SWAPPED])
@pytest.mark.parametrize("k", [NAIVE, LDS] + STREAM + TILES)
def test_kernel_anisotropic_bitwise(gpu, k, coef):
    g, lv = _plate("pos", coef)
    _check(k, lv, g, gpu)


@pytest.mark.parametrize("coef", [O.ANISO, SWAPPED])
def test_lds_mpi_numerics_anisotropic(gpu, coef):
    g, lv = _plate("pos", coef, 1, "mpi")
    _check(K("lds"), lv, g, gpu, numerics="mpi")
    assert not np.array_equal(lv[1], O.levels("pos", LX, LY, coef[0], coef[1], 12)[1])


@pytest.mark.parametrize("coef", [O.ANISO, SWAPPED])
@pytest.mark.parametrize("rl", [5, 10])
@pytest.mark.parametrize("k", [_p("DEEP@12", tb(DEEP, 12)), _p("TILE@12", tb(TILE, 12))])
def test_inner_level_residual_anisotropic(gpu, k, rl, coef):
    # A check inside a depth-12 pass: residual of step rl, state of step 12.
    g, lv = _plate("pos", coef)
    _check(k, lv, g, gpu, res_level=rl)


def _mfma_check(name, coef, dev, shape=(LX, LY)):
    g, lv = _plate(name, coef, shape=shape)
    a, b = _field(lv[0], dev, 4), _field(lv[0], dev, 4)
    r = torch.zeros(4, dtype=torch.int32, device=dev)
    K("mfma").run(a, b, g, resid=r)
    got, ref = b.owned().cpu().numpy(), lv[1]
    dev_max = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max())
    print(f"mfma {name} cx={coef[0]} cy={coef[1]}: max |got - oracle| = {dev_max:.3e} (bound 2e-5)")
    # Exact fp32 products in another association than heat::stencil: the bound
    # test_mfma_step_close_to_oracle uses on data of magnitude 100 (a swap of
    # the coefficients is off by ~10).
    assert dev_max <= 2e-5
    for sl in (np.s_[0, :], np.s_[-1, :], np.s_[:, 0], np.s_[:, -1]):
        assert_bitwise(got[sl], ref[sl], "ring")
    assert ops.resid_value(r) == float(np.abs(got - lv[0]).max())


@pytest.mark.parametrize("coef", [O.ANISO, SWAPPED])
def test_mfma_anisotropic_within_bound(gpu, coef):
    _mfma_check("pos", coef, gpu)


@pytest.mark.parametrize("coef", [O.ANISO, SWAPPED])
@pytest.mark.parametrize("k", [_p("DEEP@8", tb(DEEP, 8)), _p("TILE@8", tb(TILE, 8))])
def test_interior_subdomain_anisotropic(gpu, k, coef):
    # A block inside a larger plate with valid ghosts all around (the
    # unmasked modes), geometry of test_tb_subdomain_offsets_and_boxes,
    # against the slice of the emulated FULL plate.
    NX, NY, d = 120, 700, 8
    ox, oy, lx, ly = 30, 256, 50, 300
    lv = O.levels("pos", NX, NY, coef[0], coef[1], d)
    g = ops.Geom(nx=NX, ny=NY, gx0=ox, gy0=oy, cx=coef[0], cy=coef[1])
    if k.variant == DEEP:
        boxes = [(0, lx, 0, 296), (0, lx, 296, ly)]
    else:
        boxes = [(0, d, 0, ly), (lx - d, lx, 0, ly), (d, lx - d, 0, 8), (d, lx - d, 296, ly),
                 (d, lx - d, 8, 296)]
    _check(k, lv, g, gpu, block=(ox, oy, lx, ly), boxes=boxes)


# -- 2. hard values --------------------------------------------------------------

@pytest.mark.parametrize("name", ["signed", "wide", "tiny"])
@pytest.mark.parametrize("k", HARD)
def test_kernel_hard_values_bitwise(gpu, k, name):
    # signed, wide: from the value set itself (wide: exponents from subnormal
    # to 2^100 side by side; after a few steps the largest dominate).  tiny:
    # the kernel ends at the oracle's 48-step state (it starts from the state
    # its depth earlier), where 0.71 of the interior is non-zero subnormal
    # and no cell is zero; between steps 4 and 30 the share is below half.
    if name == "tiny":
        g, lv = _plate(name, O.ANISO, 48)
        O.check_preconditions(name, lv)
        _check(k, lv, g, gpu, start=48 - k.depth)
    else:
        g, lv = _plate(name, O.ANISO)
        O.check_preconditions(name, lv)
        _check(k, lv, g, gpu)


def test_mfma_signed_within_bound(gpu):
    _mfma_check("signed", O.ANISO, gpu)


# -- 3. NaN in every don't-care cell -----------------------------------------------

@pytest.mark.parametrize("k", POISON)
def test_poisoned_outside_cells_full_plate(gpu, k):
    # Ghost ring and pitch padding of a full plate lie outside the plate:
    # all NaN.  Masks must select, residuals must not look there.
    g, lv = _plate("pos", O.ANISO)
    _check(k, lv, g, gpu, fill=float("nan"))


@pytest.mark.parametrize("k", POISON)
def test_poisoned_outside_cells_corner_block(gpu, k):
    # A block touching only the plate's right and bottom edges: valid ghosts
    # above and to the left, NaN beyond the plate below and to the right.
    NX, NY = 240, 700
    ox, oy = 90, 256
    lx, ly = NX - ox, NY - oy
    lv = O.levels("pos", NX, NY, *O.ANISO, 12)
    g = ops.Geom(nx=NX, ny=NY, gx0=ox, gy0=oy, cx=O.ANISO[0], cy=O.ANISO[1])
    _check(k, lv, g, gpu, block=(ox, oy, lx, ly), fill=float("nan"))
