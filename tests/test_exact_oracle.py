"""The CPU backend against an INDEPENDENT exact oracle, with anisotropic
coefficients and hard values.

Everything else in the suite compares kernels with the CPU backend, which
calls the same `heat::stencil` as they do, at cx == cy and on positive normal
data.  Here the reference is `reference.step_np_fma`: NumPy only, a correctly
rounded fp32 FMA emulated in float64 (`reference.fma32`), bitwise.  A swap of
cx and cy anywhere from HeatConfig to the stencil, a re-associated sum or a
flushed subnormal fails these tests.  No GPU needed."""
import subprocess

import numpy as np
import pytest
import torch

from parallel_heat_amd import HeatConfig, HeatSolver, _native, ops
from parallel_heat_amd.models import reference as R
from parallel_heat_amd.utils import io as hio

from . import oracle_cases as O

F = np.float32
HEAT = str(_native.CLI_PATH)


_bits, assert_bitwise = O.bits, O.assert_bitwise


# -- fma32: directed cases with hand-known results ---------------------------

def test_fma32_tie_broken_by_a_tiny_addend():
    # (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24: exactly halfway between the fp32
    # neighbours 1 + 2^-11 and 1 + 2^-11 + 2^-23.  The addend decides.
    a = F(1 + 2.0 ** -12)
    lo, hi = F(1 + 2.0 ** -11), F(1 + 2.0 ** -11 + 2.0 ** -23)
    assert float(a) * float(a) == 1 + 2.0 ** -11 + 2.0 ** -24
    assert R.fma32(a, a, F(2.0 ** -60)) == hi
    assert R.fma32(a, a, F(-2.0 ** -60)) == lo
    assert R.fma32(a, a, F(0)) == lo              # the tie itself: to even
    # The plain float64 expression rounds twice and loses the addend: the
    # case bites.
    plain = np.float64(a) * np.float64(a) + np.float64(F(2.0 ** -60))
    assert plain.astype(np.float32) == lo != hi


def test_fma32_subnormal_results():
    # 3 * 2^-149 + 2^-149 = 2^-147; (2^-75)^2 = 2^-150 is half the smallest
    # subnormal: a tie to even (0), above it with any positive addend.
    tiny = F(2.0 ** -149)
    assert R.fma32(F(3), tiny, tiny) == F(2.0 ** -147)
    h = F(2.0 ** -75)
    assert _bits(R.fma32(h, h, F(0))) == 0
    assert R.fma32(h, h, tiny) == F(2) * tiny               # 1.5 ulp, tie to even: 2 ulp
    assert R.fma32(F(1.5), tiny, F(0)) == F(2) * tiny       # the same from one product
    assert R.fma32(F(2.5), tiny, F(0)) == F(2) * tiny       # 2.5 ulp, tie to even: 2 ulp
    assert R.fma32(h, h, F(3) * tiny) == F(4) * tiny        # 3.5 ulp, tie to even: 4 ulp
    # 2.5 ulp plus / minus a product bit 2^23 times smaller: no longer a tie.
    assert R.fma32(h, F(2.0 ** -75 * (1 + 2.0 ** -23)), F(2) * tiny) == F(3) * tiny
    assert R.fma32(h, F(2.0 ** -75 * (1 - 2.0 ** -24)), F(2) * tiny) == F(2) * tiny
    assert R.fma32(-h, F(2.0 ** -75 * (1 + 2.0 ** -23)), F(-2) * tiny) == F(-3) * tiny
    # Subnormal operands, normal result.
    assert R.fma32(F(2.0 ** 30), F(2.0 ** -140), F(2.0 ** -110)) == F(2.0 ** -109)


def test_fma32_rounds_up_into_the_next_binade():
    # (2 - 2^-23) * (1 + 2^-23) = 2 + 2^-23 - 2^-46 -> 2 (down, same binade
    # border); with + 2^-23 more it is 2 + 2^-22 - 2^-46 -> 2 + 2^-22.
    a, b = F(2 - 2.0 ** -23), F(1 + 2.0 ** -23)
    assert R.fma32(a, b, F(0)) == F(2)
    assert R.fma32(a, b, F(2.0 ** -23)) == F(2 + 2.0 ** -22)
    # All-ones mantissa plus half an ulp and a bit: carries into the exponent.
    ones = F(2 - 2.0 ** -23)
    assert R.fma32(ones, F(1), F(2.0 ** -24)) == F(2)           # tie -> even = 2.0
    assert R.fma32(ones, F(1), F(2.0 ** -25)) == ones
    # Overflow to inf by rounding only.
    big = np.finfo(np.float32).max
    assert np.isinf(R.fma32(big, F(1), F(2.0 ** 103)))          # half an ulp: tie -> even = inf
    assert R.fma32(big, F(1), F(2.0 ** 102)) == big


def test_fma32_signed_zeros_inf_nan():
    z, nz = F(0.0), F(-0.0)
    neg = np.uint32(0x80000000)
    assert _bits(R.fma32(nz, F(1), nz)) == neg         # -0 + -0 = -0
    assert _bits(R.fma32(nz, F(1), z)) == 0            # -0 + +0 = +0
    assert _bits(R.fma32(F(-2), z, z)) == 0            # the stencil's fma(-2, c, s + n) at zero
    assert _bits(R.fma32(F(1), F(1), F(-1))) == 0      # exact cancellation: +0
    inf = F(np.inf)
    assert R.fma32(inf, F(2), F(1)) == inf
    assert R.fma32(F(-3), inf, F(1)) == -inf
    assert R.fma32(F(1), F(1), -inf) == -inf
    assert np.isnan(R.fma32(inf, F(1), -inf))
    assert np.isnan(R.fma32(inf, z, F(1)))
    assert np.isnan(R.fma32(F(np.nan), F(1), F(1)))
    assert np.isnan(R.fma32(F(1), F(1), F(np.nan)))
    # arrays, broadcasting
    out = R.fma32(np.array([1, 2, 3], np.float32), F(2), np.array([[0], [1]], np.float32))
    assert out.dtype == np.float32 and np.array_equal(out, [[2, 4, 6], [3, 5, 7]])


def test_step_np_fma_is_not_the_plain_fp32_step():
    # On [0, 100) data the fused and the separately rounded expression differ
    # in a good share of the cells (by ulps): the exact oracle is a different,
    # sharper statement than step_np.
    u = O.values("pos", 37, 53)
    a, b = R.step_np_fma(u, *O.ANISO), R.step_np(u, *O.ANISO)
    assert (a != b).mean() > 0.05
    assert np.abs(a - b).max() <= 2e-5
    for sl in (np.s_[0, :], np.s_[-1, :], np.s_[:, 0], np.s_[:, -1]):
        assert np.array_equal(a[sl], u[sl])
    # and swapping the coefficients is visible at once
    assert np.abs(a - R.step_np_fma(u, O.ANISO[1], O.ANISO[0])).max() > 1.0


# -- the CPU backend, bitwise ---------------------------------------------------

def _set_threads(n):
    # The OpenMP thread count is process-wide and set when a CPU solver is
    # created (Solver::Solver -> cpu::set_threads).
    HeatSolver(HeatConfig(nx=3, ny=3, steps=0, backend="cpu", threads=n)).close()


CASES = [pytest.param(n, s, c, id=f"{n}-{s[0]}x{s[1]}-{c[0]}-{c[1]}")
         for n in O.SETS for s in O.SHAPES for c in O.COEFFS]


@pytest.mark.parametrize("nthreads", [1, 4])
@pytest.mark.parametrize("name,shape,coef", CASES)
def test_cpu_step_bitwise_vs_exact_oracle(name, shape, coef, nthreads):
    # ops.naive_step on CPU fields (heat_cpu_step), states after 1 and 48 steps.
    (nx, ny), (cx, cy) = shape, coef
    lv = O.levels(name, nx, ny, cx, cy, 48)
    # Preconditions on the run's result (the 48-step state).  One exception:
    # with a one-axis pair, (0.25, 0) or (0, 0.25), magnitudes decay along one
    # axis only and the tiny set's subnormal share after 48 steps on the
    # 105 k-cell plate is a statistic no seed moves (0.436 / 0.424 at seed 8,
    # 0.437 / 0.427 at seed 2, 0.433 / 0.423 at seed 3); its state after one
    # step, which is compared as well, has the share (0.62).
    one_axis_large = 0.0 in coef and shape == (203, 517)
    O.check_preconditions(name, lv[:2] if one_axis_large else lv)
    _set_threads(nthreads)
    g = ops.Geom(nx=nx, ny=ny, cx=cx, cy=cy)
    a, b = ops.Field(nx, ny, 1, "cpu"), ops.Field(nx, ny, 1, "cpu")
    a.set_owned(torch.from_numpy(lv[0].copy()))
    b.set_owned(torch.from_numpy(lv[0].copy()))
    for k in range(1, 49):
        r = torch.zeros(1, dtype=torch.int32)
        ops.naive_step(a, b, g, resid=r)
        a, b = b, a
        if k in (1, 48):
            assert_bitwise(a.owned().numpy(), lv[k], f"step {k}")
            assert ops.resid_value(r) == O.resid(lv, k), k


@pytest.mark.parametrize("nthreads", [1, 4])
@pytest.mark.parametrize("name,shape,coef", CASES)
def test_cpu_solver_bitwise_vs_exact_oracle(name, shape, coef, nthreads):
    (nx, ny), (cx, cy) = shape, coef
    lv = O.levels(name, nx, ny, cx, cy, 48)
    cfg = HeatConfig(nx=nx, ny=ny, steps=0, cx=cx, cy=cy, init="zero", backend="cpu",
                     threads=nthreads)
    with HeatSolver(cfg) as s:
        s.scatter(lv[0])
        s.run(1)
        assert_bitwise(s.gather(), lv[1], "step 1")
        s.run(47)
        assert s.step == 48
        assert_bitwise(s.gather(), lv[48], "step 48")


def test_tiny_set_subnormal_share():
    # The state the GPU tests compare on the tiny set: 48 steps at 203 x 517
    # (each kernel starts from the oracle's state its depth earlier).
    # Measured at seed 8: 0.712 non-zero subnormal, no cell zero.  (The share
    # dips to 0.46 around step 8 while the few normal cells spread, then
    # rises as magnitudes decay.)
    lv = O.levels("tiny", 203, 517, *O.ANISO, 48)
    share = O.subnormal_share(lv[48])
    print(f"tiny set, seed {O.SEED}, 203 x 517, 48 steps: subnormal share {share:.3f}")
    assert share >= 0.5
    assert (lv[48][1:-1, 1:-1] != 0).all()


# -- further paths with (cx, cy) = (0.05, 0.2) ---------------------------------

@pytest.mark.parametrize("compat", ["none", "mpi", "cuda"])
def test_cpu_convergence_predicted_exactly(compat):
    cx, cy = O.ANISO
    kw = dict(nx=24, ny=30, steps=20000, converge=True, check_interval=20, eps=1e-3)
    with HeatSolver(HeatConfig(**kw, cx=cx, cy=cy, backend="cpu", compat=compat)) as s:
        r = s.run()
        g = s.gather()
    ref, done, conv_at = R.run_np(**kw, cx=cx, cy=cy, compat=compat, numerics="fma")
    assert conv_at > 0 and r.converged
    assert (r.steps_done, r.converged_at) == (done, conv_at)
    assert_bitwise(g, ref)
    # not the isotropic run's answer
    _, _, iso = R.run_np(**kw, compat=compat, numerics="fma")
    assert iso != conv_at


@pytest.mark.parametrize("coef", [O.ANISO, O.ANISO[::-1]])
def test_cpu_mpi_numerics_anisotropic(coef):
    cx, cy = coef
    lv = O.levels("signed", 37, 53, cx, cy, 33, "mpi")
    cfg = HeatConfig(nx=37, ny=53, steps=0, cx=cx, cy=cy, init="zero", backend="cpu",
                     numerics="mpi", threads=2)
    with HeatSolver(cfg) as s:
        s.scatter(lv[0])
        s.run(33)
        assert_bitwise(s.gather(), lv[33])
    fma = O.levels("signed", 37, 53, cx, cy, 33)
    assert not np.array_equal(lv[33], fma[33])   # a genuinely different rounding


@pytest.mark.parametrize("world,kw", [(4, dict(decomp="auto", tb_depth=3, halo_passes=2))])
def test_cpu_multiprocess_anisotropic(tmp_path, world, kw):
    # A 2 x 2 process grid with deep halos: a decomposition that confuses the
    # axes (or a rank that falls back to default coefficients) shows here.
    from .dist_worker import run_world
    cx, cy = O.ANISO
    res = run_world(world, dict(nx=37, ny=45, steps=0, cx=cx, cy=cy, init="random", seed=11,
                                backend="cpu", **kw), 29, tmp_path)
    assert (int(res["px"]), int(res["py"])) == (2, 2)
    lv = O.levels_of_init(37, 45, cx, cy, 29, "random", 11)
    assert_bitwise(res["grid"], lv[29])


def _heat(args, cwd):
    return subprocess.run([HEAT] + args, cwd=cwd, capture_output=True, text=True, check=True,
                          timeout=300)


def test_cli_anisotropic_binary_output(tmp_path):
    _heat(["--backend", "cpu", "--nx", "41", "--ny", "39", "--steps", "57", "--init", "random",
           "--seed", "3", "--cx", "0.05", "--cy", "0.2", "--out", "g.bin", "--out-format",
           "bin"], tmp_path)
    g, h = hio.read_bin(str(tmp_path / "g.bin"))
    assert h["step"] == 57 and (F(h["cx"]), F(h["cy"])) == (F(0.05), F(0.2))
    assert_bitwise(np.asarray(g), O.levels_of_init(41, 39, 0.05, 0.2, 57, "random", 3)[57])


def test_cli_checkpoint_resume_anisotropic(tmp_path):
    # The header carries the coefficients: resuming with the same ones gives
    # no warning and continues bit-exactly; with swapped ones it warns.
    base = ["--backend", "cpu", "--nx", "30", "--ny", "34", "--init", "random", "--seed", "5",
            "--out-format", "bin"]
    co = ["--cx", "0.05", "--cy", "0.2"]
    _heat(base + co + ["--steps", "25", "--out", "c25.bin"], tmp_path)
    p = _heat(base + co + ["--steps", "40", "--resume", "c25.bin", "--out", "r.bin"], tmp_path)
    assert "warning" not in p.stderr, p.stderr
    g, h = hio.read_bin(str(tmp_path / "r.bin"))
    assert h["step"] == 40
    lv = O.levels_of_init(30, 34, 0.05, 0.2, 40, "random", 5)
    assert_bitwise(np.asarray(g), lv[40])
    p = _heat(base + ["--cx", "0.2", "--cy", "0.05", "--steps", "40", "--resume", "c25.bin",
                      "--out", "none"], tmp_path)
    assert "warning" in p.stderr and "cx=0.05 cy=0.2" in p.stderr


def test_solver_checkpoint_resume_anisotropic(tmp_path, capfd):
    cx, cy = O.ANISO
    lv = O.levels("signed", 33, 47, cx, cy, 40)
    cfg = HeatConfig(nx=33, ny=47, steps=0, cx=cx, cy=cy, init="zero", backend="cpu")
    with HeatSolver(cfg) as s:
        s.scatter(lv[0])
        s.run(15)
        s.save(str(tmp_path / "c.bin"))
    h = hio.read_bin_header(str(tmp_path / "c.bin"))
    assert (F(h["cx"]), F(h["cy"]), h["step"]) == (F(cx), F(cy), 15)
    capfd.readouterr()
    with HeatSolver(cfg) as s:
        s.load(str(tmp_path / "c.bin"))
        assert s.step == 15
        s.run(25)
        assert_bitwise(s.gather(), lv[40])
    assert "warning" not in capfd.readouterr().err
