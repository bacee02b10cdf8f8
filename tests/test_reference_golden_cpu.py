"""The MPI-compat path against what the reference MPI program itself wrote.

tests/golden/mpi_ref/ holds, per case, the files and stdout of the reference's
own source built as a one-rank binary (oracle/build_ref.py --record).  Here:
the goldens are what those binaries write today; the CPU backend, the NumPy
emulation every other test leans on, and the `heat` CLI reproduce them byte for
byte, stop where the reference stopped and print its lines.

What the goldens tell apart (tried as mutations of heat::stencil_mpi): a term
of the update rounded to fp32 before the double arithmetic fails 480x448_12
(and only it: on the smaller plates those differences are exact in fp32); the
default fp32 arithmetic fails 96x80_37 in 3616 of 7680 cells.  What they cannot:
another association of the double sum, or `<` for `<=` against 1e-3.  The
double operations on fp32 operands of nearly equal exponent are almost always
exact, so either order rounds the same real number once (c + (cx tx + cy ty)
gave the same fp32 cells over 3000 steps of the 480x448 plate, 6.4e8 updates);
and an fp32 residual never equals the double 1e-3, which fp32 cannot hold."""
import os

import numpy as np
import pytest

from parallel_heat_amd import HeatSolver
from parallel_heat_amd.models import reference as R

from . import ref_golden as RG
from .test_cli import heat, heat_ranks

ALL = RG.names()
CLI = ["--backend", "cpu", "--naming", "mpi", "--numerics", "mpi"]


def _need(path):
    if not os.access(path, os.X_OK):
        pytest.skip(f"reference binary {os.path.relpath(path, RG.ROOT)} not built "
                    "(oracle/build_ref.py needs the reference checkout)")


@pytest.mark.parametrize("name", ALL)
def test_goldens_are_what_the_reference_writes(tmp_path, name):
    c = RG.case(name)
    _need(c.binary)
    lines, files = RG.run_reference_binary(c.binary, tmp_path)
    assert RG.normalised(lines) == RG.expected_lines(c)
    for k, v in files.items():
        RG.assert_file(c, k, v)


def test_openmp_twin_writes_the_same_bytes(tmp_path):
    twin = RG.manifest()["omp_twin"]
    c = RG.case(twin["of"])
    path = os.path.join(RG.REF_BIN, "mpi_" + twin["name"])
    _need(path)
    lines, files = RG.run_reference_binary(path, tmp_path)
    assert RG.normalised(lines) == RG.expected_lines(c)
    for k, v in files.items():
        RG.assert_file(c, k, v)


def test_golden_sizes():
    # What may be committed: no golden over 100 KB, the directory under 400 KB.
    total = 0
    for d, _, fs in os.walk(RG.GOLDEN):
        for f in fs:
            n = os.path.getsize(os.path.join(d, f))
            assert n <= 100 * 1000, (d, f, n)
            total += n
    assert total < 400 * 1000


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("name", ALL)
def test_cpu_backend(name, threads):
    c = RG.case(name)
    with HeatSolver(c.heat_config(backend="cpu", threads=threads)) as s:
        RG.assert_file(c, "initial_im.dat", RG.dat_bytes(s.gather()))
        r = s.run()
        g = s.gather()
    RG.assert_run(c, r)
    RG.assert_grid(c, g)


@pytest.mark.parametrize("name", ALL)
def test_numpy_emulation(name):
    # reference.run_np(compat="mpi", numerics="mpi") is the oracle of every
    # other MPI-compat test: here it meets the reference itself.
    c = RG.case(name)
    RG.assert_file(c, "initial_im.dat", RG.dat_bytes(R.init_grid(c.nx, c.ny, "ref-wrap")))
    g, done, conv_at = R.run_np(c.nx, c.ny, c.steps, converge=c.converge,
                                check_interval=c.config.get("check_interval", 20),
                                compat="mpi", numerics="mpi", init="ref-wrap")
    assert done == c.total_steps
    assert conv_at == (-1 if c.ref_it is None else c.ref_it + 1)
    RG.assert_grid(c, g)


@pytest.mark.parametrize("name", ALL)
def test_cli(tmp_path, name):
    c = RG.case(name)
    p = heat(CLI + c.cli, tmp_path)
    assert RG.normalised(p.stdout.splitlines()) == RG.expected_lines(c)
    for k in ("initial_im.dat", "final_im.dat"):
        RG.assert_file(c, k, (tmp_path / k).read_bytes())


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("name", ["24x30_conv20", "33x17_conv7"])
def test_cli_tcp_ranks(tmp_path, name, world):
    # The reference's output does not depend on its task count beyond the
    # banner's number; neither does ours (33x17 on 2 x 2 ranks: remainders).
    c = RG.case(name)
    outs = heat_ranks(CLI + c.cli, tmp_path, world)
    assert RG.normalised(outs[0][0].splitlines()) == RG.expected_lines(c, world)
    assert all(o == "" for o, _ in outs[1:])
    for k in ("initial_im.dat", "final_im.dat"):
        RG.assert_file(c, k, (tmp_path / k).read_bytes())


def test_golden_tells_the_two_arithmetics_apart(tmp_path):
    # Sharpness: 96x80_37 starts with most cells >= 2^20, where "%6.1f" shows
    # every fp32 bit.  The default fp32 (FMA) arithmetic must differ from the
    # reference's mixed fp32/double arithmetic in at least one printed cell.
    # If this ever fails the case has lost its teeth: replace the case, do not
    # delete the assertion.
    c = RG.case("96x80_37")
    with HeatSolver(c.heat_config(backend="cpu", numerics="fp32")) as s:
        r = s.run()
        g = s.gather()
    assert r.steps_done == c.steps + 1
    got = RG.dat_bytes(g).decode("ascii").split()
    want = c.read("final_im.dat").decode("ascii").split()
    assert len(got) == len(want) == c.nx * c.ny
    differ = sum(a != b for a, b in zip(got, want))
    assert differ >= 1, "numerics='fp32' prints the golden: 96x80_37 no longer separates them"
    # ... and `--naming mpi` alone keeps that default arithmetic.
    p = heat(["--backend", "cpu", "--naming", "mpi"] + c.cli, tmp_path)
    assert RG.normalised(p.stdout.splitlines()) == RG.expected_lines(c)
    assert (tmp_path / "final_im.dat").read_bytes() == RG.dat_bytes(g)
    assert (tmp_path / "final_im.dat").read_bytes() != c.read("final_im.dat")


def test_large_case_is_a_wrapped_plate():
    # 480x448_12: the reference's int32 product wraps (negative cells); its
    # golden is a digest with four whole lines, two or more with negatives.
    c = RG.case("480x448_12")
    assert c.golden == "digest"
    u0 = R.init_grid(c.nx, c.ny, "ref-wrap")
    assert (u0 < 0).any() and not np.array_equal(u0, R.init_grid(c.nx, c.ny, "exact"))
    with HeatSolver(c.heat_config(backend="cpu")) as s:
        s.run()
        g = s.gather()
    RG.assert_grid(c, g)
    bad = g.copy()
    bad[7, 222] = np.nextafter(bad[7, 222], np.float32(np.inf))  # |value| >= 2^20: one ulp shows
    assert abs(bad[7, 222]) >= 2 ** 20
    with pytest.raises(AssertionError):
        RG.assert_grid(c, bad)
