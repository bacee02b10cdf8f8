"""The device's MPI-compat path against what the reference MPI program wrote.

Reads tests/golden/mpi_ref/ only (recorded from the reference's own binary,
see tests/ref_golden.py).  The `naive` and `lds` kernels under numerics="mpi",
the device-judged and the host-judged compat="mpi" convergence gate, graph
replay, loopback ranks with and without deep halos and the `heat` CLI must
give the reference's bytes, stop at the reference's step and print its lines.
The temporally blocked kernels evaluate the fp32 expression only: they must
refuse numerics="mpi" by name."""
import subprocess

import pytest

from parallel_heat_amd import HeatSolver, _native
from parallel_heat_amd.parallel.group import run_group

from . import ref_golden as RG

pytestmark = pytest.mark.gpu

LONG = "48x96_conv20"  # 24300 steps: graphs only
KERNELS = ["naive", "lds"]


def _single(c, **kw):
    with HeatSolver(c.heat_config(backend="hip", **kw)) as s:
        # the device-side init is the reference's inidat, int32 wrap included
        RG.assert_file(c, "initial_im.dat", RG.dat_bytes(s.gather()))
        r = s.run()
        g = s.gather()
    RG.assert_run(c, r)
    RG.assert_grid(c, g)
    return r


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", RG.names(exclude=(LONG,)))
def test_single_rank(gpu, monkeypatch, name, kernel, use_graph):
    # Every case but the long one, the large wrapped plate (480x448_12, a
    # digest with four whole lines) included; convergence judged on the device.
    monkeypatch.delenv("HEAT_HOST_CHECKS", raising=False)
    monkeypatch.delenv("HEAT_GRAPH", raising=False)
    c = RG.case(name)
    r = _single(c, kernel=kernel, use_graph=use_graph)
    if c.converge:
        assert r.checks >= 1


@pytest.mark.parametrize("kernel", KERNELS)
def test_single_rank_long_run(gpu, monkeypatch, kernel):
    monkeypatch.delenv("HEAT_HOST_CHECKS", raising=False)
    monkeypatch.delenv("HEAT_GRAPH", raising=False)
    c = RG.case(LONG)
    assert c.ref_it == 24299
    _single(c, kernel=kernel, use_graph=True)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", ["24x30_conv20", "33x17_conv7"])
def test_host_judged_loop(gpu, monkeypatch, name, kernel):
    # HEAT_HOST_CHECKS=1: the residual read back and compared on the host.  It
    # must stop where the reference and the device judge (test_single_rank) do.
    monkeypatch.setenv("HEAT_HOST_CHECKS", "1")
    c = RG.case(name)
    r = _single(c, kernel=kernel)
    assert r.checks == (c.ref_it + 1) // c.config["check_interval"]


@pytest.mark.parametrize("kernel,depth", [("naive", 0), ("lds", 2)], ids=["naive", "lds-depth2"])
@pytest.mark.parametrize("world,grid", [(4, (2, 2)), (3, (3, 1))], ids=["2x2", "3x1"])
@pytest.mark.parametrize("name", ["24x30_conv20", "33x17_conv7", "96x80_37"])
def test_loopback_ranks(gpu, monkeypatch, name, world, grid, kernel, depth):
    # Ranks as threads over the device-memory exchange path: same bytes and
    # the same step on every rank (33x17 on 2 x 2: blocks with remainders;
    # lds at depth 2: a deep halo, several passes per exchange).
    monkeypatch.delenv("HEAT_HOST_CHECKS", raising=False)
    c = RG.case(name)
    cfg = c.heat_config(backend="hip", kernel=kernel, tb_depth=depth, px=grid[0], py=grid[1])

    def fn(s):
        return s.run(), s.gather(), (s.info.px, s.info.py), (s.info.tb_depth, s.info.halo)

    res = run_group(cfg, world, fn, transport="loopback")
    assert len(res) == world
    for r, _, pg, (k, halo) in res:
        assert pg == grid
        RG.assert_run(c, r, world)
        if depth:
            assert k == depth and halo >= 2 * depth, (k, halo)
    grids = [g for _, g, _, _ in res if g is not None]
    assert len(grids) == 1
    RG.assert_grid(c, grids[0])


def _heat(args, cwd):
    return subprocess.run([str(_native.CLI_PATH), "--backend", "hip", "--naming", "mpi",
                           "--numerics", "mpi"] + args, cwd=cwd, capture_output=True, text=True,
                          timeout=300)


@pytest.mark.parametrize("name", ["24x30_conv20", "96x80_37"])
def test_cli_on_the_device(gpu, tmp_path, name):
    c = RG.case(name)
    p = _heat(c.cli, tmp_path)
    assert p.returncode == 0, p.stderr
    assert RG.normalised(p.stdout.splitlines()) == RG.expected_lines(c)
    for k in ("initial_im.dat", "final_im.dat"):
        RG.assert_file(c, k, (tmp_path / k).read_bytes())


def test_cli_four_loopback_ranks(gpu, tmp_path):
    c = RG.case("24x30_conv20")
    p = _heat(c.cli + ["--gpus", "4", "--transport", "loopback"], tmp_path)
    assert p.returncode == 0, p.stderr
    assert RG.normalised(p.stdout.splitlines()) == RG.expected_lines(c, world=4)
    for k in ("initial_im.dat", "final_im.dat"):
        RG.assert_file(c, k, (tmp_path / k).read_bytes())


@pytest.mark.parametrize("kernel", ["tb", "mfma"])
def test_fp32_only_kernels_refuse_mpi_numerics(gpu, tmp_path, kernel):
    # No golden run for these: they must say so, not compute something else.
    c = RG.case("96x80_37")
    with pytest.raises(_native.NativeError, match="--numerics mpi needs the lds or naive kernel"):
        HeatSolver(c.heat_config(backend="hip", kernel=kernel))
    p = _heat(c.cli + ["--kernel", kernel], tmp_path)
    assert p.returncode != 0
    assert "--numerics mpi needs the lds or naive kernel" in p.stderr
    assert not (tmp_path / "final_im.dat").exists()
