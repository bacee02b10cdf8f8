"""Insulated (zero-flux, homogeneous Neumann) plate edges, per side, without a
GPU: the NumPy oracle's properties, the CPU backend bitwise against it on one
rank and on a 2 x 2 process grid, convergence, and the front ends.

The scheme is the second-order mirror scheme: the cells of an insulated edge
are updated like interior cells, the missing neighbour being the cell's mirror
image across the edge row / column (u[-1, j] := u[1, j]).  Sides: n = row 0,
s = row nx-1, w = column 0, e = column ny-1."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from parallel_heat_amd import HeatConfig, HeatSolver, _native, ops
from parallel_heat_amd.models import reference as R
from parallel_heat_amd.utils import io as hio

from .dist_worker import run_world

HEAT = str(_native.CLI_PATH)
SIDE_SETS = ["n", "s", "w", "e", "ns", "we", "nw", "se", "nswe"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# --------------------------------------------------------------------------
# the oracle
# --------------------------------------------------------------------------
def test_oracle_deep_mirror_equivalence():
    # 12 insulated steps == 12 Dirichlet steps on the plate extended by 12
    # reflected rows per side, cropped: what the engine's deep ghost frame
    # rests on.
    u = R.init_grid(40, 45, "random", 1)
    a = u
    for _ in range(12):
        a = R.step_np_fma(a, insulated="ns")
    b = np.pad(u, ((12, 12), (0, 0)), mode="reflect")
    for _ in range(12):
        b = R.step_np_fma(b)
    assert np.array_equal(bits(a), bits(b[12:-12]))


def test_oracle_conserves_weighted_sum_exactly():
    # A fully insulated plate loses no heat: the trapezoid-weighted sum (1/2
    # on edge cells, 1/4 on corners) is constant.  Integer inputs below 256
    # and cx = cy = 1/4 keep every fp32 operation exact for 6 steps (8 integer
    # bits + 2 fraction bits per step <= 24), so it is constant bit for bit.
    nx, ny = 37, 53
    rng = np.random.default_rng(5)
    u = rng.integers(0, 256, (nx, ny)).astype(np.float32)
    w = np.ones((nx, ny), np.float64)
    w[0] *= 0.5
    w[-1] *= 0.5
    w[:, 0] *= 0.5
    w[:, -1] *= 0.5
    total = float((w * u).sum())
    for step in (R.step_np_fma, R.step_np):
        a = u
        for k in range(6):
            a = step(a, 0.25, 0.25, insulated="all")
            assert float((w * a.astype(np.float64)).sum()) == total, (step.__name__, k)
    assert not np.array_equal(a, u)


@functools.lru_cache(maxsize=None)
def converging_oracle():
    return R.run_np(24, 28, 3000, converge=True, init="random", seed=3, numerics="fma",
                    insulated="nswe")


def test_oracle_insulated_plate_converges_between_1000_and_1500():
    _, done, at = converging_oracle()
    assert 1000 < at < 1500 and done == at, (done, at)


def test_oracle_default_arguments_unchanged():
    u = R.init_grid(37, 53, "random", 2)
    c = u[1:-1, 1:-1]
    plain = u.copy()
    two = np.float32(2.0)
    plain[1:-1, 1:-1] = (c + np.float32(0.1) * ((u[2:, 1:-1] + u[:-2, 1:-1]) - two * c)) + \
        np.float32(0.1) * ((u[1:-1, 2:] + u[1:-1, :-2]) - two * c)
    assert np.array_equal(bits(R.step_np(u)), bits(plain))
    assert np.array_equal(bits(R.step_np(u, insulated="")), bits(plain))
    t = torch.from_numpy(u)
    assert torch.equal(R.step_torch(t), R.step_torch(t, insulated=""))
    # The exact oracles against the engine's Dirichlet CPU backend, as before.
    for numerics, step in (("fp32", R.step_np_fma), ("mpi", R.step_np_mpi)):
        with HeatSolver(HeatConfig(nx=37, ny=53, init="random", seed=2, backend="cpu",
                                   numerics=numerics)) as s:
            s.run(3)
            g = s.gather()
        a = b = u
        for _ in range(3):
            a, b = step(a), step(b, 0.1, 0.1, "")
        assert np.array_equal(bits(a), bits(g)) and np.array_equal(bits(b), bits(g))
    assert R.run_np(37, 53, 5, init="random", seed=2)[0].tobytes() == \
        R.run_np(37, 53, 5, init="random", seed=2, insulated="")[0].tobytes()


def test_oracle_torch_step_matches_numpy():
    u = R.init_grid(19, 23, "random", 8)
    for s in SIDE_SETS + ["all"]:
        got = R.step_torch(torch.from_numpy(u), 0.1, 0.1, insulated=s).numpy()
        assert np.allclose(got, R.step_np(u, insulated=s), rtol=0, atol=1e-4), s
    with pytest.raises(ValueError):
        R.step_np(u, insulated="x")


# --------------------------------------------------------------------------
# the host ghost fill (the twin of the HIP kernel)
# --------------------------------------------------------------------------
def fill_expected(full, hx, hy, lx, ly, sides, d):
    """The frame [-d, lx+d) x [-d, ly+d) of a field array after the fill:
    every cell beyond an insulated side takes its per-axis reflection."""
    want = full.copy()
    n, s, w, e = (c in sides for c in "nswe")
    for r in range(-d, lx + d):
        sr = -r if n and r < 0 else 2 * (lx - 1) - r if s and r >= lx else r
        for c in range(-d, ly + d):
            sc = -c if w and c < 0 else 2 * (ly - 1) - c if e and c >= ly else c
            if (sr, sc) != (r, c):
                want[hx + r, hy + c] = full[hx + sr, hy + sc]
    return want


@pytest.mark.parametrize("lx,ly,halo,d", [(9, 14, 5, 5), (9, 14, 5, 2), (6, 7, 3, 1)])
def test_host_fill_insulated_ghosts(lx, ly, halo, d):
    rng = np.random.default_rng(lx * ly)
    for mask in range(1, 16):
        sides = "".join(c for k, c in enumerate("nswe") if mask >> k & 1)
        f = ops.Field(lx, ly, halo, "cpu")
        f.data.copy_(torch.from_numpy(rng.random(tuple(f.data.shape), np.float32)))
        f.data[:f.hx] = float("nan")
        f.data[f.hx + lx:] = float("nan")
        f.data[:, :f.hy] = float("nan")
        f.data[:, f.hy + ly:] = float("nan")
        before = f.data.numpy().copy()
        ops.fill_insulated_ghosts(f, sides, d)
        want = fill_expected(before, f.hx, f.hy, lx, ly, sides, d)
        assert np.array_equal(bits(f.data.numpy()), bits(want)), sides
        # On a plate, the depth-1 frame is np.pad's reflection.
        pad = ((int("n" in sides), int("s" in sides)), (int("w" in sides), int("e" in sides)))
        own = before[f.hx:f.hx + lx, f.hy:f.hy + ly]
        got = f.data.numpy()[f.hx - pad[0][0]:f.hx + lx + pad[0][1],
                             f.hy - pad[1][0]:f.hy + ly + pad[1][1]]
        assert np.array_equal(got, np.pad(own, pad, mode="reflect")), sides
    with pytest.raises(ValueError):
        ops.fill_insulated_ghosts(ops.Field(lx, ly, halo, "cpu"), "n", halo + 1)


# --------------------------------------------------------------------------
# the CPU backend
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_levels(nx, ny, sides, numerics="fma"):
    """Levels 1 and 48 of the exact oracle from init random, seed 3."""
    step = {"fma": R.step_np_fma, "mpi": R.step_np_mpi}[numerics]
    u = R.init_grid(nx, ny, "random", 3)
    out = {}
    for k in range(1, 49):
        u = step(u, 0.1, 0.1, sides)
        if k in (1, 48):
            out[k] = u
    return out


def cpu_run(nx, ny, steps, sides, **kw):
    cfg = HeatConfig(nx=nx, ny=ny, steps=steps, init="random", seed=3, backend="cpu",
                     insulated=sides, **kw)
    with HeatSolver(cfg) as s:
        r = s.run()
        return s.gather(), r, s.info


@pytest.mark.parametrize("nx,ny,sides", [(nx, ny, s) for nx, ny in ((37, 53), (20, 20))
                                         for s in SIDE_SETS] + [(3, 40, "we")])
def test_cpu_backend_bitwise_vs_oracle(nx, ny, sides):
    want = oracle_levels(nx, ny, sides)
    for steps in (1, 48):
        for threads in (1, 4):
            for depth in (1, 4):
                g, r, info = cpu_run(nx, ny, steps, sides, threads=threads, tb_depth=depth)
                assert r.steps_done == steps and info.insulated == sides
                assert np.array_equal(bits(g), bits(want[steps])), (steps, threads, depth)


def test_cpu_backend_deep_halo_and_chunks():
    # Several passes per ghost fill (the fill refills m * K rows), chunked runs.
    want = oracle_levels(37, 53, "nswe")[48]
    cfg = HeatConfig(nx=37, ny=53, init="random", seed=3, backend="cpu", insulated="all",
                     tb_depth=3, halo_passes=4)
    with HeatSolver(cfg) as s:
        assert s.info.halo == 12 and s.info.insulated == "nswe"
        ex = sum(s.run(n).exchanges for n in (5, 1, 17, 22, 3))
        assert np.array_equal(bits(s.gather()), bits(want))
    assert ex < 48 // 3


def test_cpu_backend_thin_plate_lowers_depth_or_rejects():
    # 5 columns hold mirror sources for at most 4 ghost columns.
    g, _, info = cpu_run(20, 5, 9, "e", tb_depth=8)
    assert info.tb_depth == 4 and info.halo == 4
    u = R.init_grid(20, 5, "random", 3)
    for _ in range(9):
        u = R.step_np_fma(u, insulated="e")
    assert np.array_equal(bits(g), bits(u))
    with pytest.raises(_native.NativeError, match="at least 2"):
        cpu_run(1, 30, 1, "n")


def test_cpu_backend_mpi_numerics():
    want = oracle_levels(37, 53, "nswe", "mpi")[48]
    g, _, _ = cpu_run(37, 53, 48, "nswe", numerics="mpi", tb_depth=2)
    assert np.array_equal(bits(g), bits(want))


def test_cpu_backend_convergence_matches_oracle():
    want, done, at = converging_oracle()
    cfg = HeatConfig(nx=24, ny=28, steps=3000, converge=True, init="random", seed=3,
                     backend="cpu", insulated="nswe")
    with HeatSolver(cfg) as s:
        r = s.run()
        g = s.gather()
    assert r.converged and r.converged_at == at and r.steps_done == done
    assert np.array_equal(bits(g), bits(want))


@pytest.mark.parametrize("sides", ["nswe", "nw"])
def test_cpu_ranks_2x2_bitwise(tmp_path, sides):
    # Edge ranks mirror their own edges; the corners between an insulated side
    # and a neighbour side come from the neighbour's freshly received halo.
    kw = dict(nx=37, ny=53, steps=0, init="random", seed=3, backend="cpu", insulated=sides,
              tb_depth=2, halo_passes=2, px=2, py=2)
    res = run_world(4, kw, 0, tmp_path, chunks=[7, 1, 13, 8])
    assert (int(res["px"]), int(res["py"])) == (2, 2)
    one = HeatConfig(**{**kw, "px": 0, "py": 0, "tb_depth": 1, "halo_passes": 0})
    with HeatSolver(one) as s:
        s.run(29)
        want, cs = s.gather(), s.checksum()
    assert np.array_equal(bits(res["grid"]), bits(want))
    assert str(res["hash"]) == cs["hash"]
    u = R.init_grid(37, 53, "random", 3)
    for _ in range(29):
        u = R.step_np_fma(u, insulated=sides)
    assert np.array_equal(bits(want), bits(u))


# --------------------------------------------------------------------------
# front ends
# --------------------------------------------------------------------------
def heat(args, cwd, check=True):
    return subprocess.run([HEAT] + args, cwd=cwd, env=dict(os.environ), capture_output=True,
                          text=True, check=check, timeout=300)


def test_cli_insulated_dat_matches_oracle(tmp_path):
    p = heat(["--backend", "cpu", "--nx", "37", "--ny", "53", "--steps", "48", "--init", "random",
              "--seed", "3", "--insulated", "ns", "--out", "ns.dat", "--json"], tmp_path)
    ref = tmp_path / "ref.dat"
    hio.write_dat(str(ref), oracle_levels(37, 53, "ns")[48])
    assert (tmp_path / "ns.dat").read_bytes() == ref.read_bytes()
    m = json.loads(p.stdout.splitlines()[-1])
    assert m["insulated"] == "ns" and m["schedule"] == "sync" and m["halo"] >= 1


def test_cli_python_front_end_insulated(tmp_path):
    import sys
    p = subprocess.run([sys.executable, "-m", "parallel_heat_amd", "--backend", "cpu", "--nx", "37",
                        "--ny", "53", "--steps", "48", "--init", "random", "--seed", "3",
                        "--insulated", "all", "--out", "all.dat", "--json"], cwd=tmp_path,
                       env={**os.environ, "PYTHONPATH": str(_native.REPO_DIR)},
                       capture_output=True, text=True, check=True, timeout=300)
    ref = tmp_path / "ref.dat"
    hio.write_dat(str(ref), oracle_levels(37, 53, "nswe")[48])
    assert (tmp_path / "all.dat").read_bytes() == ref.read_bytes()
    assert json.loads(p.stdout.splitlines()[-1])["insulated"] == "nswe"


def test_cli_rejects_bad_sides(tmp_path):
    p = heat(["--backend", "cpu", "--insulated", "x"], tmp_path, check=False)
    assert p.returncode != 0 and "nswe" in p.stderr
    assert not list(tmp_path.iterdir())


def test_cli_plan_counts_insulated_ghosts(tmp_path):
    base = ["--plan", "--nx", "8192", "--ny", "8192"]
    plain = json.loads(heat(base, tmp_path).stdout)
    ins = json.loads(heat(base + ["--insulated", "all"], tmp_path).stdout)
    assert ins["halo"] > 0 and ins["halo"] == ins["tb_depth"] * ins["halo_passes"]
    assert ins["halo_passes"] > 1 and ins["bytes_per_gpu"] > plain["bytes_per_gpu"]


def test_config_validates_sides():
    with pytest.raises(ValueError, match="nswe"):
        HeatConfig(insulated="q").validate()
    with pytest.raises(ValueError):
        HeatSolver(HeatConfig(backend="cpu", insulated="nq"))
    assert HeatConfig(insulated="all").to_native().insulated == 15
    assert HeatConfig(insulated="en").to_native().insulated == 9
    assert HeatConfig().to_native().insulated == 0
