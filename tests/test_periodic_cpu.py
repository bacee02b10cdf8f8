"""Periodic (wrap-around) plate edges, per axis, without a GPU: the NumPy
oracle's properties, the host ghost fill, the CPU backend bitwise against the
oracle on one rank and on process grids whose opposite sides share a peer,
the topology mirror and the front ends.

On a periodic axis the edge cells are updated like interior cells, the missing
neighbour being the cell at the other end of the axis (u[-1, j] := u[nx-1, j]).
Axes: x = rows (north and south edges joined), y = columns (west and east)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from parallel_heat_amd import HeatConfig, HeatSolver, _native, ops
from parallel_heat_amd.models import reference as R
from parallel_heat_amd.parallel.topology import Cart
from parallel_heat_amd.utils import io as hio

from .dist_worker import free_port, run_world

HEAT = str(_native.CLI_PATH)
# (periodic, insulated) of the CPU backend cases.
MODES = [("x", ""), ("y", ""), ("xy", ""), ("y", "n"), ("y", "ns")]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# --------------------------------------------------------------------------
# the oracle
# --------------------------------------------------------------------------
def roll_step_fma(u, cx, cy):
    """heat::stencil on a fully periodic plate, written with np.roll."""
    n, s = np.roll(u, 1, 0), np.roll(u, -1, 0)
    w, e = np.roll(u, 1, 1), np.roll(u, -1, 1)
    with np.errstate(over="ignore", invalid="ignore"):
        ns, ew = s + n, e + w
    m2 = np.float32(-2.0)
    tx, ty = R.fma32(m2, u, ns), R.fma32(m2, u, ew)
    return R.fma32(np.float32(cy), ty, R.fma32(np.float32(cx), tx, u))


@pytest.mark.parametrize("nx,ny", [(37, 53), (1, 40), (40, 1), (2, 2), (1, 1)])
def test_oracle_bitwise_vs_roll(nx, ny):
    a = b = R.init_grid(nx, ny, "random", 4)
    for k in range(20):
        a, b = R.step_np_fma(a, 0.1, 0.23, periodic="xy"), roll_step_fma(b, 0.1, 0.23)
        assert a.shape == (nx, ny) and np.array_equal(bits(a), bits(b)), k


def test_oracle_mixed_edges():
    u = R.init_grid(9, 14, "random", 6)
    v = R.step_np_fma(u, 0.1, 0.23, insulated="n", periodic="y")
    assert np.array_equal(bits(v[8]), bits(u[8]))  # the fixed south edge, corners included
    assert not np.any(v[0] == u[0])                # the insulated north edge moves, every column
    # Column 0's west neighbour is column 13; row 0's north neighbour is row 1.
    c, n, s, w, e = u[3, 0], u[2, 0], u[4, 0], u[3, 13], u[3, 1]
    m2, one = np.float32(-2.0), (1,)
    want = R.fma32(np.float32(0.23), R.fma32(m2, c, np.reshape(e + w, one)),
                   R.fma32(np.float32(0.1), R.fma32(m2, c, np.reshape(s + n, one)), c))
    assert bits(v[3, 0]) == bits(want)[0]
    for f in (R.step_np, R.step_np_fma, R.step_np_mpi):
        with pytest.raises(ValueError, match="axis y"):
            f(u, periodic="y", insulated="w")
        with pytest.raises(ValueError, match="axis x"):
            f(u, periodic="xy", insulated="s")
        with pytest.raises(ValueError):
            f(u, periodic="z")


def test_oracle_torch_step_matches_numpy():
    u = R.init_grid(19, 23, "random", 8)
    for per, ins in MODES + [("x", "we"), ("x", "e")]:
        got = R.step_torch(torch.from_numpy(u), 0.1, 0.1, insulated=ins, periodic=per).numpy()
        want = R.step_np(u, insulated=ins, periodic=per)
        assert np.allclose(got, want, rtol=0, atol=1e-4), (per, ins)
    one = R.init_grid(1, 23, "random", 8)
    assert np.allclose(R.step_torch(torch.from_numpy(one), periodic="x").numpy(),
                       R.step_np(one, periodic="x"), rtol=0, atol=1e-4)


def test_oracle_default_arguments_unchanged():
    u = R.init_grid(37, 53, "random", 2)
    c = u[1:-1, 1:-1]
    plain = u.copy()
    two = np.float32(2.0)
    plain[1:-1, 1:-1] = (c + np.float32(0.1) * ((u[2:, 1:-1] + u[:-2, 1:-1]) - two * c)) + \
        np.float32(0.1) * ((u[1:-1, 2:] + u[1:-1, :-2]) - two * c)
    assert np.array_equal(bits(R.step_np(u)), bits(plain))
    assert np.array_equal(bits(R.step_np(u, periodic="")), bits(plain))
    t = torch.from_numpy(u)
    assert torch.equal(R.step_torch(t), R.step_torch(t, periodic=""))
    for step in (R.step_np_fma, R.step_np_mpi):
        assert np.array_equal(bits(step(u)), bits(step(u, 0.1, 0.1, "", "")))
        # Insulated sides alone: the one-call reflect pad of before.
        pad = np.pad(u, ((1, 0), (0, 1)), mode="reflect")
        assert np.array_equal(bits(step(u, insulated="ne")), bits(step(pad)[1:, :-1]))
    assert R.run_np(37, 53, 5, init="random", seed=2)[0].tobytes() == \
        R.run_np(37, 53, 5, init="random", seed=2, periodic="")[0].tobytes()
    # The engine with no periodic axis: the Dirichlet program, same ghost depth.
    with HeatSolver(HeatConfig(nx=37, ny=53, init="random", seed=2, backend="cpu")) as s:
        s.run(3)
        assert s.info.periodic == "" and s.info.halo == 1
        assert np.array_equal(bits(s.gather()), bits(R.run_np(37, 53, 3, init="random", seed=2,
                                                              numerics="fma")[0]))


def integer_plate():
    return np.random.default_rng(11).integers(0, 100, (12, 20)).astype(np.float32)


def test_exact_conservation():
    # A fully periodic plate keeps its total heat.  Integers below 128 (7
    # bits) with cx = 1/4, cy = 1/8: a step adds at most 3 fraction bits and
    # the values stay in [0, 100), so every fp32 operation is exact while
    # 7 + 3 k <= 24 (k <= 5), and the sum is constant bit for bit.
    u = integer_plate()
    total = float(u.astype(np.float64).sum())
    for step in (R.step_np_fma, R.step_np):
        a = u
        for k in range(4):
            a = step(a, 0.25, 0.125, periodic="xy")
            assert float(a.astype(np.float64).sum()) == total, (step.__name__, k)
    assert not np.array_equal(a, u)
    cfg = HeatConfig(nx=12, ny=20, steps=4, cx=0.25, cy=0.125, init="zero", backend="cpu",
                     periodic="xy")
    with HeatSolver(cfg) as s:
        s.scatter(u)
        s.run()
        g = s.gather()
    assert np.array_equal(bits(g), bits(a))
    assert float(g.astype(np.float64).sum()) == total


@functools.lru_cache(maxsize=None)
def converging_oracle():
    return R.run_np(24, 28, 3000, converge=True, init="random", seed=3, numerics="fma",
                    periodic="x")


# --------------------------------------------------------------------------
# the host ghost fill (the twin of the HIP kernel)
# --------------------------------------------------------------------------
def nan_payload_field(lx, ly, halo, device, rng):
    """A field of random owned cells whose every other cell is a NaN with a
    payload of its own (a fill that writes a wrong cell changes bits)."""
    f = ops.Field(lx, ly, halo, device)
    shape = tuple(f.data.shape)
    a = (np.uint32(0x7FC00000) + np.arange(shape[0] * shape[1], dtype=np.uint32)
         .reshape(shape) % np.uint32(0x3FFFFF)).view(np.float32).copy()
    a[f.hx:f.hx + lx, f.hy:f.hy + ly] = rng.random((lx, ly), np.float32)
    f.data.copy_(torch.from_numpy(a))
    return f, a


def edge_fill_expected(full, hx, hy, lx, ly, ins, per, d):
    """The field array after the fill: every cell of the frame [-d, lx+d) x
    [-d, ly+d) beyond a filled side takes its per-axis source."""
    def src(i, n, lo, hi, wrap):
        if i < 0:
            return i + n if wrap else -i if lo else i
        if i >= n:
            return i - n if wrap else 2 * (n - 1) - i if hi else i
        return i
    want = full.copy()
    for r in range(-d, lx + d):
        sr = src(r, lx, "n" in ins, "s" in ins, "x" in per)
        for c in range(-d, ly + d):
            sc = src(c, ly, "w" in ins, "e" in ins, "y" in per)
            if (sr, sc) != (r, c):
                want[hx + r, hy + c] = full[hx + sr, hy + sc]
    return want


FILL_MODES = [("x", ""), ("y", ""), ("xy", ""), ("x", "w"), ("x", "e"), ("x", "we")]


@pytest.mark.parametrize("lx,ly,halo,d", [(9, 14, 5, 5), (9, 14, 5, 2), (6, 7, 3, 1)])
def test_host_fill_edge_ghosts(lx, ly, halo, d):
    rng = np.random.default_rng(lx * ly)
    for per, ins in FILL_MODES:
        f, before = nan_payload_field(lx, ly, halo, "cpu", rng)
        ops.fill_edge_ghosts(f, ins, per, d)
        got = f.data.numpy()
        # Cells beyond fixed sides, deeper than d and the padding: bit-unchanged.
        want = edge_fill_expected(before, f.hx, f.hy, lx, ly, ins, per, d)
        assert np.array_equal(bits(got), bits(want)), (per, ins)
        # The depth-1 frame is np.pad's, axis by axis.
        px, py = int("x" in per), int("y" in per)
        n0, n1 = max(px, int("n" in ins)), max(px, int("s" in ins))
        w0, w1 = max(py, int("w" in ins)), max(py, int("e" in ins))
        own = before[f.hx:f.hx + lx, f.hy:f.hy + ly]
        pad = np.pad(own, ((n0, n1), (0, 0)), mode="wrap" if px else "reflect")
        pad = np.pad(pad, ((0, 0), (w0, w1)), mode="wrap" if py else "reflect")
        frame = got[f.hx - n0:f.hx + lx + n1, f.hy - w0:f.hy + ly + w1]
        assert np.array_equal(bits(frame), bits(pad)), (per, ins)
    f = ops.Field(lx, ly, halo, "cpu")
    with pytest.raises(ValueError):
        ops.fill_edge_ghosts(f, "", "x", halo + 1)
    with pytest.raises(ValueError, match="axis x"):
        ops.fill_edge_ghosts(f, "n", "x", 1)
    # fill_insulated_ghosts is the general fill with no periodic axis.
    a, before = nan_payload_field(lx, ly, halo, "cpu", rng)
    b = ops.Field(lx, ly, halo, "cpu")
    b.data.copy_(a.data)
    ops.fill_insulated_ghosts(a, "ne", d)
    ops.fill_edge_ghosts(b, "ne", "", d)
    assert np.array_equal(bits(a.data.numpy()), bits(b.data.numpy()))


def test_host_fill_wraps_a_thin_field():
    # A wrapped axis lends its whole extent: depth == extent, and extent 1.
    rng = np.random.default_rng(1)
    for lx, ly, d, per in ((3, 8, 3, "x"), (1, 8, 1, "x"), (6, 2, 2, "y")):
        f, before = nan_payload_field(lx, ly, 4, "cpu", rng)
        ops.fill_edge_ghosts(f, "", per, d)
        want = edge_fill_expected(before, f.hx, f.hy, lx, ly, "", per, d)
        assert np.array_equal(bits(f.data.numpy()), bits(want)), (lx, ly, d)
    with pytest.raises(ValueError, match="wrap"):
        ops.fill_edge_ghosts(ops.Field(3, 8, 4, "cpu"), "", "x", 4)


# --------------------------------------------------------------------------
# the CPU backend
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_levels(nx, ny, per, ins="", numerics="fma", levels=(1, 48)):
    """Levels of the exact oracle from init random, seed 3."""
    step = {"fma": R.step_np_fma, "mpi": R.step_np_mpi}[numerics]
    u = R.init_grid(nx, ny, "random", 3)
    out = {}
    for k in range(1, max(levels) + 1):
        u = step(u, 0.1, 0.1, ins, per)
        if k in levels:
            out[k] = u
    return out


def cpu_run(nx, ny, steps, per, ins="", **kw):
    cfg = HeatConfig(nx=nx, ny=ny, steps=steps, init="random", seed=3, backend="cpu",
                     periodic=per, insulated=ins, **kw)
    with HeatSolver(cfg) as s:
        r = s.run()
        return s.gather(), r, s.info


@pytest.mark.parametrize("nx,ny,per,ins", [(nx, ny, p, i) for nx, ny in ((37, 53), (20, 20))
                                           for p, i in MODES])
def test_cpu_backend_bitwise_vs_oracle(nx, ny, per, ins):
    want = oracle_levels(nx, ny, per, ins)
    for steps in (1, 48):
        for threads in (1, 4):
            for depth in (1, 4):
                g, r, info = cpu_run(nx, ny, steps, per, ins, threads=threads, tb_depth=depth)
                assert r.steps_done == steps and info.periodic == per and info.halo == depth
                assert info.insulated == ins
                assert np.array_equal(bits(g), bits(want[steps])), (steps, threads, depth)


def test_cpu_backend_deep_halo_and_chunks():
    want = oracle_levels(37, 53, "xy")[48]
    cfg = HeatConfig(nx=37, ny=53, init="random", seed=3, backend="cpu", periodic="xy",
                     tb_depth=3, halo_passes=4)
    with HeatSolver(cfg) as s:
        assert s.info.halo == 12 and s.info.periodic == "xy" and s.info.nbr == (-1,) * 4
        ex = sum(s.run(n).exchanges for n in (5, 1, 17, 22, 3))
        assert np.array_equal(bits(s.gather()), bits(want))
    assert ex < 48 // 3


def test_cpu_backend_mpi_numerics():
    want = oracle_levels(37, 53, "xy", "", "mpi")[48]
    g, _, _ = cpu_run(37, 53, 48, "xy", numerics="mpi", tb_depth=2)
    assert np.array_equal(bits(g), bits(want))


def test_cpu_backend_convergence_matches_oracle():
    # A fully periodic plate never reaches a fixed value, but it flattens;
    # with the west and east edges fixed the run converges like any other.
    want, done, at = converging_oracle()
    assert at > 0 and done == at
    cfg = HeatConfig(nx=24, ny=28, steps=3000, converge=True, init="random", seed=3,
                     backend="cpu", periodic="x")
    with HeatSolver(cfg) as s:
        r = s.run()
        g = s.gather()
    assert r.converged and r.converged_at == at and r.steps_done == done
    assert np.array_equal(bits(g), bits(want))


def test_cpu_backend_thin_plates():
    # A periodic axis lends its whole extent: 5 columns, 5 ghost columns.
    g, _, info = cpu_run(20, 5, 9, "y", tb_depth=8)
    assert info.tb_depth == 5 and info.halo == 5
    assert np.array_equal(bits(g), bits(oracle_levels(20, 5, "y", levels=(9,))[9]))
    # Extent 1: each cell is its own neighbour along x.
    g, _, info = cpu_run(1, 30, 9, "x", tb_depth=4)
    assert info.halo == 1
    assert np.array_equal(bits(g), bits(oracle_levels(1, 30, "x", levels=(9,))[9]))
    assert not np.array_equal(g[:, 1:-1], R.init_grid(1, 30, "random", 3)[:, 1:-1])
    with pytest.raises(ValueError, match="axis y"):
        cpu_run(20, 20, 1, "y", "e")
    # The native engine rejects the clash itself (here past the Python check).
    cfg = HeatConfig(backend="cpu", periodic="x", insulated="s")
    cfg.validate = lambda: None
    with pytest.raises(_native.NativeError, match="axis x"):
        HeatSolver(cfg)


# --------------------------------------------------------------------------
# ranks over gloo: opposite sides (corners) of a block share a peer
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def one_rank(per, ins):
    kw = dict(nx=37, ny=53, steps=0, init="random", seed=3, backend="cpu", periodic=per,
              insulated=ins)
    with HeatSolver(HeatConfig(**kw)) as s:
        s.run(29)
        return s.gather(), s.checksum()["hash"]


@pytest.mark.parametrize("world,grid,per,ins", [
    (2, dict(decomp="rows"), "x", ""),      # north and south are the same peer
    (4, dict(px=2, py=2), "xy", ""),        # so are west and east, and all four diagonals
    (4, dict(px=2, py=2), "x", "w"),        # two diagonals one peer, two missing
    (3, dict(decomp="rows"), "xy", ""),     # distinct peers on x, local wrap on y
])
def test_cpu_ranks_bitwise(tmp_path, world, grid, per, ins):
    kw = dict(nx=37, ny=53, steps=0, init="random", seed=3, backend="cpu", periodic=per,
              insulated=ins, tb_depth=2, halo_passes=2, **grid)
    res = run_world(world, kw, 0, tmp_path, transport="torch", chunks=[7, 1, 13, 8])
    want, h = one_rank(per, ins)
    assert int(res["done"]) == 29 and set(res["halo"].tolist()) == {4}
    assert np.array_equal(bits(res["grid"]), bits(want))
    assert str(res["hash"]) == h
    assert np.array_equal(bits(want), bits(oracle_levels(37, 53, per, ins, levels=(29,))[29]))


def test_cli_tcp_two_ranks_same_peer(tmp_path):
    # Both messages of an exchange go through the one socket of the pair.
    port = free_port()
    base = ["--backend", "cpu", "--nx", "37", "--ny", "53", "--steps", "29", "--init", "random",
            "--seed", "3", "--periodic", "x", "--decomp", "rows", "--tb-depth", "2",
            "--halo-passes", "2", "--out", "g.bin", "--out-format", "bin", "--transport", "tcp",
            "--port", str(port)]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r),
                   MASTER_ADDR="127.0.0.1")
        procs.append(subprocess.Popen([HEAT] + base, cwd=tmp_path, env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=300) for p in procs]
    for p, (o, e) in zip(procs, outs):
        assert p.returncode == 0, e
    g, h = hio.read_bin(str(tmp_path / "g.bin"))
    assert h["step"] == 29
    assert np.array_equal(bits(np.asarray(g)), bits(one_rank("x", "")[0]))


# --------------------------------------------------------------------------
# topology (the Python mirror of heat::Cart)
# --------------------------------------------------------------------------
def test_topology_wrapped_neighbours():
    one = Cart(1, 1, 1)
    for mask in range(4):
        assert one.neighbors(0, mask) == (-1,) * 4 and one.diagonal_neighbors(0, mask) == (-1,) * 4
    rows = Cart(2, 2, 1)
    assert rows.neighbors(0, 1) == (1, 1, -1, -1) and rows.neighbors(1, 3) == (0, 0, -1, -1)
    assert rows.neighbors(0, 2) == (-1, 1, -1, -1)       # y has one rank: no wrap
    assert rows.diagonal_neighbors(0, 3) == (-1,) * 4
    g = Cart(4, 2, 2)
    assert g.neighbors(0, 3) == (2, 2, 1, 1) and g.diagonal_neighbors(0, 3) == (3, 3, 3, 3)
    assert g.neighbors(3, 3) == (1, 1, 2, 2) and g.diagonal_neighbors(3, 3) == (0, 0, 0, 0)
    assert g.neighbors(0, 1) == (2, 2, -1, 1) and g.diagonal_neighbors(0, 1) == (-1, 3, -1, 3)
    assert g.neighbors(0, 2) == (-1, 2, 1, 1) and g.diagonal_neighbors(0, 2) == (-1, -1, 3, 3)
    c = Cart(8, 4, 2)
    assert c.neighbors(0, 1) == (6, 2, -1, 1) and c.neighbors(7, 1) == (5, 1, 6, -1)
    assert c.neighbors(7, 3) == (5, 1, 6, 6)
    assert c.diagonal_neighbors(0, 3) == (7, 7, 3, 3)
    assert c.diagonal_neighbors(0, 1) == (-1, 7, -1, 3)
    assert c.diagonal_neighbors(6, 2) == (5, 5, -1, -1)
    for cart in (one, rows, g, c):
        for r in range(cart.world):
            cx, cy = cart.coords(r)
            assert cart.neighbors(r, 0) == cart.neighbors(r) == (
                cart.rank_of(cx - 1, cy), cart.rank_of(cx + 1, cy),
                cart.rank_of(cx, cy - 1), cart.rank_of(cx, cy + 1))
            assert cart.diagonal_neighbors(r, 0) == cart.diagonal_neighbors(r)
            assert cart.block(r, 40, 40, 3).nbr == cart.neighbors(r, 3)
            assert cart.block(r, 40, 40).nbr == cart.neighbors(r)


def test_topology_native_matches_mirror():
    with HeatSolver(HeatConfig(nx=20, ny=20, backend="cpu", periodic="xy")) as s:
        assert s.info.nbr == Cart(1, 1, 1).neighbors(0, 3)


# --------------------------------------------------------------------------
# front ends
# --------------------------------------------------------------------------
def heat(args, cwd, check=True):
    return subprocess.run([HEAT] + args, cwd=cwd, env=dict(os.environ), capture_output=True,
                          text=True, check=check, timeout=300)


RUN = ["--backend", "cpu", "--nx", "37", "--ny", "53", "--steps", "48", "--init", "random",
       "--seed", "3"]


def test_cli_periodic_dat_matches_oracle(tmp_path):
    p = heat(RUN + ["--periodic", "x", "--out", "x.dat", "--json"], tmp_path)
    ref = tmp_path / "ref.dat"
    hio.write_dat(str(ref), oracle_levels(37, 53, "x")[48])
    assert (tmp_path / "x.dat").read_bytes() == ref.read_bytes()
    m = json.loads(p.stdout.splitlines()[-1])
    assert m["periodic"] == "x" and m["insulated"] == "" and m["schedule"] == "sync"
    assert m["halo"] >= 1
    plain = json.loads(heat(RUN + ["--out", "none", "--json"], tmp_path).stdout.splitlines()[-1])
    assert plain["periodic"] == ""


def test_cli_python_front_end_periodic(tmp_path):
    p = subprocess.run([sys.executable, "-m", "parallel_heat_amd"] + RUN +
                       ["--periodic", "yx", "--out", "xy.dat", "--json"], cwd=tmp_path,
                       env={**os.environ, "PYTHONPATH": str(_native.REPO_DIR)},
                       capture_output=True, text=True, check=True, timeout=300)
    ref = tmp_path / "ref.dat"
    hio.write_dat(str(ref), oracle_levels(37, 53, "xy")[48])
    assert (tmp_path / "xy.dat").read_bytes() == ref.read_bytes()
    assert json.loads(p.stdout.splitlines()[-1])["periodic"] == "xy"


def test_clis_reject_bad_axes_and_clashes(tmp_path):
    py = [sys.executable, "-m", "parallel_heat_amd"]
    env = {**os.environ, "PYTHONPATH": str(_native.REPO_DIR)}
    for args, word in ((["--periodic", "z"], "xy"), (["--periodic", "n"], "xy"),
                       (["--periodic", "x", "--insulated", "s"], "axis x"),
                       (["--insulated", "we", "--periodic", "xy"], "axis y")):
        p = heat(["--backend", "cpu"] + args, tmp_path, check=False)
        assert p.returncode != 0 and word in p.stderr, (args, p.stderr)
        q = subprocess.run(py + ["--backend", "cpu"] + args, cwd=tmp_path, env=env,
                           capture_output=True, text=True, timeout=300)
        assert q.returncode != 0 and word in q.stderr, (args, q.stderr)
        assert not list(tmp_path.iterdir())


def test_cli_plan_counts_periodic_ghosts(tmp_path):
    base = ["--plan", "--nx", "8192", "--ny", "8192"]
    plain = json.loads(heat(base, tmp_path).stdout)
    per = json.loads(heat(base + ["--periodic", "xy"], tmp_path).stdout)
    ins = json.loads(heat(base + ["--insulated", "all"], tmp_path).stdout)
    assert per["halo"] > 0 and per["halo"] == per["tb_depth"] * per["halo_passes"]
    assert per["halo_passes"] > 1 and per["bytes_per_gpu"] > plain["bytes_per_gpu"]
    assert (per["halo"], per["bytes_per_gpu"]) == (ins["halo"], ins["bytes_per_gpu"])
    # A periodic axis lends its whole extent, an insulated one a row less.
    thin = ["--plan", "--nx", "24", "--ny", "4096", "--tb-depth", "12", "--halo-passes", "8"]
    assert json.loads(heat(thin + ["--periodic", "x"], tmp_path).stdout)["halo"] == 24
    assert json.loads(heat(thin + ["--insulated", "n"], tmp_path).stdout)["halo"] == 12


def test_config_validates_axes():
    with pytest.raises(ValueError, match="xy"):
        HeatConfig(periodic="q").validate()
    with pytest.raises(ValueError, match="axis x"):
        HeatConfig(periodic="x", insulated="n").validate()
    with pytest.raises(ValueError, match="axis y"):
        HeatSolver(HeatConfig(backend="cpu", periodic="xy", insulated="e"))
    HeatConfig(periodic="x", insulated="we").validate()
    assert HeatConfig(periodic="yx").to_native().periodic == 3
    assert HeatConfig(periodic="y").to_native().periodic == 2
    assert HeatConfig().to_native().periodic == 0


def test_model_halo_rule_follows_the_plan(tmp_path):
    # parallel.model mirrors the native halo rule (heat --plan): a periodic
    # axis counts as decomposed, also on one GPU, and lends its whole extent.
    from parallel_heat_amd.parallel.model import RES_MIN_PASSES, predict, resident_halo_passes
    cases = [(8192, 8192, 1, [], 1, 1), (1024, 8192, 1, [], 1, 1), (8192, 8192, 4, [], 2, 2),
             (8192, 8192, 8, ["--decomp", "rows"], 8, 1), (300, 8192, 1, [], 1, 1),
             (40, 8192, 1, [], 1, 1)]
    for nx, ny, ranks, extra, px, py in cases:
        for per in ("x", "y", "xy"):
            plan = json.loads(heat(["--plan", "--nx", str(nx), "--ny", str(ny), "--gpus",
                                    str(ranks), "--periodic", per] + extra, tmp_path).stdout)
            rm = resident_halo_passes(nx, ny, px, py, periodic=per)
            want = rm if rm >= RES_MIN_PASSES else 8
            if "x" in per:
                want = min(want, nx // px // 12)
            if "y" in per:
                want = min(want, ny // py // 12)
            assert plan["halo_passes"] == want, (nx, ny, ranks, per, plan, rm)
            p = predict(HeatConfig(nx=nx, ny=ny, px=px, py=py, periodic=per), ranks)
            assert p["halo"] == plan["halo"] and p["resident"] == plan["resident"], (per, p, plan)
            assert p["schedule"] == "sync" and p["exchanges_per_1000"] > 0
    # No periodic axis: today's prediction, no ghosts on one GPU.
    assert resident_halo_passes(8192, 8192, 2, 2) == resident_halo_passes(8192, 8192, 2, 2,
                                                                          periodic="") == 5
    p = predict(HeatConfig(nx=8192, ny=8192), 1)
    assert p["halo"] == 12 and p["exchanges_per_1000"] == 0
