"""The heat source without a GPU: the host twin of the source step against the
NumPy oracle reference.step_np_fma(source=), the CPU backend against
reference.run_np(source=) on every edge mode, exact conservation on a torus,
the ghost rule across gloo ranks, the lifecycle, both CLIs, the stand-alone
self-test (plain and under ASan/UBSan) and the zero-scratch guardrail of the
device kernels (read from the built library's code objects)."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from parallel_heat_amd import HeatConfig, HeatSolver, _native, ops
from parallel_heat_amd.models import reference as R
from parallel_heat_amd.parallel.topology import layout
from parallel_heat_amd.utils import io as hio

from . import source_cases as C
from .source_worker import run_world

ROOT = str(_native.REPO_DIR)
HEAT = str(_native.CLI_PATH)
PY = [sys.executable, "-m", "parallel_heat_amd"]
CPU = "cpu"


def test_oracle_source_is_one_more_rounded_add():
    u = C.values("signed", (9, 11), 1)
    q = C.values("signed", (9, 11), 2)
    plain, with_q = R.step_np_fma(u, 0.05, 0.2), R.step_np_fma(u, 0.05, 0.2, source=q)
    want = plain.copy()
    want[1:-1, 1:-1] = plain[1:-1, 1:-1] + q[1:-1, 1:-1]
    C.assert_bitwise(with_q, want, "interior + q, ring untouched")
    # Edge cells of insulated sides and periodic axes take their q too.
    t = R.step_np_fma(u, 0.05, 0.2, "n", "y", source=q)
    p = R.step_np_fma(u, 0.05, 0.2, "n", "y")
    want = p + q
    want[-1, :] = p[-1, :]          # the fixed south edge ignores q
    C.assert_bitwise(t, want, "insulated north, periodic y")
    # q = +0: the plain step except that a -0 result becomes +0.
    z = np.full((3, 3), -0.0, np.float32)
    z[0, 1] = z[1, 2] = -np.float32(2.0) ** -149
    assert C.bits(R.step_np_fma(z))[1, 1] == 0x80000000
    assert C.bits(R.step_np_fma(z, source=np.zeros((3, 3), np.float32)))[1, 1] == 0


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("coef", C.COEFS, ids=str)
def test_host_twin_matches_oracle(coef, kind):
    for plate in C.PLATES:
        C.check_step(CPU, plate, coef, kind)
    nx, ny = 24, 560
    for c0 in (4, 5, 6, 7):
        for c1 in (541, 542, 543, 544):
            C.check_step(CPU, (nx, ny), coef, kind, box=(3, 19, c0, c1))
    for d in (1, 2, 3, 5):   # blocks d columns from the plate's east and west edges
        C.check_step(CPU, (30, 90), coef, kind, block=(7, 90 - d - 40, 12, 40))
        C.check_step(CPU, (30, 90), coef, kind, block=(7, d, 12, 40))
    C.check_step(CPU, (21, 519), coef, kind, raw=(527, 1))
    C.check_step(CPU, (21, 519), coef, kind, raw=(528, 3))


def test_host_twin_residual_and_zero_source():
    plate, coef = (13, 37), C.COEFS[0]
    # A word already set higher is kept.
    high = C.word_of(3e38)
    *_, word = C.run_step(CPU, plate, coef, "signed", resid0=high)
    assert word == high
    # A NaN in q inside the box gives a NaN residual, one just outside does not.
    q = C.values("signed", plate, 7)
    q[5, 20] = np.nan
    *_, word = C.run_step(CPU, plate, coef, "signed", box=(2, 9, 3, 20), q_plate=q, resid0=0)
    assert not np.isnan(np.uint32(word).view(np.float32))
    got, (bi, bj), want, _, word = C.run_step(CPU, plate, coef, "signed", box=(2, 9, 3, 21),
                                              q_plate=q, resid0=0)
    assert np.isnan(np.uint32(word).view(np.float32))
    assert np.isnan(got[bi, bj][3, 17]) and np.isnan(got[bi, bj]).sum() == 1
    # q = 0 equals the oracle's step + 0.0f.
    got, (bi, bj), want, _, _ = C.run_step(CPU, plate, coef, "subnormal",
                                           q_plate=np.zeros(plate, np.float32), resid0=0)
    u = C.values("subnormal", plate, 0)
    plain = R.step_np_fma(u, *coef)
    plus0 = plain.copy()
    plus0[1:-1, 1:-1] = plain[1:-1, 1:-1] + np.float32(0)
    C.assert_bitwise(got[bi, bj], plus0, "q = 0")


@pytest.mark.parametrize("case", C.SOLVER_CASES, ids=str)
@pytest.mark.parametrize("edges", C.EDGES, ids=C.EDGE_IDS)
def test_cpu_solver_matches_oracle(edges, case):
    C.check_solver(CPU, case, edges)


@pytest.mark.parametrize("plate", C.CONSERVATION_PLATES, ids=str)
def test_conservation_exact(plate):
    def one(cfg, fn):
        with HeatSolver(cfg.replace(backend=CPU)) as s:
            return fn(s)
    C.check_conservation(one, plate)


def test_convergence_matches_prediction():
    case, edges = C.SOLVER_CASES[0], dict(insulated="ns")
    nx, ny, fx, fy, order = case
    # A weak source on a random plate: the step-to-step change falls below eps
    # while the field still smooths (the oracle predicts where).
    S = (C.source_map(*C.dims(nx, ny, fx, fy)) * 0.01).astype(np.float32)
    kw = dict(converge=True, check_interval=5, eps=0.25)
    _, (want, done, at) = C.solver_want(case, edges, steps=100, S=S, **kw)
    assert 5 < at < 100 and at % 5 == 0, at
    with HeatSolver(C.solver_cfg(case, edges, CPU, steps=100, **kw)) as s:
        s.set_source(S, fx, fy, order)
        r = s.run()
        assert (r.converged, r.converged_at, r.steps_done) == (True, at, done)
        C.assert_bitwise(s.gather(), want, "converged state")


def test_nan_in_map_raises_at_first_check():
    case = C.SOLVER_CASES[0]
    nx, ny, fx, fy, order = case
    S = C.source_map(*C.dims(nx, ny, fx, fy))
    S[3, 2] = np.nan
    with HeatSolver(C.solver_cfg(case, {}, CPU, converge=True, check_interval=5)) as s:
        s.set_source(S, fx, fy, order)
        with pytest.raises(_native.NativeError, match="non-finite"):
            s.run()


@pytest.mark.parametrize("m", [0, 1, 4], ids=["m-auto", "m1", "m4"])
@pytest.mark.parametrize("edges", C.EDGES, ids=C.EDGE_IDS)
def test_gloo_ranks_and_the_ghost_rule(tmp_path, edges, m):
    # 2 x 2 ranks, blocks of 40 x 40: with 4 passes per exchange every pass
    # after an exchange reads ghost q; the worker checks each rank's extended
    # source block against the plate indexed through the map (the CPU backend's
    # default is one pass per exchange).
    case = (80, 80, 5, 3, 1)
    nx, ny, fx, fy, order = case
    S = C.source_map(*C.dims(nx, ny, fx, fy))
    cfg = dict(nx=nx, ny=ny, steps=0, init="random", seed=3, backend=CPU, source=True, px=2, py=2,
               halo_passes=m, **edges)
    res = run_world(4, cfg, S, case, edges, 13, tmp_path)
    assert (int(res["px"]), int(res["py"]), int(res["halo"])) == (2, 2, m or 1)
    _, (want, _, _) = C.solver_want(case, edges, steps=13, S=S)
    C.assert_bitwise(res["grid"], want, ("2x2 gloo ranks", edges, m))


def test_lifecycle(tmp_path):
    case, edges = C.SOLVER_CASES[1], dict(periodic="y")
    nx, ny, fx, fy, order = case
    S, (want, _, _) = C.solver_want(case, edges)
    # Without the option set_source raises, naming it; an explicit tb kernel
    # or the mpi numerics with a source raise; so does src without one.
    with HeatSolver(HeatConfig(nx=nx, ny=ny, backend=CPU)) as s:
        with pytest.raises(_native.NativeError, match="source"):
            s.set_source(S, fx, fy, order)
    for bad in (dict(source=True, kernel="tb"), dict(source=True, numerics="mpi"),
                dict(kernel="src")):
        with pytest.raises(ValueError, match="source"):
            HeatConfig(nx=nx, ny=ny, backend=CPU, **bad).validate()
    # The C ABI rejects them too (a front end of its own would meet these).
    ext = _native.HeatParamsExt(ctypes.sizeof(_native.HeatParamsExt), 1)
    for field, value in (("kernel", 2), ("numerics", 1)):
        p = HeatConfig(nx=nx, ny=ny, backend=CPU).to_native()
        setattr(p, field, value)
        with pytest.raises(_native.NativeError, match="source"):
            _native.call("heat_solver_create_ex", p, ext, None, ctypes.c_void_p())
    u0 = R.init_grid(nx, ny, "random", 3)
    with HeatSolver(C.solver_cfg(case, edges, CPU)) as s:
        # All +0 until set: the plain run, a -0 aside (none here: compare values).
        s.run(7)
        plain, _, _ = R.run_np(nx, ny, 7, u0=u0, numerics="fma", **edges)
        assert np.array_equal(s.gather(), plain)
        s.set_source(S, fx, fy, order)
        # reset, refine, load_local keep the source.
        s.reset()
        s.run()
        C.assert_bitwise(s.gather(), want, "after reset")
        s.load_local(u0)
        s.run(C.STEPS)
        C.assert_bitwise(s.gather(), want, "after load_local")
        s.refine(u0, 1, 1, order=0)
        s.run(C.STEPS)
        C.assert_bitwise(s.gather(), want, "after refine")
        # coarse() in the middle leaves the continued run bitwise; so do a
        # save and a new solver that loads it and sets the source again.
        s.reset()
        s.run(11)
        s.coarse(4, 8)
        s.save(str(tmp_path / "ck.bin"))
        s.run(C.STEPS - 11)
        C.assert_bitwise(s.gather(), want, "coarse() in the middle")
        assert hio.read_bin_header(str(tmp_path / "ck.bin"))["step"] == 11
        # set_source(None) then equals a zero-source run.
        s.set_source(None)
        s.reset()
        s.run()
        zero, _, _ = R.run_np(nx, ny, C.STEPS, u0=u0, numerics="fma",
                              source=np.zeros((nx, ny), np.float32), **edges)
        C.assert_bitwise(s.gather(), zero, "cleared source")
    with HeatSolver(C.solver_cfg(case, edges, CPU)) as s:
        s.load(str(tmp_path / "ck.bin"))
        assert s.step == 11
        s.set_source(S, fx, fy, order)
        s.run()
        C.assert_bitwise(s.gather(), want, "resumed")
    assert _native.lib().heat_abi_version() == 9 == _native.ABI_VERSION


def _run(cmd, cwd, check=True):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=300, check=check,
                          env=dict(os.environ, PYTHONPATH=ROOT))


PLATE = ["--backend", "cpu", "--nx", "70", "--ny", "519"]


@pytest.fixture(scope="module")
def heater(tmp_path_factory):
    """A source map (18 x 65) in the binary grid format."""
    d = tmp_path_factory.mktemp("heater")
    S = C.source_map(18, 65)
    hio.write_bin(str(d / "q.bin"), S)
    return str(d / "q.bin"), S


@pytest.mark.parametrize("extra,order,per", [([], 1, ""), (["--source-order", "0", "--source-refine",
                                                            "4x8", "--periodic", "y"], 0, "y")],
                         ids=["inferred", "order0-periodic"])
def test_both_clis_run_with_a_source(tmp_path, heater, extra, order, per):
    path, S = heater
    outs = {}
    for name, cmd in (("native", [HEAT]), ("python", PY)):
        d = tmp_path / name
        d.mkdir()
        p = _run(cmd + PLATE + ["--steps", "9", "--init", "random", "--seed", "3", "--source-from",
                                path, "--out-format", "bin", "--out", "final.bin", "--json"]
                 + extra, d)
        m = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
        assert m["source"] == {"path": path, "rows": 18, "cols": 65, "fx": 4, "fy": 8,
                               "order": order}
        assert m["steps_done"] == 9
        outs[name] = (d / "final.bin").read_bytes()
    assert outs["native"] == outs["python"]
    q = R.refine_np(S, 70, 519, 4, 8, order, per)
    want, _, _ = R.run_np(70, 519, 9, u0=R.init_grid(70, 519, "random", 3), numerics="fma",
                          periodic=per, source=q)
    last, h = hio.read_bin(str(tmp_path / "native" / "final.bin"), mmap=False)
    assert h["step"] == 9
    C.assert_bitwise(last, want, "heat --source-from, 9 steps")


@pytest.mark.parametrize("cmd", [[HEAT], PY], ids=["native", "python"])
def test_cli_refuses_bad_source(tmp_path, heater, cmd):
    path, _ = heater
    base = cmd + PLATE + ["--steps", "1", "--out", "none"]
    p = _run(base + ["--source-from", path, "--source-refine", "5x8"], tmp_path, check=False)
    assert p.returncode != 0, p.stdout
    for number in ("18x65", "5x8", "70x519", "14x65"):
        assert number in p.stderr, p.stderr
    p = _run(base + ["--source-refine", "4x8"], tmp_path, check=False)
    assert p.returncode != 0 and "--source-refine needs --source-from" in p.stderr, p.stderr
    p = _run(base + ["--source-from", str(tmp_path / "missing.bin")], tmp_path, check=False)
    assert p.returncode != 0 and "missing.bin" in p.stderr, p.stderr
    p = _run(base + ["--source-from", path, "--numerics", "mpi"], tmp_path, check=False)
    assert p.returncode != 0 and "--numerics" in p.stderr, p.stderr
    p = _run(base + ["--source-from", path, "--kernel", "tb"], tmp_path, check=False)
    assert p.returncode != 0 and "--kernel tb" in p.stderr, p.stderr
    p = _run(base + ["--kernel", "src"], tmp_path, check=False)
    assert p.returncode != 0 and "--source-from" in p.stderr, p.stderr


def test_plan_counts_the_third_field(tmp_path):
    # 16384 x 16384 on one rank at depth 4: no resident tiles, ghost depth 4.
    S = C.source_map(64, 64)
    hio.write_bin(str(tmp_path / "big.bin"), S)
    base = [HEAT, "--plan", "--nx", "16384", "--ny", "16384", "--tb-depth", "4"]
    a = json.loads(_run(base, tmp_path).stdout)
    b = json.loads(_run(base + ["--source-from", str(tmp_path / "big.bin")], tmp_path).stdout)
    pitch, rows, _, _ = layout(16384, 16384, 4)
    assert a["bytes_per_gpu"] == 2 * pitch * rows * 4
    assert b["bytes_per_gpu"] - a["bytes_per_gpu"] == pitch * rows * 4
    assert b["resident"] is False


@pytest.mark.parametrize("target", ["source-selftest", "source-selftest-asan"])
def test_standalone_selftest(target):
    # The host code alone in a program of its own; nothing loaded into Python
    # runs under a sanitizer.
    p = subprocess.run(["make", "-s", "-C", ROOT, target], capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "source selftest: ok" in p.stdout


def test_source_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    lib = os.path.join(ROOT, "parallel_heat_amd", "_lib", "libheat.so")
    from kernel_resources import kernels
    ks = [k for k in kernels(lib) if re.search(r"source_kernel", k["name"])]
    assert len(ks) == 2, [k["name"] for k in ks]   # plain and non-temporal
    bad = [(k["name"], k["scratch"]) for k in ks
           if k["scratch"] > 0 or k.get("vgpr_spill", 0) > 0]
    assert not bad, bad
    # The residual's two words are the kernel's only LDS.
    assert all(k.get("lds", 0) <= 8 for k in ks), [(k["name"], k.get("lds")) for k in ks]
