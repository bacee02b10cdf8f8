"""The heat source on the MI355X: the streaming source_step kernel through
ops.source_step against the NumPy oracle (whole and cut lanes, aligned and
unaligned origins and pitches, every loop of the kernel more than once, blocks
at their offsets, the residual word, the gate), Solver runs with a source on
one GPU (graphs on and off, every edge mode, gated and host-judged
convergence) and across loopback ranks with deep halos (the ghost rule), exact
conservation, the lifecycle and the `heat` CLI.  Equality is bitwise
throughout."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from parallel_heat_amd import HeatConfig, HeatSolver, _native, ops
from parallel_heat_amd.models import reference as R
from parallel_heat_amd.parallel.group import run_group
from parallel_heat_amd.utils import io as hio

from . import source_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[0, 1], ids=["plain", "nt"])
def nt(request):
    """Both instantiations of the kernel: plain accesses, and q loads and dst
    stores non-temporal (what a step over more than 256 MiB launches by
    default; no test plate is that large, so it is forced)."""
    ops.set_source_nontemporal(request.param)
    try:
        yield request.param
    finally:
        ops.set_source_nontemporal(-1)


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("coef", C.COEFS, ids=str)
def test_kernel_matches_oracle(gpu, nt, coef, kind):
    for plate in C.PLATES:
        C.check_step(gpu, plate, coef, kind)


@pytest.mark.parametrize("coef", C.COEFS, ids=str)
def test_sub_boxes_cut_lanes_at_every_element(gpu, nt, coef):
    # c0 in each residue mod 4 (the first lane starts 0..3 columns before the
    # box), c1 cutting the last lane after 1, 2, 3 and 4 of its cells.
    for c0 in (4, 5, 6, 7):
        for c1 in (541, 542, 543, 544):
            C.check_step(gpu, (24, 560), coef, "signed", box=(3, 19, c0, c1))
    for d in (1, 2, 3, 5):   # blocks d columns from the plate's east and west edges
        for kind in ("signed", "subnormal"):
            C.check_step(gpu, (30, 90), coef, kind, block=(7, 90 - d - 40, 12, 40))
            C.check_step(gpu, (30, 90), coef, kind, block=(7, d, 12, 40))
        C.check_step(gpu, (30, 600), coef, "wide", block=(d, 600 - d - 520, 20, 520))


@pytest.mark.parametrize("pitch,off", [(527, 1), (528, 1), (528, 2), (528, 3), (528, 4)],
                         ids=lambda v: str(v))
def test_unaligned_origin_and_pitch(gpu, nt, pitch, off):
    # Pitch 527 (no multiple of 4): every lane moves dwords; pitch 528: float4
    # rows whose first lane starts `off` mod 4 columns before the block.
    for ly in (516, 517, 518, 519):
        src, dst, q = C._fields(gpu, 21, ly, (pitch, off))
        plan = ops.source_plan(src, dst, q)
        assert plan["vector_rows"] == int(pitch % 4 == 0), plan
        assert plan["align"] == (off % 4 if pitch % 4 == 0 else 0), plan
        C.check_step(gpu, (21, ly), C.COEFS[0], "signed", raw=(pitch, off))


def test_arrays_out_of_phase_fall_back_to_dwords(gpu):
    # src and q one float apart modulo 16 bytes: no common float4 lanes.
    src = C.RawField(9, 300, 528, 4, gpu, 0.0)
    q = C.RawField(9, 300, 528, 5, gpu, 0.0)
    assert ops.source_plan(src, src, q)["vector_rows"] == 0


@pytest.mark.parametrize("kind", ["signed", "subnormal"])
def test_every_loop_runs_twice(gpu, nt, kind):
    # A shape from the planner's own constants: two chunks of max_chunk_rows
    # rows + 1 and two strips + 37 columns, the launch capped at kWaves waves:
    # the grid-stride loop, the row loop and the strips of a wave all run at
    # least twice.
    f = ops.Field(8, 8, halo=1, device=gpu)
    probe = ops.source_plan(f, f, f)
    strip_cols, max_rows = probe["strip_cols"], probe["max_chunk_rows"]
    assert (strip_cols, max_rows, probe["min_chunk_rows"], probe["waves_per_cu"]) == \
        (256, 64, 8, 16)
    kWaves = 2
    plate = (2 * max_rows + 1, 2 * strip_cols + 37)
    ops.set_source_max_waves(kWaves)
    try:
        g = ops.Field(*plate, halo=1, device=gpu)
        plan = ops.source_plan(g, g, g)
        for coef in C.COEFS:
            C.check_step(gpu, plate, coef, kind)
    finally:
        ops.set_source_max_waves(0)
    assert plan["waves"] == kWaves and plan["units"] >= 2 * kWaves, plan
    assert plan["strips"] == 3 and plan["chunks"] == 3 and plan["chunk_rows"] >= 2, plan
    assert plan["strips"] % kWaves != 0, plan   # so a wave meets more than one strip
    # The default launch (no cap) gives the same plate, in one round of waves.
    C.check_step(gpu, plate, C.COEFS[0], kind)
    plan = ops.source_plan(g, g, g)
    assert plan["waves"] == plan["units"] > kWaves, plan
    # The planner's own widths (strip_cols +- 1) are in C.PLATES: 255, 256, 257.
    assert strip_cols == 256


def test_residual_word(gpu, nt):
    plate, coef = (13, 37), C.COEFS[0]
    # A word already set higher is kept.
    high = C.word_of(3e38)
    *_, word = C.run_step(gpu, plate, coef, "signed", resid0=high)
    assert word == high
    # A NaN in q inside the box gives a NaN residual, one just outside does not.
    q = C.values("signed", plate, 7)
    q[5, 20] = np.nan
    *_, word = C.run_step(gpu, plate, coef, "signed", box=(2, 9, 3, 20), q_plate=q, resid0=0)
    assert not np.isnan(np.uint32(word).view(np.float32))
    got, (bi, bj), _, _, word = C.run_step(gpu, plate, coef, "signed", box=(2, 9, 3, 21),
                                           q_plate=q, resid0=0)
    assert np.isnan(np.uint32(word).view(np.float32))
    assert np.isnan(got[bi, bj][3, 17]) and np.isnan(got[bi, bj]).sum() == 1
    # Many workgroups, one word: the maximum over all of them.
    C.check_step(gpu, (300, 1100), coef, "wide")


def test_zero_source_and_closed_gate(gpu, nt):
    import torch
    plate, coef = (13, 300), C.COEFS[1]
    got, (bi, bj), _, _, _ = C.run_step(gpu, plate, coef, "subnormal",
                                        q_plate=np.zeros(plate, np.float32), resid0=0)
    plain = R.step_np_fma(C.values("subnormal", plate, 0), *coef)
    plus0 = plain.copy()
    plus0[1:-1, 1:-1] = plain[1:-1, 1:-1] + np.float32(0)
    C.assert_bitwise(got[bi, bj], plus0, "q = 0")
    # A closed gate writes nothing, not even the residual; an open one is no gate.
    for stop, wrote in ((1, False), (0, True)):
        gate = torch.tensor([stop, 0, 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=gpu)
        got, (bi, bj), want, _, word = C.run_step(gpu, plate, coef, "signed", resid0=0, gate=gate)
        if wrote:
            C.assert_bitwise(got[bi, bj], want, "open gate")
            assert word != 0
        else:
            assert np.all(got == np.float32(C.SENTINEL)) and word == 0


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("edges", C.EDGES, ids=C.EDGE_IDS)
def test_solver_matches_oracle_and_cpu(gpu, edges, graph):
    for case in C.SOLVER_CASES:
        got = C.check_solver("hip", case, edges, use_graph=graph, device=0)
        nx, ny, fx, fy, order = case
        S = C.source_map(*C.dims(nx, ny, fx, fy))
        with HeatSolver(C.solver_cfg(case, edges, "cpu")) as s:
            s.set_source(S, fx, fy, order)
            s.run()
            C.assert_bitwise(got, s.gather(), (case, edges, "hip vs cpu"))


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_solver_with_the_non_temporal_kernel(gpu, nt, graph):
    # Forced before the solver's first run, so that its graphs capture that
    # instantiation; deep halos and a gated check every 5 steps ride along.
    case, edges = C.SOLVER_CASES[2], dict(insulated="we", periodic="x")
    nx, ny, fx, fy, order = case
    kw = dict(converge=True, check_interval=5, eps=1e-30)   # checks that never converge
    S, (want, _, _) = C.solver_want(case, edges, **kw)
    with HeatSolver(C.solver_cfg(case, edges, "hip", use_graph=graph, device=0, halo_passes=4,
                                 **kw)) as s:
        s.set_source(S, fx, fy, order)
        r = s.run()
        assert r.steps_done == C.STEPS and not r.converged and s.info.halo == 4
        C.assert_bitwise(s.gather(), want, (nt, graph))


@pytest.mark.parametrize("host_checks", [False, True], ids=["gate", "host"])
def test_convergence_matches_prediction(gpu, monkeypatch, host_checks):
    if host_checks:
        monkeypatch.setenv("HEAT_HOST_CHECKS", "1")
    case, edges = C.SOLVER_CASES[0], dict(insulated="ns")
    nx, ny, fx, fy, order = case
    S = (C.source_map(*C.dims(nx, ny, fx, fy)) * 0.01).astype(np.float32)
    kw = dict(converge=True, check_interval=5, eps=0.25)
    _, (want, done, at) = C.solver_want(case, edges, steps=100, S=S, **kw)
    assert 5 < at < 100 and at % 5 == 0, at
    with HeatSolver(C.solver_cfg(case, edges, "hip", steps=100, device=0, **kw)) as s:
        s.set_source(S, fx, fy, order)
        r = s.run()
        assert (r.converged, r.converged_at, r.steps_done) == (True, at, done)
        C.assert_bitwise(s.gather(), want, "converged state")
    # A NaN in the map raises "non-finite" at the first check.
    S[3, 2] = np.nan
    with HeatSolver(C.solver_cfg(case, edges, "hip", steps=100, device=0, **kw)) as s:
        s.set_source(S, fx, fy, order)
        with pytest.raises(_native.NativeError, match="non-finite"):
            s.run()


@pytest.mark.parametrize("plate", C.CONSERVATION_PLATES, ids=str)
def test_conservation_exact(gpu, plate):
    def one(cfg, fn):
        with HeatSolver(cfg.replace(backend="hip", device=0)) as s:
            return fn(s)
    C.check_conservation(one, plate)


def test_conservation_exact_on_loopback_ranks(gpu):
    def group(cfg, fn):
        return run_group(cfg.replace(backend="hip", px=2, py=2), 4, fn, transport="loopback")[0]
    C.check_conservation(group, (37, 53))


@pytest.mark.parametrize("world,kw", [(4, dict(px=2, py=2)), (3, dict(px=3, py=1))],
                         ids=["2x2", "3x1"])
@pytest.mark.parametrize("m", [0, 1, 4], ids=["m-auto", "m1", "m4"])
def test_loopback_ranks_and_the_ghost_rule(gpu, world, kw, m):
    # Blocks of 40 (or 27) rows: with 4 passes per exchange every pass after
    # an exchange updates ghost cells and reads ghost q there.  Each rank's
    # extended source block is checked against the plate indexed through the
    # map (neighbour, mirror, wrap and corner cells), then the run against
    # one rank's.
    case = (80, 80, 5, 3, 1)
    nx, ny, fx, fy, order = case
    S = C.source_map(*C.dims(nx, ny, fx, fy))
    for edges in C.EDGES:
        cfg = HeatConfig(nx=nx, ny=ny, steps=13, init="random", seed=3, backend="hip",
                         source=True, halo_passes=m, **edges, **kw)

        def fn(s):
            s.set_source(S, fx, fy, order)
            C.check_source_block(s, S, case, edges)
            s.run()
            return s.gather(), s.info.halo

        res = run_group(cfg, world, fn, transport="loopback")
        if m:
            assert res[0][1] == m, res[0][1]
        _, (want, _, _) = C.solver_want(case, edges, steps=13, S=S)
        C.assert_bitwise(res[0][0], want, (world, m, edges))


def test_lifecycle(gpu, tmp_path):
    case, edges = C.SOLVER_CASES[1], dict(periodic="y")
    nx, ny, fx, fy, order = case
    S, (want, _, _) = C.solver_want(case, edges)
    with HeatSolver(HeatConfig(nx=nx, ny=ny, backend="hip", device=0)) as s:
        with pytest.raises(_native.NativeError, match="source"):
            s.set_source(S, fx, fy, order)
    u0 = R.init_grid(nx, ny, "random", 3)
    with HeatSolver(C.solver_cfg(case, edges, "hip", device=0)) as s:
        assert s.info.tb_depth == 1
        s.run(7)                                 # graphs captured before the source is set
        plain, _, _ = R.run_np(nx, ny, 7, u0=u0, numerics="fma", **edges)
        assert np.array_equal(s.gather(), plain)
        s.set_source(S, fx, fy, order)           # ... and kept: they hold the pointer
        s.reset()
        s.run()
        C.assert_bitwise(s.gather(), want, "after reset")
        s.load_local(u0)
        s.run(C.STEPS)
        C.assert_bitwise(s.gather(), want, "after load_local")
        s.refine(u0, 1, 1, order=0)
        s.run(C.STEPS)
        C.assert_bitwise(s.gather(), want, "after refine")
        s.reset()
        s.run(11)
        s.coarse(4, 8)
        s.save(str(tmp_path / "ck.bin"))
        s.run(C.STEPS - 11)
        C.assert_bitwise(s.gather(), want, "coarse() in the middle")
        s.set_source(None)
        s.reset()
        s.run()
        zero, _, _ = R.run_np(nx, ny, C.STEPS, u0=u0, numerics="fma",
                              source=np.zeros((nx, ny), np.float32), **edges)
        C.assert_bitwise(s.gather(), zero, "cleared source")
    with HeatSolver(C.solver_cfg(case, edges, "hip", device=0)) as s:
        s.load(str(tmp_path / "ck.bin"))
        s.set_source(S, fx, fy, order)
        s.run()
        C.assert_bitwise(s.gather(), want, "resumed")
    with pytest.raises(ValueError, match="source"):
        HeatSolver(HeatConfig(nx=nx, ny=ny, backend="hip", device=0, source=True, kernel="tb"))
    assert _native.lib().heat_abi_version() == 9


def test_heat_cli_agrees_with_the_python_cli(gpu, tmp_path):
    run = dict(cwd=tmp_path, capture_output=True, text=True, timeout=300, check=True)
    heat = str(_native.CLI_PATH)
    S = C.source_map(18, 65)
    hio.write_bin(str(tmp_path / "q.bin"), S)
    common = ["--nx", "70", "--ny", "519", "--steps", "9", "--init", "random", "--seed", "3",
              "--source-from", "q.bin", "--out-format", "bin", "--json"]
    outs = []
    for cmd in ([heat, "--backend", "hip"],
                [heat, "--backend", "hip", "--gpus", "2", "--transport", "loopback"],
                [sys.executable, "-m", "parallel_heat_amd", "--backend", "cpu"]):
        p = subprocess.run(cmd + common + ["--out", f"final{len(outs)}.bin"],
                           env=dict(os.environ, PYTHONPATH=str(_native.REPO_DIR)), **run)
        m = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
        assert m["source"] == {"path": "q.bin", "rows": 18, "cols": 65, "fx": 4, "fy": 8,
                               "order": 1}
        outs.append((tmp_path / f"final{len(outs)}.bin").read_bytes())
    assert outs[0] == outs[2] and outs[1] == outs[2]
    want, _, _ = R.run_np(70, 519, 9, u0=R.init_grid(70, 519, "random", 3), numerics="fma",
                          source=R.refine_np(S, 70, 519, 4, 8, 1))
    last, h = hio.read_bin(str(tmp_path / "final0.bin"), mmap=False)
    assert h["step"] == 9
    C.assert_bitwise(last, want, "heat --source-from, 9 steps")
