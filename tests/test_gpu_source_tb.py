"""Fused source passes on the MI355X: the source_tb kernel through
ops.source_tb_step against k oracle steps over the shrinking boxes (every
depth, degenerate plates, strip widths, cut lanes, sub-boxes, unaligned
origins and pitches, every loop of the kernel more than once, the residual
word, the gate, launch independence), and Solver runs whose source passes go
in fused groups (every edge mode, graphs, remainder passes, gated and
host-judged convergence, loopback ranks with deep halos, conservation, the
lifecycle).  Equality is bitwise throughout.

Every test here fails on a library without the fused kernel: its entry points
are missing."""
import numpy as np
import pytest
import torch

from parallel_heat_amd import HeatConfig, HeatSolver, _native, ops
from parallel_heat_amd.models import reference as R
from parallel_heat_amd.parallel.group import run_group

from . import source_cases as S
from . import source_tb_cases as C

pytestmark = pytest.mark.gpu


# --------------------------------------------------------------------------- kernel


@pytest.mark.parametrize("coef", C.COEFS, ids=str)
@pytest.mark.parametrize("k", C.DEPTHS)
def test_every_depth_matches_the_oracle(gpu, k, coef):
    for kind in C.KINDS:
        C.check_tb(gpu, (37, 53), coef, kind, k)


@pytest.mark.parametrize("k", C.EDGE_DEPTHS)
def test_small_plates_and_plates_without_interior(gpu, k):
    # 1 .. 2k+1 rows (up to one row more than the ramp above and below a row
    # needs) x 1 .. 9 columns: every clipping of the grown boxes.
    n = 0
    for rows in range(1, 2 * k + 2):
        for cols in range(1, 10):
            C.check_tb(gpu, (rows, cols), C.COEFS[n % 2], C.KINDS[n % 3], k)
            n += 1
    for plate in ((2, 300), (300, 2), (1, 519), (40, 1)):
        C.check_tb(gpu, plate, C.COEFS[0], "signed", k)


@pytest.mark.parametrize("k", C.EDGE_DEPTHS)
def test_widths_around_the_strips(gpu, k):
    W = C.stride(k)
    for ny in (W - 1, W, W + 1, 2 * W + 1):
        C.check_tb(gpu, (11, ny), C.COEFS[0], "signed", k)
        C.check_tb(gpu, (11, ny), C.COEFS[1], "subnormal", k)
    for ny in (516, 517, 518, 519):   # plate column ny-1 in each lane element
        C.check_tb(gpu, (13, ny), C.COEFS[0], "wide", k)


@pytest.mark.parametrize("k", C.EDGE_DEPTHS)
def test_blocks_near_the_plate_edges(gpu, k):
    # Blocks d columns (rows) from a plate edge: the grown boxes are clipped
    # after d cells, on one side, in each lane element.
    coef = C.COEFS[0]
    for d in (1, 2, 3, 5):
        for kind in ("signed", "subnormal"):
            C.check_tb(gpu, (30, 90), coef, kind, k, block=(7, 90 - d - 40, 12, 40))
            C.check_tb(gpu, (30, 90), coef, kind, k, block=(7, d, 12, 40))
            C.check_tb(gpu, (60, 50), coef, kind, k, block=(d, 9, 20, 30))
            C.check_tb(gpu, (60, 50), coef, kind, k, block=(60 - d - 20, 9, 20, 30))
        C.check_tb(gpu, (30, 600), coef, "wide", k, block=(d, 600 - d - 520, 20, 520))


@pytest.mark.parametrize("k", C.EDGE_DEPTHS)
def test_interior_sub_boxes_grow_on_all_sides(gpu, k):
    # c0 in each residue mod 4, c1 cutting the last lane after 1 .. 4 cells;
    # the grown boxes stay inside the plate: src and q are read k (k-1) cells
    # beyond the box on every side, and no further (NaN there).
    for c0 in (12, 13, 14, 15):
        for c1 in (541, 542, 543, 544):
            C.check_tb(gpu, (40, 560), C.COEFS[(c0 + c1) % 2], "signed", k, box=(9, 29, c0, c1))
    # Sub-boxes 1, 2, 3 and 5 cells from the plate's edges: clipped on the way.
    for d in (1, 2, 3, 5):
        C.check_tb(gpu, (40, 300), C.COEFS[0], "subnormal", k, box=(d, 40 - d, d, 300 - d))
        C.check_tb(gpu, (40, 300), C.COEFS[1], "wide", k, box=(d, 20, 300 - d - 7, 300 - d))


@pytest.mark.parametrize("pitch,off", [(551, 9), (552, 8), (552, 9), (552, 10), (552, 11)],
                         ids=lambda v: str(v))
def test_unaligned_origin_and_pitch(gpu, pitch, off):
    # Pitch 551 (no multiple of 4): every lane moves dwords; pitch 552: float4
    # rows whose first lane starts `off` mod 4 columns before the block.
    for k in C.EDGE_DEPTHS:
        for ly in (516, 517, 518, 519):
            src, dst, q = C.fields(gpu, 21, ly, k, (pitch, off))
            plan = ops.source_tb_plan(src, dst, q, None, k)
            assert plan["vector_rows"] == int(pitch % 4 == 0), plan
            assert plan["align"] == (off % 4 if pitch % 4 == 0 else 0), plan
            C.check_tb(gpu, (21, ly), C.COEFS[0], "signed", k, raw=(pitch, off))
    # A block inside a plate: the frame of the buffer is read too.
    C.check_tb(gpu, (40, 560), C.COEFS[1], "signed", 8, block=(10, 11, 21, 517), raw=(pitch, off))


def test_arrays_out_of_phase_fall_back_to_dwords(gpu):
    # src and q one float apart modulo 16 bytes: no common float4 lanes.
    src, dst, q = C.fields(gpu, 9, 300, 3, (552, 8), q_off=9)
    assert ops.source_tb_plan(src, dst, q, None, 3)["vector_rows"] == 0
    for k in C.EDGE_DEPTHS:
        C.check_tb(gpu, (9, 300), C.COEFS[0], "signed", k, raw=(552, 8), q_off=9)


@pytest.mark.parametrize("k", C.EDGE_DEPTHS)
def test_every_loop_runs_twice(gpu, k):
    # A shape from the planner's own constants: two chunks of max_chunk_rows
    # rows + 1 and two strips + 37 columns, the launch capped at 2 waves: the
    # loop over a wave's units, the chunks and the strips all run at least twice.
    f = ops.Field(8, 8, halo=k, device=gpu)
    probe = ops.source_tb_plan(f, f, f, None, k)
    assert (probe["strip_cols"], probe["max_chunk_rows"], probe["min_chunk_rows"],
            probe["waves_per_cu"], probe["max_depth"]) == (256, 256, 32, 8, 8)
    assert probe["strip_stride"] == C.stride(k) and probe["overlap"] == C.overlap(k)
    kWaves = 2
    plate = (2 * probe["max_chunk_rows"] + 1, 2 * probe["strip_stride"] + 37)
    g = ops.Field(*plate, halo=k, device=gpu)
    ops.set_source_tb_max_waves(kWaves)
    try:
        plan = ops.source_tb_plan(g, g, g, None, k)
        capped = C.check_tb(gpu, plate, C.COEFS[0], "signed", k)
        C.check_tb(gpu, plate, C.COEFS[1], "subnormal", k)
    finally:
        ops.set_source_tb_max_waves(0)
    assert plan["waves"] == kWaves and plan["units"] >= 2 * kWaves, plan
    assert plan["strips"] == 3 and plan["chunks"] == 3 and plan["chunk_rows"] >= 2 * k, plan
    assert plan["strips"] % kWaves != 0, plan   # so a wave meets more than one strip
    # Launch independence: the default launch (no cap) and a third cap give
    # the same bits, in one round of waves and in three chunks per strip.
    free = C.check_tb(gpu, plate, C.COEFS[0], "signed", k)
    plan = ops.source_tb_plan(g, g, g, None, k)
    assert plan["waves"] == plan["units"] > kWaves and plan["chunks"] > 3, plan
    assert np.array_equal(C.bits(capped), C.bits(free))
    ops.set_source_tb_max_waves(5)
    try:
        five = C.check_tb(gpu, plate, C.COEFS[0], "signed", k)
    finally:
        ops.set_source_tb_max_waves(0)
    assert np.array_equal(C.bits(five), C.bits(free))


@pytest.mark.parametrize("k", C.EDGE_DEPTHS)
def test_residual_word(gpu, k):
    plate, coef = (40, 64), C.COEFS[0]
    box = (12, 25, 14, 40)
    # A word already set higher is kept.
    high = C.word_of(3e38)
    *_, word = C.run_tb(gpu, plate, coef, "signed", k, box=box, resid0=high)
    assert word == high
    # The word is the last level's alone: an earlier level moves more (the
    # field relaxes), and a pass over a larger plate sees many workgroups.
    C.check_tb(gpu, (300, 1100), coef, "wide", k)
    # A NaN in q at the far corner of its reach (k-1 cells out, diagonally, is
    # beyond it: the reach is a diamond; k-1 cells out along a row is inside)
    # surfaces in the box and in the word.
    q = C.values("signed", plate, 7)
    q[box[0], box[3] + k - 2] = np.nan
    got, (bi, bj), want, old, word = C.run_tb(gpu, plate, coef, "signed", k, box=box, q_plate=q,
                                              resid0=0)
    C.assert_bitwise(got[bi, bj], want, "NaN inside the reach")
    assert np.isnan(want).sum() >= 1 and np.isnan(np.uint32(word).view(np.float32))
    # One cell further out needs no NaN of its own: run_tb frames q with NaN
    # everywhere outside the box grown by k-1 (the cell next to the one above
    # included), so every run of this file shows that such a NaN is never read.
    got, (bi, bj), want, old, word = C.run_tb(gpu, plate, coef, "signed", k, box=box, resid0=0)
    C.assert_bitwise(got[bi, bj], want, "NaN just outside the region")
    assert not np.isnan(want).any() and word == C.expected_word(want, old)


@pytest.mark.parametrize("k", C.EDGE_DEPTHS)
def test_zero_source_and_closed_gate(gpu, k):
    plate, coef = (21, 300), C.COEFS[1]
    got, (bi, bj), _, _, _ = C.run_tb(gpu, plate, coef, "subnormal", k,
                                      q_plate=np.zeros(plate, np.float32), resid0=0)
    u = C.values("subnormal", plate, 0)
    for _ in range(k):   # k plain steps, each followed by the add of +0
        nxt = R.step_np_fma(u, *coef)
        nxt[1:-1, 1:-1] = nxt[1:-1, 1:-1] + np.float32(0)
        u = nxt
    C.assert_bitwise(got[bi, bj], u, "q = 0")
    # A closed gate writes nothing, not even the residual; an open one is no gate.
    for stop, wrote in ((1, False), (0, True)):
        gate = torch.tensor([stop, 0, 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=gpu)
        got, (bi, bj), want, _, word = C.run_tb(gpu, plate, coef, "signed", k, resid0=0,
                                                gate=gate)
        if wrote:
            C.assert_bitwise(got[bi, bj], want, "open gate")
            assert word != 0
        else:
            assert np.all(got == np.float32(C.SENTINEL)) and word == 0


def test_depths_out_of_range_are_refused(gpu):
    f = ops.Field(8, 8, halo=9, device=gpu)
    g = ops.Field(8, 8, halo=9, device=gpu)
    for k in (0, 1, 9):
        with pytest.raises(_native.NativeError, match="depth"):
            ops.source_tb_step(f, g, f, ops.Geom(8, 8), None, k)


# --------------------------------------------------------------------------- solver

TB_DEPTHS = [2, 3, 8, 12]


def fused_launches(steps, depth):
    """Fused launches of an ungated one-rank run: per pass of k steps (depth,
    then the remainder) one per group of up to 8 steps that has at least 2."""
    n, left = 0, steps
    while left > 0:
        k = min(depth, left)
        left -= k
        while k > 0:
            g = min(k, 8)
            n += g >= 2
            k -= g
    return n


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("depth", TB_DEPTHS)
def test_solver_matches_oracle_and_cpu(gpu, depth, graph):
    case = S.SOLVER_CASES[0]
    nx, ny, fx, fy, order = case
    M = S.source_map(*S.dims(nx, ny, fx, fy))
    for edges in S.EDGES:
        for steps in (13, 50):   # remainder passes of 1 (13 = 12 + 1, 4 x 3 + 1) and more
            _, (want, _, _) = S.solver_want(case, edges, steps=steps)
            before = ops.source_tb_launches()
            with HeatSolver(S.solver_cfg(case, edges, "hip", steps=steps, use_graph=graph,
                                         device=0, tb_depth=depth)) as s:
                assert s.info.tb_depth == depth
                s.set_source(M, fx, fy, order)
                r = s.run()
                assert r.steps_done == steps
                got = s.gather()
            S.assert_bitwise(got, want, (depth, graph, edges, steps))
            if not graph:
                assert ops.source_tb_launches() - before == fused_launches(steps, depth)
            with HeatSolver(S.solver_cfg(case, edges, "cpu", steps=steps, tb_depth=depth)) as s:
                s.set_source(M, fx, fy, order)
                s.run()
                S.assert_bitwise(got, s.gather(), (depth, edges, steps, "hip vs cpu"))


def test_wide_plate_and_the_unfused_knob(gpu, monkeypatch):
    # Three strips at depth 8; with HEAT_SRC_FUSED=0 the same run takes the
    # single-step kernel alone and gives the same bits.
    case, edges = S.SOLVER_CASES[2], dict(insulated="we", periodic="x")
    nx, ny, fx, fy, order = case
    M, (want, _, _) = S.solver_want(case, edges)
    out = []
    for fused in (True, False):
        if not fused:
            monkeypatch.setenv("HEAT_SRC_FUSED", "0")
        before = ops.source_tb_launches()
        with HeatSolver(S.solver_cfg(case, edges, "hip", use_graph=False, device=0,
                                     tb_depth=8)) as s:
            s.set_source(M, fx, fy, order)
            s.run()
            out.append(s.gather())
        # 30 steps: 8 + 8 + 8 + 6.
        assert ops.source_tb_launches() - before == (4 if fused else 0)
        S.assert_bitwise(out[-1], want, ("fused", fused))
    assert np.array_equal(C.bits(out[0]), C.bits(out[1]))


def test_default_depth_stays_one(gpu):
    case = S.SOLVER_CASES[0]
    before = ops.source_tb_launches()
    with HeatSolver(S.solver_cfg(case, dict(), "hip", device=0, use_graph=False)) as s:
        assert s.info.tb_depth == 1
        s.run()
    assert ops.source_tb_launches() == before


@pytest.mark.parametrize("host_checks", [False, True], ids=["gate", "host"])
def test_convergence_matches_prediction(gpu, monkeypatch, host_checks):
    if host_checks:
        monkeypatch.setenv("HEAT_HOST_CHECKS", "1")
    case, edges = S.SOLVER_CASES[0], dict(insulated="ns")
    nx, ny, fx, fy, order = case
    M = (S.source_map(*S.dims(nx, ny, fx, fy)) * 0.01).astype(np.float32)
    kw = dict(converge=True, check_interval=5, eps=0.25)
    _, (want, done, at) = S.solver_want(case, edges, steps=100, S=M, **kw)
    assert 5 < at < 100 and at % 5 == 0, at
    before = ops.source_tb_launches()
    with HeatSolver(S.solver_cfg(case, edges, "hip", steps=100, device=0, tb_depth=8, **kw)) as s:
        s.set_source(M, fx, fy, order)
        r = s.run()
        assert (r.converged, r.converged_at, r.steps_done) == (True, at, done)
        S.assert_bitwise(s.gather(), want, "converged state")
    assert ops.source_tb_launches() > before   # passes of 5 steps: one fused launch each
    # A NaN in the map raises "non-finite" at the first check.
    M[3, 2] = np.nan
    with HeatSolver(S.solver_cfg(case, edges, "hip", steps=100, device=0, tb_depth=8, **kw)) as s:
        s.set_source(M, fx, fy, order)
        with pytest.raises(_native.NativeError, match="non-finite"):
            s.run()


@pytest.mark.parametrize("world,kw", [(4, dict(px=2, py=2)), (3, dict(px=3, py=1))],
                         ids=["2x2", "3x1"])
@pytest.mark.parametrize("m", [1, 4], ids=["m1", "m4"])
def test_loopback_ranks_with_deep_halos(gpu, world, kw, m):
    # Passes of 4 fused steps over boxes that reach into the ghost ring (with 4
    # passes per exchange by up to 12 cells), 13 steps: 4 + 4 + 4 + 1.
    case = (80, 80, 5, 3, 1)
    nx, ny, fx, fy, order = case
    M = S.source_map(*S.dims(nx, ny, fx, fy))
    for edges in S.EDGES:
        cfg = HeatConfig(nx=nx, ny=ny, steps=13, init="random", seed=3, backend="hip",
                         source=True, halo_passes=m, tb_depth=4, **edges, **kw)

        def fn(s):
            s.set_source(M, fx, fy, order)
            s.run()
            return s.gather(), s.info.halo, s.info.tb_depth

        before = ops.source_tb_launches()
        res = run_group(cfg, world, fn, transport="loopback")
        assert ops.source_tb_launches() > before
        assert res[0][1:] == (4 * m, 4), res[0][1:]
        with HeatSolver(cfg.replace(px=1, py=1, halo_passes=1, device=0)) as s:
            s.set_source(M, fx, fy, order)
            s.run()
            S.assert_bitwise(res[0][0], s.gather(), (world, m, edges, "vs one rank"))
        _, (want, _, _) = S.solver_want(case, edges, steps=13, S=M)
        S.assert_bitwise(res[0][0], want, (world, m, edges))


@pytest.mark.parametrize("plate", S.CONSERVATION_PLATES, ids=str)
def test_conservation_exact(gpu, plate):
    depth = []

    def one(cfg, fn):
        with HeatSolver(cfg.replace(backend="hip", device=0, tb_depth=8)) as s:
            depth.append(s.info.tb_depth)
            return fn(s)
    before = ops.source_tb_launches()
    S.check_conservation(one, plate)
    # A pass is no deeper than the plate's thinnest wrapped extent: the 1 x 9
    # torus runs single steps, the others their 6 steps in one fused pass.
    assert depth == [min(8, *plate)], depth
    assert (ops.source_tb_launches() > before) == (depth[0] >= 2)


def test_lifecycle(gpu, tmp_path):
    case, edges = S.SOLVER_CASES[1], dict(periodic="y")
    nx, ny, fx, fy, order = case
    M, (want, _, _) = S.solver_want(case, edges)
    u0 = R.init_grid(nx, ny, "random", 3)
    with HeatSolver(S.solver_cfg(case, edges, "hip", device=0, tb_depth=8)) as s:
        assert s.info.tb_depth == 8
        s.run(7)                                 # graphs captured before the source is set
        plain, _, _ = R.run_np(nx, ny, 7, u0=u0, numerics="fma", **edges)
        zero7, _, _ = R.run_np(nx, ny, 7, u0=u0, numerics="fma",
                               source=np.zeros((nx, ny), np.float32), **edges)
        S.assert_bitwise(s.gather(), zero7, "before the source is set")
        assert np.array_equal(s.gather(), plain)
        s.set_source(M, fx, fy, order)           # ... and kept: they hold the pointer
        s.reset()
        s.run()
        S.assert_bitwise(s.gather(), want, "after reset")
        s.load_local(u0)
        s.run(S.STEPS)
        S.assert_bitwise(s.gather(), want, "after load_local")
        s.reset()
        s.run(11)                                # 8 + 3: an odd number of flips
        s.coarse(4, 8)
        s.save(str(tmp_path / "ck.bin"))
        s.run(S.STEPS - 11)
        S.assert_bitwise(s.gather(), want, "coarse() in the middle")
        s.set_source(None)
        s.reset()
        s.run()
        zero, _, _ = R.run_np(nx, ny, S.STEPS, u0=u0, numerics="fma",
                              source=np.zeros((nx, ny), np.float32), **edges)
        S.assert_bitwise(s.gather(), zero, "cleared source")
    with HeatSolver(S.solver_cfg(case, edges, "hip", device=0, tb_depth=8)) as s:
        s.load(str(tmp_path / "ck.bin"))
        s.set_source(M, fx, fy, order)
        s.run()
        S.assert_bitwise(s.gather(), want, "resumed")
    assert _native.lib().heat_abi_version() == 9
