"""Replace or inspect the state of a GPU solver that has already run, continue,
and compare with the NumPy oracle (lifecycle_cases.py has the scenario and the
reasons): one rank and loopback ranks, every kernel family, edge frames, deep
halos, the three pass schedules, resident spans, segment graphs, an enqueued
run still in flight, the device-judged convergence gate, and the CLI's
checkpoint / resume across decompositions.  Needs an MI355X.

Every configuration runs every replacement operation.  Its other options
(depth, graphs, resident spans, passes per exchange, rank grid, ...) are not
crossed in full with the operations: they rotate over them, so that every
option value meets every operation somewhere and every combination of option
values occurs, and the file stays a few seconds long."""
import json
import subprocess

import pytest

from parallel_heat_amd import HeatConfig, HeatSolver, _native
from parallel_heat_amd.parallel.group import run_group

from . import lifecycle_cases as L
from .oracle_cases import assert_bitwise

pytestmark = pytest.mark.gpu

K = 8
# After a replacement: uneven calls across a full exchange interval (24 steps
# at most here) and a remainder pass; shorter after the second one.
POST, POST2 = (5, 1, 17, 2), (5, 1, 6)
# Where resident spans are wanted, the two full passes come first: behind the
# 5- and 1-step passes the column ghosts, valid in whole float4 columns only,
# last for one more full pass, and a span needs two.
POST_R, POST2_R = (17, 5, 1, 2), (17, 2)
ALL_OPS = L.OPS
BIG, SMALL, MID, TINY = (203, 517), (40, 70), (150, 300), (48, 52)


def config(plate, **kw):
    return HeatConfig(nx=plate.nx, ny=plate.ny, steps=0, cx=plate.cx, cy=plate.cy, init="random",
                      seed=plate.seed, backend="hip", insulated=plate.insulated,
                      periodic=plate.periodic,
                      numerics="mpi" if plate.numerics == "mpi" else "fp32", **kw)


def in_world(cfg, world, fn):
    """fn(solver) on one rank, or on `world` loopback ranks: the per-rank results."""
    if world == 1:
        with HeatSolver(cfg) as s:
            return [fn(s)]
    return run_group(cfg, world, fn, transport="loopback")


@pytest.fixture(scope="module")
def checkpoints(tmp_path_factory):
    """path(plate, kind, step, world): a checkpoint of that oracle state written
    once by ANOTHER solver of another decomposition than the `world` ranks
    that will load it: a 2 x 2 loopback group for one rank, one rank for a group."""
    root = tmp_path_factory.mktemp("lifecycle_ckpt")
    made = {}

    def path(plate, kind, step, world):
        writers = 4 if world == 1 else 1
        key = (plate.nx, plate.ny, plate.seed, kind, step, writers)
        if key not in made:
            p = str(root / f"ck{len(made)}.bin")
            grid = L.state(plate, kind, 0)
            cfg = config(L.Plate(plate.nx, plate.ny, cx=plate.cx, cy=plate.cy), tb_depth=K,
                         halo_passes=1, **(dict(px=2, py=2) if writers == 4 else {}))

            def write(w):
                w.run(3)   # a writer that has run, too
                L.write_checkpoint(w, grid, step, p)
            in_world(cfg, writers, write)
            made[key] = p
        return made[key]
    return path


def run_case(plate, case, checkpoints, tmp_path, world=1, px=1, py=1, H=0, **kw):
    paths = {"save": str(tmp_path / "saved.bin")}
    if case.op == "load":
        paths["load1"] = checkpoints(plate, L.target(case.op), case.s0, world)
    if case.op2 == "load":
        paths["load2"] = checkpoints(plate, L.target(case.op2, True), case.s02, world)
    plan = L.make_plan(plate, case, px, py, H, paths)
    if world > 1:
        kw.update(px=px, py=py)
    return in_world(config(plate, **kw), world, lambda s: L.play(s, plan))


def second_op(op, k):
    """Another operation for the second replacement, to a third state whose
    oracle trajectory the first replacements of the module need anyway: reset
    or a refinement (never one refinement after the other: their clamped edge
    cells agree).  load, scatter and load_local come second on the small plates."""
    if op == "reset":
        return ("refine0", "refine1")[k % 2]
    if op.startswith("refine"):
        return "reset"
    return ("reset", "refine0", "refine1")[k % 3]


def ghost_mid(odd):
    """Run calls which, behind two full passes, leave the ghosts partly valid
    (depth 8, 1 or 3 passes per exchange), in an odd or an even buffer parity."""
    return (1,) if odd else (1, 1)


def resident_passes(outs, phase="post"):
    return [sum(r.resident_passes for r in o[phase]) for o in outs]


# -- 1: one rank, the TB kernels, graphs, resident spans --------------------------------------

def one_rank_tb_cases():
    """Every operation twice: under the options spelled by the bits of its
    index (depth 8 / 12, graphs, resident spans) and under their complement,
    all eight combinations among them."""
    out = []
    for o, op in enumerate(ALL_OPS):
        for flip in (0, 7):
            b = o ^ flip
            depth, use_graph, resident = (8, 12)[b & 1], bool(b >> 1 & 1), b >> 2 & 1
            out.append(pytest.param(depth, use_graph, resident, op, flip == 0 and o in (1, 4),
                                    id=f"d{depth}-graph{int(use_graph)}-res{resident}-{op}"))
    return out


BIG_POST, BIG_POST2 = POST, POST2


@pytest.mark.parametrize("depth,use_graph,resident,op,twice", one_rank_tb_cases())
def test_one_rank_tb(gpu, monkeypatch, checkpoints, tmp_path, depth, use_graph, resident, op,
                     twice):
    monkeypatch.setenv("HEAT_TB_RESIDENT", str(resident))
    i = ALL_OPS.index(op) + resident
    # Three calls of one pass: the third finds the parity of the first and
    # replays its graph; then an odd (3 passes) or an even parity.
    case = L.Case(pre=(depth,) * 3, mid=(1,) if i % 2 else (), reads=L.rotate(L.READS, i),
                  op=op, post=BIG_POST)
    if twice:
        case = case._replace(op2=second_op(op, i), post2=BIG_POST2)
    out, = run_case(L.Plate(*BIG), case, checkpoints, tmp_path, tb_depth=depth,
                    use_graph=use_graph)
    assert [r.passes for r in out["pre"] + out["mid"]] == [1] * (3 + len(case.mid))
    assert all(r.exchanges == 0 for ph in out.values() for r in ph)
    # the 17-step call holds two equal passes: a resident span (as
    # test_resident_plate_bitwise finds on this plate)
    assert (sum(r.resident_passes for r in out["post"]) > 0) == bool(resident), out["post"]


# -- 2: a plate smaller than a tile; the other kernels and numerics ---------------------------

@pytest.mark.parametrize("op", ["load", "scatter"])
@pytest.mark.parametrize("kw,numerics", [(dict(kernel="naive", tb_depth=3), "fma"),
                                         (dict(kernel="lds", tb_depth=4), "fma"),
                                         (dict(tb_depth=4), "mpi")],
                         ids=["naive3", "lds4", "mpi"])
def test_small_plate_kernels(gpu, checkpoints, tmp_path, kw, numerics, op):
    depth = kw["tb_depth"]
    mid = (depth, 1) if op == "load" else (depth,)   # either parity of the step count
    case = L.Case(pre=(2 * depth, 2 * depth), mid=mid, reads=L.rotate(L.READS, depth + len(mid)),
                  op=op, post=POST, op2="load" if op == "scatter" else "load_local", post2=POST2)
    run_case(L.Plate(*SMALL, numerics=numerics), case, checkpoints, tmp_path, **kw)


# -- 3: one rank whose edges have a ghost frame ------------------------------------------------

EDGES = [dict(insulated="ns"), dict(insulated="all"), dict(periodic="xy"),
         dict(periodic="x", insulated="e")]
EDGE_IDS = ["ins-ns", "ins-all", "per-xy", "per-x-ins-e"]


FRAME_OPTIONS = [(1, 0), (3, 0), (3, 1), (1, 1)]   # passes per exchange, resident spans


def edge_frame_cases():
    out = []
    for e, eid in enumerate(EDGE_IDS):
        for o, op in enumerate(ALL_OPS):
            m, resident = FRAME_OPTIONS[(o + e) % 4]
            out.append(pytest.param(EDGES[e], m, resident, op, id=f"{eid}-m{m}-res{resident}-{op}"))
    return out


@pytest.mark.parametrize("edges,m,resident,op", edge_frame_cases())
def test_one_rank_edge_frames(gpu, monkeypatch, checkpoints, tmp_path, edges, m, resident, op):
    monkeypatch.setenv("HEAT_TB_RESIDENT", str(resident))
    e, o = EDGES.index(edges), ALL_OPS.index(op)
    i = e * 6 + o
    case = L.Case(pre=(K, K), mid=ghost_mid((o + e // 2) % 2 == 0), reads=L.rotate(L.READS, i),
                  op=op, post=POST_R if resident else POST)
    if o == e + 1:
        case = case._replace(op2=second_op(op, i), post2=POST2_R if resident else POST2)
    plate = L.Plate(*MID, **edges)
    out, = run_case(plate, case, checkpoints, tmp_path, H=m * K, tb_depth=K, halo_passes=m)
    if not resident:
        gr, gc = L.assert_sync_counts(out, case, plate, 1, 1, K, m, tb=True)
        assert 0 < max(gr, gc) < m * K, (gr, gc)
    elif m == 3:
        # spans of the passes between two refills of the frame
        assert sum(r.resident_passes for r in out["post"]) > 0, out["post"]


# -- 4, 5: loopback ranks, deep halos, schedules, edges -----------------------------------------

GRIDS = {"2x2": (4, 2, 2), "3rows": (3, 3, 1), "2rows": (2, 2, 1)}


def loopback_sync_cases():
    return [pytest.param(grid, (1, 3)[(o + g) % 2], op, id=f"{grid}-m{(1, 3)[(o + g) % 2]}-{op}")
            for g, grid in enumerate(["2x2", "3rows"]) for o, op in enumerate(ALL_OPS)]


@pytest.mark.parametrize("grid,m,op", loopback_sync_cases())
def test_loopback_sync(gpu, monkeypatch, checkpoints, tmp_path, grid, m, op):
    monkeypatch.setenv("HEAT_TB_RESIDENT", "1")   # ranks sharing a device: never resident
    world, px, py = GRIDS[grid]
    o = ALL_OPS.index(op)
    i = o + world
    case = L.Case(pre=(K, K), mid=ghost_mid((o // 2 + world) % 2 == 0), reads=L.rotate(L.READS, i),
                  op=op, post=POST)
    if o == world:
        case = case._replace(op2=second_op(op, i), post2=POST2)
    plate = L.Plate(*MID)
    outs = run_case(plate, case, checkpoints, tmp_path, world, px, py, H=m * K, tb_depth=K,
                    halo_passes=m, schedule="sync")
    for out in outs:
        gr, gc = L.assert_sync_counts(out, case, plate, px, py, K, m, tb=True)
        assert 0 < max(gr, gc) < m * K, (gr, gc)
    assert resident_passes(outs) == [0] * world


@pytest.mark.parametrize("grid,schedule,op", [
    ("2x2", "overlap", "load"), ("3rows", "overlap", "scatter"),
    ("3rows", "pipeline", "load"), ("2x2", "pipeline", "scatter")])
def test_loopback_overlap_schedules(gpu, checkpoints, tmp_path, grid, schedule, op):
    world, px, py = GRIDS[grid]
    i = world + (op == "load") + (schedule == "pipeline")
    case = L.Case(pre=(K, K), mid=ghost_mid(i % 2 == 0), reads=L.rotate(L.READS, i), op=op,
                  post=POST, op2=second_op(op, i), post2=POST2)
    outs = run_case(L.Plate(*MID), case, checkpoints, tmp_path, world, px, py, H=K, tb_depth=K,
                    schedule=schedule)
    assert all(o["post"][0].exchanges >= 1 for o in outs)


def loopback_edge_cases():
    out = []
    for g, (grid, edges, eid) in enumerate([("2rows", EDGES[3], EDGE_IDS[3]),
                                            ("2x2", EDGES[1], EDGE_IDS[1])]):
        for o, op in enumerate(ALL_OPS):
            m = (3, 1)[(o + g) % 2]
            out.append(pytest.param(grid, edges, m, op, id=f"{grid}-{eid}-m{m}-{op}"))
    return out


@pytest.mark.parametrize("grid,edges,m,op", loopback_edge_cases())
def test_loopback_with_edges(gpu, checkpoints, tmp_path, grid, edges, m, op):
    # periodic x on two ranks along x: both sides of a rank face the same peer
    # (the plates are those of the one-rank cases: one oracle for both)
    world, px, py = GRIDS[grid]
    o = ALL_OPS.index(op)
    i = o + world
    case = L.Case(pre=(K, K), mid=ghost_mid((o // 2 + world) % 2 == 1), reads=L.rotate(L.READS, i),
                  op=op, post=POST)
    if o == world + 1:
        case = case._replace(op2=second_op(op, i), post2=POST2)
    plate = L.Plate(*MID, **edges)
    outs = run_case(plate, case, checkpoints, tmp_path, world, px, py, H=m * K, tb_depth=K,
                    halo_passes=m, schedule="sync")
    for out in outs:
        gr, gc = L.assert_sync_counts(out, case, plate, px, py, K, m, tb=True)
        assert 0 < max(gr, gc) < m * K, (gr, gc)


# -- 6: resident spans on loopback ranks -------------------------------------------------------

@pytest.mark.parametrize("op", ["load", "scatter"])
@pytest.mark.parametrize("grid", ["2rows", "2x2"])
def test_loopback_resident_spans(gpu, monkeypatch, checkpoints, tmp_path, grid, op):
    # HEAT_TB_RESIDENT=2 lets ranks that share the device go resident.  48 x 52
    # is as small as a plate gets here: its 2 x 2 blocks (24 x 26) just hold
    # the 24-deep halo, and every rank still reports resident passes on it,
    # before and after each replacement.
    monkeypatch.setenv("HEAT_TB_RESIDENT", "2")
    world, px, py = GRIDS[grid]
    case = L.Case(pre=(2 * K, 2 * K), mid=ghost_mid(op == "load"),
                  reads=L.rotate(L.READS, world + (op == "load")), op=op, post=POST_R,
                  op2="load" if op == "scatter" else "scatter", post2=POST2_R)
    assert sum(case.pre + case.mid + case.post + case.post2) <= 120
    outs = run_case(L.Plate(*TINY), case, checkpoints, tmp_path, world, px, py, H=3 * K,
                    tb_depth=K, halo_passes=3, schedule="sync")
    for phase in ("pre", "post", "post2"):
        assert all(n > 0 for n in resident_passes(outs, phase)), (phase, outs)


# -- 7: an enqueued run still in flight ---------------------------------------------------------

@pytest.mark.parametrize("op", ALL_OPS)
def test_replace_with_a_run_in_flight(gpu, checkpoints, tmp_path, op):
    # run(wait=False) three times, then the replacement with no run(0) in
    # between: it completes the enqueued steps itself (complete_pending).
    o = ALL_OPS.index(op)
    n = (K, 12)[o % 2]
    case = L.Case(pre=(n, n, n), mid=(), reads=(), op=op, post=BIG_POST, enqueue=True)
    if o in (0, 3):
        case = case._replace(op2=second_op(op, o), post2=BIG_POST2)
    out, = run_case(L.Plate(*BIG), case, checkpoints, tmp_path, tb_depth=K)
    assert all(r.seconds == 0 for r in out["pre"])   # enqueued, not waited for


# -- convergence across a replacement ------------------------------------------------------------

DEPTH = 12   # checks inside a pass take the residual at their level; a converging one replays


def conv_config(interval, compat, **kw):
    kw.setdefault("tb_depth", DEPTH)
    return HeatConfig(nx=L.CONV["nx"], ny=L.CONV["ny"], steps=0, cx=L.CONV["cx"], cy=L.CONV["cy"],
                      converge=True, check_interval=interval, eps=L.CONV["eps"], init="random",
                      seed=L.CONV["seed"], compat=compat, backend="hip", **kw)


def converge_replace_converge(cfg, world, op, s0, first, again, ck):
    """a. on every rank: run to convergence (the gate is closed, a check
    inside a pass was replayed), put the step-0 state back at step s0, run
    again; RunResult and state against the oracle."""
    start = L.conv_start()

    def fn(s):
        depth = s.info.tb_depth
        r1 = s.run(L.CONV_RUN)
        L.assert_run_result(r1, first, ("first", s.rank))
        assert s.step == first.converged_at and first.converged_at % depth != 0
        g = s.gather()
        if g is not None:
            assert_bitwise(g, first.grid, "first")
        if op == "load":
            s.load(ck)
        else:
            s.scatter(start if s.rank == 0 else None, step=s0)
        assert s.step == s0
        g = s.gather()
        if g is not None:
            assert_bitwise(g, start, "replaced")
        r2 = s.run(L.CONV_RUN)
        L.assert_run_result(r2, again, ("again", s.rank))
        assert s.step == again.converged_at and (again.converged_at - s0) % depth != 0
        g = s.gather()
        if g is not None:
            assert_bitwise(g, again.grid, "again")
        assert s.checksum()["hash"] == L.hash_of(again.grid)
        return r1, r2
    return in_world(cfg, world, fn)


def conv_oracles(interval, s0, compat, periodic=""):
    first = L.conv_oracle(0, interval, compat, periodic)
    again = L.conv_oracle(s0, interval, compat, periodic)
    L.assert_converges_inside(first, 0, interval, compat)
    L.assert_converges_inside(again, s0, interval, compat)
    assert again.converged_at - s0 != first.converged_at
    return first, again


@pytest.fixture(scope="module")
def conv_checkpoint(tmp_path_factory):
    """path(step): the convergence plate's step-0 state as a checkpoint at `step`."""
    root = tmp_path_factory.mktemp("lifecycle_conv")
    made = {}

    def path(step):
        if step not in made:
            made[step] = str(root / f"start{step}.bin")
            with HeatSolver(conv_config(20, "none", tb_depth=K)) as w:
                L.write_checkpoint(w, L.conv_start(), step, made[step])
        return made[step]
    return path


def converge_cases():
    """Every (interval, compat) under four of the eight combinations of host
    checks, graphs and resident spans, all eight for each interval."""
    out = []
    for idx, (interval, compat) in enumerate((i, c) for i in (20, 7)
                                             for c in ("none", "cuda", "mpi")):
        for k in range(4):
            b = (idx + 2 * k) % 8
            host, use_graph, resident = ("1" if b & 1 else None), not b >> 1 & 1, b >> 2 & 1
            out.append(pytest.param(host, use_graph, resident, interval, compat,
                                    id=f"host{b & 1}-graph{int(use_graph)}-res{resident}-"
                                       f"c{interval}-{compat}"))
    return out


@pytest.mark.parametrize("host_checks,use_graph,resident,interval,compat", converge_cases())
def test_converge_then_replace(gpu, monkeypatch, conv_checkpoint, host_checks, use_graph,
                               resident, interval, compat):
    monkeypatch.setenv("HEAT_TB_RESIDENT", str(resident))
    if host_checks is None:
        monkeypatch.delenv("HEAT_HOST_CHECKS", raising=False)
    else:
        monkeypatch.setenv("HEAT_HOST_CHECKS", host_checks)
    first, again = conv_oracles(interval, L.S0, compat)
    op = "load" if (use_graph + resident + interval + len(compat)) % 2 else "scatter"
    converge_replace_converge(conv_config(interval, compat, use_graph=use_graph), 1, op, L.S0,
                              first, again, conv_checkpoint(L.S0))


def test_converge_then_replace_long_interval(gpu, conv_checkpoint):
    first, again = conv_oracles(50, L.S0_ALT, "none")
    converge_replace_converge(conv_config(50, "none"), 1, "load", L.S0_ALT, first, again,
                              conv_checkpoint(L.S0_ALT))


@pytest.mark.parametrize("compat,use_graph", [("none", True), ("cuda", False), ("mpi", True),
                                              ("none", False)])
def test_converge_then_reset(gpu, compat, use_graph):
    # b. the second life converges where the first did, to the same state.
    first = L.conv_oracle(0, 20, compat)
    with HeatSolver(conv_config(20, compat, use_graph=use_graph)) as s:
        for life in range(2):
            r = s.run(L.CONV_RUN)
            L.assert_run_result(r, first, life)
            assert s.step == first.converged_at
            assert_bitwise(s.gather(), first.grid, life)
            s.reset()
            assert s.step == 0
            assert_bitwise(s.gather(), L.conv_start(), "reset")


@pytest.mark.parametrize("host_checks", [None, "1"])
@pytest.mark.parametrize("compat", ["none", "cuda", "mpi"])
def test_uniform_plate_converges_at_the_next_check(gpu, monkeypatch, compat, host_checks):
    # c. 60 steps without converging, then a uniform plate at step s0: the
    # next check (of the new count) sees a residual of exactly 0.
    if host_checks is None:
        monkeypatch.delenv("HEAT_HOST_CHECKS", raising=False)
    else:
        monkeypatch.setenv("HEAT_HOST_CHECKS", host_checks)
    before = L.conv_oracle(0, 20, compat, n=60)
    assert before.converged_at == -1 and before.checks >= 2
    after = L.conv_oracle(L.S0, 20, compat, kind="U")
    nxt = L.check_steps_between(L.S0, L.S0 + L.CONV_RUN, 20, compat)[0]
    assert after.converged_at == nxt and after.last_resid == 0.0
    ones = L.conv_start("U")
    with HeatSolver(conv_config(20, compat)) as s:
        L.assert_run_result(s.run(60), before, "before")
        assert_bitwise(s.gather(), before.grid, "before")
        s.scatter(ones, step=L.S0)
        r = s.run(L.CONV_RUN)
        L.assert_run_result(r, after, "uniform")
        assert r.last_resid == 0.0 and r.converged_at == nxt and s.step == nxt
        assert_bitwise(s.gather(), ones, "uniform")


@pytest.mark.parametrize("op", ["load", "scatter"])
def test_converge_then_replace_loopback(gpu, conv_checkpoint, op):
    # d. 2 x 2 ranks: every rank's RunResult.
    assert L.CONV["nx"] <= 64 and L.CONV["ny"] <= 96
    first, again = conv_oracles(20, L.S0, "none")
    assert first.converged_at < 400 and again.steps_done < 400
    res = converge_replace_converge(conv_config(20, "none", px=2, py=2, halo_passes=1), 4, op,
                                    L.S0, first, again, conv_checkpoint(L.S0))
    assert len(res) == 4


@pytest.mark.parametrize("op", ["load", "scatter"])
def test_converge_then_replace_periodic(gpu, conv_checkpoint, op):
    # e. periodic in both axes: the residual covers the edge cells.
    first, again = conv_oracles(7, L.S0, "none", "xy")
    plain = L.conv_oracle(0, 7, "none")
    assert first.converged_at != plain.converged_at
    converge_replace_converge(conv_config(7, "none", periodic="xy", halo_passes=1), 1, op, L.S0,
                              first, again, conv_checkpoint(L.S0))


# -- the CLI: checkpoint on one decomposition, resume on another ---------------------------------

def heat(args, cwd):
    return subprocess.run([str(_native.CLI_PATH), "--backend", "hip"] + args, cwd=cwd,
                          capture_output=True, text=True, timeout=300, check=True)


def test_cli_checkpoint_resume_across_decompositions(gpu, tmp_path):
    # Four loopback ranks write a checkpoint, one rank resumes it and writes
    # the next, four ranks resume that: both directions, a fresh process each.
    from parallel_heat_amd.utils import io as hio
    plate = L.Plate(*SMALL)
    base = ["--nx", str(plate.nx), "--ny", str(plate.ny), "--init", "random", "--seed",
            str(plate.seed), "--cx", str(plate.cx), "--cy", str(plate.cy), "--tb-depth", str(K),
            "--checkpoint-every", "25", "--json"]

    def ranks(n):
        return ["--gpus", str(n), "--transport", "loopback"] if n > 1 else []
    at = 0
    for n, (world, steps) in enumerate([(4, 40), (1, 97), (4, 150)]):
        resume = ["--resume", f"ck{n - 1}.bin"] if n else []
        p = heat(base + ranks(world) + resume + ["--steps", str(steps), "--checkpoint",
                                                 f"ck{n}.bin", "--out", f"c{n}.json",
                                                 "--out-format", "checksum"], tmp_path)
        m = json.loads(p.stdout.splitlines()[-1])
        assert m["steps_done"] == steps - at and m["ranks"] == world, m
        at = steps
        want = L.state(plate, "A", steps)
        g, h = hio.read_bin(str(tmp_path / f"ck{n}.bin"), mmap=False)
        assert h["step"] == steps
        assert_bitwise(g, want, ("checkpoint", n))
        cs = json.loads((tmp_path / f"c{n}.json").read_text())
        assert cs["step"] == steps and cs["count"] == plate.nx * plate.ny
        assert cs["hash"] == L.hash_of(want), n
