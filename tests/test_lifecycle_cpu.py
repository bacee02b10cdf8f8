"""Replace or inspect the state of a CPU solver that has already run, continue,
and compare with the NumPy oracle (lifecycle_cases.py has the scenario and the
reasons).  One rank with insulated or periodic edges has a ghost frame that the
next run must refill, so this file guards, without a GPU, the lines of
solver.cpp that drop the ghosts' validity and set the step in load_owned,
refine and init_fields.  One case runs on two gloo ranks (dist_worker.py's
lifecycle mode), whose ghosts are each other's rows."""
import numpy as np
import pytest

from parallel_heat_amd import HeatConfig, HeatSolver
from parallel_heat_amd.models import reference as R

from . import lifecycle_cases as L
from .oracle_cases import assert_bitwise

K = 8                                  # pass depth of the ghosted cases
# After a replacement: uneven calls across a full exchange interval (24 steps
# at most here) and a remainder pass; shorter after the second one.
POST, POST2 = (5, 1, 17, 2), (5, 1, 6)
EDGES = [dict(insulated="ns"), dict(insulated="all"), dict(periodic="xy"),
         dict(periodic="x", insulated="e")]
EDGE_IDS = ["ins-ns", "ins-all", "per-xy", "per-x-ins-e"]


def config(plate, **kw):
    return HeatConfig(nx=plate.nx, ny=plate.ny, steps=0, cx=plate.cx, cy=plate.cy, init="random",
                      seed=plate.seed, backend="cpu", insulated=plate.insulated,
                      periodic=plate.periodic,
                      numerics="mpi" if plate.numerics == "mpi" else "fp32", **kw)


@pytest.fixture(scope="module")
def checkpoints(tmp_path_factory):
    """path(plate, kind, step): a checkpoint of that oracle state, written once
    by ANOTHER solver (another pass depth, no deep halo) through scatter + save."""
    root = tmp_path_factory.mktemp("lifecycle_ckpt")
    made = {}

    def path(plate, kind, step):
        key = (plate, kind, step)
        if key not in made:
            p = str(root / f"ck{len(made)}.bin")
            with HeatSolver(config(plate, tb_depth=1)) as w:
                w.run(3)   # a writer that has run, too
                L.write_checkpoint(w, L.state(plate, kind, 0), step, p)
            made[key] = p
        return made[key]
    return path


def run_case(plate, case, m, depth, checkpoints, tmp_path):
    H = m * depth
    paths = {"save": str(tmp_path / "saved.bin")}
    if case.op == "load":
        paths["load1"] = checkpoints(plate, L.target(case.op), case.s0)
    if case.op2 == "load":
        paths["load2"] = checkpoints(plate, L.target(case.op2, True), case.s02)
    plan = L.make_plan(plate, case, 1, 1, H, paths)
    with HeatSolver(config(plate, tb_depth=depth, halo_passes=m)) as s:
        assert s.info.tb_depth == depth
        out = L.play(s, plan)
    return out


# -- configuration 3: one rank whose edges have a ghost frame --------------------------------

def edge_cases():
    out = []
    for e, (edges, eid) in enumerate(zip(EDGES, EDGE_IDS)):
        for m in (1, 3):
            for o, op in enumerate(L.OPS):
                i = (e * 2 + (m == 3)) * len(L.OPS) + o
                odd = (o + e) % 2 == 0
                mid = (1,) if odd else (1, 1)
                # one case per configuration replaces twice, by another operation
                op2 = L.OPS[(o + 1 + e) % len(L.OPS)] if o == (e + m) % len(L.OPS) else None
                # (not one refinement after the other: their clamped edge cells agree)
                if op2 is not None and op2[:-1] == op[:-1] == "refine":
                    op2 = "scatter"
                case = L.Case(pre=(K, K), mid=mid, reads=L.rotate(L.READS, i), op=op, post=POST,
                              op2=op2, post2=POST2 if op2 else ())
                out.append(pytest.param(edges, m, case, id=f"{eid}-m{m}-{op}" +
                                        (f"-then-{op2}" if op2 else "")))
    return out


@pytest.mark.parametrize("edges,m,case", edge_cases())
def test_replace_with_edge_ghosts(edges, m, case, checkpoints, tmp_path):
    plate = L.Plate(150, 300, **edges)
    out = run_case(plate, case, m, K, checkpoints, tmp_path)
    gr, gc = L.assert_sync_counts(out, case, plate, 1, 1, K, m, tb=False)
    # The replacement met ghosts that were partly valid, in either parity.
    assert 0 < max(gr, gc) < m * K, (gr, gc)


def test_edge_cases_cover_both_parities_and_a_second_replacement():
    cases = [p.values[2] for p in edge_cases()]
    assert {(sum(c.pre) + sum(c.mid)) % 2 for c in cases} == {0, 1}
    for e in range(len(EDGES)):
        for m in (0, 1):
            group = cases[(e * 2 + m) * len(L.OPS):(e * 2 + m + 1) * len(L.OPS)]
            assert sum(c.op2 is not None for c in group) == 1
            assert {c.op for c in group} == set(L.OPS)


def test_replace_on_two_ranks(checkpoints, tmp_path):
    # two processes, rows, gloo: a checkpoint written by one rank, then a scatter
    import dataclasses

    from .dist_worker import run_lifecycle
    plate, m = L.Plate(150, 300), 3
    case = L.Case(pre=(K, K), mid=(1,), reads=L.rotate(L.READS, 3), op="load", post=POST,
                  op2="scatter", post2=POST2)
    paths = {"save": str(tmp_path / "saved.bin"),
             "load1": checkpoints(plate, L.target(case.op), case.s0)}
    plan = L.make_plan(plate, case, 2, 1, m * K, paths)
    cfg = config(plate, tb_depth=K, halo_passes=m, decomp="rows")
    run_lifecycle(2, dataclasses.asdict(cfg), plan)


# -- configuration 2: a small plate, short passes, the MPI arithmetic -------------------------

@pytest.mark.parametrize("op", ["load", "scatter"])
@pytest.mark.parametrize("depth,numerics", [(3, "fma"), (4, "fma"), (4, "mpi")])
def test_replace_small_plate(depth, numerics, op, checkpoints, tmp_path):
    plate = L.Plate(40, 70, numerics=numerics)
    # either parity of the step count at every depth
    mid = (depth, 1) if op == "load" else (depth,)
    case = L.Case(pre=(2 * depth, 2 * depth), mid=mid,
                  reads=L.rotate(L.READS, depth + len(mid)), op=op, post=POST,
                  op2="load" if op == "scatter" else "load_local", post2=POST2)
    run_case(plate, case, 1, depth, checkpoints, tmp_path)


def test_continue_np_is_the_trajectory():
    plate = L.Plate(40, 70, insulated="w", periodic="x")
    g, done, at = L.continue_np(L.state(plate, "B", 0), L.S0, 9, cx=plate.cx, cy=plate.cy,
                                insulated="w", periodic="x")
    assert (done, at) == (9, -1)
    assert_bitwise(g, L.state(plate, "B", 9))
    # from step 0 it is reference.run_np
    want = R.run_np(40, 70, 300, converge=True, check_interval=20, eps=0.02, init="random",
                    seed=3, numerics="fma")
    c = L.conv_oracle(0, 20)
    assert (c.steps_done, c.converged_at) == want[1:]
    assert_bitwise(c.grid, want[0])


# -- convergence across a replacement --------------------------------------------------------

def conv_config(interval, compat, depth=8, **kw):
    return HeatConfig(nx=L.CONV["nx"], ny=L.CONV["ny"], steps=0, cx=L.CONV["cx"], cy=L.CONV["cy"],
                      converge=True, check_interval=interval, eps=L.CONV["eps"], init="random",
                      seed=L.CONV["seed"], compat=compat, backend="cpu", tb_depth=depth, **kw)


@pytest.mark.parametrize("op", ["load", "scatter"])
@pytest.mark.parametrize("compat", ["none", "cuda", "mpi"])
@pytest.mark.parametrize("interval,s0", [(20, 25), (7, 25), (50, 33)])
def test_converge_then_replace(interval, s0, compat, op, tmp_path):
    # a. run to convergence, put the step-0 state back at step s0, run again:
    # the checks fall at the absolute steps of the new count.
    first, again = L.conv_oracle(0, interval, compat), L.conv_oracle(s0, interval, compat)
    L.assert_converges_inside(first, 0, interval, compat)
    L.assert_converges_inside(again, s0, interval, compat)
    assert again.converged_at - s0 != first.converged_at
    start = L.conv_start()
    ck = str(tmp_path / "start.bin")
    with HeatSolver(conv_config(interval, compat, depth=1)) as w:
        L.write_checkpoint(w, start, s0, ck)
    with HeatSolver(conv_config(interval, compat)) as s:
        r = s.run(L.CONV_RUN)
        L.assert_run_result(r, first, "first")
        assert s.step == first.converged_at
        assert_bitwise(s.gather(), first.grid, "first")
        if op == "load":
            s.load(ck)
        else:
            s.scatter(start, step=s0)
        assert s.step == s0
        assert_bitwise(s.gather(), start, "replaced")
        r = s.run(L.CONV_RUN)
        L.assert_run_result(r, again, "again")
        assert s.step == again.converged_at
        assert_bitwise(s.gather(), again.grid, "again")


@pytest.mark.parametrize("compat", ["none", "cuda", "mpi"])
def test_converge_then_reset(compat):
    # b. the second life converges where the first did, to the same state.
    first = L.conv_oracle(0, 20, compat)
    with HeatSolver(conv_config(20, compat)) as s:
        for life in range(2):
            r = s.run(L.CONV_RUN)
            L.assert_run_result(r, first, life)
            assert s.step == first.converged_at
            assert_bitwise(s.gather(), first.grid, life)
            s.reset()
            assert s.step == 0
            assert_bitwise(s.gather(), L.conv_start(), "reset")


@pytest.mark.parametrize("compat", ["none", "cuda", "mpi"])
def test_uniform_plate_converges_at_the_next_check(compat):
    # c. 60 steps without converging, then a uniform plate at step s0: the
    # next check (of the new count) sees a residual of exactly 0.
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
        assert np.array_equal(s.gather(), ones)
