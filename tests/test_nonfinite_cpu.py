"""The convergence decision end to end on the CPU backend: a residual exactly
at the threshold, and a non-finite residual on one rank of several.  eps =
1e30 makes any finite residual converge at the first check, so a NaN that the
cross-rank max drops shows as a false "converged" (torch's gloo MAX did drop
it: of [1, NaN, 3] it returned 1).  tests/test_gpu_nonfinite.py runs the GPU
paths."""
import numpy as np
import pytest

from parallel_heat_amd import HeatConfig, HeatSolver

from . import service_cases as SC
from .dist_worker import free_port, run_outcomes

NX, NY, C = 24, 40, 5
RANKS = dict(nx=NX, ny=NY, steps=C, init="zero", converge=True, check_interval=C, eps=1e30,
             backend="cpu")


def test_threshold_cpu():
    def solve(kw):
        with HeatSolver(HeatConfig(backend="cpu", **kw)) as s:
            r = s.run()
            return r, s.gather()
    SC.check_threshold(solve)


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_nonfinite_one_rank_cpu(bad):
    from parallel_heat_amd import _native
    with HeatSolver(HeatConfig(**{**RANKS, "eps": 1e-3})) as s:
        s.load_local(SC.bad_grid(NX, NY, (11, 17), bad))
        with pytest.raises(_native.NativeError, match=r"non-finite.* at step 5\b"):
            s.run()


WORLDS = {2: (dict(decomp="rows"), (2, 1)), 3: (dict(decomp="rows"), (3, 1)),
          4: (dict(px=2, py=2), (2, 2))}


@pytest.mark.parametrize("world,block", [(w, b) for w in WORLDS for b in range(w)])
def test_nonfinite_gloo_ranks(tmp_path, world, block):
    # The NaN in each block in turn: every rank must raise, whoever holds it.
    kw, blocks = WORLDS[world]
    at = SC.block_centres(NX, NY, *blocks)[block]
    texts = run_outcomes(world, {**RANKS, **kw}, C, SC.bad_grid(NX, NY, at, np.nan), tmp_path)
    SC.assert_all_nonfinite(texts, C)


def _allreduce_worker(rank, world, port, out_dir):
    import os

    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from parallel_heat_amd.parallel.comm import TorchDistTransport
    t = TorchDistTransport()
    rows = np.array(VECTORS, np.float32)[:, rank, :].copy()
    for row in rows:
        assert t._allreduce(None, row.ctypes.data, row.size, 0) == 0, t._error
    np.save(os.path.join(out_dir, f"max_{rank}.npy"), rows)
    dist.destroy_process_group()


nan, inf = np.nan, np.inf
# VECTORS[case][rank]: what each of three ranks holds.
VECTORS = [
    [[nan, 1.0, 1.0, -5.0], [1.0, nan, 1.0, -7.0], [3.0, 3.0, nan, -6.0]],  # a NaN on each rank
    [[-nan, inf, -inf, -0.0], [2.0, nan, -inf, -1e-45], [-2.0, -inf, -inf, -1.0]],
    [[1e-45, -3.5, 3e38, 0.0], [0.0, -2.5, -3e38, -0.0], [-1e-45, -4.5, 1.0, -0.0]],
]


def test_gloo_max_propagates_nan_and_orders_signed_values(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_allreduce_worker, args=(3, free_port(), str(tmp_path)), nprocs=3, join=True)
    want = np.array([[nan, nan, nan, -5.0],
                     [nan, nan, -inf, -0.0],
                     [1e-45, -2.5, 3e38, 0.0]], np.float32)
    for rank in range(3):
        got = np.load(tmp_path / f"max_{rank}.npy")
        assert np.array_equal(got, want, equal_nan=True), (rank, got)
        assert not np.signbit(got[2, 3])  # max(0.0, -0.0, -0.0) by the int keys is +0.0
