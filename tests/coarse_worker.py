"""Multi-process worker of the coarse-view tests: gloo ranks on the CPU
backend, each calling HeatSolver.coarse (a collective) and saving what IT got,
so the test can compare every rank's planes."""
import os

import numpy as np

from .dist_worker import free_port


def worker(rank, world, port, cfg_kwargs, grid_path, fx, fy, steps, out_dir):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from parallel_heat_amd import HeatConfig, HeatSolver
    from parallel_heat_amd.parallel.comm import DistInfo

    s = HeatSolver(HeatConfig(**cfg_kwargs), transport="torch", dist_info=DistInfo(rank, world, rank))
    # Rank 0 scatters the grid with 0 steps: the state is exactly that data.
    s.scatter(np.load(grid_path) if rank == 0 else None)
    v0 = s.coarse(fx, fy)
    s.run(steps)
    v1 = s.coarse(fx, fy)
    g = s.gather()
    out = {f"{k}0": v0[k] for k in ("sum", "min", "max", "mean", "count")}
    out.update({f"{k}1": v1[k] for k in ("sum", "min", "max")})
    if rank == 0:
        out["grid"] = g
    np.savez(os.path.join(out_dir, f"coarse_{rank}.npz"), px=s.info.px, py=s.info.py, **out)
    s.close()
    dist.barrier()
    dist.destroy_process_group()


def run_world(world, cfg_kwargs, grid, fx, fy, steps, tmp_path):
    """Every rank's result of a gloo world: a list of dicts, rank order."""
    import torch.multiprocessing as mp

    grid_path = str(tmp_path / "start.npy")
    np.save(grid_path, grid)
    mp.spawn(worker, args=(world, free_port(), cfg_kwargs, grid_path, fx, fy, steps, str(tmp_path)),
             nprocs=world, join=True)
    return [dict(np.load(tmp_path / f"coarse_{r}.npz")) for r in range(world)]
