"""Multi-process worker of the heat-source tests: gloo ranks on the CPU backend.
Each rank sets the same source map (set_source is not collective), checks ITS
extended source block against the ghost rule, runs and gathers."""
import os

import numpy as np

from .dist_worker import free_port


def worker(rank, world, port, cfg_kwargs, map_path, case, edges, steps, out_dir):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from parallel_heat_amd import HeatConfig, HeatSolver
    from parallel_heat_amd.parallel.comm import DistInfo

    from . import source_cases as C

    s = HeatSolver(HeatConfig(**cfg_kwargs), transport="torch",
                   dist_info=DistInfo(rank, world, rank))
    S = np.load(map_path)
    nx, ny, fx, fy, order = case
    s.set_source(S, fx, fy, order)
    C.check_source_block(s, S, case, edges)
    s.run(steps)
    g = s.gather()
    if rank == 0:
        np.savez(os.path.join(out_dir, "source_0.npz"), px=s.info.px, py=s.info.py,
                 halo=s.info.halo, grid=g)
    s.close()
    dist.barrier()
    dist.destroy_process_group()


def run_world(world, cfg_kwargs, S, case, edges, steps, tmp_path):
    import torch.multiprocessing as mp

    map_path = str(tmp_path / "map.npy")
    np.save(map_path, S)
    mp.spawn(worker, args=(world, free_port(), cfg_kwargs, map_path, tuple(case), dict(edges),
                           steps, str(tmp_path)), nprocs=world, join=True)
    return dict(np.load(tmp_path / "source_0.npz"))
