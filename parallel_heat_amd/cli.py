"""``python -m parallel_heat_amd`` — the Python front end of the ``heat`` CLI.

Same flags as the native ``build/heat`` binary (tests/test_cli.py pins the
two flag sets and their reference output lines against each other).
Multi-rank runs are launched with ``python -m torch.distributed.run
--nproc-per-node N -m parallel_heat_amd ...``: GPU ranks talk over the
engine's RCCL communicator, CPU ranks over torch.distributed (gloo).  The
single-process native modes -- ``--gpus N`` (N GPU ranks as threads of one
process) and ``--plan`` (the per-GPU memory plan) -- run the native binary
with the same arguments.  ``--transport torch`` is the one Python-only value.  Replaces the reference's -D macro builds
(``cuda/Makefile``, ``mpi/Makefile:12-22``) with run-time flags.
"""
from __future__ import annotations

import argparse
import json
import struct
import subprocess
import sys

import torch

from . import _native
from .models.config import HeatConfig, check_edges, parse_insulated
from .models.heat2d import HeatSolver
from .parallel import comm as pcomm
from .utils import io as hio
from .utils import report


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m parallel_heat_amd",
                                description="2-D heat diffusion on MI355X (5-point Jacobi)")
    a = p.add_argument
    a("--nx", type=int, default=20)
    a("--ny", type=int, default=20)
    a("--steps", type=int, default=10000)
    a("--cx", type=float, default=0.1)
    a("--cy", type=float, default=0.1)
    a("--converge", action="store_true")
    a("--check-interval", type=int, default=20)
    a("--eps", type=float, default=1e-3)
    a("--backend", choices=["cpu", "hip"], default=None)
    a("--threads", type=int, default=0)
    a("--kernel", choices=["auto", "naive", "tb", "lds", "mfma", "src"], default="auto")
    a("--tb-depth", type=int, default=0)
    a("--decomp", choices=["auto", "rows", "1d", "2d"], default="auto")
    a("--px", type=int, default=0)
    a("--py", type=int, default=0)
    a("--init", choices=["ref-wrap", "exact", "ref64", "random", "zero"], default="ref-wrap")
    a("--seed", type=int, default=0)
    a("--out", default=None)
    a("--out-format", choices=["dat", "bin", "checksum"], default="dat")
    a("--coarse", default=None, metavar="FX[xFY]",
      help="after the run, also write a coarse view of the final state: one value per FX x FY "
           "block of cells (FY = FX if omitted), reduced on the device; needs --coarse-out "
           "(at most 2^22 coarse cells)")
    a("--coarse-out", default=None, metavar="PATH",
      help="its file: a grid of ceil(nx/FX) x ceil(ny/FY) values, text with --out-format dat, "
           "else binary")
    a("--coarse-stat", choices=["mean", "min", "max"], default="mean",
      help="the value written per coarse cell")
    a("--init-from", default=None, metavar="PATH",
      help="start from a coarse grid: a binary grid file (what --coarse-out writes) refined "
           "onto the plate on the device; overrides --init, the run starts at step 0; not with "
           "--resume")
    a("--refine", default=None, metavar="FX[xFY]",
      help="its integer factors (FY = FX if omitted); the file must hold ceil(nx/FX) x "
           "ceil(ny/FY) values (default: ceil(nx/rows) x ceil(ny/cols))")
    a("--refine-order", type=int, choices=[0, 1], default=1,
      help="0 piecewise constant, 1 cell-centred bilinear")
    a("--source-from", default=None, metavar="PATH",
      help="a static heat source: a binary grid file refined onto the plate like "
           "--init-from's; every step then adds it, u' = A u + q, with the one-step src kernel "
           "(--kernel auto becomes src); not with --numerics mpi; checkpoints do not store it")
    a("--source-refine", default=None, metavar="FX[xFY]",
      help="its integer factors [ceil(nx/rows) x ceil(ny/cols)]")
    a("--source-order", type=int, choices=[0, 1], default=1,
      help="piecewise constant, or cell-centred bilinear")
    a("--naming", choices=["plain", "mpi", "cuda"], default="plain")
    a("--dump-initial", action="store_true")
    a("--compat", choices=["none", "mpi", "cuda"], default=None)
    a("--no-graph", action="store_true")
    a("--no-overlap", action="store_true")
    a("--schedule", choices=["auto", "sync", "overlap", "pipeline"], default="auto")
    a("--halo-passes", type=int, default=0)
    a("--numerics", choices=["fp32", "mpi"], default="fp32")
    a("--phase-timing", action="store_true")
    a("--insulated", default="", metavar="SIDES",
      help="insulated (zero-flux) plate edges: any of the letters nswe (n = row 0, w = column 0), "
           "or all; the other edges keep their temperature")
    a("--periodic", default="", metavar="AXES",
      help="periodic (wrap-around) axes: x (north and south edges joined), y (west and east "
           "joined) or xy")
    a("--transport", choices=["auto", "local", "rccl", "torch", "tcp", "loopback"], default="auto",
      help="loopback: --gpus ranks sharing a device (native binary)")
    a("--port", type=int, default=0, help="tcp transport rendezvous port (0: MASTER_PORT+1)")
    a("--gpus", type=int, default=0,
      help="one process, N GPU ranks as threads (native binary): RCCL with a GPU per rank, "
           "else loopback copies")
    a("--watchdog", type=float, default=None,
      help="multi-rank GPU runs: abort and exit 1 after this many seconds without device "
           "progress (HEAT_WATCHDOG_S, default 300, 0 = never)")
    a("--plan", action="store_true", help="print the per-GPU memory plan and exit (native)")
    a("--checkpoint", default=None)
    a("--checkpoint-every", type=int, default=0)
    a("--resume", default=None)
    a("--warmup", type=int, default=0,
      help="N untimed steps first (graph capture), then the initial state is restored")
    a("--json", action="store_true")
    return p


def parse_coarse(text: str, flag: str = "--coarse"):
    """"FX" or "FXxFY" -> (fx, fy); ValueError if malformed or a factor < 1."""
    parts = text.lower().split("x")
    try:
        f = [int(p) for p in parts]
    except ValueError:
        f = []
    if len(f) not in (1, 2):
        raise ValueError(f"{flag} {text}: expected FX or FXxFY (integer factors)")
    fx, fy = f[0], f[-1]
    if fx < 1 or fy < 1:
        raise ValueError(f"{flag} {text}: a factor must be >= 1")
    return fx, fy


def load_init_from(path: str, refine, order: int, nx: int, ny: int):
    """The source grid of --init-from and its factors: (S, fx, fy).  ValueError
    if the file's dimensions are not what the factors give for the plate."""
    from .ops import coarse_dims
    try:
        h = hio.read_bin_header(path)
    except (OSError, struct.error) as e:
        raise ValueError(f"cannot read {path}: {e}")
    cr, cc = int(h["nx"]), int(h["ny"])
    limit = 1 << 22
    if cr < 1 or cc < 1 or cr * cc > limit:
        raise ValueError(f"{path} holds a {cr}x{cc} grid: above the limit of {limit} source "
                         "cells (2^22)")
    fx, fy = refine if refine is not None else (-(-nx // cr), -(-ny // cc))
    r, c = coarse_dims(nx, ny, fx, fy)
    if (r, c) != (cr, cc):
        raise ValueError(f"refine: a {cr}x{cc} source grid does not fit factors {fx}x{fy} on a "
                         f"{nx}x{ny} plate, which need a {r}x{c} grid")
    S, _ = hio.read_bin(path, mmap=False)
    return S, fx, fy


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    parser = build_parser()
    args = parser.parse_args(argv)
    try:
        parse_insulated(args.insulated)
        check_edges(args.insulated, args.periodic)
    except ValueError as e:
        parser.error(str(e))
    coarse = None
    if (args.coarse is None) != (args.coarse_out is None):
        missing = "--coarse-out PATH" if args.coarse_out is None else "--coarse FX[xFY]"
        parser.error(f"--coarse and --coarse-out go together ({missing} is missing)")
    if args.coarse is not None:
        try:
            coarse = parse_coarse(args.coarse)
            from .ops import coarse_dims
            coarse_dims(args.nx, args.ny, *coarse)
        except (ValueError, _native.NativeError) as e:
            parser.error(f"--coarse: {e}" if not str(e).startswith("--coarse") else str(e))
    init_from = None
    if args.refine is not None and args.init_from is None:
        parser.error("--refine needs --init-from PATH")
    if args.init_from is not None:
        if args.resume:
            parser.error("--init-from and --resume both set the starting state: choose one")
        try:
            refine = None if args.refine is None else parse_coarse(args.refine, "--refine")
            init_from = load_init_from(args.init_from, refine, args.refine_order, args.nx,
                                       args.ny)
        except (ValueError, _native.NativeError) as e:
            parser.error(f"--init-from: {e}" if not str(e).startswith("--refine") else str(e))
    source = None
    if args.source_refine is not None and args.source_from is None:
        parser.error("--source-refine needs --source-from PATH")
    if args.source_from is not None:
        if args.numerics != "fp32":
            parser.error("--source-from needs --numerics fp32: the source step evaluates the "
                         "canonical fp32 expression only")
        if args.kernel not in ("auto", "src"):
            parser.error(f"--source-from runs the src kernel: --kernel {args.kernel} has no "
                         "source term")
        try:
            refine = (None if args.source_refine is None
                      else parse_coarse(args.source_refine, "--source-refine"))
            source = load_init_from(args.source_from, refine, args.source_order, args.nx, args.ny)
        except (ValueError, _native.NativeError) as e:
            parser.error(f"--source-from: {e}" if not str(e).startswith("--source-refine")
                         else str(e))
    elif args.kernel == "src":
        parser.error("--kernel src is the kernel of a run with a heat source: it needs "
                     "--source-from PATH")
    if args.gpus > 0 or args.plan:
        # Single-process native modes: the `heat` binary owns the threads
        # and the planner; same flags, same output.
        return subprocess.run([str(_native.CLI_PATH)] + argv).returncode
    if args.watchdog is not None:
        import os
        os.environ["HEAT_WATCHDOG_S"] = str(args.watchdog)  # read by the native solver
    if args.transport == "loopback":
        raise SystemExit("--transport loopback is the --gpus mode of ranks sharing a device")
    backend = args.backend or ("hip" if torch.cuda.is_available() else "cpu")
    compat = args.compat or {"mpi": "mpi", "cuda": "cuda"}.get(args.naming, "none")
    cfg = HeatConfig(nx=args.nx, ny=args.ny, steps=args.steps, cx=args.cx, cy=args.cy,
                     converge=args.converge, check_interval=args.check_interval, eps=args.eps,
                     init=args.init, seed=args.seed, backend=backend,
                     kernel="src" if source is not None else args.kernel,
                     tb_depth=args.tb_depth, threads=args.threads, decomp=args.decomp,
                     px=args.px, py=args.py, use_graph=not args.no_graph,
                     overlap=not args.no_overlap, compat=compat, schedule=args.schedule,
                     halo_passes=args.halo_passes, numerics=args.numerics,
                     phase_timing=args.phase_timing, insulated=args.insulated,
                     periodic=args.periodic, source=source is not None)
    info = pcomm.init_distributed("nccl" if backend == "hip" else "gloo")
    root = info.is_root
    out = sys.stdout
    if root and args.naming == "mpi":
        out.write(report.mpi_banner(info.world, cfg.nx, cfg.ny, cfg.steps, cfg.converge))
        out.flush()
    if args.port and args.transport == "tcp":
        import os
        os.environ["MASTER_PORT"] = str(args.port - 1)  # make_comm uses MASTER_PORT + 1
    solver = HeatSolver(cfg, transport=args.transport, dist_info=info)
    if source is not None:
        solver.set_source(source[0], source[1], source[2], order=args.source_order)
    if args.resume:
        solver.load(args.resume)

    def start():
        if init_from is not None:
            solver.refine(init_from[0], init_from[1], init_from[2], order=args.refine_order)

    start()

    small = cfg.nx * cfg.ny <= (1 << 24)
    if args.naming == "mpi":
        init_path, final_path = "initial_im.dat", "final_im.dat"
    elif args.naming == "cuda":
        init_path, final_path = None, report.cuda_output_name(cfg.nx, cfg.ny, cfg.steps)
    else:
        init_path, final_path = "initial.dat", ("final.dat" if small else None)
    if args.out is not None:
        final_path = None if args.out == "none" else args.out

    def emit(path):
        if not path:
            return
        if args.out_format == "bin":
            solver.save(path)
        elif args.out_format == "checksum":
            c = solver.checksum()
            if root:
                with open(path, "w") as f:
                    f.write(json.dumps({"nx": cfg.nx, "ny": cfg.ny, "step": solver.step, **c}) + "\n")
        else:
            g = solver.gather()
            if root:
                hio.write_dat(path, g)

    if args.warmup > 0:
        # Untimed warm-up (graph capture, first touch), then the initial
        # state again: the timed run and the output are a cold run's.
        if args.resume:
            raise SystemExit("--warmup with --resume")
        solver.run(args.warmup)
        solver.reset()
        start()
    if args.dump_initial or args.naming == "mpi":
        emit(init_path)
    total = cfg.total_steps()
    todo = total - solver.step
    acc = dict(steps_done=0, seconds=0.0, passes=0, exchanges=0, checks=0, t_exchange=0.0,
               t_compute=0.0, t_reduce=0.0)
    converged, converged_at, last = False, -1, -1.0
    while todo > 0:
        chunk = min(args.checkpoint_every, todo) if args.checkpoint_every > 0 else todo
        r = solver.run(chunk)
        for k in acc:
            acc[k] += getattr(r, k)
        last = r.last_resid
        todo -= r.steps_done
        if args.checkpoint and args.checkpoint_every > 0:
            solver.save(args.checkpoint)
        if r.converged:
            converged, converged_at = True, r.converged_at
            break
    emit(final_path)
    coarse_info = None
    if coarse is not None:
        # The chosen statistic of the final state as a CR x CC fp32 grid (the
        # mean rounded once from fp64): prtdat text, or a binary grid whose
        # header holds nx = CR, ny = CC and the step.
        v = solver.coarse(*coarse)
        g = v[args.coarse_stat].astype("float32")
        if root:
            if args.out_format == "dat":
                hio.write_dat(args.coarse_out, g)
            else:
                hio.write_bin(args.coarse_out, g, step=solver.step, cx=cfg.cx, cy=cfg.cy)
        coarse_info = {"fx": coarse[0], "fy": coarse[1], "rows": int(g.shape[0]),
                       "cols": int(g.shape[1]), "stat": args.coarse_stat,
                       "path": args.coarse_out}
    if root:
        if cfg.converge:
            out.write(report.convergence_line(args.naming, converged, converged_at, solver.step))
        out.write(report.elapsed_line(args.naming, acc["seconds"]))
        if args.json:
            cells = cfg.nx * cfg.ny * acc["steps_done"]
            out.write(report.metrics_json(
                nx=cfg.nx, ny=cfg.ny, steps=total, steps_done=acc["steps_done"],
                ranks=info.world, backend=backend,
                decomp=f"{solver.info.px}x{solver.info.py}", tb_depth=solver.info.tb_depth,
                seconds=acc["seconds"],
                mcells_per_s=cells / acc["seconds"] / 1e6 if acc["seconds"] > 0 else 0.0,
                s_per_1000_iters=acc["seconds"] * 1000 / max(1, acc["steps_done"]),
                converged=converged, converged_at=converged_at, last_resid=last,
                passes=acc["passes"], exchanges=acc["exchanges"],
                transport=solver.transport, schedule=solver.info.schedule,
                halo=solver.info.halo, t_exchange=acc["t_exchange"],
                t_compute=acc["t_compute"], t_reduce=acc["t_reduce"],
                insulated=solver.info.insulated, periodic=solver.info.periodic,
                native=_native.loaded_path(),
                **({"coarse": coarse_info} if coarse_info else {}),
                **({"init_from": {"path": args.init_from, "rows": int(init_from[0].shape[0]),
                                  "cols": int(init_from[0].shape[1]), "fx": init_from[1],
                                  "fy": init_from[2], "order": args.refine_order}}
                   if init_from is not None else {}),
                **({"source": {"path": args.source_from, "rows": int(source[0].shape[0]),
                               "cols": int(source[0].shape[1]), "fx": source[1],
                               "fy": source[2], "order": args.source_order}}
                   if source is not None else {})) + "\n")
        out.flush()
    solver.barrier()
    solver.close()
    return 0


if __name__ == "__main__":  # pragma: no cover
    sys.exit(main())
