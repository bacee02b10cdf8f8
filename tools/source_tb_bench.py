#!/usr/bin/env python3
"""Time the fused source pass against single source steps on one MI355X.

One process.  Per plate (8192 x 8192 and 1024 x 8192 by default) and depth k
(2, 4 and 8 by default) two things are timed over the whole plate:
  steps_k  k back-to-back gpu::source_step launches, ping-ponging two fields:
           what a source pass of depth k cost before the fused kernel (the
           yardstick; the plate's shrinking boxes are the plate itself),
  tb_k     one gpu::source_tb_step launch of depth k.
The kernels ALTERNATE inside every round, the order rotated, each between its
own pair of device events around BATCH back-to-back repetitions, so a drift of
the machine hits all alike; median and minimum over ROUNDS warm rounds.
--waves W,.. adds the fused kernel under those launch caps (the planner's A/B).

--solver STEPS adds whole Solver runs of STEPS steps with a source at
--tb-depth 8, alternating a solver built with HEAT_SRC_FUSED=0 and one with
HEAT_SRC_FUSED=1 (host clock around run(), which returns after the device has
finished), medians over --solver-rounds runs each.

Printed per plate and kernel: median and minimum time per step (the launch's
time over k), cell-updates per second, and the yardstick's median over the
kernel's (the speed-up).  Nothing is gated: the numbers are recorded
(profiles/source_tb.md).

Usage: python tools/source_tb_bench.py [--rounds 12] [--batch 4] [--depths 2,4,8]
           [--plates RxC,..] [--waves W,..] [--solver STEPS] [--json PATH]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLATES = [(8192, 8192), (1024, 8192)]


def bench_kernels(args, torch, ops, dev, nx, ny, depths, caps):
    a, b, q = (ops.Field(nx, ny, halo=1, device=dev) for _ in range(3))
    geom = ops.Geom(nx=nx, ny=ny)
    ops.init_field(a, geom, mode="random", seed=1)
    b.data.copy_(a.data)
    q.data.uniform_(-1.0, 1.0)

    def steps(k):
        def run():
            s, d = a, b
            for _ in range(k):
                ops.source_step(s, d, q, geom)
                s, d = d, s
        return run

    def fused(k, cap=0):
        def run():
            ops.set_source_tb_max_waves(cap)
            ops.source_tb_step(a, b, q, geom, None, k)
        return run

    kernels = []
    for k in depths:
        kernels += [(f"steps_{k}", steps(k), k, None), (f"tb_{k}", fused(k), k, None)]
        kernels += [(f"tb_{k}_w{w}", fused(k, w), k, w) for w in caps]
    try:
        for _ in range(3):  # warm: code objects, first touch
            for _, fn, _, _ in kernels:
                fn()
        torch.cuda.synchronize()
        n = len(kernels)
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
              for _ in range(args.rounds)]
        for r, e in enumerate(ev):
            order = kernels[r % n:] + kernels[:r % n]
            e[0].record()
            for i, (_, fn, _, _) in enumerate(order):
                for _ in range(args.batch):
                    fn()
                e[i + 1].record()
        torch.cuda.synchronize()
    finally:
        ops.set_source_tb_max_waves(0)
    t = {name: [] for name, _, _, _ in kernels}
    for r, e in enumerate(ev):
        order = kernels[r % n:] + kernels[:r % n]
        for i, (name, _, k, _) in enumerate(order):
            t[name].append(e[i].elapsed_time(e[i + 1]) * 1e-3 / args.batch / k)
    rows = []
    for name, _, k, cap in kernels:
        med, mn = statistics.median(t[name]), min(t[name])
        base = statistics.median(t[f"steps_{k}"])
        row = {"plate": f"{nx}x{ny}", "kernel": name, "depth": k, "us_per_step": med * 1e6,
               "min_us_per_step": mn * 1e6, "tcells_s": nx * ny / med / 1e12,
               "speedup": base / med}
        if name.startswith("tb_"):
            ops.set_source_tb_max_waves(cap or 0)
            row["plan"] = ops.source_tb_plan(a, b, q, None, k)
            ops.set_source_tb_max_waves(0)
        rows.append(row)
        print(f"{row['plate']:>10} {name:>12}  median {row['us_per_step']:8.1f} us/step  "
              f"min {row['min_us_per_step']:8.1f}  {row['tcells_s']:6.3f} Tcells/s  "
              f"x steps_{k} {row['speedup']:5.2f}", flush=True)
    del a, b, q
    torch.cuda.empty_cache()
    return rows


def bench_solver(args, nx, ny):
    import numpy as np
    from parallel_heat_amd import HeatConfig, HeatSolver
    S = np.linspace(-1.0, 1.0, 64 * 64, dtype=np.float32).reshape(64, 64)
    fx, fy = -(-nx // 64), -(-ny // 64)
    S = S[:-(-nx // fx), :-(-ny // fy)].copy()
    cfg = HeatConfig(nx=nx, ny=ny, steps=args.solver, init="random", seed=1, backend="hip",
                     device=0, source=True, tb_depth=8)
    solvers = {}
    for fused in (0, 1):
        os.environ["HEAT_SRC_FUSED"] = str(fused)   # read when the solver is built
        s = HeatSolver(cfg)
        s.set_source(S, fx, fy, 1)
        s.run(args.solver)   # warm: graphs captured
        solvers[fused] = s
    os.environ.pop("HEAT_SRC_FUSED", None)
    t = {0: [], 1: []}
    for r in range(args.solver_rounds):
        for fused in ((0, 1) if r % 2 == 0 else (1, 0)):
            t0 = time.perf_counter()
            solvers[fused].run(args.solver)
            t[fused].append(time.perf_counter() - t0)
    same = bool(np.array_equal(solvers[0].gather(), solvers[1].gather()))
    for s in solvers.values():
        s.close()
    rows = []
    for fused in (0, 1):
        med = statistics.median(t[fused])
        rows.append({"plate": f"{nx}x{ny}", "solver": f"HEAT_SRC_FUSED={fused}",
                     "steps": args.solver, "median_s": med, "min_s": min(t[fused]),
                     "max_s": max(t[fused]), "us_per_step": med / args.solver * 1e6,
                     "tcells_s": nx * ny * args.solver / med / 1e12, "same_bits": same})
        print(f"{nx}x{ny:<6} solver --tb-depth 8 HEAT_SRC_FUSED={fused}: median "
              f"{rows[-1]['us_per_step']:8.1f} us/step ({min(t[fused]) / args.solver * 1e6:.1f} .. "
              f"{max(t[fused]) / args.solver * 1e6:.1f})  {rows[-1]['tcells_s']:6.3f} Tcells/s  "
              f"same bits: {same}", flush=True)
    return rows


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--depths", default="2,4,8")
    ap.add_argument("--waves", default="", help="comma-separated launch caps to A/B")
    ap.add_argument("--plates", default="", help="RxC,.. instead of the two default plates")
    ap.add_argument("--solver", type=int, default=0, help="also time Solver runs of this many steps")
    ap.add_argument("--solver-rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.rounds < 10:
        ap.error("--rounds must be >= 10")

    import torch
    if not torch.cuda.is_available():
        print("source_tb_bench: no GPU: not measured", file=sys.stderr)
        return 1
    from parallel_heat_amd import ops
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    depths = [int(k) for k in args.depths.split(",") if k]
    caps = [int(w) for w in args.waves.split(",") if w]
    plates = [tuple(int(v) for v in p.split("x")) for p in args.plates.split(",") if p] or PLATES
    rows, solver_rows = [], []
    for nx, ny in plates:
        rows += bench_kernels(args, torch, ops, dev, nx, ny, depths, caps)
        if args.solver > 0:
            solver_rows += bench_solver(args, nx, ny)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump({"rows": rows, "solver": solver_rows, "rounds": args.rounds,
                       "batch": args.batch}, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
