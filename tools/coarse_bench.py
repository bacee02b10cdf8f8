#!/usr/bin/env python3
"""Time the coarse-view kernel against the checksum kernel on one MI355X.

One process.  An 8192 x 8192 `random` field and a 1024 x 8192 block of it, the
factors 2x2, 8x8, 64x64 and 512x512.  Each (block, factor) case is timed with
device events over REPS warm repetitions ALTERNATING with checksum_block on
the same block (both kernels alone: no allocation, copy or wait between the
events), so a drift of the machine hits both alike.  Per case it prints the
coarse kernel's median, the field bytes read over that time (lx * ly * 4 / t)
and their share of the 6.3 TB/s HBM read peak, the ratio to the checksum's
median, and the checksum's own repeat-to-repeat spread ((p90 - p10) / median).

Acceptance (8x8 and coarser): coarse median <= checksum median * (1 + spread).
2x2 writes a quarter of what it reads; it is recorded, not gated.

Then the wall time of HeatSolver.coarse(64) against gather() on 8192^2.

Usage: python tools/coarse_bench.py [--reps 30] [--json PATH]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_READ_PEAK = 6.3e12  # bytes/s
FACTORS = [(2, 2), (8, 8), (64, 64), (512, 512)]
GATED_FROM = 8


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be >= 20")

    import torch
    if not torch.cuda.is_available():
        print("coarse_bench: no GPU: not measured", file=sys.stderr)
        return 1
    from parallel_heat_amd import HeatConfig, HeatSolver, _native, ops
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    n = args.n
    f = ops.Field(n, n, halo=1, device=dev)
    ops.init_field(f, ops.Geom(nx=n, ny=n), mode="random", seed=1)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    record = torch.zeros(8, dtype=torch.int64, device=dev)

    def p(t):
        return ctypes.c_void_p(t.data_ptr())

    rows = []
    for (lx, ly, ox) in [(n, n, 0), (min(1024, n), n, n // 2)]:
        origin = ctypes.c_void_p(f.ptr() + 4 * ox * f.pitch)
        for fx, fy in FACTORS:
            cr, cc = -(-n // fx), -(-n // fy)  # 2x2: above the front ends' 2^22-cell limit
            s = torch.zeros(cr * cc, dtype=torch.float64, device=dev)
            kn = torch.zeros(cr * cc, dtype=torch.int32, device=dev)
            kx = torch.zeros(cr * cc, dtype=torch.int32, device=dev)
            _native.call("heat_op_coarse_reset", p(s), p(kn), p(kx), cr * cc, stream)

            def coarse():
                _native.call("heat_op_coarse_raw", origin, f.pitch, lx, ly, ox, 0, n, n, fx, fy,
                             p(s), p(kn), p(kx), stream)

            def checksum():
                _native.call("heat_op_checksum_raw", origin, f.pitch, lx, ly, ox, 0, n, p(record),
                             stream)

            for _ in range(3):  # warm: code objects, the planes' first touch
                coarse()
                checksum()
            torch.cuda.synchronize()
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)]
                  for _ in range(args.reps)]
            for e in ev:  # alternating, one pair of events per kernel
                e[0].record()
                coarse()
                e[1].record()
                checksum()
                e[2].record()
            torch.cuda.synchronize()
            tc = sorted(e[0].elapsed_time(e[1]) * 1e-3 for e in ev)
            tk = sorted(e[1].elapsed_time(e[2]) * 1e-3 for e in ev)
            mc, mk = statistics.median(tc), statistics.median(tk)
            spread = (tk[int(0.9 * (len(tk) - 1))] - tk[int(0.1 * (len(tk) - 1))]) / mk
            rate = lx * ly * 4 / mc
            plan = ops.coarse_plan(f, fx, fy) if (lx, ox) == (n, 0) else None
            row = {"block": f"{lx}x{ly}", "factors": f"{fx}x{fy}", "coarse_us": mc * 1e6,
                   "checksum_us": mk * 1e6, "read_tb_s": rate / 1e12,
                   "share_of_hbm_read_peak": rate / HBM_READ_PEAK, "ratio": mc / mk,
                   "checksum_spread": spread, "gated": fx >= GATED_FROM,
                   "accepted": (mc <= mk * (1 + spread)) if fx >= GATED_FROM else None,
                   "plan": plan}
            rows.append(row)
            print(f"{row['block']:>10} {row['factors']:>8}  coarse {row['coarse_us']:9.1f} us  "
                  f"{row['read_tb_s']:5.2f} TB/s read ({100 * row['share_of_hbm_read_peak']:4.1f} % "
                  f"of the 6.3 TB/s HBM read peak)  checksum {row['checksum_us']:9.1f} us  "
                  f"ratio {row['ratio']:5.2f}  checksum spread {100 * spread:4.1f} %  "
                  f"{'gated: ' + ('ok' if row['accepted'] else 'MISSED') if row['gated'] else 'recorded'}",
                  flush=True)
            del s, kn, kx
    del f
    torch.cuda.empty_cache()

    # End to end: the view of a plate against moving the plate to the host.
    with HeatSolver(HeatConfig(nx=n, ny=n, steps=0, init="random", seed=1, backend="hip",
                               device=0)) as sv:
        sv.coarse(64)
        walls = {"coarse64": [], "gather": []}
        for _ in range(3):
            t0 = time.perf_counter()
            sv.coarse(64)
            walls["coarse64"].append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            sv.gather()
            walls["gather"].append(time.perf_counter() - t0)
    wall = {k: statistics.median(v) for k, v in walls.items()}
    print(f"HeatSolver.coarse(64) on {n}^2: {wall['coarse64'] * 1e3:.2f} ms wall; gather(): "
          f"{wall['gather'] * 1e3:.1f} ms wall", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump({"rows": rows, "wall_s": wall, "reps": args.reps, "n": n}, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
