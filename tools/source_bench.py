#!/usr/bin/env python3
"""Time the source step against the LDS-staged step on one MI355X.

One process.  Per plate (8192 x 8192 and 1024 x 8192 by default) one step over
the whole plate is timed for gpu::lds_step (the yardstick: the project's other
one-step kernel, 8 B per cell-update), gpu::source_step as it runs by default
(src_auto), with plain accesses (src) and with non-temporal q loads and dst
stores (src_nt; 12 B per cell-update each).  The kernels ALTERNATE inside
every round, the order rotated, each between its own pair of device events around BATCH back-to-back launches,
so a drift of the machine hits all alike; median and minimum over ROUNDS warm
rounds.  --waves W,.. adds both source kernels under those launch caps (the
planner's A/B); --plates RxC,.. times other plates (the non-temporal
threshold's A/B).

Printed per plate and kernel: median and minimum time per step, the bytes the
algorithm moves over the median (GB/s), and the ratio to lds_step's median: the
expectation is 1.5 (12 B against 8), 1.65 with the 10 % allowed for the third
stream.  Nothing is gated: the numbers are recorded (profiles/source.md).

Usage: python tools/source_bench.py [--rounds 12] [--batch 10] [--plates RxC,..] [--json PATH]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLATES = [(8192, 8192), (1024, 8192)]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--waves", default="", help="comma-separated launch caps to A/B")
    ap.add_argument("--plates", default="", help="RxC,.. instead of the two default plates")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.rounds < 10:
        ap.error("--rounds must be >= 10")

    import torch
    if not torch.cuda.is_available():
        print("source_bench: no GPU: not measured", file=sys.stderr)
        return 1
    from parallel_heat_amd import ops
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    caps = [int(w) for w in args.waves.split(",") if w]

    rows = []
    plates = [tuple(int(v) for v in p.split("x")) for p in args.plates.split(",") if p] or PLATES
    for nx, ny in plates:
        src, dst, q = (ops.Field(nx, ny, halo=1, device=dev) for _ in range(3))
        geom = ops.Geom(nx=nx, ny=ny)
        ops.init_field(src, geom, mode="random", seed=1)
        q.data.uniform_(-1.0, 1.0)

        def lds():
            ops.lds_step(src, dst, geom)

        def source(nt, cap=0):
            def run():
                ops.set_source_nontemporal(nt)
                ops.set_source_max_waves(cap)
                ops.source_step(src, dst, q, geom)
            return run

        kernels = [("lds", lds, 8), ("src_auto", source(-1), 12), ("src", source(0), 12),
                   ("src_nt", source(1), 12)]
        kernels += [(f"src_w{w}", source(0, w), 12) for w in caps]
        kernels += [(f"src_nt_w{w}", source(1, w), 12) for w in caps]
        try:
            for _ in range(3):  # warm: code objects, first touch
                for _, fn, _ in kernels:
                    fn()
            torch.cuda.synchronize()
            n = len(kernels)
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
                  for _ in range(args.rounds)]
            for k, e in enumerate(ev):
                order = kernels[k % n:] + kernels[:k % n]
                e[0].record()
                for i, (_, fn, _) in enumerate(order):
                    for _ in range(args.batch):
                        fn()
                    e[i + 1].record()
            torch.cuda.synchronize()
        finally:
            ops.set_source_nontemporal(-1)
            ops.set_source_max_waves(0)
        t = {name: [] for name, _, _ in kernels}
        for k, e in enumerate(ev):
            order = kernels[k % n:] + kernels[:k % n]
            for i, (name, _, _) in enumerate(order):
                t[name].append(e[i].elapsed_time(e[i + 1]) * 1e-3 / args.batch)
        lds_med = statistics.median(t["lds"])
        for name, _, bpc in kernels:
            med, mn = statistics.median(t[name]), min(t[name])
            row = {"plate": f"{nx}x{ny}", "kernel": name, "median_us": med * 1e6,
                   "min_us": mn * 1e6, "bytes_per_cell": bpc,
                   "gb_s": nx * ny * bpc / med / 1e9, "over_lds": med / lds_med}
            if name == "src":
                row["plan"] = ops.source_plan(src, dst, q)
            rows.append(row)
            print(f"{row['plate']:>10} {name:>10}  median {row['median_us']:8.1f} us  "
                  f"min {row['min_us']:8.1f} us  {row['gb_s']:7.0f} GB/s ({bpc} B/cell)  "
                  f"x lds {row['over_lds']:5.2f}", flush=True)
        del src, dst, q
        torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump({"rows": rows, "rounds": args.rounds, "batch": args.batch}, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
