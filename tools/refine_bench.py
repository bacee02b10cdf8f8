#!/usr/bin/env python3
"""Time the refinement kernel against a memset and the init kernel on one MI355X.

One process.  Per factor f = fx = fy in {1, 8, 64, 512} and order in {0, 1} one
field is filled by gpu::refine_block (heat_op_refine_raw: the kernel alone, S
and the tables already on the device), by hipMemsetD32Async of the same number
of bytes (a pure write stream: the yardstick) and by gpu::init_field (the
`random` formula, the fill a run starts from today).  The plate is 8192 x 8192
(256 MiB); factor 1 takes a 2048 x 2048 plate, the largest whose source grid
fits the limit of 2^22 cells.  The three fills
ALTERNATE inside every repetition, each between its own pair of device events,
so a drift of the machine hits all alike; medians over REPS warm repetitions.

Printed per case: each median, the bytes written over the refine kernel's time
(lx * ly * 4 / t), the ratios refine / memset and refine / init, and the
memset's own repeat-to-repeat spread ((p90 - p10) / median).
Nothing is gated: the numbers are recorded (profiles/refine.md).

Usage: python tools/refine_bench.py [--reps 20] [--n 8192] [--json PATH]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FACTORS = [1, 8, 64, 512]
MAX_CELLS = 1 << 22


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.reps < 10:
        ap.error("--reps must be >= 10")

    import torch
    if not torch.cuda.is_available():
        print("refine_bench: no GPU: not measured", file=sys.stderr)
        return 1
    from parallel_heat_amd import _native, ops
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemsetD32Async.restype = ctypes.c_int
    hip.hipMemsetD32Async.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t,
                                      ctypes.c_void_p]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def p(t):
        return ctypes.c_void_p(t.data_ptr())

    rows = []
    for f_ in FACTORS:
        n = args.n
        while (-(-n // f_)) ** 2 > MAX_CELLS:
            n //= 2
        fld = ops.Field(n, n, halo=1, device=dev)
        geom = ops.Geom(nx=n, ny=n)
        c = -(-n // f_)
        S = torch.rand((c, c), dtype=torch.float32, device=dev) * 100
        for order in (0, 1):
            tab = [torch.from_numpy(a).to(dev) for a in ops.refine_axis(n, f_, order, False)]

            def refine():
                _native.call("heat_op_refine_raw", ctypes.c_void_p(fld.ptr()), fld.pitch, n, n,
                             p(S), c, p(tab[0]), p(tab[1]), p(tab[2]), p(tab[0]), p(tab[1]),
                             p(tab[2]), stream)

            def memset():
                rc = hip.hipMemsetD32Async(ctypes.c_void_p(fld.data.data_ptr()), 0x42C80000,
                                           n * n, stream)
                if rc != 0:
                    raise RuntimeError(f"hipMemsetD32Async: error {rc}")

            def init():
                ops.init_field(fld, geom, mode="random", seed=1)

            fills = [("refine", refine), ("memset", memset), ("init", init)]
            for _ in range(3):  # warm: code objects, first touch
                for _, fn in fills:
                    fn()
            torch.cuda.synchronize()
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(fills) + 1)]
                  for _ in range(args.reps)]
            for k, e in enumerate(ev):
                # Alternating, the order rotated so that no fill always follows the same one.
                order_k = fills[k % len(fills):] + fills[:k % len(fills)]
                e[0].record()
                for i, (_, fn) in enumerate(order_k):
                    fn()
                    e[i + 1].record()
            torch.cuda.synchronize()
            t = {name: [] for name, _ in fills}
            for k, e in enumerate(ev):
                order_k = fills[k % len(fills):] + fills[:k % len(fills)]
                for i, (name, _) in enumerate(order_k):
                    t[name].append(e[i].elapsed_time(e[i + 1]) * 1e-3)
            med = {k: statistics.median(v) for k, v in t.items()}
            ms = sorted(t["memset"])
            spread = (ms[int(0.9 * (len(ms) - 1))] - ms[int(0.1 * (len(ms) - 1))]) / med["memset"]
            nbytes = n * n * 4
            row = {"plate": f"{n}x{n}", "mib": nbytes / 2 ** 20, "factor": f_, "order": order,
                   "source": f"{c}x{c}", "plan": ops.refine_plan(fld),
                   **{f"{k}_us": v * 1e6 for k, v in med.items()},
                   "refine_tb_s": nbytes / med["refine"] / 1e12,
                   "memset_tb_s": nbytes / med["memset"] / 1e12,
                   "refine_over_memset": med["refine"] / med["memset"],
                   "refine_over_init": med["refine"] / med["init"],
                   "memset_spread": spread}
            rows.append(row)
            print(f"{row['plate']:>10} f {f_:>3} order {order}  refine {row['refine_us']:8.1f} us "
                  f"({row['refine_tb_s']:4.2f} TB/s written)  "
                  f"memset {row['memset_us']:8.1f} us ({row['memset_tb_s']:4.2f} TB/s)  "
                  f"init {row['init_us']:8.1f} us  refine/memset {row['refine_over_memset']:5.2f}  "
                  f"refine/init {row['refine_over_init']:5.2f}  "
                  f"memset spread {100 * spread:4.1f} %", flush=True)
            del tab
        del fld, S
        torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump({"rows": rows, "reps": args.reps, "n": args.n}, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
