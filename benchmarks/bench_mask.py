"""Cost of getting a causal mask into the flash kernels' packed form: generated from an
``xdot.StructuredMask`` (``mask_gen``) against the dense route (``mask_pack`` of a (B, R, T)
boolean tensor, with and without the torch ops that build that tensor).

    python benchmarks/bench_mask.py                        # (R, T) = (25000, 25000) and (3125, 25000)
    python benchmarks/bench_mask.py --shapes 4096x4096 --iters 20

One JSON line per (shape, route): median / min GPU ms over ``--iters`` HIP-event timed calls
after ``--warmup`` calls, the peak device memory one call adds on top of what is resident
before it (for ``mask_pack`` alone the dense input is resident, so ``resident_B`` is listed
too), and the bytes written per second.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timeit(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts)


def peak_of(fn, dev):
    """(bytes one call adds at its peak, bytes resident before it)."""
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    out = fn()
    torch.cuda.synchronize(dev)
    peak = torch.cuda.max_memory_allocated(dev) - base
    del out
    return peak, base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="25000x25000,3125x25000", help="comma-separated RxT")
    ap.add_argument("--B", type=int, default=1)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--row-offset", type=int, default=None, help="default: T - R (the last rank's rows)")
    a = ap.parse_args()
    from xdot import StructuredMask
    from xdot.ops import flash

    dev = torch.device("cuda", 0)
    B = a.B
    spec = StructuredMask(causal=True)
    for shape in a.shapes.split(","):
        R, T = (int(x) for x in shape.lower().split("x"))
        ro = a.row_offset if a.row_offset is not None else T - R

        def build_dense():  # what a user of the dense interface writes
            gr = ro + torch.arange(R, device=dev).view(R, 1)
            return (torch.arange(T, device=dev).view(1, T) > gr).unsqueeze(0).expand(B, R, T).contiguous()

        routes = [("mask_gen", lambda: flash.generate_mask(spec, B, R, T, ro, device=dev), False),
                  ("dense_build+mask_pack", lambda: flash.prepare_mask(build_dense(), B, R, T), False),
                  ("mask_pack", None, True)]
        out_bytes = None
        for name, fn, needs_dense in routes:
            dense = build_dense() if needs_dense else None
            if needs_dense:
                fn = lambda: flash.prepare_mask(dense, B, R, T)  # noqa: E731
            if out_bytes is None:
                pk = fn()
                out_bytes = pk.bits.numel() * 8 + pk.bits_t.numel() * 8 + pk.flags.numel()
                del pk
            ms, mn = timeit(fn, a.iters, a.warmup)
            peak, base = peak_of(fn, dev)
            print(json.dumps({"route": name, "B": B, "R": R, "T": T, "row_offset": ro, "ms": round(ms, 4),
                              "min_ms": round(mn, 4), "peak_B": peak, "resident_B": base, "packed_B": out_bytes,
                              "write_GB_s": round(out_bytes / ms / 1e6, 1)}), flush=True)
            del dense


if __name__ == "__main__":
    main()
