"""Cost of getting a causal mask into the flash kernels' packed form: generated from an
``xdot.StructuredMask`` (``mask_gen``) against the dense route (``mask_pack`` of a (B, R, T)
boolean tensor, with and without the torch ops that build that tensor).

    python benchmarks/bench_mask.py                        # (R, T) = (25000, 25000) and (3125, 25000)
    python benchmarks/bench_mask.py --shapes 4096x4096 --iters 20
    python benchmarks/bench_mask.py --docs 8,256,4096      # causal + N equal documents over T

One JSON line per (shape, route): median / min GPU ms over ``--iters`` HIP-event timed calls
after ``--warmup`` calls, the peak device memory one call adds on top of what is resident
before it (for ``mask_pack`` alone the dense input is resident, so ``resident_B`` is listed
too), and the bytes written per second.

``--docs N[,N...]``: the spec becomes ``StructuredMask(causal=True, doc_starts=<N equal documents
over T, a device tensor>)`` (one block of lines per N, each with ``"docs": N``); the ``mask_gen``
line then also carries ``causal_ms``, the causal-only generation timed alternately with it in the
same process, and ``vs_causal``, the ratio of the two medians (``generate_mask`` calls: they include
the torch ops that turn ``doc_starts`` into the kernel's int32 table); ``kernel_ms`` /
``causal_kernel_ms`` / ``kernel_vs_causal`` are the same for the ``mask_gen`` op alone on prepared
inputs, per call over windows of 20 back-to-back calls.
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
    ap.add_argument("--docs", default=None, help="comma-separated document counts: causal + N equal documents over T")
    a = ap.parse_args()
    from xdot import StructuredMask, _ext
    from xdot.ops import flash

    dev = torch.device("cuda", 0)
    B = a.B
    causal = StructuredMask(causal=True)
    for shape in a.shapes.split(","):
        R, T = (int(x) for x in shape.lower().split("x"))
        ro = a.row_offset if a.row_offset is not None else T - R
        for docs in [None] if a.docs is None else [int(n) for n in a.docs.split(",")]:
            spec = causal if docs is None else StructuredMask(
                causal=True, doc_starts=(torch.arange(docs, device=dev, dtype=torch.int64) * T) // docs)

            def build_dense():  # what a user of the dense interface writes
                if docs is not None:
                    return spec.dense(B, R, T, ro, dev)
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
                extra = {}
                if docs is not None and name == "mask_gen":  # against causal alone, taking turns call by call
                    both = [fn, lambda: flash.generate_mask(causal, B, R, T, ro, device=dev)]
                    ts = ([], [])
                    for i in range(2 * (a.warmup + a.iters)):
                        t, _ = timeit(both[i % 2], 1, 0)
                        if i >= 2 * a.warmup:
                            ts[i % 2].append(t)
                    ms, mn, cms = statistics.median(ts[0]), min(ts[0]), statistics.median(ts[1])
                    extra = {"causal_ms": round(cms, 4), "vs_causal": round(ms / cms, 3)}
                    # the kernel alone: the op on prepared inputs, windows of 20 back-to-back calls
                    op, ds32 = _ext.ops().mask_gen, spec.device_doc_starts(dev)
                    table = torch.tensor([[0, T, 0]], dtype=torch.int32, device=dev)
                    kern = [lambda: [op(B, R, T, True, 0, ro, None, table, ds32) for _ in range(20)],
                            lambda: [op(B, R, T, True, 0, ro, None, table) for _ in range(20)]]
                    ks = ([], [])
                    for i in range(2 * (a.warmup + a.iters)):
                        t, _ = timeit(kern[i % 2], 1, 0)
                        if i >= 2 * a.warmup:
                            ks[i % 2].append(t / 20)
                    k, ck = statistics.median(ks[0]), statistics.median(ks[1])
                    extra.update(kernel_ms=round(k, 4), causal_kernel_ms=round(ck, 4), kernel_vs_causal=round(k / ck, 3),
                                 causal_kernel_min_max=[round(min(ks[1]), 4), round(max(ks[1]), 4)])
                else:
                    ms, mn = timeit(fn, a.iters, a.warmup)
                peak, base = peak_of(fn, dev)
                row = {"route": name, "B": B, "R": R, "T": T, "row_offset": ro, "ms": round(ms, 4),
                       "min_ms": round(mn, 4), "peak_B": peak, "resident_B": base, "packed_B": out_bytes,
                       "write_GB_s": round(out_bytes / ms / 1e6, 1)}
                if docs is not None:
                    row = dict(row, docs=docs, **extra)
                print(json.dumps(row), flush=True)
                del dense


if __name__ == "__main__":
    main()
