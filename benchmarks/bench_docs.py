"""Module step under a document mask (``StructuredMask(causal=True, doc_starts=...)``: several
documents packed into one sequence) against the same step under ``StructuredMask(causal=True)``.

    python benchmarks/bench_docs.py                     # T = 25000: N = 1, and rank 3 of an emulated N = 8
    python benchmarks/bench_docs.py --regen             # a fresh doc_starts tensor (and description) every step
    python benchmarks/bench_docs.py --T 8192 --docs 4 --rounds 5

Forward + backward of ``DistributedDotProductAttn(768, num_heads=8, impl='flash')`` in bf16: one
module, the two masks taking turns round by round in one process; every timed window is
``--inner`` steps between two HIP events.  One JSON line per shape with both medians, their
min / max over the rounds and the ratio.  The documents are ``--docs`` equal ones over T, given as
a device tensor.  Without ``--regen`` both descriptions are built once, so after the first step
their packed masks come from the mask cache; with it the document side builds
``doc_starts`` (a device op, no host sync) and a new ``StructuredMask`` every step, as a packing
data loader does, so every step pays one ``mask_gen`` call (the causal side stays cached).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def window(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=25000)
    ap.add_argument("--world", default="1,8", help="comma-separated N: 1 runs R = T, N > 1 rank --rank of an emulated "
                                                   "N-rank job (R = T / N)")
    ap.add_argument("--rank", type=int, default=3)
    ap.add_argument("--docs", type=int, default=8)
    ap.add_argument("--regen", action="store_true")
    ap.add_argument("--C", type=int, default=768)
    ap.add_argument("--H", type=int, default=8)
    ap.add_argument("--inner", type=int, default=4, help="steps per timed window")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_docs.py needs a GPU"
    import xdot
    from xdot.utils.comm import EmulatedComm

    dev = torch.device("cuda", 0)
    T, C, H = a.T, a.C, a.H

    def starts():
        return (torch.arange(a.docs, device=dev, dtype=torch.int64) * T) // a.docs

    causal = xdot.StructuredMask(causal=True)
    fixed = xdot.StructuredMask(causal=True, doc_starts=starts())
    for n in [int(x) for x in a.world.split(",")]:
        R = T // n
        rank = min(a.rank, n - 1)
        kw = {} if n == 1 else {"comm": EmulatedComm(n, rank=rank)}
        torch.manual_seed(0)
        m = xdot.DistributedDotProductAttn(C, num_heads=H, impl="flash", **kw).to(dev, torch.bfloat16)
        x = torch.randn(1, R, C, device=dev, dtype=torch.bfloat16).requires_grad_(True)

        def step(mask):
            m.zero_grad(set_to_none=True)
            x.grad = None
            m(x, x, x, mask).float().pow(2).mean().backward()

        runs = {"causal": lambda: step(causal),
                "docs": (lambda: step(xdot.StructuredMask(causal=True, doc_starts=starts()))) if a.regen
                else (lambda: step(fixed))}
        ts = {k: [] for k in runs}
        for r in range(a.warmup + a.rounds):
            for k, fn in runs.items():
                t = window(fn, a.inner)
                if r >= a.warmup:
                    ts[k].append(t)
        med = {k: statistics.median(v) for k, v in ts.items()}
        print(json.dumps({"op": "module_step", "N": n, "rank": rank, "R": R, "T": R * n, "C": C, "H": H, "dtype": "bf16",
                          "docs": a.docs, "regen": a.regen, "causal_ms": round(med["causal"], 4),
                          "docs_ms": round(med["docs"], 4),
                          "causal_min_max": [round(min(ts["causal"]), 4), round(max(ts["causal"]), 4)],
                          "docs_min_max": [round(min(ts["docs"]), 4), round(max(ts["docs"]), 4)],
                          "ratio": round(med["docs"] / med["causal"], 4)}), flush=True)


if __name__ == "__main__":
    main()
