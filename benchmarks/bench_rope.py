"""Cost of rotary position embedding (``xdot.Rotary``): the ``rope_apply`` kernel against a copy
of the same bytes, and the module step with ``rope=Rotary()`` against ``rope=None``.

    python benchmarks/bench_rope.py                    # R = 25000 (N = 1) and R = 3125 (an N = 8 rank)
    python benchmarks/bench_rope.py --rows 4096 --rounds 5

Kernel part, bf16, C = 768, H = 8: ``rope_q`` rotates the q half of a packed ``[q | v]`` buffer
``(1, R, 2C)`` in place, ``rope_k`` rotates a contiguous ``(1, R, C)`` into another tensor.  The
yardstick of each, measured in the same process and alternating with it, is
``torch.Tensor.copy_`` of the same number of bytes between two tensors of the same strides.
Every timed window is ``--inner`` back-to-back calls between two HIP events (one call is tens of
microseconds); reported per call: median and min over ``--rounds`` windows after ``--warmup``
windows, and GB/s over the bytes the operation must move (x read + written; the rope rows add
the table, ``2 * R * D/2 * 4`` bytes, listed as ``table_B``).

Step part: forward + backward of ``DistributedDotProductAttn(768, num_heads=8, impl='flash')`` in
bf16 under a causal ``StructuredMask``, at N = 1 (R = T) and as rank 3 of an emulated 8-rank job
(``EmulatedComm``, as ``benchmarks/bench_rank.py``), ``rope=None`` and ``rope=Rotary()``
alternating round by round; one JSON line with both medians and their ratio.
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


def alternate(fns, inner, rounds, warmup):
    """{name: per-call ms of every round}, the candidates taking turns inside each round."""
    ts = {k: [] for k in fns}
    for r in range(warmup + rounds):
        for k, fn in fns.items():
            t = window(fn, inner)
            if r >= warmup:
                ts[k].append(t)
    return ts


def kernels(a, dev):
    import xdot
    from xdot.ops.rope import rope_apply

    C, H = a.C, a.H
    rot = xdot.Rotary()
    for R in a.rows:
        g = torch.Generator(device=dev).manual_seed(0)
        qv = torch.randn(1, R, 2 * C, device=dev, dtype=torch.bfloat16, generator=g)
        qv2 = torch.empty_like(qv)
        k = torch.randn(1, R, C, device=dev, dtype=torch.bfloat16, generator=g)
        k2 = torch.empty_like(k)
        cos, sin = rot.table(R, C // H, 0, dev)
        q, q2 = qv[..., :C], qv2[..., :C]
        fns = {
            "rope_q": lambda: rope_apply(q, H, cos, sin, out=q),
            "copy_q": lambda: q2.copy_(q),
            "rope_k": lambda: rope_apply(k, H, cos, sin, out=k2),
            "copy_k": lambda: k2.copy_(k),
        }
        ts = alternate(fns, a.inner, a.rounds, a.warmup)
        nbytes = 2 * R * C * 2
        med = {n: statistics.median(t) for n, t in ts.items()}
        for n, t in ts.items():
            row = {"op": n, "R": R, "C": C, "H": H, "dtype": "bf16", "ms": round(med[n], 5), "min_ms": round(min(t), 5),
                   "max_ms": round(max(t), 5), "moved_B": nbytes, "GB_s": round(nbytes / med[n] / 1e6, 1)}
            if n.startswith("rope"):
                row["table_B"] = 2 * R * (C // H // 2) * 4
                row["vs_copy"] = round(med["copy" + n[4:]] / med[n], 3)  # > 1: faster than the copy
            print(json.dumps(row), flush=True)


def steps(a, dev):
    import xdot
    from xdot.utils.comm import EmulatedComm

    C, H = a.C, a.H
    spec = xdot.StructuredMask(causal=True)
    for R, comm, tag in [(a.rows[0], None, "N=1")] + [(r, EmulatedComm(8, rank=3), "N=8 rank 3 (emulated)")
                                                       for r in a.rows[1:]]:
        runs = {}
        for name, rope in (("none", None), ("rope", xdot.Rotary())):
            torch.manual_seed(0)
            kw = {} if comm is None else {"comm": comm}
            m = xdot.DistributedDotProductAttn(C, num_heads=H, impl="flash", rope=rope, **kw).to(dev, torch.bfloat16)
            x = torch.randn(1, R, C, device=dev, dtype=torch.bfloat16).requires_grad_(True)

            def step(m=m, x=x):
                m.zero_grad(set_to_none=True)
                x.grad = None
                m(x, x, x, spec).float().pow(2).mean().backward()

            runs[name] = step
        ts = alternate(runs, a.step_inner, a.rounds, a.warmup)
        med = {n: statistics.median(t) for n, t in ts.items()}
        print(json.dumps({"op": "module_step", "shape": tag, "R": R, "C": C, "H": H, "mask": "causal", "dtype": "bf16",
                          "none_ms": round(med["none"], 4), "rope_ms": round(med["rope"], 4),
                          "none_min_max": [round(min(ts["none"]), 4), round(max(ts["none"]), 4)],
                          "rope_min_max": [round(min(ts["rope"]), 4), round(max(ts["rope"]), 4)],
                          "ratio": round(med["rope"] / med["none"], 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="25000,3125", help="comma-separated R; the first is the N = 1 step, the rest "
                                                         "are emulated N = 8 ranks")
    ap.add_argument("--C", type=int, default=768)
    ap.add_argument("--H", type=int, default=8)
    ap.add_argument("--inner", type=int, default=50, help="kernel calls per timed window")
    ap.add_argument("--step-inner", type=int, default=4, help="module steps per timed window")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-steps", action="store_true")
    a = ap.parse_args()
    a.rows = [int(r) for r in a.rows.split(",")]
    assert torch.cuda.is_available(), "bench_rope.py needs a GPU"
    dev = torch.device("cuda", 0)
    kernels(a, dev)
    if not a.skip_steps:
        steps(a, dev)


if __name__ == "__main__":
    main()
