"""Cost of attention sinks (``sinks=True``): the two kernels of ``csrc/sink.hip`` against a copy of
the same bytes, and the module step with and without sinks.

    python benchmarks/bench_sinks.py                    # R = 25000 (N = 1) and R = 3125 (an N = 8 rank)
    python benchmarks/bench_sinks.py --rows 4096 --rounds 5

Kernel part, bf16, C = 768, H = 8: ``sink_fold`` works in place on a contiguous ``out`` ``(1, R, C)``
and its ``lse`` ``(1, H, R)`` (``moved_B``: out read and written, lse read and written);
``sink_grad`` reads ``delta`` and ``lse`` ``(1, H, R)`` fp32 (two launches: partials, ordered sum).
Yardsticks, measured in the same process and alternating with them: ``torch.Tensor.copy_`` between
two tensors shaped like ``out`` (``copy_out``: the fold's bytes but for lse) and like ``[delta | lse]``
(``copy_dl``: ``sink_grad``'s bytes read AND written, twice what it moves), and ``rope_apply`` in
place on the same ``out`` (``rope_out``).  Every timed window is ``--inner`` back-to-back calls
between two HIP events; reported per call: median, min and max over ``--rounds`` windows after
``--warmup`` windows, GB/s over ``moved_B``, and ``vs_copy`` = the copy's time scaled to the
operation's bytes, divided by its own time (> 1: faster than copying those bytes).  The in-place
fold feeds on its own output call after call (``lse`` only grows, the gate tends to 1): that changes
the values the kernel reads, not its time.

Step part: forward + backward of ``DistributedDotProductAttn(768, num_heads=8, impl='flash')`` in
bf16 under a causal ``StructuredMask`` with ``window`` (default 4096), at N = 1 (R = T) and as rank
3 of an emulated 8-rank job (``EmulatedComm``: one GPU runs the rank's compute, no transport),
``sinks=False`` and ``sinks=True`` alternating round by round; one JSON line with both medians and
their ratio.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_rope import alternate  # noqa: E402


def kernels(a, dev):
    import xdot
    from xdot.ops import flash
    from xdot.ops.rope import rope_apply

    C, H = a.C, a.H
    rot = xdot.Rotary()
    for R in a.rows:
        g = torch.Generator(device=dev).manual_seed(0)
        out = torch.randn(1, R, C, device=dev, dtype=torch.bfloat16, generator=g)
        out2 = torch.empty_like(out)
        lse = 9.0 + torch.randn(1, H, R, device=dev, generator=g)
        delta = torch.randn(1, H, R, device=dev, generator=g)
        sinks = torch.rand(H, device=dev, generator=g) * 2 - 1
        dl, dl2 = torch.cat([delta, lse]), torch.empty(2, H, R, device=dev)
        cos, sin = rot.table(R, C // H, 0, dev)
        fns = {
            "sink_fold": lambda: flash.sink_fold(out, lse, sinks, H),
            "sink_grad": lambda: flash.sink_grad(delta, lse, sinks),
            "rope_out": lambda: rope_apply(out, H, cos, sin, out=out),
            "copy_out": lambda: out2.copy_(out),
            "copy_dl": lambda: dl2.copy_(dl),
        }
        ts = alternate(fns, a.inner, a.rounds, a.warmup)
        med = {n: statistics.median(t) for n, t in ts.items()}
        ob, lb = R * C * 2, R * H * 4
        moved = {"sink_fold": 2 * ob + 2 * lb, "sink_grad": 2 * lb, "rope_out": 2 * ob, "copy_out": 2 * ob, "copy_dl": 4 * lb}
        yard = {"sink_fold": "copy_out", "sink_grad": "copy_dl", "rope_out": "copy_out"}
        for n, t in ts.items():
            row = {"op": n, "R": R, "C": C, "H": H, "dtype": "bf16", "ms": round(med[n], 5), "min_ms": round(min(t), 5),
                   "max_ms": round(max(t), 5), "moved_B": moved[n], "GB_s": round(moved[n] / med[n] / 1e6, 1)}
            if n in yard:
                row["vs_copy"] = round(med[yard[n]] * moved[n] / moved[yard[n]] / med[n], 3)
            if n == "sink_fold":
                row["vs_rope"] = round(med[n] / med["rope_out"], 3)
            print(json.dumps(row), flush=True)


def steps(a, dev):
    import xdot
    from xdot.utils.comm import EmulatedComm

    C, H = a.C, a.H
    spec = xdot.StructuredMask(causal=True, window=a.window)
    for R, comm, tag in [(a.rows[0], None, "N=1")] + [(r, EmulatedComm(8, rank=3), "N=8 rank 3 (emulated)")
                                                       for r in a.rows[1:]]:
        runs = {}
        for name, sinks in (("plain", False), ("sinks", True)):
            torch.manual_seed(0)
            kw = {} if comm is None else {"comm": comm}
            m = xdot.DistributedDotProductAttn(C, num_heads=H, impl="flash", sinks=sinks, **kw).to(dev, torch.bfloat16)
            x = torch.randn(1, R, C, device=dev, dtype=torch.bfloat16).requires_grad_(True)

            def step(m=m, x=x):
                m.zero_grad(set_to_none=True)
                x.grad = None
                m(x, x, x, spec).float().pow(2).mean().backward()

            runs[name] = step
        ts = alternate(runs, a.step_inner, a.rounds, a.warmup)
        med = {n: statistics.median(t) for n, t in ts.items()}
        print(json.dumps({"op": "module_step", "shape": tag, "R": R, "C": C, "H": H, "mask": f"causal, window {a.window}",
                          "dtype": "bf16", "plain_ms": round(med["plain"], 4), "sinks_ms": round(med["sinks"], 4),
                          "plain_min_max": [round(min(ts["plain"]), 4), round(max(ts["plain"]), 4)],
                          "sinks_min_max": [round(min(ts["sinks"]), 4), round(max(ts["sinks"]), 4)],
                          "ratio": round(med["sinks"] / med["plain"], 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="25000,3125", help="comma-separated R; the first is the N = 1 step, the rest "
                                                         "are emulated N = 8 ranks")
    ap.add_argument("--C", type=int, default=768)
    ap.add_argument("--H", type=int, default=8)
    ap.add_argument("--window", type=int, default=4096, help="sliding window of the step's causal mask")
    ap.add_argument("--inner", type=int, default=50, help="kernel calls per timed window")
    ap.add_argument("--step-inner", type=int, default=4, help="module steps per timed window")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-steps", action="store_true")
    a = ap.parse_args()
    a.rows = [int(r) for r in a.rows.split(",")]
    assert torch.cuda.is_available(), "bench_sinks.py needs a GPU"
    dev = torch.device("cuda", 0)
    kernels(a, dev)
    if not a.skip_steps:
        steps(a, dev)


if __name__ == "__main__":
    main()
