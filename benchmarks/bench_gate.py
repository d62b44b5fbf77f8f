"""Cost of gated attention (``gate='elementwise' | 'headwise'``): the two kernels of ``csrc/gate.hip``
against a copy of the same bytes, ``sink_fold`` and ``rope_apply`` on the same tensor, and the module
step with each gate kind against ``gate=None``.

    python benchmarks/bench_gate.py                    # R = 25000 (N = 1) and R = 3125 (an N = 8 rank)
    python benchmarks/bench_gate.py --rows 4096 --rounds 5

Kernel part, bf16, C = 768, H = 8, contiguous tensors: ``gate_apply`` reads ``o`` and ``g`` and writes
``o'`` (``moved_B``: three tensors elementwise; two and the small ``(1, R, H)`` gate headwise);
``gate_backward`` reads ``do'``, ``o`` and ``g`` and writes ``do`` (in place over ``do'``, as the fused
node calls it) and ``dg`` (five tensors elementwise; three and two small ones headwise).  Yardsticks,
measured in the same process and alternating with them: ``torch.Tensor.copy_`` between two tensors
shaped like ``o`` (``copy_out``), ``sink_fold`` in place on the same ``o`` with its ``lse``
(``sink_fold``) and ``rope_apply`` in place on it (``rope_out``).  Every timed window is ``--inner``
back-to-back calls between two HIP events; reported per call: median, min and max over ``--rounds``
windows after ``--warmup`` windows, GB/s over ``moved_B``, ``vs_copy`` = the copy's time scaled to the
operation's bytes, divided by its own time (> 1: faster than copying those bytes), and ``vs_sink`` =
its GB/s over ``sink_fold``'s (the target: >= 1 for ``gate_apply``).  The in-place calls feed on
their own output call after call: that changes the values read, not the time.

Step part: forward + backward of ``DistributedDotProductAttn(768, num_heads=8, impl='flash')`` in
bf16 under a causal ``StructuredMask``, at N = 1 (R = T) and as rank 3 of an emulated 8-rank job
(``EmulatedComm``: one GPU runs the rank's compute, no transport), ``gate=None`` -- the step as it was
before the keyword existed, launch for launch: the baseline -- and the two gate kinds alternating
round by round; one JSON line with the three medians and the two ratios.
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
    from xdot.ops.gate import gate_apply, gate_backward
    from xdot.ops.rope import rope_apply

    C, H = a.C, a.H
    rot = xdot.Rotary()
    for R in a.rows:
        gen = torch.Generator(device=dev).manual_seed(0)
        rnd = lambda *s: torch.randn(*s, device=dev, dtype=torch.bfloat16, generator=gen)
        o, dy, ge, gh = rnd(1, R, C), rnd(1, R, C), rnd(1, R, C), rnd(1, R, H)
        y, o2 = torch.empty_like(o), torch.empty_like(o)
        fold = o.clone()
        lse = 9.0 + torch.randn(1, H, R, device=dev, generator=gen)
        sinks = torch.rand(H, device=dev, generator=gen) * 2 - 1
        cos, sin = rot.table(R, C // H, 0, dev)
        fns = {
            "gate_apply_elementwise": lambda: gate_apply(o, ge, H, out=y),
            "gate_apply_headwise": lambda: gate_apply(o, gh, H, out=y),
            "gate_backward_elementwise": lambda: gate_backward(dy, o, ge, H, out=dy),
            "gate_backward_headwise": lambda: gate_backward(dy, o, gh, H, out=dy),
            "sink_fold": lambda: flash.sink_fold(fold, lse, sinks, H),
            "rope_out": lambda: rope_apply(fold, H, cos, sin, out=fold),
            "copy_out": lambda: o2.copy_(o),
        }
        ts = alternate(fns, a.inner, a.rounds, a.warmup)
        med = {n: statistics.median(t) for n, t in ts.items()}
        ob, hb, lb = R * C * 2, R * H * 2, R * H * 4
        moved = {"gate_apply_elementwise": 3 * ob, "gate_apply_headwise": 2 * ob + hb,
                 "gate_backward_elementwise": 5 * ob, "gate_backward_headwise": 3 * ob + 2 * hb,
                 "sink_fold": 2 * ob + 2 * lb, "rope_out": 2 * ob, "copy_out": 2 * ob}
        gbs = {n: moved[n] / med[n] / 1e6 for n in ts}
        for n, t in ts.items():
            row = {"op": n, "R": R, "C": C, "H": H, "dtype": "bf16", "ms": round(med[n], 5), "min_ms": round(min(t), 5),
                   "max_ms": round(max(t), 5), "moved_B": moved[n], "GB_s": round(gbs[n], 1)}
            if n != "copy_out":
                row["vs_copy"] = round(med["copy_out"] * moved[n] / moved["copy_out"] / med[n], 3)
            if n.startswith("gate_"):
                row["vs_sink"] = round(gbs[n] / gbs["sink_fold"], 3)
            print(json.dumps(row), flush=True)


def steps(a, dev):
    import xdot
    from xdot.utils.comm import EmulatedComm

    C, H = a.C, a.H
    spec = xdot.StructuredMask(causal=True)
    for R, comm, tag in [(a.rows[0], None, "N=1")] + [(r, EmulatedComm(8, rank=3), "N=8 rank 3 (emulated)")
                                                       for r in a.rows[1:]]:
        runs = {}
        for name, gate in (("none", None), ("elementwise", "elementwise"), ("headwise", "headwise")):
            torch.manual_seed(0)
            kw = {} if comm is None else {"comm": comm}
            m = xdot.DistributedDotProductAttn(C, num_heads=H, impl="flash", gate=gate, **kw).to(dev, torch.bfloat16)
            x = torch.randn(1, R, C, device=dev, dtype=torch.bfloat16).requires_grad_(True)

            def step(m=m, x=x):
                m.zero_grad(set_to_none=True)
                x.grad = None
                m(x, x, x, spec).float().pow(2).mean().backward()

            runs[name] = step
        ts = alternate(runs, a.step_inner, a.rounds, a.warmup)
        med = {n: statistics.median(t) for n, t in ts.items()}
        row = {"op": "module_step", "shape": tag, "R": R, "C": C, "H": H, "mask": "causal", "dtype": "bf16"}
        for n in runs:
            row[f"{n}_ms"] = round(med[n], 4)
            row[f"{n}_min_max"] = [round(min(ts[n]), 4), round(max(ts[n]), 4)]
        row["elementwise_ratio"] = round(med["elementwise"] / med["none"], 4)
        row["headwise_ratio"] = round(med["headwise"] / med["none"], 4)
        print(json.dumps(row), flush=True)


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
    assert torch.cuda.is_available(), "bench_gate.py needs a GPU"
    dev = torch.device("cuda", 0)
    kernels(a, dev)
    if not a.skip_steps:
        steps(a, dev)


if __name__ == "__main__":
    main()
