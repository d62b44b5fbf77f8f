"""Cost of QK-norm (``qk_norm=True``): the fused norm + rotation kernels of ``csrc/headnorm.hip``
against a copy of the same bytes and against ``rope_apply`` alone, and the module step with
``rope`` only against ``rope`` + ``qk_norm``.

    python benchmarks/bench_qknorm.py                    # R = 25000 (N = 1) and R = 3125 (an N = 8 rank)
    python benchmarks/bench_qknorm.py --rows 4096 --rounds 5

Kernel part, bf16, C = 768, H = 8, as ``benchmarks/bench_rope.py``: the ``_q`` rows work in place
on the q half of a packed ``[q | v]`` buffer ``(1, R, 2C)``, the ``_k`` rows on a contiguous
``(1, R, C)``.  ``norm_fwd_*`` is the forward the module runs when a backward can follow: norm +
rotation in place, plus ``rstd`` and the bit copy of the input (``moved_B`` counts x read, out
written and the copy written); ``norm_fwd_nosave_*`` the same without the copy; ``norm_bwd_*`` the
backward pass in place on the gradient with its ordered ``dw`` sum (g read, x read, dx written:
two launches).  Yardsticks, measured in the same process and alternating with them:
``torch.Tensor.copy_`` between two tensors of the same strides (``copy_*``: one read and one write of
the operand) and ``rope_apply`` in place (``rope_*``).  Every timed window is ``--inner``
back-to-back calls between two HIP events; reported per call: median, min and max over ``--rounds``
windows after ``--warmup`` windows, GB/s over ``moved_B``, and ``vs_copy`` = the time of as many
copies as the operation moves operand-sized streams, divided by its own time (> 1: faster than
copying those bytes).

Step part: forward + backward of ``DistributedDotProductAttn(768, num_heads=8, impl='flash',
rope=Rotary())`` in bf16 under a causal ``StructuredMask``, at N = 1 (R = T) and as rank 3 of an
emulated 8-rank job (``EmulatedComm``), ``qk_norm=False`` and ``qk_norm=True`` alternating round by
round; one JSON line with both medians and their ratio.
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
    from xdot.ops.headnorm import head_rms_norm_apply, head_rms_norm_backward
    from xdot.ops.rope import rope_apply

    C, H, eps = a.C, a.H, 1e-6
    rot = xdot.Rotary()
    for R in a.rows:
        g = torch.Generator(device=dev).manual_seed(0)
        qv = torch.randn(1, R, 2 * C, device=dev, dtype=torch.bfloat16, generator=g)
        qv2 = torch.empty_like(qv)
        gqv = torch.randn(1, R, 2 * C, device=dev, dtype=torch.bfloat16, generator=g)
        k = torch.randn(1, R, C, device=dev, dtype=torch.bfloat16, generator=g)
        k2 = torch.empty_like(k)
        gk = torch.randn(1, R, C, device=dev, dtype=torch.bfloat16, generator=g)
        # (a gain of ones: the in-place calls feed on their own output window after window, and any
        # other gain would compound into overflow; the kernels' time does not depend on the values)
        w = torch.ones(C // H, device=dev, dtype=torch.bfloat16)
        cos, sin = rot.table(R, C // H, 0, dev)
        q, q2, gq = qv[..., :C], qv2[..., :C], gqv[..., :C]
        # the backward's inputs: a pre-norm copy and rstd of values that stay put (the timed forward
        # calls overwrite q and k again and again, which only changes what the kernels read)
        _, rq, xq = head_rms_norm_apply(q.clone(), H, w, eps, cos, sin, save=True)
        _, rk, xk = head_rms_norm_apply(k.clone(), H, w, eps, cos, sin, save=True)
        fns = {
            "norm_fwd_q": lambda: head_rms_norm_apply(q, H, w, eps, cos, sin, out=q, save=True),
            "norm_fwd_nosave_q": lambda: head_rms_norm_apply(q, H, w, eps, cos, sin, out=q),
            "norm_bwd_q": lambda: head_rms_norm_backward(gq, xq, rq, H, w, cos, sin, out=gq),
            "rope_q": lambda: rope_apply(q, H, cos, sin, out=q),
            "copy_q": lambda: q2.copy_(q),
            "norm_fwd_k": lambda: head_rms_norm_apply(k, H, w, eps, cos, sin, out=k, save=True),
            "norm_fwd_nosave_k": lambda: head_rms_norm_apply(k, H, w, eps, cos, sin, out=k),
            "norm_bwd_k": lambda: head_rms_norm_backward(gk, xk, rk, H, w, cos, sin, out=gk),
            "rope_k": lambda: rope_apply(k, H, cos, sin, out=k),
            "copy_k": lambda: k2.copy_(k),
        }
        ts = alternate(fns, a.inner, a.rounds, a.warmup)
        one = R * C * 2  # one operand-sized stream
        streams = {"norm_fwd": 3, "norm_fwd_nosave": 2, "norm_bwd": 3, "rope": 2, "copy": 2}
        med = {n: statistics.median(t) for n, t in ts.items()}
        for n, t in ts.items():
            kind, side = n.rsplit("_", 1)
            nbytes = streams[kind] * one
            row = {"op": n, "R": R, "C": C, "H": H, "dtype": "bf16", "ms": round(med[n], 5), "min_ms": round(min(t), 5),
                   "max_ms": round(max(t), 5), "moved_B": nbytes, "GB_s": round(nbytes / med[n] / 1e6, 1)}
            if kind != "copy":
                row["table_B"] = 2 * R * (C // H // 2) * 4
                row["vs_copy"] = round(med["copy_" + side] * streams[kind] / 2 / med[n], 3)
                row["vs_rope"] = round(med[n] / med["rope_" + side], 3)  # times the rotation alone
            print(json.dumps(row), flush=True)


def steps(a, dev):
    import xdot
    from xdot.utils.comm import EmulatedComm

    C, H = a.C, a.H
    spec = xdot.StructuredMask(causal=True)
    for R, comm, tag in [(a.rows[0], None, "N=1")] + [(r, EmulatedComm(8, rank=3), "N=8 rank 3 (emulated)")
                                                       for r in a.rows[1:]]:
        runs = {}
        for name, norm in (("rope", False), ("rope_norm", True)):
            torch.manual_seed(0)
            kw = {} if comm is None else {"comm": comm}
            m = xdot.DistributedDotProductAttn(C, num_heads=H, impl="flash", rope=xdot.Rotary(), qk_norm=norm,
                                               **kw).to(dev, torch.bfloat16)
            x = torch.randn(1, R, C, device=dev, dtype=torch.bfloat16).requires_grad_(True)

            def step(m=m, x=x):
                m.zero_grad(set_to_none=True)
                x.grad = None
                m(x, x, x, spec).float().pow(2).mean().backward()

            runs[name] = step
        ts = alternate(runs, a.step_inner, a.rounds, a.warmup)
        med = {n: statistics.median(t) for n, t in ts.items()}
        print(json.dumps({"op": "module_step", "shape": tag, "R": R, "C": C, "H": H, "mask": "causal", "dtype": "bf16",
                          "rope_ms": round(med["rope"], 4), "rope_norm_ms": round(med["rope_norm"], 4),
                          "rope_min_max": [round(min(ts["rope"]), 4), round(max(ts["rope"]), 4)],
                          "rope_norm_min_max": [round(min(ts["rope_norm"]), 4), round(max(ts["rope_norm"]), 4)],
                          "ratio": round(med["rope_norm"] / med["rope"], 4)}), flush=True)


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
    assert torch.cuda.is_available(), "bench_qknorm.py needs a GPU"
    dev = torch.device("cuda", 0)
    kernels(a, dev)
    if not a.skip_steps:
        steps(a, dev)


if __name__ == "__main__":
    main()
