"""Grouped-query attention (``num_gathered_heads`` = Hg < H): kernel and module-step times.

    python benchmarks/bench_gqa.py                         # Hg in {8, 2, 1}, both shapes, kernels + step
    python benchmarks/bench_gqa.py --hg 8 --skip-steps     # the Hg = H kernels only
    python benchmarks/bench_gqa.py --builds a/_C.so,b/_C.so --repeats 3
                                                           # A/B of two builds of the extension at Hg = H

Kernel part, bf16, H = 8, D = 96, no mask, pre-scaled rows (the module's default), at R = T = 25000
(N = 1) and R = 3125, T = 25000 (an N = 8 rank): the forward, the gathered-side ("column") backward
kernel with 16-bit output and the row-side backward kernel, for every ``--hg``.  The variants take
turns inside every round (one process, same clocks and neighbours); a timed window is ``--inner``
back-to-back calls between two HIP events, reported per call as median / min / max over ``--rounds``
windows after ``--warmup`` windows.

Step part: forward + backward of ``DistributedDotProductAttn(768, num_heads=8,
num_gathered_heads=Hg, impl='flash')`` in bf16 under a causal ``StructuredMask``, at N = 1 and as
rank 3 of an emulated 8-rank job (``EmulatedComm``: the collectives are device copies of the right
shapes, NOT a transport -- no multi-GPU time can be measured on one GPU), the variants alternating.

Every row also carries the gathered-side bytes of one step computed from the shapes: the
``[q | v]`` all-gather output and the ``[dq | dv]`` reduce-scatter input, ``T * 2 * Hg * D`` 16-bit
elements each (what stays resident for the backward is the former).

``--builds``: a loaded extension cannot be swapped inside a process, so each build runs the kernel
part at Hg = H in a child process of its own (``XDOT_EXT_PATH``), the builds taking turns
``--repeats`` times; the summary row gives, per kernel, every run's median, the spread between runs
of the SAME build and the difference between the builds' means.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, D = 8, 96


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


def wire_bytes(T, Hg):
    """16-bit bytes of the gathered [q | v] (= of the [dq | dv] partials) over all T rows"""
    return T * 2 * Hg * D * 2


def kernels(a, dev):
    from xdot.ops import flash

    scale = D ** -0.5
    for R, T in a.shapes:
        g = torch.Generator(device=dev).manual_seed(0)
        rows = torch.randn(1, R, H * D, device=dev, dtype=torch.bfloat16, generator=g)
        do = torch.randn(1, R, H * D, device=dev, dtype=torch.bfloat16, generator=g)
        rk = flash.prescale(rows, scale)
        fns = {}
        keep = []
        for Hg in a.hg:
            qv = torch.randn(1, T, 2 * Hg * D, device=dev, dtype=torch.bfloat16, generator=g)
            kc, vc = qv[..., :Hg * D], qv[..., Hg * D:]
            hg = None if Hg == H else Hg
            out, lse = flash.fwd(rk, kc, vc, None, H, scale, prescaled=True, Hg=hg)
            delta, lse2 = flash.bwd_prep(do, out, lse, H)
            keep.append((qv, out, lse, delta, lse2))
            fns[f"fwd/{Hg}"] = lambda kc=kc, vc=vc, hg=hg: flash.fwd(rk, kc, vc, None, H, scale, prescaled=True, Hg=hg)
            fns[f"cols/{Hg}"] = lambda kc=kc, vc=vc, hg=hg, out=out, lse=lse, delta=delta, lse2=lse2: flash.bwd_cols(
                do, rk, kc, vc, out, lse, None, H, scale, delta, fp32_out=False, prescaled=True, lse2=lse2, Hg=hg)
            fns[f"rows/{Hg}"] = lambda kc=kc, vc=vc, hg=hg, lse=lse, delta=delta: flash.bwd_rows(
                do, rk, kc, vc, lse, delta, None, H, scale, prescaled=True, Hg=hg)
        ts = alternate(fns, a.inner, a.rounds, a.warmup)
        for name, t in ts.items():
            op, Hg = name.split("/")
            print(json.dumps({"op": op, "R": R, "T": T, "H": H, "Hg": int(Hg), "D": D, "dtype": "bf16",
                              "ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                              "gathered_B": wire_bytes(T, int(Hg))}), flush=True)


def steps(a, dev):
    import xdot
    from xdot.utils.comm import EmulatedComm, LocalComm

    spec = xdot.StructuredMask(causal=True)
    for R, T in a.shapes:
        n = T // R
        comm = LocalComm() if n == 1 else EmulatedComm(n, rank=min(3, n - 1))
        runs = {}
        for Hg in a.hg:
            torch.manual_seed(0)
            m = xdot.DistributedDotProductAttn(H * D, num_heads=H, num_gathered_heads=Hg, impl="flash",
                                               comm=comm).to(dev, torch.bfloat16)
            x = torch.randn(1, R, H * D, device=dev, dtype=torch.bfloat16).requires_grad_(True)

            def step(m=m, x=x):
                m.zero_grad(set_to_none=True)
                x.grad = None
                m(x, x, x, spec).float().pow(2).mean().backward()

            runs[Hg] = step
        ts = alternate(runs, a.step_inner, a.rounds, a.warmup)
        for Hg, t in ts.items():
            print(json.dumps({"op": "module_step", "shape": "N=1" if n == 1 else f"N={n} rank {min(3, n - 1)} (emulated)",
                              "R": R, "T": T, "H": H, "Hg": Hg, "D": D, "mask": "causal", "dtype": "bf16",
                              "ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                              "allgather_B": wire_bytes(T, Hg), "reduce_scatter_B": wire_bytes(T, Hg)}), flush=True)


def builds(a):
    """The kernel part at Hg = H in a fresh child process per build, the builds taking turns."""
    paths = a.builds.split(",")
    runs = {p: [] for p in paths}  # per build: [{(op, R): ms}]
    for rep in range(a.repeats):
        for p in paths:
            env = dict(os.environ, XDOT_EXT_PATH=os.path.abspath(p))
            cmd = [sys.executable, os.path.abspath(__file__), "--hg", str(H), "--skip-steps", "--shapes", a.shapes_arg,
                   "--inner", str(a.inner), "--rounds", str(a.rounds), "--warmup", str(a.warmup)]
            r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=a.child_timeout)
            if r.returncode != 0:
                raise SystemExit(f"bench_gqa: the child for {p} failed ({r.returncode})")
            rows = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
            runs[p].append({(x["op"], x["R"]): x["ms"] for x in rows})
            print(json.dumps({"build": p, "repeat": rep, "ms": {f"{o}@R={R}": v for (o, R), v in runs[p][-1].items()}}),
                  flush=True)
    for key in runs[paths[0]][0]:
        per = {p: [r[key] for r in runs[p]] for p in paths}
        spread = max(max(v) - min(v) for v in per.values())
        means = [statistics.mean(v) for v in per.values()]
        print(json.dumps({"summary": f"{key[0]}@R={key[1]}", "runs_ms": per, "same_build_spread_ms": round(spread, 4),
                          "between_builds_ms": round(max(means) - min(means), 4),
                          "within_spread": (max(means) - min(means)) <= spread}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shapes", default="25000x25000,3125x25000", help="comma-separated RxT (T a multiple of R)")
    ap.add_argument("--hg", default="8,2,1", help="gathered heads to compare (H = 8)")
    ap.add_argument("--inner", type=int, default=5, help="kernel calls per timed window")
    ap.add_argument("--step-inner", type=int, default=3, help="module steps per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--builds", default=None, help="comma-separated extension builds to A/B at Hg = H (child processes)")
    ap.add_argument("--repeats", type=int, default=3, help="runs of every build (--builds)")
    ap.add_argument("--child-timeout", type=float, default=240.0)
    a = ap.parse_args()
    a.shapes_arg = a.shapes
    a.shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    a.hg = [int(v) for v in a.hg.split(",")]
    assert all(T % R == 0 for R, T in a.shapes) and all(H % g == 0 for g in a.hg)
    if a.builds:
        return builds(a)
    assert torch.cuda.is_available(), "bench_gqa.py needs a GPU"
    dev = torch.device("cuda", 0)
    if not a.skip_kernels:
        kernels(a, dev)
    if not a.skip_steps:
        steps(a, dev)


if __name__ == "__main__":
    main()
