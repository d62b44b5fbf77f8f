"""Row layouts under a causal mask: per-rank module-step times, ``layout="contiguous"`` against
``layout="zigzag"``.

    python benchmarks/bench_zigzag.py                    # N = 8 and N = 4, every rank, and N = 1
    python benchmarks/bench_zigzag.py --ranks 8 --md out.md

bf16, H = 8, D = 96, T = 25000, a causal ``StructuredMask``: forward + backward of
``DistributedDotProductAttn(768, num_heads=8, impl='flash', layout=...)`` for EVERY rank ``r`` of an
emulated ``N``-rank job (``EmulatedComm(N, r)``: the collectives are device copies of the right
shapes, NOT a transport -- this is per-rank COMPUTE on one GPU, no multi-GPU time can be measured
here).  A real step waits for its slowest rank at every collective, so the figure to compare between
the layouts is the MAXIMUM over ranks.  The two layouts and all ranks take turns inside every round
(one process, same clocks and neighbours); a timed window is ``--inner`` back-to-back steps between
two HIP events, reported per step as the median over ``--rounds`` windows after ``--warmup`` windows.

The N = 1 step runs under both layouts too: a world of one is the identity, so they must be the
same launches and the same time up to noise.

Each row also carries the rank's live share of the (64-row x 64-column) score tiles of its causal
mask, counted from the layout's indices: arithmetic, not a measurement.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, D = 8, 96
LAYOUTS = ("contiguous", "zigzag")


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


def live_share(layout, rank, n, R):
    """Share of the rank's 64 x 64 score tiles that a causal mask leaves some element of."""
    from xdot.parallel.layout import gathered_cols, global_rows

    rows, cols = global_rows(layout, rank, n, R), gathered_cols(layout, n, R)
    nrt, nct = -(-R // 64), -(-(n * R) // 64)
    pad = lambda v, k, fill: torch.cat([v, v.new_full((k * 64 - v.numel(),), fill)]).view(k, 64)  # noqa: E731
    rmax = pad(rows, nrt, -1).max(dim=1).values        # a tile is live if its smallest column
    cmin = pad(cols, nct, 2**62).min(dim=1).values     # is <= its largest row
    return float((cmin.view(1, -1) <= rmax.view(-1, 1)).float().mean())


def steps(n, T, dev):
    """{(layout, rank): step closure} of every rank of an emulated n-rank job (n = 1: LocalComm)."""
    import xdot
    from xdot.utils.comm import EmulatedComm, LocalComm

    spec = xdot.StructuredMask(causal=True)
    R = T // n
    out = {}
    for rank in range(n):
        for layout in LAYOUTS:
            comm = LocalComm() if n == 1 else EmulatedComm(n, rank=rank)
            torch.manual_seed(0)
            m = xdot.DistributedDotProductAttn(H * D, num_heads=H, impl="flash", comm=comm, layout=layout).to(dev, torch.bfloat16)
            x = torch.randn(1, R, H * D, device=dev, dtype=torch.bfloat16).requires_grad_(True)

            def step(m=m, x=x):
                m.zero_grad(set_to_none=True)
                x.grad = None
                m(x, x, x, spec).float().pow(2).mean().backward()

            out[(layout, rank)] = step
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--T", type=int, default=25000)
    ap.add_argument("--ranks", default="8,4,1", help="world sizes to emulate (T a multiple of each)")
    ap.add_argument("--inner", type=int, default=3, help="module steps per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--md", default=None, help="also write the tables as markdown to this file")
    a = ap.parse_args()
    worlds = [int(v) for v in a.ranks.split(",")]
    assert all(a.T % n == 0 for n in worlds)
    assert torch.cuda.is_available(), "bench_zigzag.py needs a GPU"
    dev = torch.device("cuda", 0)
    md = []
    for n in worlds:
        R = a.T // n
        ts = alternate(steps(n, a.T, dev), a.inner, a.rounds, a.warmup)
        med = {k: statistics.median(v) for k, v in ts.items()}
        for (layout, rank), t in ts.items():
            print(json.dumps({"op": "module_step", "N": n, "rank": rank, "layout": layout, "R": R, "T": a.T, "H": H, "D": D,
                              "mask": "causal", "dtype": "bf16", "emulated": n > 1, "ms": round(med[(layout, rank)], 4),
                              "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                              "live_tiles": round(live_share(layout, rank, n, R), 4)}), flush=True)
        worst = {l: max(med[(l, r)] for r in range(n)) for l in LAYOUTS}
        print(json.dumps({"summary": f"N={n}", "max_over_ranks_ms": {l: round(v, 4) for l, v in worst.items()},
                          "zigzag_over_contiguous": round(worst["zigzag"] / worst["contiguous"], 4)}), flush=True)
        md.append(f"### N = {n} (R = {R}{', emulated per-rank compute' if n > 1 else ''})\n")
        md.append("| rank | contiguous ms | live tiles | zigzag ms | live tiles |")
        md.append("|---:|---:|---:|---:|---:|")
        for r in range(n):
            md.append(f"| {r} | {med[('contiguous', r)]:.3f} | {live_share('contiguous', r, n, R):.3f} | "
                      f"{med[('zigzag', r)]:.3f} | {live_share('zigzag', r, n, R):.3f} |")
        md.append(f"| **max** | **{worst['contiguous']:.3f}** | | **{worst['zigzag']:.3f}** | |\n")
    if a.md:
        with open(a.md, "w") as f:
            f.write("\n".join(md) + "\n")


if __name__ == "__main__":
    main()
