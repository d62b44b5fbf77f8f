"""Chunked-prefill A/B on one GPU: ``flash.extend`` (csrc/flash_extend.hip) against the route the same call
had before it, ``flash.fwd`` over a packed dense mask, with the mask's build + pack timed on its own.

One process, the variants alternating inside every repetition, device-event timings, warmed median with
the 10th / 90th percentiles.  Before timing, the two routes' outputs at the timed size are compared within
the forward test bounds.  bf16, B = 1, H = 8, D = 96 over a full in-order cache; per (Tcap, Hg): a row count
just above the decode kernel's 64 packed rows (G * Rn = 72), Rn = 1024, and Rn = 1024 under a window of 4096
positions, where all but ~160 of the cache's tiles are skipped.  ``extend_wins``: the kernel's p10 is below
the forward kernel's p90 (mask already packed); a shape class where it is not is routed away in
``flash.extend_eligible``.  One JSON line per case.

    python benchmarks/bench_extend.py [--reps 20] [--warmup 5]
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchmarks.bench_decode import _stats, _timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--extra-rows", default="", help="more unwindowed row counts, comma separated")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_extend: needs a GPU")
    from xdot import _ext
    from xdot.ops import flash
    from xdot.parallel._ref import decode_mask

    dev, dt, B, H, D = torch.device("cuda", 0), torch.bfloat16, 1, 8, 96
    scale = 1.0 / math.sqrt(D)
    print(json.dumps({"device": torch.cuda.get_device_name(dev), "dtype": "bf16", "B": B, "H": H, "D": D,
                      "reps": a.reps, "warmup": a.warmup}), flush=True)
    for Tcap in (25000, 200000):
        for Hg in (8, 2):
            G = H // Hg
            for Rn, window in [(72 // G, 0), (1024, 0), (1024, 4096)] + [(int(r), 0) for r in a.extra_rows.split(",") if r]:
                g = torch.Generator().manual_seed(Tcap + Hg + Rn)
                rows = torch.randn(B, Rn, H * D, generator=g).to(dev, dt)
                qv = torch.randn(B, Tcap, 2 * Hg * D, generator=g).to(dev, dt)
                qc, vc = qv[..., :Hg * D], qv[..., Hg * D:]
                pos = torch.arange(Tcap, dtype=torch.int32, device=dev).repeat(B, 1)  # a full cache, in order
                pos0 = Tcap - Rn

                def pack():
                    return flash.prepare_mask(decode_mask(pos, pos0, Rn, window), B, Rn, Tcap)

                mk = pack()
                # the op itself: flash.extend refuses the shapes this table made extend_eligible route away
                fns = {"extend": lambda: _ext.ops().flash_extend(rows, qc, vc, pos, pos0, window, H, scale, Hg),
                       "fwd": lambda: flash.fwd(rows, qc, vc, mk, H, scale, Hg=Hg if Hg != H else None),
                       "mask_pack": pack}
                (o1, l1), (o2, l2) = fns["extend"](), fns["fwd"]()
                fro = ((o1.float() - o2.float()).norm() / o2.float().norm()).item()
                dl = (l1 - l2).abs().max().item()
                assert fro <= 1e-2 and dl < 1e-2, f"routes disagree at Tcap={Tcap} Hg={Hg} Rn={Rn} window={window}: {fro:.3e}, {dl:.3e}"
                t = {k: _stats(v) for k, v in _timed(fns, a.reps, a.warmup).items()}
                print(json.dumps({
                    "Tcap": Tcap, "Hg": Hg, "Rn": Rn, "window": window, "spans": flash.extend_plan(B, Hg, G, Rn, D, Tcap),
                    "routes_rel_fro": round(fro, 6), "routes_lse_diff": round(dl, 6), **t,
                    "speedup_vs_fwd": round(t["fwd"]["median_ms"] / t["extend"]["median_ms"], 2),
                    "speedup_vs_fwd_and_pack": round((t["fwd"]["median_ms"] + t["mask_pack"]["median_ms"]) / t["extend"]["median_ms"], 2),
                    "extend_wins": t["extend"]["p10_ms"] < t["fwd"]["p90_ms"],
                    "eligible": flash.extend_eligible(dt, D, D, G, Rn)}), flush=True)
                del mk


if __name__ == "__main__":
    main()
