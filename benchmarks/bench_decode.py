"""Decode A/B on one GPU: ``flash.decode`` (csrc/flash_decode.hip) against the route the same call had
before it, ``flash.fwd`` over a packed dense mask, with the mask's build + pack timed on its own.

One process, the variants alternating inside every repetition, device-event timings, warmed median with
the 10th / 90th percentiles.  Before timing, the two routes' outputs at the timed size are compared within
the forward test bounds.  Also printed: the bytes the algorithm must read, ``B * Tcap * (2 * Hg * D * 2 +
4)``, over the decode time, next to a device copy of as many bytes.  One JSON line per shape.

Every shape also runs over an fp8 cache (csrc/flash_decode8.hip; ``decode_fp8``, in the same repetitions):
the same values quantised by ``AttnCache.append``, its bytes ``B * Tcap * (2 * Hg * D + 8 * Hg + 4)``, and
its output against the bf16-cache decode (the quantisation error of this input).  Last, ``cache_quant`` at
n = 25000 and n = 1 rows beside a device copy of the bytes it reads.

    python benchmarks/bench_decode.py [--reps 40] [--warmup 10]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fns, reps, warmup):
    """{name: [ms]}: the callables run in turn inside every repetition, an event pair around each."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for k in fns}
    for r in range(reps):
        for k, f in fns.items():
            ev[k][r][0].record()
            f()
            ev[k][r][1].record()
    torch.cuda.synchronize()
    return {k: [a.elapsed_time(b) for a, b in v] for k, v in ev.items()}


def _stats(ms):
    q = statistics.quantiles(ms, n=10)
    return {"median_ms": round(statistics.median(ms), 4), "p10_ms": round(q[0], 4), "p90_ms": round(q[-1], 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode: needs a GPU")
    import xdot
    from xdot.ops import flash
    from xdot.parallel._ref import decode_mask

    dev, dt, B, H, D = torch.device("cuda", 0), torch.bfloat16, 1, 8, 96
    scale = 1.0 / math.sqrt(D)
    print(json.dumps({"device": torch.cuda.get_device_name(dev), "dtype": "bf16", "B": B, "H": H, "D": D,
                      "reps": a.reps, "warmup": a.warmup}), flush=True)
    for Tcap in (25000, 200000):
        for Hg in (8, 2):
            for Rn in (1, 4):
                g = torch.Generator().manual_seed(Tcap + Hg + Rn)
                rows = torch.randn(B, Rn, H * D, generator=g).to(dev, dt)
                qv = torch.randn(B, Tcap, 2 * Hg * D, generator=g).to(dev, dt)
                qc, vc = qv[..., :Hg * D], qv[..., Hg * D:]
                pos = torch.arange(Tcap, dtype=torch.int32, device=dev).repeat(B, 1)  # a full cache, in order
                pos0 = Tcap - Rn
                nbytes = B * Tcap * (2 * Hg * D * 2 + 4)
                c8 = xdot.AttnCache(B, Tcap, Hg, D, dt, device=dev, cache_dtype="fp8")
                c8.append(qv, 0)
                nbytes8 = B * Tcap * (2 * Hg * D + 8 * Hg + 4)
                src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                dst = torch.empty_like(src)

                def pack():
                    return flash.prepare_mask(decode_mask(pos, pos0, Rn), B, Rn, Tcap)

                mk = pack()
                fns = {"decode": lambda: flash.decode(rows, qc, vc, pos, pos0, H, scale, Hg=Hg),
                       "decode_fp8": lambda: flash.decode(rows, c8.q, c8.v, pos, pos0, H, scale, Hg=Hg, qscale=c8.qscale,
                                                          vscale=c8.vscale),
                       "fwd": lambda: flash.fwd(rows, qc, vc, mk, H, scale, Hg=Hg if Hg != H else None),
                       "mask_pack": pack, "copy": lambda: dst.copy_(src)}
                (o1, l1), (o2, l2) = fns["decode"](), fns["fwd"]()
                fro = ((o1.float() - o2.float()).norm() / o2.float().norm()).item()
                dl = (l1 - l2).abs().max().item()
                assert fro <= 1e-2 and dl < 1e-2, f"routes disagree at Tcap={Tcap} Hg={Hg} Rn={Rn}: {fro:.3e}, {dl:.3e}"
                o8, l8 = fns["decode_fp8"]()
                q8 = ((o8.float() - o1.float()).norm() / o1.float().norm()).item()
                t = {k: _stats(v) for k, v in _timed(fns, a.reps, a.warmup).items()}
                print(json.dumps({
                    "Tcap": Tcap, "Hg": Hg, "Rn": Rn, "spans": flash.decode_plan(B, Hg, H // Hg, Rn, Tcap),
                    "routes_rel_fro": round(fro, 6), "routes_lse_diff": round(dl, 6), **t,
                    "speedup_vs_fwd": round(t["fwd"]["median_ms"] / t["decode"]["median_ms"], 2),
                    "speedup_vs_fwd_and_pack": round((t["fwd"]["median_ms"] + t["mask_pack"]["median_ms"]) / t["decode"]["median_ms"], 2),
                    "decode_TBps": round(nbytes / t["decode"]["median_ms"] / 1e9, 3),
                    "spans_fp8": flash.decode_plan(B, Hg, H // Hg, Rn, Tcap, fp8_head_dim=D),
                    "fp8_vs_bf16_cache_rel_fro": round(q8, 6), "fp8_vs_bf16_cache_lse_diff": round((l8 - l1).abs().max().item(), 6),
                    "speedup_fp8_vs_bf16_cache": round(t["decode"]["median_ms"] / t["decode_fp8"]["median_ms"], 2),
                    "decode_fp8_TBps": round(nbytes8 / t["decode_fp8"]["median_ms"] / 1e9, 3),
                    "copy_read_TBps": round(nbytes / t["copy"]["median_ms"] / 1e9, 3)}), flush=True)
    Hg = 8
    for n in (25000, 1):
        x = torch.randn(B, n, 2 * Hg * D, generator=torch.Generator().manual_seed(n)).to(dev, dt)
        c8 = xdot.AttnCache(B, n, Hg, D, dt, device=dev, cache_dtype="fp8")
        dst = torch.empty_like(x)
        t = {k: _stats(v) for k, v in _timed({"cache_quant": lambda: torch.ops.xdot.cache_quant(x, c8.qv, c8.scales, 0, Hg),
                                              "copy": lambda: dst.copy_(x)}, a.reps, a.warmup).items()}
        print(json.dumps({"cache_quant_rows": n, "Hg": Hg, "read_bytes": x.numel() * 2, **t,
                          "cache_quant_read_TBps": round(x.numel() * 2 / t["cache_quant"]["median_ms"] / 1e9, 3),
                          "copy_read_TBps": round(x.numel() * 2 / t["copy"]["median_ms"] / 1e9, 3)}), flush=True)


if __name__ == "__main__":
    main()
