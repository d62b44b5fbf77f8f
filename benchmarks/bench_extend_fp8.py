"""Chunked prefill over an fp8 cache, A/B on one GPU: ``flash.extend(..., qscale=, vscale=)``
(csrc/flash_extend8.hip) against the route the same call had before it -- dequantise the whole cache into
fp32, build and pack the dense mask, run the exact-fp32 forward kernels -- timed whole (``slow``) and with the
dequantisation split out (``dequant``, and ``slow_rest`` over an already dequantised cache).  For context:
``extend16``, the 16-bit row-blocked kernel over the bf16 cache the fp8 one was quantised from.

One process, the variants alternating inside every repetition, device-event timings, warmed median with the
10th / 90th percentiles.  Before timing, the two routes' outputs at the timed size are compared within the
decode test bounds, and each route's peak extra device memory is read from the allocator.  bf16, B = 1,
H = 8, D = 96 over a full in-order cache.  ``extend8_wins``: the kernel's p10 is below the slow route's p90;
a shape class where it is not is routed away in ``flash.extend_fp8_eligible``.  One JSON line per case.

    python benchmarks/bench_extend_fp8.py [--reps 20] [--warmup 5]
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchmarks.bench_decode import _stats, _timed  # noqa: E402


def _peak_extra(fn):
    """Bytes the allocator held at most during ``fn()`` above what it held before."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tcaps", default="25000,200000")
    ap.add_argument("--rows", default="72,128,256,1024")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_extend_fp8: needs a GPU")
    import xdot
    from xdot import _ext
    from xdot.ops import flash

    dev, dt, B, H, D = torch.device("cuda", 0), torch.bfloat16, 1, 8, 96
    scale = 1.0 / math.sqrt(D)
    print(json.dumps({"device": torch.cuda.get_device_name(dev), "dtype": "bf16", "B": B, "H": H, "D": D,
                      "reps": a.reps, "warmup": a.warmup}), flush=True)
    for Tcap in (int(t) for t in a.tcaps.split(",")):
        for Hg in (8, 2):
            G, w = H // Hg, Hg * D
            g = torch.Generator(device=dev).manual_seed(Tcap + Hg)
            qv = torch.randn(B, Tcap, 2 * w, generator=g, device=dev).to(dt)
            cache = xdot.AttnCache(B, Tcap, Hg, D, dt, device=dev, cache_dtype="fp8")
            cache.append(qv, 0)  # a full cache, in order
            qc, vc, qs, vs, pos = cache.q, cache.v, cache.qscale, cache.vscale, cache.pos

            def dequant():
                return tuple((t.float().reshape(B, -1, Hg, D) * s.transpose(1, 2).unsqueeze(-1)).reshape(t.shape)
                             for t, s in ((qc, qs), (vc, vs)))

            q32, v32 = dequant()
            for window in (0, 4096):
                for Rn in (int(r) for r in a.rows.split(",")):
                    rows = torch.randn(B, Rn, H * D, generator=g, device=dev).to(dt)
                    rows32, pos0 = rows.float(), Tcap - Rn

                    def slow_rest():  # fp32 rows: flash.decode builds and packs the mask and runs the forward kernels
                        return flash.decode(rows32, q32, v32, pos, pos0, H, scale, window, Hg, out_fp32=True)

                    def slow():  # the parent commit's route of this call, written out
                        qd, vd = dequant()
                        return flash.decode(rows.float(), qd, vd, pos, pos0, H, scale, window, Hg, out_fp32=True)

                    # the ops themselves: flash.extend refuses what a routing table sends away
                    fns = {"extend8": lambda: _ext.ops().flash_extend_fp8(rows, qc, vc, qs, vs, pos, pos0, window, H, scale, Hg),
                           "slow": slow, "dequant": dequant, "slow_rest": slow_rest,
                           "extend16": lambda: _ext.ops().flash_extend(rows, qv[..., :w], qv[..., w:], pos, pos0, window, H, scale, Hg)}
                    (o1, l1), (o2, l2) = fns["extend8"](), slow()
                    fro = ((o1.float() - o2).norm() / o2.norm()).item()
                    dl = (l1 - l2).abs().max().item()
                    assert fro <= 1e-2 and dl < 1e-2, f"routes disagree at Tcap={Tcap} Hg={Hg} Rn={Rn} window={window}: {fro:.3e}, {dl:.3e}"
                    del o1, l1, o2, l2
                    mem = {k: _peak_extra(fns[k]) for k in ("extend8", "slow")}
                    t = {k: _stats(v) for k, v in _timed(fns, a.reps, a.warmup).items()}
                    print(json.dumps({
                        "Tcap": Tcap, "Hg": Hg, "Rn": Rn, "window": window,
                        "spans": flash.extend_plan(B, Hg, G, Rn, D, Tcap, fp8=True),
                        "routes_rel_fro": round(fro, 6), "routes_lse_diff": round(dl, 6), **t,
                        "peak_extra_bytes": mem,
                        "speedup_vs_slow": round(t["slow"]["median_ms"] / t["extend8"]["median_ms"], 2),
                        "speedup_vs_slow_rest": round(t["slow_rest"]["median_ms"] / t["extend8"]["median_ms"], 2),
                        "extend16_over_extend8": round(t["extend16"]["median_ms"] / t["extend8"]["median_ms"], 2),
                        "extend8_wins": t["extend8"]["p10_ms"] < t["slow"]["p90_ms"],
                        "extend8_wins_rest": t["extend8"]["p10_ms"] < t["slow_rest"]["p90_ms"],
                        "eligible": flash.extend_fp8_eligible(dt, D, D, G, Rn)}), flush=True)
            del q32, v32, cache, qv


if __name__ == "__main__":
    main()
