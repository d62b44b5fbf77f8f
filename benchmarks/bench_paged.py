"""Paged decode A/B on one GPU: ``flash.decode_paged`` (csrc/flash_paged.hip) against the dense decode kernel
(csrc/flash_decode.hip) over the same content.

(a) One sequence of 200 000 / 25 000 slots, one new row: the paged kernel at page sizes 32 and 128 (pages
    placed by a random permutation of the pool) against ``flash.decode`` over the dense cache; ms and TB/s of
    the cache bytes ``slots * (2 * Hg * D * 2 + 4)``.
(b) A ragged batch of 8 sequences with lengths spread 1 : 16 (2048 .. 32768 slots), one new row each: the paged
    kernel (page size 128) against a dense ``AttnCache`` layout of capacity = the longest (shorter sequences
    padded with empty slots), and against the gather-to-dense route that calls outside the kernel take; and the
    bytes of the pool against those of the dense cache, as arithmetic.

One process, the variants alternating inside every repetition, device-event timings, warmed median with the
10th / 90th percentiles.  Before timing, the variants' outputs are compared within the decode test bounds.
bf16, H = 8, D = 96, Hg = 8 and 2.  One JSON line per shape.

    python benchmarks/bench_paged.py [--reps 40] [--warmup 10]
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from benchmarks.bench_decode import _stats, _timed  # noqa: E402


def _paged(qv, pos, S, gen):
    """One sequence ``qv`` (T, C) / ``pos`` (T,) in pages of ``S`` slots placed by a random permutation ->
    (pool (P, S, C), pool_pos (P, S), table (1, P))."""
    T, C = qv.shape
    P = (T + S - 1) // S
    perm = torch.randperm(P, generator=gen, device=qv.device)
    pool, ppos = qv.new_zeros(P * S, C), pos.new_full((P * S,), -1)
    pool[:T], ppos[:T] = qv, pos
    phys, ppos_phys = torch.empty_like(pool).view(P, S, C), torch.empty_like(ppos).view(P, S)
    phys[perm], ppos_phys[perm] = pool.view(P, S, C), ppos.view(P, S)
    return phys, ppos_phys, perm.to(torch.int32).view(1, P)


def _same(a, b, what):
    fro = ((a[0].float() - b[0].float()).norm() / b[0].float().norm()).item()
    dl = (a[1] - b[1]).abs().max().item()
    assert fro <= 1e-2 and dl < 1e-2, f"{what}: outputs differ, {fro:.3e}, {dl:.3e}"
    return round(fro, 6)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_paged: needs a GPU")
    from xdot.ops import flash

    dev, dt, H, D, Rn = torch.device("cuda", 0), torch.bfloat16, 8, 96, 1
    scale, i32 = 1.0 / math.sqrt(D), dict(dtype=torch.int32, device=dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    print(json.dumps({"device": torch.cuda.get_device_name(dev), "dtype": "bf16", "H": H, "D": D, "Rn": Rn,
                      "reps": a.reps, "warmup": a.warmup}), flush=True)
    # (a) one sequence
    for T in (200000, 25000):
        for Hg in (8, 2):
            C = 2 * Hg * D
            rows = torch.randn(1, Rn, H * D, generator=gen, device=dev).to(dt)
            qv = torch.randn(T, C, generator=gen, device=dev).to(dt)
            pos = torch.arange(T, **i32)
            fns = {"dense": lambda: flash.decode(rows, qv[None, :, :Hg * D], qv[None, :, Hg * D:], pos[None], T - Rn, H, scale, Hg=Hg)}
            spans, np_, p0 = {}, {}, torch.tensor([T - Rn], **i32)
            for S in (32, 128):
                pool, ppos, table = _paged(qv, pos, S, gen)
                np_[S] = torch.tensor([table.shape[1]], **i32)
                spans[S] = flash.decode_paged_plan(1, Hg, H // Hg, Rn, table.shape[1], S)
                fns[f"paged{S}"] = (lambda pool=pool, ppos=ppos, table=table, n=np_[S]: flash.decode_paged(
                    rows, pool[..., :Hg * D], pool[..., Hg * D:], ppos, table, n, p0, H, scale, Hg=Hg))
            ref = fns["dense"]()
            fro = {k: _same(f(), ref, f"T={T} Hg={Hg} {k}") for k, f in fns.items() if k != "dense"}
            t = {k: _stats(v) for k, v in _timed(fns, a.reps, a.warmup).items()}
            nbytes = T * (C * 2 + 4)
            print(json.dumps({"case": "one_sequence", "slots": T, "Hg": Hg, "cache_bytes": nbytes,
                              "spans_dense": flash.decode_plan(1, Hg, H // Hg, Rn, T), "spans_paged": spans, "rel_fro_vs_dense": fro,
                              **t, **{f"{k}_TBps": round(nbytes / v["median_ms"] / 1e9, 3) for k, v in t.items()},
                              **{f"{k}_vs_dense": round(t["dense"]["median_ms"] / v["median_ms"], 3) for k, v in t.items() if k != "dense"}}),
                  flush=True)
            del fns, pool, ppos, qv
    # (b) a ragged batch
    B, S, Lmax = 8, 128, 32768
    lens = [Lmax * (1 + 15 * b // (B - 1)) // 16 for b in range(B)]
    for Hg in (8, 2):
        C = 2 * Hg * D
        rows = torch.randn(B, Rn, H * D, generator=gen, device=dev).to(dt)
        npg = [(n + S - 1) // S for n in lens]
        P = sum(npg)
        perm = torch.randperm(P, generator=gen, device=dev)
        pool = torch.randn(P, S, C, generator=gen, device=dev).to(dt)
        ppos, table = torch.full((P, S), -1, **i32), torch.full((B, max(npg)), -1, **i32)
        dense, dpos, at = torch.zeros(B, Lmax, C, device=dev, dtype=dt), torch.full((B, Lmax), -1, **i32), 0
        for b, n in enumerate(lens):
            pg = perm[at:at + npg[b]]
            at += npg[b]
            table[b, :npg[b]] = pg.to(torch.int32)
            p = torch.full((npg[b] * S,), -1, **i32)
            p[:n] = torch.arange(n, **i32)
            ppos[pg] = p.view(npg[b], S)
            dense[b, :n] = pool[pg].reshape(-1, C)[:n]
            dpos[b, :n] = torch.arange(Lmax - n, Lmax, **i32)   # every sequence ends at Lmax - 1: one pos0 for the batch
        npages, pos0 = torch.tensor(npg, **i32), torch.tensor([n - Rn for n in lens], **i32)
        pq, pv = pool[..., :Hg * D], pool[..., Hg * D:]
        fns = {"paged": lambda: flash.decode_paged(rows, pq, pv, ppos, table, npages, pos0, H, scale, Hg=Hg),
               "dense_padded": lambda: flash.decode(rows, dense[..., :Hg * D], dense[..., Hg * D:], dpos, Lmax - Rn, H, scale, Hg=Hg),
               "gather_to_dense": lambda: flash._decode_paged_gathered(rows, pq, pv, ppos, table, npages, pos0, H, scale, Hg=Hg)}
        ref = fns["dense_padded"]()
        fro = {k: _same(f(), ref, f"ragged Hg={Hg} {k}") for k, f in fns.items() if k != "dense_padded"}
        t = {k: _stats(v) for k, v in _timed(fns, a.reps, a.warmup).items()}
        live = sum(lens) * (C * 2 + 4)
        print(json.dumps({"case": "ragged_batch", "lens": lens, "Hg": Hg, "page_size": S, "live_cache_bytes": live,
                          "pool_bytes": P * S * (C * 2 + 4), "dense_bytes": B * Lmax * (C * 2 + 4),
                          "spans_paged": flash.decode_paged_plan(B, Hg, H // Hg, Rn, max(npg), S),
                          "spans_dense": flash.decode_plan(B, Hg, H // Hg, Rn, Lmax), "rel_fro_vs_dense_padded": fro, **t,
                          "paged_live_TBps": round(live / t["paged"]["median_ms"] / 1e9, 3),
                          **{f"paged_vs_{k}": round(v["median_ms"] / t["paged"]["median_ms"], 3) for k, v in t.items() if k != "paged"}}),
              flush=True)


if __name__ == "__main__":
    main()
