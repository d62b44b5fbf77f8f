"""Paged fp8 decode A/B on one GPU: ``flash.decode_paged`` over an fp8 pool (csrc/flash_paged8.hip) against (a)
the 16-bit paged kernel (csrc/flash_paged.hip) on the same logical content, (b) the dense fp8 kernel
(csrc/flash_decode8.hip), (c) the gather-to-dense-fp8 route; and the quantising scatter append against a
``cache_quant`` into a staging buffer plus index copies.

one_sequence   200 000 / 25 000 slots, one new row, page sizes 32 and 128 (pages placed by a random permutation):
               paged fp8 against paged 16-bit and dense fp8; ms and TB/s of each variant's own cache bytes.
ragged_batch   8 sequences with lengths spread 1 : 16 (2048 .. 32768 slots), one new row each, page size 128: paged
               fp8 against paged 16-bit and the gather route.
append         1 row x 8 sequences and a 2048-row prefill into a pool of 2048 pages of 128 slots: one
               ``cache_quant_paged`` launch against ``cache_quant`` into a staging buffer, an ``index_copy_`` of the
               bytes, an indexed write of the scales and an ``index_copy_`` of the positions.

One process, the variants alternating inside every repetition, device-event timings, warmed median with the 10th /
90th percentiles.  Before timing, the fp8 variants' outputs are compared within the decode test bounds, and the
two appends bitwise.  bf16, H = 8, D = 96, Hg = 8 and 2.  One JSON line per shape.

    python benchmarks/bench_paged_fp8.py [--reps 40] [--warmup 10]
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from benchmarks.bench_decode import _stats, _timed  # noqa: E402
from benchmarks.bench_paged import _same  # noqa: E402

F8 = torch.float8_e4m3fn


def _place(x, S, perm, fill):
    """``x`` (T, ...) padded with ``fill`` to whole pages of ``S`` slots, logical page i at physical ``perm[i]``."""
    P = perm.numel()
    flat = x.new_full((P * S, *x.shape[1:]), fill)
    flat[:x.shape[0]] = x
    out = torch.empty_like(flat).view(P, S, *x.shape[1:])
    out[perm] = flat.view(P, S, *x.shape[1:])
    return out


def _pools(qv, pos, S, perm, Hg):
    """The 16-bit pool and the fp8 pool (bytes, scales (P, 2*Hg, S)) of one content, and pool_pos."""
    from xdot.parallel import _ref

    b8, s = _ref.cache_quant(qv, Hg)
    return (_place(qv, S, perm, 0), _place(b8.view(torch.uint8), S, perm, 0).view(F8),
            _place(s, S, perm, 1).transpose(1, 2).contiguous(), _place(pos, S, perm, -1))


def _rates(t, nbytes):
    return {f"{k}_TBps": round(nbytes[k] / v["median_ms"] / 1e9, 3) for k, v in t.items() if k in nbytes}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_paged_fp8: needs a GPU")
    from xdot import _ext
    from xdot.ops import flash
    from xdot.parallel import _ref

    dev, dt, H, D, Rn = torch.device("cuda", 0), torch.bfloat16, 8, 96, 1
    scale, i32 = 1.0 / math.sqrt(D), dict(dtype=torch.int32, device=dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    print(json.dumps({"device": torch.cuda.get_device_name(dev), "dtype": "bf16", "H": H, "D": D, "Rn": Rn,
                      "reps": a.reps, "warmup": a.warmup}), flush=True)
    for T in (200000, 25000):
        for Hg in (8, 2):
            C, w = 2 * Hg * D, Hg * D
            b16, b8 = T * (C * 2 + 4), T * (C + 8 * Hg + 4)   # cache bytes per format: slots, scales, positions
            rows = torch.randn(1, Rn, H * D, generator=gen, device=dev).to(dt)
            qv = torch.randn(T, C, generator=gen, device=dev).to(dt)
            pos, p0 = torch.arange(T, **i32), torch.tensor([T - Rn], **i32)
            d8, ds = _ref.cache_quant(qv[None], Hg)
            ds = ds.transpose(1, 2).contiguous()
            fns = {"dense8": lambda: flash.decode(rows, d8[..., :w], d8[..., w:], pos[None], T - Rn, H, scale, Hg=Hg,
                                                  qscale=ds[:, :Hg], vscale=ds[:, Hg:])}
            spans, nbytes = {}, {"dense8": b8}
            for S in (32, 128):
                P = (T + S - 1) // S
                perm = torch.randperm(P, generator=gen, device=dev)
                p16, p8, sc, ppos = _pools(qv, pos, S, perm, Hg)
                table, n = perm.to(torch.int32).view(1, P), torch.tensor([P], **i32)
                spans[S] = flash.decode_paged_plan(1, Hg, H // Hg, Rn, P, S, fp8_head_dim=D)
                fns[f"paged8_{S}"] = (lambda p8=p8, sc=sc, ppos=ppos, table=table, n=n: flash.decode_paged(
                    rows, p8[..., :w], p8[..., w:], ppos, table, n, p0, H, scale, Hg=Hg, qscale=sc[:, :Hg], vscale=sc[:, Hg:]))
                fns[f"paged16_{S}"] = (lambda p16=p16, ppos=ppos, table=table, n=n: flash.decode_paged(
                    rows, p16[..., :w], p16[..., w:], ppos, table, n, p0, H, scale, Hg=Hg))
                nbytes[f"paged8_{S}"], nbytes[f"paged16_{S}"] = b8, b16
            ref = fns["dense8"]()
            fro = {k: _same(f(), ref, f"T={T} Hg={Hg} {k}") for k, f in fns.items() if k.startswith("paged8")}
            t = {k: _stats(v) for k, v in _timed(fns, a.reps, a.warmup).items()}
            ms = {k: v["median_ms"] for k, v in t.items()}
            print(json.dumps({"case": "one_sequence", "slots": T, "Hg": Hg, "bytes_fp8": b8, "bytes_16": b16, "spans_paged8": spans,
                              "spans_dense8": flash.decode_plan(1, Hg, H // Hg, Rn, T, fp8_head_dim=D), "rel_fro_vs_dense8": fro,
                              **t, **_rates(t, nbytes),
                              **{f"paged8_{S}_vs_paged16": round(ms[f"paged16_{S}"] / ms[f"paged8_{S}"], 3) for S in (32, 128)},
                              **{f"paged8_{S}_vs_dense8": round(ms["dense8"] / ms[f"paged8_{S}"], 3) for S in (32, 128)}}), flush=True)
            del fns, p16, p8, qv, d8
    B, S, Lmax = 8, 128, 32768
    lens = [Lmax * (1 + 15 * b // (B - 1)) // 16 for b in range(B)]
    npg = [(n + S - 1) // S for n in lens]
    P = sum(npg)
    for Hg in (8, 2):
        C, w = 2 * Hg * D, Hg * D
        rows = torch.randn(B, Rn, H * D, generator=gen, device=dev).to(dt)
        perm = torch.randperm(P, generator=gen, device=dev)
        p16 = torch.randn(P, S, C, generator=gen, device=dev).to(dt)
        p8, sc = _ref.cache_quant(p16, Hg)
        sc = sc.transpose(1, 2).contiguous()
        ppos, table, at = torch.full((P, S), -1, **i32), torch.full((B, max(npg)), -1, **i32), 0
        for b, n in enumerate(lens):
            pg = perm[at:at + npg[b]]
            at += npg[b]
            table[b, :npg[b]] = pg.to(torch.int32)
            p = torch.full((npg[b] * S,), -1, **i32)
            p[:n] = torch.arange(n, **i32)
            ppos[pg] = p.view(npg[b], S)
        npages, pos0 = torch.tensor(npg, **i32), torch.tensor([n - Rn for n in lens], **i32)
        kw = dict(Hg=Hg, qscale=sc[:, :Hg], vscale=sc[:, Hg:])
        fns = {"paged8": lambda: flash.decode_paged(rows, p8[..., :w], p8[..., w:], ppos, table, npages, pos0, H, scale, **kw),
               "paged16": lambda: flash.decode_paged(rows, p16[..., :w], p16[..., w:], ppos, table, npages, pos0, H, scale, Hg=Hg),
               "gather_to_dense8": lambda: flash._decode_paged_gathered(rows, p8[..., :w], p8[..., w:], ppos, table, npages, pos0, H,
                                                                        scale, **kw)}
        fro = _same(fns["paged8"](), fns["gather_to_dense8"](), f"ragged Hg={Hg}")
        t = {k: _stats(v) for k, v in _timed(fns, a.reps, a.warmup).items()}
        live8, live16 = sum(lens) * (C + 8 * Hg + 4), sum(lens) * (C * 2 + 4)
        print(json.dumps({"case": "ragged_batch", "lens": lens, "Hg": Hg, "page_size": S, "live_bytes_fp8": live8, "live_bytes_16": live16,
                          "spans_paged8": flash.decode_paged_plan(B, Hg, H // Hg, Rn, max(npg), S, fp8_head_dim=D),
                          "spans_paged16": flash.decode_paged_plan(B, Hg, H // Hg, Rn, max(npg), S), "rel_fro_vs_gather": fro, **t,
                          **_rates(t, {"paged8": live8, "paged16": live16}),
                          **{f"paged8_vs_{k}": round(v["median_ms"] / t["paged8"]["median_ms"], 3) for k, v in t.items() if k != "paged8"}}),
              flush=True)
    # the append: N rows into a pool of 2048 pages of 128 slots
    ops, P, S = _ext.ops(), 2048, 128
    for Hg in (8, 2):
        C = 2 * Hg * D
        for what, N in (("1_row_x_8_sequences", 8), ("prefill_2048_rows", 2048)):
            rows = torch.randn(N, C, generator=gen, device=dev).to(dt)
            if N == 8:   # the next slot of 8 sequences, each in a page of its own
                slots = torch.randperm(P, generator=gen, device=dev)[:N] * S + torch.randint(0, S, (N,), generator=gen, device=dev)
            else:        # 16 whole pages
                slots = (torch.randperm(P, generator=gen, device=dev)[:N // S].view(-1, 1) * S + torch.arange(S, device=dev)).reshape(-1)
            s32, p32 = slots.to(torch.int32), torch.arange(N, **i32)
            pools = [(torch.zeros(P, S, C, device=dev, dtype=F8), torch.ones(P, 2 * Hg, S, device=dev), torch.full((P, S), -1, **i32))
                     for _ in range(2)]
            st8, sts = torch.zeros(1, N, C, device=dev, dtype=F8), torch.ones(1, 2 * Hg, N, device=dev)

            def scatter(qv=pools[0][0], sc=pools[0][1], pp=pools[0][2]):
                ops.cache_quant_paged(rows, qv, sc, pp, s32, p32, Hg)

            def staged(qv=pools[1][0], sc=pools[1][1], pp=pools[1][2]):
                ops.cache_quant(rows[None], st8, sts, 0, Hg)
                qv.view(torch.uint8).view(-1, C).index_copy_(0, slots, st8.view(torch.uint8)[0])
                sc[slots // S, :, slots % S] = sts[0].t()
                pp.view(-1).index_copy_(0, slots, p32)

            scatter(), staged()
            assert all(torch.equal(x.view(torch.uint8) if x.dtype == F8 else x, y.view(torch.uint8) if y.dtype == F8 else y)
                       for x, y in zip(*pools)), f"append {what} Hg={Hg}: the two appends differ"
            t = {k: _stats(v) for k, v in _timed({"scatter": scatter, "staged": staged}, a.reps, a.warmup).items()}
            print(json.dumps({"case": "append", "rows": what, "Hg": Hg, **t,
                              "scatter_vs_staged": round(t["staged"]["median_ms"] / t["scatter"]["median_ms"], 3)}), flush=True)


if __name__ == "__main__":
    main()
