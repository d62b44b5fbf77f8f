"""The fp8 paged pool on the CPU: the torch route of ``decode_paged`` with scales, and ``PagedAttnCache``'s fp8
bookkeeping against the dense fp8 cache."""
import pytest
import torch

from xdot.ops import flash
from xdot.parallel import _ref
from xdot.parallel.decode import AttnCache, PagedAttnCache


@pytest.mark.parametrize("window", [0, 40])
def test_ref_decode_paged_with_scales_is_dense_decode_over_the_dequantised_gather(window):
    g = torch.Generator().manual_seed(0)
    B, P, S, H, Hg, D, Rn = 2, 5, 32, 4, 2, 32, 3
    b8, sc = _ref.cache_quant((torch.randn(P, S, 2 * Hg * D, generator=g) * 3).bfloat16(), Hg)
    scales = sc.transpose(1, 2).contiguous()                       # (P, 2*Hg, S)
    ppos = torch.randperm(P * S, generator=g).view(P, S).int()
    table, npages = torch.tensor([[3, -1, 0], [4, 1, 2]], dtype=torch.int32), torch.tensor([3, 2], dtype=torch.int32)
    pos0, rows = torch.tensor([150, 90], dtype=torch.int32), torch.randn(B, Rn, H * D, generator=g).bfloat16()
    out, lse = flash.decode_paged(rows, b8[..., :Hg * D], b8[..., Hg * D:], ppos, table, npages, pos0, H, 0.2, window, Hg=Hg,
                                  qscale=scales[:, :Hg], vscale=scales[:, Hg:], out_fp32=True)
    qv = _ref.cache_dequant(b8, sc, Hg, torch.float32)
    qc, vc, pos = _ref.paged_gather(qv[..., :Hg * D], qv[..., Hg * D:], ppos, table, npages)
    for b in range(B):
        o, l = _ref.decode(rows[b:b + 1], qc[b:b + 1], vc[b:b + 1], pos[b:b + 1], int(pos0[b]), H, 0.2, window, Hg)
        assert torch.equal(out[b:b + 1], o) and torch.equal(lse[b:b + 1], l)


def test_paged_fp8_cache_keeps_the_dense_fp8_cache_contents():
    """The same appends into a paged and, per sequence, a dense fp8 cache; then a free and a reuse of the pages."""
    g = torch.Generator().manual_seed(1)
    Hg, D, S = 2, 32, 32
    C = 2 * Hg * D
    paged, dense = PagedAttnCache(2, 4, S, Hg, D, torch.bfloat16, cache_dtype="fp8"), {}

    def put(key, b, n, p):
        x = (torch.randn(1, n, C, generator=g) * 5).bfloat16()
        paged.append_seq(b, x, p)
        dense.setdefault(key, AttnCache(1, 128, Hg, D, torch.bfloat16, cache_dtype="fp8")).append(x, p)

    def same(key, b):
        d, n = dense[key], dense[key].fill
        i = torch.arange(n)
        pg, sl = torch.tensor(paged.pages[b])[i // S], i % S
        assert paged.lens[b] == n and torch.equal(paged.qv.view(torch.uint8)[pg, sl], d.qv.view(torch.uint8)[0, :n])
        assert torch.equal(paged.scales[pg, :, sl], d.scales[0, :, :n].t()) and torch.equal(paged.pos[pg, sl], d.pos[0, :n])
        q, v = paged.dequant()
        assert torch.equal(q[pg, sl], d.dequant()[0][0, :n]) and torch.equal(v[pg, sl], d.dequant()[1][0, :n])

    put("a", 0, 40, 0), put("b", 1, 33, 7), put("a", 0, 1, 40)
    both = (torch.randn(2, 1, C, generator=g) * 5).bfloat16()
    paged.append(both, [41, 40])
    dense["a"].append(both[:1], 41), dense["b"].append(both[1:], 40)
    same("a", 0), same("b", 1)
    assert not paged.free_pages
    freed = paged.pages[0]
    paged.free(0)
    assert (paged.pos[freed] == -1).all() and paged.scales.isfinite().all() and paged.free_pages == freed[::-1]
    put("c", 0, 50, 3)
    same("c", 0), same("b", 1)
    assert paged.pages[0] == freed
