"""The paged cache on the host: xdot.PagedAttnCache's bookkeeping, and flash.decode_paged on CPU tensors
against ``_ref.decode`` over the equivalent dense cache of each sequence."""
import pytest
import torch

import xdot
from xdot.ops import flash
from xdot.parallel import _ref


def _dense(cache, b):
    """Sequence ``b`` as a dense cache, in append order: (qv (1, len, C), positions (1, len))."""
    S, i = cache.page_size, torch.arange(cache.lens[b])
    at = torch.tensor(cache.pages[b], dtype=torch.int64)[i // S] * S + i % S
    return cache.qv.view(-1, cache.qv.shape[-1])[at].unsqueeze(0), cache.pos.view(-1)[at].unsqueeze(0)


def test_paged_cache_bookkeeping():
    g = torch.Generator().manual_seed(0)
    c = xdot.PagedAttnCache(2, 6, 32, 2, 32, torch.float64)
    a, b1 = torch.randn(2, 40, 128, generator=g, dtype=torch.float64), torch.randn(1, 30, 128, generator=g, dtype=torch.float64)
    c.append(a, [0, 100])                       # 40 rows each: two pages per sequence, the second part-filled
    c.append_seq(1, b1, 140)                    # 70 rows: a third page for sequence 1 only
    assert [len(p) for p in c.pages] == [2, 3] and c.lens == [40, 70] and c.npages.tolist() == [2, 3]
    assert c.table[0, :2].tolist() == c.pages[0] and c.table[1, :3].tolist() == c.pages[1] and c.table[0, 2].item() == -1
    assert sorted(c.pages[0] + c.pages[1] + c.free_pages) == list(range(6))
    qv0, p0 = _dense(c, 0)
    qv1, p1 = _dense(c, 1)
    assert torch.equal(qv0, a[:1]) and p0[0].tolist() == list(range(40))
    assert torch.equal(qv1, torch.cat([a[1:], b1], 1)) and p1[0].tolist() == list(range(100, 170))
    assert (c.pos >= 0).sum().item() == 110
    with pytest.raises(RuntimeError, match="pages"):
        c.append(torch.zeros(2, 60, 128, dtype=torch.float64), 0)   # 2 + 1 pages wanted, 1 free
    assert c.lens == [40, 70] and len(c.free_pages) == 1           # a refused append changes nothing
    freed = list(c.pages[1])
    c.free(1)
    assert c.lens[1] == 0 and c.npages.tolist() == [2, 0] and (c.table[1] == -1).all() and (c.pos[freed] == -1).all()
    c.append_seq(1, b1, torch.arange(29, -1, -1))                   # the freed pages serve again
    assert c.pages[1][0] in freed and _dense(c, 1)[1][0].tolist() == list(range(29, -1, -1))


@pytest.mark.parametrize("window", [0, 50])
def test_decode_paged_cpu_matches_dense_reference(window):
    g = torch.Generator().manual_seed(1)
    H, Hg, D, Rn, lens = 4, 2, 16, 3, [70, 5, 0, 33]
    c = xdot.PagedAttnCache(4, 8, 32, Hg, D, torch.float64)
    for b in (0, 3, 1):                                             # interleaved pages
        c.append_seq(b, torch.randn(1, lens[b], 2 * Hg * D, generator=g, dtype=torch.float64), 10 * b)
    c.table[0, 1] = -1                                              # a hole: its slots are not seen
    pos0 = torch.tensor([10 * b + lens[b] - Rn for b in range(4)], dtype=torch.int32)
    pos0[1] = -1                                                    # inactive
    rows = torch.randn(4, Rn, H * D, generator=g, dtype=torch.float64)
    out, lse = flash.decode_paged(rows, c.q, c.v, c.pos, c.table, c.npages, pos0, H, 0.25, window=window, Hg=Hg)
    for b in range(4):
        qv, p = _dense(c, b)
        if b == 0:
            p[:, 32:64] = -1
        if b == 1:
            p[:] = -1
        want = _ref.decode(rows[b:b + 1], qv[..., :Hg * D], qv[..., Hg * D:], p, max(int(pos0[b]), 0), H, 0.25, window, Hg)
        assert (out[b:b + 1] - want[0]).abs().max().item() <= 1e-12 and torch.equal(torch.isinf(lse[b:b + 1]), torch.isinf(want[1]))
        assert (lse[b:b + 1] - want[1]).nan_to_num(0.0).abs().max().item() <= 1e-12
    assert torch.isinf(lse[1]).all() and torch.isinf(lse[2]).all() and torch.isfinite(lse[0]).all()
