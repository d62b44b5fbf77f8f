"""Decode against a sharded cache on the CPU (the torch path): prefill then decode equals the module's
full causal forward, in fp64."""
import copy

import pytest
import torch

import xdot
from xdot.parallel.layout import row_runs


def _module():
    torch.manual_seed(0)
    m = xdot.DistributedDotProductAttn(64, num_heads=4, num_gathered_heads=2, distributed=False, rope=xdot.Rotary(),
                                       qk_norm=True, sinks=True, gate="headwise", add_bias=True).double()
    with torch.no_grad():
        m.sinks.copy_(torch.linspace(-1.0, 1.0, 4))
        m.keys_norm.weight.copy_(torch.linspace(0.5, 1.5, 16))
    return m


@pytest.mark.parametrize("ws", [1, 2, 3])
@pytest.mark.parametrize("layout", ["contiguous", "zigzag"])
@pytest.mark.parametrize("window", [None, 40])
def test_prefill_then_decode_equals_full_forward(ws, layout, window):
    ref = _module()
    T0, new = 96, 5  # 3 single tokens, then 2 rows at once
    x = torch.randn(1, T0 + new, 64, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    full = ref(x, x, x, xdot.StructuredMask(causal=True, window=window, row_offset=0))

    def rank_fn(rank):
        m = copy.deepcopy(ref)  # (seeding inside the rank threads would race on the global generator)
        m.distributed = ws > 1
        cache = m.new_cache(1, T0 // ws + new)
        for _ls, ln, gs in row_runs(layout, rank, ws, T0 // ws):
            m.cache_append(cache, x[:, gs:gs + ln], x[:, gs:gs + ln], gs)
        outs = []
        for step, (p, n) in enumerate([(T0, 1), (T0 + 1, 1), (T0 + 2, 1), (T0 + 3, 2)]):
            if step % ws == rank:
                m.cache_append(cache, x[:, p:p + n], x[:, p:p + n], torch.arange(p, p + n))
            outs.append(m.decode(x[:, p:p + n], cache, p, window=window))
        return torch.cat(outs, dim=1)

    for out in (xdot.ThreadGroup(ws).run(rank_fn) if ws > 1 else [rank_fn(0)]):
        assert (out - full[:, T0:]).abs().max().item() <= 1e-12


def test_append_past_capacity_raises():
    cache = xdot.AttnCache(1, 4, 2, 16, torch.float64)
    cache.append(torch.zeros(1, 3, 64, dtype=torch.float64), 0)
    with pytest.raises(RuntimeError, match="do not fit"):
        cache.append(torch.zeros(1, 2, 64, dtype=torch.float64), 3)
    assert cache.fill == 3 and cache.pos[0].tolist() == [0, 1, 2, -1]


def test_empty_cache_with_sinks_gives_zero():
    rows = torch.randn(2, 3, 64, dtype=torch.float64)
    out, lse = xdot.decode_attention(rows, xdot.AttnCache(2, 8, 2, 16, torch.float64), 5, num_heads=4, scale=0.25,
                                     sinks=torch.tensor([0.0, 1.0, -1.0, 2.0]), comm=xdot.LocalComm())
    assert out.eq(0).all() and torch.equal(lse[0, :, 0], torch.tensor([0.0, 1.0, -1.0, 2.0], dtype=torch.float64))
